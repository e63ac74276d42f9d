"""Performance record of the marching-tets engine (csrc/dmtet.hip through diffsound_amd/dmtet.py).

For each grid - DMTet's 32 and 64 grids (``--grid PATH``, the data/tets/{res}_tets.npz files, repeatable) and
kuhn_grid(96) / kuhn_grid(128) - on a bumpy-sphere SDF: forward and forward+backward of the native engine and of a
torch formulation of the same algorithm (boolean masks, torch.unique of the valid tets' edges, torch.unique of the
output tets' vertices - what the reference's DMTet.__call__ does), both on the device, median of ``--reps`` timed calls
(device events) after one warm-up call.

Bytes of a native forward (the compulsory traffic, counted from the kernels): the flags pass reads tets (16 T), the
edge list (8 E), vptr and sdf (8 n) and writes the per-tet counts (20 T), flags (4 E + 4 n); the three scans read and
write those (40 T + 8 E + 8 n); the emit pass reads tets, tet_edge, offsets, ids (16 T + 24 T + 20 T + 8 E + 8 n +
12 n) and writes the outputs (12 per vertex, 32 per tet).  Quoted against the in-run STREAM triad.

Then one real shape-loop iteration on the 32 grid (DMTetGeometry.getMesh -> largest connected component ->
DiffSoundObj(mode_num=16) -> eigen_decomposition -> get_vals -> backward -> Adam), wall clock with a device
synchronisation at the end, and the DMTet share: the time of getMesh (MLP + marching tets) and of the connected
component.  Writes one JSON document (``--out``, default stdout)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

EDGES = [[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [2, 3]]
SPLIT = {1: [[0, 4, 5, 6]], 2: [[1, 4, 8, 7]], 4: [[2, 5, 7, 9]], 8: [[3, 6, 9, 8]],
         3: [[7, 1, 8, 6], [5, 1, 7, 6], [5, 0, 1, 6]], 5: [[4, 0, 6, 7], [9, 0, 7, 6], [7, 0, 9, 2]],
         6: [[4, 1, 9, 8], [5, 1, 9, 4], [5, 1, 2, 9]], 7: [[6, 0, 1, 2], [8, 6, 1, 2], [9, 6, 8, 2]],
         9: [[5, 0, 4, 8], [5, 0, 8, 3], [5, 8, 9, 3]], 10: [[1, 4, 7, 3], [4, 7, 6, 3], [9, 6, 7, 3]],
         11: [[0, 1, 5, 3], [5, 1, 9, 3], [5, 1, 7, 9]], 12: [[5, 2, 3, 7], [3, 6, 5, 8], [3, 5, 7, 8]],
         13: [[0, 4, 7, 8], [0, 3, 8, 7], [0, 3, 7, 2]], 14: [[4, 1, 2, 3], [4, 3, 2, 5], [4, 3, 5, 6]]}


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def stream_triad_gbs(reps):
    from diffsound_amd import _hip

    n = 64 << 20
    a, b, c = (torch.empty(n, device="cuda") for _ in range(3))
    b.fill_(1.0), c.fill_(2.0)
    ms = timed(lambda: _hip.check(_hip.lib().ds_stream_triad(a.data_ptr(), b.data_ptr(), c.data_ptr(), n, 3.0,
                                                            _hip.stream_ptr()), "ds_stream_triad"), reps)
    return 3 * n * 4 / ms / 1e6


class TorchMarchingTets:
    """The reference algorithm as plain torch ops (masks, unique, gathers); autograd through the interpolation."""

    def __init__(self, dev):
        self.edges = torch.tensor(EDGES, device=dev).reshape(-1)
        tab = torch.full((16, 12), -1, dtype=torch.long)
        ntet = torch.zeros(16, dtype=torch.long)
        for c, rows in SPLIT.items():
            flat = [i for r in rows for i in r]
            tab[c, :len(flat)] = torch.tensor(flat)
            ntet[c] = len(rows)
        self.tab, self.ntet = tab.to(dev), ntet.to(dev)
        self.bits = torch.tensor([1, 2, 4, 8], device=dev)

    def __call__(self, pos, sdf, tets):
        with torch.no_grad():
            inside = sdf > 0
            occ = inside[tets]
            cnt = occ.sum(1)
            valid = (cnt > 0) & (cnt < 4)
            vt = tets[valid]
            e = vt[:, self.edges].reshape(-1, 2).sort(dim=1)[0]
            ue, inv = torch.unique(e, dim=0, return_inverse=True)
            cross = inside[ue].sum(1) == 1
            num = torch.full((ue.shape[0],), -1, dtype=torch.long, device=pos.device)
            num[cross] = torch.arange(int(cross.sum()), device=pos.device)
            eid = num[inv].reshape(-1, 6)
            xe = ue[cross]
        sa, sb = sdf[xe[:, 0]], sdf[xe[:, 1]]
        d = sa - sb
        verts = pos[xe[:, 0]] * (-sb / d)[:, None] + pos[xe[:, 1]] * (sa / d)[:, None]
        with torch.no_grad():
            cls = (occ[valid] * self.bits).sum(1)
            local = torch.cat([vt, eid + pos.shape[0]], dim=1)
            nt = self.ntet[cls]
            one = torch.gather(local[nt == 1], 1, self.tab[cls[nt == 1]][:, :4]).reshape(-1, 4)
            three = torch.gather(local[nt == 3], 1, self.tab[cls[nt == 3]][:, :12]).reshape(-1, 4)
            all_tets = torch.cat([one, three, tets[cnt == 4]])
            used, t_out = torch.unique(all_tets.reshape(-1), return_inverse=True)
        return torch.cat([pos, verts])[used], t_out.reshape(-1, 4)


def bumpy_sphere(v):
    r = np.linalg.norm(v, axis=1)
    return (0.35 - r + 0.04 * np.sin(9 * v[:, 0]) * np.cos(7 * v[:, 1]) + 0.03 * np.sin(11 * v[:, 2])).astype(np.float32)


def measure_grid(name, v_np, t_np, reps, torch_mt):
    from diffsound_amd.dmtet import grid_tables, marching_tets

    dev = torch.device("cuda")
    pos = torch.from_numpy(v_np).to(dev).requires_grad_(True)
    sdf = torch.from_numpy(bumpy_sphere(v_np)).to(dev).requires_grad_(True)
    tets = torch.from_numpy(t_np.astype(np.int64)).to(dev)
    t0 = time.perf_counter()
    tab = grid_tables(tets, pos.shape[0])
    torch.cuda.synchronize()
    tables_ms = (time.perf_counter() - t0) * 1e3
    out = {}

    def fwd():
        out["v"], out["t"] = marching_tets(pos, sdf, tets)

    def fwd_bwd():
        v, _ = marching_tets(pos, sdf, tets)
        v.sum().backward()

    def tfwd():
        out["tv"], out["tt"] = torch_mt(pos, sdf, tets)

    def tfwd_bwd():
        v, _ = torch_mt(pos, sdf, tets)
        v.sum().backward()

    rec = dict(grid=name, n=int(pos.shape[0]), T=tab.T, E=tab.E, tables_ms_once=tables_ms)
    rec["native_fwd_ms"] = timed(fwd, reps)
    rec["native_fwd_bwd_ms"] = timed(fwd_bwd, reps)
    rec["torch_fwd_ms"] = timed(tfwd, reps)
    rec["torch_fwd_bwd_ms"] = timed(tfwd_bwd, reps)
    rec["out_verts"], rec["out_tets"] = int(out["v"].shape[0]), int(out["t"].shape[0])
    rec["same_as_torch"] = bool(torch.equal(out["t"], out["tt"]) and torch.equal(out["v"], out["tv"]))
    n, T, E = rec["n"], rec["T"], rec["E"]
    rec["fwd_bytes"] = int(16 * T + 8 * E + 8 * n + 20 * T + 4 * E + 4 * n + 40 * T + 8 * E + 8 * n
                           + 16 * T + 24 * T + 20 * T + 8 * E + 20 * n + 12 * rec["out_verts"] + 32 * rec["out_tets"])
    rec["fwd_GBs"] = rec["fwd_bytes"] / rec["native_fwd_ms"] / 1e6
    rec["speedup_fwd"] = rec["torch_fwd_ms"] / rec["native_fwd_ms"]
    rec["speedup_fwd_bwd"] = rec["torch_fwd_bwd_ms"] / rec["native_fwd_bwd_ms"]
    return rec


def shape_loop(v_np, t_np, iters):
    from diffsound_amd.diffelastic.diff_model import DiffSoundObj, TetMesh
    from diffsound_amd.dmtet import DMTetGeometry

    torch.manual_seed(0)
    geo = DMTetGeometry(32, grid=(v_np, t_np)).cuda()
    init = 0.36 - torch.linalg.norm(geo.verts, dim=1, keepdim=True)
    opt = torch.optim.Adam(geo.parameters(), lr=1e-3)
    for _ in range(300):  # a sphere-like start, as the reference's template pre-training gives
        opt.zero_grad()
        ((geo.sdf - init) ** 2).mean().backward()
        opt.step()
    gt_vals = None
    opt = torch.optim.Adam(geo.parameters(), lr=1e-4)
    rows = []
    for it in range(iters + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        verts, tets = geo.getMesh()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        verts, tets = geo.get_largest_connected_component(verts, tets)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        vols = torch.abs(torch.det(TetMesh(vertices=verts, tets=tets).transform_matrix))
        tets = tets[vols > 0]
        obj = DiffSoundObj(verts, tets, mode_num=16)
        obj.eigen_decomposition()
        vals = obj.get_vals()
        if gt_vals is None:
            gt_vals = vals.detach() * 1.05
        loss = (((vals - gt_vals) ** 2) / gt_vals ** 2).mean() ** 0.5
        opt.zero_grad()
        loss.backward()
        opt.step()
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        if it > 0:  # the first iteration warms the caches
            rows.append(((t3 - t0) * 1e3, (t1 - t0) * 1e3, (t2 - t1) * 1e3, int(tets.shape[0])))
    r = np.array(rows)
    it_ms = float(np.median(r[:, 0]))
    return dict(grid=32, iterations=iters, iteration_ms=it_ms, iterations_per_s=1e3 / it_ms,
                getMesh_ms=float(np.median(r[:, 1])), lcc_ms=float(np.median(r[:, 2])),
                dmtet_share=float(np.median(r[:, 1] + r[:, 2]) / it_ms), tets=int(np.median(r[:, 3])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", action="append", default=[], help="data/tets/{res}_tets.npz file (repeatable)")
    ap.add_argument("--kuhn", default="96,128")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--loop-iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from diffsound_amd.dmtet import kuhn_grid

    assert torch.cuda.is_available(), "dmtet_bench needs a HIP device"
    triad = stream_triad_gbs(args.reps)
    rec = dict(device=torch.cuda.get_device_name(0), reps=args.reps, stream_triad_GBs=triad, sizes=[])
    torch_mt = TorchMarchingTets(torch.device("cuda"))
    grids = []
    for p in args.grid:
        g = np.load(p)
        grids.append((os.path.basename(p), g["vertices"].astype(np.float32), g["indices"].astype(np.int64)))
    for r in [int(x) for x in args.kuhn.split(",") if x]:
        grids.append((f"kuhn_grid({r})",) + kuhn_grid(r))
    for name, v, t in grids:
        rec["sizes"].append(measure_grid(name, v, t, args.reps, torch_mt))
        print(json.dumps(rec["sizes"][-1]), file=sys.stderr)
    last = rec["sizes"][-1]
    rec["largest_fwd_fraction_of_triad"] = last["fwd_GBs"] / triad
    g32 = [g for g in grids if g[0].startswith("32_")]
    if g32:
        rec["shape_loop"] = shape_loop(g32[0][1], g32[0][2], args.loop_iters)
    text = json.dumps(rec, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
