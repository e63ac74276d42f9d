"""Times of ``ContactSurface.amplitude_map`` (csrc/modesample.hip), forward and backward, on the surface of the
benchmark's mesh: a 26^3 Kuhn box lifted to order 2 (105 456 elements, 8 112 boundary faces), 64 modes.  The modes are
random fp64 columns - the kernels' work does not depend on the values - so no eigensolve is run.

Per direction the median over ``--reps`` calls between device events, after a warm-up: ``fwd_call_ms`` /
``fwd_bwd_call_ms`` are the calls as a user makes them (validation, the scatter of bary3 into L, allocation of the
results, the kernels; the second one is forward and backward together), ``fwd_kernel_ms`` / ``bwd_kernel_ms`` the
launches alone on prepared operands.  The algorithmic bytes of
one pass are P * N * 3 * m * 8 for the gathered rows plus P * m * 8 for the written (forward) or read (backward) gains;
``*_share_of_triad`` is those bytes per second over the STREAM triad of the same run.  The surface points share their
elements' nodes, so most of the gathered rows come from cache: the share is a rate against a yardstick, not a fraction of
HBM traffic.  ``torch_*`` is the same map from ``index_select`` and ``einsum``, for comparison only.

Run it under a time limit of its own, e.g. ``timeout -k 10 300 python tools/mode_sample_bench.py --out
profiles/mode_sample_bench.json``.  Writes one JSON document to ``--out`` (``-`` for stdout)."""
import argparse
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps):
    for _ in range(3):
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


def triad_bytes_per_s(reps):
    from diffsound_amd import _hip

    n = 64 << 20
    a, b, c = (torch.empty(n, device="cuda") for _ in range(3))
    b.fill_(1.0), c.fill_(2.0)
    ms = timed(lambda: _hip.check(_hip.lib().ds_stream_triad(a.data_ptr(), b.data_ptr(), c.data_ptr(), n, 3.0,
                                                            _hip.stream_ptr()), "ds_stream_triad"), reps)
    return 3 * n * 4 / (ms * 1e-3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--cells", type=int, default=26)
    ap.add_argument("--order", type=int, default=2)
    ap.add_argument("--modes", type=int, default=64)
    ap.add_argument("--out", default="-")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mode_sample_bench: no HIP device (a timing taken elsewhere says nothing)")
    from diffsound_amd import fem_tables, meshgen
    from diffsound_amd.diffelastic.mesh import TetMesh
    from diffsound_amd.impact import ContactSurface

    dev = torch.device("cuda:0")
    v, t = meshgen.kuhn_box(args.cells)
    mesh = TetMesh(torch.from_numpy(v).float().to(dev), torch.from_numpy(t).long().to(dev)).to_high_order(args.order)
    nv, m = mesh.vertices.shape[0], args.modes
    gen = torch.Generator(device=dev).manual_seed(1)
    U = torch.randn((3 * nv, m), device=dev, generator=gen, dtype=torch.float64)
    surf = ContactSurface(types.SimpleNamespace(tetmesh=mesh, U_hat=U))  # (all it reads of a DiffSoundObj)
    P, N = surf.num_faces, surf.nodes_per_tet
    gout = torch.randn((P, m), device=dev, generator=gen, dtype=torch.float64)

    face = torch.arange(P, device=dev)
    bary = torch.full((P, 3), 1.0 / 3.0, dtype=torch.float64, device=dev, requires_grad=True)
    elem = surf._elem32[face].contiguous()
    L = torch.zeros((P, 4), dtype=torch.float32, device=dev).scatter_(1, surf._corner[face], bary.detach().float())
    d = surf.normals.float().contiguous()
    out = surf.amplitude_map()

    # the same map in torch: shape functions at the points, rows of U by index_select, two contractions
    nodes = surf._tets32.long()[elem.long()].reshape(-1)
    Nv = torch.from_numpy(fem_tables.shape_values(L.double().cpu().numpy(), args.order)).to(dev)
    bary_t = bary.detach().clone().requires_grad_(True)

    def torch_map(b=None):
        rows = U.reshape(nv, 3 * m).index_select(0, nodes).reshape(P, N, 3, m)
        if b is None:
            return torch.einsum("pa,pacm,pc->pm", Nv, rows, d.double())
        Lb = torch.zeros((P, 4), dtype=torch.float64, device=dev).scatter(1, surf._corner[face], b)
        if args.order == 1:
            w = Lb
        else:
            w = torch.zeros((P, 10), dtype=torch.float64, device=dev)
            for slot, k in fem_tables._CORNER.items():
                w[:, slot] = Lb[:, k] * (2 * Lb[:, k] - 1)
            for slot, (p, q) in fem_tables._MID.items():
                w[:, slot] = 4 * Lb[:, p] * Lb[:, q]
        return torch.einsum("pa,pacm,pc->pm", w, rows, d.double())

    def call_bwd():
        bary.grad = None
        surf.amplitudes(face, bary).backward(gout)

    def torch_bwd():
        bary_t.grad = None
        torch_map(bary_t).backward(gout)

    call_bwd(), torch_bwd()
    nbytes = P * N * 3 * m * 8 + P * m * 8
    triad = triad_bytes_per_s(args.reps)
    rec = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "order": args.order, "elements": surf.num_tets,
           "nodes": nv, "faces": P, "modes": m, "algorithmic_bytes": nbytes, "stream_triad_GBps": triad / 1e9,
           "fwd_call_ms": timed(lambda: surf.amplitude_map(), args.reps),
           "fwd_kernel_ms": timed(lambda: surf._launch_fwd(elem, L, d, True, False), args.reps),
           "fwd_bwd_call_ms": timed(call_bwd, args.reps),
           "bwd_kernel_ms": timed(lambda: surf._launch_bwd(elem, L, d, gout, True, True), args.reps),
           "torch_fwd_ms": timed(lambda: torch_map(), args.reps),
           "torch_fwd_bwd_ms": timed(torch_bwd, args.reps),
           "max_rel_diff_to_torch": float((out - torch_map()).abs().max() / out.abs().max()),
           "grad_rel_diff_to_torch": float((bary.grad - bary_t.grad).abs().max() / bary_t.grad.abs().max())}
    for k in ("fwd", "bwd"):
        rec[f"{k}_GBps"] = nbytes / (rec[f"{k}_kernel_ms"] * 1e-3) / 1e9
        rec[f"{k}_share_of_triad"] = rec[f"{k}_GBps"] / rec["stream_triad_GBps"]
    text = json.dumps(rec, indent=1)
    print(text)
    if args.out != "-":
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
