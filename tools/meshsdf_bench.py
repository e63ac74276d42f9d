"""Performance and accuracy record of the mesh signed distance (csrc/meshsdf.hip through diffsound_amd/meshsdf.py).

Three cases: 36 562 points x 348 faces (the frog of tests/golden/g11_meshsdf.npz at the point count of DMTet's 64
grid), 36 562 x 5 674 and 262 144 (a 64^3 lattice) x 5 674 (a watertight bumpy sphere built here: a 64 x 45 UV sphere,
5 632 faces, with 21 faces split at their centroids).  Points are seeded uniform samples of [-0.75, 0.75]^3, or the
lattice on the same cube.  Per case:

* ``kernel_ms``: the sum of the query's kernels per call from a ``rocprofv3 --kernel-trace`` run of its own (this
  script starts it as a child process with ``--trace-child`` and reads the trace), median over the child's calls;
* ``events_ms`` / ``wall_ms``: ``MeshDistance.signed_distance`` between device events, and on the host clock with a
  device synchronise at the end (points already on the device), median of ``--reps`` calls after a warm-up;
* ``torch_ms``: the same formulas as plain torch ops on the device, in chunks of at most 2^24 pairs (the
  comparison tools/dmtet_bench.py makes); ``numpy64_s``: the fp64 NumPy restatement of tests/test_meshsdf_cpu.py on the
  host, one run, on at most ``--numpy-points`` of the points (scaled to the case's point count);
* ``ns_per_pair`` of the kernel, and the largest absolute distance error of the kernel against the restatement on
  those points.

``accuracy``: the kernel's largest absolute distance error against the restatement on the three fixture cases and the
12-face box of the tests, whose 4-fold is the tests' tolerance.  Writes one JSON document (``--out``, default stdout)."""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

TRACE_CALLS = 20


def bumpy_sphere(seg=64, rings=45, faces=5674):
    """A watertight, outward-wound bumpy sphere with exactly ``faces`` triangles."""
    th = np.linspace(0, np.pi, rings + 1)[1:-1]
    ph = np.arange(seg) * 2 * np.pi / seg
    T, Ph = np.meshgrid(th, ph, indexing="ij")
    r = 0.5 + 0.06 * np.sin(3 * T) * np.cos(4 * Ph)
    v = np.stack([r * np.sin(T) * np.cos(Ph), r * np.sin(T) * np.sin(Ph), r * np.cos(T)], -1).reshape(-1, 3)
    v = np.vstack([v, [[0, 0, 0.5]], [[0, 0, -0.5]]])
    top, bot = len(v) - 2, len(v) - 1
    f = []
    for j in range(seg):
        j1 = (j + 1) % seg
        f.append((top, j, j1))
        f.append((bot, (rings - 2) * seg + j1, (rings - 2) * seg + j))
        for i in range(rings - 2):
            a, b, c, d = i * seg + j, i * seg + j1, (i + 1) * seg + j, (i + 1) * seg + j1
            f += [(a, c, d), (a, d, b)]
    v, f = list(map(tuple, v)), list(f)
    k = 0
    while len(f) < faces:  # 1 -> 3 split at the centroid: two more faces, still watertight
        a, b, c = f[k]
        v.append(tuple((np.array(v[a]) + np.array(v[b]) + np.array(v[c])) / 3))
        m = len(v) - 1
        f[k] = (a, b, m)
        f += [(b, c, m), (c, a, m)]
        k += 97
    assert len(f) == faces
    return np.array(v, dtype=np.float32), np.array(f, dtype=np.int64)


def cases():
    g = np.load(os.path.join(ROOT, "tests", "golden", "g11_meshsdf.npz"))
    rng = np.random.default_rng(0)
    cloud = rng.uniform(-0.75, 0.75, size=(36562, 3)).astype(np.float32)
    ax = np.linspace(-0.75, 0.75, 64, dtype=np.float32)
    lattice = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    sv, sf = bumpy_sphere()
    return [("frog_36562x348", g["frog_vertices"], g["frog_faces"].astype(np.int64), cloud),
            ("sphere_36562x5674", sv, sf, cloud), ("sphere_262144x5674", sv, sf, lattice)]


def timed_events(fn, reps):
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


def timed_wall(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def torch_signed_distance(p, v, f, max_pairs=1 << 24):
    """The kernel's formulas as torch ops on the device: plane or nearest edge, Van Oosterom-Strackee, fp32."""
    a, b, c = v[f[:, 0]][None], v[f[:, 1]][None], v[f[:, 2]][None]
    n = torch.cross(b - a, c - a, dim=-1)
    nn = (n * n).sum(-1)
    valid = nn > 0
    n = n / torch.where(valid, nn.sqrt(), torch.ones_like(nn))[..., None]
    out = torch.empty(len(p), device=p.device)
    step = max(1, max_pairs // len(f))

    def seg(U, d):
        dd = (d * d).sum(-1)
        t = (-(U * d).sum(-1) / torch.where(dd > 0, dd, torch.ones_like(dd))).clamp(0, 1)
        q = U + t[..., None] * d
        return (q * q).sum(-1)

    for s in range(0, len(p), step):
        x = p[s:s + step, None, :]
        A, B, C = a - x, b - x, c - x
        cab, cbc, cca = torch.cross(A, B, dim=-1), torch.cross(B, C, dim=-1), torch.cross(C, A, dim=-1)
        inside = valid & ((n * cab).sum(-1) >= 0) & ((n * cbc).sum(-1) >= 0) & ((n * cca).sum(-1) >= 0)
        edge = torch.minimum(torch.minimum(seg(A, b - a), seg(B, c - b)), seg(C, a - c))
        d2 = torch.where(inside, (A * n).sum(-1) ** 2, edge)
        la, lb, lc = A.norm(dim=-1), B.norm(dim=-1), C.norm(dim=-1)
        det = (A * cbc).sum(-1)
        den = la * lb * lc + (A * B).sum(-1) * lc + (A * C).sum(-1) * lb + (B * C).sum(-1) * la
        w = torch.where(valid, torch.atan2(det, den), torch.zeros_like(det)).sum(1) / (2 * np.pi)
        d = d2.min(1).values.sqrt()
        out[s:s + step] = torch.where(w > 0.5, -d, d)
    return out


def trace_child():
    """What the traced child runs: TRACE_CALLS queries per case, in case order, nothing else on the device."""
    from diffsound_amd.meshsdf import MeshDistance

    for _, v, f, p in cases():
        md = MeshDistance(v, f)
        pts = torch.from_numpy(p).cuda()
        for _ in range(TRACE_CALLS):
            md.signed_distance(pts)
        torch.cuda.synchronize()


def kernel_times():
    """{case: median ms of the query's kernels per call} from a rocprofv3 kernel trace of a child process."""
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        raise RuntimeError("rocprofv3 not found")
    with tempfile.TemporaryDirectory() as tmp:
        subprocess.run([exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable,
                        os.path.abspath(__file__), "--trace-child"], check=True, cwd=ROOT, timeout=420,
                       stdout=subprocess.DEVNULL)
        files = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)
        rows = []
        for path in files:
            for r in csv.DictReader(open(path)):
                name = r["Kernel_Name"]
                if "mesh_sdf_kernel" in name or "mesh_sdf_combine" in name:
                    rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), "combine" in name))
    rows.sort()
    calls, cur = [], 0.0
    for i, (s, e, comb) in enumerate(rows):  # a call is one main kernel, followed by a combine when the faces are split
        cur += (e - s) * 1e-6
        nxt_is_combine = i + 1 < len(rows) and rows[i + 1][2]
        if not nxt_is_combine:
            calls.append(cur)
            cur = 0.0
    names = [c[0] for c in cases()]
    if len(calls) != TRACE_CALLS * len(names):
        raise RuntimeError(f"kernel trace: {len(calls)} calls found, {TRACE_CALLS * len(names)} expected")
    return {nm: float(np.median(calls[i * TRACE_CALLS + 2:(i + 1) * TRACE_CALLS])) for i, nm in enumerate(names)}


def accuracy():
    import test_meshsdf_cpu as ref
    from diffsound_amd.meshsdf import MeshDistance

    g = np.load(os.path.join(ROOT, "tests", "golden", "g11_meshsdf.npz"))
    out = {}
    for case in ref.CASES:
        d = MeshDistance(g[f"{case}_vertices"], g[f"{case}_faces"]).unsigned_distance(g[f"{case}_points"]).cpu().numpy()
        out[case] = float(np.abs(d - g[f"{case}_unsigned"]).max())
    v, f = ref.box_mesh(*ref.BOX)
    v = v.astype(np.float32)
    p = ref.box_points().astype(np.float32)
    d = MeshDistance(v, f).unsigned_distance(p).cpu().numpy()
    out["box"] = float(np.abs(d - ref.restatement(p, v, f)[0]).max())
    out["max"] = max(out.values())
    out["relative_to_64_grid_edge"] = out["max"] / (1.5 / 64)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--numpy-points", type=int, default=2048)
    ap.add_argument("--no-trace", action="store_true", help="skip the rocprofv3 child (kernel_ms is then null)")
    ap.add_argument("--trace-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("meshsdf_bench: no HIP device (a timing taken elsewhere says nothing)")
    if args.trace_child:
        trace_child()
        return
    import test_meshsdf_cpu as ref
    from diffsound_amd import _hip
    from diffsound_amd.meshsdf import MeshDistance

    rec = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "trace_calls": TRACE_CALLS, "cases": []}
    ktimes, rec["kernel_trace_error"] = {}, None
    if not args.no_trace:  # first, while this process has not touched the device
        try:
            ktimes = kernel_times()
        except Exception as ex:  # recorded, not hidden: kernel_ms stays null
            rec["kernel_trace_error"] = f"{type(ex).__name__}: {ex}"
    for name, v, f, p in cases():
        md = MeshDistance(v, f)
        pts = torch.from_numpy(p).cuda()
        vt, ft = torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()
        pairs = len(p) * len(f)
        split = int(_hip.lib().ds_mesh_sdf_workspace_bytes(len(p), len(f), 0)) > 0
        ev = timed_events(lambda: md.signed_distance(pts), args.reps)
        wall = timed_wall(lambda: md.signed_distance(pts), args.reps)
        tt = timed_events(lambda: torch_signed_distance(pts, vt, ft), max(3, args.reps // 4))
        agree = float((torch_signed_distance(pts, vt, ft) - md.signed_distance(pts)).abs().max())
        sub = np.linspace(0, len(p) - 1, min(args.numpy_points, len(p))).astype(np.int64)
        t0 = time.perf_counter()
        dist, wind, _ = ref.restatement(p[sub], v, f)
        t_np = (time.perf_counter() - t0) * len(p) / len(sub)
        got = md.signed_distance(pts).cpu().numpy()[sub]
        far = dist > 1e-5
        k = ktimes.get(name)
        rec["cases"].append({
            "name": name, "points": len(p), "faces": len(f), "pairs": pairs, "faces_split_across_workgroups": split,
            "kernel_ms": k, "ns_per_pair_kernel": None if k is None else k * 1e6 / pairs,
            "events_ms": ev, "ns_per_pair_events": ev * 1e6 / pairs, "wall_ms": wall, "torch_ms": tt,
            "torch_over_native": tt / ev, "numpy64_s_scaled": t_np, "numpy64_points_run": len(sub),
            "max_abs_err_vs_numpy64": float(np.abs(np.abs(got) - dist).max()),
            "sign_flips_beyond_1e-5": int(((got < 0) != (wind > 0.5))[far].sum()),
            "max_abs_diff_torch_vs_native": agree})
        print(json.dumps(rec["cases"][-1]), file=sys.stderr, flush=True)
    rec["accuracy"] = accuracy()
    text = json.dumps(rec, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    else:
        print(text)


if __name__ == "__main__":
    main()
