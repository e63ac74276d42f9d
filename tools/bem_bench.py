"""Performance record of the Helmholtz BEM kernels (csrc/bem.hip) on icospheres with 1 280, 5 120 and 20 480 faces at
one ka, and of modal_transfer on a 64-mode object.  Device events around synchronised work; every figure is the median
of ``--reps`` timed calls after one warm-up call.  Writes one JSON document (``--out``, default stdout).

Issue bound of the assembly: a regular pair is 36 kernel evaluations of ``VALU_PER_EVAL`` plain VALU and
``TRANS_PER_EVAL`` transcendental instructions (rsq, sin, cos; counted from the inner loop of bem_assemble_kernel),
priced by the MI355X issue costs (one wave64 VALU instruction holds a SIMD 2 cycles, a transcendental 4 - the 4:8 ratio
of the per-wave issue costs), over 256 CUs x 4 SIMDs at 2.4 GHz.  Near pairs are not in the bound (they cost more)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VALU_PER_EVAL, TRANS_PER_EVAL = 23, 3
SIMDS, CLOCK = 256 * 4, 2.4e9


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--levels", default="3,4,5")
    ap.add_argument("--ka", type=float, default=2.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--modes", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from diffsound_amd import meshgen
    from diffsound_amd.diffelastic import bem

    assert torch.cuda.is_available(), "bem_bench needs a HIP device"
    triad = stream_triad_gbs(args.reps)
    rec = dict(device=torch.cuda.get_device_name(0), ka=args.ka, reps=args.reps, stream_triad_GBs=triad, sizes=[])
    x0 = np.array([0.2, -0.1, 0.25])
    for level in [int(x) for x in args.levels.split(",")]:
        v, f = meshgen.icosphere(level)
        model = bem.BEMModel(v, f)
        n, k = model.m, args.ka
        c = v[f].mean(1).astype(np.float64)
        r = np.linalg.norm(c - x0, axis=1)
        nrm = c / np.linalg.norm(c, axis=1, keepdims=True)
        gv = ((c - x0) * nrm).sum(1) * (1j * k * r - 1) * np.exp(1j * k * r) / (4 * np.pi * r ** 3)
        g = model._to_internal(gv, "g")
        holder = {}

        def asm():
            holder["A"], holder["rhs"], _ = model.assemble(k, g)

        t_asm = timed(asm, args.reps)
        bound_ms = n * n * 36 * (VALU_PER_EVAL * 2 + TRANS_PER_EVAL * 4) / 64 / (SIMDS * CLOCK) * 1e3
        A = holder["A"]
        x = torch.randn(model._lda, dtype=torch.complex64, device="cuda")
        y = torch.empty(n, dtype=torch.complex64, device="cuda")
        t_mv = timed(lambda: model.cgemv(A, x, model._inv_area, out=y), max(args.reps, 20))
        mv_bytes = n * model._lda * 8 + 2 * n * 8 + n * 4
        info = {}

        def solve():
            _, inf = model._gmres(A, holder["rhs"])
            info.update(inf)

        t_gm = timed(solve, args.reps)
        model.boundary_equation_solve(gv, k)
        rng = np.random.default_rng(0)
        d = rng.normal(size=(10000, 3))
        pts = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(2, 10, size=(10000, 1))
        pts_t = torch.from_numpy(pts).float().cuda()
        t_pot = timed(lambda: model._potential(k, model._g, model._u, pts_t), args.reps)
        rec["sizes"].append(dict(
            faces=n, assembly_ms=t_asm, pairs_per_s=n * n / (t_asm * 1e-3), assembly_issue_bound_ms=bound_ms,
            assembly_fraction_of_issue_bound=bound_ms / t_asm, cgemv_us=t_mv * 1e3, cgemv_GBs=mv_bytes / t_mv / 1e6,
            cgemv_fraction_of_triad=mv_bytes / t_mv / 1e6 / triad, gmres_iterations=info["iterations"],
            gmres_residual=info["residual"], gmres_ms=t_gm, gmres_ms_per_iteration=t_gm / max(info["iterations"], 1),
            potential_1e4_points_ms=t_pot))
        del model, A, holder
        torch.cuda.empty_cache()
        print(json.dumps(rec["sizes"][-1]), flush=True)
    # modal_transfer on a 64-mode object
    from diffsound_amd.diffelastic.diff_model import DiffSoundObj, FixedLinear

    v, t = meshgen.kuhn_box(6)
    obj = DiffSoundObj(vertices=torch.from_numpy(v).cuda(), tets=torch.from_numpy(t).long().cuda(), mode_num=args.modes,
                       mat=(1070.0, 1.4e9, 0.35, 30.0, 1e-6), order=1, mat_model=FixedLinear, task="gt")
    obj.eigen_decomposition()
    pts = v.mean(0) + 2.0 * np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [0.6, 0.6, 0.5]])
    faces = int(bem.surface_of(obj.tetmesh)[0].shape[0])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    import warnings

    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        p = bem.modal_transfer(obj, pts)
    torch.cuda.synchronize()
    rec["modal_transfer"] = dict(modes=args.modes, faces=faces, listeners=len(pts), seconds=time.perf_counter() - t0,
                                 finite=bool(np.isfinite(p).all()), warnings=len(w),
                                 max_ka=float(np.sqrt(obj.eigenvalues.max().item()) / 343.0 * np.linalg.norm(v.max(0) - v.min(0)) / 2))
    out = json.dumps(rec, indent=1)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(out + "\n")
    print(out)


if __name__ == "__main__":
    main()
