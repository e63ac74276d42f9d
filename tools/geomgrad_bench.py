"""Times of the two geometry-backward kernels of csrc/geomgrad.hip in isolation: ds_geometry_grad ((lam, mu), fp64 atomics)
and ds_geometry_grad_tangent (any 9 x 9 tangent; the element kernel plus the per-node sum).

Two cases: the shape loop's mesh (bench.py --workload geom: the 32 x 32 x 8-cell Kuhn shell, order 1, 32 modes) and the
benchmark's mesh (a 26^3 Kuhn box lifted to order 2: 105 456 elements, 64 modes).  The modes are random fp32 columns - the
kernels' work does not depend on the values - and the tangent is that of (lam, mu), so both compute the same gradient;
``max_rel_diff`` is their difference over the largest magnitude.

Per case ``lame_call_ms`` / ``tangent_call_ms``: the median over ``--reps`` calls of ``TetSystem.geometry_grad`` /
``geometry_grad_tangent`` between device events, after a warm-up (the call: allocation of the result, the kernels, the
return to the caller's numbering).  The kernels alone are read off a kernel trace of the same program,

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/geomgrad_bench.py --out -

(geometry_grad_kernel<N>, geometry_grad_tangent_kernel<N>, geometry_grad_gather_kernel; ``--case`` runs one case, so that
the statistics of the two meshes stay apart).  Writes one JSON document to ``--out`` (``-`` for stdout)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {"shape_ord1": dict(cells=(32, 32, 8), box=(0.10, 0.10, 0.025), order=1, modes=32),
         "bench_ord2": dict(cells=(26, 26, 26), box=None, order=2, modes=64)}


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--case", default="all", choices=["all"] + list(CASES))
    ap.add_argument("--out", default="-")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("geomgrad_bench: no HIP device (a timing taken elsewhere says nothing)")
    from diffsound_amd import meshgen
    from diffsound_amd.diffelastic.material_model import Material, MatSet
    from diffsound_amd.diffelastic.mesh import TetMesh
    from diffsound_amd.modal_ops import TetSystem, isotropic_tangent

    dev = torch.device("cuda:0")
    mat = Material(MatSet.Ceramic)
    lam = mat.youngs * mat.poisson / ((1 + mat.poisson) * (1 - 2 * mat.poisson))
    mu = mat.youngs / (2 * (1 + mat.poisson))
    C = isotropic_tangent(lam, mu)
    rec = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "cases": []}
    for name, c in CASES.items():
        if args.case not in ("all", name):
            continue
        v, t = meshgen.kuhn_box(*c["cells"], **({} if c["box"] is None else {"box": c["box"]}))
        mesh = TetMesh(torch.from_numpy(v).float().to(dev), torch.from_numpy(t).long().to(dev)).to_high_order(c["order"])
        s = TetSystem(mesh.vertices, mesh.tets, c["order"], mat.density)
        gen = torch.Generator(device=dev).manual_seed(1)
        U = torch.randn((s.n, c["modes"]), device=dev, generator=gen)
        gk = torch.rand((c["modes"],), device=dev, generator=gen, dtype=torch.float64) + 0.5
        gm = gk * 1e9
        s.corner_incidence()  # (topology: built once, outside the timed calls)
        old, new = s.geometry_grad(U, gk, gm, lam, mu), s.geometry_grad_tangent(U, gk, gm, C)
        case = {"name": name, "order": c["order"], "elements": s.T, "nodes": s.nv, "modes": c["modes"],
                "lame_call_ms": timed(lambda: s.geometry_grad(U, gk, gm, lam, mu), args.reps),
                "tangent_call_ms": timed(lambda: s.geometry_grad_tangent(U, gk, gm, C), args.reps),
                "max_rel_diff": float((new - old).abs().max() / old.abs().max())}
        rec["cases"].append(case)
        print(json.dumps(case), file=sys.stderr, flush=True)
        del s, U, mesh
        torch.cuda.empty_cache()
    text = json.dumps(rec, indent=1)
    if args.out != "-":
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    else:
        print(text)


if __name__ == "__main__":
    main()
