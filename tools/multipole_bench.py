"""Times of the radiation path (diffelastic/radiation.py, csrc/multipole.hip) for the record, not a gate: the one-off cost of
``ModalRadiator`` on the surface of the benchmark mesh (the Kuhn box of bench.py, coarsened while its dense boundary-element
operator would exceed ``bem.BEM_MEMORY_BUDGET_BYTES``) with 64 modes, ``transfer`` forward and forward + backward (gradient to
the listener positions) at P in {1, 1024, 65536} - medians of device events after warm-up, the first call reported apart -
and, beside them, ``bem.modal_transfer`` at P = 1024 on the same object, once.  Writes profiles/multipole_bench.json.

    python tools/multipole_bench.py [--cells 26] [--modes 64] [--out profiles/multipole_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from diffsound_amd import meshgen  # noqa: E402
from diffsound_amd.diffelastic import bem  # noqa: E402
from diffsound_amd.diffelastic.diff_model import DiffSoundObj, FixedLinear  # noqa: E402
from diffsound_amd.diffelastic.radiation import ModalRadiator  # noqa: E402

MAT = (2700.0, 5e10, 0.25, 6.0, 1e-7)
REPS = 20


def median_ms(fn, reps=REPS):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    first = a.elapsed_time(b)
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return first, statistics.median(times), min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=26)
    ap.add_argument("--modes", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multipole_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device: a timing taken elsewhere says nothing"
    dev = torch.device("cuda:0")
    cells = args.cells
    while 8 * (12 * cells * cells) ** 2 > bem.BEM_MEMORY_BUDGET_BYTES:  # 12 cells^2 boundary faces, 8 bytes per entry
        cells -= 1
    v, t = meshgen.kuhn_box(cells)
    obj = DiffSoundObj(vertices=torch.from_numpy(v).to(dev), tets=torch.from_numpy(t).long().to(dev), mode_num=args.modes, mat=MAT,
                       order=1, mat_model=FixedLinear, task="gt")
    t0 = time.perf_counter()
    obj.eigen_decomposition()
    torch.cuda.synchronize()
    eig_s = time.perf_counter() - t0
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        t0 = time.perf_counter()
        rad = ModalRadiator(obj)
        torch.cuda.synchronize()
        build_s = time.perf_counter() - t0
    ka = (rad.k * rad.radius).tolist()
    result = dict(device=torch.cuda.get_device_name(0), cells=cells, faces=12 * cells * cells, modes=args.modes, order=rad.order,
                  samples=rad.sample_points.shape[0], ka_min=min(ka), ka_max=max(ka), eigen_decomposition_s=eig_s,
                  radiator_build_s=build_s, fit_residual_median=float(rad.fit_residual.median()),
                  fit_residual_max=float(rad.fit_residual.max()), warnings=len(caught),
                  gmres_iterations=[i["iterations"] for i in rad.gmres_info], reps=REPS, rows=[])
    print(json.dumps({k: v for k, v in result.items() if k != "rows"}), flush=True)
    gen = torch.Generator().manual_seed(0)
    for P in (1, 1024, 65536):
        d = torch.randn(P, 3, dtype=torch.float64, generator=gen)
        pts = (rad.center.cpu() + 3.0 * rad.radius * d / d.norm(dim=1, keepdim=True)).to(dev)
        lead = pts.clone().requires_grad_(True)
        g = torch.randn(P, args.modes, dtype=torch.complex128, generator=gen).to(dev)
        with torch.no_grad():
            fwd = median_ms(lambda: rad.transfer(pts))

        def both():
            lead.grad = None
            rad.transfer(lead).backward(g)

        fb = median_ms(both)
        row = dict(P=P, fwd_first_ms=fwd[0], fwd_ms=fwd[1], fwd_min_ms=fwd[2], fwd_max_ms=fwd[3], fwd_bwd_first_ms=fb[0],
                   fwd_bwd_ms=fb[1], fwd_bwd_min_ms=fb[2], fwd_bwd_max_ms=fb[3],
                   fwd_ns_per_point_and_mode=1e6 * fwd[1] / (P * args.modes))
        result["rows"].append(row)
        print(json.dumps(row), flush=True)
        if P == 1024:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ref = torch.from_numpy(bem.modal_transfer(obj, pts.cpu().numpy())).to(dev)
            torch.cuda.synchronize()
            result["modal_transfer_P1024_s_once"] = time.perf_counter() - t0
            with torch.no_grad():
                err = (rad.transfer(pts) - ref).abs().max(0).values / ref.abs().max(0).values
            result["transfer_vs_modal_transfer_at_3a_max_over_peak"] = dict(median=float(err.median()), max=float(err.max()))
            print(json.dumps({k: result[k] for k in ("modal_transfer_P1024_s_once", "transfer_vs_modal_transfer_at_3a_max_over_peak")}),
                  flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
