"""Forward and backward times of the two oscillator-bank paths: the FIR kernels (ds_osc_bank_fwd / _bwd, csrc/oscillator.hip,
at most 512 taps) and the driven kernels (ds_osc_driven_fwd / _bwd, csrc/osc_driven.hip, any force length), at
A = 8, m = 64, S = 8000, sr = 32000: F in {150, 512} on both, F in {2048, 8000} on the driven pair alone.
HIP events around each call on preallocated buffers, warm-up, median of --runs calls.

    python tools/mb_osc_driven.py [--runs 30] [--out profiles/osc_driven_bench.txt]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diffsound_amd import _hip  # noqa: E402

A, M, S, SR = 8, 64, 8000, 32000.0


def _median_ms(fn, runs, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(runs):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        times.append(t0.elapsed_time(t1))
    return statistics.median(times), min(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--out", default=os.path.join("profiles", "osc_driven_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mb_osc_driven: needs a HIP device")
    dev = torch.device("cuda:0")
    L, p, st = _hip.lib(), _hip.ptr, _hip.stream_ptr()
    g = torch.Generator().manual_seed(0)
    w = (2 * torch.pi * torch.sort(torch.rand(M, generator=g, dtype=torch.float64) * 14000 + 100)[0]).to(dev)
    d = (torch.rand(M, generator=g, dtype=torch.float64) * 300 + 2).to(dev)
    amp = (torch.rand((A, M), generator=g) + 0.5).to(dev)
    gy = torch.randn((A, S), generator=g).to(dev)
    y, gs = torch.empty((A, S), device=dev), torch.empty((A, S), device=dev)
    gd, gw = torch.empty(M, dtype=torch.float64, device=dev), torch.empty(M, dtype=torch.float64, device=dev)
    gamp = torch.empty((A, M), device=dev)
    nbytes = L.ds_osc_driven_workspace_bytes(A, M, S)
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    rows = [f"# A = {A}, m = {M}, S = {S}, sr = {SR:g}; median (min) of {args.runs} calls, ms, HIP events; {torch.cuda.get_device_name(0)}",
            f"# {'F':>5} {'path':<7} {'forward':>18} {'backward':>18}"]
    for F in (150, 512, 2048, 8000):
        force = torch.randn((A, F), generator=g).to(dev)
        gforce = torch.empty((A, F), device=dev)
        if F <= 512:
            fwd = lambda: _hip.check(L.ds_osc_bank_fwd(p(d), p(w), p(amp), p(force), A, M, F, S, SR, p(y), st), "fwd")
            bwd = lambda: _hip.check(L.ds_osc_bank_bwd(p(gy), p(d), p(w), p(amp), p(force), A, M, F, S, SR, p(gs), p(gd), p(gw),
                                                       p(gamp), st), "bwd")
            (fm, fmin), (bm, bmin) = _median_ms(fwd, args.runs), _median_ms(bwd, args.runs)
            rows.append(f"  {F:>5} {'fir':<7} {fm:>9.4f} ({fmin:.4f}) {bm:>9.4f} ({bmin:.4f})")
        fwd = lambda: _hip.check(L.ds_osc_driven_fwd(p(d), p(w), p(amp), p(force), A, M, F, S, SR, p(work), nbytes, p(y), st), "fwd")
        bwd = lambda: _hip.check(L.ds_osc_driven_bwd(p(gy), p(d), p(w), p(amp), p(force), A, M, F, S, SR, p(work), nbytes, p(gd),
                                                     p(gw), p(gamp), p(gforce), st), "bwd")
        (fm, fmin), (bm, bmin) = _median_ms(fwd, args.runs), _median_ms(bwd, args.runs)
        rows.append(f"  {F:>5} {'driven':<7} {fm:>9.4f} ({fmin:.4f}) {bm:>9.4f} ({bmin:.4f})")
    text = "\n".join(rows) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
