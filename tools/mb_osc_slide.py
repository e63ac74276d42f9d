"""Forward and backward times of the sliding bank (ds_osc_slide_fwd / _bwd, csrc/osc_slide.hip) at A = 8, m = 64, S = 8000,
sr = 32000, F in {512, 8000}, hop in {64, 1024} (K = ceil(S / hop) + 1 frames), beside two yardsticks: the driven bank
(ds_osc_driven_fwd / _bwd) at the same shape, and the K-clip emulation the sliding bank replaces - one driven clip per
control frame, here as ONE driven call on A K clips (the sum over the K rows that the emulation also needs is not timed).
HIP events around each call on preallocated buffers, warm-up, median and minimum of --runs calls.

    python tools/mb_osc_slide.py [--runs 30] [--out profiles/osc_slide_bench.txt]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diffsound_amd import _hip  # noqa: E402

A, M, S, SR = 8, 64, 8000, 32000.0


def _times_ms(fn, runs, warmup=5):
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
    ap.add_argument("--out", default=os.path.join("profiles", "osc_slide_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mb_osc_slide: needs a HIP device")
    dev = torch.device("cuda:0")
    L, p, st = _hip.lib(), _hip.ptr, _hip.stream_ptr()
    g = torch.Generator().manual_seed(0)
    w = (2 * torch.pi * torch.sort(torch.rand(M, generator=g, dtype=torch.float64) * 14000 + 100)[0]).to(dev)
    d = (torch.rand(M, generator=g, dtype=torch.float64) * 300 + 2).to(dev)
    gd, gw = torch.empty(M, dtype=torch.float64, device=dev), torch.empty(M, dtype=torch.float64, device=dev)
    rows = [f"# A = {A}, m = {M}, S = {S}, sr = {SR:g}; median (min) of {args.runs} calls, ms, HIP events; {torch.cuda.get_device_name(0)}",
            f"# {'F':>5} {'hop':>5} {'K':>4} {'path':<22} {'forward':>18} {'backward':>18}"]

    def driven(clips, F, name, tag):
        amp = (torch.rand((clips, M), generator=g) + 0.5).to(dev)
        force, gy = torch.randn((clips, F), generator=g).to(dev), torch.randn((clips, S), generator=g).to(dev)
        y, gamp, gforce = torch.empty((clips, S), device=dev), torch.empty((clips, M), device=dev), torch.empty((clips, F), device=dev)
        nbytes = L.ds_osc_driven_workspace_bytes(clips, M, S)
        work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        fwd = lambda: _hip.check(L.ds_osc_driven_fwd(p(d), p(w), p(amp), p(force), clips, M, F, S, SR, p(work), nbytes, p(y), st), "fwd")
        bwd = lambda: _hip.check(L.ds_osc_driven_bwd(p(gy), p(d), p(w), p(amp), p(force), clips, M, F, S, SR, p(work), nbytes,
                                                     p(gd), p(gw), p(gamp), p(gforce), st), "bwd")
        (fm, fmin), (bm, bmin) = _times_ms(fwd, args.runs), _times_ms(bwd, args.runs)
        rows.append(f"  {tag} {name:<22} {fm:>9.4f} ({fmin:.4f}) {bm:>9.4f} ({bmin:.4f})")

    for F in (512, 8000):
        driven(A, F, "driven", f"{F:>5} {'-':>5} {'-':>4}")
        for hop in (64, 1024):
            K = -(-S // hop) + 1
            tag = f"{F:>5} {hop:>5} {K:>4}"
            amp = (torch.rand((A, M), generator=g) + 0.5).to(dev)
            force, gy = torch.randn((A, F), generator=g).to(dev), torch.randn((A, S), generator=g).to(dev)
            gain = torch.randn((A, M, K), generator=g).to(dev)
            y, gamp, gforce = torch.empty((A, S), device=dev), torch.empty((A, M), device=dev), torch.empty((A, F), device=dev)
            ggain = torch.empty((A, M, K), device=dev)
            nbytes = L.ds_osc_slide_workspace_bytes(A, M, S, K, hop)
            work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            fwd = lambda: _hip.check(L.ds_osc_slide_fwd(p(d), p(w), p(amp), p(force), p(gain), A, M, F, S, K, hop, SR, p(work), nbytes,
                                                        p(y), st), "fwd")
            bwd = lambda: _hip.check(L.ds_osc_slide_bwd(p(gy), p(d), p(w), p(amp), p(force), p(gain), A, M, F, S, K, hop, SR, p(work),
                                                        nbytes, p(gd), p(gw), p(gamp), p(gforce), p(ggain), st), "bwd")
            (fm, fmin), (bm, bmin) = _times_ms(fwd, args.runs), _times_ms(bwd, args.runs)
            rows.append(f"  {tag} {'sliding':<22} {fm:>9.4f} ({fmin:.4f}) {bm:>9.4f} ({bmin:.4f})")
            driven(A * K, F, f"emulation ({A * K} clips)", tag)
    text = "\n".join(rows) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
