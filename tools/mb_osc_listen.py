"""Forward and forward + backward times of the listener bank (ds_osc_listen_fwd / _bwd, csrc/osc_listen.hip) at A = 8,
m = 64, S = 8000, F = 8000, sr = 32000, C in {1, 2, 8}, K in {1, 126} (hop = 64 for K = 126), beside the driven bank
(ds_osc_driven_fwd / _bwd) at the same A, m, S.  A timed window is 20 back-to-back calls on preallocated buffers between two
HIP events (about 1 ms); for every row the driven bank and the listener bank are ALTERNATED window by window, after warm-up,
--runs windows each: median, minimum and spread (p10 .. p90) of both, and the median of the per-pair ratios.  Time is
reported, not gated.

    python tools/mb_osc_listen.py [--runs 30] [--out profiles/osc_listen_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diffsound_amd import _hip  # noqa: E402

A, M, S, F, SR = 8, 64, 8000, 8000, 32000.0


BATCH = 20  # calls per timed window: ~1 ms between the two events at 50 us a call


def _window_ms(fn):
    """One timed window: BATCH back-to-back calls between two events; ms per call."""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(BATCH):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / BATCH


def _stats(times):
    q = statistics.quantiles(times, n=10) if len(times) > 1 else [times[0]] * 9
    return dict(median=statistics.median(times), min=min(times), p10=q[0], p90=q[-1])


def _compare(base_fn, fn, runs, warmup=2):
    """The two versions ALTERNATED, window by window, so that clock and thermal drift reach both alike: (stats of the
    baseline, stats of fn, median of the per-pair ratios fn / baseline)."""
    for _ in range(warmup):
        _window_ms(base_fn)
        _window_ms(fn)
    torch.cuda.synchronize()
    tb, tf = [], []
    for _ in range(runs):
        tb.append(_window_ms(base_fn))
        tf.append(_window_ms(fn))
    return _stats(tb), _stats(tf), statistics.median(f / b for f, b in zip(tf, tb))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--out", default=os.path.join("profiles", "osc_listen_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mb_osc_listen: needs a HIP device")
    dev = torch.device("cuda:0")
    L, p, st = _hip.lib(), _hip.ptr, _hip.stream_ptr()
    g = torch.Generator().manual_seed(0)
    w = (2 * torch.pi * torch.sort(torch.rand(M, generator=g, dtype=torch.float64) * 14000 + 100)[0]).to(dev)
    d = (torch.rand(M, generator=g, dtype=torch.float64) * 300 + 2).to(dev)
    gd, gw = torch.empty(M, dtype=torch.float64, device=dev), torch.empty(M, dtype=torch.float64, device=dev)
    amp = (torch.rand((A, M), generator=g) + 0.5).to(dev)
    force = torch.randn((A, F), generator=g).to(dev)
    gamp, gforce = torch.empty((A, M), device=dev), torch.empty((A, F), device=dev)

    gy1, y1 = torch.randn((A, S), generator=g).to(dev), torch.empty((A, S), device=dev)
    nb = L.ds_osc_driven_workspace_bytes(A, M, S)
    work = torch.empty(nb, dtype=torch.uint8, device=dev)
    dfwd = lambda: _hip.check(L.ds_osc_driven_fwd(p(d), p(w), p(amp), p(force), A, M, F, S, SR, p(work), nb, p(y1), st), "fwd")
    dbwd = lambda: _hip.check(L.ds_osc_driven_bwd(p(gy1), p(d), p(w), p(amp), p(force), A, M, F, S, SR, p(work), nb, p(gd), p(gw),
                                                  p(gamp), p(gforce), st), "bwd")
    both = lambda f, b: (lambda: (f(), b()))
    result = dict(device=torch.cuda.get_device_name(0), A=A, m=M, S=S, F=F, sr=SR, runs=args.runs, calls_per_window=BATCH,
                  unit="ms per call", listen=[])
    for K, hop in ((1, 16), (126, 64)):
        for C in (1, 2, 8):
            h = torch.randn((A, C, M, K, 2), generator=g).to(dev)
            gy, y, gh = torch.randn((A, C, S), generator=g).to(dev), torch.empty((A, C, S), device=dev), torch.empty_like(h)
            nbl = L.ds_osc_listen_workspace_bytes(A, C, M, S, K, hop)
            wl = torch.empty(nbl, dtype=torch.uint8, device=dev)
            fwd = lambda: _hip.check(L.ds_osc_listen_fwd(p(d), p(w), p(amp), p(force), p(h), A, C, M, F, S, K, hop, SR, p(wl), nbl,
                                                         p(y), st), "fwd")
            bwd = lambda: _hip.check(L.ds_osc_listen_bwd(p(gy), p(d), p(w), p(amp), p(force), p(h), A, C, M, F, S, K, hop, SR, p(wl),
                                                         nbl, p(gd), p(gw), p(gamp), p(gforce), p(gh), st), "bwd")
            row = dict(C=C, K=K, hop=hop)
            for key, base_fn, fn in (("forward", dfwd, fwd), ("forward_backward", both(dfwd, dbwd), both(fwd, bwd))):
                sb, sf, ratio = _compare(base_fn, fn, args.runs)
                row[key] = dict(sf, driven=sb, ratio_to_driven=ratio)
            result["listen"].append(row)
            print(f"C {C} K {K:>3}  fwd {row['forward']['median']:.4f} (driven {row['forward']['driven']['median']:.4f}, "
                  f"x{row['forward']['ratio_to_driven']:.2f})  fwd+bwd {row['forward_backward']['median']:.4f} (driven "
                  f"{row['forward_backward']['driven']['median']:.4f}, x{row['forward_backward']['ratio_to_driven']:.2f}) ms")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
