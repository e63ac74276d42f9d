"""Forward and forward + backward times of the delay line (ds_delay_fwd / _bwd, csrc/delay.hip) on the rows that the listener
bank renders - A = 8 clips, C in {1, 2, 8} channels, S = 8000 samples, B = A C rows, K in {1, 126} (hop = 64) - beside the
listener bank itself (ds_osc_listen_fwd / _bwd at the same A, C, S, m = 64, F = 8000): what propagation adds to a render.
A timed window is 20 back-to-back calls on preallocated buffers between two HIP events; for every row the listener bank and
the delay line are ALTERNATED window by window, after warm-up, --runs windows each: median, minimum and spread (p10 .. p90)
of both, and the median of the per-pair ratios.  One large shape (B = 64, S = 2^20: 256 MiB in, 256 MiB out) is timed beside
ds_stream_triad in the same run and reported as the fraction of the triad's bandwidth that the forward's algorithmic bytes
(read s, write y: 8 B S) reach.  Time is reported, not gated.

    python tools/mb_delay.py [--runs 30] [--out profiles/delay_bench.json]
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
BATCH = 20  # calls per timed window


def _window_ms(fn, batch=BATCH):
    """One timed window: ``batch`` back-to-back calls between two events; ms per call."""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(batch):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / batch


def _stats(times):
    q = statistics.quantiles(times, n=10) if len(times) > 1 else [times[0]] * 9
    return dict(median=statistics.median(times), min=min(times), p10=q[0], p90=q[-1])


def _compare(base_fn, fn, runs, warmup=2, batch=BATCH):
    """The two ALTERNATED, window by window, so that clock and thermal drift reach both alike: (stats of the baseline, stats of
    fn, median of the per-pair ratios fn / baseline)."""
    for _ in range(warmup):
        _window_ms(base_fn, batch)
        _window_ms(fn, batch)
    torch.cuda.synchronize()
    tb, tf = [], []
    for _ in range(runs):
        tb.append(_window_ms(base_fn, batch))
        tf.append(_window_ms(fn, batch))
    return _stats(tb), _stats(tf), statistics.median(f / b for f, b in zip(tf, tb))


def _delay_calls(L, p, st, B, S_, K, hop, g, dev):
    """(fwd, bwd) closures of the delay line on B rows: a delay that wanders within the slope bound."""
    s, gy = torch.randn((B, S_), generator=g).to(dev), torch.randn((B, S_), generator=g).to(dev)
    steps = (torch.rand((B, K), generator=g, dtype=torch.float64) - 0.5) * hop * 0.8
    tau = (40.0 + torch.cumsum(steps, 1)).abs().to(dev)
    y, gs, gtau = torch.empty_like(s), torch.empty_like(s), torch.empty_like(tau)
    nb = L.ds_delay_workspace_bytes(B, S_, K, hop)
    work = torch.empty(nb, dtype=torch.uint8, device=dev)
    fwd = lambda: _hip.check(L.ds_delay_fwd(p(s), p(tau), B, S_, K, hop, p(y), st), "ds_delay_fwd")
    bwd = lambda: _hip.check(L.ds_delay_bwd(p(gy), p(s), p(tau), B, S_, K, hop, p(work), nb, p(gs), p(gtau), st), "ds_delay_bwd")
    return fwd, bwd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--out", default=os.path.join("profiles", "delay_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mb_delay: needs a HIP device")
    dev = torch.device("cuda:0")
    L, p, st = _hip.lib(), _hip.ptr, _hip.stream_ptr()
    g = torch.Generator().manual_seed(0)
    w = (2 * torch.pi * torch.sort(torch.rand(M, generator=g, dtype=torch.float64) * 14000 + 100)[0]).to(dev)
    d = (torch.rand(M, generator=g, dtype=torch.float64) * 300 + 2).to(dev)
    gd, gw = torch.empty(M, dtype=torch.float64, device=dev), torch.empty(M, dtype=torch.float64, device=dev)
    amp = (torch.rand((A, M), generator=g) + 0.5).to(dev)
    force = torch.randn((A, F), generator=g).to(dev)
    gamp, gforce = torch.empty((A, M), device=dev), torch.empty((A, F), device=dev)
    both = lambda f, b: (lambda: (f(), b()))
    result = dict(device=torch.cuda.get_device_name(0), A=A, m=M, S=S, F=F, sr=SR, runs=args.runs, calls_per_window=BATCH,
                  unit="ms per call", delay=[])
    for K, hop in ((1, 16), (126, 64)):
        for C in (1, 2, 8):
            h = torch.randn((A, C, M, K, 2), generator=g).to(dev)
            gy, y, gh = torch.randn((A, C, S), generator=g).to(dev), torch.empty((A, C, S), device=dev), torch.empty_like(h)
            nbl = L.ds_osc_listen_workspace_bytes(A, C, M, S, K, hop)
            wl = torch.empty(nbl, dtype=torch.uint8, device=dev)
            lfwd = lambda: _hip.check(L.ds_osc_listen_fwd(p(d), p(w), p(amp), p(force), p(h), A, C, M, F, S, K, hop, SR, p(wl), nbl,
                                                          p(y), st), "fwd")
            lbwd = lambda: _hip.check(L.ds_osc_listen_bwd(p(gy), p(d), p(w), p(amp), p(force), p(h), A, C, M, F, S, K, hop, SR, p(wl),
                                                          nbl, p(gd), p(gw), p(gamp), p(gforce), p(gh), st), "bwd")
            fwd, bwd = _delay_calls(L, p, st, A * C, S, K, hop, g, dev)
            row = dict(C=C, K=K, hop=hop, rows=A * C)
            for key, base_fn, fn in (("forward", lfwd, fwd), ("forward_backward", both(lfwd, lbwd), both(fwd, bwd))):
                sb, sf, ratio = _compare(base_fn, fn, args.runs)
                row[key] = dict(sf, listen=sb, ratio_to_listen=ratio)
            result["delay"].append(row)
            print(f"C {C} K {K:>3}  fwd {row['forward']['median']:.4f} (listen {row['forward']['listen']['median']:.4f}, "
                  f"x{row['forward']['ratio_to_listen']:.3f})  fwd+bwd {row['forward_backward']['median']:.4f} (listen "
                  f"{row['forward_backward']['listen']['median']:.4f}, x{row['forward_backward']['ratio_to_listen']:.3f}) ms")
    # the share of the run's own STREAM-triad bandwidth on a shape that does not fit a cache
    Bb, Sb, Kb, hopb = 64, 1 << 20, (1 << 20) // 64 + 1, 64
    n = 64 << 20
    ta, tb_, tc = (torch.empty(n, device=dev) for _ in range(3))
    tb_.fill_(1.0), tc.fill_(2.0)
    triad = lambda: _hip.check(L.ds_stream_triad(p(ta), p(tb_), p(tc), n, 3.0, st), "ds_stream_triad")
    fwd, bwd = _delay_calls(L, p, st, Bb, Sb, Kb, hopb, g, dev)
    st_, sf, _ = _compare(triad, fwd, max(args.runs // 3, 5), batch=4)
    _, sfb, _ = _compare(triad, both(fwd, bwd), max(args.runs // 3, 5), batch=4)
    triad_gbs = 3 * n * 4 / st_["median"] / 1e6
    fwd_gbs = 8 * Bb * Sb / sf["median"] / 1e6
    result["large"] = dict(rows=Bb, S=Sb, K=Kb, hop=hopb, forward=sf, forward_backward=sfb, triad=st_, triad_gb_s=triad_gbs,
                           forward_gb_s=fwd_gbs, forward_fraction_of_triad=fwd_gbs / triad_gbs)
    print(f"large: fwd {sf['median']:.3f} ms = {fwd_gbs:.0f} GB/s of 8 B S, triad {triad_gbs:.0f} GB/s, fraction "
          f"{fwd_gbs / triad_gbs:.3f}; fwd+bwd {sfb['median']:.3f} ms")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
