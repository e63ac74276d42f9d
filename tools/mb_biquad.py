"""Forward and forward + backward times of the biquad cascade (ds_biquad_fwd / _bwd, csrc/biquad.hip) at B in {1, 8, 64} rows,
N in {32000, 160000} samples and S in {1, 4} sections, beside the delay line (ds_delay_fwd / _bwd, K = 1: a constant delay)
on the same B x N rows - the other operator that takes a rendered row to a rendered row - and beside ds_stream_triad.
A timed window is 20 back-to-back calls on preallocated buffers between two HIP events; the delay line and the cascade are
ALTERNATED window by window, after warm-up, --runs windows each: median, minimum and spread (p10 .. p90) of both, and the
median of the per-pair ratios.  Every shape also reports the fraction of the triad's bandwidth, measured in the same run,
that the forward's algorithmic bytes (read x, write y: 8 B N) reach.  Time is reported, not gated.

    python tools/mb_biquad.py [--runs 30] [--out profiles/biquad_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diffsound_amd import _hip  # noqa: E402
from diffsound_amd.ddsp.biquad import highpass_coeffs, peaking_coeffs  # noqa: E402

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--out", default=os.path.join("profiles", "biquad_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mb_biquad: needs a HIP device")
    dev = torch.device("cuda:0")
    L, p, st = _hip.lib(), _hip.ptr, _hip.stream_ptr()
    g = torch.Generator().manual_seed(0)
    sr = 32000.0
    n = 64 << 20
    ta, tb_, tc = (torch.empty(n, device=dev) for _ in range(3))
    tb_.fill_(1.0), tc.fill_(2.0)
    triad = lambda: _hip.check(L.ds_stream_triad(p(ta), p(tb_), p(tc), n, 3.0, st), "ds_stream_triad")
    both = lambda f, b: (lambda: (f(), b()))
    result = dict(device=torch.cuda.get_device_name(0), runs=args.runs, calls_per_window=BATCH, unit="ms per call", biquad=[])
    _, s_tri, _ = _compare(triad, triad, max(args.runs // 3, 5), batch=4)
    result["triad"] = dict(s_tri, gb_s=3 * n * 4 / s_tri["median"] / 1e6)
    for N in (32000, 160000):
        for B in (1, 8, 64):
            x, gy = torch.randn((B, N), generator=g).to(dev), torch.randn((B, N), generator=g).to(dev)
            y, gx = torch.empty_like(x), torch.empty_like(x)
            tau = torch.full((B, 1), 40.25, dtype=torch.float64, device=dev)
            gtau = torch.empty_like(tau)
            nbd = L.ds_delay_workspace_bytes(B, N, 1, 16)
            wd = torch.empty(nbd, dtype=torch.uint8, device=dev)
            dfwd = lambda: _hip.check(L.ds_delay_fwd(p(x), p(tau), B, N, 1, 16, p(y), st), "ds_delay_fwd")
            dbwd = lambda: _hip.check(L.ds_delay_bwd(p(gy), p(x), p(tau), B, N, 1, 16, p(wd), nbd, p(gx), p(gtau), st), "ds_delay_bwd")
            for S in (1, 4):
                sos = torch.cat([highpass_coeffs(sr, 100.0).reshape(1, 5),
                                 peaking_coeffs(sr, torch.tensor([400.0, 2500.0, 9000.0]), 1.2, torch.tensor([3.0, -4.0, 2.0]))])[:S]
                sos = sos.contiguous().to(dev)
                gsos = torch.empty((B, S, 5), dtype=torch.float64, device=dev)
                nb = L.ds_biquad_workspace_bytes(B, N, S)
                work = torch.empty(nb, dtype=torch.uint8, device=dev)
                fwd = lambda: _hip.check(L.ds_biquad_fwd(p(x), p(sos), 0, B, N, S, p(y), st), "ds_biquad_fwd")
                bwd = lambda: _hip.check(L.ds_biquad_bwd(p(gy), p(x), p(sos), 0, B, N, S, p(work), nb, p(gx), p(gsos), st),
                                         "ds_biquad_bwd")
                row = dict(B=B, N=N, S=S)
                for key, base_fn, fn in (("forward", dfwd, fwd), ("forward_backward", both(dfwd, dbwd), both(fwd, bwd))):
                    sb, sf, ratio = _compare(base_fn, fn, args.runs)
                    row[key] = dict(sf, delay=sb, ratio_to_delay=ratio)
                gbs = 8 * B * N / row["forward"]["median"] / 1e6
                row["forward_gb_s"] = gbs
                row["forward_fraction_of_triad"] = gbs / result["triad"]["gb_s"]
                result["biquad"].append(row)
                print(f"B {B:>2} N {N:>6} S {S}  fwd {row['forward']['median']:.4f} ms (delay {row['forward']['delay']['median']:.4f}, "
                      f"x{row['forward']['ratio_to_delay']:.2f}; {gbs:.2f} GB/s = {row['forward_fraction_of_triad']:.5f} of triad)  fwd+bwd "
                      f"{row['forward_backward']['median']:.4f} ms (delay {row['forward_backward']['delay']['median']:.4f}, "
                      f"x{row['forward_backward']['ratio_to_delay']:.2f})", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
