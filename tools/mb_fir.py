"""Forward and forward + backward times of the long FIR (ds_fir_fwd / _bwd, csrc/fir.hip) at B in {2, 16} rows, N = 32000
samples, L in {2048, 16384, 65536} taps and H in {1, 2} responses, beside what one would write without it: torch's rfft /
irfft convolution in fp32 on the same inputs, forward + backward through autograd (zero-padded to the next power of two
above N + L - 1).  A timed window is 5 back-to-back calls on preallocated buffers between two HIP events; the two are
ALTERNATED window by window, after warm-up, --runs windows each: median, minimum and spread (p10 .. p90) of both, and the
median of the per-pair ratios.  Every shape also reports the fp64 multiply-add rate the native kernels reach
(B (N Lc - Lc (Lc - 1) / 2) multiply-adds a sum, Lc = min(L, N); three sums forward + backward).  Time is reported, not gated.

    python tools/mb_fir.py [--runs 20] [--out profiles/fir_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diffsound_amd import _hip  # noqa: E402

BATCH = 5  # calls per timed window


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


def _compare(base_fn, fn, runs, warmup=2):
    """The two ALTERNATED, window by window, so that clock and thermal drift reach both alike: (stats of the baseline, stats of
    fn, median of the per-pair ratios fn / baseline)."""
    for _ in range(warmup):
        _window_ms(base_fn)
        _window_ms(fn)
    torch.cuda.synchronize()
    tb, tf = [], []
    for _ in range(runs):
        tb.append(_window_ms(base_fn))
        tf.append(_window_ms(fn))
    return _stats(tb), _stats(tf), statistics.median(f / b for f, b in zip(tf, tb))


def fft_convolve(x, h):
    """The torch path: x (B, N), h (H, L) fp32 -> (B, N), causal, cut at N."""
    N, L = x.shape[-1], h.shape[-1]
    n = 1 << (N + L - 2).bit_length()
    spec = torch.fft.rfft(x, n) * torch.fft.rfft(h, n).repeat(x.shape[0] // h.shape[0], 1)
    return torch.fft.irfft(spec, n)[..., :N]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--out", default=os.path.join("profiles", "fir_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mb_fir: needs a HIP device")
    dev = torch.device("cuda:0")
    lib, p, st = _hip.lib(), _hip.ptr, _hip.stream_ptr()
    g = torch.Generator().manual_seed(0)
    N = 32000
    result = dict(device=torch.cuda.get_device_name(0), runs=args.runs, calls_per_window=BATCH, unit="ms per call", N=N, fir=[])
    for L in (2048, 16384, 65536):
        for B in (2, 16):
            for H in (1, 2):
                x, gy = torch.randn((B, N), generator=g).to(dev), torch.randn((B, N), generator=g).to(dev)
                h = (torch.randn((H, L), generator=g, dtype=torch.float64) / L ** 0.5).to(dev)
                y, gx, gh = torch.empty_like(x), torch.empty_like(x), torch.empty_like(h)
                nb = lib.ds_fir_workspace_bytes(B, H, N, L)
                work = torch.empty(nb, dtype=torch.uint8, device=dev)
                fwd = lambda: _hip.check(lib.ds_fir_fwd(p(x), p(h), B, H, N, L, p(y), st), "ds_fir_fwd")
                bwd = lambda: _hip.check(lib.ds_fir_bwd(p(gy), p(x), p(h), B, H, N, L, p(work), nb, p(gx), p(gh), st), "ds_fir_bwd")
                xr, hr = x.clone().requires_grad_(True), h.float().requires_grad_(True)

                def torch_fwd():
                    with torch.no_grad():
                        fft_convolve(xr, hr)

                def torch_both():
                    xr.grad = hr.grad = None
                    fft_convolve(xr, hr).backward(gy)

                Lc = min(L, N)
                fma = B * (N * Lc - Lc * (Lc - 1) // 2)
                row = dict(B=B, H=H, N=N, L=L, workspace_bytes=nb, multiply_adds_forward=fma)
                for key, base_fn, fn, sums in (("forward", torch_fwd, fwd, 1), ("forward_backward", torch_both, lambda: (fwd(), bwd()), 3)):
                    sb, sf, ratio = _compare(base_fn, fn, args.runs)
                    row[key] = dict(sf, torch_fft=sb, ratio_to_torch_fft=ratio, tera_fma_per_s=sums * fma / sf["median"] / 1e9)
                result["fir"].append(row)
                print(f"B {B:>2} H {H} L {L:>5}  fwd {row['forward']['median']:.4f} ms (fft {row['forward']['torch_fft']['median']:.4f}, "
                      f"x{row['forward']['ratio_to_torch_fft']:.2f}; {row['forward']['tera_fma_per_s']:.2f} Tfma/s)  fwd+bwd "
                      f"{row['forward_backward']['median']:.4f} ms (fft {row['forward_backward']['torch_fft']['median']:.4f}, "
                      f"x{row['forward_backward']['ratio_to_torch_fft']:.2f}; {row['forward_backward']['tera_fma_per_s']:.2f} Tfma/s)",
                      flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
