"""Forward and forward + backward times of the feedback delay network (ds_fdn_fwd / _bwd, csrc/fdn.hip) at B in {1, 8, 64}
rows, N = 32000 samples, n in {4, 8, 16} lines at the module's default delays (20 ms to 100 ms: blocks of 256 samples), and one
row set with every delay near the minimum of 64 (500 blocks), beside
  (a) the tail it replaces: ds_fir_fwd / _bwd on the same rows with L = N free taps, and
  (b) what one would write in torch: a frequency-sampling FDN - rfft of the row zero-padded to 2 N, times the module's
      closed-form ``response`` on that grid, irfft - forward + backward through autograd.  It aliases the tail in time and is
      here for its time only.
A timed window is 5 back-to-back calls on preallocated buffers between two HIP events; the FDN and a baseline are
ALTERNATED window by window, after warm-up, --runs windows each: median, minimum and spread (p10 .. p90) of both, and the
median of the per-pair ratios.  Time is reported, not gated.

    python tools/mb_fdn.py [--runs 20] [--out profiles/fdn_bench.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diffsound_amd import _hip  # noqa: E402
from diffsound_amd.ddsp.fdn import FeedbackDelayNetwork  # noqa: E402
from mb_fir import BATCH, _compare  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--out", default=os.path.join("profiles", "fdn_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mb_fdn: needs a HIP device")
    dev = torch.device("cuda:0")
    lib, p, st = _hip.lib(), _hip.ptr, _hip.stream_ptr()
    g = torch.Generator().manual_seed(0)
    N, sr = 32000, 32000.0
    result = dict(device=torch.cuda.get_device_name(0), runs=args.runs, calls_per_window=BATCH, unit="ms per call", N=N, fdn=[])
    shapes = [(B, n, None) for n in (4, 8, 16) for B in (1, 8, 64)] + [(8, 8, list(range(64, 72)))]
    for B, n, delays in shapes:
        net = FeedbackDelayNetwork(1, n, sr, 0.5, delays=delays, damp=0.1, wet_db=-12.0, init="wet").to(dev)
        A, b, c, d, pd = (t.detach().contiguous() for t in net.coefficients())
        m = net.delays
        x, gy = torch.randn((B, N), generator=g).to(dev), torch.randn((B, N), generator=g).to(dev)
        y, gx = torch.empty_like(x), torch.empty_like(x)
        state = torch.empty((B, n, N), dtype=torch.float64, device=dev)
        gA, gb, gc, gd, gp = (torch.empty_like(t) for t in (A, b, c, d, pd))
        nb = lib.ds_fdn_workspace_bytes(B, 1, N, n)
        work = torch.empty(nb, dtype=torch.uint8, device=dev)
        fwd = lambda: _hip.check(lib.ds_fdn_fwd(p(x), p(m), p(A), p(b), p(c), p(d), p(pd), B, 1, N, n, p(state), p(y), st), "ds_fdn_fwd")
        bwd = lambda: _hip.check(lib.ds_fdn_bwd(p(gy), p(x), p(m), p(A), p(b), p(c), p(d), p(pd), B, 1, N, n, p(state), p(work), nb,
                                                p(gx), p(gA), p(gb), p(gc), p(gd), p(gp), st), "ds_fdn_bwd")
        # (a) the FIR of L = N taps on the same rows
        h = (torch.randn((1, N), generator=g, dtype=torch.float64) / N ** 0.5).to(dev)
        gh = torch.empty_like(h)
        nbf = lib.ds_fir_workspace_bytes(B, 1, N, N)
        workf = torch.empty(nbf, dtype=torch.uint8, device=dev)
        fir_fwd = lambda: _hip.check(lib.ds_fir_fwd(p(x), p(h), B, 1, N, N, p(y), st), "ds_fir_fwd")
        fir_bwd = lambda: _hip.check(lib.ds_fir_bwd(p(gy), p(x), p(h), B, 1, N, N, p(workf), nbf, p(gx), p(gh), st), "ds_fir_bwd")
        # (b) frequency sampling in torch
        xr = x.clone().requires_grad_(True)
        freqs = torch.arange(N + 1, dtype=torch.float64, device=dev) * sr / (2 * N)

        def sampled():
            return torch.fft.irfft(torch.fft.rfft(xr, 2 * N) * net.response(freqs).to(torch.complex64), 2 * N)[..., :N]

        def torch_fwd():
            with torch.no_grad():
                sampled()

        def torch_both():
            xr.grad = None
            net.zero_grad(set_to_none=True)
            sampled().backward(gy)

        blocks = -(-N // min(int(m.min()), 256))
        row = dict(B=B, n=n, N=N, min_delay=int(m.min()), max_delay=int(m.max()), blocks=blocks, workspace_bytes=nb,
                   state_bytes=8 * B * n * N)
        for key, fn, fir_fn, torch_fn in (("forward", fwd, fir_fwd, torch_fwd),
                                          ("forward_backward", lambda: (fwd(), bwd()), lambda: (fir_fwd(), fir_bwd()), torch_both)):
            sa, sf, ra = _compare(fir_fn, fn, args.runs)
            sb, sf2, rb = _compare(torch_fn, fn, args.runs)
            row[key] = dict(sf, again=sf2, fir_full_length=sa, ratio_to_fir=ra, torch_sampled=sb, ratio_to_torch_sampled=rb,
                            us_per_block=1e3 * sf["median"] / blocks / (1 if key == "forward" else 2))
        result["fdn"].append(row)
        f_, fb = row["forward"], row["forward_backward"]
        print(f"B {B:>2} n {n:>2} m {row['min_delay']:>3}..{row['max_delay']:<4}  fwd {f_['median']:.4f} ms (fir {f_['fir_full_length']['median']:.4f}, "
              f"x{f_['ratio_to_fir']:.3f}; torch {f_['torch_sampled']['median']:.4f}, x{f_['ratio_to_torch_sampled']:.3f}; "
              f"{f_['us_per_block']:.2f} us/block)  fwd+bwd {fb['median']:.4f} ms (fir {fb['fir_full_length']['median']:.4f}, "
              f"x{fb['ratio_to_fir']:.3f}; torch {fb['torch_sampled']['median']:.4f}, x{fb['ratio_to_torch_sampled']:.3f})", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
