"""Times of the contact-force kernels (csrc/contact.hip) for the record, not a gate: forward and forward + backward of
``contact_force`` at A in {1, 8, 64}, m = 64, F = 512, R = 8 (medians of 50, device events), and the same force from a plain
torch loop over the substeps at A = 8, once.  Writes profiles/contact_bench.json.

One wavefront per clip and a time loop that is sequential by nature: with A waves on 256 compute units the kernels are
latency-bound, so the figure to read is the time per substep, given here in nanoseconds and in cycles at the 2.4 GHz peak
clock (an upper bound on the cycles: the clock under load is lower).

    python tools/contact_bench.py [--out profiles/contact_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from diffsound_amd.ddsp import contact_force  # noqa: E402

SR, M_MODES, F, R, P, REPS, CLOCK_GHZ = 44100.0, 64, 512, 8, 1.5, 50, 2.4


def operands(A, dev):
    rng = np.random.default_rng(A)
    w = 2 * np.pi * np.sort(rng.uniform(200.0, 9000.0, M_MODES))
    d = 0.5 * (5.0 + 1e-7 * w * w)
    t = lambda x: torch.from_numpy(np.asarray(x, dtype=np.float64)).to(dev)  # noqa: E731
    return (t(d), t(w), t(rng.uniform(0.5, 1.5, (A, M_MODES))), t(np.full(A, 0.01)), t(rng.uniform(0.5, 2.0, A)),
            t(np.full(A, 1e7)))


def median_ms(fn):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times)


def torch_loop(d, w, c, M, v0, kH):
    """The scheme as torch ops on the device, one substep after the other (about ten launches each)."""
    h = 1.0 / (SR * R)
    z = torch.exp(torch.complex(-d * h, w * h))
    kap = c * c / w
    A = c.shape[0]
    xh, vh = torch.zeros_like(v0), v0.clone()
    s = torch.zeros((A, M_MODES), dtype=torch.complex128, device=c.device)
    force = torch.zeros((A, F), dtype=torch.float64, device=c.device)
    for n in range(F * R):
        delta = xh - (kap * s.imag).sum(-1)
        f = kH * delta.clamp(min=0).pow(P)
        force[:, n // R] += f / R
        vh = vh - h * f / M
        xh = xh + h * vh
        s = z * (s + (h * f)[:, None])
    return force


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "contact_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device: a timing taken elsewhere says nothing"
    dev = torch.device("cuda:0")
    rows = []
    for A in (1, 8, 64):
        ops = operands(A, dev)
        lead = [x.clone().requires_grad_(True) for x in ops]
        g = torch.randn(A, F, device=dev)
        fwd = median_ms(lambda: contact_force(*ops, F, SR, P, R))

        def both():
            for x in lead:
                x.grad = None
            contact_force(*lead, F, SR, P, R).backward(g)

        fb = median_ms(both)
        steps = F * R
        rows.append(dict(A=A, m=M_MODES, F=F, R=R, fwd_ms=fwd, fwd_bwd_ms=fb, fwd_ns_per_substep=1e6 * fwd / steps,
                         fwd_cycles_per_substep_at_peak_clock=1e6 * fwd / steps * CLOCK_GHZ,
                         bwd_ns_per_substep=1e6 * (fb - fwd) / steps))
        print(rows[-1])
    ops = operands(8, dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ref = torch_loop(*ops)
    torch.cuda.synchronize()
    loop_ms = 1e3 * (time.perf_counter() - t0)
    got = contact_force(*ops, F, SR, P, R).double()
    result = dict(device=torch.cuda.get_device_name(0), reps=REPS, rows=rows, torch_loop_A8_ms_once=loop_ms,
                  torch_loop_max_abs_diff_over_peak=float((got - ref).abs().max() / ref.abs().max()),
                  note="one wavefront per clip: latency-bound, time per substep is the figure; cycles at the 2.4 GHz peak clock")
    print(json.dumps(result))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
