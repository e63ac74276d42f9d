"""Times of the friction kernels (csrc/friction.hip) for the record, not a gate: forward and forward + backward of
``friction_force`` at m = 64, R = 8, F in {512, 32000}, A in {1, 8, 64} (medians of 50 at F = 512, of 5 at F = 32000, device
events), per substep; and beside them ``contact_force`` (csrc/contact.hip) at the same m, F = 512 and R from the same run.
Writes profiles/friction_bench.json.

The comparison shows what checkpointing costs.  The hammer's backward records every substep (two passes over the substeps:
the recording forward and the reverse sweep); the bow's keeps the state only where a sample begins and re-runs each sample
before it walks it backwards (three passes), for a workspace that does not grow with R - also reported, for both.

    python tools/friction_bench.py [--out profiles/friction_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from diffsound_amd import _hip  # noqa: E402
from diffsound_amd.ddsp import contact_force, friction_force  # noqa: E402

SR, M_MODES, R, P = 44100.0, 64, 8, 1.5


def modes(rng):
    w = 2 * np.pi * np.sort(rng.uniform(200.0, 9000.0, M_MODES))
    return 0.5 * (5.0 + 1e-7 * w * w), w


def bow_operands(A, F, dev):
    """A stroke at 1.5 times the friction peak under 60 N on an object of about a kilogram at the contact."""
    rng = np.random.default_rng(A)
    d, w = modes(rng)
    t = lambda x: torch.from_numpy(np.asarray(x, dtype=np.float64)).to(dev)  # noqa: E731
    c = rng.uniform(0.5, 1.5, (A, M_MODES)) / np.sqrt(M_MODES)
    return t(d), t(w), t(c), t(np.full((A, F), 0.15)), t(np.full((A, F), 60.0)), t(np.full(A, 0.1))


def hammer_operands(A, dev):
    rng = np.random.default_rng(A)
    d, w = modes(rng)
    t = lambda x: torch.from_numpy(np.asarray(x, dtype=np.float64)).to(dev)  # noqa: E731
    return (t(d), t(w), t(rng.uniform(0.5, 1.5, (A, M_MODES))), t(np.full(A, 0.01)), t(rng.uniform(0.5, 2.0, A)),
            t(np.full(A, 1e7)))


def median_ms(fn, reps):
    for _ in range(2):
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
    return statistics.median(times)


def timed(call, ops, A, F, reps, dev):
    lead = [x.clone().requires_grad_(True) for x in ops]
    g = torch.randn(A, F, device=dev)
    fwd = median_ms(lambda: call(*ops), reps)

    def both():
        for x in lead:
            x.grad = None
        call(*lead).backward(g)

    fb = median_ms(both, reps)
    steps = F * R
    return dict(A=A, m=M_MODES, F=F, R=R, reps=reps, fwd_ms=fwd, fwd_bwd_ms=fb, fwd_ns_per_substep=1e6 * fwd / steps,
                bwd_ns_per_substep=1e6 * (fb - fwd) / steps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "friction_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device: a timing taken elsewhere says nothing"
    dev = torch.device("cuda:0")
    lib = _hip.lib()
    friction, contact = [], []
    for F, reps in ((512, 50), (32000, 5)):
        for A in (1, 8, 64):
            row = timed(lambda *o: friction_force(*o, SR, R), bow_operands(A, F, dev), A, F, reps, dev)
            row["workspace_bytes"] = lib.ds_friction_workspace_bytes(A, M_MODES, F, R)
            friction.append(row)
            print("friction", row)
    for A in (1, 8, 64):
        row = timed(lambda *o: contact_force(*o, 512, SR, P, R), hammer_operands(A, dev), A, 512, 50, dev)
        row["workspace_bytes"] = lib.ds_contact_workspace_bytes(A, M_MODES, 512, R)
        contact.append(row)
        print("contact", row)
    result = dict(device=torch.cuda.get_device_name(0), friction=friction, contact=contact,
                  note="one wavefront per clip: latency-bound, time per substep is the figure; the friction backward is the "
                       "recording forward, the re-run and the reverse walk (three passes), the contact backward two")
    print(json.dumps(result))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
