"""Filtered-noise branch: device activities and time per call, native kernels against another oscillator.py.

    python tools/filtered_noise_bench.py [--other PATH/TO/oscillator.py] [--out profiles/filtered_noise_bench.txt]

Two workloads, forward + backward each:
  noise    FilteredNoise(8, 32000)().pow(2).mean().backward()
  prefit   one damping pre-fit step of experiments/material_real_train.py:117-123 at the shapes of
           tests/test_api_gpu.py's pre-fit loop: GTDampedOscillator(1 clip, 48 modes, 8000 samples)(noise_rate=2e-4) into
           MSSLoss([512, 256, 128, 64, 32], l1_loss), backward, Adam step.
``--other`` names a second version of diffsound_amd/ddsp/oscillator.py (e.g. ``git show HEAD~1:diffsound_amd/ddsp/oscillator.py``
saved to a file); it is loaded beside the package's own on the same library build - every kernel other than the noise branch is
the same code - and the two are timed ALTERNATELY in one process.  (A version from before the file was split is self-contained; a
later one imports ``FilteredNoise`` from ddsp/filtered_noise.py, so name a version of that file's era.)  Time: HIP events around ``--calls`` calls, per call, median
(min) over ``--rounds`` rounds after a warm-up.  Device activities: torch's kernel tracer on one call."""
import argparse
import importlib.util
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def load_oscillator(path):
    import diffsound_amd.ddsp.oscillator as own

    if path is None:
        return own
    spec = importlib.util.spec_from_file_location("diffsound_amd.ddsp._other_oscillator", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def workloads(osc_mod, dev):
    from diffsound_amd.ddsp.mss_loss import MSSLoss
    from diffsound_amd.diffelastic.material_model import Material

    torch.manual_seed(0)
    fnz = osc_mod.FilteredNoise(8, 32000).to(dev)

    def noise():
        fnz.zero_grad(set_to_none=True)
        fnz().pow(2).mean().backward()

    S, sr, modes = 8000, 32000, 48
    forces = torch.zeros((1, 150), device=dev)
    forces[0, 0] = 1
    late = MSSLoss([512, 256, 128, 64, 32], sr, type="l1_loss").to(dev)
    pre = osc_mod.GTDampedOscillator(forces, 1, modes, S, sr, [20, 16000], Material((2700.0, 5.5e10, 0.25, 6.0, 1e-7))).to(dev)
    opt = torch.optim.Adam(pre.parameters(), lr=5e-3)
    t = torch.arange(S, device=dev) / sr
    target = (torch.exp(-40 * t) * torch.sin(2 * torch.pi * 880 * t)).reshape(1, S)

    def prefit():
        loss = late(pre(noise_rate=2e-4), target)
        opt.zero_grad()
        loss.backward()
        opt.step()

    return dict(noise=noise, prefit=prefit)


def time_per_call(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def activities(fn):
    from torch.profiler import ProfilerActivity, profile

    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    ev = [e for e in prof.events() if "cuda" in str(getattr(e, "device_type", "")).lower()]
    own = [e.name for e in ev if "filtered_noise" in e.name]
    return len(ev), own


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=9)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device")
    dev = torch.device("cuda:0")
    sides = {"native": workloads(load_oscillator(None), dev)}
    if args.other:
        sides["other"] = workloads(load_oscillator(args.other), dev)
    lines = [f"# FilteredNoise(8, 32000) forward + backward, and one GTDampedOscillator pre-fit step (1 clip, 48 modes, S = 8000, "
             f"noise_rate 2e-4, MSSLoss l1, Adam); {torch.cuda.get_device_name(0)}",
             f"# ms per call: median (min) of {args.rounds} rounds of {args.calls} calls, HIP events, sides alternated; device "
             "activities of one call (torch kernel tracer)",
             f"# {'workload':>8} {'side':>7} {'activities':>10} {'ms / call':>18}  filtered-noise kernels"]
    for name in ("noise", "prefit"):
        for side in sides.values():  # warm-up of every shape
            for _ in range(5):
                side[name]()
        torch.cuda.synchronize()
        times = {k: [] for k in sides}
        for _ in range(args.rounds):
            for k, side in sides.items():
                times[k].append(time_per_call(side[name], args.calls))
        for k, side in sides.items():
            n, own = activities(side[name])
            lines.append(f"  {name:>8} {k:>7} {n:>10d} {statistics.median(times[k]):>9.4f} ({min(times[k]):.4f})  "
                         + (", ".join(o[:72] for o in own) or "-"))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
