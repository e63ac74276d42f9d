"""Timing record of the native Sinkhorn divergence (csrc/sinkhorn.hip through diffsound_amd/ddsp/sinkhorn.py).

Per call, at B in {1, 8} and N = M in {513, 1025} (n_fft 1024 / 2048) for the linear and the log/40 point clouds of
rendered clips (``spec2point``, blur 0.01 as the reference's spectral loss): the native forward and forward+backward
against the torch tensorized formulation of the same algorithm on the device (tests/_sinkhorn_ref.torch_geomloss:
expanded cost, torch.logsumexp, autograd through the last step).  Device events around each call, median of ``--reps``
calls after ``--warmup``.  ``native_not_slower`` is the one pass/fail condition: the native call is not slower than
the torch formulation in the same run.

``epoch``: one epoch of experiments/material_sync_train.py's loop on the bowl mesh (tests/golden/g0_bowl_mesh.npz,
16 modes, order 1) - get_undamped_freqs -> TraditionalDampedOscillator -> loss -> backward -> Adam step, without the
eigendecomposition that runs every 15 epochs - with the early-phase loss (MSSLoss([2048, 1024], type='geomloss') on
this solver) and the late-phase loss (MSSLoss([1024, 512, 256, 128, 64], type='l1_loss')), in the same process.
Writes one JSON document (``--out``, default stdout)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "compat"))  # the material loop's 'geomloss' loss takes this solver

DEV = torch.device("cuda:0")
SR = 32000
BLUR = 0.01


def clips(B, shift):
    from diffsound_amd.ddsp.oscillator import TraditionalDampedOscillator
    from diffsound_amd.diffelastic.material_model import Material, MatSet

    force = torch.zeros((1, 150), device=DEV)
    force[0, 0] = 1
    osc = TraditionalDampedOscillator(force, 1, 16, 8000, SR, Material(MatSet.Ceramic))
    return torch.cat([osc(torch.linspace(400, 9000, 16, device=DEV).reshape(-1, 1) * (1 + 0.013 * k) * shift)
                      .detach().reshape(1, -1) for k in range(B)])


def cloud(c, n_fft, kind):
    from diffsound_amd.ddsp.mss_loss import SSSLoss, normlize, spec2point

    s = SSSLoss(n_fft, SR)
    x = normlize(c)
    return spec2point(s.spec(x) if kind == "lin" else s.log_spec(x, 1.0) / 40).contiguous()


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return float(np.median(out))


def call_cases(reps, warmup):
    import _sinkhorn_ref as ref
    from diffsound_amd.ddsp.sinkhorn import schedule, sinkhorn_divergence

    rows = []
    for B in (1, 8):
        cp, ct = clips(B, 1.02), clips(B, 1.0)
        for n_fft in (1024, 2048):
            for kind in ("lin", "log"):
                x, y = cloud(cp, n_fft, kind), cloud(ct, n_fft, kind)
                xg = x.clone().requires_grad_(True)

                def nat_fwd():
                    with torch.no_grad():
                        sinkhorn_divergence(x, y, blur=BLUR)

                def nat_fb():
                    S = sinkhorn_divergence(xg, y, blur=BLUR)
                    torch.autograd.grad(S.sum(), [xg])

                def tor_fwd():
                    ref.torch_geomloss(x, y, blur=BLUR, grad=False)

                def tor_fb():
                    ref.torch_geomloss(x, y, blur=BLUR)

                r = dict(B=B, N=int(x.shape[1]), M=int(y.shape[1]), D=int(x.shape[2]), kind=kind,
                         steps=len(schedule(x, y, blur=BLUR)[1]),
                         native_fwd_ms=timed(nat_fwd, reps, warmup), native_fwd_bwd_ms=timed(nat_fb, reps, warmup),
                         torch_fwd_ms=timed(tor_fwd, reps, warmup), torch_fwd_bwd_ms=timed(tor_fb, reps, warmup))
                r["speedup_fwd"] = r["torch_fwd_ms"] / r["native_fwd_ms"]
                r["speedup_fwd_bwd"] = r["torch_fwd_bwd_ms"] / r["native_fwd_bwd_ms"]
                r["native_not_slower"] = bool(r["native_fwd_ms"] <= r["torch_fwd_ms"]
                                              and r["native_fwd_bwd_ms"] <= r["torch_fwd_bwd_ms"])
                print(json.dumps(r), file=sys.stderr, flush=True)
                rows.append(r)
    return rows


def epoch_times(reps, warmup):
    from torch.optim import Adam

    from src.ddsp.mss_loss import MSSLoss
    from src.ddsp.oscillator import TraditionalDampedOscillator
    from src.diffelastic.diff_model import Material, build_model

    m = np.load(os.path.join(ROOT, "tests", "golden", "g0_bowl_mesh.npz"))
    v = torch.from_numpy(m["verts"]).to(DEV)
    t = torch.from_numpy(m["tets"]).long().to(DEV)
    modes = 16
    gt_mat, init_mat = (2700.0, 6.0e10, 0.25, 6.0, 1e-7), (2700.0, 4.0e10, 0.3, 6.0, 1e-7)
    forces = torch.zeros((1, 150), device=DEV)
    forces[0, 0] = 1
    gt = build_model(None, modes, 1, gt_mat, "gt", vertices=v, tets=t)
    gt.eigen_decomposition()
    gt_audio = TraditionalDampedOscillator(forces, 1, modes, 8000, SR, Material(gt_mat)).cuda()(
        gt.get_undamped_freqs().float())
    torch.manual_seed(0)
    model = build_model(None, modes, 1, init_mat, "material", vertices=v, tets=t)
    model.eigen_decomposition()
    osc = TraditionalDampedOscillator(forces, len(gt_audio), modes, 8000, SR, Material(init_mat)).cuda()
    early = MSSLoss([2048, 1024], SR, type="geomloss").cuda()
    late = MSSLoss([1024, 512, 256, 128, 64], SR, type="l1_loss").cuda()
    opt = Adam(model.parameters(), lr=5e-3)

    def epoch(loss_fn):
        def run():
            pred = osc(model.get_undamped_freqs().float())
            loss = loss_fn(pred, gt_audio, osc.damped_freq, 1)
            opt.zero_grad()
            loss.backward()
            opt.step()
        return run

    out = {}
    for name, fn in (("early_geomloss_ms", early), ("late_l1_ms", late)):
        run = epoch(fn)
        for _ in range(warmup):
            run()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            run()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        out[name] = float(np.median(ts))
    out["early_over_late"] = out["early_geomloss_ms"] / out["late_l1_ms"]
    print(json.dumps(out), file=sys.stderr, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    rec = dict(device=torch.cuda.get_device_name(0), reps=args.reps, warmup=args.warmup, blur=BLUR,
               timing="device events around each call (epoch: host clock with a synchronise), median",
               calls=call_cases(args.reps, args.warmup), epoch=epoch_times(args.reps, args.warmup))
    rec["native_not_slower_everywhere"] = all(r["native_not_slower"] for r in rec["calls"])
    text = json.dumps(rec, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    else:
        print(text)


if __name__ == "__main__":
    main()
