"""The native Sinkhorn divergence (csrc/sinkhorn.hip through diffsound_amd/ddsp/sinkhorn.py) against the fp64 oracle of
tests/_sinkhorn_ref.py, its identities, determinism, gradient, and the spectral loss of the material scripts end to end.

Tolerance (measured, not fixed in advance): on the same inputs, ``_sinkhorn_ref.torch_geomloss`` - geomloss's
tensorized arithmetic in fp32 torch on the device (expanded cost, torch.logsumexp, autograd) - is compared with the
fp64 oracle; its largest relative error over every case is the fp32 error level of the reference algorithm, separately
for the loss and the gradient.  The kernel's bound is 4x that level (the margin of tests/test_meshsdf_gpu.py).  Levels
measured on the MI355X: loss 2.21e-5, gradient 5.52e-4 - so the bounds are 8.85e-5 and 2.21e-3;
the kernel's own largest errors were loss 1.99e-5, gradient 5.36e-4 (both on the linear n_fft=2048 clouds: spectrum-scale
coordinates, smallest eps 1e-4).  The test recomputes the levels on every run."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _sinkhorn_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR = 32000
BLUR = 0.01  # what the reference's spectral loss passes


def _clips(B, shift):
    """B rendered clips of 8000 samples (the material scripts' frame count), each with its own 16 modes."""
    from diffsound_amd.ddsp.oscillator import TraditionalDampedOscillator
    from diffsound_amd.diffelastic.material_model import Material, MatSet

    force = torch.zeros((1, 150), device=DEV)
    force[0, 0] = 1
    osc = TraditionalDampedOscillator(force, 1, 16, 8000, SR, Material(MatSet.Ceramic))
    out = []
    for k in range(B):
        f = torch.linspace(400, 9000, 16, device=DEV).reshape(-1, 1) * (1 + 0.013 * k) * shift
        out.append(osc(f).detach().reshape(1, -1))
    return torch.cat(out)


def _spec_cloud(clips, n_fft, kind, scale=1.0):
    from diffsound_amd.ddsp.mss_loss import SSSLoss, normlize, spec2point

    s = SSSLoss(n_fft, SR)
    x = normlize(clips)
    sp = s.spec(x) if kind == "lin" else s.log_spec(x, scale) / 40
    return spec2point(sp).contiguous()


def _rel_loss(S, S64):
    S = np.asarray(S, np.float64)
    return float((np.abs(S - S64) / np.abs(S64)).max())


def _rel_grad(gs, g64s):
    num = max(np.abs(np.asarray(g, np.float64) - g64).max() for g, g64 in zip(gs, g64s))
    return float(num / max(np.abs(g64).max() for g64 in g64s))


def _native(x, y, a=None, b=None, blur=BLUR, **kw):
    from diffsound_amd.ddsp.sinkhorn import sinkhorn_divergence

    x = x.detach().clone().requires_grad_(True)
    y = y.detach().clone().requires_grad_(True)
    S = sinkhorn_divergence(x, y, a, b, blur=blur, **kw)
    gx, gy = torch.autograd.grad(S.sum(), [x, y])
    return S.detach(), gx, gy


def _cases():
    """(name, x, y, a, b, blur): spectral clouds of the scripts' shapes and random clouds with N != M."""
    cases = []
    spec = [(2048, "lin", 1.0, 8), (2048, "log", 1.0, 3), (2048, "log", 0.5, 1), (1024, "lin", 1.0, 3),
            (1024, "log", 1.0, 1), (1024, "log", 0.5, 8), (2048, "lin", 1.0, 1), (1024, "log", 1.0, 8)]
    for n_fft, kind, scale, B in spec:
        x = _spec_cloud(_clips(B, 1.02), n_fft, kind, scale)
        y = _spec_cloud(_clips(B, 1.0), n_fft, kind, scale)
        cases.append((f"{kind}{'' if scale == 1 else scale} n_fft={n_fft} B={B} N={x.shape[1]}", x, y, None, None, BLUR))
    rng = np.random.default_rng(7)
    for B, N, M, D in ((3, 200, 150, 2), (1, 333, 517, 7), (8, 64, 100, 4)):
        x = torch.from_numpy(rng.standard_normal((B, N, D)).astype(np.float32)).to(DEV)
        y = torch.from_numpy((rng.standard_normal((B, M, D)) * 0.7 + 0.3).astype(np.float32)).to(DEV)
        a = rng.uniform(0.2, 1.0, (B, N))
        b = rng.uniform(0.2, 1.0, (B, M))
        a = torch.from_numpy((a / a.sum(1, keepdims=True)).astype(np.float32)).to(DEV)
        b = torch.from_numpy((b / b.sum(1, keepdims=True)).astype(np.float32)).to(DEV)
        cases.append((f"random B={B} N={N} M={M} D={D}", x, y, a, b, 0.05))
    return cases


@pytest.fixture(scope="module")
def parity():
    """Every case: the oracle, the fp32 torch restatement and the kernel; the levels and the kernel's errors."""
    from diffsound_amd.ddsp.sinkhorn import schedule

    rows = []
    for name, x, y, a, b, blur in _cases():
        an = None if a is None else a.cpu().numpy()
        bn = None if b is None else b.cpu().numpy()
        S64, gx64, gy64, eps64, _ = ref.oracle(x.cpu().numpy(), y.cpu().numpy(), an, bn, blur=blur)
        d64 = ref.diameter(x.cpu().numpy(), y.cpu().numpy())
        d, eps = schedule(x, y, a, b, blur=blur)
        assert d == d64 and len(eps) == len(eps64), (name, d, d64)
        St, gxt, gyt = ref.torch_geomloss(x, y, a, b, blur=blur, diameter_=d64)
        Sn, gxn, gyn = _native(x, y, a, b, blur=blur)
        r = dict(name=name, steps=len(eps64),
                 torch_loss=_rel_loss(St.cpu().numpy(), S64),
                 torch_grad=_rel_grad([gxt.cpu().numpy(), gyt.cpu().numpy()], [gx64, gy64]),
                 kernel_loss=_rel_loss(Sn.cpu().numpy(), S64),
                 kernel_grad=_rel_grad([gxn.cpu().numpy(), gyn.cpu().numpy()], [gx64, gy64]))
        print("parity {name}: steps {steps}  torch fp32 loss {torch_loss:.2e} grad {torch_grad:.2e}  "
              "kernel loss {kernel_loss:.2e} grad {kernel_grad:.2e}".format(**r))
        rows.append(r)
    level_loss = max(r["torch_loss"] for r in rows)
    level_grad = max(r["torch_grad"] for r in rows)
    print(f"parity: level loss {level_loss:.3e} grad {level_grad:.3e}; bounds {4 * level_loss:.3e} {4 * level_grad:.3e}; "
          f"kernel max loss {max(r['kernel_loss'] for r in rows):.3e} grad {max(r['kernel_grad'] for r in rows):.3e}")
    return dict(rows=rows, loss_bound=4 * level_loss, grad_bound=4 * level_grad)


def test_parity_with_the_oracle(parity):
    for r in parity["rows"]:
        assert r["kernel_loss"] <= parity["loss_bound"], r
        assert r["kernel_grad"] <= parity["grad_bound"], r


def test_identical_clouds_give_exactly_zero():
    from diffsound_amd.ddsp.sinkhorn import sinkhorn_divergence

    for x in (_spec_cloud(_clips(3, 1.0), 1024, "lin"), _spec_cloud(_clips(2, 1.0), 2048, "log"),
              torch.randn(4, 129, 7, device=DEV)):
        S = sinkhorn_divergence(x, x.clone(), blur=BLUR)
        assert torch.equal(S, torch.zeros_like(S)), S


def test_translated_copy_and_two_diracs(parity):
    from diffsound_amd.ddsp.sinkhorn import sinkhorn_divergence

    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 129, 4, generator=g).to(DEV)
    t = torch.tensor([0.7, -0.3, 0.2, 1.1], device=DEV)
    S = sinkhorn_divergence(x, x + t, blur=0.05)
    want = float((t.double() ** 2).sum() / 2)
    err = float((S.double() - want).abs().max()) / want
    print(f"translated copy: S {S.tolist()} want {want} rel err {err:.2e}")
    assert err <= parity["loss_bound"]
    x1 = torch.tensor([[0.3, -1.2, 0.5]], device=DEV)
    y1 = torch.tensor([[1.1, 0.4, -0.7]], device=DEV)
    S1 = sinkhorn_divergence(x1, y1, blur=0.05)
    want1 = float(((x1.double() - y1.double()) ** 2).sum() / 2)
    err1 = abs(float(S1) - want1) / want1
    print(f"two Diracs: S {float(S1)} want {want1} rel err {err1:.2e}")
    assert S1.dim() == 0 and err1 <= parity["loss_bound"]


def test_determinism_and_batch_independence():
    from diffsound_amd.ddsp.sinkhorn import schedule

    x = _spec_cloud(_clips(8, 1.02), 1024, "log")
    y = _spec_cloud(_clips(8, 1.0), 1024, "log")
    S1, gx1, gy1 = _native(x, y)
    S2, gx2, gy2 = _native(x, y)
    assert torch.equal(S1, S2) and torch.equal(gx1, gx2) and torch.equal(gy1, gy2)
    d, eps = schedule(x, y, blur=BLUR)
    assert len(eps) == len(ref.eps_schedule(ref.diameter(x.cpu().numpy(), y.cpu().numpy()), BLUR, 0.5))
    for k in range(8):
        Sk, gxk, gyk = _native(x[k:k + 1], y[k:k + 1], diameter=d)
        assert torch.equal(Sk[0], S1[k]) and torch.equal(gxk[0], gx1[k]) and torch.equal(gyk[0], gy1[k]), k


def test_gradient_against_torch_autograd_and_finite_differences(parity):
    """The envelope gradient against (1) the torch restatement's autograd gradient on unit-scale clouds and (2) central
    differences of the CONVERGED fp64 loss, on the clouds and blur of the oracle's own finite-difference check
    (tests/test_sinkhorn_cpu.py).  For (2) the native loop is run to convergence through its schedule: a diameter a
    hair above blur and scaling just below 1 give ~100 averaged updates at eps = blur^2 (to fp32 rounding)."""
    g = torch.Generator().manual_seed(11)
    x = torch.randn(3, 150, 4, generator=g).to(DEV)
    y = (torch.randn(3, 170, 4, generator=g) * 0.8 + 0.2).to(DEV)
    _, gxn, gyn = _native(x, y, blur=0.05)
    _, gxt, gyt = ref.torch_geomloss(x, y, blur=0.05)
    err = _rel_grad([gxn.cpu().numpy(), gyn.cpu().numpy()], [gxt.cpu().double().numpy(), gyt.cpu().double().numpy()])
    print(f"gradient vs torch autograd: {err:.2e} (bound {parity['grad_bound']:.2e})")
    assert err <= parity["grad_bound"]

    rng = np.random.default_rng(3)  # the clouds and weights of the oracle's finite-difference test
    B, N, M, D = 1, 6, 5, 2
    xs, ys = rng.standard_normal((B, N, D)), rng.standard_normal((B, M, D))
    a = rng.uniform(0.5, 1.5, (B, N))
    b = rng.uniform(0.5, 1.5, (B, M))
    a /= a.sum(1, keepdims=True)
    b /= b.sum(1, keepdims=True)
    xs, ys = xs.astype(np.float32).astype(np.float64), ys.astype(np.float32).astype(np.float64)
    kw = dict(blur=0.5, diameter_=4.0, converge=True)
    h = 1e-5
    fds = []
    for arr in (xs, ys):
        fd = np.zeros_like(arr)
        for idx in np.ndindex(arr.shape):
            old = arr[idx]
            arr[idx] = old + h
            sp = ref.oracle(xs, ys, a, b, **kw)[0].sum()
            arr[idx] = old - h
            sm = ref.oracle(xs, ys, a, b, **kw)[0].sum()
            arr[idx] = old
            fd[idx] = (sp - sm) / (2 * h)
        fds.append(fd)
    t = lambda v: torch.from_numpy(v.astype(np.float32)).to(DEV)
    from diffsound_amd.ddsp.sinkhorn import schedule

    _, eps = schedule(t(xs), t(ys), t(a), t(b), blur=0.5, scaling=1 - 2e-9, diameter=0.5 * (1 + 2e-7))
    assert len(eps) >= 80
    _, gxn, gyn = _native(t(xs), t(ys), t(a), t(b), blur=0.5, scaling=1 - 2e-9, diameter=0.5 * (1 + 2e-7))
    err = _rel_grad([gxn.cpu().numpy(), gyn.cpu().numpy()], fds)
    print(f"gradient vs finite differences of the converged loss: {err:.2e} over {len(eps)} steps "
          f"(bound {parity['grad_bound']:.2e})")
    assert err <= parity["grad_bound"]


@pytest.fixture
def shim(monkeypatch):
    """compat/ in front of sys.path with geomloss dropped from sys.modules; restored afterwards."""
    saved = sys.modules.pop("geomloss", None)
    monkeypatch.syspath_prepend(os.path.join(ROOT, "compat"))
    yield
    sys.modules.pop("geomloss", None)
    if saved is not None:
        sys.modules["geomloss"] = saved


def test_mss_geomloss_end_to_end(parity, shim):
    """MSSLoss([2048, 1024], 32000, type='geomloss') on oscillator output, through the compat shim: finite, equal to
    alpha * log + lin from the oracle, and its gradient reaches the mode frequencies."""
    from diffsound_amd.ddsp.mss_loss import MSSLoss, normlize, spec2point
    from diffsound_amd.ddsp.oscillator import TraditionalDampedOscillator
    from diffsound_amd.diffelastic.material_model import Material, MatSet

    force = torch.zeros((1, 150), device=DEV)
    force[0, 0] = 1
    osc = TraditionalDampedOscillator(force, 1, 16, 8000, SR, Material(MatSet.Ceramic))
    f0 = torch.linspace(400, 9000, 16, device=DEV).reshape(-1, 1)
    target = osc(f0).detach()
    f = (f0 * 1.01).clone().requires_grad_(True)
    pred = osc(f)
    damped = osc.damped_freq
    m = MSSLoss([2048, 1024], SR, type="geomloss")
    loss = m(pred, target, damped, 1)
    assert torch.isfinite(loss)
    want = 0.0
    with torch.no_grad():
        for s in m.losses:
            np_, nt = normlize(pred), normlize(target)
            for sp, st, w in ((s.spec(np_), s.spec(nt), 1.0), (s.log_spec(np_, 1) / 40, s.log_spec(nt, 1) / 40, s.alpha)):
                S64 = ref.oracle(spec2point(sp, damped, SR).cpu().numpy(), spec2point(st).cpu().numpy(), blur=BLUR)[0]
                want += w * S64.sum()
    err = abs(float(loss.detach()) - want) / abs(want)
    print(f"MSSLoss geomloss: {float(loss.detach())} oracle {want} rel err {err:.2e}")
    assert err <= parity["loss_bound"]
    loss.backward()
    assert torch.isfinite(f.grad).all() and float(f.grad.abs().max()) > 0


def test_material_loop_early_phase_moves_the_material(golden, shim):
    """experiments/material_sync_train.py's early phase, shortened: build_model -> get_undamped_freqs ->
    TraditionalDampedOscillator -> MSSLoss([2048, 1024], type='geomloss') -> Adam.  E and nu move."""
    from torch.optim import Adam

    from src.ddsp.mss_loss import MSSLoss
    from src.ddsp.oscillator import TraditionalDampedOscillator
    from src.diffelastic.diff_model import Material, build_model

    m = golden("g0_bowl_mesh.npz")
    v = torch.from_numpy(m["verts"]).to(DEV)
    t = torch.from_numpy(m["tets"]).long().to(DEV)
    modes = 16
    gt_mat = (2700.0, 6.0e10, 0.25, 6.0, 1e-7)
    init_mat = (2700.0, 4.0e10, 0.3, 6.0, 1e-7)
    forces = torch.zeros((1, 150), device=DEV)
    forces[0, 0] = 1
    gt = build_model(None, modes, 1, gt_mat, "gt", vertices=v, tets=t)
    gt.eigen_decomposition()
    gt_audio = TraditionalDampedOscillator(forces, 1, modes, 8000, SR, Material(gt_mat)).cuda()(
        gt.get_undamped_freqs().float())
    torch.manual_seed(0)
    model = build_model(None, modes, 1, init_mat, "material", vertices=v, tets=t)
    osc = TraditionalDampedOscillator(forces, len(gt_audio), modes, 8000, SR, Material(init_mat)).cuda()
    loss_fn = MSSLoss([2048, 1024], SR, type="geomloss").cuda()
    opt = Adam(model.parameters(), lr=5e-3)
    E0, nu0 = float(model.material_model.youngs().detach()), float(model.material_model.poisson().detach())
    losses = []
    for epoch in range(3):
        if epoch == 0:
            model.eigen_decomposition()
        pred = osc(model.get_undamped_freqs().float())
        loss = loss_fn(pred, gt_audio, osc.damped_freq, 1)
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss))
    E1, nu1 = float(model.material_model.youngs().detach()), float(model.material_model.poisson().detach())
    print(f"early phase: losses {losses}  E {E0:.4e} -> {E1:.4e}  nu {nu0:.5f} -> {nu1:.5f}")
    assert all(np.isfinite(losses))
    assert E1 != E0 and nu1 != nu0
