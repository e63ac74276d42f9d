"""diffsound_amd.diffelastic.radiation on the device: the fit, ModalRadiator against bem.modal_transfer, the listener's
gradient through the oscillator, a position recovery, refusals and warnings."""
import functools
import math
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _multipole_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

# The 3^3 box (108 boundary faces), order 1, 8 modes, of a soft plastic: with E = 5e8 Pa the eight modes have k a between 2 and
# 3.5 (a = 0.0707 m), so that the order is set by the geometric rate (1 / fit_radius)^(L + 1) and not by k a.
MAT = (2700.0, 5e8, 0.25, 6.0, 1e-7)
BOX_ORDER = 16
F64 = torch.float64


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


@functools.lru_cache(maxsize=None)
def _box():
    """(obj, radiator): built once, never modified."""
    from diffsound_amd import meshgen
    from diffsound_amd.diffelastic.diff_model import DiffSoundObj, FixedLinear
    from diffsound_amd.diffelastic.radiation import ModalRadiator

    v, t = meshgen.kuhn_box(3)
    obj = DiffSoundObj(vertices=torch.from_numpy(v).to(_dev()), tets=torch.from_numpy(t).long().to(_dev()), mode_num=8, mat=MAT,
                       order=1, mat_model=FixedLinear, task="gt")
    obj.eigen_decomposition()
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # neither a GMRES nor a residual warning at this order
        rad = ModalRadiator(obj, order=BOX_ORDER)
    return obj, rad


@pytest.mark.parametrize("L,k", R.MONO_CASES)
def test_fit_and_eval_recover_an_offset_monopole(L, k):
    """(a) the CPU test's monopole case through fit_multipoles and multipole_eval: the same bound."""
    from diffsound_amd.diffelastic.radiation import fit_multipoles, multipole_eval

    N = R.nterms(L)
    ps = R.fibonacci_sphere(4 * N, R.MONO_RS)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(_dev())  # noqa: E731
    kk, center = up(np.array([k])), torch.zeros(3, dtype=F64, device=_dev())
    coef, res = fit_multipoles(up(ps), up(R.monopole(ps, k)[:, None]), kk, center, L)
    assert coef.shape == (1, N) and coef.dtype == torch.complex128 and res.shape == (1,)
    pt = R.fibonacci_sphere(200, R.MONO_RTEST)
    want = R.monopole(pt, k)
    got = multipole_eval(up(pt), center, kk, coef, L).cpu().numpy()[:, 0]
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"RATIO fit-gpu L={L} k={k} err/(b/Rs)^(L+1) = {err / (R.mono_bound(L) / 4):.3g} residual {float(res[0]):.2e}")
    assert err <= R.mono_bound(L)


def test_radiator_agrees_with_modal_transfer():
    """(b) held-out points at 2 a and 4 a against bem.modal_transfer, the yardstick, which is also evaluated on the sample
    sphere: the held-out error over the sample-sphere peak is at most 10 times the sample-sphere residual, itself <= 1e-3."""
    from diffsound_amd.diffelastic import bem

    obj, rad = _box()
    assert rad.order == BOX_ORDER and rad.coef.shape == (8, (BOX_ORDER + 1) ** 2) and len(rad.gmres_info) == 8
    assert all(i["converged"] for i in rad.gmres_info)
    sample = torch.from_numpy(bem.modal_transfer(obj, rad.sample_points.cpu().numpy())).to(_dev())
    fitted = rad.transfer(rad.sample_points)
    peak = sample.abs().max(0).values
    resid = torch.linalg.vector_norm(fitted - sample, dim=0) / torch.linalg.vector_norm(sample, dim=0)
    print("RATIO radiator residual", [f"{v:.3g}" for v in resid.tolist()], "k a", [f"{v:.3g}" for v in (rad.k * rad.radius).tolist()])
    assert float(resid.max()) <= 1e-3
    assert torch.allclose(resid, rad.fit_residual, rtol=1e-3, atol=1e-9)  # the radiator's own samples are modal_transfer's
    g = torch.Generator().manual_seed(1)
    dirs = torch.randn(40, 3, dtype=F64, generator=g)
    dirs = (dirs / dirs.norm(dim=1, keepdim=True)).to(_dev())
    for f in (2.0, 4.0):
        pts = rad.center + f * rad.radius * dirs
        ref = torch.from_numpy(bem.modal_transfer(obj, pts.cpu().numpy())).to(_dev())
        err = (rad.transfer(pts) - ref).abs().max(0).values / peak
        ratio = err / resid
        print(f"RATIO radiator held-out {f} a: err / peak / residual", [f"{v:.3g}" for v in ratio.tolist()])
        assert float(ratio.max()) <= 10.0
    assert torch.equal(rad.field(pts, chunk=7), rad.transfer(pts).detach())
    assert torch.equal(rad.gains(pts), rad.transfer(pts).abs())


def _phi(rad, G, x):
    """sum_j G_j |out_j(x)| on the CPU restatement fed the device's coefficients; x (P, 3) numpy."""
    out = R.restate(x, rad.center.cpu().numpy(), rad.k.cpu().numpy(), rad.coef.cpu().numpy().T, rad.order)
    return (G * np.abs(out)).sum()


def test_listener_gradient_through_the_oscillator():
    """(c) gains(x) * amplitudes_at(p) -> DampedOscillator -> sum of squares: the gradient reaches x and p, and the one to x is
    the central difference of the CPU restatement (fed the device's coefficients and autograd's gradient to the gains) within
    the truncation error measured from two step sizes plus the restatement's and the kernel's bounds over the step."""
    from diffsound_amd.ddsp.oscillator import DampedOscillator
    from diffsound_amd.diffelastic.material_model import Material
    from diffsound_amd.impact import ContactSurface

    obj, rad = _box()
    surf = ContactSurface(obj)
    A, m, S, sr = 2, 8, 800, 32000
    forces = torch.zeros((A, 16), device=_dev())
    forces[:, 0] = 1
    torch.manual_seed(4)
    osc = DampedOscillator(forces, A, m, S, sr, [20, 16000], Material(MAT)).cuda()
    freq = torch.linspace(400.0, 4000.0, m, device=_dev()).reshape(m, 1)
    a = rad.radius
    x = (rad.center + torch.tensor([[2.5 * a, 0.4 * a, -1.0 * a], [0.0, 0.0, 3.0 * a]], dtype=F64, device=_dev())).requires_grad_(True)
    p = (rad.center + torch.tensor([[0.2 * a, 0.1 * a, 2 * a], [2 * a, -0.3 * a, 0.1 * a]], dtype=F64, device=_dev())).requires_grad_(True)
    gains = rad.gains(x)
    gains.retain_grad()
    sig = osc(freq, mode_gain=gains * surf.amplitudes_at(p))
    (sig.double() ** 2).sum().backward()
    assert x.grad is not None and p.grad is not None
    assert bool(torch.isfinite(x.grad).all()) and bool(torch.isfinite(p.grad).all())
    assert float(x.grad.abs().min()) > 0 and float(p.grad.abs().max()) > 0
    G = gains.grad.cpu().numpy()
    xs, got = x.detach().cpu().numpy(), x.grad.cpu().numpy()
    # the bound of |out| over the step: K 2^-53 sum |c| |h_l| A_l (tests/_multipole_ref.py), on the restatement's own tables
    u, r, inv = R.geometry(xs, rad.center.cpu().numpy())
    hr, hi = R.hankel_restate(rad.k.cpu().numpy(), r, rad.order)
    coef = rad.coef.cpu().numpy().T
    m_out, _, _ = R.magnitudes(rad.order, u, inv, rad.k.cpu().numpy(), np.hypot(hr, hi), coef, np.ones((2, 8), dtype=complex))
    k_out, _, _ = R.K_counts(2, 8, rad.order, rad.k.cpu().numpy()[None, :] * r[:, None])
    b_phi = (np.abs(G) * k_out * R.U64 * m_out).sum()
    h = 1e-4 * a
    worst = 0.0
    for i in range(2):
        for c in range(3):
            e = np.zeros_like(xs)
            e[i, c] = h
            d1 = (_phi(rad, G, xs + e) - _phi(rad, G, xs - e)) / (2 * h)
            d2 = (_phi(rad, G, xs + 2 * e) - _phi(rad, G, xs - 2 * e)) / (4 * h)
            tol = 1.5 * abs(d1 - d2) / 3 + 2 * b_phi / h
            worst = max(worst, abs(got[i, c] - d1) / tol)
    print(f"RATIO listener-gradient {worst:.3g}")
    assert worst < 1


RECOVER_STEPS, RECOVER_LR = 300, 0.03


def _recover(gains, start, target, scale):
    """Adam on the listener position (in units of ``scale``) towards the gains at ``target``: (first loss, last loss)."""
    q = torch.tensor(start, dtype=F64, requires_grad=True)
    probe = gains(torch.tensor(target, dtype=F64) * scale)
    goal = probe.detach()
    opt = torch.optim.Adam([q], lr=RECOVER_LR)
    loss_of = lambda: ((gains(q * scale) - goal) ** 2).sum() / (goal ** 2).sum()  # noqa: E731
    first = None
    for _ in range(RECOVER_STEPS):
        opt.zero_grad()
        loss = loss_of()
        first = float(loss.detach()) if first is None else first
        loss.backward()
        opt.step()
    with torch.no_grad():
        return first, float(loss_of())


def test_listener_position_recovery():
    """(d) a listener position from the gains at a target position, Adam, the loop run on the CPU restatement (with its own
    adjoint, fed the device's coefficients) and on the device: the loss has to fall as far on the device as the restatement
    says it does - the required ratio end / start comes from the restatement, with a factor 2 for the two rounding histories."""
    _, rad = _box()
    center, kk, coef, L = rad.center.cpu().numpy(), rad.k.cpu().numpy(), rad.coef.cpu().numpy().T, rad.order
    a = rad.radius
    start, target = [[2.6, 0.9, -0.4]], [[2.0, 0.3, 0.5]]  # offsets from the centre in units of a

    class Host(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            out = R.restate(x.detach().numpy(), center, kk, coef, L)
            ctx.x, ctx.out = x.detach().numpy(), out
            return torch.from_numpy(np.abs(out))

        @staticmethod
        def backward(ctx, g):
            gout = g.numpy() * ctx.out / np.abs(ctx.out)  # d |z| = Re(conj(z / |z|) dz)
            return torch.from_numpy(R.restate(ctx.x, center, kk, coef, L, gout)[1])

    c_host = torch.from_numpy(center)
    f0, f1 = _recover(lambda x: Host.apply(c_host + x), start, target, a)
    dev_gains = lambda x: rad.gains(rad.center + x.to(_dev())).cpu()  # noqa: E731
    d0, d1 = _recover(dev_gains, start, target, a)
    print(f"RATIO recovery restatement {f1 / f0:.4g} device {d1 / d0:.4g} (start {f0:.4g})")
    assert f1 / f0 < 0.5  # the restatement itself descends; how far is what the device is held to
    assert abs(d0 - f0) <= 1e-9 * f0
    assert d1 / d0 <= 2 * f1 / f0 and d1 / d0 >= 0.5 * f1 / f0


def test_refusals_and_warnings(monkeypatch):
    """(e) what ModalRadiator and its methods refuse, and both warnings with the mode's index."""
    from diffsound_amd.diffelastic import bem
    from diffsound_amd.diffelastic.radiation import ModalRadiator, fit_multipoles, multipole_eval

    obj, rad = _box()
    inside = rad.center + torch.tensor([[0.5 * rad.radius, 0.0, 0.0]], dtype=F64, device=_dev())
    outside = rad.center + torch.tensor([[2.0 * rad.radius, 0.0, 0.0]], dtype=F64, device=_dev())
    for call in (rad.transfer, rad.gains, rad.field):
        with pytest.raises(ValueError, match="inside the bounding sphere"):
            call(torch.cat([outside, inside]))
        with pytest.raises(ValueError, match="inside the bounding sphere"):
            call(outside * float("nan"))
        with pytest.raises(ValueError, match=r"\(P, 3\)"):
            call(outside[0])
        with pytest.raises(RuntimeError, match="HIP device"):
            call(outside.cpu())
    with pytest.raises(ValueError, match="lies at the center"):
        multipole_eval(torch.cat([outside, rad.center[None]]), rad.center, rad.k, rad.coef, rad.order)
    with pytest.raises(ValueError, match="k must be positive"):
        multipole_eval(outside, rad.center, -rad.k, rad.coef, rad.order)
    with pytest.raises(ValueError, match="coef is not finite"):
        multipole_eval(outside, rad.center, rad.k, rad.coef * float("inf"), rad.order)
    with pytest.raises(ValueError, match="samples, at least"):
        fit_multipoles(rad.sample_points[:10], rad.sample_values[:10], rad.k, rad.center, 4)
    for kw, text in ((dict(order=33), "order = 33"), (dict(order=2, samples=17), "samples = 17"), (dict(fit_radius=1.0), "fit_radius")):
        with pytest.raises(ValueError, match=text):
            ModalRadiator(obj, **kw)
    with pytest.warns(RuntimeWarning, match=r"the fit of mode \d at order 0 leaves a relative residual") as rec:
        low = ModalRadiator(obj, order=0)
    assert float(low.fit_residual.max()) > 1e-2 and low.coef.shape == (8, 1)
    assert {int(str(w.message).split("mode ")[1][0]) for w in rec} == {j for j, r in enumerate(low.fit_residual.tolist()) if r > 1e-2}
    short = bem.BEMModel._gmres
    monkeypatch.setattr(bem.BEMModel, "_gmres", lambda self, A, b: short(self, A, b, maxiter=2))
    with pytest.warns(RuntimeWarning, match=r"GMRES did not converge for mode 0 \(k = "):
        bad = ModalRadiator(obj, order=2)
    assert not any(i["converged"] for i in bad.gmres_info)
