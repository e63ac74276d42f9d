"""The Python layer over the listener bank: ``oscillator_bank_listener`` through autograd against the references of
tests/_osc_listen_ref.py, the ``listener_gain`` keyword of the oscillator modules, and the chain
ModalRadiator.listener_path_gains -> bank -> loss end to end on the small box of tests/test_radiation_api_gpu.py."""
import functools
import math
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _multipole_ref as MR  # noqa: E402
import _osc_driven_ref as D  # noqa: E402
import _osc_listen_ref as LS  # noqa: E402
from _guarded import _ratio  # noqa: E402

pytestmark = pytest.mark.gpu

MAT = (2700.0, 5e8, 0.25, 6.0, 1e-7)  # the box of tests/test_radiation_api_gpu.py
BOX_ORDER = 16
F64 = torch.float64
SR = LS.SR


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _t(x, **kw):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(_dev(), **kw)


def _hc(h):
    """(A, C, m, K, 2) fp32 -> complex64 (A, C, m, K) on the device."""
    return torch.view_as_complex(_t(h))


@pytest.mark.parametrize("case", [(2, 3, 5, 70, 65, 3, 16, "material", True), (1, 2, 5, 513, LS.TILE + 1, 22, 48, "d0", False),
                                  (3, 1, 4, 40, 50, 1, 16, "nyquist", True)], ids=LS.case_id)
def test_bank_function_and_all_five_gradients(case):
    from diffsound_amd.ddsp.bank import oscillator_bank_listener

    A, C, m, F, S, K, hop = case[:7]
    d, w, amp, force, h, gy = LS.inputs(case)
    td, tw = _t(d).requires_grad_(True), _t(w).requires_grad_(True)
    tamp = None if amp is None else _t(amp).requires_grad_(True)
    tf, th = _t(force).requires_grad_(True), _hc(h).requires_grad_(True)
    static = K == 1
    y = oscillator_bank_listener(td, tw, tamp, tf, th[..., 0] if static else th, None if static else hop, S, SR)
    assert y.shape == (A, C, S) and y.dtype == torch.float32
    y.backward(_t(gy))
    y_ref, Y = LS.forward(d, w, amp, force, h, hop, S)
    b = LS.backward(gy, d, w, amp, force, h, hop)
    assert _ratio("lis.api.y", case, y.detach().cpu().numpy(), y_ref, LS.bound32(y_ref, Y, A, C, m, S)) <= 1.0
    gh = torch.view_as_real(th.grad).cpu().numpy()
    assert th.grad.dtype == torch.complex64
    assert _ratio("lis.api.gh", case, gh, b["gh"], LS.bound32(b["gh"], b["Vh"], A, C, m, S)) <= 1.0
    assert _ratio("lis.api.gforce", case, tf.grad.cpu().numpy(), b["gforce"], LS.bound32(b["gforce"], b["Eg"], A, C, m, S)) <= 1.0
    assert _ratio("lis.api.gd", case, td.grad.cpu().numpy(), b["gd"], LS.bound_gd_gw(b["W"], A, C, m, S)) <= 1.0
    assert _ratio("lis.api.gw", case, tw.grad.cpu().numpy(), b["gw"], LS.bound_gd_gw(b["W"], A, C, m, S)) <= 1.0
    if amp is not None:
        assert _ratio("lis.api.gamp", case, tamp.grad.cpu().numpy(), b["gamp"], LS.bound32(b["gamp"], b["V"], A, C, m, S)) <= 1.0


def test_gradients_are_computed_only_where_needed():
    from diffsound_amd.ddsp.bank import oscillator_bank_listener

    case = (2, 2, 3, 20, 40, 2, 16, "material", True)
    d, w, amp, force, h, gy = LS.inputs(case)
    td, th = _t(d).requires_grad_(True), _hc(h)
    y = oscillator_bank_listener(td, _t(w), _t(amp), _t(force), th, 16, 40, SR)
    y.backward(_t(gy))
    assert td.grad is not None and th.grad is None


def test_a_lazily_conjugated_gain_is_taken():
    """gain = transfer.conj() in complex64 carries torch's conjugate bit; the bank resolves it: the bits of the materialised
    gain, through the function and through the module keyword, with a gradient to the unconjugated leaf."""
    from diffsound_amd.ddsp.bank import oscillator_bank_listener
    from diffsound_amd.ddsp.oscillator import TraditionalDampedOscillator
    from diffsound_amd.diffelastic.material_model import Material, MatSet

    case = (2, 2, 3, 20, 40, 2, 16, "material", True)
    d, w, amp, force, h, gy = LS.inputs(case)
    t = _hc(h).requires_grad_(True)
    lazy = t.conj()
    assert lazy.is_conj()
    args = (_t(d), _t(w), _t(amp), _t(force))
    y = oscillator_bank_listener(*args, lazy, 16, 40, SR)
    assert torch.equal(y, oscillator_bank_listener(*args, t.detach().conj().resolve_conj(), 16, 40, SR))
    y.backward(_t(gy))
    b = LS.backward(gy, d, w, amp, force, np.stack([h[..., 0], -h[..., 1]], -1), 16)
    want = np.stack([b["gh"][..., 0], -b["gh"][..., 1]], -1)       # d / d Im t = -d / d Im conj(t)
    assert _ratio("lis.api.conj.gh", case, torch.view_as_real(t.grad.resolve_conj()).cpu().numpy(), want, LS.bound32(want, b["Vh"], 2, 2, 3, 40)) <= 1.0
    osc = TraditionalDampedOscillator(_t(force), 2, 3, 40, 32000, Material(MatSet.Ceramic))
    freq = torch.linspace(300.0, 900.0, 3, device=_dev()).reshape(3, 1)
    lg = torch.randn(2, 3, dtype=torch.complex64, device=_dev())
    assert lg.conj().is_conj() and torch.equal(osc(freq, listener_gain=lg.conj()), osc(freq, listener_gain=lg.conj().resolve_conj()))


def test_bank_function_refusals():
    from diffsound_amd.ddsp.bank import oscillator_bank_listener

    d, w, amp, force, h, _ = LS.inputs((2, 2, 3, 20, 40, 2, 16, "material", True))
    td, tw, tamp, tf, th = _t(d), _t(w), _t(amp), _t(force), _hc(h)
    for bad, hop, text in ((th.real, 16, "must be complex"), (th[:1], 16, r"must be \(2, C, 3\)"), (th[:, :, :2], 16, r"must be \(2, C, 3\)"),
                           (th, None, "multiple of 16"), (th, 24, "multiple of 16"), (th, 0, "multiple of 16"),
                           (th[..., 0], 16, "hop goes with a 4-D"), (th[:, :1].expand(2, 17, 3, 2), 16, "at most 16 channels")):
        with pytest.raises(ValueError, match=text):
            oscillator_bank_listener(td, tw, tamp, tf, bad, hop, 40, SR)


def test_a_real_gain_is_the_existing_bank_with_amp_times_gain():
    """hgain = g + 0i against oscillator_bank_driven with amp g, per channel: amp in {0.5, 1, 1.5} and g in {-2, -1, 0.5, 1}
    make amp g exact in fp32, so the two differ by their own kernels' bounds alone (both sums of magnitudes are E |g|)."""
    from diffsound_amd.ddsp.bank import oscillator_bank_driven, oscillator_bank_listener

    A, C, m, F, S = 2, 3, 5, 513, LS.TILE + 1
    d, w, _, force, _, _ = LS.inputs((A, C, m, F, S, 1, 16, "material", True))
    rng = np.random.default_rng(9)
    amp = rng.choice([0.5, 1.0, 1.5], (A, m)).astype(np.float32)
    g = rng.choice([-2.0, -1.0, 0.5, 1.0], (A, C, m)).astype(np.float32)
    y = oscillator_bank_listener(_t(d), _t(w), _t(amp), _t(force), torch.complex(_t(g), torch.zeros_like(_t(g))), None, S, SR)
    for c in range(C):
        ag = amp * g[:, c]
        yd = oscillator_bank_driven(_t(d), _t(w), _t(ag), _t(force), S, SR).cpu().numpy()
        ref, E = D.forward(d, w, ag, force, S)
        bound = LS.bound32(ref, E, A, C, m, S) + D.bound_y(ref, E, A, m, S)
        assert _ratio("lis.api.real-gain", (c,), y[:, c].cpu().numpy(), yd, bound) <= 1.0


def test_module_keyword():
    from diffsound_amd.ddsp.oscillator import DampedOscillator, TraditionalDampedOscillator
    from diffsound_amd.diffelastic.material_model import Material, MatSet

    A, m, S, C = 2, 3, 200, 2
    mat = Material(MatSet.Ceramic)
    force = torch.zeros(A, 8, device=_dev())
    force[:, 0] = 1
    freq = torch.linspace(300.0, 900.0, m, device=_dev()).reshape(m, 1)
    osc = TraditionalDampedOscillator(force, A, m, S, 32000, mat)
    plain = osc(freq)
    assert torch.equal(plain, osc(freq, listener_gain=None, listener_hop=None)) and plain.shape == (A, S)
    torch.manual_seed(2)
    lg = torch.randn(C, m, dtype=torch.complex64, device=_dev())
    y = osc(freq, listener_gain=lg)
    assert y.shape == (A, C, S) and bool(torch.isfinite(y).all())
    assert torch.equal(y, osc(freq, listener_gain=lg.unsqueeze(0).expand(A, C, m)))
    # the next two comparisons are smoke checks of the wiring only - the plain render is the fp32 FIR bank, another kernel
    # family, so 1e-5 of the peak is a loose, picked margin; the derived-bound forms of the same statements are
    # test_a_real_gain_is_the_existing_bank_with_amp_times_gain here and the unit-gain test of test_osc_listen_kernels_gpu.py
    one = torch.ones(1, m, dtype=torch.complex64, device=_dev())
    assert torch.allclose(osc(freq, listener_gain=one)[:, 0], plain, rtol=0, atol=1e-5 * float(plain.abs().max()))
    strike = torch.rand(A, m, device=_dev()) + 0.5
    ys = osc(freq, mode_gain=strike, listener_gain=one)   # a strike still folds into amp
    assert torch.allclose(ys[:, 0], osc(freq, mode_gain=strike), rtol=0, atol=1e-5 * float(plain.abs().max()))
    moving = torch.randn(C, m, 4, dtype=torch.complex64, device=_dev())
    assert osc(freq, listener_gain=moving, listener_hop=64).shape == (A, C, S)
    assert osc(freq, listener_gain=moving.unsqueeze(0).expand(A, C, m, 4), listener_hop=64).shape == (A, C, S)
    dosc = DampedOscillator(force, A, m, S, 32000, [100.0, 200.0, 400.0], mat).to(_dev())
    assert dosc(freq, listener_gain=lg).shape == (A, C, S)
    for kw, text in ((dict(listener_gain=lg.real), "must be complex"), (dict(listener_gain=lg[:, :2]), r"\(C, 3\) or \(2, C, 3\)"),
                     (dict(listener_gain=moving), r"\(C, 3\) or \(2, C, 3\)"), (dict(listener_gain=moving, listener_hop=24), "multiple of 16"),
                     (dict(listener_gain=moving.unsqueeze(0).expand(A, C, m, 4)), "needs listener_hop"),
                     (dict(listener_hop=16), "listener_hop goes with"),
                     (dict(listener_gain=torch.ones(17, m, dtype=torch.complex64, device=_dev())), "at most 16 channels"),
                     (dict(listener_gain=lg, mode_gain=torch.ones(A, 4, m, device=_dev()), gain_hop=16), "sliding contact heard")):
        with pytest.raises(ValueError, match=text):
            osc(freq, **kw)
    with pytest.raises(ValueError, match="non_linear_rate must be 0"):
        dosc(freq, non_linear_rate=0.5, listener_gain=lg)
    with pytest.raises(ValueError, match="forward_curve"):
        dosc.forward_curve(freq, lambda f: 0 * f + 5.0, listener_gain=lg)


# ------------------------------------------------------------------------------------------------- end to end
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
        warnings.simplefilter("error")
        rad = ModalRadiator(obj, order=BOX_ORDER)
    return obj, rad


def _radial_path(rad, step, K, r0=3.0):
    """K points going out along a fixed direction from r0 radii, ``step`` metres apart."""
    u = torch.tensor([0.6, -0.48, 0.64], dtype=F64, device=_dev())
    r = r0 * rad.radius + step * torch.arange(K, dtype=F64, device=_dev())
    return rad.center + r[:, None] * u[None, :]


def test_listener_gains_are_the_conjugate_transfer():
    _, rad = _box()
    pts = _radial_path(rad, 0.01, 3)
    T = rad.transfer(pts)
    assert torch.equal(rad.listener_gains(pts), T.conj()) and T.shape == (3, 8)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        hp = rad.listener_path_gains(torch.stack([pts, pts.flip(0)]))
    assert hp.shape == (2, 8, 3) and hp.dtype == torch.complex128
    assert torch.equal(hp[0], T.conj().T) and torch.equal(hp[1], T.conj().T.flip(1))
    assert rad.listener_path_gains(pts).shape == (1, 8, 3)
    with pytest.raises(ValueError, match=r"\(K, 3\) or \(C, K, 3\)"):
        rad.listener_path_gains(pts[:, :2])


def test_the_phase_step_warning():
    """Along a radius a mode's transfer turns by about k dr per frame (the e^{ikr} of the far field; the near-field terms of
    the series turn more slowly).  With the largest k of the box: k dr = 2 rad, well above pi / 4, must warn; k dr = 0.1 rad
    must not."""
    _, rad = _box()
    kmax = float(rad.k.max().cpu())
    loud, quiet = 2.0 / kmax, 0.1 / kmax
    assert kmax * loud > 2 * (math.pi / 4) and kmax * quiet < 0.25 * (math.pi / 4)
    with pytest.warns(RuntimeWarning, match=r"lower hop") as rec:
        rad.listener_path_gains(_radial_path(rad, loud, 4))
    assert "rad between two consecutive frames" in str(rec[0].message)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        rad.listener_path_gains(_radial_path(rad, quiet, 4))


def test_path_gradient_through_the_whole_chain():
    """listener_path_gains -> oscillator_bank_listener -> mean((y - target)^2): the gradient to one coordinate of one path
    point against the central difference of the fp64 restatement of the whole chain (the multipole restatement of
    tests/_multipole_ref.py fed the device's coefficients, then tests/_osc_listen_ref.forward), within
    ``_osc_listen_ref.grad_tolerance``."""
    from diffsound_amd.ddsp.bank import oscillator_bank_listener

    _, rad = _box()
    A, C, m, S, hop, K = 1, 2, 8, 400, 64, 8
    rng = np.random.default_rng(21)
    w = LS.R.TWO_PI * np.sort(rng.uniform(400.0, 4000.0, m))
    d = rng.uniform(5.0, 60.0, m)
    force = np.zeros((A, 24), dtype=np.float32)
    force[0, :24] = np.hanning(24).astype(np.float32)
    kmax = float(rad.k.max().cpu())
    p0 = _radial_path(rad, 0.2 / kmax, K)
    ear = torch.tensor([0.0, 0.15 * rad.radius, 0.0], dtype=F64, device=_dev())
    path = torch.stack([p0 + ear, p0 - ear]).requires_grad_(True)                 # (C, K, 3)
    center, kk, coef = rad.center.cpu().numpy(), rad.k.cpu().numpy(), rad.coef.cpu().numpy().T

    def restated(pnp):
        """(y, Ymag, h (1, C, m, K, 2) fp64) of the chain on the CPU."""
        T = MR.restate(pnp.reshape(C * K, 3), center, kk, coef, rad.order).reshape(C, K, m).transpose(0, 2, 1)
        h = np.stack([T.real, -T.imag], -1)[None]
        y, Y = LS.forward(d, w, None, force, h, hop, S)
        return y, Y, h

    pn = path.detach().cpu().numpy()
    y0, Y0, h0 = restated(pn)
    target = (0.5 * y0[:, ::-1] + 0.1 * np.abs(y0).max()).astype(np.float32)       # any fixed fp32 signal: it enters exactly
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        hg = rad.listener_path_gains(path)
    y = oscillator_bank_listener(_t(d), _t(w), None, _t(force), hg.unsqueeze(0), hop, S, SR)
    ((y.double() - _t(target).double()) ** 2).mean().backward()
    got = path.grad.cpu().numpy()
    assert np.isfinite(got).all() and np.abs(got).min() > 0

    def loss(pnp):
        return ((restated(pnp)[0] - target.astype(np.float64)) ** 2).mean()

    e = 1e-4 * rad.radius
    worst = 0.0
    for c, k, ax in ((0, 3, 0), (1, 5, 2), (0, K - 1, 1)):
        dp = np.zeros_like(pn)
        dp[c, k, ax] = e
        d1 = (loss(pn + dp) - loss(pn - dp)) / (2 * e)
        d2 = (loss(pn + 2 * dp) - loss(pn - 2 * dp)) / (4 * e)
        dh = (restated(pn + dp)[2] - restated(pn - dp)[2]) / (2 * e)
        dY = LS.forward(d, w, None, force, np.abs(dh), hop, S)[1]
        curvature = abs(d1 - d2) / 3 + 4 * LS.U64 * loss(pn) / e                  # truncation, and the difference's own rounding
        tol = LS.grad_tolerance(y0, Y0, target, np.zeros_like(Y0), dY, curvature)
        print(f"GRAD path[{c},{k},{ax}] device {got[c, k, ax]:.9e} central {d1:.9e} tol {tol:.3e}")
        worst = max(worst, abs(got[c, k, ax] - d1) / tol)
    print(f"RATIO lis.api.path-gradient {worst:.3g}")
    assert worst <= 1.0
