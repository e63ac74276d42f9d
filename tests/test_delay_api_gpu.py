"""``ddsp.delay.propagate``, the ``listener_delay`` keyword of the oscillator modules and ``ModalRadiator.listener_path`` on the
device: gradients through autograd against tests/_delay_ref.py, every ValueError, the Doppler shift of a tone against the
analytic signal, a listener at rest as an exact shift, and the path gradient through the whole chain."""
import math
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _delay_ref as DL  # noqa: E402
import _multipole_ref as MR  # noqa: E402
import _osc_listen_ref as LS  # noqa: E402
from _guarded import _ratio  # noqa: E402

pytestmark = pytest.mark.gpu

F64 = torch.float64
SR = LS.SR
R = DL.R


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _t(x, **kw):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(_dev(), **kw)


@pytest.mark.parametrize("case", [DL.CASES[3], DL.CASES[13], DL.CASES[17]], ids=DL.case_id)
def test_propagate_and_both_gradients(case):
    from diffsound_amd.ddsp.delay import propagate

    B, S, K, hop, _ = case
    s, tau, gy = DL.inputs(case)
    ts, tt = _t(s).requires_grad_(True), _t(tau).requires_grad_(True)
    y = propagate(ts, tt, hop)
    assert y.shape == (B, S) and y.dtype == torch.float32
    y.backward(_t(gy))
    f, b = DL.forward(s, tau, hop), DL.backward(gy, s, tau, hop)
    assert _ratio("delay.api.y", case, y.detach().cpu().numpy(), f["y"], DL.bound_y(f)) <= 1.0
    assert _ratio("delay.api.gs", case, ts.grad.cpu().numpy(), b["gs"], DL.bound_gs(b)) <= 1.0
    assert _ratio("delay.api.gtau", case, tt.grad.cpu().numpy(), b["gtau"], b["gtau_bound"]) <= 1.0
    assert tt.grad.dtype == F64 and ts.grad.dtype == torch.float32


def test_broadcast_dtypes_and_gradients_only_where_needed(monkeypatch):
    """A delay (C, K) shared by every clip of a signal (A, C, S): its gradient is the sum over the clips (autograd's, of the
    expanded rows); an fp64 signal comes back as fp64; a gradient that is not needed is not computed."""
    from diffsound_amd.ddsp import delay as dmod

    A, C, S, K, hop = 2, 3, 100, 4, 32
    rng = np.random.default_rng(8)
    s = rng.standard_normal((A, C, S)).astype(np.float32)
    tau = np.abs(np.cumsum(rng.uniform(-10, 10, (C, K)), 1))
    gy = rng.standard_normal((A, C, S)).astype(np.float32)
    ts, tt = _t(s).requires_grad_(True), _t(tau).requires_grad_(True)
    y = dmod.propagate(ts, tt, hop)
    y.backward(_t(gy))
    rows = np.tile(tau[None], (A, 1, 1)).reshape(A * C, K)
    f = DL.forward(s.reshape(A * C, S), rows, hop)
    b = DL.backward(gy.reshape(A * C, S), s.reshape(A * C, S), rows, hop)
    assert _ratio("delay.api.bcast.y", None, y.detach().cpu().numpy().reshape(A * C, S), f["y"], DL.bound_y(f)) <= 1.0
    want, bound = b["gtau"].reshape(A, C, K).sum(0), b["gtau_bound"].reshape(A, C, K).sum(0) + 4 * DL.U64 * np.abs(b["gtau"]).reshape(A, C, K).sum(0)
    assert _ratio("delay.api.bcast.gtau", None, tt.grad.cpu().numpy(), want, bound) <= 1.0
    y64 = dmod.propagate(_t(s).double(), _t(tau).float(), hop)
    assert y64.dtype == F64 and y64.shape == (A, C, S)
    calls, real = [], dmod._hip.lib()

    class Proxy:
        def __getattr__(self, name):
            return getattr(real, name)

        def ds_delay_bwd(self, *a):
            calls.append((a[9], a[10]))                                                  # the gs and gtau pointers
            return real.ds_delay_bwd(*a)

    monkeypatch.setattr(dmod._hip, "lib", lambda: Proxy())
    for need_s, need_t in ((True, False), (False, True)):
        a, d = _t(s).requires_grad_(need_s), _t(tau).requires_grad_(need_t)
        dmod.propagate(a, d, hop).backward(_t(gy))
        assert (a.grad is not None) == need_s and (d.grad is not None) == need_t
    assert [(gs is not None, gt is not None) for gs, gt in calls] == [(True, False), (False, True)]


def test_every_refusal():
    from diffsound_amd.ddsp.delay import propagate

    s, tau = torch.zeros(2, 3, 64, device=_dev()), torch.zeros(3, 4, device=_dev(), dtype=F64)
    for hop in (0, -16, 16.0, None):
        with pytest.raises(ValueError, match="not a positive int"):
            propagate(s, tau, hop)
    with pytest.raises(ValueError, match="does not broadcast"):
        propagate(s, tau[:2], 16)
    with pytest.raises(ValueError, match="floating-point tensor"):
        propagate(s.long(), tau, 16)
    with pytest.raises(ValueError, match=r"delay must be \(\.\.\., K\)"):
        propagate(s, tau[:, :0], 16)
    bad = s.clone()
    bad[1, 2, 5] = float("nan")
    with pytest.raises(ValueError, match="signal is not finite"):
        propagate(bad, tau, 16)
    for v in (float("nan"), float("inf")):
        d = tau.clone()
        d[1, 2] = v
        with pytest.raises(ValueError, match="delay is not finite"):
            propagate(s, d, 16)
    d = tau.clone()
    d[2, 0] = -0.25
    with pytest.raises(ValueError, match="a delay is negative"):
        propagate(s, d, 16)
    d = torch.tensor([[0.0, 8.0, 16.0, 24.0], [0.0, 8.0, 20.0, 28.0], [1.0, 2.0, 3.0, 4.0]], device=_dev(), dtype=F64)
    with pytest.raises(ValueError, match=r"row 1 changes by 12 samples between frames 1 and 2, 0\.75 of the speed of sound"):
        propagate(s, d, 16)
    d[1, 2:] = torch.tensor([16.0, 24.0], dtype=F64)                                      # every step exactly hop / 2: the limit
    assert propagate(s, d, 16).shape == s.shape
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        propagate(s.cpu(), tau.cpu(), 16)


@pytest.mark.parametrize("nu", [0.05, 0.3])
def test_doppler(nu):
    """A tone at nu cycles per sample heard by a listener that recedes at 0.3 of the speed of sound: the output against the
    analytic sin(2 pi nu (t - tau(t))).  Bound: the interpolator's passband error E(nu) of tests/_delay_ref.py (the 16 taps
    against an ideal delay, for any fractional part), the fp32 rounding of the input tone (U32 |s| <= U32 per tap, times the
    sum of |h|), the kernel's counted rounding against the dense reference, and the analytic value's own (its argument
    2 pi nu p carries 4 U64 of itself).  Samples whose 16 taps reach outside [0, S) are left out: p < R at the start (p stays
    below S - R here), 13 of 2048 = 0.63 %, below 2 R / S = 0.78 %."""
    from diffsound_amd.ddsp.delay import propagate

    S, hop, v = 2048, 64, 0.3
    K = DL.frames_needed(S, hop)
    tau = (0.5 + v * hop * np.arange(K))[None, :]
    s = np.sin(2 * np.pi * nu * np.arange(S))[None, :].astype(np.float32)
    y = propagate(_t(s), _t(tau), hop).cpu().numpy()
    p, _ = DL.positions(tau, hop, S)
    keep = (p >= R) & (p <= S - 1 - R)
    share = 1.0 - keep.mean()
    print(f"doppler nu {nu}: {int((~keep).sum())} of {S} samples left out ({100 * share:.2f} %)")
    assert 0 < share <= 2.0 * R / S
    f = DL.forward(s, tau, hop)
    wsum = DL.forward(np.ones_like(s), tau, hop)["mag"]
    E = DL.passband_error(nu)
    bound = E + DL.U32 * wsum + DL.bound_y(f) + 4 * DL.U64 * 2 * np.pi * nu * np.abs(p)
    want = np.sin(2 * np.pi * nu * p)
    assert _ratio(f"delay.doppler.E={E:.3g}", (nu,), y[keep], want[keep], bound[keep]) <= 1.0
    # the shift itself: the output's frequency is nu (1 - v), not nu - the undelayed tone is far outside the bound
    assert np.abs(s[keep].astype(np.float64) - want[keep]).max() > 100 * bound[keep].max()


def _modules():
    from diffsound_amd.ddsp.oscillator import DampedOscillator, GTDampedOscillator, TraditionalDampedOscillator
    from diffsound_amd.diffelastic.material_model import Material, MatSet

    A, m, S = 2, 3, 300
    mat = Material(MatSet.Ceramic)
    force = torch.zeros(A, 8, device=_dev())
    force[:, 0] = 1
    f_range = [100.0 * (i + 1) for i in range(8)]
    freq = torch.linspace(300.0, 900.0, m, device=_dev()).reshape(m, 1)
    torch.manual_seed(4)
    return [(TraditionalDampedOscillator(force, A, m, S, 32000, mat), (freq,)),
            (DampedOscillator(force, A, m, S, 32000, f_range, mat).to(_dev()), (freq,)),
            (GTDampedOscillator(force, A, m, S, 32000, f_range, mat).to(_dev()), ())], A, m, S


def test_a_listener_at_rest_is_an_exact_shift():
    """sr r / c = N, an integer: forward(listener_gain, listener_hop, listener_delay) is forward(listener_gain, listener_hop)
    shifted by N, bit for bit, the first N samples exactly 0 - for a gain at rest (K = 1) and for a gain with frames."""
    mods, A, m, S = _modules()
    C, K, hop, N = 2, 4, 64, 37
    torch.manual_seed(6)
    rest = torch.randn(C, m, dtype=torch.complex64, device=_dev())
    moving = torch.randn(C, m, K, dtype=torch.complex64, device=_dev())
    for mod, args in mods:
        for gain, kw, frames in ((rest, {}, 1), (moving, dict(listener_hop=hop), K)):
            dry = mod(*args, listener_gain=gain, **kw)
            tau = torch.tensor([float(N), float(N + 3)], dtype=F64, device=_dev())[:, None].expand(C, frames)
            wet = mod(*args, listener_gain=gain, listener_delay=tau, **kw)
            assert wet.shape == dry.shape == (A, C, S) and wet.dtype == dry.dtype
            for c, n in ((0, N), (1, N + 3)):
                assert torch.equal(wet[:, c, n:], dry[:, c, :S - n]) and not wet[:, c, :n].any()
            per_clip = mod(*args, listener_gain=gain, listener_delay=tau.unsqueeze(0).expand(A, C, frames).float(), **kw)
            assert torch.equal(per_clip, wet)
    gt, _ = mods[2]
    torch.manual_seed(9)
    dry = gt(listener_gain=rest)
    torch.manual_seed(9)
    noisy = gt(noise_rate=0.5, listener_gain=rest, listener_delay=torch.full((C, 1), float(N), dtype=F64, device=_dev()))
    torch.manual_seed(9)
    noise = gt(noise_rate=0.5, listener_gain=rest) - dry
    assert noise[:, :, :N].abs().max() > 0                                              # the noise branch is not delayed:
    shifted = torch.zeros_like(dry)
    shifted[:, :, N:] = dry[:, :, :S - N]
    assert torch.allclose(noisy - shifted, noise, rtol=0, atol=4 * 2.0 ** -24 * float((dry.abs() + noise.abs()).max().detach()))   # (two fp32 additions)


def test_none_is_the_call_without_the_keyword():
    mods, A, m, S = _modules()
    lg = torch.ones(2, m, dtype=torch.complex64, device=_dev())
    for mod, args in mods:
        assert torch.equal(mod(*args), mod(*args, listener_delay=None))
        assert torch.equal(mod(*args, listener_gain=lg), mod(*args, listener_gain=lg, listener_delay=None))
        with pytest.raises(ValueError, match="listener_delay goes with a listener_gain"):
            mod(*args, listener_delay=torch.zeros(2, 1, device=_dev()))
        with pytest.raises(ValueError, match="a delay is negative"):
            mod(*args, listener_gain=lg, listener_delay=torch.full((2, 1), -1.0, device=_dev()))


# --------------------------------------------------------------------------------------- ModalRadiator.listener_path
ORDER, C_SOUND = 2, 343.0


def _radiator(m=4):
    """A ModalRadiator whose series is set by hand - no boundary-element solve: (radiator, k (m,), coef (N, m)) with the numpy
    copies for the restatement."""
    from diffsound_amd.diffelastic.radiation import ModalRadiator

    rng = np.random.default_rng(17)
    k = 2 * np.pi * np.array([400.0, 900.0, 1700.0, 3100.0][:m]) / C_SOUND
    n = (ORDER + 1) ** 2
    coef = (rng.standard_normal((n, m)) + 1j * rng.standard_normal((n, m))) * 0.1
    rad = ModalRadiator.__new__(ModalRadiator)
    rad.center = torch.tensor([0.0, -0.25, 0.125], dtype=F64, device=_dev())     # (x = 0: center + (r, 0, 0) keeps r exactly)
    rad.radius, rad.order, rad.c = 0.1, ORDER, C_SOUND
    rad.k, rad.coef = _t(k), _t(coef.T.copy())
    return rad, k, coef


def _path(rad, K, step=0.1, r0=1.0):
    u = torch.tensor([0.6, -0.48, 0.64], dtype=F64, device=_dev())
    r = r0 + step * torch.arange(K, dtype=F64, device=_dev())
    ear = torch.tensor([0.0, 0.08, 0.0], dtype=F64, device=_dev())
    p0 = rad.center + r[:, None] * u[None, :]
    return torch.stack([p0 + ear, p0 - ear])                                             # (C = 2, K, 3)


def test_listener_path_is_gain_and_delay():
    rad, k, _ = _radiator()
    K, sr = 5, 32000.0
    path = _path(rad, K).requires_grad_(True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                                  # (the full gain turns by k dr >> pi / 4)
        full = rad.listener_path_gains(path.detach())
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                                   # the stripped gain does not
        gain, delay = rad.listener_path(path, sr)
    assert gain.shape == (2, 4, K) and gain.dtype == torch.complex128 and delay.shape == (2, K) and delay.dtype == F64
    r = torch.linalg.vector_norm(path.detach() - rad.center, dim=-1)
    assert torch.equal(delay.detach(), (sr / C_SOUND) * r)
    kr = rad.k[None, :, None] * r[:, None, :]
    restored = gain.detach() * torch.exp(-1j * kr)
    # cos, sin(k r) twice (there and back), each with the rounding of k r itself in its argument: 4 (k r + 2) U64 of |T|
    tol = 4 * (kr + 2) * DL.U64 * full.abs()
    assert bool(((restored - full).abs() <= tol).all()) and float((restored - full).abs().max()) > 0
    (gain.abs().sum() + (gain.real * gain.imag).sum() + 0.01 * (delay ** 2).sum()).backward()
    g_both = path.grad.clone()
    assert bool(torch.isfinite(g_both).all()) and float(g_both.abs().min()) > 0
    path.grad = None
    gain2, delay2 = rad.listener_path(path, sr)
    (0.01 * (delay2 ** 2).sum()).backward()
    g_delay = path.grad.clone()
    assert float(g_delay.abs().min()) > 0 and float((g_both - g_delay).abs().min()) > 0  # both results carry a gradient
    assert rad.listener_path(path[0].detach(), sr)[1].shape == (1, K)
    with pytest.raises(ValueError, match=r"\(K, 3\) or \(C, K, 3\)"):
        rad.listener_path(path[:, :, :2], sr)
    with pytest.raises(ValueError, match="not positive"):
        rad.listener_path(path, 0.0)
    with pytest.warns(RuntimeWarning, match="with the carrier removed"):                 # frames on opposite sides of the object
        far = rad.center + torch.tensor([[0.5, 0.0, 0.0], [-0.5, 0.0, 0.0], [0.0, 0.5, 0.0]], dtype=F64, device=_dev())
        rad.listener_path(far, sr)


def test_a_radius_with_an_integer_delay_is_found_and_shifts_exactly():
    """r chosen so that sr r / c is the integer N in fp64 (a few neighbouring fp64 radii are tried): the delay that
    ``listener_path`` returns for a listener at rest there shifts the module's render by N, bit for bit."""
    rad, _, _ = _radiator(m=3)
    mods, A, m, S = _modules()
    sr, N = 32000.0, 41
    cand = [N * C_SOUND / sr]
    for _ in range(16):                                                                  # 33 neighbouring fp64 radii, one of which hits N
        cand = [float(np.nextafter(cand[0], 0.0))] + cand + [float(np.nextafter(cand[-1], 1.0))]
    pts = torch.zeros(1, len(cand), 3, dtype=F64, device=_dev())
    pts[0, :, 0] = torch.tensor(cand, dtype=F64)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        delays = rad.listener_path(rad.center + pts, sr)[1][0]
    hit = torch.nonzero(delays == N).reshape(-1)
    found = rad.listener_path((rad.center + pts)[:, int(hit[0]):int(hit[0]) + 1], sr) if hit.numel() else None
    assert found is not None
    gain, delay = found
    osc, args = mods[0]
    dry = osc(*args, listener_gain=gain[:, :, 0])
    wet = osc(*args, listener_gain=gain[:, :, 0], listener_delay=delay)
    assert torch.equal(wet[:, :, N:], dry[:, :, :S - N]) and not wet[:, :, :N].any()


def test_path_gradient_through_the_whole_chain():
    """listener_path -> oscillator_bank_listener -> propagate -> mean((z - target)^2): the gradient to one coordinate of one
    path point against the central difference of the fp64 restatement of the chain (tests/_multipole_ref.restate on the
    same coefficients, tests/_osc_listen_ref.forward, tests/_delay_ref.forward).

    Tolerance, built as ``_osc_listen_ref.grad_tolerance`` builds its own, one stage longer.  Zmag[t] = sum_j |h(p - j)| Ymag[j]
    is the magnitude that enters an output of the delay line; dZmag[t] = sum_j |h| dYmag[j] + |d tau / d x| sum_j |h'| Ymag[j]
    bounds |d z[t] / d x| (the gain's share through the bank, dYmag as in the listener test, and the delay's share).
      * each render carries per sample the bank's 4 u Ymag pushed through the line (4 u Zmag) and the line's own store
        (2 u |z| <= 2 u Zmag): 6 u Zmag;  gy = 2 r / N is rounded to fp32 once: u |r|;
      * these reach the gradient through dZmag: (2 / N) sum_t (6 u Zmag + u |r|) dZmag;
      * the adjoint: gs of the line and gh of the bank are stored in fp32 (2 u each), the line's D(t) is formed from the
        fp32-rounded bank output (4 u of its magnitudes): 8 u (2 / N) sum |r| dZmag, with a factor 2 of margin: 16 u;
      * the central difference's truncation, estimated from a second quotient at 2 e, and its own rounding."""
    from diffsound_amd.ddsp.bank import oscillator_bank_listener
    from diffsound_amd.ddsp.delay import propagate

    rad, kk, coef = _radiator()
    A, C, m, S, hop, K = 1, 2, 4, 300, 64, 6
    rng = np.random.default_rng(23)
    w = LS.R.TWO_PI * np.array([400.0, 900.0, 1700.0, 3100.0])
    d = rng.uniform(5.0, 60.0, m)
    force = np.zeros((A, 24), dtype=np.float32)
    force[0] = np.hanning(24).astype(np.float32)
    path = _path(rad, K).requires_grad_(True)
    center = rad.center.cpu().numpy()

    def restated(pnp):
        """(z, y, Ymag, h (1, C, m, K, 2), delay (C, K), line's forward dict) of the chain on the CPU."""
        T = MR.restate(pnp.reshape(C * K, 3), center, kk, coef, ORDER).reshape(C, K, m).transpose(0, 2, 1)
        r = np.sqrt(((pnp - center) ** 2).sum(-1))                                       # (C, K)
        g = np.conj(T * np.exp(-1j * kk[None, :, None] * r[:, None, :]))
        h = np.stack([g.real, g.imag], -1)[None]
        y, Y = LS.forward(d, w, None, force, h, hop, S)
        delay = SR * r / C_SOUND
        f = DL.forward(y[0], delay, hop)
        return f["y"], y[0], Y[0], h, delay, f

    pn = path.detach().cpu().numpy()
    z0, y0, Y0, h0, delay0, f0 = restated(pn)
    assert (np.abs(np.diff(delay0, axis=1)) <= 0.5 * hop).all() and np.abs(np.diff(delay0, axis=1)).min() > 5
    target = (0.5 * z0[:, ::-1] + 0.1 * np.abs(z0).max()).astype(np.float32)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        gain, delay = rad.listener_path(path, SR)
    y = oscillator_bank_listener(_t(d), _t(w), None, _t(force), gain.unsqueeze(0), hop, S, SR)
    z = propagate(y, delay, hop)
    ((z[0].double() - _t(target).double()) ** 2).mean().backward()
    got = path.grad.cpu().numpy()
    assert np.isfinite(got).all() and np.abs(got).min() > 0

    def loss(pnp):
        return ((restated(pnp)[0] - target.astype(np.float64)) ** 2).mean()

    U = DL.positions(delay0, hop, S)[0][:, :, None] - np.arange(S, dtype=np.float64)[None, None, :]
    aH, aD = np.abs(DL.h(U)), np.abs(DL.dh(U))
    Zmag = np.einsum("ctj,cj->ct", aH, Y0)
    Hk = DL.hat(K, hop, S)
    u32, N = LS.U32, z0.size
    res = np.abs(z0 - target)
    e = 1e-4 * rad.radius
    worst = 0.0
    for c, k, ax in ((0, 3, 0), (1, 4, 2), (0, K - 1, 1)):
        dp = np.zeros_like(pn)
        dp[c, k, ax] = e
        rp, rm = restated(pn + dp), restated(pn - dp)
        d1 = (loss(pn + dp) - loss(pn - dp)) / (2 * e)
        d2 = (loss(pn + 2 * dp) - loss(pn - 2 * dp)) / (4 * e)
        dh_ = (rp[3] - rm[3]) / (2 * e)
        dY = LS.forward(d, w, None, force, np.abs(dh_), hop, S)[1][0]
        dtau = np.abs((rp[4] - rm[4]) / (2 * e)) @ Hk                                    # (C, S): |d tau(t) / d x|
        dZ = np.einsum("ctj,cj->ct", aH, dY) + dtau * np.einsum("ctj,cj->ct", aD, Y0)
        curvature = abs(d1 - d2) / 3 + 4 * LS.U64 * loss(pn) / e
        tol = (2.0 / N) * (((6 * u32) * Zmag + u32 * res) * dZ).sum() + 16 * u32 * (2.0 / N) * (res * dZ).sum() + curvature
        print(f"GRAD path[{c},{k},{ax}] device {got[c, k, ax]:.9e} central {d1:.9e} tol {tol:.3e}")
        worst = max(worst, abs(got[c, k, ax] - d1) / tol)
    print(f"RATIO delay.api.path-gradient {worst:.3g}")
    assert worst <= 1.0
