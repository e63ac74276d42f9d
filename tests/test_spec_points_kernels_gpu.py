"""The point-cloud kernels (csrc/specpoints.hip through diffsound_amd/ddsp/spec_points.py) against the sequential fp64
reference of tests/_spec_points_ref.py, and the fused 'geomloss' front end of SSSLoss end to end.

Column 3 and the winners are compared EXACTLY, with the reference's division in its "reciprocal" form - x * (1 / bins),
what torch performs for a device tensor divided by a Python scalar (measured on the MI355X: arange(33) / 33 on the
device equals that product in every row and differs from the correctly rounded quotient, which CPU torch forms, in 4 of
33 rows).  Columns 0..2 are compared with ``_spec_points_ref.bound_features``, which
is derived from the kernel's operation count and the device log2f allowance of tests/_stft_ref.py (2 ulp) - not from
observed errors.  Observed on the MI355X (largest error / bound): 0.45 at T = 1, 0.40 at T = 2
and 3, 0.26 - 0.35 at T = 17; every test prints its own figure.

The end-to-end bound is measured on every run: the torch-cloud path is run as is and with every cloud element moved by
one fp32 ulp (random direction); 4x the change of the loss (of the gradient) is the bound on fused against unfused - the
margin of tests/test_sinkhorn_gpu.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _spec_points_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev(a, grad=False):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t.requires_grad_(True) if grad else t


def _points(P, freq=None, sr=None, scale=1.0):
    from diffsound_amd.ddsp.spec_points import spectral_points

    return spectral_points(_dev(P), freq, sr, scale, ref.EPS)


def _check_clouds(P, fclip, lin, log, freq_np, sr, what):
    """Column 3 exact, features inside the derived bound; returns the largest error / bound."""
    want = ref.clouds(P, ref.EPS, fclip, freq_np, sr, division="reciprocal")
    bounds = dict(zip(("lin", "log"), ref.bound_features(P, ref.EPS, fclip)))
    worst = 0.0
    for name, got in (("lin", lin), ("log", log)):
        got = got.detach().cpu().numpy()
        w = want[name]
        assert got.shape == w.shape and got.dtype == np.float32, (what, name)
        assert np.array_equal(got[..., 3], w[..., 3].astype(np.float32), equal_nan=False), (what, name, "column 3")
        ratio = np.abs(got[..., :3].astype(np.float64) - w[..., :3]) / bounds[name]
        assert (ratio <= 1.0).all(), (what, name, float(ratio.max()))
        worst = max(worst, float(ratio.max()))
    return worst, want


def _torch_path(P, fclip, freq, sr):
    """The device torch path the kernels replace: spec2point on the spectrogram and on the log spectrogram / 40."""
    from diffsound_amd.ddsp.mss_loss import SSSLoss, spec2point

    Pt = _dev(P)
    s = SSSLoss(ref.N_FFT, sr or 32000)
    return spec2point(Pt, freq, sr), spec2point(s.log_func(Pt[:, :fclip]) / 40, freq, sr)


def _check_torch_path(P, fclip, lin, log, freq, sr, what):
    """Features of the kernel against the device torch path, inside the same derived bound.  (Column 3 against that path:
    test_column3_equals_the_device_torch_path.)"""
    bounds = ref.bound_features(P, ref.EPS, fclip)
    for got, tor, b, name in zip((lin, log), _torch_path(P, fclip, freq, sr), bounds, ("lin", "log")):
        got, tor = got.detach().cpu().numpy(), tor.detach().cpu().numpy()
        assert (np.abs(got[..., :3].astype(np.float64) - tor[..., :3]) <= b).all(), (what, name)


@pytest.mark.parametrize("cloud", ["lin", "log"])
@pytest.mark.parametrize("scale", ref.SCALES)
def test_column3_equals_the_device_torch_path(scale, cloud):
    """On the collision-free, finite inputs (and without freq) column 3 of the kernel equals, exactly, column 3 of
    ``spec2point`` run on the device.

    Both perform the same fp32 operations in the same order, the division by the scalar ``bins`` as the product with
    1 / bins; observed: 0 of 660 (33 rows) and 0 of 320 (16 rows) entries differ."""
    fclip = int(ref.F * scale)
    pick = 0 if cloud == "lin" else 1
    differing, rows, worst_ulp = 0, 0, 0.0
    for sr in ref.SAMPLE_RATES:
        cases = {"no_freq": None}
        cases.update({k: v for k, v in ref.freq_cases(sr).items() if k != "nonfinite"
                      and not (ref.has_collisions(ref.F, v, sr) or ref.has_collisions(fclip, v, sr))})
        for name, fnp in cases.items():
            P = ref.spectrogram(3, seed=1)
            f = None if fnp is None else _dev(fnp)
            got = _points(P, f, sr if f is not None else None, scale)[pick][..., 3].cpu().numpy()
            tor = _torch_path(P, fclip, f, sr if f is not None else None)[pick][..., 3].cpu().numpy()
            ne = got != tor
            differing, rows = differing + int(ne.sum()), rows + ne.size
            if ne.any():
                worst_ulp = max(worst_ulp, float((np.abs(got.astype(np.float64) - tor)[ne] / np.spacing(np.abs(tor[ne]))).max()))
    print(f"column 3 against the device torch path, scale={scale} {cloud} ({fclip if pick else ref.F} rows): "
          f"{differing} of {rows} entries differ, by at most {worst_ulp:.1f} ulp")
    assert differing == 0


@pytest.mark.parametrize("scale", ref.SCALES)
@pytest.mark.parametrize("T", ref.TS)
def test_target_clouds(T, scale):
    """Without freq: features inside the bound, column 3 = row / bins exactly, and the device torch path."""
    P = ref.spectrogram(T)
    fclip = int(ref.F * scale)
    lin, log = _points(P, scale=scale)
    worst, _ = _check_clouds(P, fclip, lin, log, None, None, (T, scale))
    print(f"target clouds T={T} scale={scale}: largest feature error / bound {worst:.3f}")
    _check_torch_path(P, fclip, lin, log, None, None, (T, scale))
    lin2, log2 = _points(P, scale=scale)
    assert torch.equal(lin, lin2) and torch.equal(log, log2)


def _raw_winners(P, fclip, f, sr):
    """ds_spec_points_fwd called directly: the winner table as (rows, 2) arrays (write q, entry e) / (-1, -1)."""
    from diffsound_amd import _hip

    Pt = _dev(P)
    B, F, T = Pt.shape
    lin = torch.empty((B, F, 4), device=DEV)
    log = torch.empty((B, fclip, 4), device=DEV)
    win = torch.empty(F + fclip, dtype=torch.int64, device=DEV)
    _hip.check(_hip.lib().ds_spec_points_fwd(Pt.data_ptr(), B, F, T, ref.EPS, fclip, f.data_ptr(), f.numel(), sr, win.data_ptr(),
                                             lin.data_ptr(), log.data_ptr(), _hip.stream_ptr()), "ds_spec_points_fwd")
    k = win.cpu().numpy().astype(np.uint64)
    q = (k >> np.uint64(56)).astype(np.int64) - 1
    e = np.where(q >= 0, (k & np.uint64((1 << 56) - 1)).astype(np.int64), -1)
    tab = np.stack([q, e], 1)
    return tab[:F], tab[F:]


@pytest.mark.parametrize("scale", ref.SCALES)
@pytest.mark.parametrize("sr", ref.SAMPLE_RATES)
def test_predicted_clouds_winners_and_gradient(sr, scale):
    """Every frequency case: column 3 and the winner tables equal the sequential reference exactly (collisions, the
    truncation cases, one ulp around an integer, NaN and inf, E = 1, the shapes); features inside the bound; the gradient
    to freq equals the reference's - autograd's rule: every entry of the write that owns a row is credited - to one fp32
    rounding (the kernel sums in fp64 and rounds once: 2 u relative allowed) and
    is bitwise the same on a second run; on the collision-free, finite cases the device torch path gives the same clouds."""
    fclip = int(ref.F * scale)
    rng = np.random.default_rng([sr, fclip])
    G = [rng.standard_normal((ref.B, ref.F, 4)).astype(np.float32), rng.standard_normal((ref.B, fclip, 4)).astype(np.float32)]
    Gd = [_dev(g) for g in G]
    worst, compared = 0.0, []
    for name, fnp in ref.freq_cases(sr).items():
        P = ref.spectrogram(17 if name in ("separated", "dense_tv") else 3, seed=1)
        f = _dev(fnp, grad=True)
        lin, log = _points(P, f, sr, scale)
        w, want = _check_clouds(P, fclip, lin, log, fnp, sr, name)
        worst = max(worst, w)
        wl, wg = _raw_winners(P, fclip, f.detach().reshape(-1), sr)
        assert np.array_equal(wl, want["win_lin"]) and np.array_equal(wg, want["win_log"]), name
        ((lin * Gd[0]).sum() + (log * Gd[1]).sum()).backward()
        g1 = f.grad.clone()
        gref = ref.grad_freq(fnp, sr, [want["win_lin"], want["win_log"]], G, "reciprocal").reshape(fnp.shape)
        assert g1.shape == f.shape
        err = np.abs(g1.cpu().numpy().astype(np.float64) - gref)
        assert (err <= 2 * ref.U32 * np.abs(gref)).all(), (name, float(err.max()))
        assert np.abs(gref).max() > 0, name
        f2 = _dev(fnp, grad=True)
        lin2, log2 = _points(P, f2, sr, scale)
        ((lin2 * Gd[0]).sum() + (log2 * Gd[1]).sum()).backward()
        assert torch.equal(lin, lin2) and torch.equal(log, log2) and torch.equal(f2.grad, g1), name
        if name != "nonfinite" and not (ref.has_collisions(ref.F, fnp, sr) or ref.has_collisions(fclip, fnp, sr)):
            _check_torch_path(P, fclip, lin, log, f.detach(), sr, name)
            compared.append(name)
    print(f"predicted clouds sr={sr} scale={scale}: largest feature error / bound {worst:.3f}; device torch path on {compared}")
    assert {"separated", "overlap", "single", "column"} <= set(compared)  # (low, high, ulp share rows inside one write)


@pytest.mark.parametrize("sr", ref.SAMPLE_RATES)
def test_expanded_view_reaches_its_base(sr):
    """An (A, m, S) expanded view: the clouds are those of the reference on all A m S entries; the gradient arrives at the
    (1, m, 1) base and equals the dense copy's gradient summed over the expanded dimensions - every one of the A S copies
    of a mode is credited (autograd's rule), the kernel scales the one kept entry by A S in fp64 and rounds once, the
    dense sum adds A S = 14 equal fp32 numbers: 14 u relative between them - and the reference's on all entries."""
    P = ref.spectrogram(3, seed=2)
    Gn = [np.random.default_rng(5).standard_normal((ref.B, n, 4)).astype(np.float32) for n in (ref.F, 16)]
    G = [_dev(g) for g in Gn]
    base = _dev(ref.expanded_base(sr), grad=True)
    view = base.expand(*ref.EXPANDED_SHAPE)
    lin, log = _points(P, view, sr, 0.5)
    _, want = _check_clouds(P, 16, lin, log, view.detach().cpu().numpy(), sr, "expanded")
    ((lin * G[0]).sum() + (log * G[1]).sum()).backward()
    dense = view.detach().clone().requires_grad_(True)
    lin_d, log_d = _points(P, dense, sr, 0.5)
    assert torch.equal(lin, lin_d) and torch.equal(log, log_d)
    ((lin_d * G[0]).sum() + (log_d * G[1]).sum()).backward()
    assert base.grad.shape == base.shape and float(base.grad.abs().max()) > 0
    got = base.grad.cpu().numpy().astype(np.float64)
    summed = dense.grad.sum((0, 2), keepdim=True).cpu().numpy().astype(np.float64)
    A, m, S = ref.EXPANDED_SHAPE
    assert (np.abs(got - summed) <= A * S * ref.U32 * np.abs(summed)).all()
    gref = ref.grad_freq(view.detach().cpu().numpy(), sr, [want["win_lin"], want["win_log"]], Gn, "reciprocal").reshape(A, m, S)
    assert (np.abs(dense.grad.cpu().numpy() - gref) <= 2 * ref.U32 * np.abs(gref)).all()
    gsum = gref.sum((0, 2), keepdims=True)
    assert (np.abs(got - gsum) <= 2 * ref.U32 * np.abs(gsum)).all()


def test_clouds_of_a_rendered_spectrogram_equal_the_torch_path():
    """spec2point(stft_power(...)) on two decaying clips, n_fft 64 (F = 33, T = 17), separated modes."""
    from diffsound_amd.ddsp.mss_loss import normlize, stft_power

    sr = 32000
    t = torch.arange(260, device=DEV) / sr
    x = torch.stack([(torch.exp(-60 * t) * torch.sin(2 * np.pi * f0 * t)) for f0 in (1900.0, 5200.0)])
    P = stft_power(normlize(x), ref.N_FFT, 16).cpu().numpy()
    assert P.shape == (2, 33, 17)
    fnp = ref.freq_cases(sr)["separated"]
    for scale in ref.SCALES:
        f = _dev(fnp)
        lin, log = _points(P, f, sr, scale)
        _check_clouds(P, int(33 * scale), lin, log, fnp, sr, "rendered")
        _check_torch_path(P, int(33 * scale), lin, log, f, sr, "rendered")


def test_errors_come_before_device_work():
    from diffsound_amd.ddsp.spec_points import spectral_points

    P = _dev(ref.spectrogram(3))
    f = _dev(ref.freq_cases(32000)["single"])
    with pytest.raises(RuntimeError, match="HIP"):
        spectral_points(P.cpu())
    with pytest.raises(ValueError, match="sample_rate"):
        spectral_points(P, f)
    with pytest.raises(ValueError, match="sample_rate"):
        spectral_points(P, f, 1)
    with pytest.raises(ValueError, match="scale"):
        spectral_points(P, f, 32000, scale=0.01)
    with pytest.raises(ValueError, match="scale"):
        spectral_points(P, scale=1.5)
    with pytest.raises(ValueError, match="one device"):
        spectral_points(P, f.cpu(), 32000)
    with pytest.raises(ValueError, match=r"\(batch, freq, time\)"):
        spectral_points(P[0])
    with pytest.raises(ValueError, match="eps"):
        spectral_points(P, eps=0.0)


# ------------------------------------------------------------------------------------------------- end to end
SR = 32000
MODES = [700.0, 1900.0, 3300.0, 5200.0, 7400.0, 10100.0]


@pytest.fixture
def shim(monkeypatch):
    """compat/ in front of sys.path with geomloss dropped from sys.modules; restored afterwards."""
    saved = sys.modules.pop("geomloss", None)
    monkeypatch.syspath_prepend(os.path.join(ROOT, "compat"))
    yield
    sys.modules.pop("geomloss", None)
    if saved is not None:
        sys.modules["geomloss"] = saved


def _render(shift=1.0):
    """(osc, f (m, 1) leaf, pred (2, 512)) of a 2-clip, 512-sample render."""
    from diffsound_amd.ddsp.oscillator import TraditionalDampedOscillator
    from diffsound_amd.diffelastic.material_model import Material, MatSet

    force = torch.zeros((2, 150), device=DEV)
    force[0, 0], force[1, 3] = 1.0, 0.7
    osc = TraditionalDampedOscillator(force, 2, len(MODES), 512, SR, Material(MatSet.Ceramic))
    f = (torch.tensor(MODES, device=DEV).reshape(-1, 1) * shift).requires_grad_(True)
    return osc, f, osc(f)


def _loss_and_grad(m, osc, f, pred, target):
    f.grad = None
    loss = m(pred, target, osc.damped_freq, 1)
    loss.backward(retain_graph=True)
    return float(loss.detach()), f.grad.detach().cpu().numpy().astype(np.float64).copy()


def test_fused_loss_equals_the_torch_cloud_path(shim, monkeypatch):  # noqa: PT
    """MSSLoss([64, 32], sr, type='geomloss') through the compat shim on a 2-clip, 512-sample render with
    osc.damped_freq: the fused front end against the same module with ``_fused_points = False``.  Bound: 4x what one
    fp32 ulp on every element of the torch path's clouds does to the loss and to the gradient (measured here)."""
    from diffsound_amd.ddsp import mss_loss
    from diffsound_amd.ddsp.mss_loss import MSSLoss
    from diffsound_amd.ddsp.sinkhorn import SamplesLoss

    osc, f0, target = _render()
    target = target.detach()
    osc, f, pred = _render(1.013)
    m = MSSLoss([64, 32], SR, type="geomloss")
    fused, g_fused = _loss_and_grad(m, osc, f, pred, target)
    assert all(isinstance(s.geomloss, SamplesLoss) and s._target_cache is not None for s in m.losses)
    for s in m.losses:
        s._fused_points = False
    plain, g_plain = _loss_and_grad(m, osc, f, pred, target)
    gen = torch.Generator().manual_seed(7)
    real = mss_loss.spec2point

    def one_ulp_off(x, freq=None, sample_rate=None):
        pts = real(x, freq, sample_rate)
        up = (torch.rand(pts.shape, generator=gen) < 0.5).to(pts.device)
        d = pts.detach()
        moved = torch.where(up, torch.nextafter(d, torch.full_like(d, float("inf"))),
                            torch.nextafter(d, torch.full_like(d, float("-inf"))))
        return pts + (moved - d)

    monkeypatch.setattr(mss_loss, "spec2point", one_ulp_off)
    moved, g_moved = _loss_and_grad(m, osc, f, pred, target)
    monkeypatch.setattr(mss_loss, "spec2point", real)
    b_loss, b_grad = 4 * abs(moved - plain), 4 * np.abs(g_moved - g_plain).max()
    e_loss, e_grad = abs(fused - plain), np.abs(g_fused - g_plain).max()
    print(f"fused {fused!r} torch clouds {plain!r}: |diff| {e_loss:.3e} (bound {b_loss:.3e}); "
          f"grad max |diff| {e_grad:.3e} (bound {b_grad:.3e}, largest |grad| {np.abs(g_plain).max():.3e})")
    assert np.isfinite(fused) and np.abs(g_plain).max() > 0
    assert e_loss <= b_loss
    return e_grad, b_grad, g_fused, g_plain


def test_fused_gradient_equals_the_torch_cloud_path(shim, monkeypatch):
    """``freq.grad`` of the same comparison, same kind of bound.

    osc.damped_freq is an (A = 2, m, S = 512) expanded view: autograd's backward of ``index_put_`` credits each of the 1024
    copies of a mode and the expand's backward adds them; the fused path collapses the view and scales by 1024."""
    e_grad, b_grad, g_fused, g_plain = test_fused_loss_equals_the_torch_cloud_path(shim, monkeypatch)
    print(f"ratio torch / fused gradient: {np.abs(g_plain).max() / np.abs(g_fused).max():.1f}")
    assert e_grad <= b_grad


class _CountingLib:
    """_hip.lib() with ds_stft_power counted; every other attribute is the library's."""

    def __init__(self, lib):
        self._lib, self.stft_calls = lib, 0

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def ds_stft_power(self, *a):
        self.stft_calls += 1
        return self._lib.ds_stft_power(*a)


def test_target_clouds_are_kept_until_the_target_changes(shim, monkeypatch):
    from diffsound_amd import _hip
    from diffsound_amd.ddsp.mss_loss import SSSLoss

    osc, _, target = _render()
    target = target.detach().clone()
    osc, f, pred = _render(1.013)
    s = SSSLoss(64, SR, type="geomloss")
    lib = _CountingLib(_hip.lib())
    monkeypatch.setattr(_hip, "lib", lambda: lib)
    first = s(pred, target, osc.damped_freq, 1)
    assert lib.stft_calls == 2                        # prediction and target
    clouds = s._target_cache[3]
    again = s(pred, target, osc.damped_freq, 1)
    assert lib.stft_calls == 3                        # the prediction alone
    assert s._target_cache[3] is clouds and torch.equal(first, again)
    s(pred, target, osc.damped_freq, 0.5)             # another scale: rebuilt
    assert lib.stft_calls == 5 and s._target_cache[3][1].shape[1] == 16
    s(pred, target, osc.damped_freq, 1)
    assert lib.stft_calls == 7
    kept = [c.clone() for c in s._target_cache[3]]
    target.mul_(0.5)
    target[:, 100:] = 0                               # in place: the same object, a new version, another spectrum
    s(pred, target, osc.damped_freq, 1)
    assert lib.stft_calls == 9
    assert not torch.equal(s._target_cache[3][0], kept[0])
    same_values = target.clone()                      # another object with the same values: identity is the key
    s(pred, same_values, osc.damped_freq, 1)
    assert lib.stft_calls == 11


def test_another_solver_class_takes_the_torch_path(shim, monkeypatch):
    from diffsound_amd.ddsp import mss_loss
    from diffsound_amd.ddsp.mss_loss import SSSLoss
    from diffsound_amd.ddsp.sinkhorn import SamplesLoss

    class Other(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.inner = SamplesLoss(loss="sinkhorn", p=2, blur=0.01)

        def forward(self, x, y):
            return self.inner(x, y)

    calls = {"fused": 0, "torch": 0}
    real_sp, real_s2p = mss_loss.spectral_points, mss_loss.spec2point
    monkeypatch.setattr(mss_loss, "spectral_points", lambda *a, **k: (calls.__setitem__("fused", calls["fused"] + 1), real_sp(*a, **k))[1])
    monkeypatch.setattr(mss_loss, "spec2point", lambda *a, **k: (calls.__setitem__("torch", calls["torch"] + 1), real_s2p(*a, **k))[1])
    osc, _, target = _render()
    osc, f, pred = _render(1.013)
    s = SSSLoss(64, SR, type="geomloss")
    s.geomloss = Other()
    loss = s(pred, target.detach(), osc.damped_freq, 1)
    assert bool(torch.isfinite(loss).all()) and calls == {"fused": 0, "torch": 4} and s._target_cache is None
    s.geomloss = None
    s(pred, target.detach(), osc.damped_freq, 1)
    assert calls == {"fused": 2, "torch": 4}


def test_fused_front_end_does_not_synchronise(shim):
    """normlize -> ds_stft_power -> spectral_points for the target and the prediction, and the backward to freq, under
    torch's synchronisation debug mode set to "error" (the solver, with its one bbox read per call, is outside)."""
    from diffsound_amd.ddsp.mss_loss import SSSLoss, normlize
    from diffsound_amd.ddsp.spec_points import spectral_points

    osc, _, target = _render()
    target = target.detach()
    osc, f, pred = _render(1.013)
    s = SSSLoss(64, SR, type="geomloss")
    G = torch.ones((2, 33, 4), device=DEV)
    probe = torch.ones(3, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            probe.sum().item()                        # the mode is live: a host read is refused
        lin_t, log_t = s._target_points(target, 1)
        lin, log = spectral_points(s.spec(normlize(pred)), osc.damped_freq, SR, 1, s.eps)
        ((lin * G).sum() + (log * G).sum()).backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.isfinite(f.grad).all() and float(f.grad.abs().max()) > 0 and lin_t.shape == lin.shape


def test_clouds_are_formed_on_the_operands_device():
    """The smallest call - one bin, one frame, one mode - forward and backward, with the operands off the current device."""
    from _guarded import same_on_other_device
    from diffsound_amd.ddsp.spec_points import spectral_points

    def run(device):
        P = torch.tensor([[[0.25]]], device=device)
        freq = torch.tensor([0.5], device=device, requires_grad=True)
        lin, log = spectral_points(P, freq, 2)
        return lin.detach(), log.detach(), torch.autograd.grad(lin[..., 3].sum() + 2 * log[..., 3].sum(), freq)[0]

    same_on_other_device(run)
