"""The Python layer of the recording chain on the device (diffsound_amd/ddsp/biquad.py): ``biquad_cascade`` and its autograd,
torchaudio's two functions, ``ParametricEQ`` alone and in front of ``MSSLoss`` - all against the fp64 references and bounds
of tests/_biquad_ref.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _biquad_ref as BQ  # noqa: E402
from _guarded import _ratio, dev  # noqa: E402

from diffsound_amd.ddsp import biquad as Q  # noqa: E402

pytestmark = pytest.mark.gpu


def _six(c):
    """scipy's six columns with a0 = 2: every coefficient doubled."""
    return np.concatenate([2 * c[..., :3], np.full(c.shape[:-1] + (1,), 2.0), 2 * c[..., 3:]], -1)


@pytest.mark.parametrize("per_clip", [0, 1])
@pytest.mark.parametrize("cols", [5, 6])
@pytest.mark.parametrize("flat", [False, True])
def test_cascade_values_and_gradients(per_clip, cols, flat):
    """(N,) and (B, N); five and six columns; shared and per clip: y, x.grad and sos.grad within the kernel bounds."""
    B = 1 if flat else 3
    case = (B, 1025, 2, per_clip, "highpass")
    x, sos, gy = BQ.inputs(case)
    f = BQ.forward(x, sos)
    b = BQ.backward(gy, x, sos, f)
    tx = torch.from_numpy(x[0] if flat else x).to(dev()).requires_grad_(True)
    ts = torch.from_numpy(sos if cols == 5 else _six(sos)).to(dev()).requires_grad_(True)
    y = Q.biquad_cascade(tx, ts, check=True)
    assert y.shape == tx.shape and y.dtype == torch.float32
    y.backward(torch.from_numpy(gy[0] if flat else gy).to(dev()))
    assert _ratio("biquad.api.y", case, y.detach().cpu().numpy().reshape(B, -1), f["y"], f["y_bound"]) <= 1.0
    assert _ratio("biquad.api.gx", case, tx.grad.cpu().numpy().reshape(B, -1), b["gx"], b["gx_bound"]) <= 1.0
    ref, bound = (b["gsos"], b["gsos_bound"]) if per_clip else (b["gsos"].sum(0), b["gsos_bound"].sum(0) + 3 * BQ.U64 * np.abs(b["gsos"]).sum(0))
    got = ts.grad.cpu().numpy()
    assert got.shape == ts.shape
    if cols == 6:
        # d / d(six columns) with a0 = 2: the five named columns get half the gradient (one exact scaling and the sum's
        # rounding), a0 gets - sum_k c_k g_k / a0
        c = BQ.per_row(sos, B) if per_clip else sos
        ga0 = -(c * ref).sum(-1) / 2.0
        ba0 = (np.abs(c) * bound).sum(-1) / 2.0 + 8 * BQ.U64 * (np.abs(c * ref)).sum(-1)
        assert _ratio("biquad.api.ga0", case, got[..., 3], ga0, ba0) <= 1.0
        got, ref, bound = np.delete(got, 3, -1), ref / 2.0, bound / 2.0 + 2 * BQ.U64 * np.abs(ref)
    assert _ratio("biquad.api.gsos", case, got, ref, bound) <= 1.0


def test_highpass_biquad_is_the_design_through_the_cascade_clamped():
    rng = np.random.default_rng(3)
    x = (0.9 * rng.standard_normal((2, 3, 700))).astype(np.float32)          # leading dimensions, values past 1
    sos = Q.highpass_coeffs(44100, 100.0, 0.707).numpy().reshape(1, 5)
    f = BQ.forward(x.reshape(6, -1), sos)
    tx = torch.from_numpy(x).to(dev())
    raw = Q.highpass_biquad(tx, 44100, 100, clamp=False)
    got = Q.highpass_biquad(tx, 44100, 100)
    assert got.shape == tx.shape
    assert _ratio("biquad.highpass", None, raw.cpu().numpy().reshape(6, -1), f["y"], f["y_bound"]) <= 1.0
    over = raw.abs() > 1
    assert bool(over.any()) and torch.equal(got, raw.clamp(-1, 1)) and torch.equal(got != raw, over)
    lo = Q.lowpass_biquad(tx, 44100, 3000.0, clamp=False)
    fl = BQ.forward(x.reshape(6, -1), Q.lowpass_coeffs(44100, 3000.0, 0.707).numpy().reshape(1, 5))
    assert _ratio("biquad.lowpass", None, lo.cpu().numpy().reshape(6, -1), fl["y"], fl["y_bound"]) <= 1.0


def test_flat_parametric_eq_returns_its_input():
    rng = np.random.default_rng(4)
    x = rng.standard_normal((2, 2051)).astype(np.float32)
    eq = Q.ParametricEQ(3, 44100, [150.0, 2000.0, 9000.0], Q=[0.7, 4.0, 1.0]).to(dev())
    sos = eq.coefficients().detach().cpu().numpy()
    f = BQ.forward(x, sos)
    assert np.abs(f["y"] - x).max() < 1e-9                                   # the reference: the identity up to fp64 rounding
    y = eq(torch.from_numpy(x).to(dev()))
    assert _ratio("biquad.eq.flat", None, y.detach().cpu().numpy(), x.astype(np.float64), f["y_bound"] + np.abs(f["y"] - x)) <= 1.0


def test_parametric_eq_trains_through_the_spectral_loss():
    """MSSLoss([256, 64], l1) of eq(audio) against a target, N = 4096, two peaking sections: the autograd gradient to
    (log f0, log Q, gain_db) against the same quantity built without the code under test - the fp64 numpy gsos fed the
    loss's own gradient at the output, pushed through the design functions' autograd on the CPU in fp64.  Tolerance: the
    kernel's gsos bound through the absolute Jacobian of the designs, plus 2e-5 (the spectral loss's own accuracy,
    tests/test_mss_loss.py) of the absolute terms."""
    from diffsound_amd.ddsp.mss_loss import MSSLoss

    sr, N = 16000, 4096
    rng = np.random.default_rng(5)
    audio = (0.3 * rng.standard_normal((1, N))).astype(np.float32)
    target = (0.3 * rng.standard_normal((1, N))).astype(np.float32)
    make = lambda: Q.ParametricEQ(2, sr, [400.0, 2500.0], Q=[1.5, 0.8], gain_db=[4.0, -3.0])
    eq = make().to(dev())
    out = eq(torch.from_numpy(audio).to(dev()))
    out.retain_grad()
    loss = MSSLoss([256, 64], sr, type="l1_loss").to(dev())(out, torch.from_numpy(target).to(dev()))
    loss.backward()
    g_out = out.grad.cpu().numpy()

    cpu = make()
    names = ("log_f0", "log_Q", "gain_db")
    sos = cpu.coefficients()
    b = BQ.backward(g_out, audio, sos.detach().numpy())
    gref, gbound = b["gsos"].sum(0), b["gsos_bound"].sum(0)
    (sos * torch.from_numpy(gref)).sum().backward()
    params = tuple(getattr(cpu, n) for n in names)
    J = torch.autograd.functional.jacobian(
        lambda *p: Q.peaking_coeffs(sr, torch.exp(cpu.lo + (cpu.hi - cpu.lo) * torch.sigmoid(p[0])), torch.exp(p[1]), p[2]), params)
    worst = 0.0
    for n, p, j in zip(names, params, J):                                    # j: (S, 5, S)
        aj = j.abs().numpy()
        tol = np.einsum("skp,sk->p", aj, gbound + 2e-5 * np.abs(gref))
        got = getattr(eq, n).grad.cpu().numpy()
        frac = np.abs(got - p.grad.numpy()) / tol
        print(f"FRACTION biquad.eq.{n} {frac.max():.4g}")
        worst = max(worst, float(frac.max()))
        assert np.abs(p.grad.numpy()).min() > 0
    assert worst <= 1.0


def test_check_names_the_unstable_section():
    x = torch.zeros(2, 64, device=dev())
    good, bad = torch.from_numpy(BQ.SETS["real"]), torch.tensor([1.0, 0.0, 0.0, 0.0, 1.01], dtype=torch.float64)
    with pytest.raises(ValueError, match="section 1 is unstable"):
        Q.biquad_cascade(x, torch.stack([good, bad]), check=True)
    with pytest.raises(ValueError, match="section 0 of row 1 is unstable"):
        Q.biquad_cascade(x, torch.stack([torch.stack([good, good]), torch.stack([bad, good])]), check=True)
    with pytest.raises(ValueError, match="section 1 is unstable"):            # six columns: after the division by a0
        Q.biquad_cascade(x, torch.stack([torch.tensor(_six(BQ.SETS["real"])), torch.tensor(_six(bad.numpy()))]), check=True)
    assert Q.biquad_cascade(x, torch.stack([good, bad])).shape == x.shape     # unchecked: runs


def test_value_errors_come_before_any_device_call(monkeypatch):
    """With the library handle taken away every device call would raise; the ValueErrors still come."""
    from diffsound_amd import _hip

    def no_lib():
        raise AssertionError("device call")

    monkeypatch.setattr(_hip, "lib", no_lib)
    x, sos = torch.zeros(3, 40, device=dev()), torch.zeros(2, 5, dtype=torch.float64, device=dev())
    for xx, ss, text in [(x.reshape(3, 2, 20), sos, "x must be"), (x, sos[0], "sos must be"), (x, sos[:, :4], "sos must be"),
                         (x, sos.expand(2, 2, 5), "per clip with B = 2"), (x, sos[:1].expand(17, 5), "17 sections"),
                         (x[:, :0], sos, "empty signal")]:
        with pytest.raises(ValueError, match=text):
            Q.biquad_cascade(xx, ss)
    with pytest.raises(AssertionError, match="device call"):
        Q.biquad_cascade(x, sos)
