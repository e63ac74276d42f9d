"""The Python layer of the room response on the device (diffsound_amd/ddsp/reverb.py): ``fir_convolve`` and its autograd
against torch's fp64 ``conv1d`` on the CPU at the bounds of tests/_fir_ref.py, ``RoomResponse`` alone, fitted one step, and
between ``ParametricEQ`` and ``MSSLoss``."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _fir_ref as F  # noqa: E402
from _guarded import _ratio, dev  # noqa: E402

from diffsound_amd.ddsp import reverb as V  # noqa: E402

pytestmark = pytest.mark.gpu


def _conv1d(x, h, gy):
    """y, gx, gh from torch on the CPU in fp64: conv1d with one group a row, the kernel flipped, the row padded in front."""
    B, N = x.shape
    H, L = h.shape
    tx = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
    th = torch.from_numpy(h).requires_grad_(True)
    w = th[torch.arange(B) % H].flip(-1).unsqueeze(1)                                   # (B, 1, L)
    y = torch.nn.functional.conv1d(torch.nn.functional.pad(tx, (L - 1, 0)).unsqueeze(0), w, groups=B)[0]
    y.backward(torch.from_numpy(gy.astype(np.float64)))
    return y.detach().numpy(), tx.grad.numpy(), th.grad.numpy()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("flat_h", [False, True], ids=["hHL", "hL"])
@pytest.mark.parametrize("flat_x", [False, True], ids=["xBN", "xN"])
def test_convolve_values_and_gradients(flat_x, flat_h, dtype):
    """(N,) and (B, N); (L,) and (H, L); fp32 and fp64 x: y, x.grad and h.grad against conv1d, at the kernel's bounds (P and n
    from the fp64 reference; conv1d's own sum is granted as much again: it is not compensated)."""
    B, H = (1, 1) if flat_x else ((4, 1) if flat_h else (4, 2))
    case = (B, H, 600, 2 * F.TAPS + 1)
    (x, h, gy), f, b = F.reference(case)
    ry, rgx, rgh = _conv1d(x, h, gy)
    tx = torch.from_numpy(x[0] if flat_x else x).to(dev(), dtype).requires_grad_(True)
    th = torch.from_numpy(h[0] if flat_h else h).to(dev()).requires_grad_(True)
    y = V.fir_convolve(tx, th)
    assert y.shape == tx.shape and y.dtype == dtype
    y.backward(torch.from_numpy(gy[0] if flat_x else gy).to(dev(), dtype))
    assert tx.grad.shape == tx.shape and th.grad.shape == th.shape and th.grad.dtype == torch.float64
    n = f["n"]
    assert _ratio("fir.api.y", case, y.detach().cpu().numpy().reshape(B, -1), ry, f["bound"] + n * F.U64 * f["P"]) <= 1.0
    assert _ratio("fir.api.gx", case, tx.grad.cpu().numpy().reshape(B, -1), rgx, b["gx_bound"] + n[::-1] * F.U64 * b["gx_P"]) <= 1.0
    assert _ratio("fir.api.gh", case, th.grad.cpu().numpy().reshape(H, -1), rgh, 2 * b["gh_bound"]) <= 1.0


def test_a_gradient_nobody_needs_is_not_computed(monkeypatch):
    from diffsound_amd import _hip

    lib, seen = _hip.lib(), []

    class Spy:
        def __getattr__(self, name):
            fn = getattr(lib, name)
            if name != "ds_fir_bwd":
                return fn
            return lambda *a: (seen.append((a[7], a[9], a[10])), fn(*a))[1]

    monkeypatch.setattr(_hip, "lib", lambda: Spy())
    x = torch.randn(2, 300, device=dev())
    h = torch.randn(1, 40, dtype=torch.float64, device=dev())
    V.fir_convolve(x.clone().requires_grad_(True), h).sum().backward()
    V.fir_convolve(x, h.clone().requires_grad_(True)).sum().backward()
    (w0, gx0, gh0), (w1, gx1, gh1) = seen
    assert gx0 and gh0 is None and w0 is None and gx1 is None and gh1 and w1


def test_value_errors_come_before_any_device_call(monkeypatch):
    """With the library handle taken away every device call would raise; the ValueErrors still come."""
    from diffsound_amd import _hip

    def no_lib():
        raise AssertionError("device call")

    monkeypatch.setattr(_hip, "lib", no_lib)
    x, h = torch.zeros(6, 40, device=dev()), torch.zeros(3, 5, dtype=torch.float64, device=dev())
    for xx, hh, text in [(x.reshape(3, 2, 40), h, "x must be"), (x, h.reshape(3, 5, 1), "h must be"), (x[:, :0], h, "empty signal"),
                         (x, h[:, :0], "empty response"), (x, h[:0], "empty response"), (x, torch.zeros(4, 5), "not a multiple"),
                         (x[:2], h, "not a multiple"), (x, torch.zeros(1, 65537), "65537 taps"),
                         (torch.zeros(65536, 1).expand(65536, 4), h[:1], "65536 rows"), (x.long(), h, "floating-point")]:
        with pytest.raises(ValueError, match=text):
            V.fir_convolve(xx, hh)
    with pytest.raises(AssertionError, match="device call"):
        V.fir_convolve(x, h)


def test_cpu_tensors_are_refused():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        V.fir_convolve(torch.zeros(2, 40), torch.zeros(1, 5))


def test_zero_room_returns_its_input_bit_for_bit():
    room = V.RoomResponse(2, 3000, 32000).to(dev())
    assert {k: tuple(v.shape) for k, v in room.state_dict().items()} == {"ir": (2, 2999)}
    assert room.ir.dtype == torch.float64 and tuple(room.impulse_response().shape) == (2, 3000)
    x = torch.from_numpy(F.spread(np.random.default_rng(7), (3, 2, 1500), -3, 1).astype(np.float32)).to(dev())
    y = room(x)
    assert y.shape == x.shape and torch.equal(y.view(torch.int32), x.view(torch.int32))


def test_decay_initialisation():
    sr, L, rt60, wet = 32000.0, 12000, 0.25, -12.0
    a, b, c = (V.RoomResponse(2, L, sr, init="decay", rt60=rt60, wet_db=wet, seed=s) for s in (3, 3, 4))
    assert torch.equal(a.ir, b.ir) and not torch.equal(a.ir, c.ir) and not torch.equal(a.ir[0], a.ir[1])
    assert torch.equal(a.impulse_response()[:, 0], torch.ones(2, dtype=torch.float64))
    env = V.RoomResponse.decay_envelope(L, sr, rt60, wet)                    # the noiseless envelope, lags 1 .. L - 1
    k = int(round(rt60 * sr))                                                # the lag at rt60
    down = 20 * math.log10(float(env[k - 1]) / 10 ** (wet / 20))
    assert abs(down + 60.0) < 0.05                                           # 6.91 for ln 1000 = 6.9078: 60.02 dB
    assert abs(float(env[0]) / 10 ** (wet / 20) - math.exp(-6.91 / sr / rt60)) < 1e-15
    # the taps are that envelope times unit-variance noise
    z = a.ir.detach() / env
    assert abs(float(z.mean())) < 5 / math.sqrt(z.numel()) and abs(float(z.std()) - 1) < 0.05
    with pytest.raises(ValueError, match="rt60"):
        V.RoomResponse(1, 100, sr, init="decay")
    with pytest.raises(ValueError, match="neither"):
        V.RoomResponse(1, 100, sr, init="ones")


def test_response_is_the_dft_of_the_impulse_response():
    sr, L = 16000.0, 512
    room = V.RoomResponse(2, L, sr, init="decay", rt60=0.01, wet_db=-6.0, seed=1)
    freqs = torch.arange(L // 2 + 1, dtype=torch.float64) * sr / L
    got = room.response(freqs)
    ref = torch.fft.rfft(room.impulse_response().detach(), dim=-1)
    assert got.dtype == torch.complex128 and got.shape == ref.shape and got.requires_grad
    scale = room.impulse_response().detach().abs().sum(1, keepdim=True)
    assert float(((got.detach() - ref).abs() / scale).max()) < 64 * L * F.U64   # phases of up to pi L radians, each a few U64 off relatively: 4 pi L U64
    got.abs().sum().backward()
    assert room.ir.grad is not None and bool(room.ir.grad.abs().sum() > 0)


def test_one_gradient_step_fits_the_target():
    """Squared error against a target made by a known response.  The loss is quadratic in ir; per response its Hessian is
    2 sum_{b of that response} X_b^T X_b, X_b the convolution by row b, and ||X_b d||_2 <= ||x_b||_1 ||d||_2 (Young), so the
    gradient is Lipschitz with Lip <= 2 (B / H) ||x||_1^2, ||x||_1 the largest row's.  A step eta = 1 / (B ||x||_1^2) along the
    negative gradient g has eta Lip / 2 <= 1 / H = 1 / 2 and lowers the loss by at least eta (1 - eta Lip / 2) ||g||^2 >=
    eta ||g||^2 / 2: guaranteed, not hoped for.  The minimiser is the known response, and a step of eta <= 2 / Lip on a convex
    quadratic does not move away from it."""
    B, N, L = 4, 1500, 2 * F.TAPS + 1
    rng = np.random.default_rng(9)
    x = torch.from_numpy(rng.standard_normal((B, N)).astype(np.float32)).to(dev())
    known = V.RoomResponse(2, L, 32000, init="decay", rt60=0.004, wet_db=-6.0, seed=5).to(dev())
    target = known(x).detach()
    room = V.RoomResponse(2, L, 32000).to(dev())
    loss = lambda: ((room(x) - target).double() ** 2).sum()
    before = loss()
    before.backward()
    g = room.ir.grad
    assert bool(g.abs().sum() > 0)
    eta = 1.0 / (B * float(x.double().abs().sum(1).max()) ** 2)
    with torch.no_grad():
        room.ir -= eta * g
    after = loss()
    gain = float(before - after)
    print(f"FIT loss {float(before):.6g} -> {float(after):.6g}; guaranteed {0.5 * eta * float((g * g).sum()):.6g}")
    assert float(after) < float(before)
    assert gain >= 0.5 * eta * float((g * g).sum())                        # the guaranteed decrease
    # and in the right direction: towards the known response
    d0 = float((known.ir.detach()).norm())
    assert float((room.ir.detach() - known.ir.detach()).norm()) < d0


def test_eq_room_and_spectral_loss_train_together():
    from diffsound_amd.ddsp.biquad import ParametricEQ
    from diffsound_amd.ddsp.mss_loss import MSSLoss

    sr, N = 16000, 4096
    rng = np.random.default_rng(5)
    audio = torch.from_numpy((0.3 * rng.standard_normal((2, N))).astype(np.float32)).to(dev())
    target = torch.from_numpy((0.3 * rng.standard_normal((2, N))).astype(np.float32)).to(dev())
    eq = ParametricEQ(2, sr, [400.0, 2500.0], Q=[1.5, 0.8], gain_db=[4.0, -3.0]).to(dev())
    room = V.RoomResponse(1, 800, sr, init="decay", rt60=0.02, wet_db=-10.0, seed=2).to(dev())
    mss = MSSLoss([256, 64], sr, type="l1_loss").to(dev())
    mss(room(eq(audio)), target).backward()
    params = list(eq.parameters()) + list(room.parameters()) + list(mss.parameters())
    assert len(list(eq.parameters())) == 3 and len(list(room.parameters())) == 1
    for p in params:
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool(p.grad.abs().sum() > 0)
