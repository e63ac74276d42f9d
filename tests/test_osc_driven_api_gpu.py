"""The driven oscillator bank through the Python layer (diffsound_amd/ddsp/oscillator.py): the dispatch of
``oscillator_bank`` between the FIR kernels and the recursive-resonator kernels, forces of any length in the modules, the
force gradient, and ``train_forces``.  References and bounds: tests/_osc_driven_ref.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _osc_driven_ref as D  # noqa: E402
import _osc_ref as R  # noqa: E402
from _guarded import _ratio, _up, dev as _dev, same_on_other_device  # noqa: E402

pytestmark = pytest.mark.gpu

SR = D.SR
MAT = (2700.0, 5e10, 0.25, 6.0, 1e-7)


def test_oscillator_bank_takes_513_taps():
    """On the FIR kernels alone this raised RuntimeError: ds_osc_bank_fwd: force length 513 not in 1..512."""
    from diffsound_amd.ddsp.oscillator import oscillator_bank

    case = (2, 5, 513, 700, "material", "dense", True)
    A, m, F, S = case[:4]
    d, w, amp, force, _ = D.inputs(case)
    y = oscillator_bank(_up(d), _up(w), _up(amp), _up(force), S, SR)
    assert y.shape == (A, S) and y.dtype == torch.float32 and bool(torch.isfinite(y).all())
    ref, Emag = D.forward(d, w, amp, force, S)
    assert _ratio("api.y513", None, y.cpu().numpy(), ref, D.bound_y(ref, Emag, A, m, S)) <= 1.0


def test_traditional_oscillator_with_a_long_force():
    from diffsound_amd.ddsp.oscillator import TraditionalDampedOscillator
    from diffsound_amd.diffelastic.material_model import Material

    A, m, F, S = 1, 8, 2000, 4000
    rng = np.random.default_rng(11)
    force = (rng.standard_normal((A, F)) * np.exp(-np.arange(F) / 400.0)).astype(np.float32)
    freq = torch.from_numpy(np.sort(rng.uniform(200.0, 9000.0, m)).astype(np.float32)).reshape(m, 1).to(_dev())
    osc = TraditionalDampedOscillator(torch.from_numpy(force), A, m, S, SR, Material(MAT)).cuda()
    assert osc.force_frame_num == F and osc.forces.shape == (A, 1, F)
    y = osc(freq)
    assert y.shape == (A, S)
    # d, w with the module's own operations on the device: the same bits the kernels were given
    f = freq.reshape(m).double()
    w0sq = (f * (2 * np.pi)) ** 2
    dd = 0.5 * (float(osc.alpha) + float(osc.beta) * w0sq)
    ww = torch.sqrt(w0sq - dd ** 2)
    ref, Emag = D.forward(dd.cpu().numpy(), ww.cpu().numpy(), None, force, S)
    assert _ratio("api.long", None, y.cpu().numpy(), ref, D.bound_y(ref, Emag, A, m, S)) <= 1.0
    assert sorted(osc.state_dict()) == []


def test_short_force_keeps_the_fir_path_bit_for_bit_and_the_driven_path_agrees():
    from diffsound_amd import _hip
    from diffsound_amd.ddsp.oscillator import oscillator_bank, oscillator_bank_driven

    case = (3, 17, 150, 2500, "material", "dense", True)
    A, m, F, S = case[:4]
    d, w, amp, force, _ = D.inputs(case)
    t_d, t_w, t_a, t_f = map(_up, (d, w, amp, force))
    y = oscillator_bank(t_d, t_w, t_a, t_f, S, SR)
    direct = torch.empty((A, S), dtype=torch.float32, device=_dev())
    p = _hip.ptr
    _hip.check(_hip.lib().ds_osc_bank_fwd(p(t_d), p(t_w), p(t_a), p(t_f), A, m, F, S, SR, p(direct), _hip.stream_ptr()),
               "ds_osc_bank_fwd")
    assert torch.equal(y, direct)
    drv = oscillator_bank_driven(t_d, t_w, t_a, t_f, S, SR)
    ref, Emag = D.forward(d, w, amp, force, S)
    _, E = R.bank_forward(d, w, amp, force, S, SR)
    b_drv, b_fir = D.bound_y(ref, Emag, A, m, S), R.bound_y(force, E, R.BANK_PARTIALS)
    assert _ratio("api.drv150", None, drv.cpu().numpy(), ref, b_drv) <= 1.0
    assert _ratio("api.cross150", None, drv.cpu().numpy(), y.cpu().numpy().astype(np.float64), b_drv + b_fir) <= 1.0


@pytest.mark.parametrize("F", [150, 700], ids=["F150-force-grad", "F700"])
def test_autograd_reaches_the_force(F):
    from diffsound_amd.ddsp.oscillator import oscillator_bank

    case = (2, 5, F, 1300, "material", "dense", True)
    A, m, _, S = case[:4]
    d, w, amp, force, gy = D.inputs(case)
    leaf = lambda x: _up(x).requires_grad_(True)
    t_d, t_w, t_a, t_f = leaf(d), leaf(w), leaf(amp), leaf(force)
    y = oscillator_bank(t_d, t_w, t_a, t_f, S, SR)
    gf, gd, gw, ga = torch.autograd.grad((y * _up(gy)).sum(), [t_f, t_d, t_w, t_a])
    assert gf.shape == (A, F) and gd.dtype == torch.float64 and gw.dtype == torch.float64
    b = D.backward(gy, d, w, amp, force)
    assert _ratio(f"api.gforce{F}", None, gf.cpu().numpy(), b["gforce"], D.bound_gforce(b["gforce"], b["Eg"], A, m, S)) <= 1.0
    assert _ratio(f"api.gd{F}", None, gd.cpu().numpy(), b["gd"], D.bound_gd_gw(b["W"], A, m, S)) <= 1.0
    assert _ratio(f"api.gw{F}", None, gw.cpu().numpy(), b["gw"], D.bound_gd_gw(b["W"], A, m, S)) <= 1.0
    assert _ratio(f"api.gamp{F}", None, ga.cpu().numpy(), b["gamp"], D.bound_gamp(b["gamp"], b["V"], A, m, S)) <= 1.0


def test_train_forces():
    from diffsound_amd.ddsp.oscillator import DampedOscillator, GTDampedOscillator, TraditionalDampedOscillator
    from diffsound_amd.diffelastic.material_model import Material

    A, m, F, S = 1, 8, 1200, 2400
    rng = np.random.default_rng(12)
    hit = np.exp(-np.arange(60) / 12.0)
    two_hits = np.zeros((A, F), dtype=np.float32)
    two_hits[:, :60] += hit
    two_hits[:, 900:960] += 0.6 * hit
    one_hit = np.zeros((A, F), dtype=np.float32)
    one_hit[:, :60] = hit
    freq = torch.from_numpy(np.sort(rng.uniform(300.0, 6000.0, m)).astype(np.float32)).reshape(m, 1).to(_dev())
    target = TraditionalDampedOscillator(torch.from_numpy(two_hits), A, m, S, SR, Material(MAT)).cuda()(freq).detach()

    osc = TraditionalDampedOscillator(torch.from_numpy(one_hit), A, m, S, SR, Material(MAT), train_forces=True).cuda()
    assert [k for k, _ in osc.named_parameters()] == ["force"] and sorted(osc.state_dict()) == ["force"]
    assert osc.force.shape == (A, F) and osc.force.is_cuda
    assert torch.equal(osc.forces.detach(), torch.flip(osc.force.detach().reshape(A, 1, F), [-1]))
    opt = torch.optim.Adam(osc.parameters(), lr=1e-2)
    loss0 = torch.nn.functional.mse_loss(osc(freq), target)
    opt.zero_grad()
    loss0.backward()
    assert osc.force.grad is not None and float(osc.force.grad.abs().max()) > 0
    opt.step()
    loss1 = torch.nn.functional.mse_loss(osc(freq), target)
    print(f"train_forces: mse {float(loss0):.6g} -> {float(loss1):.6g}")
    assert float(loss1) < float(loss0)

    # without the keyword nothing changes: the key lists of tests/test_api_gpu.py
    f_range = list(np.linspace(300.0, 9000.0, 40))
    forces = torch.from_numpy(one_hit[:, :150])
    assert sorted(TraditionalDampedOscillator(forces, A, m, S, SR, Material(MAT)).state_dict()) == []
    assert sorted(DampedOscillator(forces, A, m, S, SR, f_range, Material(MAT)).state_dict()) == [
        "alpha.params", "amp.value", "beta.params", "noise.coefficient_bank"]
    assert sorted(GTDampedOscillator(forces, A, m, 64, SR, f_range, Material(MAT)).state_dict()) == [
        "alpha.params", "amp.value", "beta.params", "freq_linear.params", "freq_nonlinear.params", "noise.coefficient_bank"]
    trained = DampedOscillator(forces, A, m, S, SR, f_range, Material(MAT), train_forces=True)
    assert sorted(trained.state_dict()) == ["alpha.params", "amp.value", "beta.params", "force", "noise.coefficient_bank"]


def test_time_varying_render_refuses_a_long_force():
    """The time-varying bank is no linear time-invariant filter per mode and stays on the FIR: ValueError before any device
    work (the module is still on the host, where a launch would have raised RuntimeError instead)."""
    from diffsound_amd.ddsp.oscillator import GTDampedOscillator
    from diffsound_amd.diffelastic.material_model import Material

    osc = GTDampedOscillator(torch.zeros((1, 513)), 1, 4, 64, SR, [100.0, 8000.0], Material(MAT))
    with pytest.raises(ValueError, match="512.*closed-form"):
        osc(non_linear_rate=0.05)
    assert osc.cuda()().shape == (1, 64)  # the closed-form render takes it


def _tiny_bank(entry, F):
    """``run(device)`` of ``entry`` at A = 1, m = 2, S = 64: forward and backward, every launch of the call."""
    def run(device):
        leaf = lambda x, dt: torch.tensor(x, dtype=dt, device=device).requires_grad_(True)
        d, w = leaf([3.0, 5.0], torch.float64), leaf([2 * np.pi * 440.0, 2 * np.pi * 1500.0], torch.float64)
        amp, force = leaf([[1.0, 0.5]], torch.float32), torch.linspace(1.0, 0.1, F, device=device).reshape(1, F)
        force.requires_grad_(entry.__name__ == "oscillator_bank_driven")
        y = entry(d, w, amp, force, 64, SR)
        weight = torch.linspace(-1.0, 1.0, 64, device=device)
        return (y.detach(),) + torch.autograd.grad((y * weight).sum(), [t for t in (d, w, amp, force) if t.requires_grad])
    return run


def test_banks_run_on_their_operands_device():
    """The FIR bank (F = 1) and the driven bank (F = S = 64) with operands off the current device."""
    from diffsound_amd.ddsp.oscillator import oscillator_bank, oscillator_bank_driven

    same_on_other_device(_tiny_bank(oscillator_bank, 1))
    same_on_other_device(_tiny_bank(oscillator_bank_driven, 64))
