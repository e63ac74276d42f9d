"""``contact_force`` and ``HertzHammer`` (diffsound_amd/ddsp/contact.py) end to end on the device: the gradients that
autograd carries from a rendered sound back to the hammer, the refusals, and the recovery of a hammer from its force."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _contact_ref as C  # noqa: E402
from _guarded import _ratio, dev  # noqa: E402

pytestmark = pytest.mark.gpu

LD = np.longdouble


def test_hammer_to_sound_gradients_match_the_adjoint():
    """HertzHammer -> oscillator_bank -> sum of squares.  The gforce autograd hands to the contact backward is read off
    ``force.grad`` and fed to the numpy adjoint; the parameters' gradients (chain rule of the log parameters applied here)
    must lie within the kernel test's bounds.  d, w and gain enter the hammer as leaves of their own, so that their
    gradients are the contact's alone."""
    from diffsound_amd.ddsp import HertzHammer
    from diffsound_amd.ddsp.bank import oscillator_bank

    case = C.CASES[9]  # three clips, 70 modes, different hammers
    A, m, F, R, p, kH, M, v0, _ = case
    d, w, c, M, v0, kH, _ = C.inputs(case)
    S = 256
    t = lambda x: torch.from_numpy(x).to(dev())  # noqa: E731
    hammer = HertzHammer(A, t(M), t(v0), t(kH), exponent=p, oversample=R).to(dev())
    # the mass and the stiffness the kernels are handed: exp(log(.)) as the device rounds it, not the table's numbers
    M, kH = hammer.log_mass.detach().exp().cpu().numpy(), hammer.log_stiffness.detach().exp().cpu().numpy()
    d_c, w_c, gain = (t(x).requires_grad_(True) for x in (d, w, c))
    amp = torch.full((A, m), 0.5, dtype=torch.float32, device=dev())
    force = hammer(d_c, w_c, gain, F, C.SR)
    assert force.shape == (A, F) and force.dtype == torch.float32 and force.requires_grad
    force.retain_grad()
    y = oscillator_bank(t(d), t(w), amp * t(c).float(), force, S, C.SR)
    y.square().sum().backward()
    torch.cuda.synchronize()
    gforce = force.grad.cpu().numpy()
    assert np.abs(gforce).max() > 0
    r64, rld = (C.adjoint(gforce, d, w, c, M, v0, kH, p, R, dtype=dt) for dt in (np.float64, LD))
    chain = lambda r: dict(gd=r["gd"], gw=r["gw"], gc=r["gc"], log_mass=r["gM"] * M, velocity=r["gv0"],  # noqa: E731
                           log_stiffness=r["gkH"] * kH)
    r64, rld = chain(r64), chain(rld)
    got = dict(gd=d_c.grad, gw=w_c.grad, gc=gain.grad, log_mass=hammer.log_mass.grad, velocity=hammer.velocity.grad,
               log_stiffness=hammer.log_stiffness.grad)
    for k, g in got.items():
        assert g is not None and g.dtype == torch.float64, k
        truth = np.asarray(rld[k], dtype=np.float64)
        assert _ratio("contact.api." + k, None, g.cpu().numpy(), truth, C.bound(r64[k], rld[k])) <= 1.0, k


def test_gradients_only_where_needed():
    from diffsound_amd.ddsp import HertzHammer

    d, w, c, M, v0, kH, g = C.inputs(C.CASES[0])
    t = lambda x: torch.from_numpy(x).to(dev())  # noqa: E731
    hammer = HertzHammer(1, 0.01, 1.0, 1e7, train_mass=False, train_velocity=False).to(dev())
    gain = t(c).requires_grad_(True)
    force = hammer(t(d), t(w), gain, 64, C.SR)
    force.square().sum().backward()
    assert hammer.log_mass.grad is None and hammer.velocity.grad is None
    assert hammer.log_stiffness.grad is not None and gain.grad is not None and float(gain.grad.abs().max()) > 0
    frozen = HertzHammer(1, 0.01, 1.0, 1e7, train_mass=False, train_velocity=False, train_stiffness=False).to(dev())
    assert not frozen(t(d), t(w), t(c), 64, C.SR).requires_grad


def test_refusals_come_before_device_work():
    from diffsound_amd.ddsp import contact_force

    d, w, c, M, v0, kH, _ = C.inputs(C.CASES[0])
    t = lambda x: torch.from_numpy(x).to(dev())  # noqa: E731
    good = dict(d=t(d), w=t(w), gain=t(c), mass=t(M), velocity=t(v0), stiffness=t(kH), force_len=8, sr=C.SR)
    bad = [(dict(w=-t(w)), "w must be positive"), (dict(mass=t(M) * 0), "mass and stiffness"),
           (dict(stiffness=-t(kH)), "mass and stiffness"), (dict(velocity=t(v0) * float("nan")), "velocity is not finite"),
           (dict(d=t(d) * float("inf")), "d is not finite"), (dict(gain=t(c)[:, :3]), "gain must be"),
           (dict(mass=t(M).repeat(2)), "mass must be"), (dict(w=t(w)[:2]), "d and w must be"),
           (dict(oversample=65), "oversample"), (dict(exponent=0.9), "exponent"), (dict(force_len=0), "below 1")]
    for change, text in bad:
        with pytest.raises(ValueError, match=text):
            contact_force(**dict(good, **change))
    for name in ("d", "gain", "velocity"):
        with pytest.raises(RuntimeError, match="HIP device"):
            contact_force(**dict(good, **{name: good[name].cpu()}))
    assert float(contact_force(**good).abs().max()) > 0


def test_recovery_of_stiffness_and_speed_from_the_force():
    """The target force comes from (kH, v0); from (2 kH, 0.7 v0), 80 Adam steps on (log kH, v0) with the squared error of the
    force as the loss - the steps tests/test_contact_ref_cpu.py runs on the restatement, here through ``contact_force`` and
    autograd.  The loss must end below ten times the restatement's final ratio or below 1e-3 of its start, whichever is
    larger."""
    from diffsound_amd.ddsp import contact_force

    d, w, c, M, kH, v0 = C.recovery_problem()
    F, R, p = C.RECOVERY["F"], C.RECOVERY["R"], C.RECOVERY["p"]
    t = lambda x: torch.from_numpy(x).to(dev())  # noqa: E731
    d_d, d_w, d_c, d_M = t(d), t(w), t(c), t(M)
    target = contact_force(d_d, d_w, d_c, d_M, t(v0), t(kH), F, C.SR, p, R).double()

    def lg(theta):
        th = t(theta).requires_grad_(True)
        force = contact_force(d_d, d_w, d_c, d_M, th[1:], th[:1].exp(), F, C.SR, p, R)
        loss = (force.double() - target).square().sum()
        loss.backward()
        return float(loss), th.grad.cpu().numpy()

    _, losses = C.adam(lg, [np.log(2 * kH[0]), 0.7 * v0[0]], C.RECOVERY["steps"], C.RECOVERY["lr"])
    ratio, ref = losses[-1] / losses[0], C.recovery_numpy()
    print(f"RATIO contact.recovery.device {ratio:.3g} numpy {ref:.3g}")
    assert ref < 1e-3
    assert ratio <= max(10 * ref, 1e-3)
