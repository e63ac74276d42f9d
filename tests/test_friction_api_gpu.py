"""``friction_force`` and ``Bow`` (diffsound_amd/ddsp/friction.py) end to end on the device: the gradients that autograd
carries from a rendered sound back to the stroke, the refusals, and the recovery of a stroke from its force."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _friction_ref as Fr  # noqa: E402
from _guarded import _ratio, dev  # noqa: E402

pytestmark = pytest.mark.gpu

LD = np.longdouble


def test_bow_to_sound_gradients_match_the_adjoint():
    """Bow -> oscillator_bank -> sum of squares.  The gforce autograd hands to the friction backward is read off
    ``force.grad`` and fed to the numpy adjoint together with the gesture the module formed; the parameters' gradients (the
    chain rule of the envelope and of the log parameters applied here) must lie within the kernel test's bounds.  d, w and
    gain enter the bow as leaves of their own, so that their gradients are the friction's alone."""
    from diffsound_amd.ddsp import Bow
    from diffsound_amd.ddsp.bank import oscillator_bank

    A, m, F, R, S = 3, 70, 33, 8, 256
    rng = np.random.default_rng(79)
    d, w = Fr.modes(m, rng)
    c = rng.uniform(0.5, 1.5, (A, m)) * rng.choice([-1.0, 1.0], (A, m)) / np.sqrt(m)
    t = lambda x: torch.from_numpy(x).to(dev())  # noqa: E731
    bow = Bow(A, F, Fr.SR, [0.3, 0.101, -0.2], [40.0, 120.0, 60.0], stribeck_velocity=[0.1, 0.1, 0.12], attack=4 / Fr.SR,
              release=6 / Fr.SR, oversample=R).to(dev())
    # the gesture the kernels are handed: the module's own products, as the device rounds them
    vb, N = (x.detach().cpu().numpy() for x in bow.gesture())
    vs, P = bow.log_stribeck.detach().exp().cpu().numpy(), bow.log_pressure.detach().exp().cpu().numpy()
    env = bow.envelope.cpu().numpy()
    assert np.allclose(env, Fr.envelope(F, Fr.SR, 4 / Fr.SR, 6 / Fr.SR), rtol=0, atol=1e-15)
    d_c, w_c, gain = (t(x).requires_grad_(True) for x in (d, w, c))
    amp = torch.full((A, m), 0.5, dtype=torch.float32, device=dev())
    force = bow(d_c, w_c, gain)
    assert force.shape == (A, F) and force.dtype == torch.float32 and force.requires_grad
    force.retain_grad()
    y = oscillator_bank(t(d), t(w), amp * t(c).float(), force, S, Fr.SR)
    y.square().sum().backward()
    torch.cuda.synchronize()
    gforce = force.grad.cpu().numpy()
    assert np.abs(gforce).max() > 0
    r64, rld = (Fr.adjoint(gforce, d, w, c, vb, N, vs, R, dtype=dt) for dt in (np.float64, LD))
    chain = lambda r: dict(gd=r["gd"], gw=r["gw"], gc=r["gc"], velocity=(r["gvb"] * env).sum(-1),  # noqa: E731
                           log_pressure=(r["gN"] * env).sum(-1) * P, log_stribeck=r["gvs"] * vs)
    r64, rld = chain(r64), chain(rld)
    got = dict(gd=d_c.grad, gw=w_c.grad, gc=gain.grad, velocity=bow.velocity.grad, log_pressure=bow.log_pressure.grad,
               log_stribeck=bow.log_stribeck.grad)
    for k, g in got.items():
        assert g is not None and g.dtype == torch.float64, k
        assert Fr.e64(r64[k], rld[k])[0] <= Fr.E64_MAX, k
        truth = np.asarray(rld[k], dtype=np.float64)
        assert _ratio("friction.api." + k, None, g.cpu().numpy(), truth, Fr.bound(r64[k], rld[k])) <= 1.0, k


def test_gradients_only_where_needed_and_in_the_inputs_dtypes():
    from diffsound_amd.ddsp import Bow, friction_force

    d, w, c, vb, N, vs, g = Fr.inputs(Fr.CASES[0])
    t = lambda x: torch.from_numpy(x).to(dev())  # noqa: E731
    bow = Bow(1, 64, Fr.SR, 0.15, 60.0, attack=8 / Fr.SR, release=8 / Fr.SR, train_velocity=False, train_stribeck=False).to(dev())
    gain = t(c).requires_grad_(True)
    force = bow(t(d), t(w), gain)
    force.square().sum().backward()
    assert bow.velocity.grad is None and bow.log_stribeck.grad is None
    assert bow.log_pressure.grad is not None and gain.grad is not None and float(gain.grad.abs().max()) > 0
    frozen = Bow(1, 64, Fr.SR, 0.15, 60.0, train_velocity=False, train_pressure=False, train_stribeck=False).to(dev())
    assert not frozen(t(d), t(w), t(c)).requires_grad
    # fp32 inputs: fp64 inside, fp32 gradients back
    ops = [t(x).float().requires_grad_(True) for x in (d, w, c, vb, N, vs)]
    friction_force(*ops, Fr.SR).square().sum().backward()
    assert all(o.grad is not None and o.grad.dtype == torch.float32 and o.grad.shape == o.shape for o in ops)


def test_refusals_come_before_device_work():
    from diffsound_amd.ddsp import friction_force

    d, w, c, vb, N, vs, _ = Fr.inputs(Fr.CASES[3])
    t = lambda x: torch.from_numpy(x).to(dev())  # noqa: E731
    good = dict(d=t(d), w=t(w), gain=t(c), bow_velocity=t(vb), normal_force=t(N), stribeck_velocity=t(vs), sr=Fr.SR)
    bad = [(dict(w=-t(w)), "w must be positive"), (dict(d=t(d) * 0), "d must be positive"),
           (dict(normal_force=t(N) - 1.0), "normal_force must not be negative"),
           (dict(stribeck_velocity=t(vs) * 0), "stribeck_velocity must be positive"),
           (dict(bow_velocity=t(vb) * float("nan")), "bow_velocity is not finite"), (dict(d=t(d) * float("inf")), "d is not finite"),
           (dict(gain=t(c)[:, :3]), "gain must be"), (dict(normal_force=t(N)[:, :5]), "normal_force must be"),
           (dict(bow_velocity=t(vb)[:2]), "bow_velocity must be"), (dict(stribeck_velocity=t(vs).repeat(2)), "stribeck_velocity must be"),
           (dict(w=t(w)[:2]), "d and w must be"), (dict(oversample=65), "oversample"), (dict(oversample=0), "oversample"),
           (dict(sr=-1.0), "sr")]
    for change, text in bad:
        with pytest.raises(ValueError, match=text):
            friction_force(**dict(good, **change))
    for name in ("d", "gain", "normal_force", "stribeck_velocity"):
        with pytest.raises(RuntimeError, match="HIP device"):
            friction_force(**dict(good, **{name: good[name].cpu()}))
    assert float(friction_force(**good).abs().max()) > 0


def test_recovery_of_pressure_and_speed_from_the_force():
    """The target force comes from (pressure, velocity); from (1.5 pressure, 0.8 velocity), 80 Adam steps on (log pressure,
    velocity) with the squared error of the force as the loss - the steps tests/test_friction_ref_cpu.py runs on the
    restatement, here through ``friction_force`` and autograd.  The device's loss ratio end / start must lie within a factor 2
    of the restatement's."""
    from diffsound_amd.ddsp import friction_force

    d, w, c, env, P, V = Fr.recovery_problem()
    R = Fr.RECOVERY["R"]
    t = lambda x: torch.from_numpy(np.asarray(x, dtype=np.float64)).to(dev())  # noqa: E731
    d_d, d_w, d_c, d_env, d_vs = t(d), t(w), t(c), t(env)[None, :], t([Fr.RECOVERY["vs"]])
    target = friction_force(d_d, d_w, d_c, V * d_env, P * d_env, d_vs, Fr.SR, R).double()

    def lg(theta):
        th = t(theta).requires_grad_(True)
        force = friction_force(d_d, d_w, d_c, th[1] * d_env, th[0].exp() * d_env, d_vs, Fr.SR, R)
        loss = (force.double() - target).square().sum()
        loss.backward()
        return float(loss), th.grad.cpu().numpy()

    _, losses = Fr.adam(lg, Fr.recovery_start(), Fr.RECOVERY["steps"], Fr.RECOVERY["lr"])
    ratio, ref = losses[-1] / losses[0], Fr.recovery_numpy()
    print(f"RATIO friction.recovery.device {ratio:.3g} numpy {ref:.3g}")
    assert ref / 2 <= ratio <= 2 * ref
