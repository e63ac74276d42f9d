"""``nonlinear_bank``, ``TensionModulatedBank`` and ``modal_stretch`` (diffsound_amd/ddsp/nonlinear.py) end to end on the
device: the refusals, the dtypes, the gradient groups, the linear limit against the driven bank, the chain from a hammer to a
filtered sound, the recovery of a coupling from the sound, and the stretch coefficients of a mesh's modes."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _nlbank_ref as Nl  # noqa: E402
import _osc_driven_ref as Od  # noqa: E402
from _guarded import _ratio, dev  # noqa: E402

pytestmark = pytest.mark.gpu

LD = np.longdouble
NAMES = ("d", "w", "gain", "amp", "force", "stretch", "coupling")


def t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev())


def _good(case):
    ops = Nl.inputs(case)
    return dict(zip(NAMES, (t(x) for x in ops[:7])), sample_num=case[5], sr=Nl.SR, oversample=case[3])


def test_refusals_come_before_device_work():
    from diffsound_amd.ddsp import TensionModulatedBank, nonlinear_bank

    good = _good(Nl.CASES[5])
    g = lambda k: good[k]  # noqa: E731
    nan, inf = float("nan"), float("inf")
    bad = [(dict(w=-g("w")), "w must be positive"), (dict(w=g("w") * 0), "w must be positive"),
           (dict(stretch=g("stretch") - 2.0), "stretch must not be negative"),
           (dict(coupling=g("coupling") - 1.0), "coupling must not be negative"),
           (dict(force=g("force") * nan), "force is not finite"), (dict(d=g("d") * inf), "d is not finite"),
           (dict(amp=g("amp") * nan), "amp is not finite"), (dict(coupling=g("coupling") + inf), "coupling is not finite"),
           (dict(gain=g("gain")[:, :3]), "gain must be"), (dict(amp=g("amp")[:2]), "amp must be"),
           (dict(force=g("force")[:2]), "force must be"), (dict(stretch=g("stretch")[:, :3]), "stretch must be"),
           (dict(coupling=g("coupling")[:, :1]), "coupling must be"), (dict(w=g("w")[:2]), "d and w must be"),
           (dict(oversample=65), "oversample"), (dict(oversample=0), "oversample"), (dict(sr=-1.0), "sr"),
           (dict(sample_num=0), "sample_num"), (dict(sample_num=(1 << 24) // 4 + 1), "substeps"),
           (dict(stretch=g("stretch").repeat(3, 1), coupling=g("coupling").repeat(1, 3)), "K = 6 outside 1..4")]
    for change, text in bad:
        with pytest.raises(ValueError, match=text):
            nonlinear_bank(**dict(good, **change))
    for name in ("d", "gain", "force", "stretch", "coupling"):
        with pytest.raises(RuntimeError, match="HIP device"):
            nonlinear_bank(**dict(good, **{name: good[name].cpu()}))
    assert float(nonlinear_bank(**good).abs().max()) > 0
    bank = TensionModulatedBank(3, g("stretch"), coupling=1e9, oversample=4).to(dev())
    args = [g(k) for k in ("d", "w", "gain", "amp", "force")]
    with pytest.raises(ValueError, match="w must be positive"):
        bank(args[0], -args[1], *args[2:], 70, Nl.SR)
    with pytest.raises(ValueError, match="coupling must be"):
        TensionModulatedBank(2, g("stretch"), coupling=1e9).to(dev())(*args, 70, Nl.SR)
    with pytest.raises(RuntimeError, match="HIP device"):
        bank(args[0].cpu(), *args[1:], 70, Nl.SR)
    y = bank(*args, 70, Nl.SR)
    assert y.shape == (3, 70) and y.dtype == torch.float32 and y.requires_grad


def test_gradients_only_where_needed_and_in_the_inputs_dtypes():
    from diffsound_amd.ddsp import TensionModulatedBank, nonlinear_bank

    case = Nl.CASES[1]
    ops = Nl.inputs(case)
    S, R = case[5], case[3]
    # each tensor alone requires grad: it gets a gradient, with the bits it has when all seven are asked for
    full = [t(x).requires_grad_(True) for x in ops[:7]]
    nonlinear_bank(*full, S, Nl.SR, R).square().sum().backward()
    assert all(o.grad is not None and o.grad.dtype == torch.float64 and o.grad.shape == o.shape for o in full)
    for j, name in enumerate(NAMES):
        one = [t(x).requires_grad_(i == j) for i, x in enumerate(ops[:7])]
        y = nonlinear_bank(*one, S, Nl.SR, R)
        y.square().sum().backward()
        for i, o in enumerate(one):
            assert (o.grad is not None) == (i == j), (name, NAMES[i])
        assert torch.equal(one[j].grad, full[j].grad), name
    assert not nonlinear_bank(*[t(x) for x in ops[:7]], S, Nl.SR, R).requires_grad
    # fp32 and mixed inputs: fp64 inside, the inputs' dtypes back
    for dts in ([torch.float32] * 7, [torch.float64, torch.float32, torch.float16, torch.float32, torch.float32, torch.bfloat16,
                                      torch.float64]):
        mixed = [t(x).to(dt).requires_grad_(True) for x, dt in zip(ops[:7], dts)]
        y = nonlinear_bank(*mixed, S, Nl.SR, R)
        assert y.dtype == torch.float32
        y.square().sum().backward()
        assert all(o.grad is not None and o.grad.dtype == dt and o.grad.shape == o.shape for o, dt in zip(mixed, dts))
    frozen = TensionModulatedBank(1, t(ops[5]), coupling=t(ops[6]), oversample=R, train_coupling=False).to(dev())
    assert not frozen(*[t(x) for x in ops[:5]], S, Nl.SR).requires_grad
    live = TensionModulatedBank(1, t(ops[5]), coupling=t(ops[6]), oversample=R).to(dev())
    live(*[t(x) for x in ops[:5]], S, Nl.SR).square().sum().backward()
    # d L / d log gamma = gamma d L / d gamma
    want = full[6].grad * live.log_coupling.detach().exp()
    assert torch.allclose(live.log_coupling.grad, want, rtol=1e-9, atol=0)  # (exp(log gamma) is gamma to a few ulps only)


def test_without_coupling_it_is_the_driven_bank():
    """gamma = 0, R = 1: ``nonlinear_bank`` and ``oscillator_bank_driven(d, w, amp * gain, force, S, sr)`` each within their
    own reference's bound of one float64 truth, the closed-form convolution of tests/_osc_driven_ref.py.  The driven bank
    takes its force and amplitudes in fp32, so both get fp32-representable ones (amp = 1, gain and force rounded).  The
    nonlinear bank's own truth, the longdouble recursion, sits within the driven reference's fp64 term k64 Emag of the closed
    form."""
    from diffsound_amd.ddsp import nonlinear_bank
    from diffsound_amd.ddsp.bank import oscillator_bank_driven

    case = Nl.CASES[5]
    A, m, K, R, F, S = case[:6]
    d, w, c, amp, f, C, gamma, _ = Nl.inputs(case)
    c, f = c.astype(np.float32).astype(np.float64), f.astype(np.float32).astype(np.float64)
    amp, gamma = np.ones_like(amp), np.zeros_like(gamma)
    truth, Emag = Od.forward(d, w, amp * c, f, S, Nl.SR)
    r64, rld = (Nl.forward(d, w, c, amp, f, C, gamma, S, 1, dtype=dt)["y"] for dt in (np.float64, LD))
    assert (np.abs(np.asarray(rld, dtype=np.float64) - truth) <= Od.k64(A, m, S) * Emag).all()
    y = nonlinear_bank(t(d), t(w), t(c), t(amp), t(f), t(C), t(gamma), S, Nl.SR, 1).cpu().numpy()
    assert Nl.e64(r64, rld)[0] <= Nl.E64_MAX
    assert _ratio("nlbank.linear.y", None, y, np.asarray(rld, dtype=np.float64), Nl.bound(r64, rld, stored32=True)) <= 1.0
    yd = oscillator_bank_driven(t(d), t(w), t(amp * c).float(), t(f).float(), S, Nl.SR).cpu().numpy()
    assert _ratio("nlbank.linear.driven", None, yd, truth, Od.bound_y(truth, Emag, A, m, S)) <= 1.0


def test_hammer_to_nonlinear_bank_to_filter_backpropagates():
    from diffsound_amd.ddsp import HertzHammer, TensionModulatedBank, biquad_cascade
    from diffsound_amd.ddsp.biquad import lowpass_coeffs

    case = Nl.CASES[5]
    A, m, K, R, F, S = case[:6]
    d, w, c, amp, f, C, gamma, _ = Nl.inputs(case)
    hammer = HertzHammer(A, 0.01, 1.0, 1e7).to(dev())
    # the table's couplings are scaled to a strike of 1 N; a 10 g hammer at 1 m/s presses with tens of newtons: 1e-4 of them
    bank = TensionModulatedBank(A, t(C), coupling=t(1e-4 * np.where(gamma > 0, gamma, gamma[:1])), oversample=R).to(dev())
    leaves = [t(x).requires_grad_(True) for x in (d, w, c, amp)]
    force = hammer(leaves[0], leaves[1], leaves[2], F, Nl.SR)
    y = bank(*leaves, force, S, Nl.SR)
    sos = torch.as_tensor(lowpass_coeffs(Nl.SR, 4000.0), dtype=torch.float64).reshape(1, 5).to(dev()).requires_grad_(True)
    out = biquad_cascade(y, sos)
    assert out.shape == (A, S) and out.dtype == torch.float32
    out.square().sum().backward()
    torch.cuda.synchronize()
    params = dict(hammer.named_parameters())
    assert len(params) >= 3
    for name, p in list(params.items()) + [("log_coupling", bank.log_coupling), ("sos", sos)] + list(zip("dwca", leaves)):
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, name


def test_recovery_of_the_coupling_from_the_sound():
    """The target sound comes from gamma; from 2 gamma, 80 Adam steps on log gamma with the squared error of y as the loss -
    the steps tests/test_nlbank_ref_cpu.py runs on the restatement, here through ``TensionModulatedBank`` and autograd.

    Followed to the bound: at every point theta the device run visits, its loss is compared with the float64 restatement's
    loss AT THAT theta.  An element of y deviates from the truth by at most its bound b (8 max(E64, 2^-52) scale + 2^-24 |y|,
    E64 and the scale taken from the target, of which every iterate is a neighbour), so a residual r = y - target moves by
    e <= b(y) + b(target) per sample, and the loss sum r^2 by at most 2 sum |r| e + sum e^2; the fp64 sum of S squares adds
    S 2^-52 of the loss.  Nothing here is taken from the device's result.
    The expected trajectory: the final loss is below the first by the factor the restatement's own Adam run shows, within
    the factor 2 that tests/test_friction_api_gpu.py allows for the two runs' thetas drifting apart."""
    from diffsound_amd.ddsp import TensionModulatedBank

    d, w, c, amp, f, C, gamma = Nl.recovery_problem()
    S, R = Nl.RECOVERY["S"], Nl.RECOVERY["R"]
    ops = [t(x) for x in (d, w, c, amp, f)]
    target = TensionModulatedBank(1, t(C), coupling=t(gamma), oversample=R, train_coupling=False).to(dev())(*ops, S, Nl.SR).double()
    bank = TensionModulatedBank(1, t(C), coupling=t(gamma) * Nl.RECOVERY["off"], oversample=R).to(dev())
    assert np.allclose(bank.log_coupling.detach().cpu().numpy(), Nl.recovery_start(), rtol=1e-15, atol=0)
    visited = []

    def lg(theta):
        visited.append(np.array(theta))
        with torch.no_grad():
            bank.log_coupling.copy_(t(theta).reshape(1, -1))
        bank.log_coupling.grad = None
        loss = (bank(*ops, S, Nl.SR).double() - target).square().sum()
        loss.backward()
        return float(loss), bank.log_coupling.grad.cpu().numpy().reshape(-1)

    _, losses = Nl.adam(lg, Nl.recovery_start().reshape(-1), Nl.RECOVERY["steps"], Nl.RECOVERY["lr"])
    assert len(visited) == len(losses) == Nl.RECOVERY["steps"] + 1
    t64, tld = (Nl.forward(d, w, c, amp, f, C, gamma, S, R, dtype=dt)["y"] for dt in (np.float64, LD))
    E, scale = Nl.e64(t64, tld)
    assert E <= Nl.E64_MAX
    fp64_term = 8.0 * max(E, Nl.EPS64) * scale
    worst = 0.0
    for theta, loss in zip(visited, losses):
        y = Nl.forward(d, w, c, amp, f, C, np.exp(theta).reshape(1, -1), S, R)["y"]
        r = np.abs(y - t64)
        e = 2 * fp64_term + Nl.U32 * (np.abs(y) + np.abs(t64))
        want = float((r * r).sum())
        tol = float(2 * (r * e).sum() + (e * e).sum()) + S * Nl.EPS64 * want
        worst = max(worst, abs(loss - want) / tol)
        assert abs(loss - want) <= tol, (theta, loss, want, tol)
    ref = Nl.recovery_numpy()
    print(f"RATIO nlbank.recovery.device {losses[-1] / losses[0]:.3g} numpy {ref[-1] / ref[0]:.3g} loss/bound {worst:.3g}")
    assert ref[-1] / ref[0] < 1e-2
    assert ref[-1] / ref[0] / 2 <= losses[-1] / losses[0] <= 2 * ref[-1] / ref[0]


def _two_tets(order):
    from diffsound_amd.diffelastic.deform import Deform
    from diffsound_amd.diffelastic.mesh import TetMesh

    v = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.1, 0.0], [0.2, 0.9, 0.1], [0.1, 0.2, 1.1], [0.9, 1.0, 0.8]], dtype=torch.float32)
    tets = torch.tensor([[0, 1, 2, 3], [4, 2, 1, 3]], dtype=torch.int64)
    mesh = TetMesh(v.to(dev()), tets.to(dev())).to_high_order(order)
    return mesh, Deform(mesh)


@pytest.mark.parametrize("order", [1, 2])
def test_modal_stretch_is_the_weighted_sum_of_squared_gradients(order):
    """Against the same sum formed in fp64 torch from ``Deform.shape_func_deriv`` and ``integration_weights`` directly:
    grad phi = sum_a u_a (x) B_a per Gauss point.  Agreement: 2^-22 relative - the Deform kernels write the gradient in fp32
    (2^-24 per entry, squared: 2^-23), the sum of a few hundred positive terms is formed in fp64 on both sides."""
    from diffsound_amd.ddsp import modal_stretch

    mesh, deform = _two_tets(order)
    nv = mesh.vertices.shape[0]
    U = torch.from_numpy(np.random.default_rng(order).standard_normal((3 * nv, 3))).to(dev())
    got = modal_stretch(deform, U)
    assert got.shape == (3,) and got.dtype == torch.float64 and got.device == U.device
    B = deform.shape_func_deriv.double()                                                    # (T G, N, 3)
    wts = deform.integration_weights.double().reshape(-1)                                   # (T G,)
    G = deform.num_guass_points
    nodes = mesh.tets.repeat_interleave(G, dim=0)                                           # (T G, N)
    u = U.double().t().reshape(3, nv, 3)[:, nodes]                                          # (3, T G, N, 3)
    grad = torch.einsum("mgai,gaj->mgij", u, B)
    want = (grad.square().sum((-1, -2)) * wts).sum(-1)
    assert float(want.min()) > 0
    rel = float(((got - want).abs() / want).max())
    print(f"RATIO nlbank.modal_stretch order{order} {rel / 2.0 ** -22:.3g}")
    assert rel <= 2.0 ** -22
    # in chunks of one mode: the same bits
    assert torch.equal(modal_stretch(deform, U, chunk_bytes=1), got)
    # a rigid translation stretches nothing: C = 0 to that level, against the scale of a unit-gradient field (the volume)
    shift = torch.tensor([0.3, -1.2, 0.7], dtype=torch.float64, device=dev()).repeat(nv)[:, None]
    zero = modal_stretch(deform, shift)
    assert float(zero.abs().max()) <= 2.0 ** -22 * float(wts.sum()) * 3
    with pytest.raises(ValueError, match="U must be"):
        modal_stretch(deform, U[:-1])
