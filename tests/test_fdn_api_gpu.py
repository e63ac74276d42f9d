"""The Python layer of the feedback delay network on the device (diffsound_amd/ddsp/fdn.py): ``fdn_reverb`` and its autograd
against the fp64 recursion of tests/_fdn_ref.py at its bounds, ``FeedbackDelayNetwork`` against the same recursion fed with
its coefficients, its gradients through the parametrisation against central differences, and what the module promises."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _fdn_ref as F  # noqa: E402
import _fir_ref as FIR  # noqa: E402
from _guarded import _ratio, dev, same_on_other_device  # noqa: E402

from diffsound_amd.ddsp import fdn as V  # noqa: E402

pytestmark = pytest.mark.gpu

GRAD_OF = dict(A="gA", b="gb", c="gc", d="gd", p="gp")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("flat", [False, True], ids=["sets", "flat"])
def test_reverb_values_and_gradients(flat, dtype):
    """(B, N) with (H, ...) parameters, and (N,) with parameters without the leading H; fp32 and fp64 x: y and every gradient at
    the kernel's bounds."""
    case = (1, 1, 317, F.D3, "damp") if flat else (4, 2, 317, F.D3, "damp")
    i, f, b = F.reference(case)
    cut = (lambda a: a[0]) if flat else (lambda a: a)
    tx = torch.from_numpy(cut(i["x"])).to(dev(), dtype).requires_grad_(True)
    par = {k: torch.from_numpy(np.asarray(cut(i[k]))).to(dev()).requires_grad_(True) for k in GRAD_OF}
    y = V.fdn_reverb(tx, cut(i["delays"]), par["A"], par["b"], par["c"], par["d"], par["p"])
    assert y.shape == tx.shape and y.dtype == dtype
    y.backward(torch.from_numpy(cut(i["gy"])).to(dev(), dtype))
    B = case[0]
    assert _ratio("fdn.api.y", (F.case_id(case),), y.detach().cpu().numpy().reshape(B, -1), f["y"], f["y_bound"]) <= 1.0
    assert _ratio("fdn.api.gx", (F.case_id(case),), tx.grad.cpu().numpy().reshape(B, -1), b["gx"], b["gx_bound"]) <= 1.0
    for k, g in GRAD_OF.items():
        assert par[k].grad.shape == par[k].shape and par[k].grad.dtype == torch.float64
        assert _ratio("fdn.api." + g, (F.case_id(case),), par[k].grad.cpu().numpy().reshape(b[g].shape), b[g], b[g + "_bound"]) <= 1.0


def test_no_damping_and_plain_lists():
    case = (4, 2, 317, F.D3, "null")
    i, f, _ = F.reference(case)
    x = torch.from_numpy(i["x"]).to(dev())
    y = V.fdn_reverb(x, i["delays"].tolist(), i["A"], i["b"], i["c"], i["d"])
    assert _ratio("fdn.api.null.y", None, y.cpu().numpy(), f["y"], f["y_bound"]) <= 1.0


def test_a_gradient_nobody_needs_is_not_computed(monkeypatch):
    from diffsound_amd import _hip

    lib, seen = _hip.lib(), []

    class Spy:
        def __getattr__(self, name):
            fn = getattr(lib, name)
            if name != "ds_fdn_bwd":
                return fn
            return lambda *a: (seen.append(a[15:21]), fn(*a))[1]

    monkeypatch.setattr(_hip, "lib", lambda: Spy())
    i = F.inputs((1, 1, 317, F.D3, "damp"))
    x = torch.from_numpy(i["x"]).to(dev())
    t = lambda k: torch.from_numpy(i[k]).to(dev())
    V.fdn_reverb(x.clone().requires_grad_(True), i["delays"], t("A"), t("b"), t("c"), t("d"), t("p")).sum().backward()
    V.fdn_reverb(x, i["delays"], t("A"), t("b"), t("c").requires_grad_(True), t("d"), t("p").requires_grad_(True)).sum().backward()
    first, second = ([bool(v) for v in s] for s in seen)
    assert first == [True, False, False, False, False, False] and second == [False, False, False, True, False, True]


def test_value_errors_come_before_any_native_call(monkeypatch):
    """With the library handle taken away every native call would raise; the ValueErrors still come."""
    from diffsound_amd import _hip

    def no_lib():
        raise AssertionError("native call")

    monkeypatch.setattr(_hip, "lib", no_lib)
    x = torch.zeros(6, 400, device=dev())
    m, A, b, c, d = [[64, 70], [65, 71], [66, 72]], torch.zeros(3, 2, 2), torch.zeros(3, 2), torch.zeros(3, 2), torch.zeros(3)
    for args, text in [((x.reshape(3, 2, 400), m, A, b, c, d), "x must be"), ((x.long(), m, A, b, c, d), "x must be"),
                       ((x[:, :0], m, A, b, c, d), "empty signal"), ((x, [[[64]]], A, b, c, d), "delays must be"),
                       ((x, [[64.5, 70.0]], A, b, c, d), "delays must be"), ((x, m, A[0, 0], b, c, d), "A has shape"),
                       ((x, m, A[:2], b, c, d), "A has shape"), ((x, m, A, b[:, :1], c, d), "b has shape"),
                       ((x, m, A, b, c.reshape(2, 3), d), "c has shape"), ((x, m, A, b, c, d[:2]), "d has shape"),
                       ((x, m, A, b, c, d, torch.zeros(3, 3)), "damp has shape"), ((x[:4], m, A, b, c, d), "not a multiple"),
                       ((x[:2], m, A, b, c, d), "not a multiple"), ((x, [[63, 70]], A[0], b[0], c[0], 1.0), "a delay of 63 samples"),
                       ((x, [list(range(64, 81))], torch.zeros(17, 17), torch.zeros(17), torch.zeros(17), 1.0), "17 delay lines"),
                       ((torch.zeros(65536, 1).expand(65536, 4), m[0], A[0], b[0], c[0], 1.0), "65536 rows")]:
        with pytest.raises(ValueError, match=text):
            V.fdn_reverb(*args)
    with pytest.raises(AssertionError, match="native call"):
        V.fdn_reverb(x, m, A, b, c, d)
    for kw, text in [(dict(n_lines=17), "at most 16 lines"), (dict(n_responses=0), "at least 1"), (dict(init="ones"), "neither"),
                     (dict(init="wet"), "needs wet_db"), (dict(rt60=0.0), "positive"), (dict(rt60=[0.3, 0.2, 0.1]), "positive"),
                     (dict(damp=0.5), "outside"), (dict(delays=[64, 70]), "delays of shape"), (dict(sample_rate=1000), "at least 64"),
                     (dict(delays=[64, 70, 63, 90]), "a delay of 63 samples")]:
        with pytest.raises(ValueError, match=text):
            V.FeedbackDelayNetwork(**dict(dict(n_responses=2, n_lines=4, sample_rate=32000, rt60=0.3), **kw))
    net = V.FeedbackDelayNetwork(2, 4, 32000, 0.3).to(dev())
    with pytest.raises(ValueError, match="not a multiple"):
        net(x[:3])


def test_cpu_tensors_are_refused():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        V.fdn_reverb(torch.zeros(2, 400), [64, 70], torch.zeros(2, 2), torch.zeros(2), torch.zeros(2), 1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        V.FeedbackDelayNetwork(1, 2, 32000, 0.3)(torch.zeros(2, 400))


def _net(init="wet", seed=3):
    """Two rooms of three lines at 8 kHz with short delays (N / min m stays at 6), S off zero, everything else off its start."""
    net = V.FeedbackDelayNetwork(2, 3, 8000.0, [0.05, 0.08], delays=[[64, 81, 97], [67, 90, 101]], damp=0.2, wet_db=-6.0, init=init)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        net.S.copy_(0.4 * torch.randn(net.S.shape, dtype=torch.float64, generator=g))
        net.b.mul_(1.0 + 0.3 * torch.randn(net.b.shape, dtype=torch.float64, generator=g))
        net.damp_logit.add_(torch.randn(net.damp_logit.shape, dtype=torch.float64, generator=g))
    return net


def _restated(net, x):
    """The fp64 reference fed with the coefficients the module's parametrisation gives, on the device the module is on."""
    A, b, c, d, p = (t.detach().cpu().numpy() for t in net.coefficients())
    return F.forward(x, net.delays.cpu().numpy(), A, b, c, d, p)


N_API = 384   # six times the smallest delay


def _audio(seed, shape=(4, N_API)):
    return F.spread(np.random.default_rng(seed), shape, -2, 0).astype(np.float32)


def test_module_against_the_reference():
    net, x = _net().to(dev()), _audio(1, (3, 2, N_API))
    f = _restated(net, x.reshape(6, N_API))   # (the coefficients the device formed: the kernel's own inputs)
    y = net(torch.from_numpy(x).to(dev()))
    assert y.shape == x.shape and y.dtype == torch.float32
    assert _ratio("fdn.module.y", None, y.detach().cpu().numpy().reshape(6, -1), f["y"], f["y_bound"]) <= 1.0


def test_module_gradients_against_central_differences():
    """L = sum (y - target)^2 through rt60, S, the damping, b and c.  The device rounds y to fp32 and takes gy in fp32: every
    sample's share of a gradient is off by up to 3 U32 = 1.8e-7 of its magnitude, and the magnitudes add up to more than the
    gradient itself by the cancellation in a sum of N = 384 noise-like terms, some sqrt(N) to N / 4: up to 2e-5 of the tensor's
    largest gradient.  Asked: 1e-4 of it, and 1e-7 for the central difference (h = 1e-5, third derivatives of order one)."""
    x, target = _audio(2), _audio(3)
    host = _net()
    net = _net().to(dev())
    loss = ((net(torch.from_numpy(x).to(dev())).double() - torch.from_numpy(target).to(dev()).double()) ** 2).sum()
    loss.backward()
    names = ("log_rt60", "S", "damp_logit", "b", "c")
    assert {n for n, _ in net.named_parameters()} == set(names)
    value = lambda: float(((_restated(host, x)["y"] - target.astype(np.float64)) ** 2).sum())
    h = 1e-5
    for name in names:
        got, par = getattr(net, name).grad.cpu().numpy(), getattr(host, name)
        fd = np.zeros_like(got)
        for idx in np.ndindex(got.shape):
            with torch.no_grad():
                keep = float(par[idx])
                par[idx] = keep + h
                up = value()
                par[idx] = keep - h
                down = value()
                par[idx] = keep
            fd[idx] = (up - down) / (2 * h)
        worst = float(np.abs(got - fd).max() / np.abs(fd).max())
        print(f"FD {name} {worst:.3g}")
        assert np.abs(fd).max() > 0 and worst <= 1e-4 + 1e-7, name


def test_mixing_stays_orthogonal_under_adam():
    net = _net().to(dev())
    x, target = torch.from_numpy(_audio(4)).to(dev()), torch.from_numpy(_audio(5)).to(dev())
    opt = torch.optim.Adam(net.parameters(), lr=0.05)
    for _ in range(4):
        opt.zero_grad()
        ((net(x) - target).double() ** 2).sum().backward()
        opt.step()
    U = net.mixing().detach()
    assert float((U @ U.transpose(1, 2) - torch.eye(3, dtype=torch.float64, device=U.device)).abs().max()) <= 1e-14
    A = net.coefficients()[0].detach()
    assert float(torch.linalg.matrix_norm(A, 2).max()) < 1.0   # U diag(g), g < 1: a contraction, whatever Adam did


def test_zero_init_returns_its_input_bit_for_bit():
    net = V.FeedbackDelayNetwork(2, 8, 32000, 0.3).to(dev())
    assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == dict(delays=(2, 8), U0=(8, 8), log_rt60=(2,), S=(2, 8, 8),
                                                                            damp_logit=(2, 8), b=(2, 8), c=(2, 8))
    assert net.delays[0].tolist() == V.default_delays(8, 32000) == [641, 809, 1013, 1277, 1607, 2017, 2543, 3203]
    x = torch.from_numpy(F.spread(np.random.default_rng(7), (3, 2, 4000), -3, 1).astype(np.float32)).to(dev())
    y = net(x)
    assert y.shape == x.shape and torch.equal(y.view(torch.int32), x.view(torch.int32))
    loss = (net(x).double() ** 2).sum()
    loss.backward()
    assert bool(net.c.grad.abs().sum() > 0)   # training can leave the identity


def test_impulse_response_feeds_a_room_response():
    """``forward`` against ``fir_convolve`` with the network's own impulse response over the whole row.  The exact response
    convolved with x IS the exact y, so the two differ by the FDN's bound on y, the FIR's bound on its sum, and the taps'
    own error - the FDN's bound on the impulse run, fp32 store included - convolved with |x|."""
    from diffsound_amd.ddsp.reverb import RoomResponse, fir_convolve

    net = _net().to(dev())
    x = _audio(6)
    ir = net.impulse_response(N_API)
    assert ir.shape == (2, N_API) and ir.dtype == torch.float64 and ir.requires_grad
    assert torch.equal(ir[:, 0].detach().cpu(), torch.ones(2, dtype=torch.float64))
    tx = torch.from_numpy(x).to(dev())
    y, z = net(tx).detach().cpu().numpy(), fir_convolve(tx, ir.detach()).cpu().numpy()
    f, g = _restated(net, x), FIR.forward(x, ir.detach().cpu().numpy())
    impulse = np.zeros((2, N_API))
    impulse[:, 0] = 1.0
    taps = FIR.forward(np.abs(x), _restated(net, impulse)["y_bound"])["y"]
    assert _ratio("fdn.ir.fir", None, z, y.astype(np.float64), f["y_bound"] + g["bound"] + taps) <= 1.0
    room = RoomResponse(2, N_API, 8000.0)
    with torch.no_grad():
        room.ir.copy_(ir[:, 1:].detach())
    assert torch.equal(room.impulse_response(), ir.detach().cpu())


def test_runs_on_its_operands_device():
    i = F.inputs((2, 1, 102, F.D3, "damp"))

    def run(device):
        t = lambda k: torch.from_numpy(i[k]).to(device)
        x, A, c = t("x").requires_grad_(True), t("A").requires_grad_(True), t("c").requires_grad_(True)
        y = V.fdn_reverb(x, i["delays"], A, t("b"), c, t("d"), t("p"))
        return (y.detach(),) + torch.autograd.grad((y * t("gy")).sum(), [x, A, c])

    same_on_other_device(run)
