"""The references of tests/_osc_listen_ref.py anchored without a GPU: the adjoint against central differences of the forward
for every input (both parts of h included), unit gains against the driven bank's reference, h = i against the cosine
quadrature, one impulse in closed form, exact zeros for frames no sample touches, and the complex128 recurrences - the
kernels' formulas restated - against the convolutions within the derived bounds."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _osc_driven_ref as D  # noqa: E402
import _osc_listen_ref as LS  # noqa: E402
import _osc_ref as R  # noqa: E402

SMALL = [(2, 3, 4, 40, 37, 3, 16, "material", True), (1, 2, 3, 9, 50, 5, 16, "d0", False),
         (2, 1, 2, 70, 65, 2, 48, "nyquist", True)]


def _loss(gy, *a):
    return (gy * LS.forward(*a)[0]).sum()


@pytest.mark.parametrize("case", SMALL, ids=LS.case_id)
def test_adjoint_matches_central_differences(case):
    """loss = sum gy y is linear in force, amp and both parts of h: its central difference is exact up to rounding.  In d
    and w it is smooth: steps of 1e-3 relative to the scale 1 / tau_max leave a truncation error below 1e-6 of W."""
    A, C, m, F, S, K, hop = case[:7]
    d, w, amp, force, h, gy = LS.inputs(case)
    d, w, force, h, gy = (np.asarray(x, dtype=np.float64) for x in (d, w, force, h, gy))
    amp = np.ones((A, m)) if amp is None else amp.astype(np.float64)
    b = LS.backward(gy, d, w, amp, force, h, hop)
    rng = np.random.default_rng(5)
    lossmag = (np.abs(gy) * LS.forward(d, w, amp, force, h, hop, S)[1]).sum()

    def cd(name, x, idx, e):
        args = dict(d=d, w=w, amp=amp, force=force, h=h)
        xp, xm = x.copy(), x.copy()
        xp[idx] += e
        xm[idx] -= e
        f = lambda v: _loss(gy, *(dict(args, **{name: v})[k] for k in ("d", "w", "amp", "force")), args["h"] if name != "h" else v,
                            hop, S)
        return (f(xp) - f(xm)) / (2 * e)

    for name, x, g, mag in (("force", force, b["gforce"], b["Eg"]), ("amp", amp, b["gamp"], b["V"]), ("h", h, b["gh"], b["Vh"])):
        for _ in range(6):
            idx = tuple(rng.integers(0, n) for n in x.shape)
            assert abs(cd(name, x, idx, 0.5) - g[idx]) <= 1e-12 * lossmag, (name, idx)
    for name, x, g in (("d", d, b["gd"]), ("w", w, b["gw"])):
        for i in range(m):
            e = 1e-3 * LS.SR / S
            assert abs(cd(name, x, (i,), e) - g[i]) <= 1e-5 * b["W"][i] + 1e-12 * lossmag, (name, i)


def test_unit_gains_are_the_driven_reference():
    case = (3, 1, 5, 70, 65, 1, 16, "material", True)
    d, w, amp, force, _, gy = LS.inputs(case)
    one = np.zeros((3, 1, 5, 1, 2), dtype=np.float32)
    one[..., 0] = 1.0
    y, Y = LS.forward(d, w, amp, force, one, 16, 65)
    yd, E = D.forward(d, w, amp, force, 65)
    assert np.all(np.abs(y[:, 0] - yd) <= D.k64(3, 5, 65) * E)
    assert np.allclose(Y[:, 0], E, rtol=1e-12, atol=0)
    b, bd = LS.backward(gy, d, w, amp, force, one, 16), D.backward(gy[:, 0], d, w, amp, force)
    for k, mag in (("gforce", "Eg"), ("gamp", "V")):
        assert np.all(np.abs(b[k] - bd[k]) <= D.k64(3, 5, 65) * bd[mag]), k
    for k in ("gd", "gw"):
        assert np.all(np.abs(b[k] - bd[k]) <= D.bound_gd_gw(bd["W"], 3, 5, 65)), k


def test_gain_i_is_the_cosine_quadrature_and_an_impulse_rings_in_closed_form():
    m, S = 4, 90
    rng = np.random.default_rng(3)
    d, w = rng.uniform(1.0, 400.0, m), R.TWO_PI * rng.uniform(50.0, 15000.0, m)
    force = np.zeros((1, 5), dtype=np.float32)
    force[0, 0] = 1.0
    tau, env, sn, cs = R.bank_modes(d, w, S, LS.SR)
    hi = np.zeros((1, 1, m, 1, 2), dtype=np.float32)
    hi[..., 1] = 1.0
    y, _ = LS.forward(d, w, None, force, hi, 16, S)
    assert np.allclose(y[0, 0], (env * cs).sum(0), rtol=0, atol=1e-13)
    h = rng.standard_normal((1, 2, m, 1, 2)).astype(np.float32)
    y, _ = LS.forward(d, w, None, force, h, 16, S)
    Hc = h[0, :, :, 0, 0].astype(np.float64) + 1j * h[0, :, :, 0, 1]
    ph = (w[:, None] * tau[None])
    want = (np.abs(Hc)[:, :, None] * env[None] * np.sin(ph[None] + np.angle(Hc)[:, :, None])).sum(1)
    assert np.allclose(y[0], want, rtol=0, atol=1e-9)  # (fp64 phase w tau against the reference's extended one)


def test_frames_no_sample_touches_get_exact_zeros():
    case = (2, 3, 2, 9, 33, 6, 16, "material", True)     # samples 0..32: frames 0, 1, 2 and (th of 32 = 0) nothing on 3
    d, w, amp, force, h, gy = LS.inputs(case)
    assert LS.frames_needed(33, 16) == 3 and LS.frames_needed(34, 16) == 4 and LS.frames_needed(1, 16) == 1
    b = LS.backward(gy, d, w, amp, force, h, 16)
    assert not b["gh"][:, :, :, 3:].any() and b["gh"][:, :, :, 2].all()
    assert not LS.adjoint_recurrence(gy, d, w, amp, force, h, 16)["gh"][:, :, :, 3:].any()
    assert not b["gforce"][:, 33:].any()


@pytest.mark.parametrize("case", [c for c in LS.CASES if c[2] * c[4] <= 5200], ids=LS.case_id)
def test_recurrence_agrees_with_the_convolution_within_the_bounds(case):
    A, C, m, F, S, K, hop = case[:7]
    d, w, amp, force, h, gy = LS.inputs(case)
    y, Y = LS.forward(d, w, amp, force, h, hop, S)
    assert np.all(np.abs(LS.recurrence(d, w, amp, force, h, hop, S) - y) <= LS.k64(A, C, m, S) * Y)
    assert np.all(np.abs(LS.recurrence(d, w, amp, force, h, hop, S, store32=True) - y) <= LS.bound32(y, Y, A, C, m, S))
    b, r = LS.backward(gy, d, w, amp, force, h, hop), LS.adjoint_recurrence(gy, d, w, amp, force, h, hop)
    for k, mag in (("gforce", "Eg"), ("gh", "Vh"), ("gamp", "V")):
        assert np.all(np.abs(r[k] - b[k]) <= LS.k64(A, C, m, S) * b[mag]), k
    for k in ("gd", "gw"):
        assert np.all(np.abs(r[k] - b[k]) <= LS.bound_gd_gw(b["W"], A, C, m, S)), k
    assert not b["gh"][:, :, :, LS.frames_needed(S, hop):].any()


def test_torch_chain_is_the_reference():
    import torch

    case = SMALL[0]
    A, C, m, F, S, K, hop = case[:7]
    d, w, amp, force, h, gy = LS.inputs(case)
    hc = torch.from_numpy(h[..., 0].astype(np.float64) + 1j * h[..., 1])
    y = LS.torch_chain(torch.from_numpy(d), torch.from_numpy(w), torch.from_numpy(amp).double(), torch.from_numpy(force).double(),
                       hc, hop, S)
    ref, Y = LS.forward(d, w, amp, force, h, hop, S)
    assert np.all(np.abs(y.numpy() - ref) <= 1e-9 * Y)
