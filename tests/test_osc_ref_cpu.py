"""Anchors of tests/_osc_ref.py (no GPU): the fp64 references of the oscillator kernels against the oracle and against
torch fp64 autograd, and the forward bound against a CPU model of the kernels' fp32 roundings, at the shapes of
tests/test_oscillator_kernels_gpu.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _osc_ref as R  # noqa: E402
from oracle import oscillator as oosc  # noqa: E402

SR = R.SR
TV_CASES = [(s, "base") for s in R.TV_SHAPES] + [(s, v) for s in R.TV_SHAPES if s[3] in (65, 1025) for v in R.TV_VARIANTS]
BANK_CASES = [(s, True) for s in R.BANK_SHAPES] + [(R.BANK_SHAPES[i], False) for i in (0, 3, 5)]


def _id(case):
    return "-".join(map(str, case[0])) + "-" + str(case[1])


@pytest.mark.parametrize("shape", R.TV_SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_tv_forward_matches_oracle(shape):
    """tv_forward on the oracle's own damp / freq expressions (fp64 throughout) against oracle.bank_time_varying."""
    A, m, F, S = shape
    g = torch.Generator().manual_seed(S * 100 + m)
    rnd = lambda *sz: torch.rand(*sz, generator=g, dtype=torch.float64)
    f_lin = 60.0 + 13000.0 * rnd(1, m, 1)
    f_nl = 60.0 + 13000.0 * rnd(A, m, S)
    rate = 0.05
    alpha = 2.0 + 60.0 * rnd(1, m, 1)
    beta = 1e-8 + 7e-8 * rnd(1, m, 1)
    amp = 0.5 + rnd(A, m, 1)
    force = torch.randn((A, F), generator=g, dtype=torch.float64)
    ref, _ = oosc.bank_time_varying(f_lin, f_nl, rate, alpha, beta, amp, force, S, SR)
    lbd = ((f_lin + rate * f_nl) * 2 * np.pi) ** 2
    damp = 0.5 * (alpha + beta * lbd)
    freq = (lbd - damp ** 2) ** 0.5 / (2 * np.pi)
    y, E = R.tv_forward(damp.numpy(), freq.numpy(), amp.numpy().reshape(A, m), force.numpy(), SR)
    ref = ref.numpy()
    err = np.abs(y - ref).max() / np.abs(ref).max()
    print(f"tv_forward vs oracle {shape}: {err:.2e}")
    assert err <= 1e-12
    assert np.allclose(E, (amp * torch.exp(-torch.cumsum(damp / SR, 2))).sum(1).numpy(), rtol=1e-12, atol=0)


@pytest.mark.parametrize("case", TV_CASES, ids=_id)
def test_tv_backward_matches_autograd(case):
    """tv_backward(corr(gy)) against fp64 autograd of the torch chain, for dmp, frq and amp."""
    dmp, frq, amp, force, gy = R.tv_inputs(*case)
    A, m, S = dmp.shape
    leaf = lambda x: torch.from_numpy(x).double().requires_grad_(True)
    td, tf = leaf(dmp), leaf(frq)
    ta = None if amp is None else leaf(amp)
    y = R.torch_tv_chain(td, tf, ta, torch.from_numpy(force).double(), SR)
    (y * torch.from_numpy(gy).double()).sum().backward()
    gs = R.corr(gy, force)
    g_dmp, g_frq, gamp, U, V = R.tv_backward(gs, dmp, frq, amp, SR)
    pairs = [("dmp", g_dmp, td.grad), ("frq", g_frq, tf.grad)] + ([] if amp is None else [("amp", gamp, ta.grad)])
    for name, mine, auto in pairs:
        auto = auto.numpy()
        err = np.abs(mine - auto).max() / np.abs(auto).max()
        print(f"tv_backward {name} vs autograd {case}: {err:.2e}")
        assert err <= 1e-10, name
    y_ref, _ = R.tv_forward(dmp, frq, amp, force, SR)
    assert np.abs(y_ref - y.detach().numpy()).max() <= 1e-10 * np.abs(y_ref).max()
    assert (U >= np.abs(g_dmp[:, :, 0]) * SR * (1 - 1e-12)).all() and (V > 0).all()


@pytest.mark.parametrize("case", BANK_CASES, ids=_id)
def test_bank_reference_matches_oracle_and_autograd(case):
    """The closed-form reference against oracle.bank_closed_form_f64 (through the Rayleigh-damping parameters, as
    test_oscillator_kernels does) and against fp64 autograd of the closed form.

    The other sides evaluate sin(w tau) in fp64, where w tau (up to 7.4e3 rad here) is rounded three times, ~2.5e-12 rad;
    the reference forms it in extended precision.  Hence 1e-11 of the largest sample and 1e-10 of the largest gradient."""
    shape, with_amp = case
    A, m, F, S = shape
    _, _, amp, force, gy = R.bank_inputs(shape, with_amp)
    rng = np.random.default_rng(S + m)
    f = np.sort(rng.uniform(300.0, 9300.0, m))
    alpha, beta = 6.0, 1e-7
    lbd = (2 * np.pi * f) ** 2
    d = 0.5 * (alpha + beta * lbd)
    w = np.sqrt(lbd - d * d)
    y, E = R.bank_forward(d, w, amp, force, S, SR)
    ref = oosc.bank_closed_form_f64(f, force, S, SR, alpha, beta, amp=amp)
    assert np.abs(y - ref).max() <= 1e-11 * np.abs(ref).max()
    td, tw = (torch.from_numpy(x).requires_grad_(True) for x in (d, w))
    ta = None if amp is None else torch.from_numpy(amp).double().requires_grad_(True)
    yy = R.torch_bank_chain(td, tw, ta, torch.from_numpy(force).double(), S, SR)
    (yy * torch.from_numpy(gy).double()).sum().backward()
    assert np.abs(y - yy.detach().numpy()).max() <= 1e-11 * np.abs(y).max()
    gd, gw, gamp, W, V = R.bank_backward(R.corr(gy, force), d, w, amp, SR)
    pairs = [("d", gd, td.grad), ("w", gw, tw.grad)] + ([] if amp is None else [("amp", gamp, ta.grad)])
    for name, mine, auto in pairs:
        auto = auto.numpy()
        assert np.abs(mine - auto).max() <= 1e-10 * np.abs(auto).max(), name
    assert (W >= np.abs(gd)).all() and (W >= np.abs(gw)).all()


def test_fir_and_corr_are_adjoint():
    rng = np.random.default_rng(3)
    for A, F, S in [(1, 1, 1), (2, 7, 5), (2, 5, 64), (1, 150, 130)]:
        s, gy, force = rng.standard_normal((A, S)), rng.standard_normal((A, S)), rng.standard_normal((A, F))
        full = np.stack([np.convolve(s[a], force[a])[:S] for a in range(A)])
        assert np.allclose(R.fir(s, force), full, rtol=0, atol=1e-13 * np.abs(full).max())
        lhs, rhs = (R.fir(s, force) * gy).sum(), (s * R.corr(gy, force)).sum()
        assert abs(lhs - rhs) <= 1e-12 * (np.abs(R.fir(np.abs(s), np.abs(force))) * np.abs(gy)).sum()


def test_exact_prefix():
    """_prefix against exact rational arithmetic: the phase of a 15 kHz mode after 2500 samples, to one fp64 rounding of
    its fractional part."""
    from fractions import Fraction

    rng = np.random.default_rng(5)
    v = (rng.uniform(14000, 15000, 2500).astype(np.float32).astype(np.float64)) * (1.0 / SR)
    H, L = R._prefix(v[None, :])
    acc, worst = Fraction(0), 0.0
    for t in range(v.size):
        acc += Fraction(float(v[t]))
        frac = acc - (acc.numerator // acc.denominator)
        got = Fraction(float(H[0, t] - np.floor(H[0, t]))) + Fraction(float(L[0, t]))
        worst = max(worst, abs(float(got - frac)))
    assert worst <= 2.0 ** -70


@pytest.mark.parametrize("case", TV_CASES, ids=_id)
def test_tv_forward_bound_holds_for_fp32_model(case):
    """The reference rounded through the time-varying kernels' fp32 recipe (one partial per 16 modes, the partials added in
    order, sequential fma FIR) stays inside bound_y at every sample - and uses a visible part of it."""
    dmp, frq, amp, force, _ = R.tv_inputs(*case)
    m = dmp.shape[1]
    y, E = R.tv_forward(dmp, frq, amp, force, SR)
    model = R.round_like_kernel(R.tv_mode_signals(dmp, frq, amp, SR), R.tv_groups(m), force)
    bound = R.bound_y(force, E, R.tv_partials(m))
    assert (bound > 0).all()
    ratio = np.abs(model.astype(np.float64) - y) / bound
    print(f"tv fp32 model / bound {case}: {ratio.max():.3f}")
    assert ratio.max() < 1.0


@pytest.mark.parametrize("case", BANK_CASES, ids=_id)
def test_bank_forward_bound_holds_for_fp32_model(case):
    """As above for the closed-form kernel: four partials (the modes w, w + 4, ... of wave w)."""
    shape, with_amp = case
    A, m, F, S = shape
    d, w, amp, force, _ = R.bank_inputs(shape, with_amp)
    y, E = R.bank_forward(d, w, amp, force, S, SR)
    model = R.round_like_kernel(R.bank_mode_signals(d, w, amp, A, S, SR), R.bank_groups(m), force)
    bound = R.bound_y(force, E, R.BANK_PARTIALS)
    assert (bound > 0).all()
    ratio = np.abs(model.astype(np.float64) - y) / bound
    print(f"bank fp32 model / bound {case}: {ratio.max():.3f}")
    assert ratio.max() < 1.0


def test_bounds_scale_as_documented():
    """The bound functions are the formulas of their docstrings (u = 2^-24)."""
    u = 2.0 ** -24
    force, E = np.array([[2.0, -1.0]]), np.array([[1.0, 3.0, 0.5]])
    assert np.allclose(R.bound_y(force, E, 4), 2 * (2 + 4 + 1) * u * np.array([[2.0, 7.0, 4.0]]), rtol=1e-15)
    assert np.allclose(R.bound_gs(np.array([[1.0, -3.0, 0.5]]), force), 2 * 3 * u * np.array([[5.0, 6.5, 1.0]]), rtol=1e-15)
    ref, U = np.array([[[4.0, -2.0]]]), np.array([[8.0]])
    assert np.allclose(R.bound_g_dmp(ref, U, 2, SR), 2 * u * np.abs(ref) + 2 * 2.0 ** -48 * 8.0 / SR, rtol=1e-15)
    assert np.allclose(R.bound_g_frq(ref, U, 2, SR), 2 * u * np.abs(ref) + 2 * 2.0 ** -48 * 2 * np.pi * 8.0 / SR, rtol=1e-15)
    assert np.allclose(R.bound_gamp(np.array([[3.0]]), np.array([[5.0]]), 100), 6 * u + 100 * 2.0 ** -48 * 5.0, rtol=1e-15)
    assert np.allclose(R.bound_gd_gw(np.array([2.0]), 2500), (40 + 64) * 2.0 ** -46 * 2.0, rtol=1e-15)
    assert R.tv_partials(1) == 1 and R.tv_partials(16) == 1 and R.tv_partials(17) == 2 and R.tv_partials(33) == 3
