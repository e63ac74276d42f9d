"""tests/_multipole_ref.py vouched for without a GPU: the truth against scipy and closed forms, its gradients against central
differences, the fp64 restatement of the kernels inside the bound over the grid of the GPU test (and outside it with an fp32
Hankel recurrence), and the fit's test case with scipy's basis."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _multipole_ref as R  # noqa: E402

LD = np.longdouble


def _truth_basis(pts, k, L):
    """(P, N, m) complex128: h_l Y of the truth (mpmath's h_l, longdouble harmonics), about the origin."""
    u, r, _ = R.geometry(pts, np.zeros(3), LD)
    Y, _ = R.harmonics(u, L, LD)
    hr, hi = R.hankel_truth(k, r, L)
    deg = R.degrees(L)
    return (Y[:, :, None] * hr[deg].transpose(1, 0, 2)).astype(np.float64) + 1j * (Y[:, :, None] * hi[deg].transpose(1, 0, 2)).astype(np.float64)


def test_truth_agrees_with_scipy():
    rng = np.random.default_rng(3)
    L = 12
    pts = rng.standard_normal((12, 3)) * rng.uniform(0.3, 4.0, size=(12, 1))
    # (not the south pole itself: there scipy's theta = arccos(-1) is pi to one rounding only and its P_l^n is 1e-12 off zero)
    pts[0], pts[1], pts[2] = (0, 0, 1.5), (1e-3, -2e-3, -0.7), (1.1, -0.4, 0.0)
    k = np.array([0.4, 3.0, 9.0])
    B = _truth_basis(pts, k, L)
    for j, kj in enumerate(k):
        S = R.basis_scipy(pts, kj, L)
        # scipy's own error: a few ulp of |h_l| max |Y| in each factor, and arccos / arctan2 near the poles
        tol = 1e-13 * np.abs(S).max(0, keepdims=True) + 1e-13 * np.abs(S)
        assert (np.abs(B[:, :, j] - S) <= tol + 1e-300).all(), (j, float((np.abs(B[:, :, j] - S) / (tol + 1e-300)).max()))


def test_order_zero_is_the_free_space_green_function():
    rng = np.random.default_rng(4)
    pts = rng.standard_normal((9, 3)) * 2.0
    pts[0] = (0, 0, -3.0)
    k = np.array([0.3, 2.0, 25.0])
    c = (1j * k / math.sqrt(4 * math.pi))[None, :]  # (N = 1, m)
    r = np.linalg.norm(pts, axis=1)
    want = np.exp(1j * k[None, :] * r[:, None]) / (4 * math.pi * r[:, None])
    got = R.restate(pts, np.zeros(3), k, c, 0)
    assert np.abs(got - want).max() <= 1e-14 * np.abs(want).max() * (1 + k.max() * r.max())
    u, rl, inv = R.geometry(pts, np.zeros(3), LD)
    Y, dY = R.harmonics(u, 0, LD)
    hr, hi = R.hankel_truth(k, rl, 0)
    o_r, o_i = R.evaluate(Y, dY, u, inv, k, hr, hi, c)
    assert np.abs((o_r + 1j * o_i).astype(np.complex128) - want).max() <= 1e-14 * np.abs(want).max() * (1 + k.max() * r.max())


def _truth(pts, k, coef, L, gout=None):
    u, r, inv = R.geometry(pts, R.CENTER, LD)
    Y, dY = R.harmonics(u, L, LD)
    hr, hi = R.hankel_truth(k, r, L)
    return R.evaluate(Y, dY, u, inv, k, hr, hi, coef, gout)


def test_truth_gradients_against_central_differences():
    """gpts against central differences of the truth's forward at steps h and 2 h: the truncation error of the h difference is
    a third of what separates the two (measured, not assumed), the rounding 2^-63 |terms| / h.  gcoef against the forward's
    exact linearity in the coefficients."""
    rng = np.random.default_rng(8)
    L, m, P = 6, 3, 5
    pts = R.CENTER + rng.standard_normal((P, 3)) * 1.3
    pts[0] = R.CENTER + (0, 0, 0.9)   # on the z axis: an ordinary point
    pts[1] = R.CENTER + (0, 0, -1.7)
    k = np.array([0.6, 2.5, 7.0])
    coef = rng.standard_normal((R.nterms(L), m)) + 1j * rng.standard_normal((R.nterms(L), m))
    g = rng.standard_normal((P, m)) + 1j * rng.standard_normal((P, m))
    _, _, gp, gc_r, gc_i = _truth(pts, k, coef, L, g)
    phi = lambda x: (lambda o: (LD(g.real) * o[0] + LD(g.imag) * o[1]).sum(1))(_truth(x, k, coef, L))  # noqa: E731  per point
    h = 2e-4
    worst = 0.0
    for a in range(3):
        e = np.zeros(3)
        e[a] = h
        d1 = (phi(pts + e) - phi(pts - e)) / (2 * LD(h))
        d2 = (phi(pts + 2 * e) - phi(pts - 2 * e)) / (4 * LD(h))
        tol = np.abs(d1 - d2) / 3 * 1.5 + 2.0 ** -60 * np.abs(phi(pts)).max() / h
        q = np.abs(gp[:, a] - d1) / tol
        worst = max(worst, float(q.max()))
    print(f"RATIO gpts-fd {worst:.3g}")
    assert worst < 1
    delta = rng.standard_normal(coef.shape) + 1j * rng.standard_normal(coef.shape)
    o1, o0 = _truth(pts, k, coef + delta, L), _truth(pts, k, coef, L)
    lhs = (LD(g.real) * (o1[0] - o0[0]) + LD(g.imag) * (o1[1] - o0[1])).sum()
    rhs = (gc_r * LD(delta.real) + gc_i * LD(delta.imag)).sum()
    assert abs(lhs - rhs) <= 1e-15 * (np.abs(g).sum() * np.abs(o0[0]).max() + abs(rhs))


@pytest.mark.parametrize("P,m,L", R.CASES, ids=["-".join(map(str, c)) for c in R.CASES])
def test_restatement_stays_inside_the_bound(P, m, L):
    """The fp64 numpy restatement in the kernels' operation order, every element of every output, over the GPU test's grid."""
    c = R.case_truth(P, m, L)
    out, gp, gc, _ = R.restate(c["pts"], R.CENTER, c["k"], c["coef"], L, c["gout"])
    q = R.ratios(c, out, gp, gc)
    print("RATIO restate", P, m, L, {k: f"{v:.3g}" for k, v in q.items()})
    assert max(q.values()) < 1, q
    assert np.isfinite(out).all() and np.isfinite(gp).all() and np.isfinite(gc).all()
    if m >= 5:  # a column of zeros gives exact zeros
        assert (out[:, 3] == 0).all()


@pytest.mark.parametrize("P,m,L", [(63, 5, 7), (130, 64, 2), (1, 70, 32)])
def test_fp32_recurrence_leaves_the_bound(P, m, L):
    """The same restatement with the Hankel recurrence in fp32 does not pass: the bound has teeth."""
    c = R.case_truth(P, m, L)
    with np.errstate(all="ignore"):
        out = R.restate(c["pts"], R.CENTER, c["k"], c["coef"], L, None, np.float32)
    q = R.ratios(c, out)["out"]
    assert not q < 1, q
    assert not q < 1e3 or L == 32, q  # by orders of magnitude (at L = 32 the fp32 h_l overflows: not a number)


def test_grid_covers_what_it_claims():
    pts, k = R.grid()
    d = pts - R.CENTER
    r = np.linalg.norm(d, axis=1)
    kr = k[None, :] * r[:, None]
    assert kr.min() <= 0.0501 and kr.max() >= 199.9
    assert (k[0] * r[0] > 32 + 1) and (k[1] * r[1] < 1)  # l < k r for every l, and l > k r for every l >= 1: in the smallest case
    assert (d[0, :2] == 0).all() and d[0, 2] > 0 and (d[1, :2] == 0).all() and d[1, 2] < 0
    assert (d[2:6, 2] == 0).all() and d[2, 1] == 0 and d[3, 0] == 0
    assert len(R.CASES) == 60
    c = R.coefficients(5, 7)
    assert (c[1:4] == 0).all() and (c[:, 3] == 0).all() and (c != 0).sum() > c.size // 2


@pytest.mark.parametrize("L,k", R.MONO_CASES)
def test_fit_recovers_an_offset_monopole(L, k):
    """A unit monopole at distance b from the centre, sampled on r = 1.5, fitted at order L with scipy's basis and evaluated
    with the restatement on r = 1.6: within 4 (b / 1.5)^(L + 1) of the field's peak there."""
    N = R.nterms(L)
    ps = R.fibonacci_sphere(4 * N, R.MONO_RS)
    coef, res = R.fit_columns(R.basis_scipy(ps, k, L), R.monopole(ps, k))
    pt = R.fibonacci_sphere(200, R.MONO_RTEST)
    want = R.monopole(pt, k)
    got = R.restate(pt, np.zeros(3), np.array([k]), coef[:, None], L)[:, 0]
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"RATIO fit L={L} k={k} err/(b/Rs)^(L+1) = {err / (R.mono_bound(L) / 4):.3g} residual {res:.2e}")
    assert err <= R.mono_bound(L)
