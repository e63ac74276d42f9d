"""What vouches for tests/_contact_ref.py without a GPU: the numpy adjoint against central differences of the longdouble
forward, the exact properties of the scheme, a closed form, and the recovery run the device test repeats.

Central differences.  The loss is L = sum(gforce * force), every parameter th is moved by th (1 +- eta) in longdouble.  With
u = the longdouble epsilon, a central difference D(eta) carries a rounding error of about u Lmag / (eta |th|), Lmag = sum
|gforce| |force|, and a truncation error proportional to eta^2 and the loss's third derivative.  eta = u^(1/3) balances the
two where the derivatives scale like the loss over the parameter; they need not (delta^p near the ends of a contact, a second
hit whose timing hangs on the first), so the truncation error is measured, from the forward alone: D(2 eta) has four times
the error of D(eta), hence |D(2 eta) - D(eta)| / 3 estimates the latter.  The tolerance is twice that estimate plus
16 u Lmag / (eta |th|) for the roundings of the two differences - some 1e-11 of Lmag / |th| on x86, where a wrong term in the
adjoint shows at order 1.  The adjoint itself is run in longdouble here; its float64 form is held against it at 4096 float64
epsilons (a few thousand dependent steps)."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _contact_ref as C  # noqa: E402

LD = np.longdouble
U_LD = float(np.finfo(LD).eps)
ETA = U_LD ** (1.0 / 3.0)
IDS = [C.case_id(c) + "-" + str(i) for i, c in enumerate(C.CASES)]


@functools.lru_cache(maxsize=None)
def _truth(i):
    case = C.CASES[i]
    d, w, c, M, v0, kH, g = C.inputs(case)
    A, m, F, R, p = case[:5]
    fw = C.forward(d, w, c, M, v0, kH, F, p, R, dtype=LD)
    return fw, C.adjoint(g, d, w, c, M, v0, kH, p, R, dtype=LD)


@pytest.mark.parametrize("i", range(len(C.CASES)), ids=IDS)
def test_cases_show_their_properties(i):
    case = C.CASES[i]
    assert set(case[8]) <= C.properties(case, _truth(i)[0])
    assert np.isfinite(np.asarray(_truth(i)[0]["force"], dtype=np.float64)).all()


def test_case_table_covers_the_shapes():
    cover = lambda k: {c[k] for c in C.CASES}  # noqa: E731
    assert cover(0) == {1, 3} and cover(1) == {1, 5, 64, 70, 130} and cover(3) == {1, 4, 8}
    assert cover(2) >= {1, 2, 33, 64} and cover(4) == {1.0, 1.5, 2.0}
    assert {p for c in C.CASES for p in c[8]} == {"ends", "on", "none", "double", "zero_gain", "mixed"}


@pytest.mark.parametrize("i", [0, 2, 3, 4, 8], ids=[IDS[i] for i in (0, 2, 3, 4, 8)])
def test_adjoint_equals_central_differences(i):
    case = C.CASES[i]
    d, w, c, M, v0, kH, g = C.inputs(case)
    A, m, F, R, p = case[:5]
    fw, adj = _truth(i)
    g_ld = np.asarray(g, dtype=LD)
    Lmag = float((np.abs(g_ld) * np.abs(fw["force"])).sum())
    base = dict(d=d, w=w, c=c, M=M, v0=v0, kH=kH)

    def loss(**change):
        a = dict(base, **change)
        return (g_ld * C.forward(a["d"], a["w"], a["c"], a["M"], a["v0"], a["kH"], F, p, R, dtype=LD)["force"]).sum()

    def central(name, idx):
        x = np.asarray(base[name], dtype=LD)
        th = x[idx]
        out = []
        for eta in (LD(ETA), 2 * LD(ETA)):
            hi, lo = x.copy(), x.copy()
            hi[idx], lo[idx] = th * (1 + eta), th * (1 - eta)
            out.append((loss(**{name: hi}) - loss(**{name: lo})) / (hi[idx] - lo[idx]))
        return out[0], float(abs(out[1] - out[0])) / 3, float(abs(th))

    rng = np.random.default_rng(i)
    modes = sorted(set([0, m - 1]) | set(rng.integers(0, m, 2).tolist()))
    clips = [a for a in range(A) if v0[a] > 0]
    checks = [("d", "gd", (j,)) for j in modes] + [("w", "gw", (j,)) for j in modes]
    checks += [("c", "gc", (a, j)) for a in clips for j in modes if c[a, j] != 0]
    checks += [(n, k, (a,)) for a in clips for n, k in (("M", "gM"), ("v0", "gv0"), ("kH", "gkH"))]
    worst = 0.0
    for name, key, idx in checks:
        fd, trunc, th = central(name, idx)
        tol = 2 * trunc + 16 * U_LD * Lmag / (ETA * th)
        err = float(abs(fd - adj[key][idx]))
        worst = max(worst, err / tol)
        assert err <= tol, (name, idx, float(fd), float(adj[key][idx]), err / tol)
    print(f"RATIO contact.fd {C.case_id(case)} {worst:.3g}")
    # a clip the hammer never reaches: nothing moves its force, and the adjoint says exactly that
    for a in range(A):
        if v0[a] <= 0:
            assert not adj["gc"][a].any() and adj["gM"][a] == 0 and adj["gv0"][a] == 0 and adj["gkH"][a] == 0


@pytest.mark.parametrize("i", range(len(C.CASES)), ids=IDS)
def test_float64_adjoint_follows_the_longdouble_one(i):
    case = C.CASES[i]
    d, w, c, M, v0, kH, g = C.inputs(case)
    a64 = C.adjoint(g, d, w, c, M, v0, kH, case[4], case[3])
    for k in C.GRADS:
        E, scale = C.e64(a64[k], _truth(i)[1][k])
        assert E <= 4096 * C.EPS64, (k, E)


def test_no_approach_gives_exact_zeros():
    d, w, c, M, v0, kH, g = C.inputs(C.CASES[3])
    for v in (0.0, -1.0):
        vv = np.full_like(v0, v)
        fw = C.forward(d, w, c, M, vv, kH, 33, 1.0, 4)
        assert not fw["force"].any() and not fw["f"].any()
        adj = C.adjoint(g, d, w, c, M, vv, kH, 1.0, 4)
        assert all(not np.asarray(adj[k]).any() for k in C.GRADS)


def test_zero_gain_removes_a_mode_exactly():
    d, w, c, M, v0, kH, _ = C.inputs(C.CASES[0])
    c = c.copy()
    c[:, 2] = 0.0
    keep = [0, 1, 3, 4]
    with_zero = C.forward(d, w, c, M, v0, kH, 64, 1.5, 8)
    without = C.forward(d[keep], w[keep], c[:, keep], M, v0, kH, 64, 1.5, 8)
    assert np.array_equal(with_zero["force"], without["force"]) and with_zero["force"].any()


def test_vanishing_stiffness_lets_the_hammer_move_freely():
    d, w, c, M, v0, kH, _ = C.inputs(C.CASES[0])
    fw = C.forward(d, w, c, M, v0, np.full_like(kH, 1e-30), 64, 1.5, 8)
    N = 64 * 8
    assert np.array_equal(fw["vh"], v0)
    assert abs(fw["xh"][0] / (N * fw["h"] * v0[0]) - 1) <= N * C.EPS64
    assert fw["force"].max() < 1e-30


def test_momentum_balance():
    """M (v0 - vh_end) = h sum f: the hammer's momentum goes into the impulse, to rounding (N steps, each vh -= h f / M)."""
    for i in (0, 2, 8):
        case = C.CASES[i]
        d, w, c, M, v0, kH, _ = C.inputs(case)
        fw = C.forward(d, w, c, M, v0, kH, case[2], case[4], case[3])
        N = case[2] * case[3]
        lhs, rhs = M * (v0 - fw["vh"]), fw["h"] * fw["f"].sum(-1)
        assert (np.abs(lhs - rhs) <= 4 * N * C.EPS64 * M * np.abs(v0)).all(), (lhs, rhs)
        assert (rhs > 0).all()


def _two_mass(t, M, kH, c, w, v0):
    """f(t) = kH (x - u) of  M x'' = -f,  u'' / c^2 + (w^2 / c^2) u = f,  x(0) = u(0) = 0, x'(0) = v0, u'(0) = 0 (one undamped
    mode, p = 1, in contact): two normal modes, in closed form."""
    mu = 1.0 / (c * c)
    a, b, cc = M * mu, -(M * (kH + w * w * mu) + mu * kH), kH * w * w * mu  # det(K - lam Mm) = a lam^2 + b lam + cc
    disc = np.sqrt(b * b - 4 * a * cc)
    f = np.zeros_like(t)
    for lam in ((-b - disc) / (2 * a), (-b + disc) / (2 * a)):
        phi = np.array([kH, kH - lam * M])  # (K - lam Mm) phi = 0, first row
        coef = (phi[0] * M * v0) / (phi[0] ** 2 * M + phi[1] ** 2 * mu)  # modal velocity, Mm-orthogonal expansion
        om = np.sqrt(lam)
        f += kH * (phi[0] - phi[1]) * coef * np.sin(om * t) / om
    return f


def test_linear_contact_matches_the_two_mass_system_to_first_order():
    """One undamped mode, p = 1: while in contact the substep forces follow the closed form, and the error at least halves when
    R doubles (first order is what the scheme promises; with the hammer's velocity staggered half a step against its position
    the forces come out second-order accurate on this linear system, so the measured ratio is 4)."""
    M, kH, c, wd, v0, F = 0.01, 1e7, 1.5, 2 * np.pi * 700.0, 1.0, 48
    errs = []
    for R in (4, 8, 16):
        fw = C.forward(np.zeros(1), np.array([wd]), np.array([[c]]), np.array([M]), np.array([v0]), np.array([kH]), F, 1.0, R)
        f = fw["f"][0]
        on = np.flatnonzero(f > 0)
        assert on[0] == 1 and on[-1] < F * R - 1 and C.contact_intervals(f) == 1
        last = on[-1] - R  # stay clear of the release, where the closed form ends at a slightly different time
        t = np.arange(1, last) * float(fw["h"])
        errs.append(np.abs(f[1:last] - _two_mass(t, M, kH, c, wd, v0)).max() / f.max())
    assert errs[0] < 0.05
    for coarse, fine in zip(errs, errs[1:]):
        assert coarse / fine >= 2.0, errs


def test_recovery_run_on_the_restatement():
    ratio = C.recovery_numpy()
    print(f"RATIO contact.recovery.numpy {ratio:.3g}")
    assert ratio < 1e-3
