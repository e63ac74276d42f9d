"""What vouches for tests/_friction_ref.py without a GPU: the numpy adjoint against central differences of the longdouble
forward, the condition E64 <= 1e-10 that admits a case to the device tests, the exact properties of the scheme, its two
limits (free slipping, sticking), the energy balance and the recovery run the device test repeats.

Central differences, as in tests/test_contact_ref_cpu.py.  The loss is L = sum(gforce * force), a parameter th is moved by
+- eta |th| in longdouble (by +- eta where th = 0: a normal force that has been released).  With u = the longdouble epsilon, a
central difference D(eta) carries a rounding error of about u Lmag / step, Lmag = sum |gforce| |force|, and a truncation
error proportional to eta^2 and the loss's third derivative, which is measured from the forward alone: D(2 eta) has four
times the error of D(eta), hence |D(2 eta) - D(eta)| / 3 estimates the latter.  The tolerance is twice that estimate plus
16 u Lmag / step for the roundings of the two differences.  The adjoint itself is run in longdouble here."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _friction_ref as Fr  # noqa: E402

LD = np.longdouble
U_LD = float(np.finfo(LD).eps)
ETA = U_LD ** (1.0 / 3.0)
IDS = [Fr.case_id(c) + "-" + str(i) for i, c in enumerate(Fr.CASES)]


@functools.lru_cache(maxsize=None)
def _refs(i):
    """(float64, longdouble) restatements of case i: forward and adjoint."""
    case = Fr.CASES[i]
    d, w, c, vb, N, vs, g = Fr.inputs(case)
    out = []
    for dt in (np.float64, LD):
        fw = Fr.forward(d, w, c, vb, N, vs, case[3], dtype=dt)
        out.append(dict(Fr.adjoint(g, d, w, c, vb, N, vs, case[3], dtype=dt), force=fw["force"], vr=fw["vr"]))
    return out


@pytest.mark.parametrize("i", range(len(Fr.CASES)), ids=IDS)
def test_cases_show_their_properties_and_are_well_conditioned(i):
    """Each gesture shows what it is there for on the reference's vr, the explicit scheme is far inside its stability bound,
    and the float64 restatement alone stays within E64_MAX of the longdouble one in every output: what admits the case to the
    device tests."""
    case = Fr.CASES[i]
    r64, rld = _refs(i)
    assert set(case[4]) | set(case[5]) <= Fr.properties(case, rld)
    assert (Fr.stability(case) < 0.1).all()
    worst = 0.0
    for k in ("force",) + Fr.GRADS:
        assert np.isfinite(np.asarray(rld[k], dtype=np.float64)).all(), k
        E, _ = Fr.e64(r64[k], rld[k])
        worst = max(worst, E)
        assert E <= Fr.E64_MAX, (k, E)
    print(f"RATIO friction.e64 {Fr.case_id(case)} {worst:.3g}")


def test_case_table_covers_the_shapes():
    cover = lambda k: {c[k] for c in Fr.CASES}  # noqa: E731
    assert cover(0) == {1, 3} and cover(1) == {1, 5, 64, 70, 130} and cover(3) == {1, 4, 8, 64}
    assert cover(2) == {1, 2, 32, 33, 64}
    assert {p for c in Fr.CASES for p in c[4]} == set(Fr.KINDS)
    assert {p for c in Fr.CASES for p in c[5]} == {"zero_gain", "mixed"}


@pytest.mark.parametrize("i", [0, 2, 3, 4, 7, 8], ids=[IDS[i] for i in (0, 2, 3, 4, 7, 8)])
def test_adjoint_equals_central_differences(i):
    case = Fr.CASES[i]
    d, w, c, vb, N, vs, g = Fr.inputs(case)
    A, m, F, R = case[:4]
    r64, adj = _refs(i)
    g_ld = np.asarray(g, dtype=LD)
    Lmag = float((np.abs(g_ld) * np.abs(adj["force"])).sum())
    base = dict(d=d, w=w, c=c, vb=vb, N=N, vs=vs)

    def loss(**change):
        a = dict(base, **change)
        return (g_ld * Fr.forward(a["d"], a["w"], a["c"], a["vb"], a["N"], a["vs"], R, dtype=LD)["force"]).sum()

    def central(name, idx):
        x = np.asarray(base[name], dtype=LD)
        step = abs(x[idx]) if x[idx] != 0 else LD(1)
        out = []
        for eta in (LD(ETA), 2 * LD(ETA)):
            hi, lo = x.copy(), x.copy()
            hi[idx], lo[idx] = x[idx] + eta * step, x[idx] - eta * step
            out.append((loss(**{name: hi}) - loss(**{name: lo})) / (hi[idx] - lo[idx]))
        return out[0], float(abs(out[1] - out[0])) / 3, float(step)

    rng = np.random.default_rng(i)
    modes = sorted(set([0, m - 1]) | set(rng.integers(0, m, 2).tolist()))
    samples = sorted(set([0, F - 1, (F + 1) // 2 - 1, min((F + 1) // 2, F - 1)]) | set(rng.integers(0, F, 2).tolist()))
    checks = [("d", "gd", (j,)) for j in modes] + [("w", "gw", (j,)) for j in modes]
    checks += [("c", "gc", (a, j)) for a in range(A) for j in modes]
    checks += [(n, k, (a, t)) for a in range(A) for t in samples for n, k in (("vb", "gvb"), ("N", "gN"))]
    checks += [("vs", "gvs", (a,)) for a in range(A)]
    worst = 0.0
    for name, key, idx in checks:
        fd, trunc, step = central(name, idx)
        tol = 2 * trunc + 16 * U_LD * Lmag / (ETA * step)
        err = float(abs(fd - adj[key][idx]))
        worst = max(worst, err / tol)
        assert err <= tol, (name, idx, float(fd), float(adj[key][idx]), err / tol)
    print(f"RATIO friction.fd {Fr.case_id(case)} {worst:.3g}")


def test_no_normal_force_gives_exact_zeros():
    """N = 0 for a whole clip: its force and every gradient but gN are exact zeros; gN is not (pressing would make a force)."""
    case = Fr.CASES[3]
    d, w, c, vb, N, vs, g = Fr.inputs(case)
    a = case[4].index("idle")
    for dt in (np.float64, LD):
        fw = Fr.forward(d, w, c, vb, N, vs, case[3], dtype=dt)
        assert not fw["force"][a].any() and not fw["f"][a].any() and not fw["s_end"][a].any()
        adj = Fr.adjoint(g, d, w, c, vb, N, vs, case[3], dtype=dt)
        assert not adj["gc"][a].any() and not adj["gvb"][a].any() and adj["gvs"][a] == 0
        assert adj["gN"][a].all()
    # every clip idle: the modes' gradients are exact zeros too
    adj = Fr.adjoint(g, d, w, c, vb, np.zeros_like(N), vs, case[3])
    assert all(not np.asarray(adj[k]).any() for k in Fr.GRADS if k != "gN") and adj["gN"].any()


def test_zero_gain_removes_a_mode_exactly():
    case = Fr.CASES[0]
    d, w, c, vb, N, vs, _ = Fr.inputs(case)
    c = c.copy()
    c[:, 2] = 0.0
    keep = [0, 1, 3, 4]
    with_zero = Fr.forward(d, w, c, vb, N, vs, case[3])
    without = Fr.forward(d[keep], w[keep], c[:, keep], vb, N, vs, case[3])
    assert np.array_equal(with_zero["force"], without["force"]) and with_zero["force"].any()


def test_a_fast_bow_slips_freely():
    """vb = 5 vs and one mode: the surface hardly answers, and the force tends to N phi(vb).  The surface's velocity under a
    force f0 stays below f0 g / w (a step on a continuous resonator; twice that is allowed for the discrete one), which moves
    phi by the factor (x - 1 / x) v / vs at most."""
    wd, dd, g, vs, Nn, F, R = Fr.TWO_PI * 700.0, 4.0, 1.0, 0.1, 40.0, 64, 8
    x = 5.0
    f0 = Nn * x * np.exp((1 - x * x) / 2)
    fw = Fr.forward(np.array([dd]), np.array([wd]), np.array([[np.sqrt(g)]]), np.full((1, F), x * vs), np.full((1, F), Nn),
                    np.array([vs]), R)
    vmax = 2 * f0 * g / wd
    tol = (x - 1 / x) * vmax / vs
    assert tol < 1e-3
    assert np.abs(fw["force"] / f0 - 1).max() <= tol
    assert 0 < np.abs(fw["v"]).max() <= vmax


def test_a_heavy_slow_bow_sticks():
    """Large N / vs inside the stability bound, a bow at vs / 2 on one mode of 200 Hz: around vr = 0 the characteristic is a
    damper K = N sqrt(e) / vs that drags the surface along, so v follows vb.  The mode holds back with its spring, w^2 t vb / g
    after t seconds, which the damper balances at vr = w^2 t vb / (g K): 7 % of vb at the end of the window.  Asserted: |vr| below
    vs, and below vb / 5, from the first eighth of the window on (the damper settles in 1 / (g K) = 1.3 samples)."""
    wd, dd, g, vs, Nn, F, R = Fr.TWO_PI * 200.0, 4.0, 1.0, 0.1, 2000.0, 64, 8
    K = Nn * np.sqrt(np.e) / vs
    assert K * g / (Fr.SR * R) < 0.1 and wd * wd * (F / Fr.SR) / (g * K) < 0.1
    vb = 0.5 * vs
    fw = Fr.forward(np.array([dd]), np.array([wd]), np.array([[np.sqrt(g)]]), np.full((1, F), vb), np.full((1, F), Nn),
                    np.array([vs]), R)
    assert fw["vr"][0, 0] == vb  # it starts at the bow's own velocity, the surface at rest
    settled = np.abs(fw["vr"][0, F * R // 8:])
    assert (settled < vs).all() and (settled < 0.2 * vb).all()
    assert (np.abs(fw["v"][0, F * R // 8:] - vb) < 0.2 * vb).all()


def _energy_gap(R):
    """|work of the friction force - (the modes' energy gain + their dissipation)| over the gross work sum_n h |f v| (the net
    work of a slipping bow on a surface that swings to and fro nearly cancels), one slipping clip.
    Mode i is q'' + 2 d q' + (w^2 + d^2) q = f with q = Im s / w, q' = Re s - r Im s and the weight g_i = c_i^2: energy
    g (q'^2 + (w^2 + d^2) q^2) / 2, dissipated power 2 d g q'^2, power taken f g q'."""
    rng = np.random.default_rng(73)
    m, F, vs = 5, 64, 0.1
    d, w = Fr.modes(m, rng)
    c = rng.uniform(0.5, 1.5, (1, m)) / np.sqrt(m)
    vb, N = np.full((1, F), 2 * vs), np.full((1, F), 100.0)
    fw = Fr.forward(d, w, c, vb, N, np.array([vs]), R, keep=True)
    h, g = float(fw["h"]), (c * c)[0]
    qd = fw["s"][:, 0, :].real - (d / w) * fw["s"][:, 0, :].imag
    work = h * (fw["f"][0] * fw["v"][0]).sum()
    lost = h * (2 * d * g * qd * qd).sum()
    s_end = fw["s_end"][0]
    qd_end, q_end = s_end.real - (d / w) * s_end.imag, s_end.imag / w
    gain = 0.5 * (g * (qd_end ** 2 + (w * w + d * d) * q_end ** 2)).sum()
    assert gain > 0 and lost > 0
    return abs(work - gain - lost) / (h * np.abs(fw["f"][0] * fw["v"][0]).sum())


def test_energy_balance_to_the_schemes_order():
    """sum_n h f v = the modes' energy gain + their dissipation, to first order in h: the gap at least halves (less a tenth
    for the higher-order terms) when R doubles, and is small at R = 32."""
    gaps = [_energy_gap(R) for R in (8, 16, 32)]
    print("RATIO friction.energy_gap " + " ".join(f"{x:.3g}" for x in gaps))
    assert gaps[-1] < 0.05
    for coarse, fine in zip(gaps, gaps[1:]):
        assert coarse / fine >= 1.8, gaps


def test_bow_envelope():
    env = Fr.envelope(64, Fr.SR, 8 / Fr.SR, 16 / Fr.SR)
    assert env[0] == 0 and env[-1] == 0 and (env[8:48] == 1).all() and (np.diff(env[:9]) > 0).all() and (np.diff(env[47:]) < 0).all()
    assert (Fr.envelope(5, Fr.SR, 0.0, 0.0) == 1).all()


def test_recovery_run_on_the_restatement():
    ratio = Fr.recovery_numpy()
    print(f"RATIO friction.recovery.numpy {ratio:.3g}")
    assert ratio < 1e-2
