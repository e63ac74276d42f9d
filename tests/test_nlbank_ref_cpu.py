"""What vouches for tests/_nlbank_ref.py without a GPU: the numpy adjoint against central differences of the longdouble
forward, the condition E64 <= 1e-10 that admits a case to the device tests, the linear limit (the driven bank), the glide of
the Duffing oscillator, the scheme's first order in the substep and the recovery run the device test repeats.

Central differences, as in tests/test_friction_ref_cpu.py.  The loss is L = sum(gy * y), a parameter th is moved by
+- eta |th| in longdouble (by +- eta where th = 0: a coupling of zero, a force of zero, a stretch coefficient of zero).  With
u = the longdouble epsilon, a central difference D(eta) carries a rounding error of about u Lmag / step, Lmag = sum |gy| |y|,
and a truncation error proportional to eta^2 and the loss's third derivative, which is measured from the forward alone:
D(2 eta) has four times the error of D(eta), hence |D(2 eta) - D(eta)| / 3 estimates the latter.  The tolerance is twice that
estimate plus 16 u Lmag / step for the roundings of the two differences.  The adjoint itself is run in longdouble here."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _nlbank_ref as Nl  # noqa: E402
import _osc_driven_ref as Od  # noqa: E402

LD = np.longdouble
U_LD = float(np.finfo(LD).eps)
ETA = U_LD ** (1.0 / 3.0)
IDS = [Nl.case_id(c) + "-" + str(i) for i, c in enumerate(Nl.CASES)]


@functools.lru_cache(maxsize=None)
def _refs(i):
    """(float64, longdouble) restatements of case i: forward and adjoint."""
    case = Nl.CASES[i]
    d, w, c, amp, f, C, gamma, gy = Nl.inputs(case)
    out = []
    for dt in (np.float64, LD):
        fw = Nl.forward(d, w, c, amp, f, C, gamma, case[5], case[3], dtype=dt)
        out.append(dict(Nl.adjoint(gy, d, w, c, amp, f, C, gamma, case[3], dtype=dt), y=fw["y"], kap_max=fw["kap_max"]))
    return out


@pytest.mark.parametrize("i", range(len(Nl.CASES)), ids=IDS)
def test_cases_are_well_conditioned(i):
    """The explicit scheme is far inside its stability bound, and the float64 restatement alone stays within E64_MAX of the
    longdouble one in every output: what admits the case to the device tests."""
    case = Nl.CASES[i]
    r64, rld = _refs(i)
    assert (Nl.stability(case, rld) < 0.1).all()
    worst = 0.0
    for k in ("y",) + Nl.GRADS:
        assert np.isfinite(np.asarray(rld[k], dtype=np.float64)).all(), k
        E, _ = Nl.e64(r64[k], rld[k])
        worst = max(worst, E)
        assert E <= Nl.E64_MAX, (k, E)
    print(f"RATIO nlbank.e64 {Nl.case_id(case)} {worst:.3g} glide {Nl.glide(case, rld).max():.3g}")


def test_case_table_covers_the_shapes_and_the_strongest_case_glides():
    """The shapes the kernels branch on, and amplitudes that matter: the strongest case raises its lowest mode's frequency by
    5 to 10 % at the peak of the stiffening, every hard strike by more than 1 %."""
    cover = lambda k: {c[k] for c in Nl.CASES}  # noqa: E731
    assert cover(0) == {1, 3} and cover(1) == {1, 3, 5, 65, 70, 130, 260} and cover(2) == {1, 2, 3, 4}
    assert cover(3) == {1, 2, 4, 8, 64}
    assert {(-(-c[1] // 64)) for c in Nl.CASES} == {1, 2, 3, 5} and (1, 260, 4, 2, 40, 40, ("hard",)) in Nl.CASES
    rel = {np.sign(c[4] - c[5]) * min(abs(c[4] - c[5]), 3) for c in Nl.CASES}
    assert rel >= {-3, 0, 3} and {70, 130} <= cover(4)
    assert {k for c in Nl.CASES for k in c[6]} == set(Nl.KINDS)
    glides = []
    for i, case in enumerate(Nl.CASES):
        g = Nl.glide(case, _refs(i)[1])
        for a, kind in enumerate(case[6]):
            if kind == "hard":
                assert g[a] > 0.01, (i, a, g[a])
                glides.append(g[a])
            else:
                assert (g[a] == 0) == (kind == "linear" or kind == "idle")
    print(f"RATIO nlbank.glide max {max(glides):.3g} min {min(glides):.3g}")
    assert 0.05 <= max(glides) <= 0.10


@pytest.mark.parametrize("i", [0, 1, 4, 5], ids=[IDS[i] for i in (0, 1, 4, 5)])
def test_adjoint_equals_central_differences(i):
    case = Nl.CASES[i]
    d, w, c, amp, f, C, gamma, gy = Nl.inputs(case)
    A, m, K, R, F, S = case[:6]
    _, adj = _refs(i)
    g_ld = np.asarray(gy, dtype=LD)
    Lmag = float((np.abs(g_ld) * np.abs(adj["y"])).sum())
    base = dict(d=d, w=w, c=c, amp=amp, f=f, C=C, gamma=gamma)

    def loss(**change):
        a = dict(base, **change)
        return (g_ld * Nl.forward(a["d"], a["w"], a["c"], a["amp"], a["f"], a["C"], a["gamma"], S, R, dtype=LD)["y"]).sum()

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
    samples = sorted(set([0, F - 1, min(S, F) - 1, min(11, F - 1)]) | set(rng.integers(0, F, 2).tolist()))
    checks = [("d", "gd", (j,)) for j in modes] + [("w", "gw", (j,)) for j in modes]
    checks += [(n, k, (a, j)) for a in range(A) for j in modes for n, k in (("c", "gc"), ("amp", "gamp"))]
    checks += [("f", "gf", (a, t)) for a in range(A) for t in samples]
    checks += [("C", "gC", (r, j)) for r in range(K) for j in modes]
    checks += [("gamma", "ggamma", (a, r)) for a in range(A) for r in range(K)]
    worst = 0.0
    for name, key, idx in checks:
        fd, trunc, step = central(name, idx)
        tol = 2 * trunc + 16 * U_LD * Lmag / (ETA * step)
        err = float(abs(fd - adj[key][idx]))
        worst = max(worst, err / tol)
        assert err <= tol, (name, idx, float(fd), float(adj[key][idx]), err / tol)
    print(f"RATIO nlbank.fd {Nl.case_id(case)} {worst:.3g}")


def test_exact_zeros_of_the_idle_and_the_linear_clip():
    """A clip without force: y and every gradient of its own but gf are exact zeros.  A clip with gamma = 0: its contribution
    to gC is exact zeros, its ggamma is not (coupling would change the sound).  Force samples at k >= S: gf is exactly 0."""
    case = Nl.CASES[5]
    d, w, c, amp, f, C, gamma, gy = Nl.inputs(case)
    idle, lin = case[6].index("idle"), case[6].index("linear")
    for dt in (np.float64, LD):
        fw = Nl.forward(d, w, c, amp, f, C, gamma, case[5], case[3], dtype=dt)
        adj = Nl.adjoint(gy, d, w, c, amp, f, C, gamma, case[3], dtype=dt, per_clip=True)
        assert not fw["y"][idle].any() and not fw["s_end"][idle].any()
        for k in ("gc", "gamp", "ggamma", "gd_a", "gw_a", "gC_a"):
            assert not adj[k][idle].any(), k
        assert adj["gf"][idle].all()
        assert not adj["gC_a"][lin].any() and adj["ggamma"][lin].all() and adj["gC_a"][0].any()
    case = Nl.CASES[2]
    d, w, c, amp, f, C, gamma, gy = Nl.inputs(case)
    adj = Nl.adjoint(gy, d, w, c, amp, f, C, gamma, case[3])
    assert case[4] == case[5] + 3 and not adj["gf"][:, case[5]:].any() and adj["gf"][:, :case[5]].all()
    longer = np.concatenate([f, np.full((1, 4), 7.0)], axis=1)
    y0, y1 = (Nl.forward(d, w, c, amp, x, C, gamma, case[5], case[3])["y"] for x in (f, longer))
    assert np.array_equal(y0, y1)


@pytest.mark.parametrize("i", [1, 5, 6], ids=[IDS[i] for i in (1, 5, 6)])
def test_without_coupling_it_is_the_driven_bank(i):
    """gamma = 0 and R = 1: y is the driven bank's with the amplitudes amp c, to the float64 level - the recurrence against
    the direct convolution of tests/_osc_driven_ref.py, at that file's own fp64 bound k64 Emag (no fp32 term: nothing is
    rounded to fp32 here)."""
    case = Nl.CASES[i]
    A, m, K, R, F, S = case[:6]
    d, w, c, amp, f, C, gamma, _ = Nl.inputs(case)
    y = Nl.forward(d, w, c, amp, f, C, np.zeros_like(gamma), S, 1)["y"]
    ref, Emag = Od.forward(d, w, amp * c, f, S, Nl.SR)
    assert np.abs(ref).max() > 0
    err = np.abs(y - ref)
    bound = Od.k64(A, m, S) * Emag
    print(f"RATIO nlbank.linear {Nl.case_id(case)} {float((err[bound > 0] / bound[bound > 0]).max()):.3g}")
    assert (err <= bound).all()


DUFFING = dict(f0=1000.0, d=300.0, S=1024, R=16, shift=0.08)


@functools.lru_cache(maxsize=None)
def _duffing():
    """One mode of 1 kHz that decays by e^-7 over the window, struck by a 12-sample pulse, its coupling scaled so that the
    first-order shift at the amplitude of the linear response's peak is 8 %; longdouble.  Returns (t of the upward zero
    crossings of q, by linear interpolation between substeps [s], q (S R,), w, gamma C^2)."""
    P = DUFFING
    w = np.array([Nl.TWO_PI * P["f0"]])
    d = np.array([P["d"]])
    one = np.ones((1, 1))
    f = np.zeros((1, 12))
    f[0] = 0.5 - 0.5 * np.cos(Nl.TWO_PI * (np.arange(12) + 0.5) / 12)
    lin = Nl.forward(d, w, one, one, f, one, np.zeros((1, 1)), 64, P["R"], keep=True)
    apk = np.abs(lin["s"][:, 0, 0].imag / w[0]).max()
    gamma = np.array([[P["shift"] * 8 * w[0] ** 2 / (3 * apk ** 2)]])
    fw = Nl.forward(d, w, one, one, f, one, gamma, P["S"], P["R"], dtype=LD, keep=True)
    q = np.asarray(fw["s"][:, 0, 0].imag, dtype=np.float64) / w[0]
    h = 1.0 / (Nl.SR * P["R"])
    n = np.nonzero((q[:-1] < 0) & (q[1:] >= 0))[0]
    n = n[n >= 12 * P["R"]]  # free vibration only
    t = (n + q[n] / (q[n] - q[n + 1])) * h
    return t, q, w[0], float(gamma[0, 0])


def test_the_duffing_oscillator_glides_down_to_its_small_amplitude_pitch():
    """m = 1, K = 1: q'' + 2 d q' + (w^2 + d^2) q + gamma C^2 q^3 = 0 after the strike.  The period between upward zero crossings
    is shorter early than late and grows monotonically over the first ten of them; late it is 2 pi / w - to 1e-4: the residual
    shift 3 gamma C^2 a^2 / (8 w^2) at an amplitude that has decayed by e^-6 since the first period is 0.08 e^-12 = 5e-7, and
    the crossing's linear interpolation between substeps errs by (w h)^2 / 8 = 1e-5 of a period at most.

    Early, the shift of the first period against 2 pi / w is compared with the first-order prediction
    dw = 3 gamma C^2 a^2 / (8 w) at the measured amplitude, a^2 = the period's crest times its trough (the amplitude decays by
    e^-0.3 inside the period; crest and trough lie a quarter and three quarters into it, their product is a^2 at its middle).
    Measured on the longdouble reference: the shift is 0.9867 of the prediction, 1.33 % short of it - what lies beyond first
    order (the Duffing frequency's second-order term, -15/256 (gamma C^2 a^2 / w^2)^2 w, and the decay's own curvature).  The
    margin is twice that: 2.7 %."""
    t, q, w, g = _duffing()
    periods = np.diff(t)
    assert len(periods) >= 20
    assert (np.diff(periods[:10]) > 0).all() and periods[0] < 0.97 * periods[-1]
    late = periods[-3:].mean()
    assert abs(late * w / Nl.TWO_PI - 1) <= 1e-4
    h = 1.0 / (Nl.SR * DUFFING["R"])
    first = q[int(t[0] / h):int(t[1] / h) + 1]
    a2 = first.max() * -first.min()
    shift = Nl.TWO_PI / periods[0] - w
    predicted = 3 * g * a2 / (8 * w)
    print(f"RATIO nlbank.duffing shift/w {shift / w:.4g} predicted/w {predicted / w:.4g} ratio {shift / predicted:.4g}")
    assert 0.03 * w < shift < 0.12 * w
    assert abs(shift / predicted - 1) <= 0.027


def test_first_order_in_the_substep():
    """Doubling R at a fixed input changes y by about half as much again: the differences between R, 2 R, 4 R and 8 R fall
    monotonically, each below 0.7 of the one before (first order would be 0.5)."""
    case = Nl.CASES[1]
    d, w, c, amp, f, C, gamma, _ = Nl.inputs(case)
    ys = [Nl.forward(d, w, c, amp, f, C, gamma, case[5], R)["y"] for R in (8, 16, 32, 64)]
    diffs = [float(np.abs(b - a).max()) for a, b in zip(ys, ys[1:])]
    print("RATIO nlbank.order " + " ".join(f"{x:.3g}" for x in diffs))
    assert diffs[0] > 0
    for coarse, fine in zip(diffs, diffs[1:]):
        assert fine < 0.7 * coarse, diffs


def test_recovery_run_on_the_restatement():
    losses = Nl.recovery_numpy()
    print(f"RATIO nlbank.recovery.numpy {losses[-1] / losses[0]:.3g}")
    assert losses[-1] / losses[0] < 1e-2
