"""tests/_delay_ref.py anchored without a GPU: the interpolation kernel's properties, the integer delay as a shift, and the
reference's adjoint against central differences of its own forward, in fp64."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _delay_ref as DL  # noqa: E402

R = DL.R


def test_h_is_the_unit_sample_at_the_integers():
    i = np.arange(-R - 2, R + 3, dtype=np.float64)
    assert np.abs(DL.h(-i) - (i == 0)).max() < 1e-16
    assert DL.h(0.0) == 1.0 and DL.dh(0.0) == 0.0


def test_value_and_slope_vanish_at_the_ends():
    """h = O(e^3) and h' = O(e^2) a distance e inside +-R (sinc has a zero there, the window a double one); 0 outside."""
    for e in (1e-2, 1e-3, 1e-4):
        for sgn in (-1.0, 1.0):
            assert abs(DL.h(sgn * (R - e))) < e ** 3 and abs(DL.dh(sgn * (R - e))) < e ** 2
    out = np.array([-R - 1.0, -float(R), float(R), R + 0.5])
    assert not DL.h(out).any() and not DL.dh(out).any()


def test_the_derivative_is_that_of_h():
    """h' against central differences of h at step e: truncation e^2 / 6 |h'''| (|h'''| < 40), rounding 2 U64 / e."""
    u = np.concatenate([np.linspace(-R + 0.01, R - 0.01, 4001), [0.0, 1e-9, -1e-7, 0.1249999, 0.125, 0.1250001, -0.125, 3e-4]])
    e = 1e-5
    cd = (DL.h(u + e) - DL.h(u - e)) / (2 * e)
    assert np.abs(DL.dh(u) - cd).max() < e * e * 40 / 6 + 4 * DL.U64 / e
    # the series and the quotient of sinc' agree where they meet
    x = np.array([0.125 - 1e-12, 0.125])
    assert abs(np.diff(DL.dsinc(x))[0]) < 1e-11
    q = (np.cos(np.pi * 0.12) - np.sinc(0.12)) / 0.12
    assert abs(DL.dsinc(np.array([0.12]))[0] - q) < 64 * DL.U64


@pytest.mark.parametrize("N", [0, 1, 5, 40])
def test_an_integer_delay_is_a_shift(N):
    rng = np.random.default_rng(N)
    s = rng.standard_normal((2, 33)).astype(np.float32)
    y = DL.forward(s, np.full((2, 3), float(N)), 16)["y"]
    want = np.zeros((2, 33))
    if N < 33:
        want[:, N:] = s[:, :33 - N]
    assert np.abs(y - want).max() < 64 * DL.U64 * np.abs(s).sum(1).max()


def test_frames_and_a_delay_past_everything():
    p, _ = DL.positions(np.array([[2.0, 10.0, 4.0]]), 16, 50)
    assert p[0, 0] == -2.0 and p[0, 8] == 8 - 6.0 and p[0, 16] == 16 - 10.0 and p[0, 24] == 24 - 7.0
    assert (p[0, 32:] == np.arange(32, 50) - 4.0).all()                                   # the last frame held
    f = DL.forward(np.ones((1, 20), dtype=np.float32), np.full((1, 1), 20 + R + 1.5), 16)
    assert not f["y"].any() and not f["mag"].any()
    assert np.isnan(DL.forward(np.ones((1, 20), dtype=np.float32), np.array([[0.0, np.inf]]), 16)["y"][0, 1:16]).all()


# (B, S, K, hop, tau): the last one puts every p on an integer, so that the two difference points lie on either side of it
ADJ = [(2, 70, 4, 16, None), (1, 45, 1, 16, None), (2, 60, 6, 16, None), (1, 40, 2, 16, np.array([[2.0, 2.0]])),
       (1, 40, 3, 16, np.array([[3.0, 7.0, 1.0]]))]


@pytest.mark.parametrize("case", ADJ, ids=[f"{c[0]}-{c[1]}-{c[2]}-{c[3]}-{'int' if c[4] is not None else 'rnd'}" for c in ADJ])
def test_adjoint_against_central_differences(case):
    """loss = sum gy y.  It is linear in s: gs is compared with the exact difference quotient.  In tau the central difference
    at step e carries e^2 / 6 |d^3 y / d tau^3| <= e^2 / 6 * 40 sum |s| over the taps, and the rounding of the two losses."""
    B, S, K, hop, tau = case
    rng = np.random.default_rng([B, S, K, hop])
    s = rng.standard_normal((B, S))
    gy = rng.standard_normal((B, S))
    if tau is None:
        tau = np.abs(np.cumsum(rng.uniform(-0.5 * hop, 0.5 * hop, (B, K)), 1))
    loss = lambda ss, tt: float((gy * DL.forward(ss, tt, hop)["y"]).sum())
    b = DL.backward(gy, s, tau, hop)
    f = DL.forward(s, tau, hop)
    lmag = float((np.abs(gy) * f["mag"]).sum())
    for bb, j in ((0, 0), (B - 1, S // 2), (0, S - 1)):
        ds = np.zeros_like(s)
        ds[bb, j] = 1.0
        assert abs((loss(s + ds, tau) - loss(s - ds, tau)) / 2 - b["gs"][bb, j]) < 64 * DL.U64 * (lmag + np.abs(gy).sum())
    e = 1e-5
    Hk = DL.hat(K, hop, S)
    sabs = np.abs(s).sum(1)                                                               # (above the taps' own sum)
    for bb in range(B):
        for k in range(K):
            dt = np.zeros_like(tau)
            dt[bb, k] = e
            cd = (loss(s, tau + dt) - loss(s, tau - dt)) / (2 * e)
            tol = e * e * 40 / 6 * float((Hk[k] * np.abs(gy[bb])).sum()) * sabs[bb] + 8 * DL.U64 * lmag / e
            assert abs(cd - b["gtau"][bb, k]) <= tol, (bb, k, cd, b["gtau"][bb, k], tol)
    assert np.abs(b["gtau"]).max() > 0


def test_a_frame_that_no_sample_touches_gets_exactly_zero():
    rng = np.random.default_rng(3)
    S, hop, K = 40, 16, 6                                                                 # frames_needed = 4
    assert DL.frames_needed(S, hop) == 4 and DL.frames_needed(33, 16) == 3 and DL.frames_needed(34, 16) == 4
    b = DL.backward(rng.standard_normal((1, S)), rng.standard_normal((1, S)), np.full((1, K), 2.5), hop)
    assert not b["gtau"][:, 4:].any() and not b["gtau_bound"][:, 4:].any() and b["gtau"][:, :4].all()


def test_passband_error():
    """The 16 taps delay a low tone far better than a high one, and the grid's slack for what lies between its points is small."""
    lo, hi = DL.passband_error(0.05), DL.passband_error(0.3)
    assert 0 < lo < hi < 0.1, (lo, hi)
    fine = DL.passband_error(0.3, grid=65537)
    assert fine <= hi <= 1.01 * fine                                                      # the grid's own slack is small


def test_inputs_respect_the_preconditions():
    for case in DL.CASES:
        s, tau, gy = DL.inputs(case)
        B, S, K, hop, _ = case
        assert s.shape == gy.shape == (B, S) and tau.shape == (B, K) and s.dtype == np.float32 and tau.dtype == np.float64
    assert {c[1] for c in DL.CASES} == {1, R, 2 * R - 1, DL.TILE - 1, DL.TILE, DL.TILE + 1, 2 * DL.TILE + R + 3}
