"""The sequential point-cloud reference of tests/_spec_points_ref.py against the repository's ``spec2point`` on CPU
tensors, and the reference's own properties - no device.

torch's CPU ``index_put`` (non-accumulating) walks its indices in order, so on every input here, the collision inputs
included, it is last-wins and equals the sequential loop: no input is excluded from the comparison."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _spec_points_ref as ref  # noqa: E402

from diffsound_amd.ddsp.mss_loss import spec2point  # noqa: E402
from diffsound_amd.ddsp.spec_points import collapse_expanded  # noqa: E402


def _torch_clouds(P, fclip, freq, sr):
    Pt = torch.from_numpy(P)
    e = ref.EPS
    logspec = ((Pt[:, :fclip] + e).log2() - np.log2(e)) / 40
    f = None if freq is None else torch.from_numpy(np.ascontiguousarray(freq))
    return spec2point(Pt, f, sr).numpy(), spec2point(logspec, f, sr).numpy()


def _check_against_torch(P, fclip, freq, sr):
    want = ref.clouds(P, ref.EPS, fclip, freq, sr)
    lin, log = _torch_clouds(P, fclip, freq, sr)
    bound = dict(zip(("lin", "log"), ref.bound_features(P, ref.EPS, fclip)))
    for got, name in ((lin, "lin"), (log, "log")):
        w = want[name]
        assert np.array_equal(got[..., 3], w[..., 3].astype(np.float32)), name
        # features: torch's CPU kernels perform the fp32 operations the bound counts (their log2 is within its allowance)
        assert (np.abs(got[..., :3] - w[..., :3]) <= bound[name]).all(), name


@pytest.mark.parametrize("T", ref.TS)
@pytest.mark.parametrize("scale", ref.SCALES)
def test_reference_equals_spec2point_without_freq(T, scale):
    _check_against_torch(ref.spectrogram(T), int(ref.F * scale), None, None)


@pytest.mark.parametrize("sr", ref.SAMPLE_RATES)
@pytest.mark.parametrize("scale", ref.SCALES)
def test_reference_equals_spec2point_with_freq(sr, scale):
    """Every frequency case, collisions included (CPU index_put is sequential), except the non-finite one: ``.long()`` of
    NaN or inf is undefined in torch; the reference and the kernel define that such entries write nothing."""
    P = ref.spectrogram(3)
    fclip = int(ref.F * scale)
    collided = 0
    for name, freq in ref.freq_cases(sr).items():
        if name == "nonfinite":
            continue
        collided += ref.has_collisions(ref.F, freq, sr) or ref.has_collisions(fclip, freq, sr)
        _check_against_torch(P, fclip, freq, sr)
    assert collided >= 2  # same_bin and dense_tv do collide


def test_collision_flags():
    sr = 32000
    c = ref.freq_cases(sr)
    assert not ref.has_collisions(ref.F, c["separated"], sr) and not ref.has_collisions(16, c["separated"], sr)
    assert ref.has_collisions(ref.F, c["same_bin"], sr)
    assert not ref.has_collisions(ref.F, c["overlap"], sr)  # its rows are shared between DIFFERENT writes: ordered in torch too
    assert ref.has_collisions(ref.F, c["dense_tv"], sr)
    ex = np.broadcast_to(ref.expanded_base(sr), ref.EXPANDED_SHAPE)
    assert ref.has_collisions(ref.F, ex, sr)  # 16.2 and 16.6 share a bin


@pytest.mark.parametrize("sr", ref.SAMPLE_RATES)
def test_collapsing_expanded_dimensions_changes_nothing(sr):
    """An (A, m, S) expanded view and its (1, m, 1) base give the same clouds and winners up to the flat index's
    renumbering; a view expanded along the middle dimension only keeps the order of the dense ones."""
    base = torch.from_numpy(ref.expanded_base(sr))
    view = base.expand(*ref.EXPANDED_SHAPE)
    col = collapse_expanded(view)
    assert col.shape == base.shape and col.data_ptr() == base.data_ptr()
    for bins in (33, 16):
        a, wa = ref.positions(bins, view.numpy(), sr)
        b, wb = ref.positions(bins, col.numpy(), sr)
        assert np.array_equal(a, b)
        A, m, S = ref.EXPANDED_SHAPE
        own = wa[:, 1] >= 0
        assert np.array_equal(wa[own, 0], wb[own, 0]) and np.array_equal((wa[own, 1] // S) % m, wb[own, 1])
        assert np.array_equal(wa[~own], wb[~own])
    dense = torch.from_numpy(ref.freq_cases(sr)["dense_tv"])       # (2, 3, 40)
    mid = dense[:, :1, :].expand(2, 3, 40)                           # stride 0 along the middle dimension
    cm = collapse_expanded(mid)
    assert cm.shape == (2, 1, 40)
    for bins in (33, 16):
        assert np.array_equal(ref.positions(bins, mid.numpy(), sr)[0], ref.positions(bins, cm.numpy(), sr)[0])
    assert collapse_expanded(dense) is dense


def test_truncation_is_toward_zero_and_bounds_are_half_open():
    sr, bins = 32000, 33
    c = float(ref.coefficient(bins, sr))
    f = np.array([1.5 / c, 0.4 / c, (bins - 2.0) / c], dtype=np.float32)
    cur, row = ref.candidates(bins, f, sr)
    assert -1 < cur[0, 0] < 0 and row[0, 0] == 0            # 1.5 - 2 = -0.5 lands in row 0
    assert cur[0, 1] < -1 and row[0, 1] == -1               # 0.4 - 2 = -1.6 writes nothing
    assert -1 < cur[2, 1] < 0 and row[2, 1] == 0            # 0.4 - 1 = -0.6 lands in row 0
    assert cur[1, 2] == bins and row[1, 2] == -1            # (bins - 2) + 2 = bins: outside
    assert row[3, 2] == bins - 1                            # (bins - 2) + 1 = bins - 1: the last row
    nf = np.array([np.nan, np.inf, -np.inf], dtype=np.float32)
    assert (ref.candidates(bins, nf, sr)[1] == -1).all()
    col, win = ref.positions(bins, nf, sr)
    assert (win == -1).all() and np.array_equal(col, (np.arange(bins, dtype=np.float32) / np.float32(bins)))
    # one ulp on either side of an integer: different rows
    u = ref.freq_cases(sr)["ulp"]
    cur, row = ref.candidates(bins, u, sr)
    assert row[5, 0] == 6 and row[5, 1] == 7 and row[5, 2] == 7 and cur[5, 0] < 7 <= cur[5, 1]


def test_last_write_wins():
    """Two entries in one bin: the higher flat index owns the w = 0 row; a later round overrides an earlier one."""
    sr, bins = 32000, 33
    f = ref.freq_cases(sr)["same_bin"]  # positions 10.2 and 10.7
    col, win = ref.positions(bins, f, sr)
    assert tuple(win[10]) == (5, 1)
    assert col[10] == (ref.coefficient(bins, sr) * f[1] + np.float32(0)) / np.float32(bins)
    f3 = ref.freq_cases(sr)["overlap"]  # 10.2, 12.9, 11.4: row 12 gets 10.2 + 2 (q 1), 12.9 - 0 and + 0 (q 4, 5), 11.4 + 1 (q 3)
    assert tuple(ref.positions(bins, f3, sr)[1][12]) == (5, 1)
    assert tuple(ref.positions(bins, f3, sr)[1][11]) == (5, 2)  # 11.4's own bin beats 10.2 + 1 and 12.9 - 1


@pytest.mark.parametrize("sr", ref.SAMPLE_RATES)
def test_gradient_against_central_differences(sr):
    """``grad_freq`` against central differences of the fp64 position formula.  The positions keep at least 0.05 bins from
    every integer in both clouds and the step moves them by 1e-4 bins at most, so no entry changes its row; the formula is
    piecewise linear, so the difference quotient is exact up to its own rounding (1e-16 / 1e-4 relative) and what is left is
    the fp32 rounding of c: 2^-24 relative.  Tolerance 1e-6 of the largest gradient."""
    rng = np.random.default_rng(sr)
    posn = np.array([1.3, 4.45, 7.7, 11.15, 15.6, 19.3, 24.4, 29.7, 33.9])  # more than 33 / 16 bins apart: no shared row
    f = ref._at(posn, ref.F, sr)
    assert not ref.has_collisions(33, f, sr) and not ref.has_collisions(16, f, sr)
    for bins in (33, 16):
        p = float(ref.coefficient(bins, sr)) * f.astype(np.float64)
        assert (np.abs(p - np.rint(p)) > 0.05).all()
    G = [rng.standard_normal((ref.B, 33, 4)), rng.standard_normal((ref.B, 16, 4))]
    wins = [ref.positions(33, f, sr)[1], ref.positions(16, f, sr)[1]]
    g = ref.grad_freq(f, sr, wins, G)

    def total(fv):
        return sum((Gc[:, :, 3].sum(0) * ref.positions64(bins, fv, sr)).sum() for Gc, bins in zip(G, (33, 16)))

    h = 1e-4 * (sr // 2) / 33
    fd = np.zeros(len(f))
    for e in range(len(f)):
        d = np.zeros(len(f))
        d[e] = h
        fd[e] = (total(f.astype(np.float64) + d) - total(f.astype(np.float64) - d)) / (2 * h)
    assert np.abs(g).max() > 0
    assert np.abs(g - fd).max() <= 1e-6 * np.abs(fd).max()


@pytest.mark.parametrize("sr", ref.SAMPLE_RATES)
def test_gradient_equals_autograd_through_spec2point(sr):
    """``grad_freq`` against torch's autograd through the repository's ``spec2point`` on CPU tensors, for every frequency
    case (collisions included: every entry of the write that owns a row is credited) and for an expanded view, whose base
    receives the sum over all its copies.  fp32 autograd against the fp64 sum: 1e-5 of the largest gradient."""
    rng = np.random.default_rng(sr + 1)
    P = torch.from_numpy(ref.spectrogram(3))
    G = [rng.standard_normal((ref.B, n, 4)).astype(np.float32) for n in (33, 16)]
    cases = {k: v for k, v in ref.freq_cases(sr).items() if k != "nonfinite"}
    cases["expanded"] = np.broadcast_to(ref.expanded_base(sr), ref.EXPANDED_SHAPE)
    for name, fnp in cases.items():
        f = torch.from_numpy(np.ascontiguousarray(fnp)).requires_grad_(True)
        total = (spec2point(P, f, sr) * torch.from_numpy(G[0])).sum() + (spec2point(P[:, :16], f, sr) * torch.from_numpy(G[1])).sum()
        total.backward()
        wins = [ref.positions(33, fnp, sr)[1], ref.positions(16, fnp, sr)[1]]
        g = ref.grad_freq(fnp, sr, wins, G).reshape(fnp.shape)
        assert np.abs(g).max() > 0, name
        assert np.abs(f.grad.numpy() - g).max() <= 1e-5 * np.abs(g).max(), name


def test_feature_bound_is_small_and_positive():
    """The derived bound is a few ulp of the row for the linear cloud and at most a few 1e-6 for the log cloud (values up to 0.7) - it would see a
    wrong sample index or a logarithm taken after the interpolation (both move values by orders of magnitude more)."""
    for T in ref.TS:
        P = ref.spectrogram(T)
        bl, bg = ref.bound_features(P, ref.EPS, 16)
        fl, fg = ref.features(P, ref.EPS, 16)
        assert (bl > 0).all() and (bg > 0).all()
        assert (bl <= 64 * ref.U32 * P.max(-1, keepdims=True)).all() and bg.max() < 5e-6
        if T == 17:  # (no output sits on a sample) the log of the interpolated P is far outside the interpolated log's bound
            wrong = ref.log_feature(fl[:, :16], ref.EPS)
            assert (np.abs(wrong - fg) > bg).mean() > 0.5
