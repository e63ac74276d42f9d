"""tests/_osc_slide_ref.py without a GPU: the reference gradients are the central differences of the reference forward, the
degenerate cases reduce to the driven bank's reference, the sliding bank is the sum of K driven banks (linearity), the
recurrence the kernels of csrc/osc_slide.hip run is the convolution the references evaluate, a CPU model of the kernels'
roundings stays inside the bounds and one with a rounding too many does not."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _osc_driven_ref as D  # noqa: E402
import _osc_slide_ref as SL  # noqa: E402

IDS = [SL.case_id(c) for c in SL.CASES]
SMALL = (2, 3, 37, 40, 3, 16, "material", True)   # the last frame held from sample 32 on
SMALL_FS = (2, 3, 50, 40, 4, 16, "material", False)


@functools.lru_cache(maxsize=None)
def _refs(case):
    d, w, amp, force, gain, gy = SL.inputs(case)
    S, hop = case[3], case[5]
    y, Y = SL.forward(d, w, amp, force, gain, hop, S)
    b = SL.backward(gy, d, w, amp, force, gain, hop)
    for a in (y, Y, *b.values()):
        a.setflags(write=False)
    return y, Y, b


def _worst(got, ref, bound):
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    r = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))
    return float(r.max())


@pytest.mark.parametrize("case", [SMALL, SMALL_FS], ids=SL.case_id)
def test_reference_gradients_are_central_differences(case):
    """d / dp of sum(gy y) for every element p of d, w, amp, force and gain: central differences of ``forward`` at a step
    of 1e-6 |p| + 1e-7 agree with ``backward`` to 1e-6 of the largest entry of that gradient (the differences' own
    truncation and cancellation error at these steps is ~1e-8 relative)."""
    A, m, F, S, K, hop = case[:6]
    d, w, amp, force, gain, gy = SL.inputs(case)
    ops = dict(d=d.copy(), w=w.copy(), amp=None if amp is None else amp.astype(np.float64), force=force.astype(np.float64),
               gain=gain.astype(np.float64))
    b = SL.backward(gy, d, w, amp, force, gain, hop)
    loss = lambda: float((gy * SL.forward(ops["d"], ops["w"], ops["amp"], ops["force"], ops["gain"], hop, S)[0]).sum())
    for name, key in (("d", "gd"), ("w", "gw"), ("amp", "gamp"), ("force", "gforce"), ("gain", "ggain")):
        x = ops[name]
        if x is None:
            continue
        fd = np.zeros(x.size)
        flat = x.reshape(-1)
        for i in range(x.size):
            keep = flat[i]
            h = 1e-6 * abs(keep) + 1e-7
            flat[i] = keep + h
            up = loss()
            flat[i] = keep - h
            dn = loss()
            flat[i] = keep
            fd[i] = (up - dn) / (2 * h)
        ref = b[key].reshape(-1)
        assert np.abs(fd - ref).max() <= 1e-6 * np.abs(ref).max(), name
    assert not b["gforce"][:, S:].any()


def test_one_frame_is_the_driven_bank_with_the_gain_folded_into_amp():
    case = (2, 4, 70, 90, 1, 32, "material", True)
    d, w, amp, force, gain, gy = SL.inputs(case)
    y, _ = SL.forward(d, w, amp, force, gain, 32, 90)
    y_drv, E = D.forward(d, w, amp.astype(np.float64) * gain[:, :, 0], force, 90)
    assert np.all(np.abs(y - y_drv) <= 1e-13 * E + 1e-300)
    b, bd = SL.backward(gy, d, w, amp, force, gain, 32), D.backward(gy, d, w, amp.astype(np.float64) * gain[:, :, 0], force)
    for k in ("gd", "gw"):
        assert np.abs(b[k] - bd[k]).max() <= 1e-12 * np.abs(bd[k]).max()


@pytest.mark.parametrize("K,hop", [(1, 16), (4, 16), (2, 1024)])
def test_unit_gains_reproduce_the_driven_bank(K, hop):
    case = (2, 4, 70, 90, K, hop, "material", True)
    d, w, amp, force, _, gy = SL.inputs(case)
    ones = np.ones((2, 4, K), dtype=np.float32)
    y, Y = SL.forward(d, w, amp, force, ones, hop, 90)
    y_drv, E = D.forward(d, w, amp, force, 90)
    assert np.all(np.abs(y - y_drv) <= 1e-13 * E) and np.all(np.abs(Y - E) <= 1e-13 * E)
    b, bd = SL.backward(gy, d, w, amp, force, ones, hop), D.backward(gy, d, w, amp, force)
    for k in ("gforce", "gamp", "gd", "gw"):
        assert np.abs(b[k] - bd[k]).max() <= 1e-12 * np.abs(bd[k]).max(), k


def test_linearity_sliding_is_the_sum_of_one_driven_bank_per_frame():
    """sliding(gain) = sum_k driven(hat_k f, amp gain_k)."""
    case = (2, 4, 70, 90, 5, 16, "material", True)
    A, m, F, S, K, hop = case[:6]
    d, w, amp, force, gain, _ = SL.inputs(case)
    y, Y = SL.forward(d, w, amp, force, gain, hop, S)
    H = SL.hat(K, hop, F)
    total = np.zeros_like(y)
    for k in range(K):
        total += D.forward(d, w, amp.astype(np.float64) * gain[:, :, k], force.astype(np.float64) * H[k][None, :], S)[0]
    assert np.all(np.abs(total - y) <= 1e-13 * Y + 1e-300)
    assert np.allclose(H.sum(0), 1.0, rtol=0, atol=1e-15) and (H >= 0).all()


@pytest.mark.parametrize("case", SL.CASES, ids=IDS)
def test_recurrence_is_the_convolution(case):
    A, m, F, S, K, hop = case[:6]
    d, w, amp, force, gain, gy = SL.inputs(case)
    y, Y, b = _refs(case)
    assert np.all(np.abs(SL.recurrence(d, w, amp, force, gain, hop, S) - y) <= 1e-11 * Y)
    gf, gg = SL.adjoint_recurrence(gy, d, w, amp, force, gain, hop)
    assert np.all(np.abs(gf - b["gforce"]) <= 1e-11 * b["Eg"])
    assert np.all(np.abs(gg - b["ggain"]) <= 1e-11 * b["Vg"])
    untouched = SL.frames_needed(S, F, hop)
    assert not b["ggain"][:, :, untouched:].any() and not b["Vg"][:, :, untouched:].any()


@pytest.mark.parametrize("case", SL.CASES, ids=IDS)
def test_model_of_the_kernel_roundings_is_inside_the_bounds(case):
    A, m, F, S, K, hop = case[:6]
    d, w, amp, force, gain, gy = SL.inputs(case)
    y, Y, b = _refs(case)
    assert _worst(SL.recurrence(d, w, amp, force, gain, hop, S, store32=True), y, SL.bound32(y, Y, A, m, S)) <= 1.0
    gf, gg = SL.adjoint_recurrence(gy, d, w, amp, force, gain, hop, store32=True)
    assert _worst(gf, b["gforce"], SL.bound32(b["gforce"], b["Eg"], A, m, S)) <= 1.0
    assert _worst(gg, b["ggain"], SL.bound32(b["ggain"], b["Vg"], A, m, S)) <= 1.0


def test_a_state_rounded_to_fp32_at_tile_boundaries_is_outside_the_bounds():
    """As for the driven bank: the same model with the states rounded once per tile boundary exceeds the bound on y on every
    case with a full tile behind a boundary, a force that reaches the boundary and modes that still ring there."""
    seen = 0
    for case in SL.CASES:
        A, m, F, S, K, hop, modes = case[:7]
        if S < 2 * SL.TILE or min(F, S) < SL.TILE or modes == "underflow":
            continue
        d, w, amp, force, gain, gy = SL.inputs(case)
        y, Y, _ = _refs(case)
        wrong = SL.recurrence(d, w, amp, force, gain, hop, S, store32=True, round_state_at_tiles=True)
        assert _worst(wrong, y, SL.bound32(y, Y, A, m, S)) > 1.0, case
        seen += 1
    assert seen >= 4


def test_case_list_covers_every_boundary():
    T, Rn = SL.TILE, SL.RUN
    C = SL.CASES
    assert {1, 15, 16, 17, T - 1, T, T + 1, 2 * T + Rn + 1} <= {c[3] for c in C}
    assert any(c[3] == c[5] for c in C) and any(c[3] == c[5] + 1 for c in C)
    assert {16, 48, 1024, 1040} <= {c[5] for c in C} and any(c[5] > c[3] for c in C)
    assert all(c[5] % Rn == 0 for c in C)
    need = [SL.frames_needed(c[3], c[2], c[5]) for c in C]
    assert any(c[4] == 1 for c in C) and any(c[4] == e for c, e in zip(C, need))
    assert any(c[4] == e - 1 and c[4] > 1 for c, e in zip(C, need)) and any(c[4] >= e + 3 for c, e in zip(C, need))
    assert {c[2] - c[3] for c in C} >= {-1, 0, 7} and any(c[2] == 1 for c in C)
    assert {c[1] for c in C} == {1, 5, 70} and {c[0] for c in C} == {1, 3}
    assert {c[6] for c in C} == set(SL.MODE_SETS)
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    assert "#define DS_OSC_SCAN_RUN %d" % Rn in open(os.path.join(root, "include", "diffsound_hip.h")).read()
    assert "constexpr int TILE = 64 * RUN;" in open(os.path.join(root, "diffsound_amd", "csrc", "osc_scan.h")).read()
