"""tests/_osc_driven_ref.py without a GPU: the recurrence the kernels of csrc/osc_driven.hip run is the convolution the
references evaluate, the reference gradients are the autograd gradients of that convolution, a CPU model of the kernels'
roundings stays inside the bounds, and a model with one rounding too many does not."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _osc_driven_ref as D  # noqa: E402
import _osc_ref as R  # noqa: E402

IDS = [D.case_id(c) for c in D.CASES]


@functools.lru_cache(maxsize=None)
def _refs(case):
    d, w, amp, force, gy = D.inputs(case)
    S = case[3]
    y, Emag = D.forward(d, w, amp, force, S)
    b = D.backward(gy, d, w, amp, force)
    for a in (y, Emag, *b.values()):
        a.setflags(write=False)
    return y, Emag, b


def _worst(got, ref, bound):
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    r = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))
    return float(r.max())


@pytest.mark.parametrize("case", D.CASES, ids=IDS)
def test_recurrence_is_the_convolution(case):
    """x[t] = z (x[t-1] + f[t]) in complex128 against the direct convolution of the closed-form mode signals: 1e-11 of
    the magnitudes entering each sample, and 1e-11 of the largest sample in the max norm; the adjoint recurrence against
    the explicit sum for gforce likewise."""
    A, m, F, S = case[:4]
    d, w, amp, force, gy = D.inputs(case)
    y, Emag, b = _refs(case)
    rec = D.recurrence(d, w, amp, force, S)
    assert np.all(np.abs(rec - y) <= 1e-11 * Emag)
    assert np.abs(rec - y).max() <= 1e-11 * np.abs(y).max()
    gf = np.zeros((A, F))
    n = min(F, S)
    gf[:, :n] = D.recurrence(d, w, amp, gy, S, reverse=True)[:, :n]
    assert np.all(np.abs(gf - b["gforce"]) <= 1e-11 * b["Eg"])
    assert np.abs(gf - b["gforce"]).max() <= 1e-11 * np.abs(b["gforce"]).max()
    assert not b["gforce"][:, n:].any()


@pytest.mark.parametrize("case", D.CASES, ids=IDS)
def test_reference_gradients_are_autograd_of_the_convolution(case):
    A, m, F, S = case[:4]
    d, w, amp, force, gy = D.inputs(case)
    _, _, b = _refs(case)
    leaf = lambda x: None if x is None else torch.from_numpy(np.asarray(x)).double().requires_grad_(True)
    t_d, t_w, t_a, t_f = leaf(d), leaf(w), leaf(amp), leaf(force)
    y = R.torch_bank_chain(t_d, t_w, t_a, t_f, S, D.SR)
    (y * torch.from_numpy(gy).double()).sum().backward()
    pairs = [("gforce", t_f), ("gd", t_d), ("gw", t_w)] + ([("gamp", t_a)] if amp is not None else [])
    for name, t in pairs:
        got, ref = t.grad.numpy(), b[name]
        assert np.abs(got - ref).max() <= 1e-9 * max(np.abs(ref).max(), 1e-300), name


@pytest.mark.parametrize("case", D.CASES, ids=IDS)
def test_model_of_the_kernel_roundings_is_inside_the_bounds(case):
    A, m, F, S = case[:4]
    d, w, amp, force, gy = D.inputs(case)
    y, Emag, b = _refs(case)
    model = D.recurrence(d, w, amp, force, S, store32=True)
    assert _worst(model, y, D.bound_y(y, Emag, A, m, S)) <= 1.0
    n = min(F, S)
    gf = D.recurrence(d, w, amp, gy, S, reverse=True, store32=True)[:, :n]
    assert _worst(gf, b["gforce"][:, :n], D.bound_gforce(b["gforce"], b["Eg"], A, m, S)[:, :n]) <= 1.0


def test_a_state_rounded_to_fp32_at_tile_boundaries_is_outside_the_bounds():
    """The bounds tell a kernel that keeps its carried state in fp32 from one that keeps it in fp64: the same model with
    the state rounded once per tile boundary exceeds them somewhere in y on every case with more than one tile whose
    modes still ring at the boundary, and somewhere in gforce where the force reaches past a tile."""
    seen = 0
    for case in D.CASES:
        A, m, F, S, modes = case[:5]
        if S <= D.TILE or modes == "underflow":
            continue
        d, w, amp, force, gy = D.inputs(case)
        y, Emag, b = _refs(case)
        wrong = D.recurrence(d, w, amp, force, S, round_state_at_tiles=True, store32=True)
        assert _worst(wrong, y, D.bound_y(y, Emag, A, m, S)) > 1.0, case
        n = min(F, S)
        if n <= D.TILE:  # gforce has no tap beyond the first boundary the adjoint state crosses with weight
            continue
        wrong = D.recurrence(d, w, amp, gy, S, reverse=True, round_state_at_tiles=True, store32=True)[:, :n]
        assert _worst(wrong, b["gforce"][:, :n], D.bound_gforce(b["gforce"], b["Eg"], A, m, S)[:, :n]) > 1.0, case
        seen += 1
    assert seen >= 2


def test_case_list_covers_every_boundary():
    T, Rn = D.TILE, D.RUN
    assert {c[3] for c in D.CASES} == {1, 63, 64, 65, T - 1, T, T + 1, 2 * T + Rn + 1}
    assert {c[1] for c in D.CASES} == {1, 3, 4, 5, 17} and {c[0] for c in D.CASES} == {1, 3}
    assert {c[4] for c in D.CASES} == set(D.MODE_SETS) and {c[5] for c in D.CASES} == set(D.FORCES)
    assert {c[2] for c in D.CASES} >= {1, 2, 512, 513}
    assert {c[2] - c[3] for c in D.CASES} >= {-1, 0, 7}
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")  # the kernels' constants: osc_scan.h, from the public header
    src = open(os.path.join(root, "diffsound_amd", "csrc", "osc_scan.h")).read()
    assert "constexpr int RUN = DS_OSC_SCAN_RUN;" in src and "constexpr int TILE = 64 * RUN;" in src
    assert f"#define DS_OSC_SCAN_RUN {Rn} " in open(os.path.join(root, "include", "diffsound_hip.h")).read()
    driven = open(os.path.join(root, "diffsound_amd", "csrc", "osc_driven.hip")).read()
    assert "constexpr int RUN" not in driven and "constexpr int TILE" not in driven and "using namespace osc_scan;" in driven
