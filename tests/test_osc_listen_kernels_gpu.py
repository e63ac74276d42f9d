"""The kernels of diffsound_amd/csrc/osc_listen.hip behind ds_osc_listen_fwd / ds_osc_listen_bwd, element by element against
the direct-convolution references of tests/_osc_listen_ref.py at the bounds derived there (tests/test_osc_listen_ref_cpu.py
anchors both without a GPU).

Every output and both workspaces (sized exactly to ds_osc_listen_workspace_bytes) live inside NaN-filled guard zones; each
case is run twice and every output and workspace must come out with the same bits.  Each case prints its largest
error / bound ratio per output (``pytest -s``)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _osc_listen_ref as LS  # noqa: E402
from _guarded import Guarded, _lib, _ratio, _up, same_bits as _same_bits  # noqa: E402

pytestmark = pytest.mark.gpu

SR = LS.SR
IDS = [LS.case_id(c) for c in LS.CASES]


def _call(case, inputs, with_gh=True, with_gforce=True):
    """One forward and one backward call, each with its own workspace, on fresh guarded buffers."""
    _hip, L = _lib()
    A, C, m, F, S, K, hop = case[:7]
    d, w, amp, force, h, gy = inputs
    p = _hip.ptr
    d_d, d_w, d_amp, d_force, d_h, d_gy = map(_up, (d, w, amp, force, h, gy))
    nbytes = L.ds_osc_listen_workspace_bytes(A, C, m, S, K, hop)
    assert nbytes == 16 * (A * m * LS.ntiles(S) + A * m)
    out = dict(fwork=Guarded((nbytes // 8,), torch.float64), bwork=Guarded((nbytes // 8,), torch.float64),
               y=Guarded((A, C, S)), gforce=Guarded((A, F)), gd=Guarded((m,), torch.float64), gw=Guarded((m,), torch.float64),
               gh=Guarded((A, C, m, K, 2)))
    if amp is not None:
        out["gamp"] = Guarded((A, m))
    _hip.check(L.ds_osc_listen_fwd(p(d_d), p(d_w), p(d_amp), p(d_force), p(d_h), A, C, m, F, S, K, hop, SR, out["fwork"].ptr,
                                   nbytes, out["y"].ptr, _hip.stream_ptr()), "ds_osc_listen_fwd")
    _hip.check(L.ds_osc_listen_bwd(p(d_gy), p(d_d), p(d_w), p(d_amp), p(d_force), p(d_h), A, C, m, F, S, K, hop, SR,
                                   out["bwork"].ptr, nbytes, out["gd"].ptr, out["gw"].ptr,
                                   out["gamp"].ptr if amp is not None else None, out["gforce"].ptr if with_gforce else None,
                                   out["gh"].ptr if with_gh else None, _hip.stream_ptr()), "ds_osc_listen_bwd")
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def _run(case):
    inputs = LS.inputs(case)
    return inputs, _call(case, inputs), _call(case, inputs)


@functools.lru_cache(maxsize=None)
def _ref_backward(case):
    d, w, amp, force, h, gy = LS.inputs(case)
    return LS.backward(gy, d, w, amp, force, h, case[6])


@pytest.mark.parametrize("case", LS.CASES, ids=IDS)
def test_forward(case):
    A, C, m, F, S, K, hop = case[:7]
    (d, w, amp, force, h, gy), out, again = _run(case)
    out["y"].check("y")
    nstate = 2 * A * m * LS.ntiles(S)
    whole = out["fwork"].buf.cpu().numpy()
    assert np.isfinite(out["fwork"].numpy()[:nstate]).all() and np.isnan(out["fwork"].numpy()[nstate:]).all()
    assert np.isnan(whole[:64]).all() and np.isnan(whole[-64:]).all(), "workspace: written outside"
    assert _same_bits(out["y"], again["y"]) and _same_bits(out["fwork"], again["fwork"])
    y_ref, Y = LS.forward(d, w, amp, force, h, hop, S)
    assert _ratio("lis.y", case, out["y"].numpy(), y_ref, LS.bound32(y_ref, Y, A, C, m, S)) <= 1.0


@pytest.mark.parametrize("case", LS.CASES, ids=IDS)
def test_backward(case):
    A, C, m, F, S, K, hop = case[:7]
    (d, w, amp, force, h, gy), out, again = _run(case)
    for k in ("bwork", "gforce", "gh", "gd", "gw", "gamp"):
        if k in out:
            out[k].check(k)
            assert _same_bits(out[k], again[k]), k
    b = _ref_backward(case)
    gf, gg = out["gforce"].numpy(), out["gh"].numpy()
    assert not gf[:, S:].any(), "taps no sample hears must get exactly 0"
    assert not gg[:, :, :, LS.frames_needed(S, hop):].any(), "frames no sample touches must get exactly (0, 0)"
    assert _ratio("lis.gforce", case, gf, b["gforce"], LS.bound32(b["gforce"], b["Eg"], A, C, m, S)) <= 1.0
    assert _ratio("lis.gh", case, gg, b["gh"], LS.bound32(b["gh"], b["Vh"], A, C, m, S)) <= 1.0
    assert _ratio("lis.gd", case, out["gd"].numpy(), b["gd"], LS.bound_gd_gw(b["W"], A, C, m, S)) <= 1.0
    assert _ratio("lis.gw", case, out["gw"].numpy(), b["gw"], LS.bound_gd_gw(b["W"], A, C, m, S)) <= 1.0
    if amp is not None:
        assert _ratio("lis.gamp", case, out["gamp"].numpy(), b["gamp"], LS.bound32(b["gamp"], b["V"], A, C, m, S)) <= 1.0


@pytest.mark.parametrize("which", ["gh", "gforce"])
def test_backward_without_an_optional_output_leaves_it_alone(which):
    """gh = NULL or gforce = NULL: nothing is computed for it, and every other output has the bits of the call with it."""
    case = LS.CASES[8]
    inputs, out, _ = _run(case)
    bare = _call(case, inputs, with_gh=which != "gh", with_gforce=which != "gforce")
    assert bare[which].untouched()
    for k in ("gforce", "gh", "gd", "gw", "gamp", "bwork"):
        if k != which:
            bare[k].check(k)
            assert _same_bits(bare[k], out[k]), k


def test_unit_gains_give_the_driven_bank_within_both_bounds():
    import _osc_driven_ref as D

    case = (3, 1, 5, 513, LS.TILE + 1, 1, 16, "material", True)
    A, C, m, F, S, K, hop = case[:7]
    d, w, amp, force, _, gy = LS.inputs(case)
    one = np.zeros((A, C, m, K, 2), dtype=np.float32)
    one[..., 0] = 1.0
    out = _call(case, (d, w, amp, force, one, gy))
    y_ref, E = D.forward(d, w, amp, force, S)
    assert _ratio("lis.unit.y", case, out["y"].numpy()[:, 0], y_ref, LS.bound32(y_ref, E, A, C, m, S)) <= 1.0  # (Ymag = E)
    assert _ratio("lis.unit.y.driven", case, out["y"].numpy()[:, 0], y_ref, D.bound_y(y_ref, E, A, m, S)) <= 1.0
    b = D.backward(gy[:, 0], d, w, amp, force)
    assert _ratio("lis.unit.gforce", case, out["gforce"].numpy(), b["gforce"], D.bound_gforce(b["gforce"], b["Eg"], A, m, S)) <= 1.0
    assert _ratio("lis.unit.gamp", case, out["gamp"].numpy(), b["gamp"], D.bound_gamp(b["gamp"], b["V"], A, m, S)) <= 1.0
    assert _ratio("lis.unit.gd", case, out["gd"].numpy(), b["gd"], D.bound_gd_gw(b["W"], A, m, S)) <= 1.0
    assert _ratio("lis.unit.gw", case, out["gw"].numpy(), b["gw"], D.bound_gd_gw(b["W"], A, m, S)) <= 1.0


def test_two_channels_with_one_gain_give_identical_rows():
    case = (3, 2, 5, 513, LS.TILE + 1, 22, 48, "material", True)
    d, w, amp, force, h, gy = LS.inputs(case)
    h[:, 1] = h[:, 0]
    y = _call(case, (d, w, amp, force, h, gy))["y"].numpy()
    assert np.array_equal(y[:, 0].view(np.uint32), y[:, 1].view(np.uint32))


def test_workspace_bytes():
    _, L = _lib()
    for a in [(0, 1, 1, 1, 1, 16), (1, 0, 1, 1, 1, 16), (1, 17, 1, 1, 1, 16), (1, 1, 0, 1, 1, 16), (1, 1, 1, 0, 1, 16),
              (1, 1, 1, 1, 0, 16), (1, 1, 1, 1, 1, 0), (1, 1, 1, 1, 1, 24), (1, 1, 1, 1, 1, -16)]:
        assert L.ds_osc_listen_workspace_bytes(*a) == 0
    for A, m, S in [(1, 1, 1), (2, 17, LS.TILE + 1), (8, 64, 8000), (65535, 64, 2 ** 20)]:
        for C in (1, 16):
            assert L.ds_osc_listen_workspace_bytes(A, C, m, S, 3, 48) == 16 * (A * m * LS.ntiles(S) + A * m)
