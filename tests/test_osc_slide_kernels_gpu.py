"""The kernels of diffsound_amd/csrc/osc_slide.hip behind ds_osc_slide_fwd / ds_osc_slide_bwd, element by element against
the direct-convolution references of tests/_osc_slide_ref.py at the bounds derived there (tests/test_osc_slide_ref_cpu.py
anchors both without a GPU).

Every output and both workspaces (sized exactly to ds_osc_slide_workspace_bytes) live inside NaN-filled guard zones; each
case is run twice and every output and workspace must come out with the same bits.  Each case prints its largest
error / bound ratio per output (``pytest -s``)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _osc_slide_ref as SL  # noqa: E402
from _guarded import Guarded, _lib, _ratio, _up, same_bits as _same_bits  # noqa: E402

pytestmark = pytest.mark.gpu

SR = SL.SR
IDS = [SL.case_id(c) for c in SL.CASES]


def _call(case, inputs, with_ggain=True):
    """One forward and one backward call, each with its own workspace, on fresh guarded buffers."""
    _hip, L = _lib()
    A, m, F, S, K, hop = case[:6]
    d, w, amp, force, gain, gy = inputs
    p = _hip.ptr
    d_d, d_w, d_amp, d_force, d_gain, d_gy = map(_up, (d, w, amp, force, gain, gy))
    nbytes = L.ds_osc_slide_workspace_bytes(A, m, S, K, hop)
    assert nbytes == 16 * (A * m * SL.ntiles(S) + A * m)
    out = dict(fwork=Guarded((nbytes // 8,), torch.float64), bwork=Guarded((nbytes // 8,), torch.float64),
               y=Guarded((A, S)), gforce=Guarded((A, F)), gd=Guarded((m,), torch.float64), gw=Guarded((m,), torch.float64),
               ggain=Guarded((A, m, K)))
    if amp is not None:
        out["gamp"] = Guarded((A, m))
    _hip.check(L.ds_osc_slide_fwd(p(d_d), p(d_w), p(d_amp), p(d_force), p(d_gain), A, m, F, S, K, hop, SR, out["fwork"].ptr,
                                  nbytes, out["y"].ptr, _hip.stream_ptr()), "ds_osc_slide_fwd")
    _hip.check(L.ds_osc_slide_bwd(p(d_gy), p(d_d), p(d_w), p(d_amp), p(d_force), p(d_gain), A, m, F, S, K, hop, SR,
                                  out["bwork"].ptr, nbytes, out["gd"].ptr, out["gw"].ptr,
                                  out["gamp"].ptr if amp is not None else None, out["gforce"].ptr,
                                  out["ggain"].ptr if with_ggain else None, _hip.stream_ptr()), "ds_osc_slide_bwd")
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def _run(case):
    inputs = SL.inputs(case)
    return inputs, _call(case, inputs), _call(case, inputs)


@pytest.mark.parametrize("case", SL.CASES, ids=IDS)
def test_forward(case):
    A, m, F, S, K, hop = case[:6]
    (d, w, amp, force, gain, gy), out, again = _run(case)
    out["y"].check("y")
    nstate = 2 * A * m * SL.ntiles(S)
    whole = out["fwork"].buf.cpu().numpy()
    assert np.isfinite(out["fwork"].numpy()[:nstate]).all() and np.isnan(out["fwork"].numpy()[nstate:]).all()
    assert np.isnan(whole[:64]).all() and np.isnan(whole[-64:]).all(), "workspace: written outside"
    assert _same_bits(out["y"], again["y"]) and _same_bits(out["fwork"], again["fwork"])
    y_ref, Y = SL.forward(d, w, amp, force, gain, hop, S)
    assert _ratio("sld.y", case, out["y"].numpy(), y_ref, SL.bound32(y_ref, Y, A, m, S)) <= 1.0


@pytest.mark.parametrize("case", SL.CASES, ids=IDS)
def test_backward(case):
    A, m, F, S, K, hop = case[:6]
    (d, w, amp, force, gain, gy), out, again = _run(case)
    for k in ("bwork", "gforce", "ggain", "gd", "gw", "gamp"):
        if k in out:
            out[k].check(k)
            assert _same_bits(out[k], again[k]), k
    b = SL.backward(gy, d, w, amp, force, gain, hop)
    gf, gg = out["gforce"].numpy(), out["ggain"].numpy()
    assert not gf[:, S:].any(), "taps no sample hears must get exactly 0"
    assert not gg[:, :, SL.frames_needed(S, F, hop):].any(), "frames no driven sample touches must get exactly 0"
    assert _ratio("sld.gforce", case, gf, b["gforce"], SL.bound32(b["gforce"], b["Eg"], A, m, S)) <= 1.0
    assert _ratio("sld.ggain", case, gg, b["ggain"], SL.bound32(b["ggain"], b["Vg"], A, m, S)) <= 1.0
    assert _ratio("sld.gd", case, out["gd"].numpy(), b["gd"], SL.bound_gd_gw(b["W"], A, m, S)) <= 1.0
    assert _ratio("sld.gw", case, out["gw"].numpy(), b["gw"], SL.bound_gd_gw(b["W"], A, m, S)) <= 1.0
    if amp is not None:
        assert _ratio("sld.gamp", case, out["gamp"].numpy(), b["gamp"], SL.bound32(b["gamp"], b["V"], A, m, S)) <= 1.0


def test_backward_without_ggain_leaves_it_alone():
    """ggain = NULL: nothing is computed for it, and every other output has the bits of the call with it."""
    case = SL.CASES[11]
    inputs, out, _ = _run(case)
    bare = _call(case, inputs, with_ggain=False)
    assert bare["ggain"].untouched()
    for k in ("gforce", "gd", "gw", "bwork"):
        bare[k].check(k)
        assert _same_bits(bare[k], out[k]), k


def test_unit_gains_give_the_driven_bank_within_both_bounds():
    import _osc_driven_ref as D

    _hip, L = _lib()
    case = (3, 5, 513, SL.TILE + 1, 3, 48, "material", True)
    A, m, F, S, K, hop = case[:6]
    d, w, amp, force, _, gy = SL.inputs(case)
    ones = np.ones((A, m, K), dtype=np.float32)
    out = _call(case, (d, w, amp, force, ones, gy))
    y_ref, E = D.forward(d, w, amp, force, S)
    assert _ratio("sld.unit.y", case, out["y"].numpy(), y_ref, SL.bound32(y_ref, E, A, m, S)) <= 1.0  # (unit gains: Ymag = E)


def test_workspace_bytes():
    _, L = _lib()
    for a in [(0, 1, 1, 1, 16), (1, 0, 1, 1, 16), (1, 1, 0, 1, 16), (1, 1, 1, 0, 16), (1, 1, 1, 1, 0), (1, 1, 1, 1, 24),
              (1, 1, 1, 1, -16)]:
        assert L.ds_osc_slide_workspace_bytes(*a) == 0
    for A, m, S in [(1, 1, 1), (2, 17, SL.TILE + 1), (8, 64, 8000), (65535, 64, 2 ** 20)]:
        assert L.ds_osc_slide_workspace_bytes(A, m, S, 3, 48) == 16 * (A * m * SL.ntiles(S) + A * m)
