"""The kernels of diffsound_amd/csrc/osc_driven.hip behind ds_osc_driven_fwd / ds_osc_driven_bwd, element by element
against the direct-convolution references of tests/_osc_driven_ref.py at the bounds derived there
(tests/test_osc_driven_ref_cpu.py anchors both without a GPU).

Every output and both workspaces (sized exactly to ds_osc_driven_workspace_bytes) live inside NaN-filled guard zones;
each case is run twice and every output and workspace must come out with the same bits.  Each case prints its largest
error / bound ratio per output (``pytest -s``)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _osc_driven_ref as D  # noqa: E402
from _guarded import Guarded, _lib, _ratio, _up, dev as _dev, same_bits as _same_bits  # noqa: E402

pytestmark = pytest.mark.gpu

SR = D.SR
IDS = [D.case_id(c) for c in D.CASES]


def _call(case, inputs):
    """One forward and one backward call, each with its own workspace, on fresh guarded buffers."""
    _hip, L = _lib()
    A, m, F, S = case[:4]
    d, w, amp, force, gy = inputs
    p = _hip.ptr
    d_d, d_w, d_amp, d_force, d_gy = map(_up, (d, w, amp, force, gy))
    nbytes = L.ds_osc_driven_workspace_bytes(A, m, S)
    assert nbytes == 16 * (A * m * D.ntiles(S) + A * m)
    out = dict(fwork=Guarded((nbytes // 8,), torch.float64), bwork=Guarded((nbytes // 8,), torch.float64),
               y=Guarded((A, S)), gforce=Guarded((A, F)), gd=Guarded((m,), torch.float64), gw=Guarded((m,), torch.float64))
    if amp is not None:
        out["gamp"] = Guarded((A, m))
    _hip.check(L.ds_osc_driven_fwd(p(d_d), p(d_w), p(d_amp), p(d_force), A, m, F, S, SR, out["fwork"].ptr, nbytes,
                                   out["y"].ptr, _hip.stream_ptr()), "ds_osc_driven_fwd")
    _hip.check(L.ds_osc_driven_bwd(p(d_gy), p(d_d), p(d_w), p(d_amp), p(d_force), A, m, F, S, SR, out["bwork"].ptr, nbytes,
                                   out["gd"].ptr, out["gw"].ptr, out["gamp"].ptr if amp is not None else None,
                                   out["gforce"].ptr, _hip.stream_ptr()), "ds_osc_driven_bwd")
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def _run(case):
    inputs = D.inputs(case)
    return inputs, _call(case, inputs), _call(case, inputs)


@pytest.mark.parametrize("case", D.CASES, ids=IDS)
def test_forward(case):
    A, m, F, S = case[:4]
    (d, w, amp, force, gy), out, again = _run(case)
    out["y"].check("y")
    # the forward fills the tile-entry states (2 A m NT doubles); the A m partial sums behind them belong to the backward
    nstate = 2 * A * m * D.ntiles(S)
    whole = out["fwork"].buf.cpu().numpy()
    assert np.isfinite(out["fwork"].numpy()[:nstate]).all() and np.isnan(out["fwork"].numpy()[nstate:]).all()
    assert np.isnan(whole[:64]).all() and np.isnan(whole[-64:]).all(), "workspace: written outside"
    assert _same_bits(out["y"], again["y"]) and _same_bits(out["fwork"], again["fwork"])
    y_ref, Emag = D.forward(d, w, amp, force, S)
    assert _ratio("drv.y", case, out["y"].numpy(), y_ref, D.bound_y(y_ref, Emag, A, m, S)) <= 1.0


@pytest.mark.parametrize("case", D.CASES, ids=IDS)
def test_backward(case):
    A, m, F, S = case[:4]
    (d, w, amp, force, gy), out, again = _run(case)
    for k in ("bwork", "gforce", "gd", "gw", "gamp"):
        if k in out:
            out[k].check(k)
            assert _same_bits(out[k], again[k]), k
    b = D.backward(gy, d, w, amp, force)
    gf = out["gforce"].numpy()
    assert not gf[:, S:].any(), "taps no sample hears must get exactly 0"
    assert _ratio("drv.gforce", case, gf, b["gforce"], D.bound_gforce(b["gforce"], b["Eg"], A, m, S)) <= 1.0
    assert _ratio("drv.gd", case, out["gd"].numpy(), b["gd"], D.bound_gd_gw(b["W"], A, m, S)) <= 1.0
    assert _ratio("drv.gw", case, out["gw"].numpy(), b["gw"], D.bound_gd_gw(b["W"], A, m, S)) <= 1.0
    if amp is not None:
        assert _ratio("drv.gamp", case, out["gamp"].numpy(), b["gamp"], D.bound_gamp(b["gamp"], b["V"], A, m, S)) <= 1.0


def test_backward_without_optional_outputs():
    """gamp = NULL and gforce = NULL: gd and gw are the same bits as with them."""
    _hip, L = _lib()
    case = D.CASES[11]
    A, m, F, S = case[:4]
    (d, w, amp, force, gy), out, _ = _run(case)
    p = _hip.ptr
    nbytes = L.ds_osc_driven_workspace_bytes(A, m, S)
    work, gd, gw = Guarded((nbytes // 8,), torch.float64), Guarded((m,), torch.float64), Guarded((m,), torch.float64)
    d_d, d_w, d_amp, d_force, d_gy = map(_up, (d, w, amp, force, gy))
    _hip.check(L.ds_osc_driven_bwd(p(d_gy), p(d_d), p(d_w), p(d_amp), p(d_force), A, m, F, S, SR, work.ptr, nbytes,
                                   gd.ptr, gw.ptr, None, None, _hip.stream_ptr()), "ds_osc_driven_bwd")
    torch.cuda.synchronize()
    for g in (work, gd, gw):
        g.check("output")
    assert _same_bits(gd, out["gd"]) and _same_bits(gw, out["gw"])


# -------------------------------------------------------------------------------------------------- refusals
_BAD = ["null-d", "null-force", "null-work", "null-out", "A=0", "m=0", "S=0", "F=0", "A=-1", "A=65536", "work-short",
        "work-misaligned", "gd-misaligned", "gw-misaligned"]
_REFUSALS = [(fn, bad) for fn in ("ds_osc_driven_fwd", "ds_osc_driven_bwd") for bad in _BAD
             if not (fn.endswith("fwd") and bad in ("gd-misaligned", "gw-misaligned"))]


@pytest.mark.parametrize("fn,bad", _REFUSALS, ids=[f"{f}-{b}" for f, b in _REFUSALS])
def test_refusals_write_nothing(fn, bad):
    """Arguments outside the limits are rejected before any launch: non-zero status, a message naming the entry point,
    every guarded output and the workspace still NaN.  (The buffers are as large as the largest in-range reading of the
    arguments, so a call that wrongly went ahead would stay inside them.)"""
    _hip, L = _lib()
    dims = dict(A=2, m=3, F=5, S=7)
    if "=" in bad:
        k, v = bad.split("=")
        dims[k] = int(v)
        if k == "A" and int(v) > 2:
            dims.update(m=1, F=1, S=1)
    A, m, F, S = (dims[k] for k in "AmFS")
    Ab, mb, Fb, Sb = max(A, 1), max(m, 1), max(F, 1), max(S, 1)
    dev = _dev()
    ones = lambda *s, dt=torch.float32: torch.ones(s, dtype=dt, device=dev)
    d, w = ones(mb, dt=torch.float64), ones(mb, dt=torch.float64)
    force, amp, gy = ones(Ab, Fb), ones(Ab, mb), ones(Ab, Sb)
    nbytes = max(L.ds_osc_driven_workspace_bytes(Ab, mb, Sb), 16)
    work = Guarded((nbytes // 8 + 2,), torch.float64)
    y, gforce, gamp = Guarded((Ab, Sb)), Guarded((Ab, Fb)), Guarded((Ab, mb))
    gd, gw = Guarded((mb + 1,), torch.float64), Guarded((mb + 1,), torch.float64)
    p = _hip.ptr
    a = dict(d=p(d), w=p(w), amp=p(amp), force=p(force), gy=p(gy), work=work.ptr, nbytes=nbytes, y=y.ptr, gd=gd.ptr, gw=gw.ptr,
             gamp=gamp.ptr, gforce=gforce.ptr)
    if bad == "null-d":
        a["d"] = None
    elif bad == "null-force":
        a["force"] = None
    elif bad == "null-work":
        a["work"] = None
    elif bad == "null-out":
        a["y"] = a["gd"] = None
    elif bad == "work-short":
        a["nbytes"] = L.ds_osc_driven_workspace_bytes(A, m, S) - 1
    elif bad == "work-misaligned":
        a["work"] += 8
    elif bad == "gd-misaligned":
        a["gd"] += 4
    elif bad == "gw-misaligned":
        a["gw"] += 4
    st = _hip.stream_ptr()
    if fn.endswith("fwd"):
        rc = L.ds_osc_driven_fwd(a["d"], a["w"], a["amp"], a["force"], A, m, F, S, SR, a["work"], a["nbytes"], a["y"], st)
    else:
        rc = L.ds_osc_driven_bwd(a["gy"], a["d"], a["w"], a["amp"], a["force"], A, m, F, S, SR, a["work"], a["nbytes"],
                                 a["gd"], a["gw"], a["gamp"], a["gforce"], st)
    torch.cuda.synchronize()
    assert rc != 0
    msg = L.ds_last_error()
    assert msg and fn in msg.decode()
    for g in (work, y, gforce, gamp, gd, gw):
        assert g.untouched()
    with pytest.raises(RuntimeError, match=fn):
        _hip.check(rc, fn)


def test_workspace_bytes():
    _, L = _lib()
    for A, m, S in [(0, 1, 1), (1, 0, 1), (1, 1, 0), (-1, 4, 4), (2, -3, 4), (2, 3, -4)]:
        assert L.ds_osc_driven_workspace_bytes(A, m, S) == 0
    for A, m, S in [(1, 1, 1), (2, 16, D.TILE), (2, 17, D.TILE + 1), (8, 64, 8000), (65535, 64, 2 ** 20)]:
        assert L.ds_osc_driven_workspace_bytes(A, m, S) == 16 * (A * m * D.ntiles(S) + A * m)
