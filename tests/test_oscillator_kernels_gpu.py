"""The six kernels of diffsound_amd/csrc/oscillator.hip behind their four C entry points, sample by sample against the
fp64 references of tests/_osc_ref.py at the bounds derived there (tests/test_osc_ref_cpu.py anchors both without a GPU).

Every output lives 64 elements inside a NaN-filled buffer: after a call both guard zones must still be NaN and the
output finite, the scratch array of the time-varying forward (sized exactly to ds_osc_tv_workspace_floats) included.
Each case prints its largest error / bound ratio per output (``pytest -s``)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _osc_ref as R  # noqa: E402
from _guarded import Guarded, _id, _lib, _ratio, _up, dev as _dev  # noqa: E402

pytestmark = pytest.mark.gpu

SR = R.SR
TV_CASES = [(s, "base") for s in R.TV_SHAPES] + [(s, v) for s in R.TV_SHAPES if s[3] in (65, 1025) for v in R.TV_VARIANTS]
BANK_CASES = [(s, True) for s in R.BANK_SHAPES] + [(R.BANK_SHAPES[i], False) for i in (0, 3, 5)]


# ------------------------------------------------------------------------------------------ time-varying pair
def _tv_call(inputs):
    """One forward and one backward call on fresh guarded buffers.  Returns the buffers by name."""
    _hip, L = _lib()
    dmp, frq, amp, force, gy = inputs
    A, m, S = dmp.shape
    F = force.shape[1]
    p = _hip.ptr
    d_dmp, d_frq, d_amp, d_force, d_gy = map(_up, (dmp, frq, amp, force, gy))
    nwork = L.ds_osc_tv_workspace_floats(A, m, S)
    assert nwork == A * R.tv_partials(m) * S
    out = dict(work=Guarded((nwork,)), y=Guarded((A, S)), gs=Guarded((A, S)), g_dmp=Guarded((A, m, S)),
               g_frq=Guarded((A, m, S)))
    if amp is not None:
        out["gamp"] = Guarded((A, m))
    _hip.check(L.ds_osc_tv_fwd(p(d_dmp), p(d_frq), p(d_amp), p(d_force), A, m, F, S, SR, out["work"].ptr, out["y"].ptr,
                               _hip.stream_ptr()), "ds_osc_tv_fwd")
    _hip.check(L.ds_osc_tv_bwd(p(d_gy), p(d_dmp), p(d_frq), p(d_amp), p(d_force), A, m, F, S, SR, out["gs"].ptr,
                               out["g_dmp"].ptr, out["g_frq"].ptr, out["gamp"].ptr if amp is not None else None,
                               _hip.stream_ptr()), "ds_osc_tv_bwd")
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def _tv_run(case):
    inputs = R.tv_inputs(*case)
    first, second = _tv_call(inputs), _tv_call(inputs)
    return inputs, first, second


@pytest.mark.parametrize("case", TV_CASES, ids=_id)
def test_tv_forward(case):
    (dmp, frq, amp, force, gy), out, again = _tv_run(case)
    m = dmp.shape[1]
    out["work"].check("work")
    out["y"].check("y")
    y_ref, E = R.tv_forward(dmp, frq, amp, force, SR)
    assert _ratio("tv.y", case, out["y"].numpy(), y_ref, R.bound_y(force, E, R.tv_partials(m))) <= 1.0
    assert np.array_equal(out["y"].numpy(), again["y"].numpy())
    assert np.array_equal(out["work"].numpy(), again["work"].numpy())


@pytest.mark.parametrize("case", TV_CASES, ids=_id)
def test_tv_backward(case):
    (dmp, frq, amp, force, gy), out, again = _tv_run(case)
    S = dmp.shape[2]
    for k in ("gs", "g_dmp", "g_frq", "gamp"):
        if k in out:
            out[k].check(k)
            assert np.array_equal(out[k].numpy(), again[k].numpy()), k
    gs = out["gs"].numpy()
    assert _ratio("tv.gs", case, gs, R.corr(gy, force), R.bound_gs(gy, force)) <= 1.0
    # the reference is fed the device's own gs: what follows is osc_tv_bwd_kernel alone
    g_dmp, g_frq, gamp, U, V = R.tv_backward(gs, dmp, frq, amp, SR)
    assert _ratio("tv.g_dmp", case, out["g_dmp"].numpy(), g_dmp, R.bound_g_dmp(g_dmp, U, S, SR)) <= 1.0
    assert _ratio("tv.g_frq", case, out["g_frq"].numpy(), g_frq, R.bound_g_frq(g_frq, U, S, SR)) <= 1.0
    if amp is not None:
        assert _ratio("tv.gamp", case, out["gamp"].numpy(), gamp, R.bound_gamp(gamp, V, S)) <= 1.0


# ------------------------------------------------------------------------------------------- closed-form pair
def _bank_call(inputs, S):
    _hip, L = _lib()
    d, w, amp, force, gy = inputs
    A, F = force.shape
    m = d.shape[0]
    p = _hip.ptr
    d_d, d_w, d_amp, d_force, d_gy = map(_up, (d, w, amp, force, gy))
    out = dict(y=Guarded((A, S)), gs=Guarded((A, S)), gd=Guarded((m,), torch.float64), gw=Guarded((m,), torch.float64))
    if amp is not None:
        out["gamp"] = Guarded((A, m))
    _hip.check(L.ds_osc_bank_fwd(p(d_d), p(d_w), p(d_amp), p(d_force), A, m, F, S, SR, out["y"].ptr, _hip.stream_ptr()),
               "ds_osc_bank_fwd")
    _hip.check(L.ds_osc_bank_bwd(p(d_gy), p(d_d), p(d_w), p(d_amp), p(d_force), A, m, F, S, SR, out["gs"].ptr,
                                 out["gd"].ptr, out["gw"].ptr, out["gamp"].ptr if amp is not None else None,
                                 _hip.stream_ptr()), "ds_osc_bank_bwd")
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def _bank_run(case):
    inputs = R.bank_inputs(*case)
    S = case[0][3]
    return inputs, _bank_call(inputs, S), _bank_call(inputs, S)


@pytest.mark.parametrize("case", BANK_CASES, ids=_id)
def test_bank_forward(case):
    (d, w, amp, force, gy), out, again = _bank_run(case)
    S = case[0][3]
    out["y"].check("y")
    y_ref, E = R.bank_forward(d, w, amp, force, S, SR)
    assert _ratio("bank.y", case, out["y"].numpy(), y_ref, R.bound_y(force, E, R.BANK_PARTIALS)) <= 1.0
    assert np.array_equal(out["y"].numpy(), again["y"].numpy())


@pytest.mark.parametrize("case", BANK_CASES, ids=_id)
def test_bank_backward(case):
    (d, w, amp, force, gy), out, again = _bank_run(case)
    S = case[0][3]
    for k in ("gs", "gd", "gw", "gamp"):
        if k in out:
            out[k].check(k)
            assert np.array_equal(out[k].numpy(), again[k].numpy()), k
    gs = out["gs"].numpy()
    assert _ratio("bank.gs", case, gs, R.corr(gy, force), R.bound_gs(gy, force)) <= 1.0
    gd, gw, gamp, W, V = R.bank_backward(gs, d, w, amp, SR)
    assert _ratio("bank.gd", case, out["gd"].numpy(), gd, R.bound_gd_gw(W, S)) <= 1.0
    assert _ratio("bank.gw", case, out["gw"].numpy(), gw, R.bound_gd_gw(W, S)) <= 1.0
    if amp is not None:
        assert _ratio("bank.gamp", case, out["gamp"].numpy(), gamp, R.bound_gamp(gamp, V, S)) <= 1.0


# ------------------------------------------------------------------------------------------------ cross-check
@pytest.mark.parametrize("shape", [(1, 5, 7, 65), (1, 17, 150, 1025)], ids=lambda s: "-".join(map(str, s)))
def test_tv_with_constant_rates_is_the_bank(shape):
    """With dmp and frq constant in time the two banks compute the same signal (both at tau = (t + 1) / sr): the outputs
    agree within the sum of their bounds, and sum_t g_dmp = gd, sum_t g_frq = 2 pi gw (w = 2 pi frq), within the
    time-varying per-sample bounds summed over clips and samples plus the bank's bound."""
    case = (shape, "const")
    dmp, frq, amp, force, gy = R.tv_inputs(*case)
    A, m, S = dmp.shape
    d, w = dmp[0, :, 0].astype(np.float64), R.TWO_PI * frq[0, :, 0].astype(np.float64)
    tv = _tv_call((dmp, frq, amp, force, gy))
    bank = _bank_call((d, w, amp, force, gy), S)
    for o in list(tv.values()) + list(bank.values()):
        o.check("cross-check output")
    _, E_tv = R.tv_forward(dmp, frq, amp, force, SR)
    _, E_bank = R.bank_forward(d, w, amp, force, S, SR)
    tol = R.bound_y(force, E_tv, R.tv_partials(m)) + R.bound_y(force, E_bank, R.BANK_PARTIALS)
    assert _ratio("cross.y", case, tv["y"].numpy(), bank["y"].numpy().astype(np.float64), tol) <= 1.0
    gs = tv["gs"].numpy()
    assert np.array_equal(gs, bank["gs"].numpy())  # the same kernel on the same operands
    g_dmp, g_frq, _, U, _ = R.tv_backward(gs, dmp, frq, amp, SR)
    _, _, _, W, _ = R.bank_backward(gs, d, w, amp, SR)
    tol_d = R.bound_g_dmp(g_dmp, U, S, SR).sum((0, 2)) + R.bound_gd_gw(W, S)
    tol_w = R.bound_g_frq(g_frq, U, S, SR).sum((0, 2)) + R.TWO_PI * R.bound_gd_gw(W, S)
    sum_d = tv["g_dmp"].numpy().astype(np.float64).sum((0, 2))
    sum_f = tv["g_frq"].numpy().astype(np.float64).sum((0, 2))
    assert _ratio("cross.gd", case, sum_d, bank["gd"].numpy(), tol_d) <= 1.0
    assert _ratio("cross.gw", case, sum_f, R.TWO_PI * bank["gw"].numpy(), tol_w) <= 1.0


# -------------------------------------------------------------------------------------------------- refusals
_BAD = {"F=0": dict(F=0), "F=513": dict(F=513), "S=0": dict(S=0), "m=0": dict(m=0), "A=65536": dict(A=65536, m=1, F=1, S=1)}
_REFUSALS = [(fn, bad) for fn in ("ds_osc_bank_fwd", "ds_osc_bank_bwd", "ds_osc_tv_fwd", "ds_osc_tv_bwd") for bad in _BAD
             if bad != "A=65536" or "_tv_" in fn]


@pytest.mark.parametrize("fn,bad", _REFUSALS, ids=[f"{f}-{b}" for f, b in _REFUSALS])
def test_refusals_write_nothing(fn, bad):
    """Arguments outside the kernels' limits are rejected before any launch: nonzero status, a message naming the entry
    point, every output still NaN.  (The buffers are as large as the largest in-range reading of the arguments, so a
    call that wrongly went ahead would stay inside them.)"""
    _hip, L = _lib()
    dims = dict(A=2, m=3, F=5, S=7)
    dims.update(_BAD[bad])
    A, m, F, S = (dims[k] for k in "AmFS")
    Ab, mb, Fb, Sb = max(A, 1), max(m, 1), max(F, 1), max(S, 1)
    dev = _dev()
    ones = lambda *s: torch.ones(s, device=dev)
    force, amp, gy = ones(Ab, Fb), ones(Ab, mb), ones(Ab, Sb)
    nan = lambda *s, dt=torch.float32: torch.full(s, float("nan"), dtype=dt, device=dev)
    p = _hip.ptr
    st = _hip.stream_ptr()
    if "_tv_" in fn:
        dmp, frq = ones(Ab, mb, Sb), ones(Ab, mb, Sb)
        if fn.endswith("fwd"):
            outs = [nan(Ab * mb * Sb), nan(Ab, Sb)]
            rc = L.ds_osc_tv_fwd(p(dmp), p(frq), p(amp), p(force), A, m, F, S, SR, p(outs[0]), p(outs[1]), st)
        else:
            outs = [nan(Ab, Sb), nan(Ab, mb, Sb), nan(Ab, mb, Sb), nan(Ab, mb)]
            rc = L.ds_osc_tv_bwd(p(gy), p(dmp), p(frq), p(amp), p(force), A, m, F, S, SR, *map(p, outs), st)
    else:
        d, w = torch.ones(mb, dtype=torch.float64, device=dev), torch.ones(mb, dtype=torch.float64, device=dev)
        if fn.endswith("fwd"):
            outs = [nan(Ab, Sb)]
            rc = L.ds_osc_bank_fwd(p(d), p(w), p(amp), p(force), A, m, F, S, SR, p(outs[0]), st)
        else:
            outs = [nan(Ab, Sb), nan(mb, dt=torch.float64), nan(mb, dt=torch.float64), nan(Ab, mb)]
            rc = L.ds_osc_bank_bwd(p(gy), p(d), p(w), p(amp), p(force), A, m, F, S, SR, *map(p, outs), st)
    torch.cuda.synchronize()
    assert rc != 0
    msg = L.ds_last_error()
    assert msg and fn in msg.decode()
    for o in outs:
        assert bool(torch.isnan(o).all())
    with pytest.raises(RuntimeError, match=fn):
        _hip.check(rc, fn)


def test_tv_workspace_floats():
    _, L = _lib()
    for A, m, S in [(0, 1, 1), (1, 0, 1), (1, 1, 0), (-1, 4, 4), (2, -3, 4), (2, 3, -4)]:
        assert L.ds_osc_tv_workspace_floats(A, m, S) == 0
    for A, m, S in [(1, 1, 1), (2, 16, 5), (2, 17, 5), (3, 33, 2500)]:
        assert L.ds_osc_tv_workspace_floats(A, m, S) == A * R.tv_partials(m) * S


# ------------------------------------------------------------------------------------------ autograd wrappers
@pytest.mark.parametrize("with_amp", [False, True], ids=["noamp", "amp"])
def test_autograd_wrappers(with_amp):
    """oscillator_bank_tv and oscillator_bank through .backward(), with and without amplitudes (the has_amp branches of
    both Functions), against fp64 autograd of the torch chains.  Tolerances: the kernel bounds, and for the gradients
    the correlation's bound carried through the (linear) mode kernel: |delta g_dmp| <= U(bound_gs) / sr and so on."""
    from diffsound_amd.ddsp.oscillator import oscillator_bank, oscillator_bank_tv

    shape = (2, 5, 3, 130)
    A, m, F, S = shape
    case = (shape, "amp" if with_amp else "noamp")
    dev = _dev()
    leaf32 = lambda x: None if x is None else torch.from_numpy(x).to(dev).requires_grad_(True)
    leaf64 = lambda x: None if x is None else torch.from_numpy(np.asarray(x)).double().requires_grad_(True)

    # time-varying bank
    dmp, frq, amp, force, gy = R.tv_inputs(shape, "base" if with_amp else "noamp")
    g_d, g_f, g_a = leaf32(dmp), leaf32(frq), leaf32(amp)
    y = oscillator_bank_tv(g_d, g_f, g_a, _up(force), S, SR)
    (y * _up(gy)).sum().backward()
    r_d, r_f, r_a = leaf64(dmp), leaf64(frq), leaf64(amp)
    yr = R.torch_tv_chain(r_d, r_f, r_a, torch.from_numpy(force).double(), SR)
    (yr * torch.from_numpy(gy).double()).sum().backward()
    _, E = R.tv_forward(dmp, frq, amp, force, SR)
    assert _ratio("wrap.tv.y", case, y.detach().cpu().numpy(), yr.detach().numpy(), R.bound_y(force, E, R.tv_partials(m))) <= 1.0
    _, _, _, U, V = R.tv_backward(R.corr(gy, force), dmp, frq, amp, SR)
    _, _, _, Ub, Vb = R.tv_backward(R.bound_gs(gy, force), dmp, frq, amp, SR)
    ref = r_d.grad.numpy()
    assert _ratio("wrap.tv.g_dmp", case, g_d.grad.cpu().numpy(), ref,
                  R.bound_g_dmp(ref, U, S, SR) + Ub[:, :, None] / SR) <= 1.0
    ref = r_f.grad.numpy()
    assert _ratio("wrap.tv.g_frq", case, g_f.grad.cpu().numpy(), ref,
                  R.bound_g_frq(ref, U, S, SR) + R.TWO_PI * Ub[:, :, None] / SR) <= 1.0
    if with_amp:
        ref = r_a.grad.numpy()
        assert _ratio("wrap.tv.gamp", case, g_a.grad.cpu().numpy(), ref, R.bound_gamp(ref, V, S) + Vb) <= 1.0

    # closed-form bank
    d, w, amp, force, gy = R.bank_inputs(shape, with_amp)
    g_d, g_w, g_a = leaf32(d), leaf32(w), leaf32(amp)  # (d, w stay fp64: from_numpy keeps the dtype)
    y = oscillator_bank(g_d, g_w, g_a, _up(force), S, SR)
    (y * _up(gy)).sum().backward()
    r_d, r_w, r_a = leaf64(d), leaf64(w), leaf64(amp)
    yr = R.torch_bank_chain(r_d, r_w, r_a, torch.from_numpy(force).double(), S, SR)
    (yr * torch.from_numpy(gy).double()).sum().backward()
    _, E = R.bank_forward(d, w, amp, force, S, SR)
    assert _ratio("wrap.bank.y", case, y.detach().cpu().numpy(), yr.detach().numpy(),
                  R.bound_y(force, E, R.BANK_PARTIALS)) <= 1.0
    _, _, _, W, V = R.bank_backward(R.corr(gy, force), d, w, amp, SR)
    _, _, _, Wb, Vb = R.bank_backward(R.bound_gs(gy, force), d, w, amp, SR)
    assert g_d.grad.dtype == torch.float64 and g_w.grad.dtype == torch.float64
    assert _ratio("wrap.bank.gd", case, g_d.grad.cpu().numpy(), r_d.grad.numpy(), R.bound_gd_gw(W, S) + Wb) <= 1.0
    assert _ratio("wrap.bank.gw", case, g_w.grad.cpu().numpy(), r_w.grad.numpy(), R.bound_gd_gw(W, S) + Wb) <= 1.0
    if with_amp:
        ref = r_a.grad.numpy()
        assert _ratio("wrap.bank.gamp", case, g_a.grad.cpu().numpy(), ref, R.bound_gamp(ref, V, S) + Vb) <= 1.0
