"""The four kernels of diffsound_amd/csrc/stft.hip behind their three C entry points (ds_stft_power, ds_stft_power_bwd,
ds_spec_loss), element by element against the fp64 references of tests/_stft_ref.py at the bounds derived there
(tests/test_stft_ref_cpu.py anchors both without a GPU and shows that the bounds see planted faults).

Every output lives 64 elements inside a NaN-filled buffer: after a call both guard zones must still be NaN and the output
finite.  The backward is fed the device's own fp32 re / im and the reference reads the same numbers, so no kink of the loss
is involved and the kernels are checked at rounding level; the fold is also checked alone, against the fold of the device's
own gframes.  A second call of every entry point must be bitwise equal.  Each case prints its largest error / bound ratio
per output (``pytest -s``).

Worst error / bound ratio per output over all cases: MI355X as measured, and the CPU model of the fp32 roundings
(_stft_ref.round_like_kernel; for ds_spec_loss the fp32 NumPy model of test_stft_ref_cpu.py):

    output              MI355X   CPU model
    stft.re             0.22     0.22
    stft.im             0.188    0.187
    stft.P              0.187    0.187
    bwd.gframes         0.498    0.498
    bwd.gx_fold         0.979    0.979
    bwd.gx              0.473    0.473
    loss.sums kind 0    0.32     0.32
    loss.gP kind 0      0.644    0.645
    loss.sums kind 1    0.136    0.096
    loss.gP kind 1      0.368    0.322
    module.value        0.0365   -        (of the tolerances 2e-5 and 2e-3)
    module.grad         0.0528   -        (of the tolerances 2e-5 and 2e-3)
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _stft_ref as R  # noqa: E402
from _guarded import Guarded, _id, _lib, _ratio, _up, dev as _dev  # noqa: E402

pytestmark = pytest.mark.gpu

LOSS_CASES = [(c, k, a) for c in R.LOSS_SHAPES for k in (0, 1) for a in R.ALPHAS]


# ------------------------------------------------------------------------------------------------------ STFT
def _fwd_call(d_x, case, parts):
    _hip, L = _lib()
    B, S, N, hop = case
    shape = (B, N // 2 + 1, R.n_frames(S, hop))
    out = dict(P=Guarded(shape))
    if parts:
        out.update(re=Guarded(shape), im=Guarded(shape))
    _hip.check(L.ds_stft_power(_hip.ptr(d_x), B, S, N, hop, out["P"].ptr, out["re"].ptr if parts else None,
                               out["im"].ptr if parts else None, _hip.stream_ptr()), "ds_stft_power")
    torch.cuda.synchronize()
    return out


def _bwd_call(d_gP, fwd, case, gscale):
    """ds_stft_power_bwd on the re / im that ``fwd`` (a forward call's buffers) holds on the device."""
    _hip, L = _lib()
    B, S, N, hop = case
    out = dict(gframes=Guarded((B, R.n_frames(S, hop), N)), gx=Guarded((B, S)))
    _hip.check(L.ds_stft_power_bwd(_hip.ptr(d_gP), fwd["re"].ptr, fwd["im"].ptr, B, S, N, hop, gscale, out["gframes"].ptr,
                                   out["gx"].ptr, _hip.stream_ptr()), "ds_stft_power_bwd")
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def _stft_run(case):
    """Everything the device computes for one case, once: two forward calls with re / im, one without, and two backward
    calls per gscale."""
    x, gP = R.stft_inputs(case)
    d_x, d_gP = _up(x), _up(gP)
    first, again, bare = _fwd_call(d_x, case, True), _fwd_call(d_x, case, True), _fwd_call(d_x, case, False)
    bwd = {g: (_bwd_call(d_gP, first, case, g), _bwd_call(d_gP, first, case, g)) for g in R.GSCALES}
    return x, gP, first, again, bare, bwd


@pytest.mark.parametrize("case", R.STFT_SHAPES, ids=_id)
def test_stft_forward(case):
    B, S, N, hop = case
    x, _, out, again, bare, _ = _stft_run(case)
    for k in ("P", "re", "im"):
        out[k].check(k)
        again[k].check(k)
        assert np.array_equal(out[k].numpy(), again[k].numpy()), k  # deterministic
    bare["P"].check("P without re / im")
    assert np.array_equal(out["P"].numpy(), bare["P"].numpy())  # re = im = NULL changes nothing in P
    re, im, P = R.stft(x, N, hop)
    b_re, b_im, b_P = R.bound_stft(x, N, hop, re, im)
    worst = [_ratio("stft.re", case, out["re"].numpy(), re, b_re), _ratio("stft.im", case, out["im"].numpy(), im, b_im),
             _ratio("stft.P", case, out["P"].numpy(), P, b_P)]
    assert max(worst) <= 1.0


@pytest.mark.parametrize("gscale", R.GSCALES)
@pytest.mark.parametrize("case", R.STFT_SHAPES, ids=_id)
def test_stft_backward(case, gscale):
    B, S, N, hop = case
    _, gP, fwd, _, _, bwd = _stft_run(case)
    out, again = bwd[gscale]
    for k in ("gframes", "gx"):
        out[k].check(k)
        assert np.array_equal(out[k].numpy(), again[k].numpy()), k
    for k in ("P", "re", "im"):
        fwd[k].check(k + " after the backward")  # the backward reads them and writes nothing there
    tag = (*case, gscale)
    re, im = fwd["re"].numpy(), fwd["im"].numpy()  # the device's own fp32 values: the reference reads the same
    gf, gx = out["gframes"].numpy(), out["gx"].numpy()
    gf_ref = R.bwd_frames(gP, re, im, N, gscale)
    worst = [_ratio("bwd.gframes", tag, gf, gf_ref, R.bound_gframes(gP, re, im, N, gscale)),
             # the fold alone, on the device's own gframes
             _ratio("bwd.gx_fold", tag, gx, R.fold(gf, S, N, hop), R.bound_fold(gf, S, N, hop)),
             # both kernels end to end
             _ratio("bwd.gx", tag, gx, R.fold(gf_ref, S, N, hop), R.bound_gx(gP, re, im, S, N, hop, gscale))]
    assert max(worst) <= 1.0
    dead = R.fold_terms(S, N, hop) == 0  # samples under no frame (the two hop == n_fft shapes have some): gradient exactly 0
    assert dead.any() == (hop == N)
    assert not gx[:, dead].any()


# -------------------------------------------------------------------------------------------------- spec_loss
def _loss_call(d_Pp, d_Pt, case, kind, alpha, with_g):
    _hip, L = _lib()
    B, F, T, fclip = case
    out = dict(sums=Guarded((B, F, 2), torch.float64))
    if with_g:
        out["gP"] = Guarded((B, F, T))  # NaN-filled: a row the kernel failed to write stays NaN
    _hip.check(L.ds_spec_loss(kind, _hip.ptr(d_Pp), _hip.ptr(d_Pt), B, F, T, alpha, R.EPS, fclip, out["sums"].ptr,
                              out["gP"].ptr if with_g else None, _hip.stream_ptr()), "ds_spec_loss")
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("case,kind,alpha", LOSS_CASES, ids=[f"{_id(c)}-kind{k}-alpha{a}" for c, k, a in LOSS_CASES])
def test_spec_loss(case, kind, alpha):
    B, F, T, fclip = case
    Pp, Pt = R.loss_inputs(case)
    d_Pp, d_Pt = _up(Pp), _up(Pt)
    out, again, bare = (_loss_call(d_Pp, d_Pt, case, kind, alpha, g) for g in (True, True, False))
    for o in (out, again, bare):
        for k, v in o.items():
            v.check(k)
    sums, gP = out["sums"].numpy(), out["gP"].numpy()
    assert np.array_equal(sums, again["sums"].numpy()) and np.array_equal(gP, again["gP"].numpy())  # deterministic
    assert np.array_equal(sums, bare["sums"].numpy())  # gP = NULL changes nothing in the sums
    ref_s, ref_g = R.spec_loss(kind, Pp, Pt, alpha, R.EPS, fclip)
    b_s, b_g = R.bound_spec_loss(kind, Pp, Pt, alpha, R.EPS, fclip)
    tag = (*case, f"kind{kind}", alpha)
    worst = [_ratio("loss.sums", tag, sums, ref_s, b_s), _ratio("loss.gP", tag, gP, ref_g, b_g)]
    assert max(worst) <= 1.0
    # exact zeros: the excluded rows (DC for kind 0, f >= fclip for kind 1), the unused second sum of kind 1, and for
    # kind 0 the elements where prediction and target tie (sign(0) = 0 in both terms)
    gone = np.arange(F) < 1 if kind == 0 else np.arange(F) >= fclip
    assert not sums[:, gone].any() and not gP[:, gone].any()
    if kind == 1:
        assert not sums[..., 1].any()
    else:
        assert (Pp == Pt).any() and not gP[Pp == Pt].any()
        if T == 1:
            # the reference's weights are 0 / 0 at T == 1 (NaN loss); the kernel documents wnorm = 0 instead: all zeros,
            # no NaN.  This departure is the kernel's stated choice and is what is asserted here.
            assert not sums.any() and not gP.any()


# --------------------------------------------------------------------------------------------------- refusals
_OK = dict(B=2, S=100, N=64, hop=16)
_BAD_STFT = {"n_fft=4": dict(N=4), "n_fft=48": dict(N=48), "n_fft=4096": dict(N=4096, S=4000), "hop=0": dict(hop=0),
             "hop=n_fft+1": dict(hop=65), "S=n_fft/2": dict(S=32), "B=0": dict(B=0), "B=65536": dict(B=65536)}
_STFT_REFUSALS = [(fn, bad) for fn in ("ds_stft_power", "ds_stft_power_bwd") for bad in _BAD_STFT] + [("ds_stft_power", "re-without-im"),
                                                                                                    ("ds_stft_power", "im-without-re")]


@pytest.mark.parametrize("fn,bad", _STFT_REFUSALS, ids=[f"{f}-{b}" for f, b in _STFT_REFUSALS])
def test_stft_refusals_write_nothing(fn, bad):
    """Arguments outside stft_shape_ok, and re without im, are rejected by the entry point's argument checks, before any
    launch: nonzero status, a message naming the entry point, every output still NaN."""
    _hip, L = _lib()
    dims = dict(_OK)
    dims.update(_BAD_STFT.get(bad, {}))
    B, S, N, hop = (dims[k] for k in ("B", "S", "N", "hop"))
    F, T = 64, 64  # outputs sized for the legal base shape and above; the calls return before they would be used
    ones = lambda *s: torch.ones(s, device=_dev())
    x, gP, re, im = ones(2, 4000), ones(2, F, T), ones(2, F, T), ones(2, F, T)
    p, st = _hip.ptr, _hip.stream_ptr()
    if fn == "ds_stft_power":
        outs = [Guarded((2, F, T)) for _ in range(3)]
        ptrs = [o.ptr for o in outs]
        if bad == "re-without-im":
            ptrs[2] = None
        elif bad == "im-without-re":
            ptrs[1] = None
        rc = L.ds_stft_power(p(x), B, S, N, hop, *ptrs, st)
    else:
        outs = [Guarded((2, T, 64)), Guarded((2, 4000))]
        rc = L.ds_stft_power_bwd(p(gP), p(re), p(im), B, S, N, hop, 1.0, outs[0].ptr, outs[1].ptr, st)
    torch.cuda.synchronize()
    assert rc != 0
    msg = L.ds_last_error()
    assert msg and fn in msg.decode()
    assert all(o.untouched() for o in outs)
    with pytest.raises(RuntimeError, match=fn):
        _hip.check(rc, fn)


_BAD_LOSS = {"kind=2": dict(kind=2), "F=1": dict(F=1, fclip=1), "fclip>F": dict(fclip=6), "fclip=0-kind1": dict(kind=1, fclip=0)}


@pytest.mark.parametrize("bad", list(_BAD_LOSS))
def test_spec_loss_refusals_write_nothing(bad):
    _hip, L = _lib()
    a = dict(kind=0, B=2, F=5, T=7, fclip=5)
    a.update(_BAD_LOSS[bad])
    Pp = torch.ones((2, 5, 7), device=_dev())
    sums, gP = Guarded((2, 5, 2), torch.float64), Guarded((2, 5, 7))
    rc = L.ds_spec_loss(a["kind"], _hip.ptr(Pp), _hip.ptr(Pp), a["B"], a["F"], a["T"], 1.0, R.EPS, a["fclip"], sums.ptr, gP.ptr,
                        _hip.stream_ptr())
    torch.cuda.synchronize()
    assert rc != 0
    msg = L.ds_last_error()
    assert msg and "ds_spec_loss" in msg.decode()
    assert sums.untouched() and gP.untouched()


# ------------------------------------------------------------------------------------------ through the module
@pytest.mark.parametrize("overlap", R.MODULE_OVERLAPS)
def test_sssloss_at_hops_other_than_a_quarter(overlap):
    """SSSLoss(type='rmse_loss', n_fft=64, overlap) on clips of 1000 samples: hops 32, 64 and 6, which ``overlap`` can
    produce and the tests of MSSLoss (always n_fft / 4) never do.  Value and gradient against the fp64 torch.stft
    expression of tests/test_mss_loss.py::_torch_loss with the hop as an argument, at that file's tolerances."""
    from diffsound_amd.ddsp.mss_loss import SSSLoss

    a, b = R.module_inputs(overlap)
    m = SSSLoss(R.MODULE_N, int(R.SR), overlap=overlap, type="rmse_loss")
    hop = {0.5: 32, 0.0: 64, 0.9: 6}[overlap]
    assert m.hop_length == hop
    xp = _up(a).requires_grad_(True)
    loss = m(xp, _up(b))
    loss.backward()
    xr = torch.from_numpy(a).double().requires_grad_(True)
    ref = R.torch_rmse_loss(xr, torch.from_numpy(b).double(), R.MODULE_N, hop, R.EPS)
    ref.backward()
    dv = abs(float(loss.detach()) / float(ref.detach()) - 1)
    dg = float((xp.grad.double().cpu() - xr.grad).norm() / xr.grad.norm())
    print(f"RATIO module.value {overlap} {dv / 2e-5:.4g}")
    print(f"RATIO module.grad {overlap} {dg / 2e-3:.4g}")
    assert dv < 2e-5
    assert dg < 2e-3
    assert float(m(xp.detach(), _up(b))) == float(loss.detach())  # deterministic
