"""Anchors of tests/_stft_ref.py (no GPU), at the shapes of tests/test_stft_kernels_gpu.py: the fp64 references of the STFT
kernels against torch.stft and its fp64 autograd, the spectral-loss reference against the oracle and fp64 autograd, every
bound against a CPU model of the kernels' fp32 roundings, and the same model with one fault planted at a time - a bound
that holds must also see a wrong kernel."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _stft_ref as R  # noqa: E402
from oracle import mss_loss as omss  # noqa: E402


def _id(case):
    return "-".join(map(str, case))


def _worst(err, bound):
    """Largest |err| / bound; a zero bound admits only an exact match."""
    err = np.abs(err)
    return float(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf)).max())


# ------------------------------------------------------------------------------------------ references vs torch
@pytest.mark.parametrize("case", R.STFT_SHAPES, ids=_id)
def test_stft_and_its_adjoint_match_torch(case):
    """stft against torch.stft (fp64) and fold(bwd_frames(gP, re, im)) against fp64 autograd of sum gscale gP |stft|^2,
    relative to the largest element (measured: 1e-15 for P, 1e-13 for gx); T and the shapes are torch's."""
    B, S, N, hop = case
    x, gP = R.stft_inputs(case)
    re, im, P = R.stft(x, N, hop)
    xt = torch.from_numpy(x).double().requires_grad_(True)
    Z = R.torch_stft(xt, N, hop)
    T = R.n_frames(S, hop)
    assert tuple(Z.shape) == (B, N // 2 + 1, T) == re.shape == im.shape == P.shape == gP.shape
    assert R.frames(x, N, hop).shape == (B, T, N)
    Zn = Z.detach().numpy()
    rel = lambda got, ref, top=None: float(np.abs(got - ref).max() / (np.abs(ref).max() if top is None else top))
    # (re and im share one scale, the largest |Z|: frame 0 is even about its centre, so a lone frame has im = 0 + rounding)
    errs = dict(re=rel(re, Zn.real, np.abs(Zn).max()), im=rel(im, Zn.imag, np.abs(Zn).max()), P=rel(P, np.abs(Zn) ** 2))
    gscale = R.GSCALES[1]
    (gscale * torch.from_numpy(gP).double() * (Z.real ** 2 + Z.imag ** 2)).sum().backward()
    gf = R.bwd_frames(gP, re, im, N, gscale)
    gx = R.fold(gf, S, N, hop)
    assert gf.shape == (B, T, N) and gx.shape == (B, S)
    errs["gx"] = rel(gx, xt.grad.numpy())
    print(f"reference vs torch {_id(case)}: " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    assert max(errs.values()) <= 1e-12, errs


def test_fold_is_the_adjoint_of_framing():
    """<frames(x) / w, G> = <x, fold(G)> for any G, and fold_terms counts the frame elements that read each sample."""
    rng = np.random.default_rng(2)
    for B, S, N, hop in R.STFT_SHAPES[:6]:
        x, G = rng.standard_normal((B, S)), rng.standard_normal((B, R.n_frames(S, hop), N))
        pos = np.arange(R.n_frames(S, hop))[:, None] * hop + np.arange(N)[None, :] - N // 2
        lhs, rhs = (x[:, R.reflect(pos, S)] * G).sum(), (x * R.fold(G, S, N, hop)).sum()
        assert abs(lhs - rhs) <= 1e-12 * (np.abs(x[:, R.reflect(pos, S)]) * np.abs(G)).sum()
        m = R.fold_terms(S, N, hop)
        assert m.sum() == R.n_frames(S, hop) * N
        assert np.array_equal(m, np.bincount(R.reflect(pos, S).reshape(-1), minlength=S))
    # of the shapes, exactly the two with hop == n_fft leave samples under no frame (the GPU file asserts 0.0 there)
    for B, S, N, hop in R.STFT_SHAPES:
        assert (R.fold_terms(S, N, hop) == 0).any() == (hop == N)
    m = R.fold_terms(1500, 2048, 2048)  # T == 1: the lone frame reads samples 0 .. 1023 directly and 1 .. 1024 reflected
    assert (m[:1025] > 0).all() and (m[1025:] == 0).all()
    # hop == n_fft: samples past the last frame get nothing; hop 1: the longest sums
    assert (R.fold_terms(100, 64, 64)[-3:] == 0).all() and R.fold_terms(40, 32, 1).max() >= 32


# ------------------------------------------------------------------------------------- spec_loss vs the oracle
@pytest.mark.parametrize("alpha", R.ALPHAS)
@pytest.mark.parametrize("case", R.LOSS_SHAPES, ids=_id)
def test_spec_loss_matches_oracle_and_autograd(case, alpha):
    """spec_loss after the reduction _SpecLoss.forward does: kind 0 against oracle.weighted_l1 on log2 and linear power,
    kind 1 against the RMSE expression of oracle.sss_loss; gP against fp64 autograd of the same expressions.  (T == 1: the
    oracle's weights are 0 / 0; the reference follows the kernel, w = 0, and kind 0 is checked to be all zeros.)"""
    B, F, T, fclip = case
    Pp, Pt = R.loss_inputs(case)
    eps = float(np.float32(R.EPS))
    p64, t64 = Pp.astype(np.float64), Pt.astype(np.float64)
    tie = Pp == Pt
    assert (tie.any(-1).all() if T > 1 else tie.any()) and not tie.all() and tie.mean() <= 0.6
    assert ((p64 + eps < 2e-7).any() and (p64 > 1.0).any()) or Pp.size < 20

    sums, gP = R.spec_loss(0, Pp, Pt, alpha, R.EPS, fclip)
    assert sums.shape == (B, F, 2) and gP.shape == (B, F, T)
    assert not sums[:, 0].any() and not gP[:, 0].any() and not gP[tie].any()
    if T == 1:
        assert not sums.any() and not gP.any()
    else:
        cnt = B * (F - 1) * T
        assert abs(sums[..., 0].sum() / cnt / omss.weighted_l1(np.log2(p64 + eps), np.log2(t64 + eps)) - 1) <= 1e-12
        assert abs(sums[..., 1].sum() / cnt / omss.weighted_l1(p64, t64) - 1) <= 1e-12
        tp = torch.from_numpy(p64).requires_grad_(True)
        tt = torch.from_numpy(t64)
        w = 1 - torch.linspace(1.0, 0.9, T, dtype=torch.float64)
        w = w / w.sum() * T
        wl1 = lambda a, b: ((a[:, 1:] - b[:, 1:]) * w).abs().mean()
        (alpha * wl1((tp + eps).log2(), (tt + eps).log2()) + wl1(tp, tt)).backward()
        assert np.abs(gP - tp.grad.numpy()).max() <= 1e-12 * np.abs(gP).max()

    sums, gP = R.spec_loss(1, Pp, Pt, alpha, R.EPS, fclip)
    assert not sums[:, fclip:].any() and not gP[:, fclip:].any() and not sums[..., 1].any()
    f = lambda s: np.log2(s[:, :fclip] + eps) - np.log2(eps)
    want = np.sqrt(((f(p64) - f(t64)) ** 2).mean())  # oracle.sss_loss, branch 'rmse_loss'
    loss = np.sqrt(sums[..., 0].sum() / (B * fclip * T))
    assert abs(loss / want - 1) <= 1e-12
    tp = torch.from_numpy(p64).requires_grad_(True)
    tt = torch.from_numpy(t64)
    torch.sqrt((((tp[:, :fclip] + eps).log2() - (tt[:, :fclip] + eps).log2()) ** 2).mean()).backward()
    assert np.abs(gP / loss - tp.grad.numpy()).max() <= 1e-12 * np.abs(tp.grad.numpy()).max()


@pytest.mark.parametrize("case", R.LOSS_SHAPES, ids=_id)
def test_loss_inputs_keep_the_signs_unambiguous(case):
    """Every element that is no exact tie has |dlog| above the error an fp32 evaluation may make in it (bound_dlog), so
    sign(dlog) cannot differ between the kernel and the reference; sign(dlin) is that of two distinct fp32 numbers."""
    Pp, Pt = R.loss_inputs(case)
    eps = float(np.float32(R.EPS))
    dlog = np.abs(np.log2(Pp.astype(np.float64) + eps) - np.log2(Pt.astype(np.float64) + eps))
    E = R.bound_dlog(Pp, Pt, R.EPS)
    free = Pp != Pt
    assert (E[~free] == 0).all()
    if free.any():
        margin = float((dlog[free] / E[free]).min())
        print(f"dlog / its error bound {_id(case)}: at least {margin:.1f}")
        assert margin > 1.5


def test_log_error_model():
    """_ulp32 is the fp32 spacing; fp32 rounding of p + eps and a correctly rounded fp32 log2 stay inside _log_err."""
    v = np.array([1.0, 1.5, 2.0, 3.9999, 2.0 ** -30, 23.25, 0.0])
    assert np.array_equal(R._ulp32(v)[:-1], np.spacing(v[:-1].astype(np.float32)).astype(np.float64))
    assert R._ulp32(0.0) == 2.0 ** -149
    rng = np.random.default_rng(4)
    p = (10.0 ** rng.uniform(-9, 2, 5000)).astype(np.float32)
    a32 = p + np.float32(R.EPS)
    got = np.log2(a32.astype(np.float64)).astype(np.float32).astype(np.float64)
    ref = np.log2(p.astype(np.float64) + float(np.float32(R.EPS)))
    assert (np.abs(got - ref) <= R._log_err(p.astype(np.float64) + float(np.float32(R.EPS)))).all()


# ------------------------------------------------------------------------------- bounds vs the fp32 rounding model
@functools.lru_cache(maxsize=None)
def _model_ratios(case, gscale, fault=None):
    """Worst |model - reference| / bound per output, the model being ``round_like_kernel`` (with ``fault``), the references
    fed what the GPU test feeds them: the model's own re / im for the backward, its own gframes for the fold alone."""
    B, S, N, hop = case
    x, gP = R.stft_inputs(case)
    m = R.round_like_kernel(x, N, hop, gP, gscale, fault)
    re, im, P = R.stft(x, N, hop)
    b_re, b_im, b_P = R.bound_stft(x, N, hop, re, im)
    out = dict(re=_worst(m["re"] - re, b_re), im=_worst(m["im"] - im, b_im), P=_worst(m["P"] - P, b_P))
    gf = R.bwd_frames(gP, m["re"], m["im"], N, gscale)
    out["gframes"] = _worst(m["gframes"] - gf, R.bound_gframes(gP, m["re"], m["im"], N, gscale))
    out["gx_fold"] = _worst(m["gx"] - R.fold(m["gframes"], S, N, hop), R.bound_fold(m["gframes"], S, N, hop))
    out["gx"] = _worst(m["gx"] - R.fold(gf, S, N, hop), R.bound_gx(gP, m["re"], m["im"], S, N, hop, gscale))
    return out, m


@pytest.mark.parametrize("gscale", R.GSCALES)
@pytest.mark.parametrize("case", R.STFT_SHAPES, ids=_id)
def test_bounds_hold_for_fp32_model(case, gscale):
    ratios, _ = _model_ratios(case, gscale)
    print(f"fp32 model / bound {_id(case)} gscale {gscale}: " + " ".join(f"{k} {v:.3g}" for k, v in ratios.items()))
    assert max(ratios.values()) < 1.0, ratios
    assert min(ratios["re"], ratios["P"], ratios["gframes"]) > 1e-3  # the bounds are not vacuous


# which outputs each fault must show in, and the shapes at which it changes nothing
_SEEN_IN = dict(fold_left=("gx_fold", "gx"), fold_right=("gx_fold", "gx"), t1=("gx_fold", "gx"),
                window=("re", "im", "P", "gframes"), im_sign=("gframes", "gx"), offset=("re", "im", "P"))
_NO_CHANGE = dict(
    fold_left=[], t1=[], window=[],
    # a lone frame is even about its centre (x[|j|] under a symmetric window): im is rounding only, below an ulp of the sums
    im_sign=[(1, 1500, 2048, 2048)],
    # no frame reaches the right reflection: hop == n_fft with S not past the last frame's end, and T == 1
    fold_right=[(2, 100, 64, 64), (1, 1500, 2048, 2048)],
    # hop == n_fft / 4, or a single frame
    offset=[(2, 5, 8, 2), (1, 9, 16, 4), (2, 1000, 256, 64), (2, 700, 512, 128), (1, 1025, 2048, 512),
            (1, 1500, 2048, 2048), (2, 8000, 1024, 256)])


@pytest.mark.parametrize("fault", R.FAULTS)
def test_planted_faults_exceed_the_bounds(fault):
    """Mutation check.  Each fault of _stft_ref.FAULTS, planted in the fp32 model, exceeds the bound of every output listed
    for it by at least 10x at every shape where it changes the model's output at all.  Those shapes are all eleven for the
    left reflection, t1 and the window (the two smallest, (2, 5, 8, 2) and (1, 9, 16, 4), among them); all but T == 1 for the
    sign of im; all but the two of _NO_CHANGE for the right reflection; and the four shapes with hop != n_fft / 4 and T > 1
    for the frame offset, (1, 40, 32, 1) the smallest."""
    unchanged = []
    for case in R.STFT_SHAPES:
        clean, m0 = _model_ratios(case, R.GSCALES[1])
        bad, m1 = _model_ratios(case, R.GSCALES[1], fault)
        if all(np.array_equal(m0[k], m1[k]) for k in m0):
            unchanged.append(case)
            continue
        line = " ".join(f"{k} {bad[k]:.3g}" for k in _SEEN_IN[fault])
        print(f"fault {fault} {_id(case)}: {line}")
        for k in _SEEN_IN[fault]:
            assert bad[k] >= 10.0, (fault, case, k, bad[k])
    assert unchanged == _NO_CHANGE[fault]
    assert any(c[1] <= 40 for c in R.STFT_SHAPES if c not in unchanged)  # a small shape sees it


@pytest.mark.parametrize("alpha", R.ALPHAS)
@pytest.mark.parametrize("case", R.LOSS_SHAPES, ids=_id)
def test_spec_loss_bounds_hold_for_fp32_model(case, alpha):
    """The kernel's expression order in NumPy fp32 (correctly rounded operations, log2 rounded from fp64) inside
    bound_spec_loss, with exact zeros where the bounds are zero."""
    B, F, T, fclip = case
    Pp, Pt = R.loss_inputs(case)
    f32 = np.float32
    eps, il2, al = f32(R.EPS), f32(1.4426950408889634), f32(alpha)
    a = Pp + eps
    lg = lambda v: np.log2(v.astype(np.float64)).astype(f32)
    dlog = lg(a) - lg(Pt + eps)
    for kind in (0, 1):
        sums, gP = R.spec_loss(kind, Pp, Pt, alpha, R.EPS, fclip)
        bs, bg = R.bound_spec_loss(kind, Pp, Pt, alpha, R.EPS, fclip)
        ms, mg = np.zeros((B, F, 2)), np.zeros((B, F, T), dtype=f32)
        if kind == 0:
            w = R.time_weights(T).astype(f32)
            dlin = Pp - Pt
            inv = f32(1.0 / (B * (F - 1) * T))
            ms[:, 1:, 0] = np.abs((w * dlog).astype(np.float64))[:, 1:].sum(-1)
            ms[:, 1:, 1] = np.abs((w * dlin).astype(np.float64))[:, 1:].sum(-1)
            mg[:, 1:] = (w * (al * np.sign(dlog) * il2 / a + np.sign(dlin)) * inv)[:, 1:]
        else:
            inv = f32(1.0 / (B * fclip * T))
            ms[:, :fclip, 0] = (dlog.astype(np.float64) ** 2)[:, :fclip].sum(-1)
            mg[:, :fclip] = (dlog * il2 / a * inv)[:, :fclip]
        assert mg.dtype == f32
        rs, rg = _worst(ms - sums, bs), _worst(mg - gP, bg)
        print(f"fp32 model / bound spec_loss kind {kind} {_id(case)} alpha {alpha}: sums {rs:.3g} gP {rg:.3g}")
        assert rs < 1.0 and rg < 1.0


# ------------------------------------------------------------------------------------ the module-level case's inputs
@pytest.mark.parametrize("overlap", R.MODULE_OVERLAPS)
def test_module_case_reference_is_stable_in_fp32(overlap):
    """The SSSLoss case of the GPU file compares at 2e-5 (value) and 2e-3 (gradient norm) with the fp64 torch.stft
    expression.  That asks the inputs to keep the expression itself that stable between fp32 and fp64 spectrograms:
    checked here with a wide margin, so that the tolerance measures the kernels."""
    hop = int(R.MODULE_N * (1 - overlap))
    assert hop == {0.5: 32, 0.0: 64, 0.9: 6}[overlap]
    a, b = R.module_inputs(overlap)
    res = {}
    for dt in (torch.float32, torch.float64):
        xp = torch.from_numpy(a).to(dt).requires_grad_(True)
        loss = R.torch_rmse_loss(xp, torch.from_numpy(b).to(dt), R.MODULE_N, hop, R.EPS)
        loss.backward()
        res[dt] = (float(loss.detach()), xp.grad.double())
    v32, g32 = res[torch.float32]
    v64, g64 = res[torch.float64]
    dv, dg = abs(v32 / v64 - 1), float((g32 - g64).norm() / g64.norm())
    print(f"module case overlap {overlap}: fp32 vs fp64 expression value {dv:.1e} gradient {dg:.1e}")
    assert dv < 2e-6 and dg < 4e-4  # a tenth and a fifth of the tolerances
