"""Debiased Sinkhorn divergence between point clouds on HIP kernels (csrc/sinkhorn.hip).

What ``geomloss==0.2.6`` ``SamplesLoss(loss="sinkhorn", p=2, blur, scaling, debias, reach=None)`` returns on its
tensorized backend - the solver behind the reference's spectral loss (src/ddsp/mss_loss.py:104-117) - forward and
backward, batched:

- cost ``C(x, y) = |x - y|^2 / 2`` and ``softmin_eps(C, h)_i = -eps * logsumexp_j(h_j - C_ij / eps)``;
- eps schedule ``[d^2] + exp(arange(2 ln d, 2 ln blur, 2 ln scaling)) + [blur^2]``, ``d`` the diagonal of the joint
  bounding box of every point of both clouds (or ``diameter=``);
- initialisation at ``d^2``, one symmetric averaged update per eps, one last extrapolation at ``blur^2``;
- ``S = <a, f_ba - f_aa> + <b, g_ab - g_bb>`` and the gradient autograd gives through geomloss's last step.

``SamplesLoss`` takes geomloss's constructor and call forms; ``compat/geomloss`` re-exports it so that code written
against the third-party package (``from geomloss import SamplesLoss``) gets this solver when ``compat`` is on the path.
Options outside the contract raise ValueError.  Device tensors only: there is no CPU path.
"""
import ctypes
import math

import numpy as np
import torch
import torch.nn as nn

from .. import _hip

MAX_D = 32  # the kernels keep a point's coordinates in registers


def eps_schedule(diameter, blur, scaling):
    """geomloss's epsilon_schedule for p = 2 (numpy ``arange`` semantics: the last entry is ``blur^2``)."""
    d = float(diameter)
    return ([d ** 2] + [float(np.exp(e)) for e in np.arange(2 * np.log(d), 2 * np.log(blur), 2 * np.log(scaling))]
            + [float(blur) ** 2])


def _check_options(blur, scaling, diameter):
    if not (isinstance(blur, (int, float)) and math.isfinite(blur) and blur > 0):
        raise ValueError(f"sinkhorn: blur={blur!r} must be a positive finite number")
    if not (isinstance(scaling, (int, float)) and 0 < scaling < 1):
        raise ValueError(f"sinkhorn: scaling={scaling!r} must lie in (0, 1)")
    if diameter is not None and not (math.isfinite(diameter) and diameter > 0):
        raise ValueError(f"sinkhorn: diameter={diameter!r} must be a positive finite number")


def _prepare(x, y, a, b):
    """Shapes and devices, checked before any device work: (x, y, a, b, batched) as contiguous f32 (B, ., .)."""
    for name, t in (("x", x), ("y", y)):
        if not torch.is_tensor(t) or not t.is_floating_point():
            raise ValueError(f"sinkhorn: {name} must be a floating-point tensor")
        if t.dim() not in (2, 3):
            raise ValueError(f"sinkhorn: {name} must be (N, D) or (B, N, D), got {tuple(t.shape)}")
    if x.dim() != y.dim():
        raise ValueError(f"sinkhorn: x {tuple(x.shape)} and y {tuple(y.shape)} must both be batched or both not")
    batched = x.dim() == 3
    if not batched:
        x, y = x.unsqueeze(0), y.unsqueeze(0)
    B, N, D = x.shape
    if y.shape[0] != B or y.shape[2] != D:
        raise ValueError(f"sinkhorn: x {tuple(x.shape)} and y {tuple(y.shape)} must share the batch size and D")
    M = y.shape[1]
    if N < 1 or M < 1 or B < 1 or D < 1 or D > MAX_D:
        raise ValueError(f"sinkhorn: need B, N, M >= 1 and 1 <= D <= {MAX_D}, got B={B} N={N} M={M} D={D}")
    ws = []
    for name, w, n in (("a", a, N), ("b", b, M)):
        if w is None:
            w = torch.full((B, n), 1.0 / n, dtype=torch.float32, device=x.device)
        else:
            if not torch.is_tensor(w) or not w.is_floating_point():
                raise ValueError(f"sinkhorn: weights {name} must be a floating-point tensor")
            if not batched:
                w = w.unsqueeze(0)
            if tuple(w.shape) != (B, n):
                raise ValueError(f"sinkhorn: weights {name} must have shape {(B, n) if batched else (n,)}, "
                                 f"got {tuple(w.shape)}")
            w = w.detach().float().contiguous()  # no gradient flows to the weights
        ws.append(w)
    for t in (x, y, *ws):
        if not t.is_cuda:
            raise ValueError("sinkhorn: tensors must live on the HIP device (no CPU fallback)")
    if len({t.device for t in (x, y, *ws)}) != 1:
        raise ValueError("sinkhorn: all tensors must live on one device")
    return x.float().contiguous(), y.float().contiguous(), ws[0], ws[1], batched


def _bbox_record(x, y, a, b):
    """The one synchronisation of a call: the bounding box, least weights and non-finite counts (ds_sinkhorn_bbox)."""
    B, N, D = x.shape
    M = y.shape[1]
    out = torch.empty(3 * D + 3, dtype=torch.float32, device=x.device)
    _hip.launch("ds_sinkhorn_bbox", x.data_ptr(), y.data_ptr(), a.data_ptr(), b.data_ptr(), B, N, M, D, out.data_ptr(), device=x.device)
    r = out.cpu().numpy().astype(np.float64)
    if r[2 * D + 2:].sum() > 0:
        raise ValueError("sinkhorn: coordinates and weights must be finite")
    if r[2 * D] <= 0 or r[2 * D + 1] <= 0:
        raise ValueError("sinkhorn: weights must be positive")
    return r[:D], r[D:2 * D]


def _schedule(x, y, a, b, blur, scaling, diameter):
    with torch.no_grad():
        lo, hi = _bbox_record(x, y, a, b)
    d = float(diameter) if diameter is not None else float(np.sqrt(((hi - lo) ** 2).sum()))
    if not d > 0:
        raise ValueError("sinkhorn: the clouds have a zero diameter (a single repeated point); pass diameter=")
    return d, eps_schedule(d, blur, scaling)


def schedule(x, y, a=None, b=None, blur=0.05, scaling=0.5, diameter=None):
    """(diameter, eps_list) that ``sinkhorn_divergence`` uses on these inputs."""
    _check_options(blur, scaling, diameter)
    x, y, a, b, _ = _prepare(x, y, a, b)
    return _schedule(x, y, a, b, blur, scaling, diameter)


class _Sinkhorn(torch.autograd.Function):
    """(x (B,N,D), y (B,M,D)) -> S (B,) f32; backward to x and y (not to the weights)."""

    @staticmethod
    def forward(ctx, x, y, a, b, eps_list, debias):
        B, N, D = x.shape
        M = y.shape[1]
        nw = _hip.lib().ds_sinkhorn_workspace_floats(B, N, M)  # (not _hip.workspace: a negative answer is this query's refusal)
        if nw < 0:
            raise ValueError(f"sinkhorn: sizes out of range B={B} N={N} M={M}")
        work = torch.empty(nw, dtype=torch.float32, device=x.device)
        loss = torch.empty(B, dtype=torch.float64, device=x.device)
        eps = (ctypes.c_float * len(eps_list))(*eps_list)
        args = (x.data_ptr(), y.data_ptr(), a.data_ptr(), b.data_ptr(), B, N, M, D)
        _hip.launch("ds_sinkhorn_loop", *args, eps, len(eps_list), int(debias), work.data_ptr(), device=x.device)
        _hip.launch("ds_sinkhorn_final", *args, float(eps_list[-1]), int(debias), work.data_ptr(), loss.data_ptr(), device=x.device)
        ctx.save_for_backward(x, y, a, b, work)
        ctx.meta = (float(eps_list[-1]), int(debias))
        return loss.float()

    @staticmethod
    def backward(ctx, g):
        x, y, a, b, work = ctx.saved_tensors
        eps, debias = ctx.meta
        B, N, D = x.shape
        M = y.shape[1]
        gx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        gy = torch.empty_like(y) if ctx.needs_input_grad[1] else None
        if gx is None and gy is None:
            return (None,) * 6
        g = g.detach().float().contiguous()
        _hip.launch("ds_sinkhorn_backward", x.data_ptr(), y.data_ptr(), a.data_ptr(), b.data_ptr(), B, N, M, D, eps, debias,
                    work.data_ptr(), g.data_ptr(), _hip.ptr(gx), _hip.ptr(gy), device=x.device)
        return gx, gy, None, None, None, None


def sinkhorn_divergence(x, y, a=None, b=None, blur=0.05, scaling=0.5, diameter=None, debias=True):
    """Debiased Sinkhorn divergence S(a x, b y) for p = 2 (geomloss's ``SamplesLoss("sinkhorn", p=2, blur, scaling,
    debias)``).  x (N, D) / (B, N, D), y (M, D) / (B, M, D) on the HIP device; a, b (N,) / (B, N) positive weights,
    uniform when None.  Returns a scalar, or (B,) for batched input.  ``debias=False`` gives <a, f_ba> + <b, g_ab>."""
    _check_options(blur, scaling, diameter)
    xf, yf, af, bf, batched = _prepare(x, y, a, b)
    _, eps_list = _schedule(xf, yf, af, bf, blur, scaling, diameter)
    S = _Sinkhorn.apply(xf, yf, af, bf, eps_list, bool(debias))
    return S if batched else S[0]


_OUTSIDE = "is outside this native solver's contract (debiased Sinkhorn, p=2, balanced, tensorized); use the " \
           "third-party package geomloss for it"


class SamplesLoss(nn.Module):
    """geomloss-compatible front end of ``sinkhorn_divergence``: ``SamplesLoss(loss="sinkhorn", p=2, blur=...)``
    called as ``loss(x, y)`` or ``loss(a, x, b, y)``.  Options the native solver does not cover raise ValueError
    naming the option."""

    def __init__(self, loss="sinkhorn", p=2, blur=0.05, reach=None, diameter=None, scaling=0.5, truncate=5, cost=None,
                 kernel=None, cluster_scale=None, debias=True, potentials=False, verbose=False, backend="auto"):
        super().__init__()
        if loss != "sinkhorn":
            raise ValueError(f"SamplesLoss: loss={loss!r} {_OUTSIDE}")
        if p != 2:
            raise ValueError(f"SamplesLoss: p={p!r} {_OUTSIDE}")
        if reach is not None:
            raise ValueError(f"SamplesLoss: reach={reach!r} (unbalanced transport) {_OUTSIDE}")
        if potentials:
            raise ValueError(f"SamplesLoss: potentials=True {_OUTSIDE}")
        if cost is not None:
            raise ValueError(f"SamplesLoss: a custom cost {_OUTSIDE}")
        if kernel is not None:
            raise ValueError(f"SamplesLoss: a custom kernel {_OUTSIDE}")
        if backend == "multiscale":
            raise ValueError(f"SamplesLoss: backend='multiscale' {_OUTSIDE}")
        if backend not in ("auto", "tensorized", "online"):
            raise ValueError(f"SamplesLoss: unknown backend={backend!r}")
        _check_options(blur, scaling, diameter)
        self.loss, self.p, self.blur, self.reach = loss, p, blur, reach
        self.diameter, self.scaling, self.debias, self.backend = diameter, scaling, debias, backend
        self.potentials, self.verbose, self.truncate, self.cluster_scale = potentials, verbose, truncate, cluster_scale

    def forward(self, *args):
        if len(args) == 2:
            x, y = args
            a = b = None
        elif len(args) == 4:
            a, x, b, y = args
        else:
            raise ValueError("SamplesLoss: call as loss(x, y) or loss(a, x, b, y)")
        if torch.is_tensor(x) and torch.is_tensor(y) and x.dim() >= 2 and y.dim() >= 2 and self.backend == "auto":
            D, NM = x.shape[-1], x.shape[-2] * y.shape[-2]
            if D <= 3 and NM > 10000 ** 2:
                raise ValueError(f"SamplesLoss: N*M = {NM} > 10000^2 with D = {D} would select backend "
                                 f"'multiscale', which {_OUTSIDE}")
        return sinkhorn_divergence(x, y, a, b, blur=self.blur, scaling=self.scaling, diameter=self.diameter,
                                   debias=self.debias)
