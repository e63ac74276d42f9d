"""Propagation delay: a time-varying fractional delay line (ds_delay_fwd / ds_delay_bwd, csrc/delay.hip).

What a receiver on a path x(t) hears of a source at rest is s(t - r(t) / c).  ``propagate`` delays each row of a rendered
signal by a delay given in samples at K control frames ``hop`` samples apart, linear in between, the last frame held
(the frames of the sliding and the listener bank), with a 16-tap Hann-windowed sinc:

    tau(t) = (1 - th) delay[k] + th delay[min(k + 1, K - 1)],   p(t) = t - tau(t),  n = floor(p),  f = p - n,
    y[t]   = sum_{i = -7 .. 8} h(f - i) signal[n + i],          h(u) = sinc(u) cos^2(pi u / 16) for |u| < 8, 0 outside,

``signal`` taken as 0 outside [0, S).  An integer delay is an exact shift.  h is C1, so the gradient to the delay is
continuous; both gradients are exact adjoints of the forward (``ModalRadiator.listener_path`` gives the delay of a path).
"""
import math

import torch

from .. import _hip

HALF_TAPS = 8      # DS_DELAY_HALF_TAPS
MAX_SLOPE = 0.5    # DS_DELAY_MAX_SLOPE: |delay[k + 1] - delay[k]| <= hop MAX_SLOPE, a receiver below Mach 0.5
MAX_ROWS = 65535   # DS_DELAY_MAX_ROWS


class _Delay(torch.autograd.Function):
    """y (B, S) fp32 from s (B, S) fp32 and tau (B, K) fp64; gradients for both, each computed only where it is needed."""

    @staticmethod
    def forward(ctx, s, tau, hop):
        s, tau = s.detach().contiguous(), tau.detach().contiguous()
        B, S = s.shape
        y = torch.empty_like(s)
        p = _hip.ptr
        _hip.launch("ds_delay_fwd", p(s), p(tau), B, S, tau.shape[1], hop, p(y), device=s.device)
        ctx.save_for_backward(s, tau)
        ctx.hop = hop
        return y

    @staticmethod
    def backward(ctx, gy):
        s, tau = ctx.saved_tensors
        need_s, need_t = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_s or need_t):
            return None, None, None
        B, S = s.shape
        K = tau.shape[1]
        gy = gy.float().contiguous()
        work, nbytes = _hip.workspace("ds_delay_workspace_bytes", B, S, K, ctx.hop, device=s.device)
        gs = torch.empty_like(s) if need_s else None
        gtau = torch.empty_like(tau) if need_t else None
        p = _hip.ptr
        _hip.launch("ds_delay_bwd", p(gy), p(s), p(tau), B, S, K, ctx.hop, p(work), nbytes, p(gs), p(gtau), device=s.device)
        return gs, gtau, None


def _check(signal, delay, hop):
    """Every refusal, shapes first: ValueError before any launch.  The checks of values are flags read in one transfer."""
    for name, t in (("signal", signal), ("delay", delay)):
        if not isinstance(t, torch.Tensor) or not t.is_floating_point():
            raise ValueError(f"propagate: {name} must be a floating-point tensor")
    if isinstance(hop, bool) or not isinstance(hop, int) or hop <= 0:
        raise ValueError(f"propagate: hop = {hop!r} is not a positive int (the samples between two frames)")
    if signal.dim() < 1 or signal.shape[-1] < 1 or signal.numel() < 1:
        raise ValueError(f"propagate: signal must be (..., S) with S >= 1 and no empty dimension, got {tuple(signal.shape)}")
    if delay.dim() < 1 or delay.shape[-1] < 1:
        raise ValueError(f"propagate: delay must be (..., K) with K >= 1, got {tuple(delay.shape)}")
    lead = signal.shape[:-1]
    try:
        ok = torch.broadcast_shapes(delay.shape[:-1], lead) == lead
    except RuntimeError:
        ok = False
    if not ok:
        raise ValueError(f"propagate: delay {tuple(delay.shape)} = (..., K) does not broadcast against the leading dimensions "
                         f"{tuple(lead)} of signal")
    if math.prod(lead) > MAX_ROWS:
        raise ValueError(f"propagate: {math.prod(lead)} rows, at most {MAX_ROWS} per call")
    _hip.require_gpu(signal, delay)
    d = delay.detach().double().reshape(-1, delay.shape[-1])
    dev = d.device
    if d.shape[1] > 1:
        step = (d[:, 1:] - d[:, :-1]).abs()
        step = torch.where(torch.isfinite(step), step, torch.zeros_like(step))  # (a non-finite delay is named as such below)
        worst, at = step.reshape(-1).max(0)
    else:
        worst, at = torch.zeros((), dtype=torch.float64, device=dev), torch.zeros((), dtype=torch.int64, device=dev)
    flags = torch.stack([torch.isfinite(signal.detach()).all().to(dev, torch.float64), torch.isfinite(d).all().double(),
                         (d >= 0).logical_or(torch.isnan(d)).all().double(), worst, at.double()]).tolist()
    if not flags[0]:
        raise ValueError("propagate: signal is not finite")
    if not flags[1]:
        raise ValueError("propagate: delay is not finite")
    if not flags[2]:
        raise ValueError("propagate: a delay is negative (the line is causal: delay >= 0 samples)")
    if flags[3] > hop * MAX_SLOPE:
        row, frame = divmod(int(flags[4]), d.shape[1] - 1)
        raise ValueError(f"propagate: the delay of row {row} changes by {flags[3]:g} samples between frames {frame} and "
                         f"{frame + 1}, {flags[3] / hop:.3g} of the speed of sound (hop = {hop}); at most {MAX_SLOPE:g} - "
                         "slow the path down")


def propagate(signal, delay, hop):
    """``signal`` (..., S) delayed by ``delay`` (..., K) samples, the delay at K control frames ``hop`` samples apart (linear
    in between, the last frame held; K = 1 is a constant delay), broadcast against the leading dimensions of ``signal``.
    Returns the shape and dtype of ``signal``.  Autograd reaches both inputs, each gradient computed only where needed.
    HIP tensors only: there is no CPU path (RuntimeError).  ValueError before any launch: wrong shapes, non-finite inputs,
    a negative delay, a step between two frames above ``hop`` / 2 samples (a receiver at Mach 0.5; the message names the row,
    the frame and the speed ratio), ``hop`` not a positive int, more than 65535 rows."""
    _check(signal, delay, hop)
    S, K = signal.shape[-1], delay.shape[-1]
    lead = signal.shape[:-1]
    s2 = signal.reshape(-1, S).float()
    tau2 = delay.to(signal.device).double().expand(*lead, K).reshape(-1, K)
    return _Delay.apply(s2, tau2, hop).to(signal.dtype).reshape(signal.shape)
