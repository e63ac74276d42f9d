"""Point clouds of the early-phase spectral loss on HIP kernels (csrc/specpoints.hip).

What the reference's ``spec2point`` (src/ddsp/mss_loss.py:19-48) makes of a spectrogram on the 'geomloss' path
(:104-117), for the linear and the log cloud of one scale in one call: ``spectral_points(P, freq, sample_rate, scale)``
takes the power spectrogram ``ds_stft_power`` left and returns ``(lin (B, F, 4), log (B, int(F * scale), 4))`` -

- columns 0..2: the row's time profile resampled linearly to three values, of ``P`` for ``lin`` and of
  ``(log2(P + eps) - log2(eps)) / 40`` for ``log`` (no log spectrogram is written);
- column 3: ``row / bins``, overwritten near every entry of ``freq`` by the reference's ``(bin(freq) -+ w) / bins`` in
  the reference's order - the only place a gradient enters; it goes to ``freq``, nothing goes to ``P``.

Where two entries write one row the reference's ``index_put`` leaves the winner to the device; here it is defined: a
later write overrides an earlier one, and inside one write the highest flat index of ``freq`` wins (what a sequential
loop does).  The gradient is the one autograd gives through the reference: the backward of ``index_put_`` credits
every entry of the write that owns a row, so each copy of an expanded ``freq`` receives the row's gradient and the
expand's backward adds them up - here the copies are collapsed into one entry whose gradient is scaled by their number.
The arithmetic of column 3 is what torch performs on device tensors.  Device tensors only; no host synchronisation.
"""
import torch

from .. import _hip


def collapse_expanded(freq):
    """``freq`` with every stride-0 dimension sliced to length 1.  All copies along such a dimension carry one value and the
    flat order between the entries that remain is unchanged, so the clouds are the same; autograd's backward of the slice
    and of the expand hands the kept copy's gradient to the base (the other copies add exact zeros)."""
    for d in range(freq.dim()):
        if freq.shape[d] > 1 and freq.stride(d) == 0:
            freq = freq.narrow(d, 0, 1)
    return freq


class _SpecPoints(torch.autograd.Function):
    """(P (B, F, T), freq (E,) or None) -> (lin, log); backward to freq."""

    @staticmethod
    def forward(ctx, P, freq, sample_rate, fclip, eps, copies):
        B, F_, T = P.shape
        lin = torch.empty((B, F_, 4), dtype=torch.float32, device=P.device)
        log = torch.empty((B, fclip, 4), dtype=torch.float32, device=P.device)
        win = None if freq is None else torch.empty(F_ + fclip, dtype=torch.int64, device=P.device)
        E = 0 if freq is None else freq.numel()
        p = _hip.ptr
        _hip.launch("ds_spec_points_fwd", p(P), B, F_, T, eps, fclip, p(freq), E, sample_rate, p(win), p(lin), p(log), device=P.device)
        if freq is not None:
            ctx.save_for_backward(freq, win)
        ctx.meta = (B, F_, fclip, sample_rate, copies)
        return lin, log

    @staticmethod
    def backward(ctx, g_lin, g_log):
        if not ctx.saved_tensors or not ctx.needs_input_grad[1]:
            return None, None, None, None, None, None
        freq, win = ctx.saved_tensors
        B, F_, fclip, sample_rate, copies = ctx.meta
        g_lin = None if g_lin is None else g_lin.detach().float().contiguous()
        g_log = None if g_log is None else g_log.detach().float().contiguous()
        g_freq = torch.empty_like(freq)
        p = _hip.ptr
        _hip.launch("ds_spec_points_bwd", p(g_lin), p(g_log), B, F_, fclip, p(freq), freq.numel(), sample_rate, p(win), float(copies),
                    p(g_freq), device=freq.device)
        return None, g_freq, None, None, None, None


def spectral_points(P, freq=None, sample_rate=None, scale=1.0, eps=1e-7):
    """Both point clouds of one scale: ``(lin (B, F, 4), log (B, int(F * scale), 4))`` f32 from the power spectrogram
    ``P (B, F, T)``.  ``freq``: mode frequencies in Hz, any shape (an expanded view is collapsed first, a dense tensor is
    taken as is), with ``sample_rate``; None for a target cloud.  The gradient goes to ``freq`` only."""
    if not torch.is_tensor(P) or not P.is_floating_point() or P.dim() != 3:
        raise ValueError("spectral_points: P must be a floating-point (batch, freq, time) tensor")
    B, F_, T = P.shape
    if B < 1 or F_ < 1 or T < 1:
        raise ValueError(f"spectral_points: P {tuple(P.shape)} has an empty dimension")
    fclip = int(F_ * scale)
    if not 1 <= fclip <= F_:
        raise ValueError(f"spectral_points: scale={scale!r} keeps {fclip} of {F_} bins; need 1 <= int(F * scale) <= F")
    if not (isinstance(eps, (int, float)) and 0 < eps < float("inf")):
        raise ValueError(f"spectral_points: eps={eps!r} must be a positive finite number")
    if freq is not None:
        if not torch.is_tensor(freq) or not freq.is_floating_point():
            raise ValueError("spectral_points: freq must be a floating-point tensor")
        if freq.numel() < 1:
            raise ValueError("spectral_points: freq is empty")
        if sample_rate is None or int(sample_rate) != sample_rate or int(sample_rate) // 2 < 1:
            raise ValueError(f"spectral_points: freq needs an integral sample_rate >= 2, got {sample_rate!r}")
        if freq.device != P.device:
            raise ValueError("spectral_points: P and freq must live on one device")
    _hip.require_gpu(P, freq)
    P = P.detach().float().contiguous()
    copies = 1
    if freq is not None:
        total = freq.numel()
        freq = collapse_expanded(freq).reshape(-1).float().contiguous()
        copies = total // freq.numel()  # every kept entry stands for this many equal ones
    return _SpecPoints.apply(P, freq, 0 if freq is None else int(sample_rate), fclip, float(eps), copies)
