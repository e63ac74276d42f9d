"""Room response: a differentiable long FIR convolution (ds_fir_fwd / ds_fir_bwd, csrc/fir.hip).

A recorded clip is the radiated sound coloured by a microphone and a room.  ``biquad.ParametricEQ`` colours; a room is early
reflections and a decaying tail that run for thousands of samples.  ``fir_convolve`` convolves rendered rows with responses
of up to 65536 taps, causal, from rest, cut at the length of the row,

    y[b,t] = sum_{j=0..min(t, L-1)} h[b mod H, j] x[b, t-j],

in the direct form and in fp64 on the device, with exact gradients to the signal and to every tap.  ``RoomResponse`` is the
trainable impulse-response reverb of DDSP that goes between a render and ``MSSLoss``: a fixed dry tap and a trainable tail.
"""
import math

import torch
from torch import nn

from .. import _hip

MAX_TAPS = 65536  # DS_FIR_MAX_TAPS
MAX_ROWS = 65535  # DS_FIR_MAX_ROWS


class _Fir(torch.autograd.Function):
    """y (B, N) fp32 from x (B, N) fp32 and h (H, L) fp64; gradients for both, NULL for the one nobody needs."""

    @staticmethod
    def forward(ctx, x, h):
        x, h = x.detach().contiguous(), h.detach().contiguous()
        (B, N), (H, L) = x.shape, h.shape
        y = torch.empty_like(x)
        p = _hip.ptr
        _hip.launch("ds_fir_fwd", p(x), p(h), B, H, N, L, p(y), device=x.device)
        ctx.save_for_backward(x, h)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, h = ctx.saved_tensors
        need_x, need_h = ctx.needs_input_grad
        if not (need_x or need_h):
            return None, None
        (B, N), (H, L) = x.shape, h.shape
        gy = gy.float().contiguous()
        work, nbytes = _hip.workspace("ds_fir_workspace_bytes", B, H, N, L, device=x.device) if need_h else (None, 0)
        gx = torch.empty_like(x) if need_x else None
        gh = torch.empty_like(h) if need_h else None
        p = _hip.ptr
        _hip.launch("ds_fir_bwd", p(gy), p(x), p(h), B, H, N, L, p(work), nbytes, p(gx), p(gh), device=x.device)
        return gx, gh


def fir_convolve(x, h):
    """``x`` (N,) or (B, N) convolved with ``h`` (L,) or (H, L): B a multiple of H, row b uses response b mod H (H = 1: one
    response for all rows; H = the number of channels, the channel varying fastest: one per channel; H = B: one per row).
    Causal, zero initial state, the result cut at N; L may exceed N.  fp64 arithmetic on the device, fp32 signal in and out;
    returns the shape and dtype of ``x``.  Autograd reaches ``x`` and ``h``.  A unit tap at lag k shifts ``x`` by k bit for bit.
    ValueError before any device call: wrong ranks, empty operands, a B that is no multiple of H, more than 65536 taps, more
    than 65535 rows.  HIP tensors only: there is no CPU path (RuntimeError)."""
    for name, t in (("x", x), ("h", h)):
        if not isinstance(t, torch.Tensor) or not t.is_floating_point():
            raise ValueError(f"fir_convolve: {name} must be a floating-point tensor")
    if x.dim() not in (1, 2):
        raise ValueError(f"fir_convolve: x must be (N,) or (B, N), got {tuple(x.shape)}")
    if h.dim() not in (1, 2):
        raise ValueError(f"fir_convolve: h must be (L,) or (H, L), got {tuple(h.shape)}")
    if x.numel() < 1:
        raise ValueError(f"fir_convolve: empty signal {tuple(x.shape)}")
    if h.numel() < 1:
        raise ValueError(f"fir_convolve: empty response {tuple(h.shape)}")
    B = x.shape[0] if x.dim() == 2 else 1
    H, L = (h.shape[0] if h.dim() == 2 else 1), h.shape[-1]
    if H > B or B % H:
        raise ValueError(f"fir_convolve: {B} row{'s' if B != 1 else ''} is not a multiple of the {H} responses")
    if L > MAX_TAPS:
        raise ValueError(f"fir_convolve: {L} taps, at most {MAX_TAPS}")
    if B > MAX_ROWS:
        raise ValueError(f"fir_convolve: {B} rows, at most {MAX_ROWS} per call")
    _hip.require_gpu(x)
    return _Fir.apply(x.reshape(B, -1).float(), h.to(x.device).double().reshape(H, L)).to(x.dtype).reshape(x.shape)


class RoomResponse(nn.Module):
    """``n_responses`` impulse responses of ``n_taps`` taps: a fixed dry tap ``h[:, 0] = 1`` followed by the trainable ``ir``
    (n_responses, n_taps - 1), fp64.  ``init="zero"``: the module is the identity, bit for bit, and training can only add a
    room.  ``init="decay"``: DDSP's exponential-decay initialisation - Gaussian noise from ``seed`` times
    ``10^(wet_db / 20) exp(-6.91 t / rt60)``, t [s] the tap's lag: the envelope is 60 dB down at ``rt60`` [s]."""

    def __init__(self, n_responses, n_taps, sample_rate, init="zero", rt60=None, wet_db=None, seed=0):
        super().__init__()
        H, L = int(n_responses), int(n_taps)
        if H < 1 or L < 1 or L > MAX_TAPS:
            raise ValueError(f"RoomResponse: {H} responses of {L} taps; at least 1 of each, at most {MAX_TAPS} taps")
        if init not in ("zero", "decay"):
            raise ValueError(f"RoomResponse: init = {init!r} is neither 'zero' nor 'decay'")
        self.sample_rate = float(sample_rate)
        ir = torch.zeros((H, L - 1), dtype=torch.float64)
        if init == "decay":
            if rt60 is None or wet_db is None or not float(rt60) > 0:
                raise ValueError("RoomResponse: init='decay' needs rt60 > 0 [s] and wet_db")
            noise = torch.randn((H, L - 1), dtype=torch.float64, generator=torch.Generator().manual_seed(int(seed)))
            ir = noise * self.decay_envelope(L, self.sample_rate, rt60, wet_db)
        self.ir = nn.Parameter(ir)

    @staticmethod
    def decay_envelope(n_taps, sample_rate, rt60, wet_db):
        """(n_taps - 1,) fp64: ``10^(wet_db / 20) exp(-6.91 t / rt60)`` at the lags 1 .. n_taps - 1 of the trainable taps."""
        t = torch.arange(1, int(n_taps), dtype=torch.float64) / float(sample_rate)
        return 10.0 ** (float(wet_db) / 20.0) * torch.exp(-6.91 * t / float(rt60))

    def impulse_response(self):
        """(H, L) fp64: the dry tap, then ``ir``."""
        return torch.cat([torch.ones_like(self.ir[:, :1]), self.ir], 1)

    def forward(self, audio):
        """``audio`` (..., time) through the responses; the leading dimensions are flattened to rows."""
        return fir_convolve(audio.reshape(-1, audio.shape[-1]), self.impulse_response()).reshape(audio.shape)

    def response(self, freqs):
        """The complex frequency response sum_j h[j] e^{-i w j} at ``freqs`` [Hz], (H, ...) in torch (complex128,
        differentiable)."""
        h = self.impulse_response()
        w = 2.0 * math.pi * torch.as_tensor(freqs, dtype=torch.float64, device=h.device) / self.sample_rate
        lag = torch.arange(h.shape[1], dtype=torch.float64, device=h.device)
        phase = w[..., None] * lag
        return torch.einsum("...j,rj->r...", torch.polar(torch.ones_like(phase), -phase), h.to(torch.complex128))
