"""Recording chain: a differentiable cascade of second-order sections (ds_biquad_fwd / ds_biquad_bwd, csrc/biquad.hip).

A recorded clip is the radiated sound coloured by a microphone and a room.  ``biquad_cascade`` filters rendered rows with
S biquads, each a row ``b0 b1 b2 a1 a2`` (a0 = 1), zero initial state,

    w[n] = u[n] - a1 w[n-1] - a2 w[n-2],    v[n] = b0 w[n] + b1 w[n-1] + b2 w[n-2],    section s + 1 reads the v of section s,

with exact gradients to the signal and to every coefficient.  The RBJ cookbook designs (``highpass_coeffs`` ...) are plain
torch in fp64 and differentiable in f0, Q and the gain; ``highpass_biquad`` / ``lowpass_biquad`` carry torchaudio's
signatures, and ``ParametricEQ`` is the trainable response model that goes between a render and ``MSSLoss``.
"""
import math

import torch
from torch import nn

from .. import _hip

MAX_SECTIONS = 16  # DS_BIQUAD_MAX_SECTIONS
MAX_ROWS = 65535   # DS_BIQUAD_MAX_ROWS


class _Biquad(torch.autograd.Function):
    """y (B, N) fp32 from x (B, N) fp32 and sos (S, 5) or (B, S, 5) fp64; gradients for both."""

    @staticmethod
    def forward(ctx, x, sos):
        x, sos = x.detach().contiguous(), sos.detach().contiguous()
        B, N = x.shape
        S, per_clip = sos.shape[-2], int(sos.dim() == 3)
        y = torch.empty_like(x)
        p = _hip.ptr
        _hip.launch("ds_biquad_fwd", p(x), p(sos), per_clip, B, N, S, p(y), device=x.device)
        ctx.save_for_backward(x, sos)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, sos = ctx.saved_tensors
        if not (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]):
            return None, None
        B, N = x.shape
        S, per_clip = sos.shape[-2], int(sos.dim() == 3)
        gy = gy.float().contiguous()
        work, nbytes = _hip.workspace("ds_biquad_workspace_bytes", B, N, S, device=x.device)
        gx = torch.empty_like(x)
        gsos = torch.empty((B, S, 5), dtype=torch.float64, device=x.device)
        p = _hip.ptr
        _hip.launch("ds_biquad_bwd", p(gy), p(x), p(sos), per_clip, B, N, S, p(work), nbytes, p(gx), p(gsos), device=x.device)
        return gx, (gsos if per_clip else gsos.sum(0))


def unstable_sections(sos):
    """Indices (into the flattened leading dimensions) of the rows ``b0 b1 b2 a1 a2`` whose poles are not strictly inside
    the unit circle: the triangle |a2| < 1, |a1| < 1 + a2."""
    a1, a2 = sos[..., 3].reshape(-1), sos[..., 4].reshape(-1)
    ok = (a2.abs() < 1) & (a1.abs() < 1 + a2)
    return torch.nonzero(~ok).reshape(-1).tolist()


def biquad_cascade(x, sos, check=False):
    """``x`` (N,) or (B, N) through the cascade ``sos``: (S, 5) shared by the rows or (B, S, 5) per row, each row
    ``b0 b1 b2 a1 a2`` with a0 = 1; or six columns, scipy's ``b0 b1 b2 a0 a1 a2``, divided through by a0 (in torch: the
    gradient passes).  fp64 arithmetic on the device, fp32 signal in and out; returns the shape and dtype of ``x``.
    Autograd reaches ``x`` and ``sos``.  ``check=True`` tests |a2| < 1 and |a1| < 1 + a2 on the host and raises ValueError
    naming the section (one synchronisation; off by default: unstable coefficients give inf / NaN, nothing worse).
    ValueError before any device call: wrong ranks or column counts, a B that does not match, more than 16 sections, an
    empty signal, more than 65535 rows.  HIP tensors only: there is no CPU path (RuntimeError)."""
    for name, t in (("x", x), ("sos", sos)):
        if not isinstance(t, torch.Tensor) or not t.is_floating_point():
            raise ValueError(f"biquad_cascade: {name} must be a floating-point tensor")
    if x.dim() not in (1, 2):
        raise ValueError(f"biquad_cascade: x must be (N,) or (B, N), got {tuple(x.shape)}")
    if sos.dim() not in (2, 3) or sos.shape[-1] not in (5, 6):
        raise ValueError(f"biquad_cascade: sos must be (S, 5), (B, S, 5), (S, 6) or (B, S, 6), got {tuple(sos.shape)}")
    if x.shape[-1] < 1 or x.numel() < 1:
        raise ValueError(f"biquad_cascade: empty signal {tuple(x.shape)}")
    S = sos.shape[-2]
    if S < 1:
        raise ValueError("biquad_cascade: no section")
    if S > MAX_SECTIONS:
        raise ValueError(f"biquad_cascade: {S} sections, at most {MAX_SECTIONS}")
    B = x.shape[0] if x.dim() == 2 else 1
    if sos.dim() == 3 and sos.shape[0] != B:
        raise ValueError(f"biquad_cascade: sos is per clip with B = {sos.shape[0]}, x has {B} row{'s' if B != 1 else ''}")
    if B > MAX_ROWS:
        raise ValueError(f"biquad_cascade: {B} rows, at most {MAX_ROWS} per call")
    _hip.require_gpu(x)
    c = sos.to(x.device).double()
    if c.shape[-1] == 6:
        c = torch.cat([c[..., :3], c[..., 4:]], -1) / c[..., 3:4]
    if check:
        bad = unstable_sections(c.detach())
        if bad:
            where = f"section {bad[0] % S}" + (f" of row {bad[0] // S}" if c.dim() == 3 else "")
            raise ValueError(f"biquad_cascade: {where} is unstable (needs |a2| < 1 and |a1| < 1 + a2)")
    return _Biquad.apply(x.reshape(B, -1).float(), c).to(x.dtype).reshape(x.shape)


# ------------------------------------------------------------------------------------------ RBJ cookbook designs
def _design(sample_rate, f0, Q, gain_db=None):
    """(cos w0, alpha, A) in fp64, broadcast against each other; plain numbers become tensors."""
    ref = next((t for t in (f0, Q, gain_db) if isinstance(t, torch.Tensor)), None)
    dev = ref.device if ref is not None else None
    f0, Q = (torch.as_tensor(t, dtype=torch.float64, device=dev) for t in (f0, Q))
    w0 = 2.0 * math.pi * f0 / float(sample_rate)
    alpha = torch.sin(w0) / (2.0 * Q)
    A = None
    if gain_db is not None:
        A = 10.0 ** (torch.as_tensor(gain_db, dtype=torch.float64, device=dev) / 40.0)
    return torch.cos(w0), alpha, A


def _rows(b0, b1, b2, a0, a1, a2):
    b0, b1, b2, a0, a1, a2 = torch.broadcast_tensors(b0, b1, b2, a0, a1, a2)
    return torch.stack([b0, b1, b2, a1, a2], -1) / a0.unsqueeze(-1)


def lowpass_coeffs(sample_rate, f0, Q=0.707):
    """(..., 5) fp64 rows ``b0 b1 b2 a1 a2`` of the cookbook's low-pass; Q = 2^-0.5 is the second-order Butterworth."""
    c, al, _ = _design(sample_rate, f0, Q)
    return _rows((1 - c) / 2, 1 - c, (1 - c) / 2, 1 + al, -2 * c, 1 - al)


def highpass_coeffs(sample_rate, f0, Q=0.707):
    """The cookbook's high-pass."""
    c, al, _ = _design(sample_rate, f0, Q)
    return _rows((1 + c) / 2, -(1 + c), (1 + c) / 2, 1 + al, -2 * c, 1 - al)


def peaking_coeffs(sample_rate, f0, Q=0.707, gain_db=0.0):
    """The cookbook's peaking EQ; at 0 dB numerator and denominator are equal: the identity."""
    c, al, A = _design(sample_rate, f0, Q, gain_db)
    return _rows(1 + al * A, -2 * c, 1 - al * A, 1 + al / A, -2 * c, 1 - al / A)


def lowshelf_coeffs(sample_rate, f0, Q=0.707, gain_db=0.0):
    """The cookbook's low shelf (alpha = sin w0 / (2 Q))."""
    c, al, A = _design(sample_rate, f0, Q, gain_db)
    r = 2 * torch.sqrt(A) * al
    return _rows(A * ((A + 1) - (A - 1) * c + r), 2 * A * ((A - 1) - (A + 1) * c), A * ((A + 1) - (A - 1) * c - r),
                 (A + 1) + (A - 1) * c + r, -2 * ((A - 1) + (A + 1) * c), (A + 1) + (A - 1) * c - r)


def highshelf_coeffs(sample_rate, f0, Q=0.707, gain_db=0.0):
    """The cookbook's high shelf."""
    c, al, A = _design(sample_rate, f0, Q, gain_db)
    r = 2 * torch.sqrt(A) * al
    return _rows(A * ((A + 1) + (A - 1) * c + r), -2 * A * ((A - 1) + (A + 1) * c), A * ((A + 1) + (A - 1) * c - r),
                 (A + 1) - (A - 1) * c + r, 2 * ((A - 1) - (A + 1) * c), (A + 1) - (A - 1) * c - r)


# ------------------------------------------------------------------------------------- torchaudio's two functions
def _apply_one(name, coeffs, waveform, clamp):
    if not isinstance(waveform, torch.Tensor) or not waveform.is_floating_point():
        raise ValueError(f"{name}: waveform must be a floating-point tensor")
    if waveform.dim() < 1 or waveform.numel() < 1:
        raise ValueError(f"{name}: empty waveform {tuple(waveform.shape)}")
    y = biquad_cascade(waveform.reshape(-1, waveform.shape[-1]), coeffs.reshape(1, 5)).reshape(waveform.shape)
    return y.clamp(-1.0, 1.0) if clamp else y


def highpass_biquad(waveform, sample_rate, cutoff_freq, Q=0.707, clamp=True):
    """``torchaudio.functional.highpass_biquad``: the cookbook high-pass applied to ``waveform`` (..., time), leading
    dimensions flattened to rows.  ``clamp=True`` clips the result to [-1, 1], because torchaudio's ``biquad`` calls
    ``lfilter`` with its default ``clamp=True``.  torchaudio is not a dependency: signature, coefficients and the clamp are
    restated from its published source, not compared against it (the coefficients are held against scipy's Butterworth)."""
    return _apply_one("highpass_biquad", highpass_coeffs(sample_rate, cutoff_freq, Q), waveform, clamp)


def lowpass_biquad(waveform, sample_rate, cutoff_freq, Q=0.707, clamp=True):
    """``torchaudio.functional.lowpass_biquad``; see ``highpass_biquad``."""
    return _apply_one("lowpass_biquad", lowpass_coeffs(sample_rate, cutoff_freq, Q), waveform, clamp)


# --------------------------------------------------------------------------------------------------- the module
class ParametricEQ(nn.Module):
    """``n_sections`` peaking sections with trainable centre, width and gain, in front of them a fixed high-pass at
    ``low_cut`` Hz where given.  Parameters per section: ``log_f0`` (read through a sigmoid onto the log-frequency range
    [F_MIN, 0.49 sample_rate], so f0 stays below Nyquist), ``log_Q`` and ``gain_db``: any parameter value is a stable filter.
    ``f0``, ``Q``, ``gain_db``: numbers or sequences of length n_sections, the initial values.  At 0 dB a section is the
    identity."""

    F_MIN = 10.0

    def __init__(self, n_sections, sample_rate, f0, Q=0.707, gain_db=0.0, low_cut=None):
        super().__init__()
        n = int(n_sections)
        if n < 1 or n + (low_cut is not None) > MAX_SECTIONS:
            raise ValueError(f"ParametricEQ: {n} sections{' and a low cut' if low_cut is not None else ''}, "
                             f"1 to {MAX_SECTIONS} in all")
        self.sample_rate = float(sample_rate)
        self.lo, self.hi = math.log(self.F_MIN), math.log(0.49 * self.sample_rate)
        full = lambda v: torch.as_tensor(v, dtype=torch.float64).expand(n).clone()
        f0, Q = full(f0), full(Q)
        if not bool(((f0 > self.F_MIN) & (f0 < 0.49 * self.sample_rate)).all()) or not bool((Q > 0).all()):
            raise ValueError(f"ParametricEQ: f0 must lie in ({self.F_MIN:g}, {0.49 * self.sample_rate:g}) Hz and Q above 0")
        u = (torch.log(f0) - self.lo) / (self.hi - self.lo)
        self.log_f0 = nn.Parameter(torch.log(u) - torch.log1p(-u))  # the logit
        self.log_Q = nn.Parameter(torch.log(Q))
        self.gain_db = nn.Parameter(full(gain_db))
        self.low_cut = None if low_cut is None else float(low_cut)

    def f0(self):
        return torch.exp(self.lo + (self.hi - self.lo) * torch.sigmoid(self.log_f0))

    def coefficients(self):
        """(S, 5) fp64: the low cut first where there is one."""
        sos = peaking_coeffs(self.sample_rate, self.f0(), torch.exp(self.log_Q), self.gain_db)
        if self.low_cut is not None:
            sos = torch.cat([highpass_coeffs(self.sample_rate, self.low_cut).to(sos.device).reshape(1, 5), sos], 0)
        return sos

    def forward(self, audio):
        """``audio`` (..., time) through the cascade."""
        return biquad_cascade(audio.reshape(-1, audio.shape[-1]), self.coefficients()).reshape(audio.shape)

    def response(self, freqs):
        """The complex frequency response H(e^{i w}) at ``freqs`` [Hz], in torch (complex128, differentiable)."""
        sos = self.coefficients()
        w = 2.0 * math.pi * torch.as_tensor(freqs, dtype=torch.float64, device=sos.device) / self.sample_rate
        z1 = torch.polar(torch.ones_like(w), -w)[..., None]  # z^-1
        num = sos[:, 0] + sos[:, 1] * z1 + sos[:, 2] * z1 * z1
        den = 1.0 + sos[:, 3] * z1 + sos[:, 4] * z1 * z1
        return (num / den).prod(-1)
