"""Filtered-noise branch - host-side mirror of reference src/ddsp/filtered_noise.py: the ``FilteredNoise`` module, its native
autograd function (ds_filtered_noise_fwd / ds_filtered_noise_bwd, csrc/filtered_noise.hip) and the reference's torch.fft
formulation for what the kernels do not take."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _hip
from .utils import modifed_sigmoid

FN_MAX_COEFF, FN_MAX_FRAME = 129, 256  # filter_coeff_length / frame_length csrc/filtered_noise.hip holds in LDS (FN_MAXL, FN_MAXF)


def _filtered_noise_torch(bank, noise, sample_num, frame_length, attenuate_gain):
    """The reference's formulation (src/ddsp/filtered_noise.py:20-67) op by op, torch.fft plumbing: CPU tensors, sizes
    outside the native range, and a noise that itself requires grad."""
    mag = modifed_sigmoid(bank)
    B, nf, L = mag.shape
    taps = 2 * L - 1
    ir = torch.fft.irfft(torch.complex(mag, torch.zeros_like(mag)), n=taps, dim=-1)  # zero-phase
    ir = torch.roll(ir, L - 1, dims=-1) * torch.hann_window(taps, dtype=torch.float32, device=mag.device)
    nfft = taps + frame_length - 1
    frames = torch.fft.irfft(torch.fft.rfft(noise, n=nfft) * torch.fft.rfft(ir, n=nfft), n=nfft)
    frames = frames * attenuate_gain
    total = (nf - 1) * frame_length + nfft
    out = F.fold(frames.transpose(1, 2), output_size=(1, total), kernel_size=(1, nfft),
                 stride=(1, frame_length)).reshape(B, total)
    return out[:, :sample_num]


class _FilteredNoiseFn(torch.autograd.Function):
    """out (B, S) = overlap-add of gain (noise_f * h_f), h_f the Hann-windowed linear-phase FIR of bank[:, f]
    (ds_filtered_noise_fwd / ds_filtered_noise_bwd, one launch each); the gradient goes to the bank only."""

    @staticmethod
    def forward(ctx, bank, noise, S, frame_length, gain):
        _hip.require_gpu(bank, noise)
        bank = bank.detach().float().contiguous()
        noise = noise.detach().float().contiguous()
        B, nf, L = bank.shape
        if nf != S // frame_length + 1 or noise.shape != (B, nf, frame_length):
            raise ValueError(f"filtered noise: bank {tuple(bank.shape)} / noise {tuple(noise.shape)} do not fit "
                             f"(noise_num, {S // frame_length + 1}, filter_coeff_length / {frame_length})")
        out = torch.empty((B, S), dtype=torch.float32, device=bank.device)
        p = _hip.ptr
        _hip.launch("ds_filtered_noise_fwd", p(bank), p(noise), B, S, L, frame_length, float(gain), p(out), device=bank.device)
        ctx.save_for_backward(bank, noise)
        ctx.S, ctx.frame_length, ctx.gain = S, frame_length, float(gain)
        return out

    @staticmethod
    def backward(ctx, gy):
        bank, noise = ctx.saved_tensors
        B, nf, L = bank.shape
        gy = gy.float().contiguous()
        gc = torch.empty_like(bank)
        p = _hip.ptr
        _hip.launch("ds_filtered_noise_bwd", p(gy), p(bank), p(noise), B, ctx.S, L, ctx.frame_length, ctx.gain, p(gc),
                    device=bank.device)
        return gc, None, None, None, None


class FilteredNoise(nn.Module):
    """Time-varying filtered white noise (DDSP style): per 64-sample frame a learnable magnitude response
    (65 bins) is turned into a Hann-windowed linear-phase FIR, applied to a fresh white-noise frame, and the frames are
    overlap-added.  Interface of reference src/ddsp/filtered_noise.py:7-67 (``coefficient_bank`` parameter,
    ``forward() -> (noise_num, sample_num)``).  On a HIP device, with ``filter_coeff_length`` in [2, 129] and
    ``frame_length`` in [1, 256], the whole map is ONE kernel forward and one backward (ds_filtered_noise_fwd / _bwd:
    direct sums, no FFT, no temporaries, deterministic; the gradient reaches ``coefficient_bank``); CPU tensors, other
    sizes and an injected noise that requires grad take the reference's torch.fft formulation."""

    def __init__(self, noise_num, sample_num, filter_coeff_length=65, frame_length=64, attenuate_gain=1.0,
                 device="cuda"):
        super().__init__()
        self.noise_num, self.sample_num = noise_num, sample_num
        self.filter_coeff_length, self.frame_length, self.attenuate_gain = filter_coeff_length, frame_length, attenuate_gain
        self.coefficient_bank = nn.Parameter(torch.zeros(noise_num, sample_num // frame_length + 1, filter_coeff_length))
        self.coefficient_bank.data.uniform_(-1, 1)

    def forward(self, noise=None):
        """noise: optional (noise_num, frames, frame_length) tensor in [-1, 1) replacing the internal draw (tests)."""
        bank = self.coefficient_bank
        B, nf, L = bank.shape
        if noise is None:
            noise = torch.rand(B, nf, self.frame_length, device=bank.device) * 2 - 1
        native = (bank.is_cuda and noise.is_cuda and not noise.requires_grad and self.sample_num >= 1
                  and 2 <= L <= FN_MAX_COEFF and 1 <= self.frame_length <= FN_MAX_FRAME)
        if native:
            return _FilteredNoiseFn.apply(bank, noise, int(self.sample_num), int(self.frame_length), float(self.attenuate_gain))
        return _filtered_noise_torch(bank, noise, self.sample_num, self.frame_length, self.attenuate_gain)
