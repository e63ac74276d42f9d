"""Damped-oscillator modules - host-side mirror of reference src/ddsp/oscillator.py.

Class names, constructor arguments, ``forward`` signatures, returned shapes/dtypes and the
``damped_freq`` attribute follow the reference; the (A, m, S) signal path itself is ONE fused HIP
kernel (``ds_osc_bank_fwd`` / ``ds_osc_bank_bwd``) wrapped in a ``torch.autograd.Function``; a force of more
than 512 taps, or one that is itself trained (``train_forces=True``), renders through the recursive-resonator
kernels (``ds_osc_driven_fwd`` / ``ds_osc_driven_bwd``), which also return the force gradient; a 3-D ``mode_gain``
(audio_num, K, mode_num) with ``gain_hop`` - a contact that slides while the force acts - renders through the sliding bank
(``ds_osc_slide_fwd`` / ``ds_osc_slide_bwd``); a complex ``listener_gain`` - what each mode sounds like at C listening points,
``ModalRadiator.listener_gains`` / ``listener_path_gains`` - renders (audio_num, C, sample_num) through the listener bank
(``ds_osc_listen_fwd`` / ``ds_osc_listen_bwd``); a ``listener_delay`` with it - the propagation delay of every channel,
``ModalRadiator.listener_path`` - sends the rendered channels through the fractional delay line (``delay.propagate``).
The tiny per-mode parameter algebra (softplus-weighted bins, d = (alpha + beta w0^2)/2,
w = sqrt(w0^2 - d^2)) stays in torch so autograd reaches every learnable leaf exactly as in the
reference.

This file holds the parameter modules and the ``nn.Module`` banks.  The autograd Functions and the functional entries
(``oscillator_bank`` ...) live in ``bank.py``, ``FilteredNoise`` in ``filtered_noise.py`` and ``modifed_sigmoid`` in
``utils.py`` (the last two as in the reference); every name that used to be defined here is still importable from here.
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _hip  # noqa: F401
from ..diffelastic.material_model import Material, MatSet  # noqa: F401  (re-exported like the reference)
from .bank import (FIR_MAX_FORCE, LISTEN_MAX_CHANNELS, SLIDE_HOP_UNIT, _OscBank, _OscBankTV, _OscDriven,  # noqa: F401
                   _OscListener, _OscSliding, oscillator_bank, oscillator_bank_driven, oscillator_bank_listener,
                   oscillator_bank_sliding, oscillator_bank_tv)
from .delay import propagate
from .filtered_noise import (FN_MAX_COEFF, FN_MAX_FRAME, FilteredNoise, _FilteredNoiseFn,  # noqa: F401
                             _filtered_noise_torch)
from .utils import modifed_sigmoid

class WeightedParam(nn.Module):
    """Scalar = sum_j v_j softplus(p_j) / sum softplus(p)  (reference oscillator.py:10-21)."""

    def __init__(self, values_list: torch.Tensor):
        super().__init__()
        self.values_list = values_list
        self.probablity = nn.Parameter(torch.zeros(len(values_list)))
        self.probablity.data.uniform_(-1, 1)

    def forward(self):
        p = F.softplus(self.probablity)
        p = p / p.sum()
        return (self.values_list.to(p.device) * p).sum()


class WeightedSum(nn.Module):
    """reference oscillator.py:23-35."""

    def __init__(self, dims: list, vlist: list):
        super().__init__()
        # (a plain attribute in the reference: not part of the state_dict, so checkpoints load strictly both ways)
        self.register_buffer("values_list", torch.tensor([float(v) for v in vlist], dtype=torch.float32),
                             persistent=False)
        self.params = nn.Parameter(torch.zeros(*dims, len(self.values_list)))
        self.params.data.uniform_(-4, 4)

    def forward(self):
        x = F.softplus(self.params)
        x = x / x.sum(dim=-1).unsqueeze(-1)
        return (self.values_list * x).sum(dim=-1)


class DirectValue(nn.Module):
    """reference oscillator.py:38-46."""

    def __init__(self, dims: list):
        super().__init__()
        self.value = nn.Parameter(torch.zeros(*dims))
        self.value.data.uniform_(0, 0.04)

    def forward(self):
        return modifed_sigmoid(self.value)


def _device_of(t):
    if t.is_cuda:
        return t.device
    if not torch.cuda.is_available():
        raise RuntimeError("diffsound_amd: no HIP device available (there is no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


class _BankBase(nn.Module):
    def _setup(self, forces, audio_num, mode_num, sample_num, sr, mat, train_forces=False):
        self.audio_num = audio_num
        self.sr = sr
        self.sample_num = sample_num
        self.mode_num = mode_num
        self.mat = mat
        self.force_frame_num = forces.shape[-1]
        self.train_forces = bool(train_forces)
        if self.train_forces:  # the force itself is fitted: a parameter, rendered through the driven bank
            self.force = nn.Parameter(forces.detach().reshape(audio_num, -1).float().clone())
        else:
            self.register_buffer("_force", forces.detach().reshape(audio_num, -1).float().clone(), persistent=False)
            # the reference keeps the time-flipped conv1d weight as ``forces`` (oscillator.py:80-82)
            self.forces = torch.flip(forces.reshape(audio_num, 1, -1), [-1])

    @property
    def forces(self):
        if self.train_forces:
            return torch.flip(self.force.reshape(self.audio_num, 1, -1), [-1])
        return self._forces_flipped

    @forces.setter
    def forces(self, value):
        if self.train_forces:
            raise AttributeError("forces is computed from the parameter ``force`` (train_forces=True)")
        self._forces_flipped = value

    def _force_on_device(self):
        """(device, force (A, F) on it): the buffer is moved once, a trained force stays where the module was put."""
        if self.train_forces:
            dev = _device_of(self.force)
            return dev, self.force.to(dev)
        dev = _device_of(self._force)
        if self._force.device != dev:
            self._force = self._force.to(dev)
        return dev, self._force

    def _render(self, freq_linear, alpha, beta, amp, slide=None, listen=None):
        """freq_linear (m,1) or (m,) any float dtype; alpha/beta python floats or (1,m,1) tensors; amp (A,m,1)|None;
        slide: None, or the (gain (A, K, m), hop) of ``_sliding`` - the render then goes through the sliding bank;
        listen: None, or the (hgain (A, C, m[, K]), hop) of ``_listening`` - the render then goes through the listener bank
        and returns (A, C, S)."""
        dev, force = self._force_on_device()
        f = freq_linear.reshape(self.mode_num).to(dev).double()
        w0sq = (f * (2 * np.pi)) ** 2
        if torch.is_tensor(alpha):
            alpha = alpha.reshape(self.mode_num).to(dev).double()
        if torch.is_tensor(beta):
            beta = beta.reshape(self.mode_num).to(dev).double()
        d = 0.5 * (alpha + beta * w0sq)
        w = torch.sqrt(w0sq - d ** 2)
        fd = (w / (2 * np.pi)).float()
        self.damped_freq = fd.reshape(1, self.mode_num, 1).expand(self.audio_num, self.mode_num, self.sample_num)
        a = None if amp is None else amp.reshape(self.audio_num, self.mode_num).to(dev)
        if slide is not None:
            return oscillator_bank_sliding(d, w, a, force, slide[0].to(dev), slide[1], self.sample_num, self.sr)
        if listen is not None:
            return oscillator_bank_listener(d, w, a, force, listen[0].to(dev), listen[1], self.sample_num, self.sr)
        return oscillator_bank(d, w, a, force, self.sample_num, self.sr)

    def _listening(self, listener_gain, listener_hop, slide=None, time_varying=False):
        """None for ``listener_gain`` = None: the path and the bits of a call without the keyword.  Otherwise the pair
        (hgain, hop) for the listener bank, after the checks that need no device.  ``listener_gain`` is complex: without
        ``listener_hop`` (C, mode_num) or (audio_num, C, mode_num), a listener at rest; with ``listener_hop`` - the samples
        between two frames, a positive multiple of 16 - (C, mode_num, K) or (audio_num, C, mode_num, K), a listener that
        moves (``ModalRadiator.listener_path_gains``).  A gain without the clip axis is shared by every clip.  ValueError:
        a real gain, another shape, more than 16 channels, a missing or bad hop, a 3-D ``mode_gain`` (a sliding contact
        heard by a listener that has gains of its own is not rendered here), or a time-varying render."""
        if listener_gain is None:
            if listener_hop is not None:
                raise ValueError("listener_hop goes with a listener_gain")
            return None
        A, m = self.audio_num, self.mode_num
        if not torch.is_tensor(listener_gain) or not listener_gain.is_complex():
            raise ValueError("listener_gain must be complex (ModalRadiator.listener_gains; a real gain g is g + 0i)")
        g = listener_gain
        if listener_hop is None:
            if g.dim() == 4:
                raise ValueError(f"a listener_gain with frames ({A}, C, {m}, K) needs listener_hop, the samples between two frames")
            ok = (g.dim() == 2 and g.shape[1] == m) or (g.dim() == 3 and g.shape[0] == A and g.shape[2] == m)
            if not ok:
                raise ValueError(f"listener_gain must be (C, {m}) or ({A}, C, {m}), got {tuple(g.shape)}")
            if g.dim() == 2:
                g = g.unsqueeze(0).expand(A, -1, -1)
        else:
            ok = (g.dim() == 3 and g.shape[1] == m) or (g.dim() == 4 and g.shape[0] == A and g.shape[2] == m)
            if not ok:
                raise ValueError(f"listener_gain with listener_hop must be (C, {m}, K) or ({A}, C, {m}, K), got {tuple(g.shape)}")
            if int(listener_hop) != listener_hop or listener_hop <= 0 or int(listener_hop) % SLIDE_HOP_UNIT:
                raise ValueError(f"listener_hop = {listener_hop} is not a positive multiple of {SLIDE_HOP_UNIT}")
            listener_hop = int(listener_hop)
            if g.dim() == 3:
                g = g.unsqueeze(0).expand(A, -1, -1, -1)
        if min(g.shape) < 1 or g.shape[1] > LISTEN_MAX_CHANNELS:
            raise ValueError(f"listener_gain: {g.shape[1]} channels, at least 1 and at most {LISTEN_MAX_CHANNELS} channels per call")
        if slide is not None:
            raise ValueError("a 3-D mode_gain together with listener_gain - a sliding contact heard by a listener - is not "
                             "rendered: use a 2-D mode_gain (a strike)")
        if time_varying:
            raise ValueError("listener_gain renders through the closed-form bank only: non_linear_rate must be 0 (and "
                             "forward_curve has no listener form)")
        return g, listener_hop

    def _delaying(self, listener_delay, listen):
        """None for ``listener_delay`` = None: the path and the bits of a call without the keyword.  Otherwise the delay in
        samples as (audio_num, C, K) for ``delay.propagate``, after the checks that need no device: ``listener_delay`` is
        (C, K) or (audio_num, C, K) with the C of ``listener_gain`` and, for a listener that moves, its K and its
        ``listener_hop``; with a gain at rest (no frames) K is 1.  ValueError: no ``listener_gain``, another shape, another K."""
        if listener_delay is None:
            return None
        if listen is None:
            raise ValueError("listener_delay goes with a listener_gain (ModalRadiator.listener_path returns both)")
        g = listen[0]
        A, C, K = self.audio_num, g.shape[1], (g.shape[3] if g.dim() == 4 else 1)
        t = listener_delay
        if not torch.is_tensor(t) or not t.is_floating_point() or not (
                (t.dim() == 2 and t.shape[0] == C) or (t.dim() == 3 and t.shape[0] == A and t.shape[1] == C)):
            raise ValueError(f"listener_delay must be a floating-point (C, K) or ({A}, C, K) tensor with C = {C}, got "
                             f"{tuple(t.shape) if torch.is_tensor(t) else type(t).__name__}")
        if t.shape[-1] != K:
            raise ValueError(f"listener_delay has {t.shape[-1]} frames, listener_gain has K = {K}: both share listener_hop")
        return t if t.dim() == 3 else t.unsqueeze(0).expand(A, -1, -1)

    def _propagated(self, sig, delay, listen):
        """``sig`` (audio_num, C, S) through the delay line; ``delay`` from ``_delaying`` (None: ``sig`` itself)."""
        if delay is None:
            return sig
        return propagate(sig, delay.to(sig.device), listen[1] if listen[1] is not None else SLIDE_HOP_UNIT)

    def _sliding(self, mode_gain, gain_hop, time_varying=False):
        """None for ``mode_gain`` = None or a 2-D gain (``_with_gain`` takes those).  For a 3-D gain (audio_num, K, mode_num)
        - the input gains of a contact that moves, one frame every ``gain_hop`` samples
        (``diffsound_amd.impact.ContactSurface.path_gains``) - the pair (mode_gain, gain_hop) for the sliding bank, after
        the checks that need no device: ValueError for a missing ``gain_hop``, one that is not a positive multiple of 16,
        a gain of another shape, or the time-varying render, which has no sliding form."""
        if not torch.is_tensor(mode_gain) or mode_gain.dim() != 3:
            if gain_hop is not None:
                raise ValueError("gain_hop goes with a 3-D mode_gain (audio_num, K, mode_num)")
            return None
        if gain_hop is None:
            raise ValueError("a 3-D mode_gain (audio_num, K, mode_num) needs gain_hop, the samples between two frames")
        if int(gain_hop) != gain_hop or gain_hop <= 0 or int(gain_hop) % SLIDE_HOP_UNIT:
            raise ValueError(f"gain_hop = {gain_hop} is not a positive multiple of {SLIDE_HOP_UNIT}")
        if mode_gain.shape[0] != self.audio_num or mode_gain.shape[2] != self.mode_num or mode_gain.shape[1] < 1:
            raise ValueError(f"a 3-D mode_gain must be ({self.audio_num}, K, {self.mode_num}), got {tuple(mode_gain.shape)}")
        if time_varying:
            raise ValueError("a 3-D mode_gain (a sliding contact) renders through the closed-form bank only: "
                             "non_linear_rate must be 0")
        return mode_gain, int(gain_hop)

    def _with_gain(self, amp, mode_gain):
        """``amp`` (A, m, 1) or None (unit amplitudes) times ``mode_gain`` (audio_num, mode_num): the gains of a strike
        (``diffsound_amd.impact.ContactSurface.amplitudes``) in place of, or on top of, the free amplitudes.  None
        returns ``amp`` itself - the path and the bits of a call without the keyword."""
        if mode_gain is None:
            return amp
        if not torch.is_tensor(mode_gain) or tuple(mode_gain.shape) != (self.audio_num, self.mode_num):
            raise ValueError(f"mode_gain must be a ({self.audio_num}, {self.mode_num}) tensor, got "
                             f"{tuple(mode_gain.shape) if torch.is_tensor(mode_gain) else type(mode_gain).__name__}")
        if amp is None:
            return mode_gain.float().reshape(self.audio_num, self.mode_num, 1)
        return amp * mode_gain.to(amp.device, amp.dtype).reshape(self.audio_num, self.mode_num, 1)


class TraditionalDampedOscillator(_BankBase):
    """Fixed Rayleigh damping (alpha, beta from the material), unit amplitudes
    (reference oscillator.py:246-310)."""

    def __init__(self, forces, audio_num, mode_num, sample_num, sr, mat: Material, train_forces=False):
        super().__init__()
        self._setup(forces, audio_num, mode_num, sample_num, sr, mat, train_forces)
        self.alpha = mat.alpha
        self.beta = mat.beta

    def forward(self, freq_linear, mode_gain=None, gain_hop=None, listener_gain=None, listener_hop=None, listener_delay=None):
        """``listener_gain`` (complex; see ``_listening``) returns (audio_num, C, sample_num), what C listening points hear;
        a 2-D ``mode_gain`` (a strike) still folds into the amplitudes.  A sliding contact (3-D ``mode_gain``) heard by a
        moving listener is out of scope: ValueError.  ``listener_delay`` (see ``_delaying``): the propagation delay of
        every channel in samples, (C, K) or (audio_num, C, K) at the frames of ``listener_gain``
        (``ModalRadiator.listener_path`` returns the pair) - the rendered channels then pass through ``delay.propagate``."""
        slide = self._sliding(mode_gain, gain_hop)
        listen = self._listening(listener_gain, listener_hop, slide)
        delay = self._delaying(listener_delay, listen)
        sig = self._render(freq_linear, float(self.alpha), float(self.beta),
                           None if slide else self._with_gain(None, mode_gain), slide, listen)
        sig = self._propagated(sig, delay, listen)
        w = self.damped_freq[0, :, 0].double() * (2 * np.pi)
        self.undamped_freq = freq_linear.reshape(1, self.mode_num, 1).to(w.device)
        return sig


class DampedOscillator(_BankBase):
    """Per-mode learnable alpha/beta (64 log-spaced bins) and per-(audio, mode) amplitude
    (reference oscillator.py:49-141)."""

    def __init__(self, forces, audio_num, mode_num, sample_num, sr, f_range: list, mat: Material, train_forces=False):
        super().__init__()
        self._setup(forces, audio_num, mode_num, sample_num, sr, mat, train_forces)
        bin_num = 64
        self.alpha_list = torch.exp(torch.linspace(np.log(mat.alpha / 10), np.log(mat.alpha * 10), bin_num))
        self.alpha = WeightedSum([1, mode_num, 1], list(self.alpha_list))
        self.beta_list = torch.exp(torch.linspace(np.log(mat.beta / 10), np.log(mat.beta * 10), bin_num))
        self.beta = WeightedSum([1, mode_num, 1], list(self.beta_list))
        self.amp = DirectValue([audio_num, mode_num, 1])
        # unused by forward(), kept so that the reference's checkpoints load strictly (oscillator.py:78: "just for load")
        self.noise = FilteredNoise(audio_num, 8000)

    def forward(self, freq_linear, non_linear_rate=0.0, noise_rate=0.0, mode_gain=None, gain_hop=None, listener_gain=None,
                listener_hop=None, listener_delay=None):
        """``listener_gain`` / ``listener_hop`` / ``listener_delay``: as ``TraditionalDampedOscillator.forward`` -
        (audio_num, C, sample_num); no sliding contact and no non-zero ``non_linear_rate`` with it."""
        slide = self._sliding(mode_gain, gain_hop)
        listen = self._listening(listener_gain, listener_hop, slide, time_varying=non_linear_rate != 0.0)
        delay = self._delaying(listener_delay, listen)
        amp = self.amp() if slide else self._with_gain(self.amp(), mode_gain)
        return self._propagated(self._render(freq_linear, self.alpha(), self.beta(), amp, slide, listen), delay, listen)

    def _curve_render(self, freq_linear, damping_curve):
        dev, force = self._force_on_device()
        f = freq_linear.reshape(self.mode_num).to(dev).double()
        d = curve_on_device(damping_curve, f.detach())  # the reference evaluates the curve on detached frequencies
        w0sq = (f * (2 * np.pi)) ** 2
        w = torch.sqrt(w0sq - d ** 2)
        self.damped_freq = (w / (2 * np.pi)).float().reshape(1, self.mode_num, 1)
        return oscillator_bank(d, w, None, force, self.sample_num, self.sr)

    def early(self, freq_linear, damping_curve):
        """Damping per mode from ``damping_curve``, unit amplitudes, no normalisation (reference oscillator.py:85-109)."""
        return self._curve_render(freq_linear, damping_curve)

    def forward_curve(self, freq_linear, damping_curve, listener_gain=None):
        """As ``early`` with the output peak-normalised per clip (reference oscillator.py:143-176).  It has no listener
        form: a ``listener_gain`` is a ValueError."""
        if listener_gain is not None:
            raise ValueError("forward_curve has no listener form: render with forward(..., listener_gain=...)")
        sig = self._curve_render(freq_linear, damping_curve)
        return sig / torch.max(torch.abs(sig), dim=1, keepdim=True)[0]


def curve_on_device(curve, f):
    """damping_curve(f_i) for every mode WITHOUT the reference's per-mode host callback (oscillator.py:152-154,
    one ``interp1d`` call and two host-to-device copies per mode): a piecewise-linear table - an object with knot
    arrays ``x`` / ``y`` such as the ``scipy.interpolate.interp1d(x, y, fill_value="extrapolate")`` of
    experiments/material_real_train.py:151, or an ``(x, y)`` pair - is uploaded once and interpolated (linearly
    extrapolated beyond the end knots) on the device; any other callable is evaluated ONCE on the whole frequency
    vector (element by element only if it rejects arrays).  f: (m,) fp64 device tensor -> (m,) fp64 on f.device."""
    table = None
    if isinstance(curve, (tuple, list)) and len(curve) == 2:
        table = curve
    elif hasattr(curve, "x") and hasattr(curve, "y") and getattr(curve, "_kind", "linear") in ("linear", 1):
        table = (curve.x, curve.y)
    if table is not None:
        x = torch.as_tensor(np.asarray(table[0], dtype=np.float64), device=f.device)
        y = torch.as_tensor(np.asarray(table[1], dtype=np.float64), device=f.device)
        if x.numel() == 1:
            return y.expand_as(f).clone()
        o = torch.argsort(x)
        x, y = x[o], y[o]
        i = torch.searchsorted(x, f.contiguous()).clamp_(1, x.numel() - 1)
        x0, x1, y0, y1 = x[i - 1], x[i], y[i - 1], y[i]
        return y0 + (y1 - y0) * (f - x0) / (x1 - x0)
    fr = f.detach().cpu().numpy()
    try:
        vals = np.asarray(curve(fr), dtype=np.float64).reshape(-1)
        if vals.shape != fr.shape:
            raise ValueError
    except Exception:
        vals = np.array([float(curve(fi)) for fi in fr], dtype=np.float64)
    return torch.from_numpy(vals).to(f.device)


def init_damps(osc):
    """Pre-fit alpha/beta bins to the material table values (reference oscillator.py:314-325)."""
    optimizer = torch.optim.Adam(list(osc.alpha.parameters()) + list(osc.beta.parameters()), lr=0.01)
    for _ in range(2000):
        optimizer.zero_grad()
        loss = (osc.alpha() - osc.mat.alpha) ** 2 / osc.mat.alpha ** 2 + (osc.beta() - osc.mat.beta) ** 2 / osc.mat.beta ** 2
        loss.mean().backward()
        optimizer.step()


class GTDampedOscillator(_BankBase):
    """Free-running bank with learnable frequencies (softplus-weighted over ``f_range``), dampings and
    amplitudes, used to pre-fit recorded audio (reference oscillator.py:178-243,
    experiments/material_real_train.py:113-134).  ``freq_nonlinear`` is the reference's per-sample frequency
    offset, an (A, m, S, len(f_range)) parameter (:186-187, kept so that checkpoints and optimisers see the same
    parameter set); with ``non_linear_rate = 0`` - what the reference's callers pass - it is not touched and the
    closed-form bank renders the clip, otherwise the time-varying kernel (ds_osc_tv_fwd / ds_osc_tv_bwd) does."""

    def __init__(self, forces, audio_num, mode_num, sample_num, sr, f_range: list, mat: Material, train_forces=False):
        super().__init__()
        self._setup(forces, audio_num, mode_num, sample_num, sr, mat, train_forces)
        self.freq_linear = WeightedSum([1, mode_num, 1], f_range)
        self.freq_nonlinear = WeightedSum([audio_num, mode_num, sample_num], f_range)
        bin_num = 64
        self.alpha_list = torch.exp(torch.linspace(np.log(mat.alpha / 10), np.log(mat.alpha * 100), bin_num))
        self.alpha = WeightedSum([1, mode_num, 1], list(self.alpha_list))
        self.beta_list = torch.exp(torch.linspace(np.log(mat.beta / 10), np.log(mat.beta * 100), bin_num))
        self.beta = WeightedSum([1, mode_num, 1], list(self.beta_list))
        self.amp = DirectValue([audio_num, mode_num, 1])
        self.noise = FilteredNoise(audio_num, sample_num)

    def damping(self):
        lbd = (self.freq_linear() * 2 * np.pi) ** 2
        return 0.5 * (self.alpha() + self.beta() * lbd)

    def forward(self, non_linear_rate=0.0, noise_rate=0.0, mode_gain=None, gain_hop=None, listener_gain=None,
                listener_hop=None, listener_delay=None):
        """``listener_gain`` / ``listener_hop``: as ``TraditionalDampedOscillator.forward`` - (audio_num, C, sample_num), the
        noise branch (one signal per clip) added to every channel; ``non_linear_rate`` must be 0 with it.
        ``listener_delay`` delays the modal channels only: the noise branch is added AFTER propagation and is not delayed."""
        slide = self._sliding(mode_gain, gain_hop, time_varying=non_linear_rate != 0.0)
        listen = self._listening(listener_gain, listener_hop, slide, time_varying=non_linear_rate != 0.0)
        delay = self._delaying(listener_delay, listen)
        if non_linear_rate != 0.0:
            sig = self._render_time_varying(non_linear_rate, mode_gain)
        else:
            amp = self.amp() if slide else self._with_gain(self.amp(), mode_gain)
            sig = self._render(self.freq_linear(), self.alpha(), self.beta(), amp, slide, listen)
            fd = self.damped_freq[0, :, 0].double()
            d = self.damping().reshape(-1).double().to(fd.device)
            self.undamped_freq = (torch.sqrt((2 * np.pi * fd) ** 2 + d ** 2) / (2 * np.pi)).float().reshape(1, -1, 1)
            sig = self._propagated(sig, delay, listen)
        if noise_rate != 0.0:
            noise = self.noise() * noise_rate
            sig = sig + (noise.unsqueeze(1) if listen else noise)
        return sig

    def _render_time_varying(self, rate, mode_gain=None):
        """reference :219-242 with the (A, m, S) cumsum / exp / sin / mode-sum / conv1d chain as one kernel pair."""
        if self.force_frame_num > FIR_MAX_FORCE:
            raise ValueError(f"time-varying render (non_linear_rate != 0): force of {self.force_frame_num} taps, the FIR "
                             f"kernels hold at most {FIR_MAX_FORCE}; the closed-form render (non_linear_rate = 0) takes a "
                             "force of any length")
        dev, force = self._force_on_device()
        undamped = (self.freq_linear() + rate * self.freq_nonlinear()).to(dev)  # (A, m, S)
        lbd = (undamped * 2 * np.pi) ** 2
        damp = 0.5 * (self.alpha().to(dev) + self.beta().to(dev) * lbd)
        freq = (lbd - damp ** 2) ** 0.5 / (2 * np.pi)
        self.undamped_freq = ((2 * np.pi * freq) ** 2 + damp ** 2) ** 0.5 / (2 * np.pi)
        amp = self._with_gain(self.amp(), mode_gain).reshape(self.audio_num, self.mode_num).to(dev)
        return oscillator_bank_tv(damp, freq, amp, force.detach(), self.sample_num, self.sr)
