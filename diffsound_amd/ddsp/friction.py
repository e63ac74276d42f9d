"""The force of a sustained excitation - a bow, a rubbing finger, a wet rim - from the friction between the exciter and the
object's own motion at the contact point (ds_friction_fwd / ds_friction_bwd, csrc/friction.hip).  ``friction_force`` is the
function of tensors, ``Bow`` the module that keeps a stroke's three numbers as parameters.  The result is an ordinary (A, F)
force that requires grad; ``bank.oscillator_bank`` sends such a force through the driven bank, as with ``HertzHammer``."""
import math

import torch
from torch import nn

from .. import _hip

MAX_MODES = 512         # DS_FRICTION_MAX_MODES
MAX_OVERSAMPLE = 64     # DS_FRICTION_MAX_OVERSAMPLE
MAX_CLIPS = 65535       # DS_FRICTION_MAX_CLIPS
MAX_SUBSTEPS = 1 << 24  # DS_FRICTION_MAX_SUBSTEPS


def _check(d, w, gain, bow_velocity, normal_force, stribeck_velocity, sr, oversample):
    """Every refusal that needs no device, shapes first: ValueError."""
    named = (("d", d), ("w", w), ("gain", gain), ("bow_velocity", bow_velocity), ("normal_force", normal_force),
             ("stribeck_velocity", stribeck_velocity))
    for name, t in named:
        if not isinstance(t, torch.Tensor) or not t.is_floating_point():
            raise ValueError(f"friction_force: {name} must be a floating-point tensor")
    if d.dim() != 1 or d.numel() < 1 or w.shape != d.shape:
        raise ValueError(f"friction_force: d and w must be (m,), got {tuple(d.shape)} and {tuple(w.shape)}")
    m = d.shape[0]
    if gain.dim() != 2 or gain.shape[1] != m or gain.shape[0] < 1:
        raise ValueError(f"friction_force: gain must be (A, {m}), got {tuple(gain.shape)}")
    A = gain.shape[0]
    if bow_velocity.dim() != 2 or bow_velocity.shape[0] != A or bow_velocity.shape[1] < 1:
        raise ValueError(f"friction_force: bow_velocity must be ({A}, F), got {tuple(bow_velocity.shape)}")
    F = bow_velocity.shape[1]
    if normal_force.shape != (A, F):
        raise ValueError(f"friction_force: normal_force must be ({A}, {F}), got {tuple(normal_force.shape)}")
    if stribeck_velocity.shape != (A,):
        raise ValueError(f"friction_force: stribeck_velocity must be ({A},), got {tuple(stribeck_velocity.shape)}")
    if not 1 <= A <= MAX_CLIPS or not 1 <= m <= MAX_MODES:
        raise ValueError(f"friction_force: A = {A} outside 1..{MAX_CLIPS} or m = {m} outside 1..{MAX_MODES}")
    if not 1 <= oversample <= MAX_OVERSAMPLE or F * oversample > MAX_SUBSTEPS:
        raise ValueError(f"friction_force: oversample = {oversample} outside 1..{MAX_OVERSAMPLE} or more than {MAX_SUBSTEPS} "
                         f"substeps")
    if not (math.isfinite(sr) and sr > 0):
        raise ValueError(f"friction_force: sr = {sr} is not positive")
    # the checks of values: one flag each, read in one transfer (tensors on different devices are refused after this)
    flags = [torch.isfinite(t).all() for _, t in named] + [(w > 0).all(), (d > 0).all(), (normal_force >= 0).all(),
                                                          (stribeck_velocity > 0).all()]
    flags = torch.stack([f.to(d.device) for f in flags]).tolist()
    for (name, _), ok in zip(named, flags):
        if not ok:
            raise ValueError(f"friction_force: {name} is not finite")
    for ok, text in zip(flags[6:], ("w must be positive (damped angular frequencies)", "d must be positive (decay rates)",
                                    "normal_force must not be negative", "stribeck_velocity must be positive")):
        if not ok:
            raise ValueError("friction_force: " + text)


class _FrictionForce(torch.autograd.Function):
    """force (A, F) fp32 of the recursion in csrc/friction.hip; gradients for d, w, gain, bow_velocity, normal_force and
    stribeck_velocity, each group computed only where it is needed."""

    @staticmethod
    def forward(ctx, d, w, gain, bow_velocity, normal_force, stribeck_velocity, sr, oversample):
        inputs = (d, w, gain, bow_velocity, normal_force, stribeck_velocity)
        _check(*inputs, sr, oversample)
        _hip.require_gpu(*inputs)
        ops = tuple(t.detach().to(torch.float64).contiguous() for t in inputs)
        (A, m), F = ops[2].shape, ops[3].shape[1]
        force = torch.empty((A, F), dtype=torch.float32, device=d.device)
        p = _hip.ptr
        _hip.launch("ds_friction_fwd", *map(p, ops), A, m, F, oversample, sr, p(force), device=d.device)
        ctx.save_for_backward(*ops)
        ctx.args = (sr, oversample)
        ctx.dtypes = tuple(t.dtype for t in inputs)
        return force

    @staticmethod
    def backward(ctx, gforce):
        ops = ctx.saved_tensors
        sr, R = ctx.args
        (A, m), F = ops[2].shape, ops[3].shape[1]
        need = ctx.needs_input_grad
        new = lambda like, on: torch.empty_like(like) if on else None  # noqa: E731
        gd, gw = new(ops[0], need[0] or need[1]), new(ops[1], need[0] or need[1])
        ggain = new(ops[2], need[2])
        gvb, gN = new(ops[3], need[3] or need[4]), new(ops[4], need[3] or need[4])
        gvs = new(ops[5], need[5])
        work, nbytes = _hip.workspace("ds_friction_workspace_bytes", A, m, F, R, device=gforce.device)
        gforce = gforce.float().contiguous()
        p = _hip.ptr
        _hip.launch("ds_friction_bwd", p(gforce), *map(p, ops), A, m, F, R, sr, p(work), nbytes, p(gd), p(gw), p(ggain), p(gvb),
                    p(gN), p(gvs), device=gforce.device)
        grads = (gd, gw, ggain, gvb, gN, gvs)
        return tuple(g.to(dt) if g is not None and on else None for g, dt, on in zip(grads, ctx.dtypes, need)) + (None,) * 2


def friction_force(d, w, gain, bow_velocity, normal_force, stribeck_velocity, sr, oversample=8):
    """The friction force (A, F) fp32 between an exciter that moves with ``bow_velocity`` [m/s] under ``normal_force`` [N]
    (both (A, F): the gesture, per clip and output sample - attack, sustain, release, reversal) and the object's surface,
    whose velocity at the contact point comes from the object's own modes.  ``stribeck_velocity`` (A,) [m/s] is the relative
    velocity at which the friction characteristic peaks.

    d [1/s], w [rad/s, damped] (m,): the pair the banks take, shared by the clips.  gain (A, m): the mass-orthonormal mode
    shapes at the contact point along the stroke, ``ContactSurface.amplitudes``.  Autograd reaches all six tensors.  HIP
    tensors only: there is no CPU path.

    With h = 1 / (sr oversample), z_i = exp((-d_i + i w_i) h), g_i = gain_i^2, r_i = d_i / w_i and s_i = 0 at the start:
        v = sum_i g_i (Re s_i - r_i Im s_i) ;  vr = bow_velocity[n // oversample] - v ;  x = vr / stribeck_velocity ;
        f = normal_force[n // oversample] x exp((1 - x^2) / 2) ;  force[n // oversample] += f / oversample ;  s_i = z_i (s_i + h f),
    in fp64; the backward is the exact adjoint of this recursion, checkpointed at the output samples (its workspace does not
    grow with ``oversample``).  The characteristic is odd, peaks at 1 where vr = stribeck_velocity and falls beyond: the
    steep branch around 0 is sticking, the falling branch is what sustains a tone.  A clip whose normal force is 0 throughout
    gives a force of exact zeros and exact zero gradients but the normal force's.  The scheme is explicit; it is stable while
        h max(normal_force) (sqrt(e) / stribeck_velocity) sum_i g_i << 2,
    and a larger ``oversample`` is the remedy.  A non-finite result is not detected on the device.

    ValueError before any device work: wrong shapes, w <= 0, d <= 0, normal_force < 0, stribeck_velocity <= 0, a non-finite
    input, A above 65535, m above 512, oversample outside 1..64, more than 2^24 substeps, sr <= 0."""
    return _FrictionForce.apply(d, w, gain, bow_velocity, normal_force, stribeck_velocity, float(sr), int(oversample))


class Bow(nn.Module):
    """A stroke per clip: ``velocity``, ``log_pressure`` and ``log_stribeck`` (audio_num,) fp64 parameters, each trainable
    or not (``train_velocity``, ``train_pressure``, ``train_stribeck``).  ``velocity`` [m/s], ``pressure`` [N, the normal
    force] and ``stribeck_velocity`` [m/s]: numbers or (audio_num,) values to start from.  A fixed raised-cosine envelope -
    a rise over ``attack`` seconds from the first sample, a fall over ``release`` seconds to the last - multiplies both the
    velocity and the pressure, which gives the (audio_num, force_len) gesture of ``friction_force``.

        gain  = ContactSurface.amplitudes_at(...)
        force = bow(d, w, gain)
        y     = oscillator_bank(d, w, amp * gain, force, S, sr)

    A light, fast stroke slips and hisses, a heavy slow one sticks; between them the falling branch of the friction curve
    feeds the modes and the object sings.  See ``friction_force`` for the model, its stability condition and what it leaves
    out."""

    def __init__(self, audio_num, force_len, sample_rate, velocity, pressure, stribeck_velocity=0.1, attack=0.05, release=0.05,
                 oversample=8, train_velocity=True, train_pressure=True, train_stribeck=True):
        super().__init__()
        full = lambda v: torch.as_tensor(v, dtype=torch.float64).detach().reshape(-1).expand(audio_num).clone()  # noqa: E731
        pressure, stribeck = full(pressure), full(stribeck_velocity)
        if not bool((pressure > 0).all()) or not bool((stribeck > 0).all()):
            raise ValueError("Bow: pressure and stribeck_velocity must be positive")
        if force_len < 1 or not sample_rate > 0 or attack < 0 or release < 0:
            raise ValueError("Bow: force_len >= 1, sample_rate > 0, attack >= 0 and release >= 0 are required")
        self.velocity = nn.Parameter(full(velocity), requires_grad=train_velocity)
        self.log_pressure = nn.Parameter(pressure.log(), requires_grad=train_pressure)
        self.log_stribeck = nn.Parameter(stribeck.log(), requires_grad=train_stribeck)
        self.sample_rate, self.oversample = float(sample_rate), int(oversample)
        k = torch.arange(int(force_len), dtype=torch.float64)
        one = torch.ones_like(k)
        rise = 0.5 - 0.5 * torch.cos(math.pi * (k / (attack * self.sample_rate)).clamp(max=1.0)) if attack > 0 else one
        fall = 0.5 - 0.5 * torch.cos(math.pi * ((force_len - 1 - k) / (release * self.sample_rate)).clamp(max=1.0)) if release > 0 else one
        self.register_buffer("envelope", rise * fall)

    def gesture(self):
        """(bow_velocity, normal_force), both (audio_num, force_len) fp64."""
        return self.velocity[:, None] * self.envelope[None, :], self.log_pressure.exp()[:, None] * self.envelope[None, :]

    def forward(self, d, w, gain):
        bow_velocity, normal_force = self.gesture()
        return friction_force(d, w, gain, bow_velocity, normal_force, self.log_stribeck.exp(), self.sample_rate, self.oversample)
