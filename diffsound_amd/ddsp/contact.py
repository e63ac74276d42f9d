"""The force of a strike from the hammer that makes it: a nonlinear contact spring between a point mass and the object's
modes at the contact point (ds_contact_fwd / ds_contact_bwd, csrc/contact.hip).  ``contact_force`` is the function of
tensors, ``HertzHammer`` the module that keeps the hammer's three numbers as parameters.  The result is an ordinary
(A, F) force that requires grad; ``bank.oscillator_bank`` sends such a force through the driven bank."""
import math

import torch
from torch import nn

from .. import _hip

MAX_MODES = 512         # DS_CONTACT_MAX_MODES
MAX_OVERSAMPLE = 64     # DS_CONTACT_MAX_OVERSAMPLE
MAX_SUBSTEPS = 1 << 20  # DS_CONTACT_MAX_SUBSTEPS


def _check(d, w, gain, mass, velocity, stiffness, force_len, sr, exponent, oversample):
    """Every refusal that needs no device, shapes first: ValueError."""
    for name, t in (("d", d), ("w", w), ("gain", gain), ("mass", mass), ("velocity", velocity), ("stiffness", stiffness)):
        if not isinstance(t, torch.Tensor) or not t.is_floating_point():
            raise ValueError(f"contact_force: {name} must be a floating-point tensor")
    if d.dim() != 1 or d.numel() < 1 or w.shape != d.shape:
        raise ValueError(f"contact_force: d and w must be (m,), got {tuple(d.shape)} and {tuple(w.shape)}")
    m = d.shape[0]
    if gain.dim() != 2 or gain.shape[1] != m or gain.shape[0] < 1:
        raise ValueError(f"contact_force: gain must be (A, {m}), got {tuple(gain.shape)}")
    A = gain.shape[0]
    for name, t in (("mass", mass), ("velocity", velocity), ("stiffness", stiffness)):
        if t.shape != (A,):
            raise ValueError(f"contact_force: {name} must be ({A},), got {tuple(t.shape)}")
    if not 1 <= A <= 65535 or not 1 <= m <= MAX_MODES:
        raise ValueError(f"contact_force: A = {A} outside 1..65535 or m = {m} outside 1..{MAX_MODES}")
    if not 1 <= oversample <= MAX_OVERSAMPLE or force_len < 1 or force_len * oversample > MAX_SUBSTEPS:
        raise ValueError(f"contact_force: oversample = {oversample} outside 1..{MAX_OVERSAMPLE}, force_len = {force_len} below 1 "
                         f"or more than {MAX_SUBSTEPS} substeps")
    if not (math.isfinite(exponent) and exponent >= 1.0):
        raise ValueError(f"contact_force: exponent = {exponent} is not a finite number >= 1")
    if not (math.isfinite(sr) and sr > 0):
        raise ValueError(f"contact_force: sr = {sr} is not positive")
    # the checks of values: one flag each, read in one transfer (tensors on different devices are refused after this)
    named = (("d", d), ("w", w), ("gain", gain), ("mass", mass), ("velocity", velocity), ("stiffness", stiffness))
    flags = [torch.isfinite(t).all() for _, t in named] + [(w > 0).all(), (mass > 0).all() & (stiffness > 0).all()]
    flags = torch.stack([f.to(d.device) for f in flags]).tolist()
    for (name, _), ok in zip(named, flags):
        if not ok:
            raise ValueError(f"contact_force: {name} is not finite")
    if not flags[6]:
        raise ValueError("contact_force: w must be positive (damped angular frequencies)")
    if not flags[7]:
        raise ValueError("contact_force: mass and stiffness must be positive")


class _ContactForce(torch.autograd.Function):
    """force (A, F) fp32 of the recursion in csrc/contact.hip; gradients for d, w, gain, mass, velocity and stiffness, each
    group computed only where it is needed."""

    @staticmethod
    def forward(ctx, d, w, gain, mass, velocity, stiffness, force_len, sr, exponent, oversample):
        _check(d, w, gain, mass, velocity, stiffness, force_len, sr, exponent, oversample)
        _hip.require_gpu(d, w, gain, mass, velocity, stiffness)
        ops = tuple(t.detach().to(torch.float64).contiguous() for t in (d, w, gain, mass, velocity, stiffness))
        A, m = ops[2].shape
        force = torch.empty((A, force_len), dtype=torch.float32, device=d.device)
        p = _hip.ptr
        _hip.launch("ds_contact_fwd", *map(p, ops), A, m, force_len, oversample, exponent, sr, p(force), device=d.device)
        ctx.save_for_backward(*ops)
        ctx.args = (force_len, sr, exponent, oversample)
        ctx.dtypes = tuple(t.dtype for t in (d, w, gain, mass, velocity, stiffness))
        return force

    @staticmethod
    def backward(ctx, gforce):
        ops = ctx.saved_tensors
        F, sr, exponent, R = ctx.args
        A, m = ops[2].shape
        need = ctx.needs_input_grad
        new = lambda like, on: torch.empty_like(like) if on else None  # noqa: E731
        gd, gw = new(ops[0], need[0] or need[1]), new(ops[1], need[0] or need[1])
        ggain = new(ops[2], need[2])
        hammer = need[3] or need[4] or need[5]
        gmass, gvel, gstiff = new(ops[3], hammer), new(ops[4], hammer), new(ops[5], hammer)
        work, nbytes = _hip.workspace("ds_contact_workspace_bytes", A, m, F, R, device=gforce.device)
        gforce = gforce.float().contiguous()
        p = _hip.ptr
        _hip.launch("ds_contact_bwd", p(gforce), *map(p, ops), A, m, F, R, exponent, sr, p(work), nbytes, p(gd), p(gw), p(ggain),
                    p(gmass), p(gvel), p(gstiff), device=gforce.device)
        grads = (gd, gw, ggain, gmass, gvel, gstiff)
        return tuple(g.to(dt) if g is not None and on else None for g, dt, on in zip(grads, ctx.dtypes, need)) + (None,) * 4


def contact_force(d, w, gain, mass, velocity, stiffness, force_len, sr, exponent=1.5, oversample=8):
    """The contact force (A, force_len) fp32 of a hammer of ``mass`` [kg] that arrives with ``velocity`` [m/s] on a contact
    spring f = stiffness max(delta, 0)^exponent (1.5: Hertz; no gradient to the exponent), coupled to the object's modes.

    d [1/s], w [rad/s, damped] (m,): the pair the banks take, shared by the clips.  gain (A, m): the mass-orthonormal mode
    shapes at the contact point along the strike direction, ``ContactSurface.amplitudes``.  mass, velocity, stiffness (A,).
    Autograd reaches all six.  HIP tensors only: there is no CPU path.

    With h = 1 / (sr oversample), z_i = exp((-d_i + i w_i) h), kap_i = gain_i^2 / w_i, and xh = 0, vh = velocity, s_i = 0:
        delta = xh - sum_i kap_i Im s_i ;  f = stiffness max(delta, 0)^exponent ;  force[n // oversample] += f / oversample ;
        vh -= h f / mass ;  xh += h vh ;  s_i = z_i (s_i + h f),
    in fp64; the backward is the exact adjoint of this recursion.  velocity <= 0 gives a force of exact zeros and exact zero
    gradients.  The rigid-body modes of the object are not in the model (as everywhere in this package): it does not move
    away as a whole.  The scheme is explicit; it is stable while
        h sqrt(exponent stiffness delta_max^(exponent - 1) (1 / mass + sum_i kap_i w_i)) << 2,
    and a larger ``oversample`` is the remedy.  A non-finite result is not detected on the device.

    ValueError before any device work: wrong shapes, w <= 0, mass or stiffness <= 0, a non-finite input, m above 512, oversample
    outside 1..64, more than 2^20 substeps, exponent < 1."""
    return _ContactForce.apply(d, w, gain, mass, velocity, stiffness, int(force_len), float(sr), float(exponent),
                               int(oversample))


class HertzHammer(nn.Module):
    """A hammer per clip: ``log_mass``, ``log_stiffness`` and ``velocity`` (audio_num,) fp64 parameters, each trainable or
    not (``train_mass``, ``train_velocity``, ``train_stiffness``).  ``mass``, ``velocity``, ``stiffness``: numbers or
    (audio_num,) values to start from.

        gain  = ContactSurface.amplitudes_at(...)
        force = hammer(d, w, gain, F, sr)
        y     = oscillator_bank(d, w, amp * gain, force, S, sr)

    A hard, light hammer gives a short pulse and a bright sound, a soft one a long pulse and a dull sound; see
    ``contact_force`` for the model, its stability condition and what it leaves out."""

    def __init__(self, audio_num, mass, velocity, stiffness, exponent=1.5, oversample=8, train_mass=True, train_velocity=True,
                 train_stiffness=True):
        super().__init__()
        full = lambda v: torch.as_tensor(v, dtype=torch.float64).detach().reshape(-1).expand(audio_num).clone()  # noqa: E731
        mass, stiffness = full(mass), full(stiffness)
        if not bool((mass > 0).all()) or not bool((stiffness > 0).all()):
            raise ValueError("HertzHammer: mass and stiffness must be positive")
        self.log_mass = nn.Parameter(mass.log(), requires_grad=train_mass)
        self.log_stiffness = nn.Parameter(stiffness.log(), requires_grad=train_stiffness)
        self.velocity = nn.Parameter(full(velocity), requires_grad=train_velocity)
        self.exponent, self.oversample = float(exponent), int(oversample)

    def forward(self, d, w, gain, force_len, sr):
        return contact_force(d, w, gain, self.log_mass.exp(), self.velocity, self.log_stiffness.exp(), force_len, sr,
                             self.exponent, self.oversample)
