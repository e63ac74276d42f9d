"""A modal bank whose pitch depends on how hard it is struck: the tension-modulated bank (ds_nlbank_fwd / ds_nlbank_bwd,
csrc/nlbank.hip).  ``nonlinear_bank`` is the function of tensors, ``TensionModulatedBank`` the module that keeps the coupling
strengths as parameters, ``modal_stretch`` the stretch coefficients of an object's modes from its mesh.  A force goes in - a
recording, a ``HertzHammer``'s, a ``Bow``'s - and the sound comes out, (A, S) fp32 as the banks give it, for ``propagate``,
``biquad_cascade``, ``RoomResponse``, ``FeedbackDelayNetwork`` and the losses."""
import math

import torch
from torch import nn

from .. import _hip

MAX_MODES = 512         # DS_NLBANK_MAX_MODES
MAX_TERMS = 4           # DS_NLBANK_MAX_TERMS
MAX_OVERSAMPLE = 64     # DS_NLBANK_MAX_OVERSAMPLE
MAX_CLIPS = 65535       # DS_NLBANK_MAX_CLIPS
MAX_SUBSTEPS = 1 << 24  # DS_NLBANK_MAX_SUBSTEPS


def _check(d, w, gain, amp, force, stretch, coupling, sample_num, sr, oversample):
    """Every refusal that needs no device, shapes first: ValueError."""
    named = (("d", d), ("w", w), ("gain", gain), ("amp", amp), ("force", force), ("stretch", stretch), ("coupling", coupling))
    for name, t in named:
        if not isinstance(t, torch.Tensor) or not t.is_floating_point():
            raise ValueError(f"nonlinear_bank: {name} must be a floating-point tensor")
    if d.dim() != 1 or d.numel() < 1 or w.shape != d.shape:
        raise ValueError(f"nonlinear_bank: d and w must be (m,), got {tuple(d.shape)} and {tuple(w.shape)}")
    m = d.shape[0]
    if gain.dim() != 2 or gain.shape[1] != m or gain.shape[0] < 1:
        raise ValueError(f"nonlinear_bank: gain must be (A, {m}), got {tuple(gain.shape)}")
    A = gain.shape[0]
    if amp.shape != (A, m):
        raise ValueError(f"nonlinear_bank: amp must be ({A}, {m}), got {tuple(amp.shape)}")
    if force.dim() != 2 or force.shape[0] != A or force.shape[1] < 1:
        raise ValueError(f"nonlinear_bank: force must be ({A}, F), got {tuple(force.shape)}")
    if stretch.dim() != 2 or stretch.shape[1] != m or stretch.shape[0] < 1:
        raise ValueError(f"nonlinear_bank: stretch must be (K, {m}), got {tuple(stretch.shape)}")
    K = stretch.shape[0]
    if coupling.shape != (A, K):
        raise ValueError(f"nonlinear_bank: coupling must be ({A}, {K}), got {tuple(coupling.shape)}")
    if not 1 <= A <= MAX_CLIPS or not 1 <= m <= MAX_MODES or not 1 <= K <= MAX_TERMS:
        raise ValueError(f"nonlinear_bank: A = {A} outside 1..{MAX_CLIPS}, m = {m} outside 1..{MAX_MODES} or K = {K} outside "
                         f"1..{MAX_TERMS}")
    if sample_num < 1:
        raise ValueError(f"nonlinear_bank: sample_num = {sample_num} below 1")
    if not 1 <= oversample <= MAX_OVERSAMPLE or sample_num * oversample > MAX_SUBSTEPS:
        raise ValueError(f"nonlinear_bank: oversample = {oversample} outside 1..{MAX_OVERSAMPLE} or more than {MAX_SUBSTEPS} "
                         f"substeps")
    if not (math.isfinite(sr) and sr > 0):
        raise ValueError(f"nonlinear_bank: sr = {sr} is not positive")
    # the checks of values: one flag each, read in one transfer (tensors on different devices are refused after this)
    flags = [torch.isfinite(t).all() for _, t in named] + [(w > 0).all(), (stretch >= 0).all(), (coupling >= 0).all()]
    flags = torch.stack([f.to(d.device) for f in flags]).tolist()
    for (name, _), ok in zip(named, flags):
        if not ok:
            raise ValueError(f"nonlinear_bank: {name} is not finite")
    for ok, text in zip(flags[7:], ("w must be positive (damped angular frequencies)", "stretch must not be negative",
                                    "coupling must not be negative")):
        if not ok:
            raise ValueError("nonlinear_bank: " + text)


class _NonlinearBank(torch.autograd.Function):
    """y (A, S) fp32 of the recursion in csrc/nlbank.hip; gradients for d, w, gain, amp, force, stretch and coupling, each
    group computed only where it is needed."""

    @staticmethod
    def forward(ctx, d, w, gain, amp, force, stretch, coupling, sample_num, sr, oversample):
        inputs = (d, w, gain, amp, force, stretch, coupling)
        _check(*inputs, sample_num, sr, oversample)
        _hip.require_gpu(*inputs)
        ops = tuple(t.detach().to(torch.float64).contiguous() for t in inputs)
        (A, m), F, K = ops[2].shape, ops[4].shape[1], ops[5].shape[0]
        y = torch.empty((A, sample_num), dtype=torch.float32, device=d.device)
        p = _hip.ptr
        _hip.launch("ds_nlbank_fwd", *map(p, ops), A, m, K, F, sample_num, oversample, sr, p(y), device=d.device)
        ctx.save_for_backward(*ops)
        ctx.args = (sample_num, sr, oversample)
        ctx.dtypes = tuple(t.dtype for t in inputs)
        return y

    @staticmethod
    def backward(ctx, gy):
        ops = ctx.saved_tensors
        S, sr, R = ctx.args
        (A, m), F, K = ops[2].shape, ops[4].shape[1], ops[5].shape[0]
        need = ctx.needs_input_grad
        new = lambda like, on: torch.empty_like(like) if on else None  # noqa: E731
        gd, gw = new(ops[0], need[0] or need[1]), new(ops[1], need[0] or need[1])
        rest = [new(ops[i], need[i]) for i in range(2, 7)]
        work, nbytes = _hip.workspace("ds_nlbank_workspace_bytes", A, m, K, S, R, device=gy.device)
        gy = gy.float().contiguous()
        p = _hip.ptr
        _hip.launch("ds_nlbank_bwd", p(gy), *map(p, ops), A, m, K, F, S, R, sr, p(work), nbytes, p(gd), p(gw), *map(p, rest),
                    device=gy.device)
        grads = (gd, gw, *rest)
        return tuple(g.to(dt) if g is not None and on else None for g, dt, on in zip(grads, ctx.dtypes, need)) + (None,) * 3


def nonlinear_bank(d, w, gain, amp, force, stretch, coupling, sample_num, sr, oversample=8):
    """The sound (A, sample_num) fp32 of m modes whose stiffness rises with their own amplitude: a plate, a gong, a bowl's wall
    or a bar struck hard starts sharp and glides down to its small-amplitude pitch, because bending stretches the mid-surface
    and the stretch stiffens every mode.  The model is the tension-modulation form (Kirchhoff-Carrier for strings, Berger for
    plates): on top of the modal quadratic energy the quartic
        V(q) = 1/4 sum_r coupling_r (sum_i stretch[r,i] q_i^2)^2,
    K scalar tensions T_r = coupling_r sum_i stretch[r,i] q_i^2, each stiffening mode i by stretch[r,i] T_r.

    d [1/s], w [rad/s, damped] (m,): the pair the banks take, shared by the clips.  gain (A, m): the mass-orthonormal mode
    shapes at the contact, ``ContactSurface.amplitudes``; amp (A, m): the output gains.  force (A, F) [N]: zero from F on,
    samples at or behind ``sample_num`` are not read.  stretch (K, m) >= 0: ``modal_stretch`` gives one row; coupling (A, K)
    >= 0.  Autograd reaches all seven tensors; any floating dtype goes in and the gradients come back in the inputs' dtypes.
    HIP tensors only: there is no CPU path.

    With h = 1 / (sr oversample), z_i = exp((-d_i + i w_i) h) and s_i = 0 at the start, for n = 0 .. sample_num oversample - 1
    and k = n // oversample:
        q_i = Im s_i / w_i ;  E_r = sum_i stretch[r,i] q_i^2 ;  T_r = coupling_r E_r ;  kap_i = sum_r stretch[r,i] T_r ;
        p_i = gain_i force[k] - kap_i q_i ;  s_i = z_i (s_i + h p_i) ;
        y[k] = sr sum_i amp_i Im s_i after the sample's last substep,
    in fp64; the backward is the exact adjoint of this recursion, checkpointed at the output samples (its workspace does not
    grow with ``oversample`` beyond one segment a clip).  Linear limit: with coupling = 0 and oversample = 1 this is
    ``oscillator_bank_driven(d, w, amp * gain, force, sample_num, sr)``; a clip whose coupling is 0 takes the same path, and
    its nonlinear terms are exact zeros.  The scheme is explicit; it is stable while
        h sqrt(max_i kap_i) << 2
    at the largest amplitude reached, and a larger ``oversample`` is the remedy.  Left out: the off-diagonal part of the
    stretch form (only sums of squares q_i^2 make tension here, no products q_i q_j), the quadratic, asymmetric couplings of
    curved shells, and non-finite results, which are not detected on the device.

    ValueError before any device work: wrong shapes, w <= 0, stretch < 0, coupling < 0, a non-finite input, A above 65535, m
    above 512, K above 4, oversample outside 1..64, more than 2^24 substeps, sr <= 0, sample_num < 1."""
    return _NonlinearBank.apply(d, w, gain, amp, force, stretch, coupling, int(sample_num), float(sr), int(oversample))


class TensionModulatedBank(nn.Module):
    """The tension-modulated bank of an object: ``stretch`` (K, m) is a buffer, ``log_coupling`` (audio_num, K) an fp64
    parameter, trainable or not (``train_coupling``).  ``coupling``: a number, (K,) or (audio_num, K) values to start from,
    all positive.

        gain  = ContactSurface.amplitudes_at(...)
        force = hammer(d, w, gain, F, sr)
        bank  = TensionModulatedBank(A, modal_stretch(Deform(obj.tetmesh), obj.U_hat), coupling=1e9)
        y     = bank(d, w, gain, amp, force, S, sr)

    See ``nonlinear_bank`` for the model, its linear limit, its stability condition and what it leaves out."""

    def __init__(self, audio_num, stretch, coupling=1.0, oversample=8, train_coupling=True):
        super().__init__()
        stretch = torch.as_tensor(stretch).detach().to(torch.float64)
        if stretch.dim() == 1:
            stretch = stretch[None, :]
        if stretch.dim() != 2 or not 1 <= stretch.shape[0] <= MAX_TERMS or not 1 <= stretch.shape[1] <= MAX_MODES:
            raise ValueError(f"TensionModulatedBank: stretch must be (K, m) with K in 1..{MAX_TERMS} and m in 1..{MAX_MODES}, got "
                             f"{tuple(stretch.shape)}")
        if not bool((torch.isfinite(stretch) & (stretch >= 0)).all()):
            raise ValueError("TensionModulatedBank: stretch must be finite and not negative")
        if audio_num < 1 or not 1 <= int(oversample) <= MAX_OVERSAMPLE:
            raise ValueError(f"TensionModulatedBank: audio_num >= 1 and oversample in 1..{MAX_OVERSAMPLE} are required")
        K = stretch.shape[0]
        coupling = torch.as_tensor(coupling, dtype=torch.float64).detach()
        try:
            coupling = coupling.expand(audio_num, K).clone()
        except RuntimeError:
            raise ValueError(f"TensionModulatedBank: coupling must be a number, ({K},) or ({audio_num}, {K}), got "
                             f"{tuple(coupling.shape)}") from None
        if not bool((torch.isfinite(coupling) & (coupling > 0)).all()):
            raise ValueError("TensionModulatedBank: coupling must be positive")
        self.register_buffer("stretch", stretch.clone())
        self.log_coupling = nn.Parameter(coupling.log(), requires_grad=train_coupling)
        self.oversample = int(oversample)

    def forward(self, d, w, gain, amp, force, sample_num, sr):
        return nonlinear_bank(d, w, gain, amp, force, self.stretch, self.log_coupling.exp(), sample_num, sr, self.oversample)


def modal_stretch(deform, U, chunk_bytes=1 << 28):
    """(m,) fp64: C_i = sum over the Gauss points of weight |grad phi_i|_F^2, the integral of the squared displacement gradient
    of mode i - how much mode i stretches the material per unit of q_i^2.  ``deform``: the ``Deform`` of the mesh; ``U``
    (3 nodes, m): the mode shapes, ``DiffSoundObj.U_hat``.  This is the DIAGONAL of the stretch form
    int grad phi_i : grad phi_j: only the diagonal is kept, as ``nonlinear_bank`` couples the modes through sums of q_i^2
    alone.  Pure torch on the device over ``Deform.gradient_batch`` and ``Deform.integration_weights`` (both fp32, summed
    in fp64), in chunks of modes so that nothing of size m x Gauss points x 9 outlives a chunk (``chunk_bytes`` of fp32
    gradients at a time).  No autograd: the shapes are constants here."""
    nv = deform.tetmesh.vertices.shape[0]
    if not isinstance(U, torch.Tensor) or U.dim() != 2 or U.shape[0] != 3 * nv or U.shape[1] < 1:
        raise ValueError(f"modal_stretch: U must be ({3 * nv}, m), got {tuple(getattr(U, 'shape', ()))}")
    weights = deform.integration_weights.reshape(-1).to(torch.float64)
    step = max(1, int(chunk_bytes) // (36 * weights.numel()))
    out = []
    with torch.no_grad():
        for lo in range(0, U.shape[1], step):
            u = U[:, lo:lo + step].detach().t().reshape(-1, nv, 3)
            grad = deform.gradient_batch(u).to(torch.float64)
            out.append((grad.square().sum((-1, -2)) * weights[None, :]).sum(-1))
    return torch.cat(out)
