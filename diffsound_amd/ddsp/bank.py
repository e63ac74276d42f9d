"""The oscillator banks as functions of tensors: five ``torch.autograd.Function`` wrappers, one per kernel family, and their
functional entries.  ``_OscBank`` is the closed-form bank with the force as a causal FIR out of LDS (ds_osc_bank_fwd / _bwd,
csrc/oscillator.hip), ``_OscBankTV`` the bank with per-sample rates (ds_osc_tv_fwd / _bwd, same file), ``_OscDriven`` the
recursive resonator under a force of any length, with a force gradient (ds_osc_driven_fwd / _bwd, csrc/osc_driven.hip),
``_OscSliding`` the same resonator with an input gain per mode and per sample, a contact that moves while the force acts
(ds_osc_slide_fwd / _bwd, csrc/osc_slide.hip), ``_OscListener`` the resonator read out through complex gains per channel, mode
and frame, a listener that may move (ds_osc_listen_fwd / _bwd, csrc/osc_listen.hip).
What they share - operand preparation, the optional ``amp`` across save_for_backward, the gradient buffers - is written
once below; a ``forward`` / ``backward`` holds its entry point, its workspace and its extra gradient."""
import torch

from .. import _hip

FIR_MAX_FORCE = 512  # taps the FIR kernels of csrc/oscillator.hip hold in LDS (MAXF)
SLIDE_HOP_UNIT = 16  # samples per lane of csrc/osc_slide.hip (DS_OSC_SCAN_RUN): the sliding bank's hop is a multiple of it
LISTEN_MAX_CHANNELS = 16  # DS_OSC_LISTEN_MAX_CHANNELS of csrc/osc_listen.hip


def _prepare(dtype, d, w, amp, force):
    """The kernels' operands: on the device, detached, contiguous; d and w (the per-mode pair) in ``dtype``, amp (or None)
    and force fp32."""
    _hip.require_gpu(d, w, force, amp)
    return (d.detach().to(dtype).contiguous(), w.detach().to(dtype).contiguous(),
            None if amp is None else amp.detach().float().contiguous(), force.detach().float().contiguous())


def _save(ctx, d, w, amp, force, S, sr):
    """save_for_backward takes tensors: an absent amp goes in as an empty sentinel and a flag."""
    ctx.save_for_backward(d, w, force, amp if amp is not None else torch.empty(0, device=force.device))
    ctx.has_amp = amp is not None
    ctx.S, ctx.sr = S, float(sr)


def _restore(ctx, gy):
    """(d, w, amp or None, force) as saved, and gy as the kernels take it."""
    d, w, force, amp = ctx.saved_tensors
    return d, w, (amp if ctx.has_amp else None), force, gy.float().contiguous()


def _grad_buffers(d, w, amp):
    """Uninitialised gradients of d, w and, where there is one, amp: the kernels write every element."""
    return torch.empty_like(d), torch.empty_like(w), (None if amp is None else torch.empty_like(amp))


class _OscBank(torch.autograd.Function):
    """y[a,t] = sum_j force[a,j] sum_m amp[a,m] exp(-d_m tau) sin(w_m tau) at tau = (t-j+1)/sr."""

    @staticmethod
    def forward(ctx, d, w, amp, force, S, sr):
        d, w, amp, force = _prepare(torch.float64, d, w, amp, force)
        A, nF = force.shape
        y = torch.empty((A, S), dtype=torch.float32, device=force.device)
        p = _hip.ptr
        _hip.launch("ds_osc_bank_fwd", p(d), p(w), p(amp), p(force), A, d.shape[0], nF, S, float(sr), p(y), device=d.device)
        _save(ctx, d, w, amp, force, S, sr)
        return y

    @staticmethod
    def backward(ctx, gy):
        d, w, amp, force, gy = _restore(ctx, gy)
        A, nF = force.shape
        gs = torch.empty_like(gy)
        gd, gw, gamp = _grad_buffers(d, w, amp)
        p = _hip.ptr
        _hip.launch("ds_osc_bank_bwd", p(gy), p(d), p(w), p(amp), p(force), A, d.shape[0], nF, ctx.S, ctx.sr, p(gs), p(gd), p(gw),
                    p(gamp), device=d.device)
        return gd, gw, gamp, None, None, None


class _OscBankTV(torch.autograd.Function):
    """Time-varying bank: y = FIR(sum_m amp exp(-cumsum(dmp / sr)) sin(2 pi cumsum(frq / sr))), dmp / frq (A, m, S)."""

    @staticmethod
    def forward(ctx, dmp, frq, amp, force, S, sr):
        dmp, frq, amp, force = _prepare(torch.float32, dmp, frq, amp, force)
        A, m, S_ = dmp.shape
        if S_ != S or frq.shape != dmp.shape or force.shape[0] != A:
            raise ValueError("time-varying bank: dmp and frq must be (audio_num, mode_num, sample_num)")
        work, _ = _hip.workspace("ds_osc_tv_workspace_floats", A, m, S, device=dmp.device, dtype=torch.float32)
        y = torch.empty((A, S), dtype=torch.float32, device=dmp.device)
        p = _hip.ptr
        _hip.launch("ds_osc_tv_fwd", p(dmp), p(frq), p(amp), p(force), A, m, force.shape[1], S, float(sr), p(work), p(y),
                    device=dmp.device)
        _save(ctx, dmp, frq, amp, force, S, sr)
        return y

    @staticmethod
    def backward(ctx, gy):
        dmp, frq, amp, force, gy = _restore(ctx, gy)
        A, m, S = dmp.shape
        gs = torch.empty_like(gy)
        gd, gf, gamp = _grad_buffers(dmp, frq, amp)
        p = _hip.ptr
        _hip.launch("ds_osc_tv_bwd", p(gy), p(dmp), p(frq), p(amp), p(force), A, m, force.shape[1], S, ctx.sr, p(gs), p(gd), p(gf),
                    p(gamp), device=dmp.device)
        return gd, gf, gamp, None, None, None


class _OscDriven(torch.autograd.Function):
    """The same y as ``_OscBank`` from the recursive resonator x[t] = z (x[t-1] + force[t]) per mode (ds_osc_driven_fwd /
    ds_osc_driven_bwd): any force length, gradients for d, w, amp and force."""

    @staticmethod
    def forward(ctx, d, w, amp, force, S, sr):
        d, w, amp, force = _prepare(torch.float64, d, w, amp, force)
        A, nF = force.shape
        m = d.shape[0]
        work, nbytes = _hip.workspace("ds_osc_driven_workspace_bytes", A, m, S, device=d.device)
        y = torch.empty((A, S), dtype=torch.float32, device=force.device)
        p = _hip.ptr
        _hip.launch("ds_osc_driven_fwd", p(d), p(w), p(amp), p(force), A, m, nF, S, float(sr), p(work), nbytes, p(y), device=d.device)
        _save(ctx, d, w, amp, force, S, sr)
        return y

    @staticmethod
    def backward(ctx, gy):
        d, w, amp, force, gy = _restore(ctx, gy)
        A, nF = force.shape
        m = d.shape[0]
        work, nbytes = _hip.workspace("ds_osc_driven_workspace_bytes", A, m, ctx.S, device=d.device)
        gd, gw, gamp = _grad_buffers(d, w, amp)
        gforce = torch.empty_like(force) if ctx.needs_input_grad[3] else None
        p = _hip.ptr
        _hip.launch("ds_osc_driven_bwd", p(gy), p(d), p(w), p(amp), p(force), A, m, nF, ctx.S, ctx.sr, p(work), nbytes, p(gd), p(gw),
                    p(gamp), p(gforce), device=d.device)
        return gd, gw, gamp, gforce, None, None


class _OscSliding(torch.autograd.Function):
    """The driven bank with an input gain per mode and per sample, x[t] = z (x[t-1] + g[t] force[t]), g piecewise linear
    between the K frames of ``gain`` (A, K, m), ``hop`` samples apart, the last one held (ds_osc_slide_fwd / ds_osc_slide_bwd,
    csrc/osc_slide.hip): a contact that moves while the force acts.  Gradients for d, w, amp, force and gain."""

    @staticmethod
    def forward(ctx, d, w, amp, force, gain, hop, S, sr):
        d, w, amp, force = _prepare(torch.float64, d, w, amp, force)
        _hip.require_gpu(gain)
        A, nF = force.shape
        m = d.shape[0]
        if gain.dim() != 3 or gain.shape[0] != A or gain.shape[2] != m or gain.shape[1] < 1:
            raise ValueError(f"sliding bank: gain must be ({A}, K, {m}), got {tuple(gain.shape)}")
        if hop <= 0 or hop % SLIDE_HOP_UNIT:
            raise ValueError(f"sliding bank: hop = {hop} is not a positive multiple of {SLIDE_HOP_UNIT}")
        K = gain.shape[1]
        gain_k = gain.detach().float().transpose(1, 2).contiguous()  # the kernels' layout: (A, m, K), frames contiguous
        work, nbytes = _hip.workspace("ds_osc_slide_workspace_bytes", A, m, S, K, hop, device=d.device)
        y = torch.empty((A, S), dtype=torch.float32, device=force.device)
        p = _hip.ptr
        _hip.launch("ds_osc_slide_fwd", p(d), p(w), p(amp), p(force), p(gain_k), A, m, nF, S, K, hop, float(sr), p(work), nbytes,
                    p(y), device=d.device)
        _save(ctx, d, w, amp, force, S, sr)
        ctx.gain_k, ctx.hop, ctx.gain_dtype = gain_k, hop, gain.dtype
        return y

    @staticmethod
    def backward(ctx, gy):
        d, w, amp, force, gy = _restore(ctx, gy)
        gain_k, hop = ctx.gain_k, ctx.hop
        A, nF = force.shape
        m, K = d.shape[0], gain_k.shape[2]
        work, nbytes = _hip.workspace("ds_osc_slide_workspace_bytes", A, m, ctx.S, K, hop, device=d.device)
        gd, gw, gamp = _grad_buffers(d, w, amp)
        gforce = torch.empty_like(force) if ctx.needs_input_grad[3] else None
        ggain = torch.empty_like(gain_k) if ctx.needs_input_grad[4] else None
        p = _hip.ptr
        _hip.launch("ds_osc_slide_bwd", p(gy), p(d), p(w), p(amp), p(force), p(gain_k), A, m, nF, ctx.S, K, hop, ctx.sr, p(work),
                    nbytes, p(gd), p(gw), p(gamp), p(gforce), p(ggain), device=d.device)
        if ggain is not None:
            ggain = ggain.transpose(1, 2).to(ctx.gain_dtype)
        return gd, gw, gamp, gforce, ggain, None, None, None


def _listener_gain_check(hgain, A, m, hop):
    """The refusals of ``oscillator_bank_listener`` that need no device; returns (hgain as (A, C, m, K), hop)."""
    if not torch.is_tensor(hgain) or not hgain.is_complex():
        raise ValueError("listener bank: hgain must be complex (a real gain g is g + 0i)")
    if hgain.dim() not in (3, 4) or hgain.shape[0] != A or hgain.shape[2] != m or min(hgain.shape) < 1:
        raise ValueError(f"listener bank: hgain must be ({A}, C, {m}) or ({A}, C, {m}, K), got {tuple(hgain.shape)}")
    if hgain.shape[1] > LISTEN_MAX_CHANNELS:
        raise ValueError(f"listener bank: {hgain.shape[1]} channels, at most {LISTEN_MAX_CHANNELS} channels per call")
    if hgain.dim() == 3:
        if hop is not None:
            raise ValueError("listener bank: hop goes with a 4-D hgain (A, C, m, K); a 3-D one is a listener at rest")
        return hgain.unsqueeze(-1), SLIDE_HOP_UNIT
    if hop is None or int(hop) != hop or hop <= 0 or int(hop) % SLIDE_HOP_UNIT:
        raise ValueError(f"listener bank: hop = {hop} is not a positive multiple of {SLIDE_HOP_UNIT}")
    return hgain, int(hop)


class _OscListener(torch.autograd.Function):
    """The driven bank read out through a complex gain per (channel, mode, frame), y[a,c,t] = sum_m amp Im(H[a,c,m](t) x_m[a,t]),
    H piecewise linear between the K frames of ``hgain`` (A, C, m, K), ``hop`` samples apart, the last one held
    (ds_osc_listen_fwd / ds_osc_listen_bwd, csrc/osc_listen.hip).  Gradients for d, w, amp, force and hgain (complex), each
    computed only where it is needed."""

    @staticmethod
    def forward(ctx, d, w, amp, force, hgain, hop, S, sr):
        d, w, amp, force = _prepare(torch.float64, d, w, amp, force)
        _hip.require_gpu(hgain)
        A, nF = force.shape
        m = d.shape[0]
        C, K = hgain.shape[1], hgain.shape[3]
        # the kernels' layout: (A, C, m, K, 2); a gain built as t.conj() carries torch's lazy conjugate bit, which view_as_real refuses
        h = torch.view_as_real(hgain.detach().to(torch.complex64).resolve_conj().contiguous())
        work, nbytes = _hip.workspace("ds_osc_listen_workspace_bytes", A, C, m, S, K, hop, device=d.device)
        y = torch.empty((A, C, S), dtype=torch.float32, device=force.device)
        p = _hip.ptr
        _hip.launch("ds_osc_listen_fwd", p(d), p(w), p(amp), p(force), p(h), A, C, m, nF, S, K, hop, float(sr), p(work), nbytes,
                    p(y), device=d.device)
        _save(ctx, d, w, amp, force, S, sr)
        ctx.h, ctx.hop, ctx.h_dtype = h, hop, hgain.dtype
        return y

    @staticmethod
    def backward(ctx, gy):
        d, w, amp, force, gy = _restore(ctx, gy)
        h, hop = ctx.h, ctx.hop
        A, nF = force.shape
        m, C, K = d.shape[0], h.shape[1], h.shape[3]
        work, nbytes = _hip.workspace("ds_osc_listen_workspace_bytes", A, C, m, ctx.S, K, hop, device=d.device)
        gd, gw, gamp = _grad_buffers(d, w, amp)
        gforce = torch.empty_like(force) if ctx.needs_input_grad[3] else None
        gh = torch.empty_like(h) if ctx.needs_input_grad[4] else None
        p = _hip.ptr
        _hip.launch("ds_osc_listen_bwd", p(gy), p(d), p(w), p(amp), p(force), p(h), A, C, m, nF, ctx.S, K, hop, ctx.sr, p(work),
                    nbytes, p(gd), p(gw), p(gamp), p(gforce), p(gh), device=d.device)
        if gh is not None:  # (d loss / d Re h, d loss / d Im h) is the gradient of a real loss as torch keeps it for a complex leaf
            gh = torch.view_as_complex(gh).to(ctx.h_dtype)
        return gd, gw, gamp, gforce, gh, None, None, None


def oscillator_bank_listener(d, w, amp, force, hgain, hop, sample_num, sr):
    """The bank heard through complex output gains: ``oscillator_bank``'s operands plus ``hgain``, complex, (A, C, m) - a
    listener at rest, ``hop`` None - or (A, C, m, K): the gain of every (channel, mode) at K control frames ``hop`` samples
    apart (``ModalRadiator.listener_path_gains``), linear in between, the last frame held; ``hop`` a positive multiple of 16.
    Returns (A, C, sample_num): y[a,c,t] = sum_m amp[a,m] Im(H[a,c,m](t) x_m[a,t]), one scan of the modes for all C <= 16
    channels.  Autograd reaches d, w, amp, force and hgain (a complex gradient).  ValueError before any launch: hgain not
    complex or of another shape, more than 16 channels, a bad or missing hop."""
    if force.dim() != 2:
        raise ValueError(f"listener bank: force must be (A, F), got {tuple(force.shape)}")
    hgain, hop = _listener_gain_check(hgain, force.shape[0], d.shape[0], hop)
    return _OscListener.apply(d, w, amp, force, hgain, hop, int(sample_num), float(sr))


def oscillator_bank_sliding(d, w, amp, force, gain, hop, sample_num, sr):
    """The bank under a contact that slides: ``oscillator_bank``'s operands plus ``gain`` (A, K, m), the input gain of every
    mode at K control frames ``hop`` samples apart (``ContactSurface.path_gains``), linear in between, the last frame held;
    ``hop`` a positive multiple of 16.  ``amp`` stays the output amplitude.  Autograd reaches d, w, amp, force and gain."""
    return _OscSliding.apply(d, w, amp, force, gain, int(hop), int(sample_num), float(sr))


def oscillator_bank_tv(dmp, frq, amp, force, sample_num, sr):
    """Functional entry of the time-varying bank: dmp [1/s], frq [Hz] (A, m, S) HIP tensors (autograd ok)."""
    return _OscBankTV.apply(dmp, frq, amp, force, int(sample_num), float(sr))


def oscillator_bank_driven(d, w, amp, force, sample_num, sr):
    """``oscillator_bank`` on the recursive-resonator kernels whatever the force length (tests, measurement)."""
    return _OscDriven.apply(d, w, amp, force, int(sample_num), float(sr))


def oscillator_bank(d, w, amp, force, sample_num, sr):
    """Functional entry: d, w (m,) fp64 HIP tensors (autograd ok), amp (A,m) or None, force (A,F), any F >= 1.
    Up to 512 taps without a force gradient this is the FIR bank (ds_osc_bank_fwd / _bwd); a longer force, or one that
    requires grad, goes through the driven bank (ds_osc_driven_fwd / _bwd), which also returns the force gradient."""
    if force.shape[-1] <= FIR_MAX_FORCE and not force.requires_grad:
        return _OscBank.apply(d, w, amp, force, int(sample_num), float(sr))
    return _OscDriven.apply(d, w, amp, force, int(sample_num), float(sr))
