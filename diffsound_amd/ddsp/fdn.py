"""Late reverberation: a differentiable feedback delay network (ds_fdn_fwd / ds_fdn_bwd, csrc/fdn.hip).

``reverb.RoomResponse`` spends one free parameter per tap and a cost that grows with the tail.  A feedback delay network
(FDN) makes the late field of a room from ``n`` delay lines that feed one another through a mixing matrix,

    q_j[t] = (1 - p_j) s_j[t - m_j] + p_j s_j[t - m_j - 1]      line j's output: its delay and a two-tap absorption low-pass
    s_i[t] = b_i x[t] + sum_j A_ij q_j[t]                       what enters line i
    y[t]   = d x[t]   + sum_j c_j q_j[t],

from rest, in fp64 on the device and in the time domain: the tail is not aliased, whatever its length, and the cost per
sample does not depend on it.  ``fdn_reverb`` is the recursion with exact gradients to the signal and to A, b, c, d and p;
``FeedbackDelayNetwork`` is the trainable room that goes between a render and ``MSSLoss``: a few dozen parameters, stable
for every value of them.
"""
import math

import torch
from torch import nn

from .. import _hip

MAX_LINES = 16    # DS_FDN_MAX_LINES
MIN_DELAY = 64    # DS_FDN_MIN_DELAY
MAX_ROWS = 65535  # DS_FDN_MAX_ROWS


class _Fdn(torch.autograd.Function):
    """y (B, N) fp32 from x (B, N) fp32, delays (H, n) int32 and A (H, n, n), b, c (H, n), d (H), p (H, n) or None, fp64;
    gradients for all but the delays, NULL for those nobody needs."""

    @staticmethod
    def forward(ctx, x, delays, A, b, c, d, p):
        x, A, b, c, d = (t.detach().contiguous() for t in (x, A, b, c, d))
        p = None if p is None else p.detach().contiguous()
        (B, N), (H, n) = x.shape, delays.shape
        y = torch.empty_like(x)
        state = torch.empty((B, n, N), dtype=torch.float64, device=x.device)
        q = _hip.ptr
        _hip.launch("ds_fdn_fwd", q(x), q(delays), q(A), q(b), q(c), q(d), q(p), B, H, N, n, q(state), q(y), device=x.device)
        ctx.save_for_backward(x, delays, A, b, c, d, p, state)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, delays, A, b, c, d, p, state = ctx.saved_tensors
        need = ctx.needs_input_grad
        if not any(need):
            return (None,) * 7
        (B, N), (H, n) = x.shape, delays.shape
        gy = gy.float().contiguous()
        work, nbytes = _hip.workspace("ds_fdn_workspace_bytes", B, H, N, n, device=x.device)
        grads = [torch.empty_like(t) if t is not None and wanted else None
                 for t, wanted in zip((x, None, A, b, c, d, p), need)]
        q = _hip.ptr
        _hip.launch("ds_fdn_bwd", q(gy), q(x), q(delays), q(A), q(b), q(c), q(d), q(p), B, H, N, n, q(state), q(work), nbytes,
                    q(grads[0]), *(q(g) for g in grads[2:]), device=x.device)
        return tuple(grads)


def _shapes(who, x, n_sets, n_lines):
    """(B, N) of ``x`` (N,) or (B, N) for H sets of n lines; ValueError for what the entry points would refuse."""
    if not isinstance(x, torch.Tensor) or not x.is_floating_point() or x.dim() not in (1, 2):
        raise ValueError(f"{who}: x must be a floating-point tensor (N,) or (B, N)")
    if x.numel() < 1:
        raise ValueError(f"{who}: empty signal {tuple(x.shape)}")
    B = x.shape[0] if x.dim() == 2 else 1
    if n_lines > MAX_LINES:
        raise ValueError(f"{who}: {n_lines} delay lines, at most {MAX_LINES}")
    if n_sets > B or B % n_sets:
        raise ValueError(f"{who}: {B} row{'s' if B != 1 else ''} is not a multiple of the {n_sets} parameter sets")
    if B > MAX_ROWS:
        raise ValueError(f"{who}: {B} rows, at most {MAX_ROWS} per call")
    return B, x.shape[-1]


def _host_delays(who, delays):
    """``delays`` as a host int64 tensor (H, n), every one at least MIN_DELAY (the entry points never read them on the host)."""
    t = torch.as_tensor(delays)
    if t.is_floating_point() or t.is_complex() or t.dtype == torch.bool or t.dim() not in (1, 2) or t.numel() < 1:
        raise ValueError(f"{who}: delays must be integers (n,) or (H, n)")
    t = t.detach().to("cpu", torch.int64).reshape(-1, t.shape[-1])
    if int(t.min()) < MIN_DELAY:
        raise ValueError(f"{who}: a delay of {int(t.min())} samples, at least {MIN_DELAY}")
    if int(t.max()) > 2 ** 31 - 2:
        raise ValueError(f"{who}: a delay of {int(t.max())} samples does not fit an int32")
    return t


def fdn_reverb(x, delays, A, b, c, d, damp=None):
    """``x`` (N,) or (B, N) through feedback delay networks of n lines: ``delays`` integers (n,) or (H, n), ``A`` (n, n) or
    (H, n, n) (row i: what enters line i), ``b``, ``c`` (n,) or (H, n), ``d`` a number or (H,), ``damp`` None (no absorption
    filter) or the p of the two-tap low-pass, (n,) or (H, n).  B is a multiple of H and row b uses set b mod H.  From rest,
    fp64 arithmetic on the device, fp32 signal in and out; returns the shape and dtype of ``x``.  Autograd reaches ``x``, ``A``,
    ``b``, ``c``, ``d`` and ``damp``; the delays are fixed.  ValueError before any native call: wrong ranks, shapes that do
    not agree, a B that is no multiple of H, more than 16 lines, a delay below 64 samples, more than 65535 rows.  HIP
    tensors only: there is no CPU path (RuntimeError)."""
    who = "fdn_reverb"
    host = _host_delays(who, delays)
    H, n = host.shape
    if not isinstance(x, torch.Tensor):
        raise ValueError(f"{who}: x must be a floating-point tensor (N,) or (B, N)")
    as64 = lambda t: torch.as_tensor(t, dtype=torch.float64, device=x.device)
    A, b, c, d = as64(A), as64(b), as64(c), as64(d)
    p = None if damp is None else as64(damp)
    for name, t, lead, tail in (("A", A, (2, 3), (n, n)), ("b", b, (1, 2), (n,)), ("c", c, (1, 2), (n,)), ("d", d, (0, 1), ()),
                                ("damp", p, (1, 2), (n,))):
        if t is None:
            continue
        if t.dim() not in lead or tuple(t.shape[t.dim() - len(tail):]) != tail or (t.dim() == lead[1] and t.shape[0] != H):
            raise ValueError(f"{who}: {name} has shape {tuple(t.shape)}; {H} set{'s' if H != 1 else ''} of {n} lines need "
                             f"{tail} or {(H,) + tail}")
    B, N = _shapes(who, x, H, n)
    _hip.require_gpu(x)
    full = lambda t, tail: None if t is None else t.expand((H,) + tail) if t.dim() == len(tail) else t
    y = _Fdn.apply(x.reshape(B, N).float(), host.to(x.device, torch.int32).contiguous(), full(A, (n, n)), full(b, (n,)),
                   full(c, (n,)), full(d, ()), full(p, (n,)))
    return y.to(x.dtype).reshape(x.shape)


def _is_prime(k):
    return k >= 2 and all(k % f for f in range(2, math.isqrt(k) + 1))


def default_delays(n_lines, sample_rate):
    """The module's delays [samples]: for j = 0 .. n - 1 the prime nearest to sample_rate 0.02 5^(j / (n - 1)) - a geometric
    progression from 20 ms to 100 ms (20 ms alone for one line) - that no earlier line has taken; of two equally near, the
    smaller.  Primes share no factor, so the lines' echoes do not pile up on common multiples."""
    taken = []
    for j in range(int(n_lines)):
        target = float(sample_rate) * 0.02 * 5.0 ** (j / max(int(n_lines) - 1, 1))
        k0, step = int(round(target)), 0
        while True:
            near = sorted({k0 - step, k0 + step}, key=lambda k: (abs(k - target), k))
            hit = [k for k in near if _is_prime(k) and k not in taken]
            if hit:
                taken.append(hit[0])
                break
            step += 1
    return taken


class FeedbackDelayNetwork(nn.Module):
    """``n_responses`` rooms of ``n_lines`` delay lines each; ``forward`` flattens the leading dimensions of ``audio`` to rows
    and row b goes through room b mod n_responses.

    The dry path is fixed, d = 1.  A = U diag(g) with g_j = 10^(-3 m_j / (sample_rate rt60)): every line loses 60 dB in ``rt60``
    seconds; ``rt60`` (a number or one per room) is trainable through ``log_rt60``.  U = U0 matrix_exp(S - S^T) in fp64, U0 the
    Householder matrix I - (2 / n) 1 1^T and ``S`` (n x n, zero at the start) trainable: U is orthogonal for EVERY S, so with
    0 < g_j < 1 the loop is stable for every parameter value.  The absorption p_j = 0.5 sigmoid(``damp_logit``_j) stays in (0, 0.5):
    a low-pass; ``damp`` is its start value in [0, 0.5), a start of 0 is taken as 1e-4 (a sigmoid does not reach 0).  ``b``
    (ones at the start) and ``c`` are trainable.  ``init="zero"``: c = 0 and the module is the identity bit for bit (a negative
    zero is the number zero and comes out as +0); training can only add a room.  ``init="wet"``: c_j = (-1)^j 10^(wet_db / 20) /
    sqrt(n).  ``delays``: integers (n,) or (n_responses, n), each at least 64, fixed; None: ``default_delays`` - distinct primes
    nearest to a geometric progression from 20 ms to 100 ms."""

    def __init__(self, n_responses, n_lines, sample_rate, rt60, delays=None, damp=0.0, wet_db=None, init="zero"):
        super().__init__()
        H, n = int(n_responses), int(n_lines)
        who = "FeedbackDelayNetwork"
        if H < 1 or n < 1 or n > MAX_LINES:
            raise ValueError(f"{who}: {H} responses of {n} lines; at least 1 of each, at most {MAX_LINES} lines")
        if init not in ("zero", "wet"):
            raise ValueError(f"{who}: init = {init!r} is neither 'zero' nor 'wet'")
        if init == "wet" and wet_db is None:
            raise ValueError(f"{who}: init='wet' needs wet_db")
        self.sample_rate = float(sample_rate)
        rt = torch.as_tensor(rt60, dtype=torch.float64).reshape(-1)
        if not self.sample_rate > 0 or rt.numel() not in (1, H) or not bool((rt > 0).all()):
            raise ValueError(f"{who}: sample_rate and rt60 [s] must be positive, rt60 a number or one per response")
        if not 0.0 <= float(damp) < 0.5:
            raise ValueError(f"{who}: damp = {damp} outside [0, 0.5)")
        host = _host_delays(who, default_delays(n, self.sample_rate) if delays is None else delays)
        if host.shape[1] != n or host.shape[0] not in (1, H):
            raise ValueError(f"{who}: delays of shape {tuple(host.shape)} for {H} responses of {n} lines")
        self.register_buffer("delays", host.expand(H, n).to(torch.int32).contiguous())
        self.register_buffer("U0", torch.eye(n, dtype=torch.float64) - (2.0 / n) * torch.ones((n, n), dtype=torch.float64))
        self.log_rt60 = nn.Parameter(rt.expand(H).log().clone())
        self.S = nn.Parameter(torch.zeros((H, n, n), dtype=torch.float64))
        p0 = max(float(damp), 1e-4)
        self.damp_logit = nn.Parameter(torch.full((H, n), math.log(2.0 * p0 / (1.0 - 2.0 * p0)), dtype=torch.float64))
        self.b = nn.Parameter(torch.ones((H, n), dtype=torch.float64))
        c = torch.zeros((H, n), dtype=torch.float64)
        if init == "wet":
            c = c + (10.0 ** (float(wet_db) / 20.0) / math.sqrt(n)) * (-1.0) ** torch.arange(n, dtype=torch.float64)
        self.c = nn.Parameter(c)

    def mixing(self):
        """U (H, n, n) fp64: orthogonal for every ``S``."""
        return self.U0 @ torch.matrix_exp(self.S - self.S.transpose(1, 2))

    def coefficients(self):
        """(A (H, n, n), b, c (H, n), d (H), p (H, n)) of the recursion, fp64, differentiable."""
        g = 10.0 ** (-3.0 * self.delays.double() / (self.sample_rate * self.log_rt60.exp()[:, None]))
        return self.mixing() * g[:, None, :], self.b, self.c, torch.ones_like(self.log_rt60), 0.5 * torch.sigmoid(self.damp_logit)

    def _rows(self, x):
        H, n = self.delays.shape
        B, N = _shapes("FeedbackDelayNetwork", x, H, n)
        _hip.require_gpu(x, self.delays)
        return _Fdn.apply(x.reshape(B, N).float(), self.delays, *self.coefficients())

    def forward(self, audio):
        """``audio`` (..., time) through the rooms; the leading dimensions are flattened to rows."""
        return self._rows(audio.reshape(-1, audio.shape[-1])).to(audio.dtype).reshape(audio.shape)

    def impulse_response(self, n_taps):
        """(H, n_taps) fp64: the kernel's answer to a unit impulse, differentiable.  ``ir[:, 1:]`` can initialise the ``ir``
        of a ``RoomResponse`` of n_taps taps (its dry tap is this one's ``ir[:, 0] = d = 1``)."""
        x = torch.zeros((self.delays.shape[0], int(n_taps)), dtype=torch.float32, device=self.delays.device)
        x[:, 0] = 1.0
        return self._rows(x).double()

    def response(self, freqs):
        """The complex frequency response d + c^T Q (I - A Q)^-1 b at ``freqs`` [Hz], Q = diag(e^{-i w m_j} ((1 - p_j) + p_j e^{-i w})),
        (H, ...) in torch (complex128, differentiable): the transfer function of the infinite tail, closed form."""
        A, b, c, d, p = self.coefficients()
        w = 2.0 * math.pi * torch.as_tensor(freqs, dtype=torch.float64, device=A.device) / self.sample_rate
        shape, w = w.shape, w.reshape(-1)
        unit = lambda ph: torch.polar(torch.ones_like(ph), -ph)
        Q = unit(w[None, :, None] * self.delays.double()[:, None, :]) * ((1.0 - p)[:, None, :] + p[:, None, :] * unit(w)[None, :, None])
        cplx = lambda t: t.to(torch.complex128)
        eye = torch.eye(A.shape[1], dtype=torch.complex128, device=A.device)
        s = torch.linalg.solve(eye - cplx(A)[:, None] * Q[:, :, None, :], cplx(b)[:, None, :, None].expand(-1, w.numel(), -1, -1))
        out = cplx(d)[:, None] + (cplx(c)[:, None, :] * Q * s[..., 0]).sum(-1)
        return out.reshape((A.shape[0],) + tuple(shape))
