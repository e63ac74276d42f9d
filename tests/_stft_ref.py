"""References and per-element error bounds for the STFT and spectral-loss kernels of diffsound_amd/csrc/stft.hip (not a
test module).

The references are NumPy fp64 restatements of what the kernels compute, written from the kernels' header comment
(frame t covers padded samples [t hop, t hop + N), padded sample p = x[reflect(p - N / 2)], T = 1 + S // hop):

``frames`` / ``stft``       ds_stft_power: reflect-padded periodic-Hann frames, re, im = -sum x sin, P = re^2 + im^2,
``bwd_frames``              stft_bwd_frames_kernel: gframes = w[n] sum_k g_k (re_k cos - im_k sin), g = 2 gscale gP,
``fold``                    stft_bwd_fold_kernel: the adjoint of framing and reflect padding, as a SCATTER over padded
                            positions (the kernel gathers per sample: the two share no index arithmetic),
``spec_loss``               ds_spec_loss: per-row sums and d loss / d P_p of the weighted L1 (kind 0) and log RMSE (kind 1),
``bound_*``                 what the device result may differ from the reference by, derived from the code,
``round_like_kernel``       a CPU model of the kernels' fp32 roundings (forward and both backward kernels), optionally
                            with one of ``FAULTS`` planted, so that a bound that holds is shown to see a wrong kernel,
``torch_stft`` / ``torch_rmse_loss``  the same maps through torch.stft, for fp64 autograd.

Notation of the bounds: u = 2^-24 (unit roundoff of fp32), gamma_k = k u / (1 - k u) (k roundings compounded; k u to
first order).  The fp64 accumulations of the kernels and of the references contribute terms named ``fp64`` below:
(number of fp64 operations) 2^-52 times the sum of absolute terms, 2^-52 rather than 2^-53 so that both sides and the
fp64 twiddles / window (an ulp or two each) are inside.  They are 1e-5 of the fp32 terms at the largest n_fft."""
import functools

import numpy as np

U32 = 2.0 ** -24
U64 = 2.0 ** -52
LN2 = float(np.log(2.0))
LOG2F_ULPS = 2.0
"""Accuracy allowed to the device's log2f, in ulp of the result.  The ROCm documentation tree of the build image holds no
HIP math-function accuracy table (no document there mentions log2f), so this is the fallback: 2 ulp.  The library is built
without fast-math (csrc/Makefile: -O3 only), so log2f is the device library's full-accuracy routine."""


def gamma(k):
    return k * U32 / (1.0 - k * U32)


def _f64(x):
    return np.asarray(x, dtype=np.float64)


def _f32(x):
    return np.asarray(x, dtype=np.float32)


# ------------------------------------------------------------------------------------------------- references
def n_frames(S, hop):
    return 1 + S // hop


def window(N):
    """Periodic Hann, fp64."""
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N) / N)


def reflect(i, S):
    """Index of the sample that position i of the reflect-extended clip reads (-S < i < 2 S - 1)."""
    i = np.abs(i)
    return np.where(i >= S, 2 * (S - 1) - i, i)


@functools.lru_cache(maxsize=4)
def _twiddles(N):
    """cos, sin of 2 pi k n / N, (N / 2 + 1, N) each; the integer k n is reduced mod N first, so the argument is exact.
    (Cached: callers read the tables and leave them unchanged.)"""
    m = (np.arange(N // 2 + 1)[:, None] * np.arange(N)[None, :]) % N
    ang = 2.0 * np.pi * m / N
    return np.cos(ang), np.sin(ang)


def frames(x, N, hop):
    """x (B, S) -> windowed frames (B, T, N), fp64."""
    x = _f64(x)
    S = x.shape[1]
    pos = np.arange(n_frames(S, hop))[:, None] * hop + np.arange(N)[None, :] - N // 2
    return x[:, reflect(pos, S)] * window(N)


def stft(x, N, hop):
    """x (B, S) -> (re, im, P), (B, N / 2 + 1, T) each: re = sum_n f_n cos(2 pi k n / N), im = -sum_n f_n sin(...)."""
    f = frames(x, N, hop)
    C, Sn = _twiddles(N)
    re = np.transpose(f @ C.T, (0, 2, 1))
    im = -np.transpose(f @ Sn.T, (0, 2, 1))
    return re, im, re * re + im * im


def bwd_frames_sums(gP, re, im, N, gscale):
    """(a, A), (B, T, N) each: a_n = sum_k g_k (re_k cos(2 pi k n / N) - im_k sin(2 pi k n / N)) with g = 2 gscale gP, the
    sum the kernel forms before the window, and A_n = sum_k (|g re_k| + |g im_k|)."""
    g = 2.0 * float(gscale) * _f64(gP)
    gr, gi = np.transpose(g * _f64(re), (0, 2, 1)), np.transpose(g * _f64(im), (0, 2, 1))  # (B, T, F)
    C, Sn = _twiddles(N)
    a = gr @ C - gi @ Sn
    A = (np.abs(gr) + np.abs(gi)).sum(-1, keepdims=True) * np.ones(N)
    return a, A


def bwd_frames(gP, re, im, N, gscale):
    """d / d frame of sum gscale gP P: gframes (B, T, N) = w[n] a_n."""
    return window(N) * bwd_frames_sums(gP, re, im, N, gscale)[0]


def _scatter(gframes, S, N, hop):
    """Overlap-add onto the padded axis, then the padded axis onto the samples it was read from.  Two np.add.at."""
    gframes = _f64(gframes)
    B, T, _ = gframes.shape
    assert T == n_frames(S, hop)
    padded = np.zeros((B, S + N))
    pos = np.arange(T)[:, None] * hop + np.arange(N)[None, :]
    np.add.at(padded, (slice(None), pos.reshape(-1)), gframes.reshape(B, -1))
    gx = np.zeros((B, S))
    np.add.at(gx, (slice(None), reflect(np.arange(S + N) - N // 2, S)), padded)
    return gx


def fold(gframes, S, N, hop):
    """gx (B, S): the adjoint of ``frames`` without its window - every frame element is added to the sample it read."""
    return _scatter(gframes, S, N, hop)


def fold_terms(S, N, hop):
    """m (S,): how many frame elements ``fold`` adds into each sample (0 for samples under no frame)."""
    return np.rint(_scatter(np.ones((1, n_frames(S, hop), N)), S, N, hop)[0]).astype(np.int64)


def time_weights(T):
    """w_t = 2 t / (T - 1): (1 - linspace(1, 0.9, T)) normalised to mean 1.  T == 1 is 0 / 0 there; the kernel defines 0."""
    return 2.0 * np.arange(T) / (T - 1) if T > 1 else np.zeros(1)


def spec_loss(kind, Pp, Pt, alpha, eps, fclip):
    """ds_spec_loss.  Pp, Pt (B, F, T) fp32, ``eps`` the fp32 number the kernel is handed.  Returns (sums (B, F, 2),
    gP (B, F, T)):
      kind 0: sums[..., 0] = sum_t |w_t dlog|, sums[..., 1] = sum_t |w_t dlin| on rows f >= 1,
              gP = w_t (alpha sign(dlog) / ((Pp + eps) ln 2) + sign(dlin)) / (B (F - 1) T);
      kind 1: sums[..., 0] = sum_t dlog^2 on rows f < fclip, gP = dlog / ((Pp + eps) ln 2 B fclip T);
    dlog = log2(Pp + eps) - log2(Pt + eps), dlin = Pp - Pt; zeros on the other rows."""
    Pp, Pt = _f64(Pp), _f64(Pt)
    B, F, T = Pp.shape
    eps = float(np.float32(eps))
    a = Pp + eps
    dlog = np.log2(a) - np.log2(Pt + eps)
    sums, gP = np.zeros((B, F, 2)), np.zeros((B, F, T))
    if kind == 0:
        w, dlin = time_weights(T), Pp - Pt
        sums[:, 1:, 0] = np.abs(w * dlog)[:, 1:].sum(-1)
        sums[:, 1:, 1] = np.abs(w * dlin)[:, 1:].sum(-1)
        gP[:, 1:] = (w * (float(alpha) * np.sign(dlog) / (a * LN2) + np.sign(dlin)) / (B * (F - 1) * T))[:, 1:]
    else:
        sums[:, :fclip, 0] = (dlog * dlog)[:, :fclip].sum(-1)
        gP[:, :fclip] = (dlog / (a * LN2 * (B * fclip * T)))[:, :fclip]
    return sums, gP


# ----------------------------------------------------------------------------------------------------- bounds
def bound_stft(x, N, hop, re, im):
    """(bound_re, bound_im, bound_P), each (B, F, T), against ``stft``.

    stft_power_kernel rounds to fp32 three times on the way to a term of the DFT sum: the window (float)(0.5 - 0.5 cos)
    (formed in fp64: relative u, also where it is tiny), the product w x stored to LDS, and the twiddle (float)cos or
    (float)sin (|error| <= u |twiddle| <= u).  The sum itself is N fp64 fmas.  Before the store therefore
        |re^ - re|, |im^ - im| <= delta = gamma_3 sum_n |w_n x_n| + fp64,   fp64 = (N + 4) 2^-52 sum_n |w_n x_n|,
    the same for every bin of a frame.  The stores round once more:  delta (1 + u) + u |re|.
    P = re^2 + im^2 is formed in fp64 from the unrounded sums ((re + d)^2 - re^2 = 2 re d + d^2) and stored:
        |P^ - P| <= (2 (|re| + |im|) delta + 2 delta^2) (1 + u) + u P."""
    l1 = np.abs(frames(x, N, hop)).sum(-1)[:, None, :]  # (B, 1, T)
    delta = (gamma(3) + (N + 4) * U64) * l1
    re, im = np.abs(_f64(re)), np.abs(_f64(im))
    b_re, b_im = delta * (1 + U32) + U32 * re, delta * (1 + U32) + U32 * im
    b_P = (2.0 * (re + im) * delta + 2.0 * delta * delta) * (1 + U32) + U32 * (re * re + im * im)
    return b_re, b_im, b_P


def bound_gframes(gP, re, im, N, gscale):
    """(B, T, N) against ``bwd_frames`` fed the same fp32 gP, re, im.  With a_n, A_n of ``bwd_frames_sums``:
        3 u w_n A_n + (u / 2 + 3 u w_n) |a_n|   to first order.

    stft_bwd_frames_kernel: g = (2 gscale) gP rounds once (2 gscale is exact), g re and g im once more, the twiddle once:
    |a^ - a| <= E_a = gamma_3 A_n + fp64, fp64 = (2 F + 4) 2^-52 A_n for the 2 F fp64 fmas.  The window is the fp32
    expression 0.5f - 0.5f * (float)cos, which has NO relative accuracy near n = 0: 0.5f * c is exact, the subtraction
    rounds by at most u / 2 (results in [1/2, 1]; exact below 1/4 by Sterbenz), and the rounding of the cosine itself adds
    at most u / 4, and that much only where w >= 3/4:  |w^ - w| <= e_w = u / 2 + u w.  Then (float)a^ and the product
    w^ (float)a^ round once each.  Together
        (w + e_w) (1 + gamma_2) E_a + (e_w + gamma_2 (w + e_w)) |a|,
    whose first-order part is the line above: the three u w |a| are (float)a^, the product and the cosine's share of e_w."""
    a, A = bwd_frames_sums(gP, re, im, N, gscale)
    w = window(N)
    E_a = (gamma(3) + (N + 6) * U64) * A
    e_w = U32 / 2 + U32 * w
    return (w + e_w) * (1 + gamma(2)) * E_a + (e_w + gamma(2) * (w + e_w)) * np.abs(a)


def bound_fold(gframes, S, N, hop):
    """(B, S) against ``fold`` of the SAME fp32 gframes: gamma_{m-1} sum |terms| + fp64, m = ``fold_terms``.

    stft_bwd_fold_kernel adds the m elements of a sample one after the other in fp32, starting from 0 (the first addition
    is exact): m - 1 roundings of partial sums that never exceed sum |terms|.  fp64 = m 2^-52 sum |terms| is the
    reference's own summation; it is 0 for m <= 1, where the result must be exact (the one element, or 0.0)."""
    m = fold_terms(S, N, hop)[None, :]
    l1 = _scatter(np.abs(_f64(gframes)), S, N, hop)
    return np.where(m > 1, gamma(np.maximum(m - 1, 0)) + m * U64, 0.0) * l1


def bound_gx(gP, re, im, S, N, hop, gscale):
    """(B, S) against fold(bwd_frames(gP, re, im)): the element bounds of ``bound_gframes`` carried through the (linear,
    0 / 1-weighted) fold, plus the fold's own m - 1 roundings on elements that may be as large as |reference| + bound."""
    b = bound_gframes(gP, re, im, N, gscale)
    return _scatter(b, S, N, hop) + bound_fold(np.abs(bwd_frames(gP, re, im, N, gscale)) + b, S, N, hop)


def _ulp32(v):
    """Spacing of fp32 at |v| (fp64 in, fp64 out): 2^(e - 24) for |v| in [2^(e-1), 2^e), at least the subnormal spacing."""
    v = np.abs(_f64(v))
    _, e = np.frexp(v)
    return np.where(v == 0, 2.0 ** -149, np.maximum(np.ldexp(1.0, e - 24), 2.0 ** -149))


def _log_err(arg):
    """|log2f(fl(p + eps)) - log2(p + eps)| for arg = p + eps: the rounding of the sum moves the logarithm by at most
    u / ((1 - u) ln 2), and log2f is allowed LOG2F_ULPS ulp of a result that may be that much larger."""
    shift = U32 / ((1 - U32) * LN2)
    return shift + LOG2F_ULPS * _ulp32(np.abs(np.log2(arg)) + shift)


def bound_dlog(Pp, Pt, eps):
    """(B, F, T): |dlog^ - dlog| for dlog^ = fl(log2f(fl(Pp + eps)) - log2f(fl(Pt + eps))): ``_log_err`` of both and the
    rounding of the difference, u (|dlog| + the two).  Elements with Pp == Pt bitwise compute 0.0 exactly."""
    Pp, Pt = _f64(Pp), _f64(Pt)
    eps = float(np.float32(eps))
    a, b = Pp + eps, Pt + eps
    e = _log_err(a) + _log_err(b)
    return np.where(Pp == Pt, 0.0, e + U32 * (np.abs(np.log2(a) - np.log2(b)) + e))


def bound_spec_loss(kind, Pp, Pt, alpha, eps, fclip):
    """(bound_sums (B, F, 2), bound_gP (B, F, T)) against ``spec_loss``; zero on the excluded rows.  E = ``bound_dlog``.

    kind 0.  w = (float)(wnorm t) rounds once (the fp64 product adds 2^-52), w dlog and w dlin are fp32 products, dlin =
    fl(Pp - Pt) rounds once; the row sums are fp64:
        sums[0]: sum_t w_t (E_t + gamma_2 (|dlog_t| + E_t)) + fp64,   sums[1]: gamma_3 sum_t w_t |dlin_t| + fp64,
        fp64 = (T + 16) 2^-52 (sum of the absolute terms) for the lane sums, the shuffles and the four-wave tree.
      g = w (alpha sl il2 / fl(Pp + eps) + sn) (float)inv_count.  The signs sl, sn are those of the reference (the inputs keep
      |dlog| above E or tie exactly).  q = alpha sl / ((Pp + eps) ln 2) carries four roundings (the constant il2, alpha il2,
      the sum Pp + eps, the division); then the addition of sn, w, the product, (float)inv_count, the product: five more on
      everything:   |g^ - g| <= w inv_count (gamma_4 (1 + gamma_5) |q| + gamma_5 |q + sn|).
    kind 1.  a0 += (double)dlog^2 exactly:  sum_t (2 |dlog_t| E_t + E_t^2) + fp64.
      g = dlog il2 / fl(Pp + eps) (float)inv_count: six roundings (il2, two products, the sum, the division, inv_count)
      around dlog^:   |g^ - g| <= (gamma_6 |dlog| + (1 + gamma_6) E) inv_count / ((Pp + eps) ln 2)."""
    Pp64, Pt64 = _f64(Pp), _f64(Pt)
    B, F, T = Pp64.shape
    eps64 = float(np.float32(eps))
    a = Pp64 + eps64
    dlog = np.abs(np.log2(a) - np.log2(Pt64 + eps64))
    E = bound_dlog(Pp, Pt, eps)
    bs, bg = np.zeros((B, F, 2)), np.zeros((B, F, T))
    acc = (T + 16) * U64
    if kind == 0:
        w, dlin = time_weights(T), np.abs(Pp64 - Pt64)
        t0 = w * (E + gamma(2) * (dlog + E))
        bs[:, 1:, 0] = (t0 + acc * w * (dlog + E))[:, 1:].sum(-1)
        bs[:, 1:, 1] = ((gamma(3) + acc) * w * dlin)[:, 1:].sum(-1)
        q = float(alpha) * np.sign(dlog) / (a * LN2)  # |q| where dlog != 0
        qs = np.abs(float(alpha) * np.sign(np.log2(a) - np.log2(Pt64 + eps64)) / (a * LN2) + np.sign(Pp64 - Pt64))
        bg[:, 1:] = (w / (B * (F - 1) * T) * (gamma(4) * (1 + gamma(5)) * q + gamma(5) * qs))[:, 1:]
    else:
        bs[:, :fclip, 0] = ((2.0 * dlog * E + E * E) + acc * (dlog + E) ** 2)[:, :fclip].sum(-1)
        bg[:, :fclip] = ((gamma(6) * dlog + (1 + gamma(6)) * E) / (a * LN2 * (B * fclip * T)))[:, :fclip]
    return bs, bg


# ------------------------------------------------------------------------------- CPU model of the fp32 roundings
FAULTS = ("fold_left", "fold_right", "t1", "window", "im_sign", "offset")
"""Faults ``round_like_kernel`` can plant: the left / the right reflection term dropped in the fold; the fold's last frame
index t1 one too small; a symmetric instead of a periodic Hann window; the sign of im flipped in the backward; the
frame offset t hop replaced by t (N / 4)."""


def _rnd(x):
    """Round fp64 to fp32 and return it as fp64 (products and sums of two fp32 numbers are exact or correctly rounded in
    fp64 first; the double rounding can differ from a native fp32 operation by one ulp in rare ties)."""
    return _f64(x).astype(np.float32).astype(np.float64)


def round_like_kernel(x, N, hop, gP=None, gscale=1.0, fault=None):
    """The kernels' recipe on the CPU: the window, the windowed frame and the twiddles rounded to fp32, the DFT sums in
    fp64, fp32 where the kernels store; the backward reads the model's own fp32 re / im, and the fold gathers per sample
    in the kernel's order (direct position, left reflection, right reflection; frames ascending) with fp32 additions.
    Returns a dict of fp32 arrays: re, im, P and, with ``gP``, gframes and gx.  ``fault`` plants one of ``FAULTS``."""
    assert fault is None or fault in FAULTS
    x = _f32(x)
    B, S = x.shape
    T, F, pad = n_frames(S, hop), N // 2 + 1, N // 2
    n = np.arange(N)
    cosn = np.cos(2.0 * np.pi * n / (N - 1 if fault == "window" else N))
    C64, S64 = _twiddles(N)
    C32, S32 = _rnd(C64), _rnd(S64)
    step = N // 4 if fault == "offset" else hop
    pos = np.clip(reflect(np.arange(T)[:, None] * step + n[None, :] - pad, S), 0, S - 1)
    fx = _rnd(_rnd(0.5 - 0.5 * cosn) * x[:, pos].astype(np.float64))  # (B, T, N)
    re = np.transpose(fx @ C32.T, (0, 2, 1))
    im = -np.transpose(fx @ S32.T, (0, 2, 1))
    out = dict(re=_f32(re), im=_f32(im), P=_f32(re * re + im * im))
    if gP is None:
        return out
    g = _rnd(2.0 * float(np.float32(gscale)) * _f64(_f32(gP)))
    gr = np.transpose(_rnd(g * out["re"]), (0, 2, 1))
    gi = np.transpose(_rnd(g * out["im"]), (0, 2, 1))
    if fault == "im_sign":
        gi = -gi
    a = gr @ C32 - gi @ S32
    w32 = _rnd(0.5 - _rnd(0.5 * _rnd(cosn)))
    gf = _rnd(w32 * _rnd(a))
    out["gframes"] = _f32(gf)
    s = np.arange(S)
    cand = [(pad + s, np.ones(S, bool))]
    if fault != "fold_left":
        cand.append((pad - s, (s >= 1) & (s <= pad)))
    if fault != "fold_right":
        cand.append((pad + 2 * (S - 1) - s, (s <= S - 2) & (s >= S - 1 - pad)))
    acc = np.zeros((B, S))
    for p, ok in cand:
        t0 = np.where(p - N + 1 <= 0, 0, (p - N + 1 + hop - 1) // hop)
        t1 = np.minimum(T - 1, p // hop) - (1 if fault == "t1" else 0)
        for j in range(-(-N // hop)):
            t = t0 + j
            live = ok & (t <= t1)
            if not live.any():
                break
            acc[:, live] = _rnd(acc[:, live] + gf[:, t[live], (p - t * hop)[live]])
    out["gx"] = _f32(acc)
    return out


# ----------------------------------------------------------------------------------------------- torch references
def torch_stft(x, N, hop):
    """Complex STFT of x (B, S) as the reference's Spectrogram computes it (centred, reflect-padded, periodic Hann,
    one-sided), at x's dtype; autograd-capable."""
    import torch

    win = torch.hann_window(N, periodic=True, dtype=x.dtype, device=x.device)
    return torch.stft(x, N, hop_length=hop, window=win, center=True, pad_mode="reflect", return_complex=True)


def torch_rmse_loss(xp, xt, N, hop, eps=1e-7, scale=1.0):
    """The 'rmse_loss' expression of tests/test_mss_loss.py::_torch_loss for one scale, with the hop as an argument."""
    import torch

    lp, lt = torch_stft(xp, N, hop).abs() ** 2, torch_stft(xt, N, hop).abs() ** 2
    nb = int(lp.shape[-2] * scale)
    return torch.sqrt((((lp[:, :nb] + eps).log2() - (lt[:, :nb] + eps).log2()) ** 2).mean())


# ------------------------------------------------------------------------------------------- shapes and inputs
SR = 32000.0
# (B, S, n_fft, hop): smallest legal everything, S = n_fft / 2 + 1 (a sample read through both reflections); the same at
# the next size; a hop dividing neither S nor n_fft, three clips; hop == n_fft (no overlap, tail samples under no frame);
# hop > n_fft / 2 (samples under one frame only); hop 1 (the longest fold sums); n_fft == 256 (one pass of the
# 256-thread loops, F = 129); strided loops with bin 256 alone in a second pass; the largest n_fft at the shortest legal
# clip; T == 1; one scale of the workload
STFT_SHAPES = [(2, 5, 8, 2), (1, 9, 16, 4), (3, 131, 64, 5), (2, 100, 64, 64), (2, 101, 64, 48), (1, 40, 32, 1),
               (2, 1000, 256, 64), (2, 700, 512, 128), (1, 1025, 2048, 512), (1, 1500, 2048, 2048), (2, 8000, 1024, 256)]
GSCALES = (1.0, 0.3)  # one exact, one that is no power of two
# (B, F, T, fclip), both kinds: T == 1 and F == 2; fclip 1; T on either side of the 256-thread stride; three passes
LOSS_SHAPES = [(1, 2, 1, 2), (2, 5, 2, 1), (3, 33, 255, 33), (1, 9, 256, 4), (2, 9, 257, 9), (1, 3, 600, 2)]
ALPHAS = (1.0, 0.25)
EPS = 1e-7
# SSSLoss(n_fft = 64, overlap) on clips of 1000 samples: hops 32, 64 and 6
MODULE_N, MODULE_S, MODULE_OVERLAPS = 64, 1000, (0.5, 0.0, 0.9)


def clips(rng, B, S, floor=1e-3):
    """fp32 (B, S): six decaying sines per clip (200 Hz .. 12 kHz at 32 kHz, 20 .. 400 1/s) on a noise floor."""
    t = np.arange(S) / SR
    f = rng.uniform(200.0, 12000.0, (B, 6, 1))
    d = rng.uniform(20.0, 400.0, (B, 6, 1))
    ph = rng.uniform(0.0, 2.0 * np.pi, (B, 6, 1))
    amp = rng.uniform(0.2, 1.0, (B, 6, 1))
    return ((amp * np.exp(-d * t) * np.sin(2.0 * np.pi * f * t + ph)).sum(1) + floor * rng.standard_normal((B, S))).astype(np.float32)


def stft_inputs(case):
    """(x (B, S), gP (B, F, T)) fp32 for case = (B, S, n_fft, hop); fixed seed per case."""
    B, S, N, hop = case
    rng = np.random.default_rng([B, S, N, hop, 11])
    return clips(rng, B, S), rng.standard_normal((B, N // 2 + 1, n_frames(S, hop))).astype(np.float32)


def loss_inputs(case):
    """(Pp, Pt) fp32 (B, F, T) for case = (B, F, T, fclip): Pp log-uniform in [1e-9, 1e2], so both sides of eps = 1e-7 are
    visited; Pt = Pp bitwise for about 5 % of the elements and for at least one per row (when T == 1: for every other row),
    else Pp 2^(+-e) with e log-uniform in [0.003, 4] - the ratio is then outside [1 - 2^-10, 1 + 2^-10] (2^0.003 = 1.0021)
    also after the fp32 rounding of Pt, and sign(dlog), sign(dlin) are the same in fp32 and fp64."""
    B, F, T, fclip = case
    rng = np.random.default_rng([B, F, T, fclip, 13])
    Pp = (10.0 ** rng.uniform(-9.0, 2.0, (B, F, T))).astype(np.float32)
    e = np.exp(rng.uniform(np.log(0.003), np.log(4.0), (B, F, T))) * rng.choice([-1.0, 1.0], (B, F, T))
    Pt = (Pp.astype(np.float64) * 2.0 ** e).astype(np.float32)
    tie = rng.random((B, F, T)) < 0.05
    if T > 1:
        tie[np.arange(B)[:, None], np.arange(F)[None, :], rng.integers(0, T, (B, F))] = True
    else:
        tie[:, ::2, 0], tie[:, 1::2, 0] = True, False
    Pt[tie] = Pp[tie]
    ratio = Pp.astype(np.float64) / Pt.astype(np.float64)
    assert ((ratio == 1.0) | (np.abs(ratio - 1.0) > 2.0 ** -10)).all()
    return Pp, Pt


def module_inputs(overlap):
    """(x_pred, x_true) fp32 (2, MODULE_S) for the SSSLoss case.  The noise floor is 0.3 here.  A bin whose |Z| falls by chance
    far below its neighbours' has d log2(P + eps) / dP ~ 1 / P and an fp32 rounding error of Z that does not shrink with it, so
    the gradient of the loss expression itself moves between fp32 and fp64 spectrograms by ~(rounding error) sqrt(bins) /
    (typical |Z|): with the floor at 1e-3 that reaches 9e-4 for some draws, at 0.3 it stays below 2e-4
    (tests/test_stft_ref_cpu.py asserts it for these inputs)."""
    rng = np.random.default_rng([int(overlap * 100), 17])
    return clips(rng, 2, MODULE_S, 0.3), clips(rng, 2, MODULE_S, 0.3)
