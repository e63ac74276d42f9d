"""References and per-element error bounds for the two kernels of diffsound_amd/csrc/filtered_noise.hip (not a test
module).

The references are NumPy fp64 restatements of what the kernels compute, written from the kernels' header comment as
direct sums - no FFT anywhere (L = filter_coeff_length, T = 2 L - 1 taps, F = frame_length, nf = S // F + 1 frames):

``mag`` / ``dmag``          2 sigmoid(c)^2.3 + 1e-6 and its derivative 4.6 sigmoid^2.3 (1 - sigmoid),
``impulse``                 h[j] = z[(j - (L - 1)) mod T] w[j], z the cosine sum of mag over (k n) mod T, w periodic Hann,
``forward``                 ds_filtered_noise_fwd: out[b, f F + s] += gain sum_t noise[b, f, t] h[b, f, s - t], cut at S,
``backward``                ds_filtered_noise_bwd: gh = correlation of noise with gy (0 from S on), window, un-roll, cosine
                            sum, derivative of mag,
``bound_forward`` / ``bound_backward``   what the device result may differ from the reference by, derived from the code,
``round_like_kernel``       a CPU model of the kernels' roundings, optionally with one of ``FAULTS`` planted, so that a
                            bound that holds is shown to see a wrong kernel,
``torch_formulation``       the reference's chain of torch.fft operations, for fp64 autograd.

Notation of the bounds: u = 2^-24 (unit roundoff of fp32), gamma_k = k u / (1 - k u).  fp64 operations contribute
2^-52 each times the sum of the absolute terms (2^-52 rather than 2^-53 so that the reference's own fp64 arithmetic is
inside).  The kernels call NO fp32 transcendental: sigmoid, the power and the cosines are fp64 exp / pow / cospi whose
results round to fp32 once, so there is no expf / powf / cosf allowance; the fp64 routines are allowed ``TR64`` ulp of
fp64.  The ROCm documentation of the build image holds no accuracy table for the device's math library, so that figure
is a fallback: 8 ulp, of 2^-52 - it would have to be 10^7 times larger to matter next to u."""
import functools

import numpy as np

U32 = 2.0 ** -24
U64 = 2.0 ** -52
TR64 = 8.0
MAX_L, MAX_F = 129, 256


def gamma(k):
    return k * U32 / (1.0 - k * U32)


def _f64(x):
    return np.asarray(x, dtype=np.float64)


def _f32(x):
    return np.asarray(x, dtype=np.float32)


# ------------------------------------------------------------------------------------------------- references
def n_frames(S, F):
    return S // F + 1


def sigmoid(c):
    return 1.0 / (1.0 + np.exp(-_f64(c)))


def mag(c):
    return 2.0 * sigmoid(c) ** 2.3 + 1e-6


def dmag(c):
    s = sigmoid(c)
    return 4.6 * s ** 2.3 * (1.0 - s)


def window(T, periodic=True):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(T) / (T if periodic else T - 1))


@functools.lru_cache(maxsize=8)
def twiddles(L):
    """cos(2 pi ((k n) mod T) / T), (L, T); the integer k n is reduced first, so the argument is exact.  (Cached: callers
    read the table and leave it unchanged.)"""
    T = 2 * L - 1
    m = (np.arange(L)[:, None] * np.arange(T)[None, :]) % T
    return np.cos(2.0 * np.pi * m / T)


def _weights(L, doubled=True):
    ck = np.full(L, 2.0 if doubled else 1.0)
    ck[0] = 1.0
    return ck


def zero_phase(m):
    """z (..., T) of magnitudes m (..., L): (m_0 + 2 sum_{k >= 1} m_k cos(2 pi k n / T)) / T."""
    L = m.shape[-1]
    return (_f64(m) * _weights(L)) @ twiddles(L) / (2 * L - 1)


def impulse(c):
    """c (B, nf, L) logits -> h (B, nf, T)."""
    L = np.shape(c)[-1]
    return np.roll(zero_phase(mag(c)), L - 1, axis=-1) * window(2 * L - 1)


def _overlap_add(noise, h, S, F):
    """out (B, S) = sum over frames f and taps of noise[b, f, t] h[b, f, j] at sample f F + t + j, cut at S."""
    noise, h = _f64(noise), _f64(h)
    B, nf, T = h.shape
    y = np.zeros((B, nf, T + F - 1))
    for t in range(F):
        y[:, :, t:t + T] += noise[:, :, t, None] * h
    out = np.zeros((B, (nf - 1) * F + T + F - 1))
    for f in range(nf):
        out[:, f * F:f * F + T + F - 1] += y[:, f]
    return out[:, :S]


def forward(c, noise, S, F, gain=1.0):
    assert np.shape(c)[1] == n_frames(S, F) and np.shape(noise) == (*np.shape(c)[:2], F)
    return float(gain) * _overlap_add(noise, impulse(c), S, F)


def _gy_frames(gy, nf, T, F, fill=0.0):
    """(B, nf, T + F - 1): the samples f F ... f F + T + F - 2 of gy, ``fill`` from S on."""
    gy = _f64(gy)
    B, S = gy.shape
    ext = np.full((B, nf * F + T + F), float(fill))
    ext[:, :S] = gy
    return ext[:, np.arange(nf)[:, None] * F + np.arange(T + F - 1)[None, :]]


def _correlate(noise, gyf, T):
    """gh (B, nf, T) = sum_t noise[b, f, t] gyf[b, f, t + j]."""
    noise = _f64(noise)
    gh = np.zeros((*noise.shape[:2], T))
    for t in range(noise.shape[-1]):
        gh += noise[:, :, t, None] * gyf[:, :, t:t + T]
    return gh


def backward(gy, c, noise, S, F, gain=1.0):
    """gc (B, nf, L) = d / dc of sum gy forward(c, noise)."""
    B, nf, L = np.shape(c)
    T = 2 * L - 1
    gh = _correlate(noise, _gy_frames(gy, nf, T, F), T)
    gz = np.roll(gh * window(T), -(L - 1), axis=-1)
    gmag = (gz @ twiddles(L).T) * _weights(L) / T
    return float(gain) * gmag * dmag(c)


# ----------------------------------------------------------------------------------------------------- bounds
def terms_per_sample(S, L, F):
    """(S,): how many products the forward adds into each sample."""
    nf, T = n_frames(S, F), 2 * L - 1
    return np.rint(_overlap_add(np.ones((1, nf, F)), np.ones((1, nf, T)), S, F)[0]).astype(np.int64)


def bound_impulse(c):
    """(B, nf, T) against ``impulse``.

    mag rounds to fp32 once after fp64 exp / pow (relative u + TR64 2^-52), the twiddle rounds once; their product is exact
    in fp64 and the L-term sum, the doubling, the addition of mag_0 and the division are fp64:
        |z^ - z| <= E_z = (gamma_2 + (L + 8 + TR64) 2^-52) A_n,   A_n = (mag_0 + 2 sum_k mag_k |cos|) / T.
    z rounds to fp32, the window (float)(0.5 - 0.5 cospi) rounds once (its fp64 value is off by at most 4 2^-52 absolutely;
    w_0 = 0 exactly), and h = z w is one fp32 product:  |h^ - h| <= (1 + gamma_3) (w + 4 2^-52) E_z + gamma_3 |h| + 4 2^-52 |z|."""
    L = np.shape(c)[-1]
    T = 2 * L - 1
    m = mag(c)
    A = (m * _weights(L)) @ np.abs(twiddles(L)) / T
    E_z = (gamma(2) + (L + 8 + TR64) * U64) * A
    z = np.roll(zero_phase(m), L - 1, axis=-1)
    w = window(T)
    w4 = np.where(w > 0, w + 4 * U64, 0.0)
    return (1 + gamma(3)) * w4 * np.roll(E_z, L - 1, axis=-1) + gamma(3) * np.abs(z * w) + np.where(w > 0, 4 * U64, 0.0) * np.abs(z)


def bound_forward(c, noise, S, F, gain=1.0):
    """(B, S) against ``forward``.  The kernel adds the M products of a sample (``terms_per_sample``) by fp32 fmas into one
    accumulator, each rounding once, on impulse responses that are off by E_h = ``bound_impulse``:
        |acc^ - acc| <= E = sum |noise| E_h + gamma_M sum |noise| (|h| + E_h),
    and out = (float)(gain (double)acc) rounds once (the fp64 product adds 2^-52):  |gain| E (1 + 2 u) + (u + 2^-52) |out|."""
    L = np.shape(c)[-1]
    h, E_h = impulse(c), bound_impulse(c)
    an = np.abs(_f64(noise))
    M = terms_per_sample(S, L, F)[None, :]
    E = _overlap_add(an, E_h, S, F) + gamma(M) * _overlap_add(an, np.abs(h) + E_h, S, F)
    out = float(gain) * _overlap_add(noise, h, S, F)
    return abs(float(gain)) * E * (1 + 2 * U32) + (U32 + U64) * np.abs(out)


def bound_backward(gy, c, noise, S, F, gain=1.0):
    """(B, nf, L) against ``backward``.  gh_j is F fp32 fmas (zeros past S included): |gh^ - gh| <= gamma_F G_j, G_j =
    sum_t |noise_t gy_{t+j}|; the window's rounding and the product gh w add two more (and 4 2^-52 for the fp64 window):
    E_gz = (gamma_{F+2} + 4 2^-52) w G, un-rolled.  The twiddle rounds once and the T-term sum is fp64:
        |a^ - a| <= E_a = (1 + u) sum_n |cos| E_gz + (u + (T + 8) 2^-52) sum_n |gz cos|.
    gain, c_k / T and the derivative 4.6 sigmoid^2.3 (1 - sigmoid) are fp64 (exp, pow: TR64 ulp; 1 - sigmoid loses
    2^-52 / (1 - sigmoid) relatively), one fp32 rounding at the store:
        |gc^ - gc| <= |gain| (c_k / T) dmag E_a (1 + 2 u) + (u + (TR64 + 4 + 1 / (1 - sigmoid)) 2^-52) |gc|.
    A frame that starts at or after S has G = 0: bound 0, the gradient must be exactly zero."""
    B, nf, L = np.shape(c)
    T = 2 * L - 1
    gyf = _gy_frames(gy, nf, T, F)
    w = window(T)
    G = _correlate(np.abs(_f64(noise)), np.abs(gyf), T)
    gz = np.roll(_correlate(noise, gyf, T) * w, -(L - 1), axis=-1)
    E_gz = np.roll((gamma(F + 2) + 4 * U64) * w * G, -(L - 1), axis=-1)
    C = np.abs(twiddles(L)).T
    E_a = (1 + U32) * (E_gz @ C) + (U32 + (T + 8) * U64) * (np.abs(gz) @ C)
    ref = backward(gy, c, noise, S, F, gain)
    rel = U32 + (TR64 + 4 + 1.0 / (1.0 - sigmoid(c))) * U64
    return abs(float(gain)) * _weights(L) / T * dmag(c) * E_a * (1 + 2 * U32) + rel * np.abs(ref)


# ------------------------------------------------------------------------------- CPU model of the kernels' roundings
FAULTS = ("window", "roll", "undoubled", "oldest_frame", "tail", "one_minus_sigmoid")
"""Faults ``round_like_kernel`` can plant: a symmetric instead of a periodic Hann window; a roll of L instead of L - 1; the
bins k >= 1 not doubled; the oldest frame that reaches a sample dropped (forward); the tail past S not cut - the backward
reads ones instead of zeros from index S on; the factor (1 - sigmoid) missing in the backward."""
FORWARD_FAULTS = ("window", "roll", "undoubled", "oldest_frame")
BACKWARD_FAULTS = ("window", "roll", "undoubled", "tail", "one_minus_sigmoid")


def _rnd(x):
    """Round fp64 to fp32 and return it as fp64 (a product of two fp32 numbers is exact in fp64; a sum rounded to fp64 and
    then to fp32 can differ from the native fp32 fma by one ulp in rare ties)."""
    return _f64(x).astype(np.float32).astype(np.float64)


def round_like_kernel(c, noise, S, F, gain=1.0, gy=None, fault=None):
    """The kernels' recipe on the CPU: mag, twiddles and window rounded to fp32 once, fp64 cosine sums, z and h rounded
    where the kernel rounds, the convolution as fp32 multiply-adds in the kernel's order (frames ascending, t ascending),
    one rounding at each store.  Returns a dict of fp32 arrays: h, out and, with ``gy``, gc.  ``fault``: one of FAULTS."""
    assert fault is None or fault in FAULTS
    c, noise = _f32(c), _f32(noise)
    B, nf, L = c.shape
    T = 2 * L - 1
    gain = float(gain)
    shift = L if fault == "roll" else L - 1
    ck = _weights(L, doubled=fault != "undoubled")
    C32 = _rnd(twiddles(L))
    w32 = _rnd(window(T, periodic=fault != "window"))
    m32 = _rnd(mag(c))
    z32 = _rnd((m32 * ck) @ C32 / T)
    h = _rnd(np.roll(z32, shift, axis=-1) * w32)
    n64 = noise.astype(np.float64)
    reach = (T + F - 2) // F
    acc = np.zeros((B, S + T + F))
    j = np.arange(T)
    for f in range(nf):
        for t in range(F):
            o = f * F + t + j
            live = o < S
            if fault == "oldest_frame":
                live &= (o // F - f) != reach
            if not live.any():
                continue
            o = o[live]
            acc[:, o] = _rnd(acc[:, o] + n64[:, f, t, None] * h[:, f, live])
    out = dict(h=_f32(h), out=_f32(gain * acc[:, :S]))
    if gy is None:
        return out
    gyf = _gy_frames(_f32(gy), nf, T, F, fill=1.0 if fault == "tail" else 0.0)
    gh = np.zeros((B, nf, T))
    for t in range(F):
        gh = _rnd(gh + n64[:, :, t, None] * gyf[:, :, t:t + T])
    gz = np.roll(_rnd(gh * w32), -shift, axis=-1)
    a = (gz @ C32.T) * ck / T
    s = sigmoid(c)
    d = 4.6 * s ** 2.3 * (1.0 if fault == "one_minus_sigmoid" else 1.0 - s)
    gc = gain * a * d
    gc[:, np.arange(nf) * F >= S] = 0.0
    out["gc"] = _f32(gc)
    return out


# ----------------------------------------------------------------------------------------------- torch formulation
def torch_formulation(bank, noise, S, F, gain=1.0):
    """The reference's chain (src/ddsp/filtered_noise.py:20-67) at the dtype of ``bank``; autograd-capable."""
    import torch
    import torch.nn.functional as TF

    m = 2 * (torch.sigmoid(bank) ** 2.3) + 1e-6
    B, nf, L = m.shape
    T = 2 * L - 1
    ir = torch.fft.irfft(torch.complex(m, torch.zeros_like(m)), n=T, dim=-1)
    ir = torch.roll(ir, L - 1, dims=-1) * torch.hann_window(T, dtype=m.dtype)
    nfft = T + F - 1
    frames = torch.fft.irfft(torch.fft.rfft(noise, n=nfft) * torch.fft.rfft(ir, n=nfft), n=nfft) * gain
    total = (nf - 1) * F + nfft
    out = TF.fold(frames.transpose(1, 2), output_size=(1, total), kernel_size=(1, nfft), stride=(1, F)).reshape(B, total)
    return out[:, :S]


# ------------------------------------------------------------------------------------------- shapes and inputs
# (B, L, F, S).  (65, 64) are the module's defaults: a single sample; S < F, one live frame; F divides S, so the last frame
# contributes nothing (64: one live frame, 128: two); the cut inside overlapping tails (130, 200: three frames reach a
# sample, more than one workgroup in the backward).  (5, 3): four frames per sample.  (2, 7): T = 3, the shortest filter.
# (3, 1): F = 1, five frames per sample.  (129, 256): the upper limits, T = 257 taps on 256 threads, three workgroups.
SHAPES = [(2, 65, 64, 1), (2, 65, 64, 63), (2, 65, 64, 64), (2, 65, 64, 128), (2, 65, 64, 130), (2, 65, 64, 200),
          (2, 5, 3, 20), (2, 2, 7, 20), (2, 3, 1, 5), (2, 129, 256, 600)]
GAINS = (1.0, 0.7)  # one exact, one that is no power of two
REFUSED = {"L=1": dict(L=1), "L=130": dict(L=130), "F=0": dict(F=0), "F=257": dict(F=257), "S=0": dict(S=0)}
"""Arguments outside the native range, and the name the message must carry."""


def inputs(case):
    """(c (B, nf, L) in [-2, 2), noise (B, nf, F) in [-1, 1), gy (B, S) standard normal), fp32; fixed seed per case."""
    B, L, F, S = case
    rng = np.random.default_rng([B, L, F, S, 19])
    nf = n_frames(S, F)
    return (rng.uniform(-2.0, 2.0, (B, nf, L)).astype(np.float32), rng.uniform(-1.0, 1.0, (B, nf, F)).astype(np.float32),
            rng.standard_normal((B, S)).astype(np.float32))
