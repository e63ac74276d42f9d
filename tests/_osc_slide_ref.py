"""References, per-element error bounds and inputs for the sliding-contact bank of diffsound_amd/csrc/osc_slide.hip
(ds_osc_slide_fwd / ds_osc_slide_bwd).  Not a test module.

The kernels run a recurrence, x_m[t] = z_m (x_m[t-1] + g_m[t] f[t]).  The references here do NOT: as in
``_osc_driven_ref`` they build the closed-form mode signals with ``_osc_ref.bank_modes`` (phase in extended precision) and
convolve directly.  With sig_m[n] = e^{-d_m tau_n} sin(w_m tau_n), tau_n = (n + 1) / sr, and the interpolated gains

  g[a,m,t] = (1 - th) gain[a,m,k] + th gain[a,m,min(k+1, K-1)],  k = min(t // hop, K-1),  th = (t - k hop) / hop,
             th = 0 where t // hop >= K-1                                     (fp64 from the fp32 gains: ``interp``)

  y[a,t]       = sum_m amp[a,m] sum_{j < F, j <= t} g[a,m,j] f[a,j] sig_m[t-j]
  L[a,m,j]     = sum_{t >= j} gy[a,t] sig_m[t-j]                              (Im l_m[j] of the adjoint recurrence)
  gforce[a,j]  = sum_m g[a,m,j] amp[a,m] L[a,m,j]        (j < min(F, S); 0 for j >= S)
  ggain[a,m,k] = sum_j hat_k(j) f[a,j] amp[a,m] L[a,m,j]  (hat_k: the weight of frame k in g[., ., j]; ``hat``)
  gamp[a,m]    = sum_j g[a,m,j] f[a,j] L[a,m,j]
  gd[m]        = -sum_{a,j} amp g f sum_{t >= j} gy[a,t] tau sig_m[t-j],   gw[m] = the same with tau e^{-d tau} cos(w tau).

Bounds.  The driven bank's error model (``_osc_driven_ref``: K64 of the sum of magnitudes that enters an element, plus
one fp32 rounding, 2 u |ref|, for the outputs stored in fp32) holds for the chain of powers and for the sums, which are
those of osc_driven.hip.  What the sliding kernels add, per term:
  th = (off + i) (1 / hop): the integer converts exactly, 1 / hop and the product round (2 roundings; the reference divides:
       1 more); 1 - th: 1; the two products and the sum of the interpolation: 3, each relative to the interpolation's
       magnitude gmag = (1 - th) |gain_k| + th |gain_k+1| (a sign change between two frames cancels, so |g| is not it);
  the product g f (forward, gamp, gd / gw), am g (gforce) or the weights (1 - th) f Im l, th f Im l (ggain): 2;
  ggain: the lanes of a frame are added by a 6-step scan and the tiles of a frame in order: 6 + NT additions.
That is 12 + 6 + NT more roundings of the running magnitude than the driven bank's count, inside the same margin of 4:
      K64s = K64(driven) + 4 (18 + NT) 2^-53,
with every magnitude below built with gmag in place of |g| and |hat| = hat.  ggain is stored in fp32 like gamp: 2 u |ref|.

End to end (``grad_tolerance``): see there.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _osc_driven_ref as D  # noqa: E402
import _osc_ref as R  # noqa: E402

RUN, TILE, SR, U32, U64 = D.RUN, D.TILE, D.SR, D.U32, D.U64
ntiles = D.ntiles


def k64(A, m, S, chains=1):
    return D.k64(A, m, S, chains) + 4.0 * (18 + ntiles(S)) * U64


# ----------------------------------------------------------------------------------------------- interpolation
def hat(K, hop, n):
    """(K, n) fp64: hat[k, j] = the weight of frame k in the gain of sample j."""
    j = np.arange(n)
    kk = j // hop
    held = kk >= K - 1
    k = np.where(held, K - 1, kk)
    th = np.where(held, 0.0, (j - k * hop) / float(hop))
    H = np.zeros((K, n))
    H[k, j] += 1.0 - th
    H[np.minimum(k + 1, K - 1), j] += th
    return H


def interp(gain, hop, n):
    """g (A, m, n) fp64 from gain (A, m, K) fp32: (1 - th) gain_k + th gain_k+1 as the kernels form it."""
    gain = np.asarray(gain, dtype=np.float64)
    K = gain.shape[-1]
    j = np.arange(n)
    kk = j // hop
    held = kk >= K - 1
    k = np.where(held, K - 1, kk)
    th = np.where(held, 0.0, (j - k * hop) / float(hop))
    return (1.0 - th) * gain[..., k] + th * gain[..., np.minimum(k + 1, K - 1)]


# ------------------------------------------------------------------------------------------------ references
def forward(d, w, amp, force, gain, hop, S, sr=SR):
    """(y (A, S), Ymag (A, S)): the direct convolution and the sum of magnitudes entering each sample."""
    force = np.asarray(force, dtype=np.float64)
    A, F = force.shape
    m = len(d)
    n = min(F, S)
    _, env, sn, _ = R.bank_modes(d, w, S, sr)
    sig = env * sn
    am = R._amp(amp, A, m)
    coef = am[:, :, None] * interp(gain, hop, n) * force[:, None, :n]
    cmag = np.abs(am)[:, :, None] * interp(np.abs(gain), hop, n) * np.abs(force)[:, None, :n]
    y, Y = np.zeros((A, S)), np.zeros((A, S))
    for j in range(n):
        y[:, j:] += coef[:, :, j] @ sig[:, :S - j]
        Y[:, j:] += cmag[:, :, j] @ env[:, :S - j]
    return y, Y


def backward(gy, d, w, amp, force, gain, hop, sr=SR):
    """dict of references gforce (A, F), ggain (A, m, K), gamp (A, m), gd, gw (m,) and of the magnitudes behind each:
    Eg (A, F), Vg (A, m, K), V (A, m), W (m,)."""
    gy = np.asarray(gy, dtype=np.float64)
    force = np.asarray(force, dtype=np.float64)
    A, S = gy.shape
    F = force.shape[1]
    m, K = len(d), np.shape(gain)[-1]
    n = min(F, S)
    tau, env, sn, cs = R.bank_modes(d, w, S, sr)
    M = np.concatenate([env * sn, tau * env * sn, tau * env * cs, env, tau * env])  # (5 m, S)
    Gs = np.concatenate([gy, np.abs(gy)])                                            # (2 A, S)
    acc = np.zeros((5 * m, 2 * A, n))
    for j in range(n):
        acc[:, :, j] = M[:, :S - j] @ Gs[:, j:].T
    tr = lambda x: np.transpose(x, (1, 0, 2))                                        # -> (A, m, n)
    L, Ls, Lc = tr(acc[:m, :A]), tr(acc[m:2 * m, :A]), tr(acc[2 * m:3 * m, :A])
    Lmag, Ltmag = tr(acc[3 * m:4 * m, A:]), tr(acc[4 * m:, A:])
    am = R._amp(amp, A, m)[:, :, None]
    g, gmag = interp(gain, hop, n), interp(np.abs(gain), hop, n)
    f, fa = force[:, None, :n], np.abs(force)[:, None, :n]
    H = hat(K, hop, n)
    gforce, Eg = np.zeros((A, F)), np.zeros((A, F))
    gforce[:, :n] = (g * am * L).sum(1)
    Eg[:, :n] = (gmag * np.abs(am) * Lmag).sum(1)
    return dict(gforce=gforce, Eg=Eg,
                ggain=np.einsum("kj,amj->amk", H, f * am * L), Vg=np.einsum("kj,amj->amk", H, fa * np.abs(am) * Lmag),
                gamp=(g * f * L).sum(-1), V=(gmag * fa * Lmag).sum(-1),
                gd=-(am * g * f * Ls).sum((0, 2)), gw=(am * g * f * Lc).sum((0, 2)),
                W=(np.abs(am) * gmag * fa * Ltmag).sum((0, 2)))


# ---------------------------------------------------------------------------------------------------- bounds
def bound32(ref, mag, A, m, S):
    """y, gforce, gamp, ggain: one fp32 rounding at the store and the fp64 interior."""
    return 2.0 * U32 * np.abs(ref) + k64(A, m, S) * mag


def bound_gd_gw(W, A, m, S):
    return k64(A, m, S, chains=2) * W


# ------------------------------------------------------------------------------------- the recurrence on the CPU
def recurrence(d, w, amp, force, gain, hop, S, sr=SR, store32=False, round_state_at_tiles=False):
    """y of the recurrence x_m[t] = z_m (x_m[t-1] + g_m[t] f[t]) in complex128; ``store32`` rounds it to fp32 once, as the
    kernels' store does; ``round_state_at_tiles`` ALSO rounds the states to fp32 at every tile boundary, which the kernels
    do not do."""
    force = np.asarray(force, dtype=np.float64)
    A, F = force.shape
    m = len(d)
    n = min(F, S)
    inv = 1.0 / float(sr)
    z = np.exp(-np.asarray(d, dtype=np.float64) * inv) * np.exp(1j * (np.asarray(w, dtype=np.float64) * inv))
    am = R._amp(amp, A, m)
    u = interp(gain, hop, n) * force[:, None, :n]
    x = np.zeros((A, m), dtype=np.complex128)
    out = np.zeros((A, S))
    for t in range(S):
        x = z[None, :] * (x + (u[:, :, t] if t < n else 0.0))
        out[:, t] = (am * x.imag).sum(-1)
        if round_state_at_tiles and t % TILE == TILE - 1:
            x = x.astype(np.complex64).astype(np.complex128)
    return out.astype(np.float32) if store32 else out


def adjoint_recurrence(gy, d, w, amp, force, gain, hop, sr=SR, store32=False):
    """(gforce (A, F), ggain (A, m, K)) from l_m[t] = z_m (l_m[t+1] + gy[t]) in complex128."""
    gy = np.asarray(gy, dtype=np.float64)
    force = np.asarray(force, dtype=np.float64)
    A, S = gy.shape
    F = force.shape[1]
    m, K = len(d), np.shape(gain)[-1]
    n = min(F, S)
    inv = 1.0 / float(sr)
    z = np.exp(-np.asarray(d, dtype=np.float64) * inv) * np.exp(1j * (np.asarray(w, dtype=np.float64) * inv))
    am = R._amp(amp, A, m)
    l = np.zeros((A, m), dtype=np.complex128)
    gin = np.zeros((A, m, n))
    for t in range(S - 1, -1, -1):
        l = z[None, :] * (l + gy[:, t, None])
        if t < n:
            gin[:, :, t] = am * l.imag
    gforce = np.zeros((A, F))
    gforce[:, :n] = (interp(gain, hop, n) * gin).sum(1)
    ggain = np.einsum("kj,amj->amk", hat(K, hop, n), force[:, None, :n] * gin)
    if store32:
        return gforce.astype(np.float32), ggain.astype(np.float32)
    return gforce, ggain


def torch_chain(d, w, amp, force, gain, hop, S, sr=SR):
    """y as torch ops at d's dtype, autograd-capable in d, w, amp, force and gain (A, m, K): one convolution per mode."""
    import torch

    A, F = force.shape
    m, K = gain.shape[1], gain.shape[2]
    n = min(F, S)
    H = torch.from_numpy(hat(K, hop, n)).to(d.dtype)
    tau = (torch.arange(S, dtype=d.dtype) + 1) / sr
    sig = torch.exp(-d[:, None] * tau[None]) * torch.sin(w[:, None] * tau[None])     # (m, S)
    u = (gain.to(d.dtype) @ H) * force[:, None, :n]                                     # (A, m, n)
    if amp is not None:
        u = u * amp[:, :, None]
    idx = torch.arange(S)[None, :] - torch.arange(n)[:, None]                          # t - j
    ok = (idx >= 0).to(d.dtype)
    Sm = sig[:, idx.clamp(min=0)] * ok[None]                                            # (m, n, S)
    return torch.einsum("amj,mjt->at", u, Sm)


# ------------------------------------------------------------------------------------------- shapes and inputs
MODE_SETS = D.MODE_SETS
S3 = 2 * TILE + RUN + 1


def frames_needed(S, F, hop):
    """Frames that a driven sample touches: the last driven sample n - 1 lies in interval (n - 1) // hop and weighs on the
    frame after it unless it sits on the frame itself."""
    n = min(F, S)
    last = n - 1
    return last // hop + (2 if last % hop else 1)


# (A, m, F, S, K, hop, mode set, with_amp).  S over {1, 15, 16, 17, hop, hop + 1, TILE - 1, TILE, TILE + 1, 2 TILE + RUN + 1},
# hop over {16, 48, 1024, 1040, above S}, K over {1, exactly enough, one too few, several too many}, F over {1, S - 1, S,
# S + 7}, m over {1, 5, 70}, A over {1, 3}, the four mode sets.  K: E = frames_needed.
CASES = [
    (1, 1, 1, 1, 1, 16, "material", True),                       # smallest; K = 1
    (3, 5, 14, 15, 2, 16, "d0", False),                          # S = 15, F = S - 1, exactly enough
    (1, 70, 16, 16, 5, 16, "nyquist", True),                     # S = hop = 16, several too many, 70 modes
    (3, 1, 24, 17, 2, 16, "underflow", True),                    # S = hop + 1 = 17, F = S + 7, exactly enough
    (1, 5, 48, 48, 1, 48, "material", True),                     # S = hop = 48, K = 1
    (3, 70, 48, 49, 2, 48, "d0", True),                          # S = hop + 1 = 49, exactly enough
    (1, 5, TILE - 2, TILE - 1, 64, 16, "material", True),        # one too few at hop 16 (E = 65)
    (3, 5, TILE - 1, TILE - 1, 23, 48, "nyquist", False),        # hop 48 against the tile, exactly enough (E = 23)
    (1, 1, TILE, TILE, 2, 1024, "d0", True),                     # S = hop = TILE, exactly enough
    (3, 5, TILE + 7, TILE, 9, 1040, "underflow", True),          # hop above S, several too many
    (1, 5, TILE + 1, TILE + 1, 3, 1024, "material", True),       # S = hop + 1, one frame more than enough
    (3, 1, TILE, TILE + 1, 22, 48, "d0", False),                 # hop 48 across the tile boundary, one too few (E = 23)
    (1, 5, 1041, 1041, 2, 1040, "nyquist", True),                # S = hop + 1 at hop 1040 > TILE
    (1, 5, S3, S3, 130, 16, "material", True),                   # three tiles at hop 16, exactly enough
    (3, 5, S3 - 1, S3, 43, 48, "underflow", True),               # three tiles at hop 48, one too few (E = 44)
    (1, 5, S3 + 7, S3, 2, 1040, "d0", True),                     # frame spans a whole tile; one too few (E = 3)
    (3, 1, S3, S3, 4, 1024, "nyquist", False),                   # hop = TILE, one more than enough
    (1, 70, 1, S3, 7, 1040, "material", True),                   # F = 1: one driven sample, six untouched frames
    (1, 5, S3, S3, 1, 2080, "material", True),                   # hop above S, K = 1
    (3, 5, 1040, 1040, 3, 1040, "material", True),               # S = hop = 1040, several too many
]


def case_id(case):
    return "-".join(map(str, case))


def inputs(case):
    """(d, w (m,) fp64, amp (A, m) fp32 or None, force (A, F) fp32, gain (A, m, K) fp32, gy (A, S) fp32); fixed seed per
    case.  The gains are standard normal (sign changes) with every seventh one zero."""
    A, m, F, S, K, hop, modes, with_amp = case
    rng = np.random.default_rng([A, m, F, S, K, hop, MODE_SETS.index(modes), int(with_amp), 47])
    w = R.TWO_PI * np.sort(rng.uniform(50.0, 15000.0, m))
    d = rng.uniform(1.0, 400.0, m)
    if modes == "d0":
        d = np.zeros(m)
    elif modes == "underflow":
        d[::2] = 3.0e4
    elif modes == "nyquist":
        w = SR * (np.pi - rng.uniform(1e-3, 1e-2, m))
    amp = rng.uniform(0.5, 1.5, (A, m)).astype(np.float32) if with_amp else None
    force = rng.standard_normal((A, F)).astype(np.float32)
    gain = rng.standard_normal((A, m, K)).astype(np.float32)
    gain.reshape(-1)[::7] = 0.0
    gy = rng.standard_normal((A, S)).astype(np.float32)
    return d, w, amp, force, gain, gy


# ------------------------------------------------------------------------------------------------ end to end
def grad_tolerance(y, Ymag, target, Tmag, dYmag):
    """What the device gradient of loss = mean((y - target)^2) with respect to a path parameter p may differ by from a
    central difference of the fp64 restatement, fed the same U_hat.  y is linear in the gains and, on P1 faces, the gains
    are affine in the points while no point changes its face, so the loss is a quadratic in p and its central difference
    exact; what is left is the device's fp32 (u = 2^-24), as in ``_mode_sample_ref``:
      * each render carries, per sample, the store's rounding (2 u |y| <= 2 u Ymag) and the fp32 roundings of what feeds
        it - the barycentrics and the direction inside ds_mode_sample_fwd and the gains handed to ds_osc_slide_fwd, one
        u each of the magnitude Ymag that enters the sample: 5 u Ymag[t], and 5 u Tmag[t] for the target;
      * gy = 2 r / N is rounded to fp32 once: u |r[t]|;
      * these errors of gy[t] reach the gradient through |dy[t]/dp| <= dYmag[t], the forward magnitude of the gains'
        derivative:  (2 / N) sum_t (5 u (Ymag + Tmag) + u |r|)[t] dYmag[t];
      * the adjoint itself (ggain stored in fp32: 2 u, its transposition into the fp32 direction and barycentrics of
        ds_mode_sample_bwd: 2 u, the fp64 interior far below) adds at most 8 u (2 / N) sum_t |r[t]| dYmag[t] with a
        factor 2 of margin.
    All arrays (A, S) fp64 from the restatement; dYmag = ``forward`` magnitude with |d gain / dp| as gains."""
    y, Ymag, target, Tmag, dYmag = (np.asarray(x, dtype=np.float64) for x in (y, Ymag, target, Tmag, dYmag))
    N = y.size
    r = np.abs(y - target)
    return (2.0 / N) * (((5 * U32) * (Ymag + Tmag) + U32 * r) * dYmag).sum() + 8 * U32 * (2.0 / N) * (r * dYmag).sum()
