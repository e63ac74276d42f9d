"""References, per-element error bounds and inputs for the driven oscillator bank of diffsound_amd/csrc/osc_driven.hip
(ds_osc_driven_fwd / ds_osc_driven_bwd).  Not a test module.

The kernels run a recurrence, x[t] = z (x[t-1] + f[t]).  The references here do NOT: they build the closed-form mode
signals e^{-d tau} sin(w tau) with ``_osc_ref.bank_modes`` (phase in extended precision) and convolve directly,

  y[a,t]      = sum_{j < F, j <= t} f[a,j] s_a[t-j],      s_a[n] = sum_m amp[a,m] e^{-d_m tau_n} sin(w_m tau_n), tau_n = (n+1)/sr
  gforce[a,j] = sum_{t >= j} gy[a,t] s_a[t-j]             (j < min(F, S); 0 for j >= S)
  c[a,n]      = sum_j f[a,j] gy[a,j+n]                    (every pair (t, j) with t - j = n)
  gamp[a,m]   = sum_n c[a,n] e^{-d tau_n} sin(w tau_n)
  gd[m]       = -sum_{a,n} amp c tau_n e^{-d tau_n} sin(w tau_n),   gw[m] = sum_{a,n} amp c tau_n e^{-d tau_n} cos(w tau_n).

Bounds, derived from the code of osc_driven.hip (no constant comes from a run):

fp32.  y, gforce and gamp are summed in fp64 registers and rounded to fp32 ONCE, at the store: u |ref|, u = 2^-24
  (2 u with the cross term of the fp64 error).  gd and gw are stored in fp64: no fp32 term.
fp64.  A term f[j] amp Im z^(t-j+1) reaches sample t through a chain of multiplications whose powers add up to exactly
  t - j + 1: at most RUN single steps by z in the lane of j, the lane scan (6 steps, powers z^(RUN 2^k)), one z^TILE per
  tile crossed (NT(S) - 1 at most), the lane's entry power z^(RUN q), and at most RUN single steps in the lane of t.  Each
  factor z^n is exp(-d n / sr) (cos, sin)(w n / sr) with n / sr and the two products rounded: a relative error of at
  most 2 (w n / sr) 2^-53 <= 2 pi n 2^-53 in the phase (w / sr <= pi), (d n / sr) 2^-53 in the modulus - below 745 2^-53
  wherever the power is not already 0 - and about 4 2^-53 for exp, sincos and the complex product that applies it.
  Summed along the chain: (2 pi S + 745 + 4 J) 2^-53 of the term's magnitude, J = 2 RUN + 6 + NT + 1 jumps.  The sums
  over taps, modes, lanes and clips add at most one 2^-53 per addition on the running sum of magnitudes: RUN NT + 6 per
  lane for the reductions over time, m over modes, A over clips; the reference's own direct sum adds S 2^-53.  With
  every term measured against the sum of magnitudes that enters the element,
      K64 = 4 (2 pi S + 745 + 4 (2 RUN + NT + 7) + RUN NT + 6 + m + A + S) 2^-53           (the 4: a margin)
  and, for gd / gw, where a product (x[t-1] + f[t]) l[t] carries two chains whose lengths add up to at most S + 1, twice
  the jump count: the same K64 with 8 in place of 4.
Magnitudes.  E[a,n] = sum_m |amp| e^{-d tau_n} (from ``_osc_ref.bank_forward``):
      y:      sum_j |f[j]| E[t-j]          gforce: sum_{t >= j} |gy[t]| E[t-j]
      gamp:   V[a,m] = sum_n |c|[a,n] e^{-d tau_n},   gd, gw: W[m] = sum_{a,n} |amp| |c|[a,n] tau_n e^{-d tau_n}
  with |c| = corr(|gy|, |f|): exactly the V and W of ``_osc_ref.bank_backward`` on absolute values (sum_t of the
  magnitudes of x[t-1] + f[t] and l[t] multiplied out gives the same sum over pairs (t, j), each with its tau).
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _osc_ref as R  # noqa: E402

RUN = 16            # samples per lane          (csrc/osc_driven.hip)
TILE = 64 * RUN     # samples per wavefront tile
SR = R.SR
U32 = R.U32
U64 = 2.0 ** -53


def ntiles(S):
    return -(-S // TILE)


def k64(A, m, S, chains=1):
    NT = ntiles(S)
    return 4.0 * (2 * np.pi * S + 745 + 4 * chains * (2 * RUN + NT + 7) + RUN * NT + 6 + m + A + S) * U64


# ------------------------------------------------------------------------------------------------ references
def forward(d, w, amp, force, S, sr=SR):
    """(y (A, S), Emag (A, S)): the direct convolution and the sum of magnitudes entering each sample."""
    y, E = R.bank_forward(d, w, amp, force, S, sr)
    return y, R.fir(E, np.abs(np.asarray(force, dtype=np.float64)))


def _signal(d, w, amp, A, S, sr):
    _, env, sn, _ = R.bank_modes(d, w, S, sr)
    am = R._amp(amp, A, len(env))
    return am @ (env * sn), np.abs(am) @ env


def backward(gy, d, w, amp, force, sr=SR):
    """dict of references gforce (A, F), gamp (A, m), gd, gw (m,) and magnitudes Eg (A, F), V (A, m), W (m,)."""
    gy = np.asarray(gy, dtype=np.float64)
    force = np.asarray(force, dtype=np.float64)
    A, S = gy.shape
    F = force.shape[1]
    s, E = _signal(d, w, amp, A, S, sr)
    gforce, Eg = np.zeros((A, F)), np.zeros((A, F))
    for j in range(min(F, S)):
        gforce[:, j] = (gy[:, j:] * s[:, :S - j]).sum(-1)
        Eg[:, j] = (np.abs(gy[:, j:]) * E[:, :S - j]).sum(-1)
    gd, gw, gamp, _, _ = R.bank_backward(R.corr(gy, force), d, w, amp, sr)
    cabs = R.corr(np.abs(gy), np.abs(force))
    _, _, _, W, V = R.bank_backward(cabs, d, w, None if amp is None else np.abs(amp), sr)
    return dict(gforce=gforce, gamp=gamp, gd=gd, gw=gw, Eg=Eg, V=V, W=W)


# ---------------------------------------------------------------------------------------------------- bounds
def bound_y(ref, Emag, A, m, S):
    return 2.0 * U32 * np.abs(ref) + k64(A, m, S) * Emag


def bound_gforce(ref, Eg, A, m, S):
    return 2.0 * U32 * np.abs(ref) + k64(A, m, S) * Eg


def bound_gamp(ref, V, A, m, S):
    return 2.0 * U32 * np.abs(ref) + k64(A, m, S) * V


def bound_gd_gw(W, A, m, S):
    return k64(A, m, S, chains=2) * W


# ------------------------------------------------------------------------------------- the recurrence on the CPU
def recurrence(d, w, amp, drive, S, sr=SR, reverse=False, round_state_at_tiles=False, store32=False):
    """sum_m amp Im x_m with x[t] = z (x[t-1] + drive[t]) in complex128, drive (A, L) zero from L on, S samples; with
    ``reverse`` time runs down from S - 1 (the adjoint: drive = gy).  ``store32`` rounds the result to fp32 once, as
    the kernels' store does; ``round_state_at_tiles`` ALSO rounds the state to fp32 wherever it crosses a tile boundary
    - which the kernels do not do (a wrong kernel for the bounds to catch)."""
    drive = np.asarray(drive, dtype=np.float64)
    A, L = drive.shape
    m = len(d)
    inv = 1.0 / float(sr)
    z = np.exp(-np.asarray(d, dtype=np.float64) * inv) * np.exp(1j * (np.asarray(w, dtype=np.float64) * inv))
    am = R._amp(amp, A, m)
    x = np.zeros((A, m), dtype=np.complex128)
    out = np.zeros((A, S))
    order = range(S - 1, -1, -1) if reverse else range(S)
    for t in order:
        f = drive[:, t] if t < L else np.zeros(A)
        x = z[None, :] * (x + f[:, None])
        out[:, t] = (am * x.imag).sum(-1)
        leaving = (t % TILE == 0) if reverse else (t % TILE == TILE - 1)
        if round_state_at_tiles and leaving:
            x = x.astype(np.complex64).astype(np.complex128)
    return out.astype(np.float32) if store32 else out


# ------------------------------------------------------------------------------------------- shapes and inputs
MODE_SETS = ("material", "d0", "underflow", "nyquist")
FORCES = ("impulse", "dense", "last")
# (A, m, F, S, mode set, force, with_amp): S over {1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 TILE + RUN + 1}, F over
# {1, 2, 512, 513, S - 1, S, S + 7}, m over {1, 3, 4, 5, 17}, A over {1, 3}; every pair of (S, F class), (S, mode set),
# (mode set, force) and both amp forms appear.
S3 = 2 * TILE + RUN + 1
CASES = [
    (1, 1, 1, 1, "material", "impulse", True),
    (3, 3, 8, 1, "d0", "dense", False),
    (1, 4, 2, 63, "nyquist", "dense", True),
    (3, 5, 62, 63, "underflow", "last", True),
    (1, 17, 64, 64, "material", "dense", False),
    (3, 1, 72, 65, "d0", "last", True),
    (1, 3, 512, TILE - 1, "underflow", "dense", True),
    (3, 4, 513, TILE - 1, "nyquist", "impulse", True),
    (1, 5, TILE - 1, TILE, "material", "last", True),
    (3, 17, TILE, TILE, "d0", "dense", True),
    (1, 4, TILE + 8, TILE + 1, "underflow", "dense", False),
    (3, 3, 513, TILE + 1, "material", "dense", True),
    (1, 17, S3, S3, "nyquist", "dense", True),
    (3, 5, 513, S3, "underflow", "last", True),
    (1, 1, 2, S3, "d0", "impulse", True),
    (3, 4, S3 + 7, S3, "material", "dense", False),
    (1, 5, 512, S3, "nyquist", "last", True),
]


def case_id(case):
    return "-".join(map(str, case))


def inputs(case):
    """(d, w (m,) fp64, amp (A, m) fp32 or None, force (A, F) fp32, gy (A, S) fp32); fixed seed per case."""
    A, m, F, S, modes, fk, with_amp = case
    rng = np.random.default_rng([A, m, F, S, MODE_SETS.index(modes), FORCES.index(fk), int(with_amp), 43])
    w = R.TWO_PI * np.sort(rng.uniform(50.0, 15000.0, m))
    d = rng.uniform(1.0, 400.0, m)          # the range of the material scripts
    if modes == "d0":
        d = np.zeros(m)
    elif modes == "underflow":                # z^TILE = exp(-960) = 0 for every other mode
        d[::2] = 3.0e4
    elif modes == "nyquist":
        w = SR * (np.pi - rng.uniform(1e-3, 1e-2, m))
    amp = rng.uniform(0.5, 1.5, (A, m)).astype(np.float32) if with_amp else None
    n = min(F, S)
    force = np.zeros((A, F), dtype=np.float32)
    if fk == "impulse":
        force[:, 0] = 1.0
    elif fk == "last":                        # the only non-zero tap is the last one inside S
        force[:, n - 1] = rng.uniform(0.5, 1.5, A).astype(np.float32)
    else:
        force[:] = rng.standard_normal((A, F)).astype(np.float32)
    gy = rng.standard_normal((A, S)).astype(np.float32)
    return d, w, amp, force, gy
