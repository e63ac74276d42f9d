"""References, per-element error bounds and inputs for the delay line of diffsound_amd/csrc/delay.hip (ds_delay_fwd /
ds_delay_bwd).  Not a test module.

The kernels split the read position p into n = floor(p) and f and walk 16 taps.  The references here do NOT: they evaluate
the definitions as dense sums over every input j, in fp64 numpy,

  tau(t)     = tau_k + th (tau_k+1 - tau_k),  k, th the frames of ``_osc_slide_ref`` (last frame held),   p(t) = t - tau(t)
  h(u)       = sinc(u) cos^2(pi u / (2 R)) for |u| < R, 0 outside,  R = 8
  y[b,t]     = sum_j h(p[b,t] - j) s[b,j]
  gs[b,j]    = sum_t gy[b,t] h(p[b,t] - j)
  gtau[b,k]  = - sum_t hat_k(t) gy[b,t] sum_j s[b,j] h'(p[b,t] - j)

(a non-finite p gives NaN in y).  h' = sinc' win + sinc win', sinc'(u) = (cos(pi u) - sinc(u)) / u, which cancels near 0: below
|u| = 1/8 it is summed as a series here too (``dsinc``); tests/test_delay_ref_cpu.py holds it against differences of h.

Bounds, derived and counted.  U32 = 2^-24, U64 = 2^-53 (half an ulp).  NS = 4: the ulps granted to one device sin / cos
(sincospi in fp64; the math library documents 2).  One weight of the device is
  w = [(-1)^i sin(pi f) / (pi (f - i))] * [0.5 (1 + cos(pi f / R) C_i + sin(pi f / R) S_i)],  C_i, S_i a table of cos, sin(pi i / R):
  * the sinc factor carries RELATIVE errors: NS (sin), 1 (pi u), 1 (the division); then the product with the window 1, the
    product with s 1: NS + 4, and the sum of the taps at most NADD roundings (16 forward, 4R + 1 = 33 in the gather)
    -> (NS + 4 + NADD) U64 of sum |w s|                                                                        ("mag")
  * the window's bracket carries ABSOLUTE errors (its terms are <= 1 whatever the window's own size): 2 NS (cos, sin), 1 (the
    two table entries, half an ulp each), 2 products, 2 sums -> (2 NS + 5) U64, times |sinc| |s| summed       ("smag")
  * both doubled: the reference forms the same quantities with roundings of its own.
  * the reference's np.sinc reduces its argument in fp64, sin(fl(pi u)) / fl(pi u): pi u is off by up to 2 U64 pi |u|, the sine
    by as much, the quotient by 2 U64 - ABSOLUTE, however small sinc(u) is next to an integer u (the device reduces f, not
    u: none of this).  With a factor 2 of margin: 4 U64 times |s| summed over the taps                          ("sabs")
  -> e64 = 2 U64 ((NS + 4 + NADD) mag + (2 NS + 5) smag) + 4 U64 sabs.
The read position: th takes 2 roundings (1 / hop, the product; the reference divides: 1), tau_k+1 - tau_k 1, the product 1,
the sum 1 and t - tau 1, each at most U64 of a quantity below t + |tau_k| + |tau_k+1|; the reference's own p has as many:
  -> |dp| <= EP U64 (t + |tau_k| + |tau_k+1|),  EP = 12, and it moves a sum by |dp| sum |s h'(p - j)|              ("dmag")
     to first order (h' is Lipschitz with constant < 4; the second order, dp^2, is far below U64).
  Because h is continuous and a tap enters at weight 0 - value AND slope vanish at +-R - a different floor(p) at f ~ 0 (the
  device takes n one lower or higher than p's true floor) changes the sum by no more than this same term: the tap that
  enters or leaves has weight |h'| |dp| at most, which dmag already counts.  The same holds for a sample that the gather's
  search admits or leaves out at the end of a run.
The stored fp32: 2 U32 |ref| (one rounding, on a value itself in error) and 2^-150 for the fp32 subnormals.
  bound(y)  = 2 U32 |y| + e64(NADD = 16) + EP U64 (t + |tau|..) dmag + 2^-150,       bound(gs) the same with NADD = 33.
gtau (stored in fp64).  q[t] = gy[t] D[t], D = sum_j s_j h'(p - j).  One h' of the device: sinc' by the quotient with |u| >= 1/8
carries (2 NS + 3) U64 / |u| <= 8 (2 NS + 3) U64 = 88 U64 absolute (the series branch far less), times the window <= 1; the
window's (2 NS + 5) U64 times |sinc'| <= 1.5; sinc win' with |win'| <= pi / 16 as much again: below ED = 130 U64 absolute per
tap, so |dD| <= 2 ED U64 sabs + 2 (16 + 2) U64 dmag, sabs the sum of |s| over the taps, dmag as above; the read position moves D
by |dp| sum |s h''| <= 4 |dp| sabs.  The sum over a frame: lane by lane at most ceil(S / 64) additions, 6 in the butterfly,
2 roundings of th, 2 products -> (S / 64 + 12) U64 of sum hat |gy| dmag.
  bound(gtau[k]) = sum_t hat_k(t) |gy| [U64 (2 ED sabs + 36 dmag) + 4 EP U64 (t + |tau|..) sabs] + (S / 64 + 12) U64 sum_t hat_k |gy| dmag;
a frame that no sample touches has bound 0: only an exact 0 passes.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _osc_slide_ref as SL  # noqa: E402

R = 8                 # DS_DELAY_HALF_TAPS
MAX_SLOPE = 0.5       # DS_DELAY_MAX_SLOPE
TILE = 256            # outputs per workgroup of csrc/delay.hip (T, and GT of the gather)
U32, U64 = 2.0 ** -24, 2.0 ** -53
TINY32 = 2.0 ** -150
NS, EP, ED = 4, 12, 130
hat = SL.hat


# ---------------------------------------------------------------------------------------------------- the kernel h
def window(u):
    return np.cos(np.pi * u / (2 * R)) ** 2


def h(u):
    u = np.asarray(u, dtype=np.float64)
    return np.where(np.abs(u) < R, np.sinc(u) * window(u), 0.0)


def dsinc(u):
    """sinc'(u): the quotient (cos(pi u) - sinc(u)) / u, and below |u| = 1/8 the series -pi^2 u sum_k (-x)^(k-1) 2k / (2k+1)!,
    x = (pi u)^2, through k = 7."""
    u = np.asarray(u, dtype=np.float64)
    x = (np.pi * np.clip(u, -1.0, 1.0)) ** 2
    c = [1 / 3, 1 / 30, 1 / 840, 1 / 45360, 1 / 3991680, 1 / 518918400, 1 / 93405312000]
    ser = np.zeros_like(u)
    for ck in reversed(c):
        ser = ck - x * ser
    small = np.abs(u) < 0.125
    safe = np.where(small, 1.0, u)
    return np.where(small, -(np.pi ** 2) * u * ser, (np.cos(np.pi * safe) - np.sinc(safe)) / safe)


def dh(u):
    u = np.asarray(u, dtype=np.float64)
    dwin = -(np.pi / (2 * R)) * np.sin(np.pi * u / R)
    return np.where(np.abs(u) < R, dsinc(u) * window(u) + np.sinc(u) * dwin, 0.0)


# --------------------------------------------------------------------------------------------------- references
def frames(K, hop, S):
    """(k, k1, th) per sample t < S: the frames of the sliding bank."""
    t = np.arange(S)
    kk = t // hop
    held = kk >= K - 1
    k = np.where(held, K - 1, kk)
    th = np.where(held, 0.0, (t - k * hop) / float(hop))
    return k, np.minimum(k + 1, K - 1), th


def positions(tau, hop, S):
    """(p (B, S), pmag (B, S) = t + |tau_k| + |tau_k+1|)."""
    tau = np.asarray(tau, dtype=np.float64)
    k, k1, th = frames(tau.shape[1], hop, S)
    t = np.arange(S, dtype=np.float64)
    a, b = tau[:, k], tau[:, k1]
    with np.errstate(invalid="ignore"):                                                  # (inf - inf of a non-finite tau)
        return t - (a + th * (b - a)), t + np.abs(a) + np.abs(b)


def _dense(tau, hop, S):
    """U[b,t,j] = p[b,t] - j; a non-finite p is kept out of the sums (its weights are 0) and marked."""
    p, pmag = positions(tau, hop, S)
    bad = ~np.isfinite(p)
    U = np.where(bad, 1e300, p)[:, :, None] - np.arange(S, dtype=np.float64)[None, None, :]
    return U, pmag, bad


def forward(s, tau, hop):
    """dict y, and the magnitudes mag, smag, dmag, pmag (all (B, S))."""
    s = np.asarray(s, dtype=np.float64)
    U, pmag, bad = _dense(tau, hop, s.shape[1])
    W = h(U)
    inside = np.abs(U) < R
    y = np.einsum("btj,bj->bt", W, s)
    y[bad] = np.nan
    return dict(y=y, mag=np.einsum("btj,bj->bt", np.abs(W), np.abs(s)),
                smag=np.einsum("btj,bj->bt", np.abs(np.sinc(U)) * inside, np.abs(s)),
                dmag=np.einsum("btj,bj->bt", np.abs(dh(U)), np.abs(s)), pmag=pmag,
                sabs=np.einsum("btj,bj->bt", inside.astype(np.float64), np.abs(s)))


def backward(gy, s, tau, hop):
    """dict gs (B, S) with mag, smag, dmag (pmag folded in); gtau (B, K) with its bound's parts."""
    gy, s, tau = (np.asarray(x, dtype=np.float64) for x in (gy, s, tau))
    B, S = s.shape
    K = tau.shape[1]
    U, pmag, _ = _dense(tau, hop, S)
    W, DW = h(U), dh(U)
    inside = np.abs(U) < R
    ag = np.abs(gy)
    out = dict(gs=np.einsum("bt,btj->bj", gy, W), gs_mag=np.einsum("bt,btj->bj", ag, np.abs(W)),
               gs_smag=np.einsum("bt,btj->bj", ag, np.abs(np.sinc(U)) * inside),
               gs_dp=np.einsum("bt,btj->bj", ag * pmag, np.abs(DW)), gs_sabs=np.einsum("bt,btj->bj", ag, inside.astype(np.float64)))
    D = np.einsum("btj,bj->bt", DW, s)
    dmag = np.einsum("btj,bj->bt", np.abs(DW), np.abs(s))
    sabs = np.einsum("btj,bj->bt", inside.astype(np.float64), np.abs(s))
    Hk = hat(K, hop, S)                                                                  # (K, S)
    out["gtau"] = -np.einsum("kt,bt->bk", Hk, gy * D)
    per = ag * (U64 * (2 * ED * sabs + 36 * dmag) + 4 * EP * U64 * pmag * sabs)
    out["gtau_bound"] = np.einsum("kt,bt->bk", Hk, per) + (S / 64.0 + 12) * U64 * np.einsum("kt,bt->bk", Hk, ag * dmag)
    return out


# ------------------------------------------------------------------------------------------------------- bounds
def e64(mag, smag, sabs, nadd):
    return 2 * U64 * ((NS + 4 + nadd) * mag + (2 * NS + 5) * smag) + 4 * U64 * sabs


def bound_y(f):
    ok = np.isfinite(f["y"])                                                           # (a NaN of the reference has no bound)
    ref, pmag = np.where(ok, f["y"], 0.0), np.where(ok, f["pmag"], 0.0)
    return 2 * U32 * np.abs(ref) + e64(f["mag"], f["smag"], f["sabs"], 2 * R) + EP * U64 * pmag * f["dmag"] + TINY32


def bound_gs(b):
    return 2 * U32 * np.abs(b["gs"]) + e64(b["gs_mag"], b["gs_smag"], b["gs_sabs"], 4 * R + 1) + EP * U64 * b["gs_dp"] + TINY32


def passband_error(nu, grid=4097):
    """E(nu) = max_f |G(f) - 1|,  G(f) = sum_{i = -R+1 .. R} h(f - i) e^{2 pi i nu (i - f)}, over ``grid`` values of f in [0, 1]: how far
    the 16 taps are from an ideal delay of a tone at nu cycles per sample.  So that the value holds BETWEEN the grid's points
    too, half a grid step times the largest |G'| on the grid is added (G' from h'; G is nearly constant, so this is small)."""
    f = np.linspace(0.0, 1.0, grid)[:, None]
    i = np.arange(-R + 1, R + 1)[None, :]
    ph = np.exp(2j * np.pi * nu * (i - f))
    G = (h(f - i) * ph).sum(1)
    dG = ((dh(f - i) - 2j * np.pi * nu * h(f - i)) * ph).sum(1)
    return float(np.abs(G - 1.0).max() + np.abs(dG).max() * 0.5 / (grid - 1))


# ------------------------------------------------------------------------------------------- shapes and inputs
def frames_needed(S, hop):
    last = S - 1
    return last // hop + (2 if last % hop else 1)


S3 = 2 * TILE + R + 3
# (B, S, K, hop, delay).  S over {1, R, 2R - 1, T - 1, T, T + 1, 2T + R + 3}; B over {1, 3}; K = 1; K = 2 (the last frame held for
# most of the clip); hop 16 and 48 (at 48 a frame interval straddles the tile boundary at 256); exactly the frames needed, and
# frames past S (their gtau is exactly 0).  Delays: "zero"; "int" (an integer N: an exact shift); "half" (N + 0.5); "far"
# (S + R + 1.5: nothing is read); "up" / "down" (ramps at the slope limit +0.5 / -0.5 a sample: p rises by 0.5 / 1.5);
# "random" (frame steps uniform within the limit, reflected at 0).
CASES = [
    (1, 1, 1, 16, "zero"),
    (3, 1, 2, 16, "half"),
    (3, R, 1, 16, "int"),
    (1, R, 2, 16, "random"),
    (1, 2 * R - 1, 2, 16, "half"),
    (3, 2 * R - 1, 1, 48, "far"),
    (3, TILE - 1, 1, 16, "half"),
    (1, TILE - 1, 2, 16, "random"),           # last frame held from sample 16 on
    (1, TILE - 1, 7, 48, "up"),               # hop 48, exactly enough (E = 7)
    (3, TILE, 6, 48, "up"),                   # the last frame held from sample 240 on
    (1, TILE, 17, 16, "down"),                # exactly enough (E = 17)
    (1, TILE, 1, 48, "int"),
    (1, TILE + 1, 7, 48, "random"),           # a frame interval across the tile boundary, exactly enough (E = 7)
    (3, TILE + 1, 9, 48, "random"),           # two frames past S
    (3, TILE + 1, 2, 16, "int"),
    (1, TILE + 1, 3, 48, "far"),
    (1, S3, 3, 48, "up"),                     # three tiles, the last frame held over 427 samples
    (3, S3, 12, 48, "random"),                # exactly enough (E = 12)
    (1, S3, 34, 16, "down"),                  # hop 16, exactly enough (E = 34)
    (1, S3, 40, 16, "random"),                # six frames past S
    (1, S3, 5, 48, "zero"),
    (3, S3, 1, 16, "half"),
]


def case_id(case):
    return "-".join(map(str, case))


def int_delay(S):
    return min(5, S - 1) if S > 1 else 0


def delays(case):
    """tau (B, K) fp64."""
    B, S, K, hop, kind = case
    k = np.arange(K, dtype=np.float64)
    if kind == "zero":
        row = np.zeros(K)
    elif kind == "int":
        row = np.full(K, float(int_delay(S)))
    elif kind == "half":
        row = np.full(K, int_delay(S) + 0.5)
    elif kind == "far":
        row = np.full(K, S + R + 1.5)
    elif kind == "up":
        row = 3.25 + MAX_SLOPE * hop * k
    elif kind == "down":
        row = 1.75 + MAX_SLOPE * hop * (K - 1 - k)
    else:
        rng = np.random.default_rng([B, S, K, hop, 77])
        steps = rng.uniform(-MAX_SLOPE * hop, MAX_SLOPE * hop, (B, K))
        steps[:, 0] = rng.uniform(0.0, 20.0, B)
        return np.abs(np.cumsum(steps, 1))    # (reflection at 0 keeps every step within the limit)
    return np.tile(row, (B, 1)) + (0.0 if kind in ("zero", "int", "far") else 0.125 * np.arange(B)[:, None])


def inputs(case):
    """(s (B, S) fp32, tau (B, K) fp64, gy (B, S) fp32); fixed seed per case, every seventh number of s zero."""
    B, S, K, hop, kind = case
    rng = np.random.default_rng([B, S, K, hop, sum(map(ord, kind)), 31])
    s = rng.standard_normal((B, S)).astype(np.float32)
    s.reshape(-1)[::7] = 0.0
    gy = rng.standard_normal((B, S)).astype(np.float32)
    tau = delays(case)
    assert (np.abs(np.diff(tau, axis=1)) <= MAX_SLOPE * hop).all() and (tau >= 0).all()
    return s, tau, gy
