"""References, per-element error bounds and inputs for the biquad cascade of diffsound_amd/csrc/biquad.hip (ds_biquad_fwd /
ds_biquad_bwd).  Not a test module.

The kernels join the lanes of a wavefront with a scan over powers of the companion matrix.  The references here do NOT:
they are the plain recurrences, sample by sample, in fp64 numpy (vectorised over the rows only),

  w[n]   = u[n] - a1 w[n-1] - a2 w[n-2],   v[n] = b0 w[n] + b1 w[n-1] + b2 w[n-2],   section s + 1 reads the v of section s
  r[n]   = sum_k b_k g[n+k],   lam[n] = r[n] - a1 lam[n+1] - a2 lam[n+2]          (g the gradient at the section's output)
  gb_k   = sum_n g[n] w[n-k],  ga_k = - sum_n lam[n] w[n-k],                       gx = lam of section 0.

Bounds, derived and counted.  U32 = 2^-24, U64 = 2^-53 (half an ulp).  RUN = 16 samples a lane, 64 lanes a tile.
Notation for one section: h[k] its all-pole impulse response (from the recurrence on a unit pulse, so from the
coefficients alone); A = [[-a1, -a2], [1, 0]], A^k = [[h[k], -a2 h[k-1]], [h[k-1], -a2 h[k-2]]]; kap[k] = the largest |entry| of
A^k: an error of size e in EITHER component of a state at sample j reaches w[n] no larger than kap[n-j] e.
Majorants: M[n] = sum_j kap[n-j] |u[j]| >= |w[n]|, and also >= every partial form of it that the kernel holds (a lane's run
from the zero state, a scan's partial sum, a carried state: all are sums of h-weighted inputs over a SUBSET of j);
m[j] = |u[j]| + |a1| M[j-1] + |a2| M[j-2]: the magnitude sum of the terms formed at sample j.
A rounding made on a quantity that belongs to sample j is at most U64 m[j] and reaches sample n through the all-pole
response: every count below multiplies U64 sum_j kap[n-j] m[j].   Counted, per sample or per state it belongs to:
  *  4  the recurrence of the second run (2 products, 2 sums; fewer where the compiler fuses)
  *  4  the same in the run from the zero state, whose end state enters the scan
  * 24  the scan: 6 steps, each a 2 x 2 product (2 products and a sum a component: 3) and the sum onto the lane's value (1)
  * 30  the squarings: log2(64 RUN) = 10, each entry 2 products and a sum (3); a power's error acts on the state it multiplies
  * 18  the lane's own power A^(RUN q): up to 6 products of the squares (3 each)
  *  4  the entering state: A^(RUN q) times the carried state (3) and the sum (1)
  *  4  the carry: A^(64 RUN) times the carried state (3) and the sum (1), once a tile; the error of a carried state is a
        source at the tile's first sample and runs on through the same response, so the convolution counts every tile
  *  4  the reference's own recurrence
  -> CW = 92:  ew[n] = sum_j kap[n-j] (CW U64 m[j] + eu[j]),   eu the error bound of the section's input (0 for x).
The three taps: 3 products and 2 sums in the kernel, as many in the reference, each at most the magnitude sum
  -> CV = 10:  ev[n] = sum_k |b_k| ew[n-k] + CV U64 sum_k |b_k| M[n-k],   and ev is the next section's eu.
First order in U64 throughout (second order is below 1e-28 of the terms).  The stored fp32: 2 U32 |ref| (one rounding, on a
value itself in error) + 2^-150 for the fp32 subnormals:   bound(y) = 2 U32 |y| + ev + 2^-150.
Backward.  The kernel forms lam as the section run DOWN in time (mu = all-pole of g, lam = the three taps of mu: both are
shift-invariant from rest, so they commute with the order above).  Its bound is the forward's on reversed sequences, eu the
bound of g (0 for gy, else the el of the section after); the reference's own order adds 5 U64 r^[j] + 4 U64 m_r[j] as a
source, r^ = sum_k |b_k| |g[n+k]|:   el as ev, plus sum_j kap[j-n] (5 U64 r^[j] + 4 U64 m_r[j]).   bound(gx) = 2 U32 |gx| + el + 2^-150.
gsos (fp64): a term g[n] w[n-k] carries eg[n] M[n-k] + |g[n]| ew[n-k] (ew: the recomputed w has the forward's bound, it is
the same code), and the sum (N / 64 + 6) U64 for the lane's additions over the tiles and the butterfly, + 2 for the product
and the first sum, + 13 for the reference's product and pairwise sum (N <= 2^12), of sum_n |g[n]| M[n-k]:
  bound(gb_k) = sum_n (eg[n] M[n-k] + |g[n]| ew[n-k]) + (N / 64 + 21) U64 sum_n |g[n]| M[n-k],   ga_k the same with lam, el for g, eg.
"""
import numpy as np

U32, U64 = 2.0 ** -24, 2.0 ** -53
TINY32 = 2.0 ** -150
RUN, TILE = 16, 1024     # DS_OSC_SCAN_RUN, 64 RUN
CW, CV = 92, 10
MAX_SECTIONS = 16


# --------------------------------------------------------------------------------------------------- recurrences
def allpole(u, a1, a2):
    """w[n] = u[n] - a1 w[n-1] - a2 w[n-2] from rest; u (B, N), a1, a2 (B,)."""
    u = np.asarray(u, dtype=np.float64)
    w = np.zeros_like(u)
    w1 = np.zeros(u.shape[0])
    w2 = np.zeros(u.shape[0])
    for n in range(u.shape[1]):
        wn = u[:, n] - a1 * w1 - a2 * w2
        w[:, n] = wn
        w2, w1 = w1, wn
    return w


def shift(w, k):
    """w[n-k], 0 in front."""
    if k == 0:
        return w
    out = np.zeros_like(w)
    out[:, k:] = w[:, :-k]
    return out


def taps(w, b):
    """b0 w[n] + b1 w[n-1] + b2 w[n-2]; b (B, 3)."""
    return b[:, 0:1] * w + b[:, 1:2] * shift(w, 1) + b[:, 2:3] * shift(w, 2)


def per_row(sos, B):
    """(B, S, 5) from (S, 5) or (B, S, 5)."""
    sos = np.asarray(sos, dtype=np.float64)
    return np.broadcast_to(sos, (B,) + sos.shape[-2:]) if sos.ndim == 2 else sos


def cascade(x, sos):
    """y (B, N) fp64 alone: what the CPU tests compare with scipy."""
    u = np.asarray(x, dtype=np.float64)
    c = per_row(sos, u.shape[0])
    for s in range(c.shape[1]):
        u = taps(allpole(u, c[:, s, 3], c[:, s, 4]), c[:, s, :3])
    return u


def stable(sos):
    """Per row of (..., 5): the poles strictly inside the unit circle."""
    sos = np.asarray(sos, dtype=np.float64)
    return (np.abs(sos[..., 4]) < 1) & (np.abs(sos[..., 3]) < 1 + sos[..., 4])


# -------------------------------------------------------------------------------------------------------- bounds
def kappa(a1, a2, N):
    """kap[k], k < N + 2: the largest |entry| of A^k, per row."""
    B = a1.shape[0]
    d = np.zeros((B, N + 2))
    d[:, 0] = 1.0
    h = np.abs(allpole(d, a1, a2))
    a = np.abs(a2)[:, None]
    return np.maximum.reduce([h, shift(h, 1), a * shift(h, 1), a * shift(h, 2)])


def conv(k, v):
    """sum_j k[n-j] v[j] per row, n < len(v)."""
    N = v.shape[1]
    return np.stack([np.convolve(k[i], v[i])[:N] for i in range(v.shape[0])])


def section_bound(u, eu, c, kap):
    """(M, ew, ev) of one section: u its (reference) input, eu the input's error bound, c (B, 5)."""
    au = np.abs(u)
    M = conv(kap, au)
    m = au + np.abs(c[:, 3:4]) * shift(M, 1) + np.abs(c[:, 4:5]) * shift(M, 2)
    ew = conv(kap, CW * U64 * m + eu)
    ab = np.abs(c[:, :3])
    ev = sum(ab[:, k:k + 1] * shift(ew, k) for k in range(3)) + CV * U64 * sum(ab[:, k:k + 1] * shift(M, k) for k in range(3))
    return M, ew, ev


def forward(x, sos):
    """dict: y (B, N), y_bound; and per section w, M (the majorant of |w|), ew - what the backward's bounds need."""
    u = np.asarray(x, dtype=np.float64)
    B, N = u.shape
    c = per_row(sos, B)
    eu = np.zeros_like(u)
    out = dict(w=[], M=[], ew=[], kap=[])
    for s in range(c.shape[1]):
        kap = kappa(c[:, s, 3], c[:, s, 4], N)
        w = allpole(u, c[:, s, 3], c[:, s, 4])
        M, ew, ev = section_bound(u, eu, c[:, s], kap)
        out["w"].append(w), out["M"].append(M), out["ew"].append(ew), out["kap"].append(kap)
        u, eu = taps(w, c[:, s, :3]), ev
    out["y"] = u
    out["y_bound"] = 2 * U32 * np.abs(u) + eu + TINY32
    return out


def backward(gy, x, sos, f=None):
    """dict gx (B, N), gx_bound, gsos (B, S, 5), gsos_bound."""
    f = forward(x, sos) if f is None else f
    g = np.asarray(gy, dtype=np.float64)
    B, N = g.shape
    c = per_row(sos, B)
    S = c.shape[1]
    rev = lambda v: v[:, ::-1]
    eg = np.zeros_like(g)
    gsos, gbound = np.zeros((B, S, 5)), np.zeros((B, S, 5))
    csum = (N / 64.0 + 21) * U64
    for s in range(S - 1, -1, -1):
        cs, w, M, ew, kap = c[:, s], f["w"][s], f["M"][s], f["ew"][s], f["kap"][s]
        # the reference, in the order of the definition: the taps up in time, then the all-pole part down
        r = rev(taps(rev(g), cs[:, :3]))
        lam = rev(allpole(rev(r), cs[:, 3], cs[:, 4]))
        # the kernel's order bounds its error (the forward's bound on reversed sequences) ...
        _, _, el = section_bound(rev(g), rev(eg), cs, kap)
        # ... and the reference's own roundings are a source of their own
        rh = rev(sum(np.abs(cs[:, k:k + 1]) * shift(np.abs(rev(g)), k) for k in range(3)))
        Mr = conv(kap, rev(rh))
        mr = rev(rh) + np.abs(cs[:, 3:4]) * shift(Mr, 1) + np.abs(cs[:, 4:5]) * shift(Mr, 2)
        el = rev(el + conv(kap, 5 * U64 * rev(rh) + 4 * U64 * mr))
        ag, al = np.abs(g), np.abs(lam)
        for k in range(3):
            wk, Mk, ewk = shift(w, k), shift(M, k), shift(ew, k)
            gsos[:, s, k] = (g * wk).sum(1)
            gbound[:, s, k] = (eg * Mk + ag * ewk).sum(1) + csum * (ag * Mk).sum(1)
            if k:
                gsos[:, s, 2 + k] = -(lam * wk).sum(1)
                gbound[:, s, 2 + k] = (el * Mk + al * ewk).sum(1) + csum * (al * Mk).sum(1)
        g, eg = lam, el
    return dict(gx=g, gx_bound=2 * U32 * np.abs(g) + eg + TINY32, gsos=gsos, gsos_bound=gbound)


# ---------------------------------------------------------------------------------------------- inputs and shapes
def _rbj_highpass(sr, f0, Q):
    w0 = 2 * np.pi * f0 / sr
    c, al = np.cos(w0), np.sin(w0) / (2 * Q)
    return np.array([(1 + c) / 2, -(1 + c), (1 + c) / 2, -2 * c, 1 - al]) / (1 + al)


_TH = 2 * np.pi * 2000.0 / 44100.0
SETS = {
    "complex": np.array([0.02, 0.01, -0.015, -2 * 0.999 * np.cos(_TH), 0.999 ** 2]),  # radius 0.999, 2 kHz at 44.1 kHz
    "highpass": _rbj_highpass(44100.0, 100.0, 0.707),                                   # the clips' 100 Hz high-pass
    "real": np.array([1.0, -0.3, 0.2, -(0.9 - 0.5), 0.9 * -0.5]),                       # poles 0.9 and -0.5
    "repeated": np.array([0.5, 0.2, 0.1, -1.6, 0.64]),                                  # a double pole at 0.8
    "fir": np.array([0.7, -0.4, 0.3, 0.0, 0.0]),                                        # a1 = a2 = 0
    "first": np.array([0.3, 0.3, 0.0, -0.95, 0.0]),                                     # first order: a2 = b2 = 0
}
NAMES = tuple(SETS)
NS = (1, 2, 15, 16, 17, 1023, 1024, 1025, 2051)   # around a lane's run (16) and a tile (1024); 2051: three tiles
CASES = [(B, N, S, per_clip, name) for N in NS for S in (1, 2, 3) for B in (1, 3) for per_clip in (0, 1) for name in NAMES]


def case_id(case):
    return "-".join(map(str, case))


def coefficients(S, name, B=None):
    """(S, 5), or (B, S, 5) with B given.  Section 0 is the named set, the following ones the sets after it in NAMES (all
    different, so an order of sections is a property of the result); row b starts b sets further on and scales the
    numerator by 1 + b / 8."""
    i0 = NAMES.index(name)
    one = lambda off, gain: np.stack([SETS[NAMES[(i0 + off + s) % len(NAMES)]] * np.array([gain] * 3 + [1.0, 1.0]) for s in range(S)])
    return one(0, 1.0) if B is None else np.stack([one(b, 1.0 + b / 8.0) for b in range(B)])


def sixteen(B):
    """(B, 16, 5): DS_BIQUAD_MAX_SECTIONS sections of gain near 1 (the four sets without a narrow resonance, their numerators
    scaled by the inverse of their gain at DC), row b starting b sets further on: a cascade whose bound stays 1e-7 of its
    values - sixteen sections of the resonant sets condition each other to a bound of no use."""
    names, gain = ("real", "fir", "first", "repeated"), (1 / 3.0, 1.0, 1 / 6.0, 1 / 10.0)
    one = lambda off: np.stack([SETS[names[(s + off) % 4]] * np.array([gain[(s + off) % 4]] * 3 + [1.0, 1.0]) for s in range(16)])
    return np.stack([one(b) for b in range(B)])


def inputs(case):
    """(x (B, N) fp32, sos (S, 5) or (B, S, 5) fp64, gy (B, N) fp32); fixed seed per case, every seventh number of x zero."""
    B, N, S, per_clip, name = case
    rng = np.random.default_rng([B, N, S, per_clip, NAMES.index(name), 53])
    x = rng.standard_normal((B, N)).astype(np.float32)
    x.reshape(-1)[::7] = 0.0
    gy = rng.standard_normal((B, N)).astype(np.float32)
    return x, coefficients(S, name, B if per_clip else None), gy
