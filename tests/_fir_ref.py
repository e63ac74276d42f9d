"""References, per-element error bounds and inputs for the long FIR of diffsound_amd/csrc/fir.hip (ds_fir_fwd / ds_fir_bwd).
Not a test module.

The kernels tile the three sums, stage them through LDS and read the row backwards for y.  The references here do NOT: they
are the sums as the header writes them, plain fp64 numpy loops over the lag (vectorised over the rows and the samples),

  y[b,t]  = sum_{j=0..min(t, L-1)}      h[b mod H, j] x[b, t-j]
  gx[b,s] = sum_{j=0..min(L-1, N-1-s)}  h[b mod H, j] gy[b, s+j]
  gh[r,j] = sum_{b = r, r+H, ...} sum_{s=0..N-1-j} x[b,s] gy[b, s+j]        (t = s + j; exactly 0 for j >= N)

and with every element they return P, the sum of |a_i b_i| over the element's terms, and n, their number (for gh: per row).

Bounds, derived.  U32 = 2^-24, U64 = 2^-53 (half an ulp).  One sum of n products in fp64, in ANY order of the additions and
with the products fused or not: every partial sum is at most P in magnitude, so each of the n - 1 additions errs by at most
U64 P and the n roundings of the products (none where they are fused) by U64 P in all: n U64 P to first order, whatever tiles,
chunks or trees the kernel chooses.  The reference's own sum is COMPENSATED (Knuth's two-sum beside the running sum, added
at the end), so that it adds no n-fold term of its own: its products' roundings are U64 P in all, its last addition
U64 |ref| <= U64 P, the rest is second order (n U64^2 P, below 1e-11 of the bound).  Together:
  y, gx:  |got - ref| <= U32 |ref| + (n + 2) U64 P + 2^-149     (the one fp32 rounding on the store; the smallest fp32 subnormal
          for results below the normal range),
  gh:     |got - ref| <= (n + B/H + 2) U64 P                    (n = N - j terms a row; the B / H row sums, each at most its
          row's P, are added in B / H - 1 more additions here and there), P summed over the rows; 0 - exact - for j >= N.
A unit tap makes every term but one an exact zero and that one an exact product: P = |ref|, and the test asks for the bits.
"""
import functools
import math
from concurrent.futures import ThreadPoolExecutor

import numpy as np

U32, U64 = 2.0 ** -24, 2.0 ** -53
TINY32 = 2.0 ** -149
R, TILE, TAPS, GH_CHUNK = 8, 512, 256, 2048   # fir.hip's constants (tests/test_fir_cabi_cpu.py holds them against the source)
MAX_TAPS, MAX_ROWS = 65536, 65535


class _Sum:
    """A compensated running sum of arrays: s the fp64 sum, c the two-sum errors, p the sum of magnitudes."""

    def __init__(self, shape):
        self.s, self.c, self.p = np.zeros(shape), np.zeros(shape), np.zeros(shape)

    def add(self, sl, term):
        s = self.s[sl]
        t = s + term
        bp = t - s
        self.c[sl] += (s - (t - bp)) + (term - bp)
        self.s[sl] = t
        self.p[sl] += np.abs(term)

    def value(self):
        return self.s + self.c


def _taps(h, B, lags):
    h = np.asarray(h, dtype=np.float64)
    H, L = h.shape
    rows = np.arange(B) % H
    return h, H, L, rows, (range(L) if lags is None else lags)


def forward(x, h, lags=None):
    """dict y, P, n, bound, all (B, N).  ``lags``: only these taps are non-zero (the sum skips the others' exact zeros; n
    counts them all the same, as the kernel adds them)."""
    x = np.asarray(x, dtype=np.float64)
    B, N = x.shape
    h, H, L, rows, js = _taps(h, B, lags)
    acc = _Sum((B, N))
    for j in js:
        if j < N:
            acc.add((slice(None), slice(j, N)), h[rows, j:j + 1] * x[:, :N - j])
    y = acc.value()
    n = np.minimum(np.arange(N), L - 1) + 1.0
    return dict(y=y, P=acc.p, n=n, bound=U32 * np.abs(y) + (n + 2) * U64 * acc.p + TINY32)


def input_gradient(gy, h, lags=None):
    """dict gx, gx_P, gx_bound (B, N); ``lags`` as in forward."""
    g = np.asarray(gy, dtype=np.float64)
    B, N = g.shape
    h, H, L, rows, js = _taps(h, B, lags)
    acc = _Sum((B, N))
    for j in js:
        if j < N:
            acc.add((slice(None), slice(0, N - j)), h[rows, j:j + 1] * g[:, j:])
    gx = acc.value()
    n = np.minimum(L - 1, N - 1 - np.arange(N)) + 1.0
    return dict(gx=gx, gx_P=acc.p, gx_bound=U32 * np.abs(gx) + (n + 2) * U64 * acc.p + TINY32)


def tap_gradient(gy, x, H, L, gh_lags=None):
    """dict gh, gh_P, gh_bound (H, L); ``gh_lags``: gh at these lags alone, (H, len(gh_lags)), each a plain dot product (math.fsum
    of the products: their exact sum)."""
    g, x = np.asarray(gy, dtype=np.float64), np.asarray(x, dtype=np.float64)
    B, N = g.shape
    if gh_lags is None:
        a = _Sum((B, L))
        for s in range(N):
            m = min(L, N - s)
            a.add((slice(None), slice(0, m)), x[:, s:s + 1] * g[:, s:s + m])
        per_row, P, nj = a.value(), a.p, np.maximum(N - np.arange(L), 0.0)
    else:
        per_row, P = np.zeros((B, len(gh_lags))), np.zeros((B, len(gh_lags)))
        for k, j in enumerate(gh_lags):
            if j < N:
                term = x[:, :N - j] * g[:, j:]
                per_row[:, k], P[:, k] = [math.fsum(row) for row in term], np.abs(term).sum(1)
        nj = np.maximum(N - np.asarray(gh_lags), 0.0)
    P = P.reshape(B // H, H, -1).sum(0)
    return dict(gh=per_row.reshape(B // H, H, -1).sum(0), gh_P=P, gh_bound=(nj + B // H + 2) * U64 * P)


def backward(gy, x, h, lags=None, gh_lags=None):
    """Both gradients in one dict."""
    return dict(input_gradient(gy, h, lags), **tap_gradient(gy, x, *np.shape(h), gh_lags))


# ---------------------------------------------------------------------------------------------- inputs and shapes
# (B, H, N, L)
CASES = [(2, 1, 1, 5), (2, 2, 33, 1), (1, 1, 64, 64), (2, 1, 37, 100), (3, 1, 70, 9), (3, 3, 70, 9), (6, 3, 70, 9)]
CASES += [(2, 2, N, 40) for N in (TILE - 1, TILE, TILE + 1, 2 * TILE + 1)]              # the output tile
CASES += [(2, 1, 600, L) for L in (TAPS - 1, TAPS, TAPS + 1, 2 * TAPS + 1)]             # the tap tile (a staged pass)
CASES += [(2, 2, N, 300) for N in (GH_CHUNK - 1, GH_CHUNK, GH_CHUNK + 1)]               # the gh chunk
CASES += [(4, 2, 4097, 4096)]                                                           # dense: 3 chunks, 8 lag tiles
SMALLEST = CASES[:2]


def case_id(case):
    return "-".join(map(str, case))


def spread(rng, shape, lo, hi):
    """Gaussian numbers (both signs: cancellation) times 10^u, u uniform in [lo, hi): magnitudes over several decades."""
    return rng.standard_normal(shape) * 10.0 ** rng.uniform(lo, hi, shape)


def inputs(case):
    """(x (B, N) fp32, h (H, L) fp64, gy (B, N) fp32); fixed seed per case, every seventh number of x zero."""
    B, H, N, L = case
    rng = np.random.default_rng([B, H, N, L, 61])
    x = spread(rng, (B, N), -3, 1).astype(np.float32)
    x.reshape(-1)[::7] = 0.0
    h = spread(rng, (H, L), -3, 0)
    gy = spread(rng, (B, N), -3, 1).astype(np.float32)
    return x, h, gy


@functools.lru_cache(maxsize=None)
def reference(case):
    """(inputs, forward dict, backward dict) of a case, computed once and shared; callers leave it unchanged."""
    x, h, gy = inputs(case)
    with ThreadPoolExecutor(3) as pool:   # the three sums side by side (numpy releases the interpreter lock)
        f, bx, bh = pool.submit(forward, x, h), pool.submit(input_gradient, gy, h), pool.submit(tap_gradient, gy, x, *h.shape)
        return (x, h, gy), f.result(), dict(bx.result(), **bh.result())


def shifted(x, k):
    """x[b, t-k], zeros in front: what a unit tap at lag k makes of x (and, on reversed rows, of gy)."""
    out = np.zeros_like(x)
    if k < x.shape[1]:
        out[:, k:] = x[:, :x.shape[1] - k]
    return out


def advanced(g, k):
    """g[b, s+k], zeros at the end: gx of a unit tap at lag k."""
    out = np.zeros_like(g)
    if k < g.shape[1]:
        out[:, :g.shape[1] - k] = g[:, k:]
    return out


# the long-addressing case: 32 non-zero taps of 65536 at seeded lags with 0 and L - 1 among them
LONG = (2, 2, 70001, 65536)


@functools.lru_cache(maxsize=1)
def long_case():
    """(x, h, gy, lags, zero_lags, forward dict, backward dict with gh at lags + zero_lags)."""
    B, H, N, L = LONG
    rng = np.random.default_rng(67)
    lags = np.concatenate([[0, L - 1], rng.choice(np.arange(1, L - 1), 62, replace=False)])
    lags, zero_lags = np.sort(lags[:32]), np.sort(lags[32:])
    h = np.zeros((H, L))
    h[:, lags] = spread(rng, (H, 32), -2, 0)
    x = spread(rng, (B, N), -3, 1).astype(np.float32)
    gy = spread(rng, (B, N), -3, 1).astype(np.float32)
    both = [int(j) for j in lags] + [int(j) for j in zero_lags]
    return x, h, gy, lags, zero_lags, forward(x, h, [int(j) for j in lags]), backward(gy, x, h, [int(j) for j in lags], both)
