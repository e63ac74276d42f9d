"""Reference, restatement and error bounds of csrc/multipole.hip: the multipole series of the modes' exterior fields.

  out[p, j]  = sum_{l <= L} sum_{|n| <= l} c[l^2 + l + n, j] h_l(k_j r_p) Y_{l,n}(u_p),   d = x_p - x0, r = |d|, u = d / r
  gpts[p]    = d/dx_p Re sum_j conj(gout[p, j]) out[p, j]
  gcoef[e,j] = sum_p gout[p, j] conj(h_l(k_j r_p)) Y_e(u_p)

``harmonics`` is the kernel's Cartesian recurrence for the real solid harmonics and their gradient at a unit vector, in any
dtype.  ``restate`` runs the whole unit in the kernel's operation order (fp64, or with ``hdtype=np.float32`` for the Hankel
recurrence: the negative control).  The TRUTH is the same formulas with h_l from mpmath at 50 digits (h_0 = -i e^{iz} / z and
the upward recurrence in mpmath arithmetic, z = k r from the exact product of the fp64 k and the longdouble r) and with the
harmonics and every sum in np.longdouble; tests/test_multipole_ref_cpu.py vouches for it against scipy's spherical_jn / yn /
sph_harm_y, the closed-form monopole and central differences.

Bound.  An output passes when it deviates from the truth by at most  K 2^-53 MAG,  MAG the sum of the magnitudes of its terms
     out:   sum_{l,n} |c| |h_l| A_{l,n} ;   gcoef: sum_p |gout| |h_l| A_{l,n} ;
     gpts:  sum_j |gout_j| sum_{l,n} |c| (k |u_x| |h_(l+1)| A_{l,n} + |h_l| / r A'_{l,n;x})
and K counted from the operations on the longest path to the output, each rounding as one 2^-53:
     point        d = x - x0, r2 (3 products, 2 sums), sqrt, 1 / r, u = d / r                                    6
     harmonic     (x + i y)^m: 3 per step; D_m: 3 per step (quotient, sqrt, product); Q_l^m: 13 per level (a and b: quotient
                  and sqrt each, b r2, two products, a difference, the product with a; one more sum in the gradient's
                  recurrence), m + (l - m) <= L steps and levels; the closing products and sums 4                13 L + 4
     Hankel       z = k r 1, the rounding of z and of r's 6 move the phase of e^{iz} by z 2^-53 each               7 z
                  sincos 2 (the device's are within 2 ulp), 1 / z, h_0 2, h_1 3, per level 4 (the factor, its product,
                  the difference, and the growth of what the earlier levels left, which follows |h_l| on both sides
                  of l = z as the computed solution is the dominant one), L + 1 levels for the gradient       8 + 4 (L + 1)
     sums         2 l + 1 terms of a degree, L + 1 degrees, the complex products 4                               3 L + 6
     gpts         the product with conj(gout) 3, k E, inv F, the difference 3, the columns ceil(m / 64) and the butterfly 6
     gcoef        the product gout conj(h_l) 3, Y 1, the points of a slab ceil(P / G), the G slabs
  A_{l,n} = sqrt((2 l + 1) / (4 pi)) >= |Y_{l,n}| and A'_{l,n;x} = (2 l + 1) sqrt(l / (4 pi)) >= |d R_{l,n} / dx| on the unit sphere
  stand for |Y| and |grad R|: the norms of ALL harmonics of the degree at a point (sum_n Y_{l,n}^2 = (2 l + 1) / (4 pi), sum_n
  |grad R_{l,n}|^2 = l (2 l + 1)^2 / (4 pi)).  Near a nodal line of Y_{l,n} the recurrence - and any evaluation from fp64
  Cartesian coordinates - keeps an error of the size of the degree's other harmonics, not of that one harmonic, so |Y_{l,n}|
  itself would ask for more than fp64 arithmetic gives (a gcoef element is a single harmonic at P = 1).  At l = 0 and on the z
  axis A = |Y| exactly.
"""
import math

import numpy as np

U64 = 2.0 ** -53
MAX_ORDER = 32           # DS_MULTIPOLE_MAX_ORDER
GCOEF_BLOCKS = 128       # DS_MULTIPOLE_GCOEF_BLOCKS
LD = np.longdouble


def nterms(L):
    return (L + 1) * (L + 1)


def degrees(L):
    """l of every index e = l^2 + l + n."""
    return np.concatenate([np.full(2 * l + 1, l) for l in range(L + 1)])


# ------------------------------------------------------------------------------------------------- harmonics
def harmonics(u, L, dtype=np.float64):
    """(Y (P, N), dY (P, N, 3)) at the vectors u (P, 3): R_{l,n}(u) and its Cartesian gradient by the kernel's recurrences in
    ``dtype``."""
    u = np.asarray(u, dtype=dtype)
    x, y, z = u[:, 0], u[:, 1], u[:, 2]
    P = u.shape[0]
    Y = np.zeros((P, nterms(L)), dtype=dtype)
    dY = np.zeros((P, nterms(L), 3), dtype=dtype)
    r2 = x * x + y * y + z * z
    two = dtype(2.0)
    c, s = np.ones(P, dtype=dtype), np.zeros(P, dtype=dtype)
    cp, sp = np.zeros(P, dtype=dtype), np.zeros(P, dtype=dtype)
    D = np.sqrt(LD(1) / (4 * _pi_ld())) if dtype is LD else dtype(0.28209479177387814)  # sqrt(1 / (4 pi))
    for m in range(L + 1):
        if m > 0:
            cp, sp = c, s
            c, s = cp * x - sp * y, cp * y + sp * x
            D = D * np.sqrt(dtype(2 * m + 1) / dtype(2 * m))
        Dm = D * (np.sqrt(dtype(2.0)) if dtype is LD else dtype(1.4142135623730951)) if m > 0 else D
        fm = dtype(m)
        zero = np.zeros(P, dtype=dtype)
        Q1, Q2, Qz1, Qz2, Qr1, Qr2 = zero, zero, zero, zero, zero, zero
        for l in range(m, L + 1):
            if l == m:
                Q, Qz, Qr = np.full(P, Dm, dtype=dtype), zero, zero
            else:
                a = np.sqrt(dtype(4 * l * l - 1) / dtype(l * l - m * m))
                b = np.sqrt(dtype((l - 1) * (l - 1) - m * m) / dtype(4 * (l - 1) * (l - 1) - 1))
                br2 = b * r2
                Q = a * (z * Q1 - br2 * Q2)
                Qz = a * ((Q1 + z * Qz1) - br2 * Qz2)
                Qr = a * (z * Qr1 - b * (Q2 + r2 * Qr2))
            e = l * l + l
            t, qx, qy, mq = Qz + (two * z) * Qr, (two * x) * Qr, (two * y) * Qr, fm * Q
            Y[:, e + m] = Q * c
            dY[:, e + m, 0] = qx * c + mq * cp
            dY[:, e + m, 1] = qy * c - mq * sp
            dY[:, e + m, 2] = t * c
            if m > 0:
                Y[:, e - m] = Q * s
                dY[:, e - m, 0] = qx * s + mq * sp
                dY[:, e - m, 1] = qy * s + mq * cp
                dY[:, e - m, 2] = t * s
            Q2, Q1, Qz2, Qz1, Qr2, Qr1 = Q1, Q, Qz1, Qz, Qr1, Qr
    return Y, dY


def _pi_ld():
    import mpmath

    with mpmath.workdps(30):
        s = mpmath.nstr(mpmath.pi, 25)
    return LD(s)


def geometry(pts, center, dtype=np.float64):
    """(u (P, 3), r (P,), inv (P,)) as the kernel forms them."""
    d = np.asarray(pts, dtype=dtype) - np.asarray(center, dtype=dtype)
    r = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
    inv = dtype(1.0) / r
    return d * inv[:, None], r, inv


# ------------------------------------------------------------------------------------------------- Hankel functions
def hankel_restate(k, r, L, dtype=np.float64):
    """h_l(k_j r_p), l = 0 .. L + 1, as (re, im) arrays (L + 2, P, m) by the kernel's recurrence in ``dtype``."""
    z = (np.asarray(k, dtype=np.float64)[None, :] * np.asarray(r, dtype=np.float64)[:, None]).astype(dtype)
    sn, cs = np.sin(z), np.cos(z)
    iz = dtype(1.0) / z
    hr, hi = [sn * iz], [dtype(0.0) - cs * iz]
    hr.append(hr[0] * iz + hi[0])
    hi.append(hi[0] * iz - hr[0])
    for l in range(L):
        f = dtype(2 * l + 3) * iz
        hr.append(f * hr[l + 1] - hr[l])
        hi.append(f * hi[l + 1] - hi[l])
    return np.stack(hr).astype(dtype), np.stack(hi).astype(dtype)


def hankel_truth(k, r_ld, L, dps=50):
    """The same table from mpmath at ``dps`` digits, rounded to longdouble: (re, im) (L + 2, P, m).  r_ld: longdouble radii."""
    import mpmath

    P, m = len(r_ld), len(k)
    hr = np.zeros((L + 2, P, m), dtype=LD)
    hi = np.zeros((L + 2, P, m), dtype=LD)

    def to_ld(v):  # the two leading fp64 pieces of v: 106 bits, rounded once to longdouble's 64
        hi_ = float(v)
        return LD(hi_) + LD(float(v - hi_))

    with mpmath.workdps(dps):
        for p in range(P):
            hi_, lo_ = np.float64(r_ld[p]), None
            lo_ = np.float64(r_ld[p] - LD(hi_))
            rp = mpmath.mpf(float(hi_)) + mpmath.mpf(float(lo_))
            for j in range(m):
                z = mpmath.mpf(float(k[j])) * rp
                iz = 1 / z
                h0 = mpmath.mpc(0, -1) * mpmath.expj(z) * iz
                h1 = h0 * mpmath.mpc(iz, -1)
                hs = [h0, h1]
                for l in range(L):
                    hs.append((2 * l + 3) * iz * hs[l + 1] - hs[l])
                for l, h in enumerate(hs):
                    hr[l, p, j], hi[l, p, j] = to_ld(h.real), to_ld(h.imag)
    return hr, hi


# ------------------------------------------------------------------------------------------------- the three outputs
def _cplx(a):
    a = np.asarray(a)
    return (a.real, a.imag) if np.iscomplexobj(a) else (a[..., 0], a[..., 1])


def _per_degree(L):
    return [(l, slice(l * l, l * l + 2 * l + 1)) for l in range(L + 1)]


def evaluate(Y, dY, u, inv, k, hr, hi, coef, gout=None, dtype=LD):
    """out (P, m) as parts (re, im), and with gout also gpts (P, 3) and gcoef (N, m) as parts, from given harmonics and Hankel
    tables; products and sums in ``dtype``, degree by degree in numpy's own order (the truth; not the kernel's order)."""
    L = int(round(math.sqrt(Y.shape[1]))) - 1
    P, m = Y.shape[0], hr.shape[2]
    cr, ci = (np.asarray(t, dtype=dtype) for t in _cplx(coef))  # (N, m)
    zeros = lambda *s: np.zeros(s, dtype=dtype)  # noqa: E731
    out_r, out_i = zeros(P, m), zeros(P, m)
    if gout is not None:
        gr, gi = (np.asarray(t, dtype=dtype) for t in _cplx(gout))  # (P, m)
        gc_r, gc_i = zeros(Y.shape[1], m), zeros(Y.shape[1], m)
        E, F = zeros(P, m), zeros(P, m, 3)
    for l, es in _per_degree(L):
        sr, si = Y[:, es] @ cr[es], Y[:, es] @ ci[es]
        out_r += hr[l] * sr - hi[l] * si
        out_i += hr[l] * si + hi[l] * sr
        if gout is None:
            continue
        gc_r[es] = Y[:, es].T @ (gr * hr[l] + gi * hi[l])
        gc_i[es] = Y[:, es].T @ (gi * hr[l] - gr * hi[l])
        wr, wi = gr * hr[l] + gi * hi[l], gr * hi[l] - gi * hr[l]  # conj(g) h_l
        w1r, w1i = gr * hr[l + 1] + gi * hi[l + 1], gr * hi[l + 1] - gi * hr[l + 1]
        E += w1r * sr - w1i * si
        for a in range(3):
            F[:, :, a] += wr * (dY[:, es, a] @ cr[es]) - wi * (dY[:, es, a] @ ci[es])
    if gout is None:
        return out_r, out_i
    kk = np.asarray(k, dtype=dtype)
    gp = (inv[:, None, None] * F - u[:, None, :] * (kk[None, :] * E)[..., None]).sum(1)
    return out_r, out_i, gp, gc_r, gc_i


def envelopes(L):
    """(A (N,), A' (N,)) of the docstring, per index e."""
    l = degrees(L).astype(np.float64)
    return np.sqrt((2 * l + 1) / (4 * math.pi)), (2 * l + 1) * np.sqrt(l / (4 * math.pi))


def magnitudes(L, u, inv, k, habs, coef, gout):
    """The sums of the magnitudes of the terms of out (P, m), gpts (P, 3), gcoef (N, m); habs (L + 2, P, m) = |h_l|; fp64."""
    P, m = habs.shape[1], habs.shape[2]
    A, dA = envelopes(L)
    ca = np.hypot(*(np.asarray(t, dtype=np.float64) for t in _cplx(coef)))
    ga = np.hypot(*(np.asarray(t, dtype=np.float64) for t in _cplx(gout)))
    m_out, m_gc, t1, t2 = np.zeros((P, m)), np.zeros((A.shape[0], m)), np.zeros((P, m)), np.zeros((P, m))
    for l, es in _per_degree(L):
        s = (A[es, None] * ca[es]).sum(0)[None, :]
        m_out += habs[l] * s
        m_gc[es] = A[es, None] * (ga * habs[l]).sum(0)[None, :]
        t1 += habs[l + 1] * s
        t2 += habs[l] * (dA[es, None] * ca[es]).sum(0)[None, :]
    kk = np.asarray(k, dtype=np.float64)
    m_gp = (ga[..., None] * (np.abs(u)[:, None, :] * (kk[None, :] * t1)[..., None] + (inv[:, None] * t2)[..., None])).sum(1)
    return m_out, m_gp, m_gc


def K_counts(P, m, L, kr):
    """K of the docstring per output: (K_out (P, m), K_gpts (P,), K_gcoef (m,)); kr (P, m)."""
    base = 6 + (13 * L + 4) + (8 + 4 * (L + 1)) + 7 * kr
    k_out = base + (3 * L + 6)
    k_gp = (base + (3 * L + 6) + 6 + math.ceil(m / 64) + 6).max(1)
    G = min(P, GCOEF_BLOCKS)
    k_gc = (base + 4 + math.ceil(P / G) + G).max(0)
    return k_out, k_gp, k_gc


# ------------------------------------------------------------------------------------------------- restatement
def _butterfly(v):
    """ds::wave_sum of a (64,) array: the xor butterfly, the value every lane ends with (lane 0's here)."""
    v = np.array(v)
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[idx ^ o]
    return v[0]


def restate(pts, center, k, coef, L, gout=None, hdtype=np.float64):
    """The unit in the kernel's operation order, fp64 (``hdtype``: the dtype of the Hankel recurrence).  coef, gout: complex
    (N, m) and (P, m).  Returns out (P, m) complex, and with gout also gpts (P, 3) and gcoef (N, m) complex."""
    f8 = np.float64
    pts, k = np.asarray(pts, dtype=f8), np.asarray(k, dtype=f8)
    P, m = pts.shape[0], k.shape[0]
    u, r, inv = geometry(pts, center)
    Y, dY = harmonics(u, L)
    hr, hi = (t.astype(f8) for t in hankel_restate(k, r, L, hdtype))
    cr, ci = np.ascontiguousarray(coef.real), np.ascontiguousarray(coef.imag)
    out = np.zeros((P, m), dtype=np.complex128)
    pr, pi = np.zeros((P, m)), np.zeros((P, m))
    S = np.zeros((L + 1, 2, P, m))
    T = np.zeros((L + 1, 2, P, m, 3))
    for l in range(L + 1):
        sr, si = np.zeros((P, m)), np.zeros((P, m))
        tr, ti = np.zeros((P, m, 3)), np.zeros((P, m, 3))
        for e in range(l * l, l * l + 2 * l + 1):
            sr = sr + cr[e][None, :] * Y[:, e, None]
            si = si + ci[e][None, :] * Y[:, e, None]
            if gout is not None:
                tr = tr + cr[e][None, :, None] * dY[:, e, None, :]
                ti = ti + ci[e][None, :, None] * dY[:, e, None, :]
        pr = pr + (hr[l] * sr - hi[l] * si)
        pi = pi + (hr[l] * si + hi[l] * sr)
        S[l, 0], S[l, 1], T[l, 0], T[l, 1] = sr, si, tr, ti
    out = pr + 1j * pi
    if gout is None:
        return out
    gr, gi = np.ascontiguousarray(gout.real), np.ascontiguousarray(gout.imag)
    E, F = np.zeros((P, m)), np.zeros((P, m, 3))
    for l in range(L + 1):
        wr, wi = gr * hr[l] + gi * hi[l], gr * hi[l] - gi * hr[l]
        w1r, w1i = gr * hr[l + 1] + gi * hi[l + 1], gr * hi[l + 1] - gi * hr[l + 1]
        E = E + (w1r * S[l, 0] - w1i * S[l, 1])
        F = F + (wr[..., None] * T[l, 0] - wi[..., None] * T[l, 1])
    kE = k[None, :] * E
    per = inv[:, None, None] * F - u[:, None, :] * kE[..., None]  # (P, m, 3)
    gpts = np.zeros((P, 3))
    for p in range(P):
        lanes = np.zeros((64, 3))
        for j in range(m):  # lane j % 64 adds its columns in ascending order
            lanes[j % 64] = lanes[j % 64] + per[p, j]
        gpts[p] = [_butterfly(lanes[:, a]) for a in range(3)]
    deg = degrees(L)
    G = min(P, GCOEF_BLOCKS)
    slabs = np.zeros((G, nterms(L), m), dtype=np.complex128)
    for p in range(P):
        wr, wi = gr[p] * hr[:L + 1, p] + gi[p] * hi[:L + 1, p], gi[p] * hr[:L + 1, p] - gr[p] * hi[:L + 1, p]  # (L + 1, m)
        v = wr[deg] * Y[p][:, None] + 1j * (wi[deg] * Y[p][:, None])
        slabs[p % G] = v if p < G else slabs[p % G] + v
    gcoef = np.zeros((nterms(L), m), dtype=np.complex128)
    for b in range(G):
        gcoef = gcoef + slabs[b]
    return out, gpts, gcoef, slabs


# ------------------------------------------------------------------------------------------------- the shared grid
P_MAX, M_MAX = 130, 70
CENTER = np.array([0.3, -0.2, 0.1])
CASES = [(P, m, L) for P in (1, 63, 130) for m in (1, 5, 64, 70) for L in (0, 1, 2, 7, 32)]


def grid():
    """(pts (130, 3), k (70,)): every case takes the first P points and the first m wave numbers.  The radii run over
    0.1 .. 5 and the wave numbers over 0.5 .. 40 in an order that puts both ends among the first few, so k r spans 0.05 .. 200
    in the small cases too and l < k r and l > k r both occur; points 0 / 1 are on +z / -z, 2 .. 5 in the xy plane (two of them
    on the x and y axes), 6 has z = 0 to one rounding of the subtraction, the rest are generic."""
    rng = np.random.default_rng(2207)
    rad = np.geomspace(0.1, 5.0, P_MAX)
    rad = rad[np.argsort(np.argsort(rng.permutation(P_MAX)))]
    rad[[0, 1, 2, 3]] = [5.0, 0.1, 0.1, 5.0]
    d = rng.standard_normal((P_MAX, 3))
    d[0], d[1] = (0, 0, 1), (0, 0, -1)
    d[2], d[3] = (1, 0, 0), (0, -1, 0)
    d[4, 2] = d[5, 2] = d[6, 2] = 0.0
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    off = d * rad[:, None]
    pts = CENTER + off
    for i in range(6):  # exact zeros of the offset survive the addition of the centre
        for a in range(3):
            if off[i, a] == 0.0:
                pts[i, a] = CENTER[a]
    kk = np.geomspace(0.5, 40.0, M_MAX)
    kk = kk[rng.permutation(M_MAX)]
    kk[[0, 1, 2]] = [40.0, 0.5, 3.0]
    return pts, kk


def coefficients(m, L, seed=11):
    """(N, m) complex with zeros: a whole degree (l = 1 where there is one beyond it), every seventh entry, the real part of
    one column, and - from m = 5 on - all of column 3."""
    rng = np.random.default_rng(seed + 1000 * L + m)
    N = nterms(L)
    c = rng.standard_normal((N, m)) + 1j * rng.standard_normal((N, m))
    c *= 10.0 ** rng.uniform(-2, 2, size=(N, 1))
    if L >= 2:
        c[1:4] = 0
    c.reshape(-1)[::7] = 0
    c[:, 0] = 1j * c[:, 0].imag if L >= 1 else c[:, 0]
    if m >= 5:
        c[:, 3] = 0
    return c


def cotangent(P, m, seed=5):
    rng = np.random.default_rng(seed + 1000 * P + m)
    g = rng.standard_normal((P, m)) + 1j * rng.standard_normal((P, m))
    g.reshape(-1)[::5] = 0
    return g


_TRUTH = {}


def truth_tables():
    """Once per process: the longdouble geometry and harmonics of the grid's points at L = 32 (their leading (L + 1)^2 columns are
    those of a smaller L) and mpmath's Hankel table (34, 130, 70)."""
    if not _TRUTH:
        pts, kk = grid()
        u, r, inv = geometry(pts, CENTER, LD)
        Y, dY = harmonics(u, MAX_ORDER, LD)
        hr, hi = hankel_truth(kk, r, MAX_ORDER)
        _TRUTH.update(pts=pts, k=kk, u=u, r=r, inv=inv, Y=Y, dY=dY, hr=hr, hi=hi,
                      habs=np.hypot(hr, hi).astype(np.float64))
    return _TRUTH


def case_truth(P, m, L):
    """dict of the case's inputs, truth (out, gpts, gcoef as complex128 / float64 roundings plus longdouble parts) and bounds."""
    t = truth_tables()
    N = nterms(L)
    coef, gout = coefficients(m, L), cotangent(P, m)
    sl = (slice(0, L + 2), slice(0, P), slice(0, m))
    Y, dY, u, inv = t["Y"][:P, :N], t["dY"][:P, :N], t["u"][:P], t["inv"][:P]
    o_r, o_i, gp, gc_r, gc_i = evaluate(Y, dY, u, inv, t["k"][:m], t["hr"][sl], t["hi"][sl], coef, gout)
    f8 = np.float64
    m_out, m_gp, m_gc = magnitudes(L, u.astype(f8), inv.astype(f8), t["k"][:m], t["habs"][sl], coef, gout)
    kr = t["k"][None, :m] * t["r"][:P, None].astype(f8)
    k_out, k_gp, k_gc = K_counts(P, m, L, kr)
    return dict(pts=t["pts"][:P], k=t["k"][:m], coef=coef, gout=gout, out=(o_r, o_i), gpts=gp, gcoef=(gc_r, gc_i),
                b_out=k_out * U64 * m_out, b_gpts=k_gp[:, None] * U64 * m_gp, b_gcoef=k_gc[None, :] * U64 * m_gc)


def ratios(case, out=None, gpts=None, gcoef=None):
    """Largest error / bound of whichever outputs are given (complex arrays for out and gcoef); an element whose bound is 0 must
    be exact (ratio 0 if it is, inf if not)."""
    def worst(err, bound):
        err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
        q = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))
        return float(q.max())

    res = {}
    if out is not None:
        res["out"] = worst(np.hypot(LD(out.real) - case["out"][0], LD(out.imag) - case["out"][1]), case["b_out"])
    if gpts is not None:
        res["gpts"] = worst(np.abs(LD(gpts) - case["gpts"]), case["b_gpts"])
    if gcoef is not None:
        res["gcoef"] = worst(np.hypot(LD(gcoef.real) - case["gcoef"][0], LD(gcoef.imag) - case["gcoef"][1]), case["b_gcoef"])
    return res


# ------------------------------------------------------------------------------------------------- the fit's test case
MONO_OFFSET = np.array([0.3, 0.1, -0.2])
MONO_RS, MONO_RTEST = 1.5, 1.6
MONO_CASES = [(L, k) for L in (4, 8, 12) for k in (0.5, 2.0)]


def fibonacci_sphere(n, radius, center=(0.0, 0.0, 0.0)):
    i = np.arange(n) + 0.5
    z = 1.0 - 2.0 * i / n
    ph = i * (math.pi * (3.0 - math.sqrt(5.0)))
    rho = np.sqrt(1.0 - z * z)
    return np.asarray(center) + radius * np.stack([rho * np.cos(ph), rho * np.sin(ph), z], 1)


def monopole(points, k):
    """e^{ikR} / (4 pi R) of a unit source at MONO_OFFSET."""
    R = np.linalg.norm(np.asarray(points) - MONO_OFFSET, axis=1)
    return np.exp(1j * k * R) / (4 * math.pi * R)


def mono_bound(L):
    return 4.0 * (np.linalg.norm(MONO_OFFSET) / MONO_RS) ** (L + 1)


def basis_scipy(points, k, L):
    """(Q, N) complex h_l(k r) Y_{l,n} from scipy alone (spherical_jn / yn, sph_harm_y converted to the real basis)."""
    from scipy.special import sph_harm_y, spherical_jn, spherical_yn

    p = np.asarray(points, dtype=np.float64)
    r = np.linalg.norm(p, axis=1)
    th, ph = np.arctan2(np.hypot(p[:, 0], p[:, 1]), p[:, 2]), np.arctan2(p[:, 1], p[:, 0])
    B = np.zeros((len(p), nterms(L)), dtype=np.complex128)
    for l in range(L + 1):
        h = spherical_jn(l, k * r) + 1j * spherical_yn(l, k * r)
        for n in range(-l, l + 1):
            Yc = sph_harm_y(l, abs(n), th, ph)
            Yr = Yc.real if n == 0 else math.sqrt(2) * (-1) ** n * (Yc.real if n > 0 else Yc.imag)
            B[:, l * l + l + n] = h * Yr
    return B


def fit_columns(B, v):
    """Least squares with the columns scaled to unit norm: (coef (N,), relative residual)."""
    s = np.linalg.norm(B, axis=0)
    c = np.linalg.lstsq(B / s, v, rcond=None)[0] / s
    return c, float(np.linalg.norm(B @ c - v) / np.linalg.norm(v))
