"""Per-entry references of the numeric assembly (ds_assemble_kml: tet_geometry_kernel, assemble_blocks_kernel<4|10>), their
bounds and the test meshes, for tests/test_assembly_ref_cpu.py and tests/test_assembly_kernels_gpu.py.

Plain numpy, with fractions.Fraction for the geometry.  Nothing here comes from the oracle or from the code under test
except diffsound_amd.fem_tables: its tables are the kernel's documented input, and test_assembly_ref_cpu.py pins them against
an fp64 quadrature of its own.

Every value comes with a MAGNITUDE: the same sum over the absolute values of its terms.  A bound "c * 2^-53 * mag" then
needs no conditioning argument: c counts roundings, mag is what each rounding is relative to.
"""
from fractions import Fraction

import numpy as np

from diffsound_amd import fem_tables

U53 = 2.0 ** -53  # unit roundoff of fp64
# accumulate in the widest float numpy has (80-bit on x86; fp64 elsewhere - the bounds below hold either way, with less to spare)
_ACC = np.longdouble


# ---------------------------------------------------------------------------------------------------------------- geometry

def _cofactors(a):
    """cof[r][c] of the 3 x 3 ``a`` (any exact or float type) and, from the same formulas on absolute values, cofabs[r][c]."""
    cof = [[None] * 3 for _ in range(3)]
    cab = [[None] * 3 for _ in range(3)]
    for r in range(3):
        r1, r2 = (r + 1) % 3, (r + 2) % 3
        for c in range(3):
            c1, c2 = (c + 1) % 3, (c + 2) % 3
            cof[r][c] = a[r1][c1] * a[r2][c2] - a[r1][c2] * a[r2][c1]
            cab[r][c] = abs(a[r1][c1] * a[r2][c2]) + abs(a[r1][c2] * a[r2][c1])
    return cof, cab


def tet_geometry_exact(verts_f32, tets, order):
    """(geo (T, 13) fp64, bound (T, 13) fp64) from the fp32 coordinates the kernel reads, in exact rational arithmetic.

    geo: the kernel's layout - grad L_1..4 (rows of A^-1 and minus their sum, A = [p0-p3, p1-p3, p2-p3] as columns of the
    corner slots), then |det A| - each correctly rounded to fp64.
    bound: the running-error magnitude of a computed value: g = cof / det has  cofabs / |det| + |cof| detabs / det^2,
    grad L_4 the sum of its three terms' bounds and magnitudes, |det| has detabs.  A kernel that evaluates the cofactor
    formulas in fp64 stays within a small multiple of 2^-53 * bound (the GPU test derives the multiple)."""
    v = np.asarray(verts_f32)
    assert v.dtype == np.float32, "the reference reads the fp32 coordinates the kernel reads"
    tets = np.asarray(tets)
    cs = fem_tables.CORNER_SLOTS[order]
    T = tets.shape[0]
    geo = np.zeros((T, 13))
    bound = np.zeros((T, 13))
    for t in range(T):
        p = [[Fraction(float(v[tets[t, s], r])) for r in range(3)] for s in cs]
        a = [[p[c][r] - p[3][r] for c in range(3)] for r in range(3)]
        for r in range(3):
            for c in range(3):
                # (the kernel subtracts in fp64; the bound starts at the cofactors and takes the differences as exact)
                assert Fraction(float(a[r][c])) == a[r][c], "coordinate differences must be exact in fp64"
        cof, cab = _cofactors(a)
        det = sum(a[0][c] * cof[0][c] for c in range(3))
        assert det != 0, f"tet {t} has no volume"
        detabs = sum(abs(a[0][c]) * cab[0][c] for c in range(3))
        g = [[cof[c][k] / det for c in range(3)] for k in range(3)]  # (A^-1)[k][c] = cof[c][k] / det
        gb = [[cab[c][k] / abs(det) + abs(cof[c][k]) * detabs / (det * det) for c in range(3)] for k in range(3)]
        for c in range(3):
            g4 = -(g[0][c] + g[1][c] + g[2][c])
            b4 = sum(gb[k][c] + abs(g[k][c]) for k in range(3))
            for k in range(3):
                geo[t, 3 * k + c] = float(g[k][c])
                bound[t, 3 * k + c] = float(gb[k][c])
            geo[t, 9 + c] = float(g4)
            bound[t, 9 + c] = float(b4)
        geo[t, 12] = float(abs(det))
        bound[t, 12] = float(detabs)
    return geo, bound


def signed_dets(verts_f32, tets, order):
    """det A per tet (with its sign), exact, as fp64."""
    v = np.asarray(verts_f32)
    tets = np.asarray(tets)
    cs = fem_tables.CORNER_SLOTS[order]
    out = np.zeros(tets.shape[0])
    for t in range(tets.shape[0]):
        p = [[Fraction(float(v[tets[t, s], r])) for r in range(3)] for s in cs]
        a = [[p[c][r] - p[3][r] for c in range(3)] for r in range(3)]
        cof, _ = _cofactors(a)
        out[t] = float(sum(a[0][c] * cof[0][c] for c in range(3)))
    return out


# ---------------------------------------------------------------------------------------------------------------- assembly

def _element_blocks(D, G, J):
    """h[t,a,b,i,j] = J_t sum_kl D[a,k,b,l] G[t,k,i] G[t,l,j] in the accumulation type."""
    u = np.einsum("akbl,tki->tabli", D, G)
    h = np.einsum("tabli,tlj->tabij", u, G)
    return h * J[:, None, None, None, None]


def _mu_blocks(h):
    """tr(h) I + h^T per block."""
    tr = np.trace(h, axis1=-2, axis2=-1)
    return np.swapaxes(h, -1, -2) + tr[..., None, None] * np.eye(3, dtype=h.dtype)


def assemble_from_geometry(geo, tets, order, dtab, mtab, nv=None, dgeo=None):
    """Dense K_lambda, K_mu (nv, nv, 3, 3) and M_s (nv, nv) from the 13 geometry scalars per tet, by the formulas in the header
    of assemble.hip:  H_ab = J sum_kl D[a,k,b,l] grad L_k (x) grad L_l,  K_lambda += H,  K_mu += tr(H) I + H^T,
    M_s += J mtab[a,b], scattered with np.add.at.

    ``geo`` may be the exact geometry or the kernel's own array read back.  Returns a dict of fp64 arrays:
      Kl, Km, Ms              the values
      Kl_mag, Km_mag, Ms_mag  the same sums over the absolute value of every term (for K_mu with the trace terms)
      ncontrib (nv, nv)       element contributions per block
    and, when ``dgeo`` (T, 13) gives an absolute uncertainty of every geometry scalar,
      Kl_dgeo, Km_dgeo, Ms_dgeo   its first-order propagation: sum |D| (dG |G| + |G| dG) J + sum |D| |G| |G| dJ."""
    tets = np.asarray(tets).astype(np.int64)
    T, N = tets.shape
    assert N == fem_tables.NODES_PER_TET[order]
    nv = int(tets.max()) + 1 if nv is None else int(nv)
    geo = np.asarray(geo, dtype=np.float64)
    G = geo[:, :12].reshape(T, 4, 3).astype(_ACC)
    J = geo[:, 12].astype(_ACC)
    D = np.asarray(dtab, dtype=np.float64).astype(_ACC)
    M = np.asarray(mtab, dtype=np.float64).astype(_ACC)
    Ga, Da = np.abs(G), np.abs(D)

    h = _element_blocks(D, G, J)
    ha = _element_blocks(Da, Ga, np.abs(J))
    me = J[:, None, None] * M[None]
    per_elem = dict(Kl=h, Km=_mu_blocks(h), Ms=me, Kl_mag=ha, Km_mag=_mu_blocks(ha), Ms_mag=np.abs(me))
    if dgeo is not None:
        dgeo = np.asarray(dgeo, dtype=np.float64)
        dG = dgeo[:, :12].reshape(T, 4, 3).astype(_ACC)
        dJ = dgeo[:, 12].astype(_ACC)
        u1 = np.einsum("akbl,tki->tabli", Da, dG)
        u0 = np.einsum("akbl,tki->tabli", Da, Ga)
        hd = (np.einsum("tabli,tlj->tabij", u1, Ga) + np.einsum("tabli,tlj->tabij", u0, dG)) * np.abs(J)[:, None, None, None, None]
        hd = hd + np.einsum("tabli,tlj->tabij", u0, Ga) * dJ[:, None, None, None, None]
        per_elem.update(Kl_dgeo=hd, Km_dgeo=_mu_blocks(hd), Ms_dgeo=dJ[:, None, None] * np.abs(M)[None])

    rows = np.repeat(tets, N, axis=1).reshape(-1)  # (t, a, b) -> node of a
    cols = np.tile(tets, (1, N)).reshape(-1)       # (t, a, b) -> node of b
    out = {}
    for name, e in per_elem.items():
        dense = np.zeros((nv, nv) + e.shape[3:], dtype=_ACC)
        np.add.at(dense, (rows, cols), e.reshape((T * N * N,) + e.shape[3:]))
        out[name] = dense.astype(np.float64)
    nc = np.zeros((nv, nv), dtype=np.int64)
    np.add.at(nc, (rows, cols), 1)
    out["ncontrib"] = nc
    return out


# ---------------------------------------------------------------------------------------------------------------- BSR <-> dense

def bsr_rows(rowptr):
    """Row index of every slot of a CSR / BSR pattern."""
    rowptr = np.asarray(rowptr).astype(np.int64)
    return np.repeat(np.arange(rowptr.size - 1), np.diff(rowptr))


def bsr_to_dense(rowptr, colidx, vals):
    """The kernel's arrays in the dense layout of ``assemble_from_geometry``: vals (nnzb, 9) -> (nv, nv, 3, 3), vals (nnzb,)
    -> (nv, nv).  A slot that occurs twice in the pattern would be lost here: the caller asserts the pattern is duplicate-free
    (``pattern_is_clean``)."""
    rows = bsr_rows(rowptr)
    cols = np.asarray(colidx).astype(np.int64)
    vals = np.asarray(vals)
    nv = np.asarray(rowptr).size - 1
    if vals.ndim == 2:
        dense = np.zeros((nv, nv, 3, 3), dtype=vals.dtype)
        dense[rows, cols] = vals.reshape(-1, 3, 3)
    else:
        dense = np.zeros((nv, nv), dtype=vals.dtype)
        dense[rows, cols] = vals
    return dense


def pattern_is_clean(rowptr, colidx):
    """Monotone rowptr, columns strictly ascending inside every row (so no slot twice), all in range."""
    rowptr = np.asarray(rowptr).astype(np.int64)
    cols = np.asarray(colidx).astype(np.int64)
    nv = rowptr.size - 1
    if rowptr[0] != 0 or rowptr[-1] != cols.size or (np.diff(rowptr) < 0).any():
        return False
    if cols.size and (cols.min() < 0 or cols.max() >= nv):
        return False
    rows = bsr_rows(rowptr)
    same_row = rows[1:] == rows[:-1]
    return bool((np.diff(cols)[same_row] > 0).all())


# ---------------------------------------------------------------------------------------------------------------- the bounds

def block_bounds(ref):
    """The per-entry bounds of the kernel's block values GIVEN its geometry:  (nterms + 8) 2^-53 mag, with nterms = 16 + 16 * 3 +
    ncontrib fused operations behind an entry of K (16 for u = D G, 16 * 3 for h = u G over the three columns the lane carries,
    one per contribution for H += J h) and ncontrib for an entry of M_s; the 8 covers the trace and the final sum of K_mu."""
    nc = ref["ncontrib"].astype(np.float64)
    kb = (64.0 + nc + 8.0)[:, :, None, None] * U53
    return dict(Kl=kb * ref["Kl_mag"], Km=kb * ref["Km_mag"], Ms=(nc + 8.0) * U53 * ref["Ms_mag"])


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound over all entries and where it sits; 0 / 0 counts as 0, anything over a zero bound as inf, a
    NaN as inf."""
    got, ref, bound = np.broadcast_arrays(np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64),
                                          np.asarray(bound, dtype=np.float64))
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / bound)
    ratio = np.where(np.isnan(ratio), np.inf, ratio)
    if ratio.size == 0:
        return 0.0, ()
    at = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    return float(ratio[at]), tuple(int(i) for i in at)


def block_ratios(got, ref, bounds=None):
    """{name: (worst |got - ref| / bound, where)} for Kl, Km, Ms; ``got``: dict of dense arrays, ``bounds`` defaults to
    ``block_bounds(ref)``."""
    bounds = block_bounds(ref) if bounds is None else bounds
    return {k: worst_ratio(got[k], ref[k], bounds[k]) for k in ("Kl", "Km", "Ms")}


def flip_twin(geo, tets, order, dtab, mtab, flipped, nv=None):
    """What a mesh whose tets ``flipped`` (boolean per tet) had their local order swapped v1 <-> v2 must assemble to, from the
    UNFLIPPED tets and their geometry: relabelling the local nodes of an element is the same as permuting the tables, so the
    flipped tets take dtab[s][:, p][:, :, s][:, :, :, p] and mtab[s][:, s] (s = FLIP_SLOTS, p the swap of L_1 and L_2) and the
    others the tables as they are.  (The fp32 tables are symmetric under the swap only to their own rounding, 1e-7: comparing
    with the unflipped mesh under the SAME tables cannot hold to fp64 level.)  Returns the dict of assemble_from_geometry."""
    tets = np.asarray(tets)
    flipped = np.asarray(flipped, dtype=bool)
    nv = int(tets.max()) + 1 if nv is None else nv
    s, p = list(FLIP_SLOTS[order]), [1, 0, 2, 3]
    dsw = np.ascontiguousarray(np.asarray(dtab)[s][:, p][:, :, s][:, :, :, p])
    msw = np.ascontiguousarray(np.asarray(mtab)[s][:, s])
    a = assemble_from_geometry(geo[~flipped], tets[~flipped], order, dtab, mtab, nv=nv)
    b = assemble_from_geometry(geo[flipped], tets[flipped], order, dsw, msw, nv=nv)
    return {k: a[k] + b[k] for k in a}


def flip_geometry_allowance(plain, flipped, order, dtab, mtab, mask, nv):
    """What two ASSEMBLIES of the same elements may differ by because their geometry kernels saw the corners in different
    orders: each kernel's 13 scalars are within GEO_FACTOR 2^-53 bound of the exact ones (check (a)), but not the same bits -
    an exactly vanishing cofactor comes out as 0 in one order and as a residue of a fused multiply-add in the other - so every
    entry gets the first-order propagation of both uncertainties through H, on the swapped tets only (the others have the same
    bits in both).  ``plain`` / ``flipped``: (geo, bound, tets) of the exact geometry of the two meshes."""
    s, p = list(FLIP_SLOTS[order]), [1, 0, 2, 3]
    dsw = np.ascontiguousarray(np.asarray(dtab)[s][:, p][:, :, s][:, :, :, p])
    msw = np.ascontiguousarray(np.asarray(mtab)[s][:, s])
    out = None
    for (geo, gb, tets), (d, m) in ((plain, (dsw, msw)), (flipped, (dtab, mtab))):
        r = assemble_from_geometry(geo[mask], np.asarray(tets)[mask], order, d, m, nv=nv, dgeo=GEO_FACTOR * U53 * gb[mask])
        add = {k: r[k + "_dgeo"] for k in ("Kl", "Km", "Ms")}
        out = add if out is None else {k: out[k] + add[k] for k in add}
    return out


GEO_FACTOR = 16.0  # |kernel geometry - exact| <= GEO_FACTOR 2^-53 bound: a cofactor (2 roundings of cofabs), the determinant
# (that, a product and two sums: 5 of detabs), the reciprocal and the product (2), so at most 5 (cofabs / |det| + |cof| detabs /
# det^2) for a gradient, 5 detabs for |det| and 5 bound + 2 magnitudes for grad L_4 - and a factor of two to spare on top of 8.


# ---------------------------------------------------------------------------------------------------------------- meshes

# a symmetry of the element: swap v1 <-> v2 of the local node order (it flips the sign of det A)
FLIP_SLOTS = {1: (1, 0, 2, 3), 2: (2, 1, 0, 5, 4, 3, 7, 6, 8, 9)}


def flip_mask(T, every=3):
    """Boolean per tet: every ``every``-th one."""
    return np.arange(T) % every == 0


def flip_tets(tets, order, every=3):
    """``tets`` with the local order of every ``every``-th tet swapped v1 <-> v2."""
    tets = np.array(tets, copy=True)
    sel = flip_mask(tets.shape[0], every)
    tets[sel] = tets[sel][:, list(FLIP_SLOTS[order])]
    return tets


def islands(n, seed):
    """``n`` disconnected P1 tets with random well-shaped, positively oriented corners: nv = 4 n, nnzb = 16 n."""
    rng = np.random.default_rng(seed)
    base = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], dtype=np.float64)  # a regular tet
    verts = np.zeros((4 * n, 3))
    for t in range(n):
        q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        p = (base + 0.25 * rng.uniform(-1, 1, (4, 3))) @ q.T * rng.uniform(0.01, 0.03) + rng.uniform(-0.2, 0.2, 3)
        a = (p[:3] - p[3]).T
        if np.linalg.det(a) < 0:
            p[[0, 1]] = p[[1, 0]]
        verts[4 * t:4 * t + 4] = p
    return verts.astype(np.float32), np.arange(4 * n, dtype=np.int64).reshape(n, 4)


def graded_vertices(verts):
    """A fixed smooth distortion of a Kuhn box's nodes (it grades the cells towards one corner and shears them), then the
    scales (1, 1e-2, 1e2), then the offsets (1e3, -1e3, 1e3), then fp32: entries of K over many orders of magnitude, sliver
    elements with a large cond(A), and coordinates whose differences cancel most of their digits."""
    v = np.asarray(verts, dtype=np.float64)
    s = v / v.max(0)  # unit cube
    w = np.stack([s[:, 0] ** 2.0 + 0.15 * np.sin(2.0 * s[:, 1]) * s[:, 2],
                  s[:, 1] ** 1.5 + 0.20 * s[:, 0] * s[:, 2],
                  s[:, 2] ** 3.0 + 0.10 * np.cos(3.0 * s[:, 0]) * s[:, 1]], 1) * v.max(0)
    return (w * np.array([1.0, 1e-2, 1e2]) + np.array([1e3, -1e3, 1e3])).astype(np.float32)


def with_unused_nodes(verts, tets, at=3):
    """The mesh with two extra vertices that no tet references: one inserted at index ``at`` (the ids behind it move up), one
    appended.  Returns (verts, tets, ids of the two)."""
    verts = np.asarray(verts, dtype=np.float32)
    tets = np.asarray(tets).astype(np.int64)
    extra = np.array([[0.5, 0.5, 0.5], [-0.25, 0.75, 0.125]], dtype=np.float32)
    v = np.concatenate([verts[:at], extra[:1], verts[at:], extra[1:]], 0)
    t = np.where(tets >= at, tets + 1, tets)
    return v, t, (at, v.shape[0] - 1)


# ---------------------------------------------------------------------------------------------------------------- quadrature

def gauss_rule_f64(order):
    """(points (G, 4) barycentric, weights (G,)) of the (order+2)^3 collapsed Gauss-Legendre rule on the unit tet, in fp64:
    exact to degree 2 (order + 2) - 3 >= 4."""
    npts = order + 2
    x, w1 = np.polynomial.legendre.leggauss(npts)
    r, w1 = (x + 1) / 2, w1 / 2
    pts, wts = [], []
    for i in range(npts):
        lw = r[i]
        for j in range(npts):
            lz = r[j] * (1 - lw)
            for k in range(npts):
                ly = r[k] * (1 - lw - lz)
                pts.append((1 - lw - lz - ly, ly, lz, lw))
                wts.append(w1[i] * w1[j] * w1[k] * (1 - lw) ** 2 * (1 - r[j]))
    return np.array(pts), np.array(wts)


def tables_f64(order):
    """(dtab (N,4,N,4), mtab (N,N)) of the fp64 rule, shape functions written out here (local order of fem_tables)."""
    L, w = gauss_rule_f64(order)
    G = L.shape[0]
    if order == 1:
        N = L.copy()
        dN = np.broadcast_to(np.eye(4), (G, 4, 4)).copy()
    else:
        corner = {0: 0, 2: 1, 4: 2, 9: 3}
        mid = {1: (0, 1), 3: (1, 2), 5: (2, 0), 6: (0, 3), 7: (1, 3), 8: (2, 3)}
        N = np.zeros((G, 10))
        dN = np.zeros((G, 10, 4))
        for s, k in corner.items():
            N[:, s] = L[:, k] * (2 * L[:, k] - 1)
            dN[:, s, k] = 4 * L[:, k] - 1
        for s, (p, q) in mid.items():
            N[:, s] = 4 * L[:, p] * L[:, q]
            dN[:, s, p] = 4 * L[:, q]
            dN[:, s, q] = 4 * L[:, p]
    return np.einsum("g,gak,gbl->akbl", w, dN, dN), np.einsum("g,ga,gb->ab", w, N, N)
