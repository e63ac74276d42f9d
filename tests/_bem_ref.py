"""What the BEM tests share (not a test module): the NumPy restatement of csrc/bem.hip's formulation and quadrature
(6-point rules for regular pairs; for near pairs a 96-point outer rule with the static inner part in closed form and the
smooth remainder by the inner 6-point rule), runnable in fp64 (the oracle) or in fp32 throughout (only to measure what
fp32 arithmetic costs this algorithm), the per-entry scales that errors are divided by, the near / regular
classification with its borderline band, and the cases of tests/test_bem_kernels_gpu.py.
tests/test_bem_cpu.py checks the restatement against brute-force integration and the exact field of a point source;
tests/test_bem_ref_cpu.py checks the scales, the cases and that the fp64 values are the ones the restatement always gave."""
import functools

import numpy as np

NEAR_RATIO = 1.75  # DS_BEM_NEAR_RATIO of include/diffsound_hip.h
INV4PI = 1.0 / (4.0 * np.pi)
BORDERLINE = 1e-5  # a pair is borderline when |d2 - (1.75 h)^2| <= BORDERLINE (1.75 h)^2
MARGIN = 4.0       # kernel bound = MARGIN x the fp32 restatement's level on the same case

_A1, _W1, _A2, _W2 = 0.445948490915965, 0.223381589678011, 0.091576213509771, 0.109951743655322


def cdtype(dtype):
    """The complex type of a real one: float32 -> complex64, float64 -> complex128."""
    return np.result_type(dtype, np.complex64)


def rule6(dtype=np.float64):
    """6-point degree-4 rule: barycentrics (6, 3) and weights (6,) summing to 1 (the kernel's order)."""
    L, W = [], []
    for a, w in ((_A1, _W1), (_A2, _W2)):
        b = 1.0 - 2.0 * a
        for r in range(3):
            l0 = b if r == 0 else a
            l1 = b if r == 1 else a
            L.append((l0, l1, 1.0 - l0 - l1))
            W.append(w)
    return np.array(L, dtype=dtype), np.array(W, dtype=dtype)


def split_rule(levels, dtype=np.float64):
    """The 6-point rule on each of the 4**levels congruent pieces of the triangle: (l0, l1, l2) on the corners
    (p0, p1, p2) as the kernel maps them (x = p0 + u e1 + v e2) and weights summing to 1.  The table is built in fp64
    and rounded once to ``dtype``."""
    s = 2 ** levels
    L6, W6 = rule6()
    out, wts = [], []
    for i in range(s):
        for j in range(s - i):
            tris = [((i, j), (i + 1, j), (i, j + 1))]
            if i + j <= s - 2:
                tris.append(((i + 1, j), (i + 1, j + 1), (i, j + 1)))
            for c in tris:
                c = np.array(c, dtype=np.float64) / s  # (u, v) corners
                uv = L6 @ c
                out.append(np.stack([1 - uv[:, 0] - uv[:, 1], uv[:, 0], uv[:, 1]], 1))
                wts.append(W6 / s ** 2)
    return np.concatenate(out).astype(dtype), np.concatenate(wts).astype(dtype)


NEAR_OUTER = split_rule(2)  # 16 pieces x 6 points = 96 (the kernel's near-pair outer rule)


def geometry(V, F, dtype=np.float64):
    V = np.asarray(V, dtype=dtype)
    F = np.asarray(F, dtype=np.int64)
    P = V[F]  # (m, 3, 3)
    cr = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    area = 0.5 * np.linalg.norm(cr, axis=1)
    L6, W6 = rule6(dtype)
    e = [P[:, 1] - P[:, 0], P[:, 2] - P[:, 0], P[:, 2] - P[:, 1]]
    return dict(P=P, n=cr / np.linalg.norm(cr, axis=1, keepdims=True), area=area, c=P.mean(1),
                h=np.sqrt(np.max([(x * x).sum(1) for x in e], axis=0)),
                q=np.einsum("qa,mad->mqd", L6, P), w=area[:, None] * W6[None, :])


def static_integrals(x, P, n):
    """x (K, 3) points, P (K, 3, 3) triangles, n (K, 3) unit normals -> (int 1/|x-y| dy, int n.(x-y)/|x-y|^3 dy), in
    the type of ``x``."""
    a = P - x[:, None, :]
    la = np.linalg.norm(a, axis=2)
    w = -(n * a[:, 0]).sum(1)
    aw = np.abs(w)
    acc = np.zeros(len(x), dtype=x.dtype)
    for e in range(3):
        pa, pb = a[:, e], a[:, (e + 1) % 3]
        ra, rb = la[:, e], la[:, (e + 1) % 3]
        d = pb - pa
        s = d / np.linalg.norm(d, axis=1, keepdims=True)
        m = np.cross(s, n)
        t0 = (m * pa).sum(1)
        sm, sp = (s * pa).sum(1), (s * pb).sum(1)
        ok = np.abs(t0) > 1e-30
        with np.errstate(divide="ignore", invalid="ignore"):
            f = np.where(sp + sm >= 0, np.log((rb + sp) / (ra + sm)), np.log((ra - sm) / (rb - sp)))
            r02 = t0 * t0 + w * w
            at = np.arctan(t0 * sp / (r02 + aw * rb)) - np.arctan(t0 * sm / (r02 + aw * ra))
        acc += np.where(ok, t0 * f - np.where(aw > 0, aw * at, 0.0), 0.0)
    det = np.einsum("kd,kd->k", a[:, 0], np.cross(a[:, 1], a[:, 2]))
    den = (la[:, 0] * la[:, 1] * la[:, 2] + (a[:, 0] * a[:, 1]).sum(1) * la[:, 2] + (a[:, 0] * a[:, 2]).sum(1) * la[:, 1]
           + (a[:, 1] * a[:, 2]).sum(1) * la[:, 0])
    return acc, -2.0 * np.arctan2(det, den)


def kernels(x, y, ny, k):
    """G and dG/dn_y for broadcastable point arrays (..., 3), in their type (k is a Python float)."""
    d = x - y
    r = np.sqrt((d * d).sum(-1))
    e = np.exp(1j * k * r)
    G = e * INV4PI / r
    dG = (ny * d).sum(-1) * (1 - 1j * k * r) * e * INV4PI / r ** 3
    return G, dG


def near_inner(x, gj, j, k, coincident):
    """Inner integrals (int G, int dG/dn_y) over faces j (K,) at the points x (K, 3): static part exact, remainder by
    the 6-point rule.  ``coincident`` (K,) bool: K = 0 there."""
    s1, dl = static_integrals(x, gj["P"][j], gj["n"][j])
    d = x[:, None, :] - gj["q"][j]
    r = np.maximum(np.sqrt((d * d).sum(-1)), 1e-15)
    e = np.exp(1j * k * r)
    w = gj["w"][j]
    v = s1 * INV4PI + (w * (e - 1) * INV4PI / r).sum(1)
    nd = (d * gj["n"][j][:, None, :]).sum(-1)
    kk = dl * INV4PI + (w * nd * ((1 - 1j * k * r) * e - 1) * INV4PI / r ** 3).sum(1)
    return v, np.where(coincident, 0.0, kk)


def near_pair(gi, i, gj, j, k, coincident, outer=NEAR_OUTER):
    """Near-pair entries (V_ij, K_ij) for index arrays i, j (Np,) (or scalars)."""
    i, j, coincident = np.atleast_1d(i), np.atleast_1d(j), np.atleast_1d(coincident)
    dt = gi["P"].dtype
    L, W = outer[0].astype(dt), outer[1].astype(dt)
    nq = len(W)
    x = np.einsum("qa,pad->pqd", L, gi["P"][i]).reshape(-1, 3)
    v, kk = near_inner(x, gj, np.repeat(j, nq), k, np.repeat(coincident, nq))
    wx = W[None, :] * gi["area"][i][:, None]
    return (wx * v.reshape(-1, nq)).sum(1), (wx * kk.reshape(-1, nq)).sum(1)


def _pair_d2_t2(g):
    d2 = ((g["c"][:, None, :] - g["c"][None, :, :]) ** 2).sum(-1)
    h = NEAR_RATIO * np.maximum(g["h"][:, None], g["h"][None, :])
    return d2, h * h


def near_mask(g):
    d2, t2 = _pair_d2_t2(g)
    return d2 < t2


def assemble(g, k, gvec=None, rows=256, near=None):
    """Restatement of ds_bem_assemble in the type of ``g``: (A = -1/2 M + K, V, rhs = V g, near mask).  ``near`` given:
    that classification instead of this type's own (the fp32 run of a case takes the fp64 run's)."""
    m = len(g["area"])
    ct = cdtype(g["P"].dtype)
    near = near_mask(g) if near is None else near
    V = np.empty((m, m), ct)
    K = np.empty((m, m), ct)
    for i0 in range(0, m, rows):
        sl = slice(i0, min(m, i0 + rows))
        x = g["q"][sl][:, None, :, None, :]  # (r, 1, 6, 1, 3)
        y = g["q"][None, :, None, :, :]      # (1, m, 1, 6, 3)
        with np.errstate(divide="ignore", invalid="ignore"):  # coincident points: near pairs, replaced below
            G, dG = kernels(x, y, g["n"][None, :, None, None, :], k)
            ww = g["w"][sl][:, None, :, None] * g["w"][None, :, None, :]
            V[sl] = (ww * G).sum((2, 3))
            K[sl] = (ww * dG).sum((2, 3))
    I, J = np.nonzero(near)
    for c0 in range(0, len(I), 512):
        i, j = I[c0:c0 + 512], J[c0:c0 + 512]
        V[i, j], K[i, j] = near_pair(g, i, g, j, k, i == j)
    A = K - 0.5 * np.diag(g["area"])
    rhs = None if gvec is None else V @ np.asarray(gvec).astype(ct)
    return A, V, rhs, near


def _point_d2_t2(g, pts):
    d2 = ((pts[:, None, :] - g["c"][None]) ** 2).sum(-1)
    return d2, (NEAR_RATIO * g["h"][None]) ** 2


def potential(g, k, gco, uco, pts, near=None):
    """Restatement of ds_bem_potential in the type of ``g``: -S g + D u at pts (P, 3).  ``near`` (P, m): as in assemble."""
    dt = g["P"].dtype
    pts = np.asarray(pts, dtype=dt)
    S, D = _point_operators(g, k, pts, near)
    return -S @ np.asarray(gco).astype(cdtype(dt)) + D @ np.asarray(uco).astype(cdtype(dt))


def _point_operators(g, k, pts, near=None):
    x = pts[:, None, None, :]
    G, dG = kernels(x, g["q"][None], g["n"][None, :, None, :], k)
    S = (g["w"][None] * G).sum(-1)
    D = (g["w"][None] * dG).sum(-1)
    if near is None:
        d2, t2 = _point_d2_t2(g, pts)
        near = d2 < t2
    p, j = np.nonzero(near)
    if len(p):
        S[p, j], D[p, j] = near_inner(pts[p], g, j, k, np.zeros(len(p), bool))
    return S, D


# ---------------------------------------------------------------------- point-source problem
def point_source_data(g, k, x0):
    """g = DP0 projection (face mean, 6-point rule) of dG(., x0)/dn and the exact boundary trace G(., x0)."""
    d = g["q"] - x0
    r = np.linalg.norm(d, axis=-1)
    e = np.exp(1j * k * r)
    dn = (d * g["n"][:, None, :]).sum(-1) * (1j * k * r - 1) * e * INV4PI / r ** 3
    gvec = (g["w"] * dn).sum(1) / g["area"]
    u_ex = (g["w"] * e * INV4PI / r).sum(1) / g["area"]
    return gvec, u_ex


def listener_points(radius):
    rng = np.random.default_rng(7)
    dirs = rng.normal(size=(24, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    return np.concatenate([dirs * radius * s for s in (2.0, 5.0, 10.0)])


def exact_field(pts, k, x0):
    r = np.linalg.norm(pts - x0, axis=1)
    return np.exp(1j * k * r) * INV4PI / r


# ---------------------------------------------------------------------- classification
def borderline_pairs(g):
    """(m, m) bool: pairs within BORDERLINE of the near threshold, where fp32 and fp64 may classify differently."""
    d2, t2 = _pair_d2_t2(g)
    return np.abs(d2 - t2) <= BORDERLINE * t2


def borderline_points(g, pts):
    """(P,) bool: points with at least one face within BORDERLINE of the near threshold (left out whole)."""
    d2, t2 = _point_d2_t2(g, np.asarray(pts, dtype=g["P"].dtype))
    return (np.abs(d2 - t2) <= BORDERLINE * t2).any(1)


def threshold_clearance(d2, t2):
    """Smallest |d2 - t2| / t2: how far the closest pair is from the threshold (borderline below BORDERLINE)."""
    return float((np.abs(d2 - t2) / t2).min())


# ---------------------------------------------------------------------- per-entry scales
def pair_scales(g, k, near, rows=256):
    """(sV, sK) (m, m) real: the magnitude of what entry (i, j) sums.  Regular pairs, over the 6 x 6 rule:
    sV = sum w_p w_q / (4 pi r), sK = sum w_p w_q sqrt(1 + (k r)^2) / (4 pi r^2) (|d| where the kernel has n.d, so that
    coplanar neighbours, whose K is rounding, keep a scale).  Near pairs, coincident included: sV = V_ij at k = 0 and
    sK = area_i / 2, the bound of the solid-angle integral and the diagonal's own magnitude."""
    m = len(g["area"])
    sV = np.empty((m, m))
    sK = np.empty((m, m))
    for i0 in range(0, m, rows):
        sl = slice(i0, min(m, i0 + rows))
        d = g["q"][sl][:, None, :, None, :] - g["q"][None, :, None, :, :]
        r = np.sqrt((d * d).sum(-1))
        ww = g["w"][sl][:, None, :, None] * g["w"][None, :, None, :]
        with np.errstate(divide="ignore", invalid="ignore"):  # coincident points: near pairs, replaced below
            sV[sl] = (ww * INV4PI / r).sum((2, 3))
            sK[sl] = (ww * np.sqrt(1 + (k * r) ** 2) * INV4PI / r ** 2).sum((2, 3))
    I, J = np.nonzero(near)
    for c0 in range(0, len(I), 512):
        i, j = I[c0:c0 + 512], J[c0:c0 + 512]
        sV[i, j] = near_pair(g, i, g, j, 0.0, i == j)[0].real
        sK[i, j] = 0.5 * g["area"][i]
    return sV, sK


def point_scales(g, k, pts, gco, uco, near):
    """(P,) real: s_p = sum_j (sS_pj |g_j| + sD_pj |u_j|); regular faces as in pair_scales with the single point x, near
    faces sS = the static S at k = 0 and sD = 1/2."""
    d = pts[:, None, None, :] - g["q"][None]
    r = np.sqrt((d * d).sum(-1))
    sS = (g["w"][None] * INV4PI / r).sum(-1)
    sD = (g["w"][None] * np.sqrt(1 + (k * r) ** 2) * INV4PI / r ** 2).sum(-1)
    p, j = np.nonzero(near)
    if len(p):
        sS[p, j] = near_inner(pts[p], g, j, 0.0, np.zeros(len(p), bool))[0].real
        sD[p, j] = 0.5
    return sS @ np.abs(gco) + sD @ np.abs(uco)


def worst(got, want, scale, mask=None):
    """Largest complex error |got - want| / scale over the entries of ``mask`` (all of them: None); 0.0 over none."""
    e = np.abs(np.asarray(got).astype(np.complex128) - want) / scale
    if mask is not None:
        e = e[mask]
    return float(e.max()) if e.size else 0.0


# ---------------------------------------------------------------------- the cases of tests/test_bem_kernels_gpu.py
RADIUS = 0.1
SHIFT = (0.7, -0.4, 1.1)
PLATE = (0.1, 0.03, 0.005)
CASES_A = [("A", 0.0, False), ("A", 1.0, False), ("A", 30.0, False), ("A", 300.0, False), ("A", 500.0, False),
           ("A", 300.0, True)]
CASES_B = [("B", 0.0, False), ("B", 30.0, False), ("B", 300.0, False)]
C_SIZES = (1, 7, 9, 255, 256, 257)
C_K = 30.0


def case_id(case):
    return f"{case[0]}-k{case[1]:g}" + ("-shifted" if case[2] else "")


@functools.lru_cache(maxsize=None)
def mesh(name, shifted=False):
    """fp32 vertices and faces of a case's surface.  A: icosphere(1) at radius 0.1 (80 faces), also translated by SHIFT;
    B: the surface of kuhn_box(2) as a 0.1 x 0.03 x 0.005 plate (48 faces: stretched, and the two large sides are
    stacked near pairs); C: icosphere(2) at radius 0.1 (320 faces, the first n are used)."""
    import torch

    from diffsound_amd import meshgen
    from diffsound_amd.diffelastic import bem
    from diffsound_amd.diffelastic.mesh import TetMesh

    if name == "B":
        v, t = meshgen.kuhn_box(2, box=(1.0, 1.0, 1.0))
        tri, _ = bem.surface_of(TetMesh(torch.from_numpy(v), torch.from_numpy(t).long()))
        v, f = (v.astype(np.float64) * np.array(PLATE)).astype(np.float32), tri.numpy().astype(np.int32)
    else:
        v, f = meshgen.icosphere(1 if name == "A" else 2, radius=RADIUS)
    if shifted:
        v = (v.astype(np.float64) + np.array(SHIFT)).astype(np.float32)
    v.setflags(write=False)
    f.setflags(write=False)
    return v, f


def internal_order(v, f):
    """The model's face order (Morton order of the fp32 centroids), computed on the host."""
    import torch

    from diffsound_amd.diffelastic import bem

    vt = torch.from_numpy(np.array(v))
    return bem._morton_order(vt[torch.from_numpy(np.array(f)).long()].mean(1)).numpy()


def coefficients(m, seed):
    """Two complex64 coefficient vectors (Neumann data g, surface pressure u) of a case."""
    rng = np.random.default_rng(seed)
    z = rng.normal(size=(4, m))
    return (z[0] + 1j * z[1]).astype(np.complex64), (z[2] + 1j * z[3]).astype(np.complex64)


def point_triangle_distance(x, P):
    """Distances (K, m) from the points x (K, 3) to the triangles P (m, 3, 3): the plane where the foot lies inside, else
    the nearest edge."""
    best = np.full((len(x), len(P)), np.inf)
    for e in range(3):
        a, d = P[None, :, e], (P[:, (e + 1) % 3] - P[:, e])[None]
        t = np.clip(((x[:, None] - a) * d).sum(-1) / (d * d).sum(-1), 0.0, 1.0)
        best = np.minimum(best, np.linalg.norm(x[:, None] - a - t[..., None] * d, axis=-1))
    e1, e2 = (P[:, 1] - P[:, 0])[None], (P[:, 2] - P[:, 0])[None]
    n = np.cross(e1, e2)
    r = x[:, None] - P[None, :, 0]
    nn = (n * n).sum(-1)
    u = (np.cross(r, e2) * n).sum(-1) / nn
    v = (np.cross(e1, r) * n).sum(-1) / nn
    inside = (u >= 0) & (v >= 0) & (u + v <= 1)
    return np.where(inside, np.minimum(best, np.abs((r * n).sum(-1)) / np.sqrt(nn)), best)


def potential_points(g, k, count=257):
    """The points of the potential check for a surface ``g`` (fp64 geometry in the order the kernel sees), rounded to
    fp32 (what the kernel is given) and cast up, cycled to ``count`` points:
    listeners at 2, 5, 10 radii about the surface's centre, while k r <= 100; 0.3 h above and 0.2 h below centroids;
    1e-3 h above and below an interior point of a face (solid angle near -+2 pi); points in the plane of a face but
    outside it, on the line of an edge and off it, kept only if no other face comes closer than 0.1 edge lengths.
    Returns (points (count, 3) fp64, kinds (count,) of "far", "offset", "skin", "edge-line", "in-plane")."""
    P, c, n, h = g["P"], g["c"], g["n"], g["h"]
    m = len(h)
    verts = P.reshape(-1, 3)
    centre = 0.5 * (verts.min(0) + verts.max(0))
    radius = np.linalg.norm(verts - centre, axis=1).max()
    out, kinds = [], []
    unit = listener_points(0.5)[:24]  # unit directions
    for s in (2.0, 5.0, 10.0):
        if k * s * radius <= 100.0 * (1 + 1e-6):  # fp32 vertices: the radius is 0.1 to rounding
            out.append(centre + unit * s * radius)
            kinds += ["far"] * 24
    a = min(40, m - 8)
    out += [c[:a] + 0.3 * h[:a, None] * n[:a], c[a:a + 20] - 0.2 * h[a:a + 20, None] * n[a:a + 20]]
    kinds += ["offset"] * (a + len(c[a:a + 20]))
    inner = 0.45 * P[:8, 0] + 0.35 * P[:8, 1] + 0.2 * P[:8, 2]
    out += [inner + 1e-3 * h[:8, None] * n[:8], inner - 1e-3 * h[:8, None] * n[:8]]
    kinds += ["skin"] * 16
    cand, ckind, clen = [], [], []
    for f in range(0, m, max(1, m // 16)):
        for e in range(3):
            va, vb, vc = P[f, e], P[f, (e + 1) % 3], P[f, (e + 2) % 3]
            mid = 0.5 * (va + vb)
            cand += [va + 1.5 * (vb - va), mid + 0.7 * (mid - vc)]
            ckind += ["edge-line", "in-plane"]
            clen += [np.linalg.norm(vb - va)] * 2
    cand, clen = np.array(cand), np.array(clen)
    clear = point_triangle_distance(cand, P).min(1) >= 0.1 * clen
    out.append(cand[clear])
    kinds += [kk for kk, ok in zip(ckind, clear) if ok]
    pts = np.concatenate(out).astype(np.float32).astype(np.float64)
    idx = np.arange(count) % len(pts)
    return pts[idx], np.array(kinds)[idx]


# ---------------------------------------------------------------------- ds_bem_geometry's record
EPS32 = 2.0 ** -24  # unit roundoff of fp32


def face_records(g):
    """(m, 48) fp64: the face record of include/diffsound_hip.h from the fp64 geometry ``g``."""
    m = len(g["area"])
    rec = np.zeros((m, 48))
    rec[:, 0:18] = g["q"].reshape(m, 18)
    rec[:, 18:24] = g["w"]
    rec[:, 24:27], rec[:, 27:30], rec[:, 30], rec[:, 31] = g["n"], g["c"], g["h"], g["area"]
    rec[:, 32:41] = g["P"].reshape(m, 9)
    return rec


def record_bounds(g):
    """(m, 48) absolute bounds on the fp32 record, from the operation count of each field, u = EPS32.  The vertices are
    the inputs (exact), M = the face's largest |coordinate|, h = its diameter, and every edge component is one rounded
    subtraction of exact inputs (relative error u).
    q: the barycentrics carry a(u) + the rounding of b = 1 - 2a (2u absolute) + l2 = 1 - l0 - l1 (two more roundings on
       top of both): at most 10u in all three together; three products (u, the l's sum to 1) and two additions (2u of a
       partial sum <= M): 13u M, taken as 16u M.
    c: two additions of a sum <= 3M (5u M), the rounded 1/3 and its product (2u M), over 3: taken as 5u M.
    cross product, per component: two products of two edge components (3u each) and one subtraction (u):
       <= 4u |e1| |e2| <= 4u h^2, 7u h^2 for the vector.
    area = |cr| / 2: the vector's 7u h^2 and the norm's own three squares, two additions and root (2.5u |cr|, |cr| <= h^2)
       halved: taken as 5u h^2.  weights (<= 0.2234 area): the rounded constant and the product add 2u: taken as 1.5u h^2.
    n = cr / |cr|: (4u h^2 + 9.5u h^2) / |cr| and the division's u: taken as 15u h^2 / |cr|.
    h: squares (3u), two additions (2u), root: 4u h.
    Floats 32-40 (vertices) and 41-47 (zero tail): exact."""
    m = len(g["area"])
    M = np.abs(g["P"]).reshape(m, 9).max(1)
    h, two_area = g["h"], 2 * g["area"]
    b = np.zeros((m, 48))
    b[:, 0:18] = 16 * EPS32 * M[:, None]
    b[:, 18:24] = 1.5 * EPS32 * (h * h)[:, None]
    b[:, 24:27] = (15 * EPS32 * h * h / two_area)[:, None]
    b[:, 27:30] = 5 * EPS32 * M[:, None]
    b[:, 30] = 4 * EPS32 * h
    b[:, 31] = 5 * EPS32 * h * h
    return b


# ---------------------------------------------------------------------- a case's truth, fp32 level and bounds
def _categories(near, skip):
    return {"regular": ~near & ~skip, "near": near & ~skip}


def assembly_truth(v, f, k, gvec):
    """Everything the assembly check of one surface and wave number needs: the fp64 restatement from the fp32 vertices
    (A, V, K, rhs, near), the borderline pairs, the scales, and the fp32 restatement's level per quantity and category
    (the fp32 run takes the fp64 classification, so it measures arithmetic alone)."""
    g = geometry(v, f)
    g32 = geometry(v, f, np.float32)
    A, V, rhs, near = assemble(g, k, gvec.astype(np.complex128))
    A32, V32, rhs32, _ = assemble(g32, k, gvec, near=near)
    skip = borderline_pairs(g)
    sV, sK = pair_scales(g, k, near)
    half = 0.5 * np.diag(g["area"])
    return dict(g=g, A=A, V=V, K=A + half, rhs=rhs, near=near, skip=skip, sV=sV, sK=sK, srhs=sV @ np.abs(gvec),
                V32=V32, K32=A32 + 0.5 * np.diag(g32["area"]).astype(np.float32), rhs32=rhs32)


def assembly_levels(t, n=None):
    """fp32 level per (quantity, category) for the leading n x n block of the truth ``t`` (all of it: None)."""
    n = len(t["sV"]) if n is None else n
    s = np.s_[:n, :n]
    out = {}
    for cat, mask in _categories(t["near"][s], t["skip"][s]).items():
        out["V", cat] = worst(t["V32"][s], t["V"][s], t["sV"][s], mask)
        out["K", cat] = worst(t["K32"][s], t["K"][s], t["sK"][s], mask)
    return out
