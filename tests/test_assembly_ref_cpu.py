"""Anchors of tests/_assembly_ref.py (no GPU): the tables against an fp64 quadrature, one element in closed form, the structure of
the assembled matrices, the oracle, the invariances - and the sensitivity of the bounds of tests/test_assembly_kernels_gpu.py:
each deliberately wrong copy of the reference's own output must trip the check that guards against it."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _assembly_ref as R  # noqa: E402
from diffsound_amd import fem_tables, meshgen  # noqa: E402
from oracle import fem  # noqa: E402

RHO = 2700.0
LAM, MU = fem.lame(5e10, 0.25)


def _box(cells, order):
    v, t = meshgen.kuhn_box(cells)
    v, t = fem.to_high_order(torch.from_numpy(v), torch.from_numpy(t).long(), order)
    return v.numpy().astype(np.float32), t.numpy()


@pytest.fixture(scope="module")
def meshes():
    out = {}
    for name, (cells, order) in {"box2-o1": (2, 1), "box2-o2": (2, 2), "box3-o1": (3, 1)}.items():
        v, t = _box(cells, order)
        out[name] = (v, t, order)
    v, t, _ = out["box2-o2"]
    out["graded"] = (R.graded_vertices(v), t, 2)
    return out


@pytest.fixture(scope="module")
def refs(meshes):
    """name -> (geo, geo bound, assembled dict), computed once and left unchanged."""
    out = {}
    for name, (v, t, order) in meshes.items():
        geo, gb = R.tet_geometry_exact(v, t, order)
        ref = R.assemble_from_geometry(geo, t, order, fem_tables.stiffness_table(order), fem_tables.mass_table(order, RHO),
                                       nv=v.shape[0])
        out[name] = (geo, gb, ref)
    return out


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


# ---------------------------------------------------------------------------------------------------------------- tables

@pytest.mark.parametrize("order", [1, 2])
def test_tables_against_fp64_quadrature(order):
    """The tables the kernel reads against the same collapsed Gauss-Legendre rule built in fp64 (exact for these integrands):
    the distance is the fp32 rounding of the reference project's rule.  Measured: dtab 3.5e-7 / 1.4e-7, mtab 5.0e-7 / 3.1e-7,
    mass_table(., 2700) 5.1e-7 / 3.0e-7 for orders 1 / 2; bound 1e-6, a few fp32 roundings."""
    pts, w = R.gauss_rule_f64(order)
    assert abs(w.sum() - 1.0 / 6.0) <= 1e-15
    assert np.abs(pts.sum(1) - 1).max() <= 1e-15
    d64, m64 = R.tables_f64(order)
    dd = _rel(fem_tables.stiffness_table(order), d64)
    dm = _rel(fem_tables.mass_table_f32(order).astype(np.float64), m64)
    dr = _rel(fem_tables.mass_table(order, RHO), RHO * m64)
    print(f"tables order {order}: dtab {dd:.2e} mtab {dm:.2e} mass_table(., {RHO:g}) {dr:.2e}")
    assert dd < 1e-6 and dm < 1e-6 and dr < 1e-6
    # the fp64 rule integrates the P2 mass products exactly: closed forms of the unit tet
    if order == 1:
        assert np.allclose(m64, (1 + np.eye(4)) / 120, rtol=0, atol=1e-16)
        assert np.allclose(d64, np.einsum("ak,bl->akbl", np.eye(4), np.eye(4)) / 6, rtol=0, atol=1e-16)
    else:
        assert abs(m64.sum() - 1.0 / 6.0) <= 1e-15 and np.allclose(m64, m64.T, rtol=0, atol=1e-17)
        assert abs(m64[0, 0] - 1.0 / 420.0) <= 1e-16 and abs(m64[1, 1] - 4.0 / 315.0) <= 1e-16


# ---------------------------------------------------------------------------------------------------------------- one element

def test_single_p1_element_closed_form():
    """One P1 tet with rational corners: A = [[1,1,1/2],[0,2,1],[0,0,4]] (columns p0-p3, p1-p3, p2-p3), det 8, V = 4/3,
    A^-1 = [[1,-1/2,0],[0,1/2,-1/8],[0,0,1/4]] written out by hand.  K_lambda = V g_a,i g_b,j, K_mu = V (g_a . g_b I + g_b (x)
    g_a), M_s = rho V (1 + delta_ab) / 20; agreement at the tables' fp32 level."""
    off = np.array([0.25, -0.5, 2.0])
    p = np.array([[1, 0, 0], [1, 2, 0], [0.5, 1, 4], [0, 0, 0]], dtype=np.float64) + off
    v = p.astype(np.float32)
    assert np.array_equal(v.astype(np.float64), p)
    t = np.array([[0, 1, 2, 3]])
    geo, gb = R.tet_geometry_exact(v, t, 1)
    g = np.array([[1, -0.5, 0], [0, 0.5, -0.125], [0, 0, 0.25], [-1, 0, -0.125]])
    assert np.array_equal(geo[0, :12].reshape(4, 3), g) and geo[0, 12] == 8.0
    assert (gb[0] >= np.abs(geo[0]) - 1e-300).all()  # a magnitude is never below the value
    V = 8.0 / 6.0
    ref = R.assemble_from_geometry(geo, t, 1, fem_tables.stiffness_table(1), fem_tables.mass_table(1, RHO))
    Kl = V * np.einsum("ai,bj->abij", g, g)
    Km = V * (np.einsum("ak,bk->ab", g, g)[:, :, None, None] * np.eye(3) + np.einsum("bi,aj->abij", g, g))
    Ms = RHO * V * (1 + np.eye(4)) / 20
    for name, want in (("Kl", Kl), ("Km", Km), ("Ms", Ms)):
        d = _rel(ref[name], want)
        print(f"single P1 element {name}: {d:.2e}")
        assert d < 1e-6
    assert (ref["ncontrib"] == 1).all()
    # the flipped element (v1 <-> v2) has det -8 and the same |det|
    gf, _ = R.tet_geometry_exact(v, t[:, list(R.FLIP_SLOTS[1])], 1)
    assert gf[0, 12] == 8.0 and R.signed_dets(v, t[:, list(R.FLIP_SLOTS[1])], 1)[0] == -8.0
    assert np.array_equal(gf[0, :12].reshape(4, 3), g[[1, 0, 2, 3]])


# ---------------------------------------------------------------------------------------------------------------- structure

def _effective_positions(v, t, order):
    """Where the affine element map puts every node: the corners at their coordinates, a mid-edge node at the mean of its edge's
    corners (the assembly reads the corners only, so a rigid motion is interpolated from THESE positions)."""
    x = v.astype(np.float64).copy()
    if order == 2:
        cs = fem_tables.CORNER_SLOTS[2]
        for slot, (p, q) in fem_tables._MID.items():
            x[t[:, slot]] = 0.5 * (v[t[:, cs[p]]].astype(np.float64) + v[t[:, cs[q]]].astype(np.float64))
    return x


def _rigid_defect(K4, x):
    """max over rows and the six rigid-body fields about the centroid of |K f| / (|K| |f|)."""
    nv = x.shape[0]
    K = K4.transpose(0, 2, 1, 3).reshape(3 * nv, 3 * nv)
    c = x - x.mean(0)
    F = np.zeros((3 * nv, 6))
    for a in range(3):
        F[a::3, a] = 1
    F[0::3, 3], F[1::3, 3] = -c[:, 1], c[:, 0]
    F[1::3, 4], F[2::3, 4] = -c[:, 2], c[:, 1]
    F[2::3, 5], F[0::3, 5] = -c[:, 0], c[:, 2]
    return float((np.abs(K @ F) / (np.abs(K) @ np.abs(F))).max()), float(np.abs(K - K.T).max() / np.abs(K).max())


@pytest.mark.parametrize("name", ["box2-o1", "box2-o2", "graded"])
def test_structure(meshes, refs, name):
    """K = lam K_lambda + mu K_mu is symmetric to 1e-14 and annihilates the six rigid-body fields to 1e-12 of the row sums of
    |K| |field| - the latter with the tables of the fp64 rule, and with the project's own P1 table.  The project's P2 table
    carries the reference project's fp32 rounding of the Gauss points (sum_b dN_b / dL_l is constant in l only to 1e-7), so with
    it the defect is the tables' distance: measured 1.8e-9 on box2-o2, bound 1e-6 as in test_tables_against_fp64_quadrature."""
    v, t, order = meshes[name]
    geo, _, ref = refs[name]
    x = _effective_positions(v, t, order)
    d64, m64 = R.tables_f64(order)
    r64 = R.assemble_from_geometry(geo, t, order, d64, RHO * m64, nv=v.shape[0])
    rigid64, sym64 = _rigid_defect(LAM * r64["Kl"] + MU * r64["Km"], x)
    rigid, sym = _rigid_defect(LAM * ref["Kl"] + MU * ref["Km"], x)
    # total mass
    w32 = fem_tables.gauss_rule(order)[1].astype(np.float64).sum()
    vol = geo[:, 12].sum() / 6
    mass = float(ref["Ms"].sum() / (RHO * vol * 6 * w32) - 1)
    mass64 = float(r64["Ms"].sum() / (RHO * vol) - 1)
    print(f"{name}: fp64 tables: symmetry {sym64:.2e} rigid {rigid64:.2e} total mass {mass64:.2e};  "
          f"project tables: symmetry {sym:.2e} rigid {rigid:.2e} total mass {mass:.2e}")
    assert sym64 <= 1e-14 and sym <= 1e-14
    assert rigid64 <= 1e-12
    assert rigid <= (1e-12 if order == 1 else 1e-6)
    assert abs(mass64) <= 1e-13
    assert abs(mass) < 1e-6  # the fp32 roundings of the partition of unity inside mass_table_f32
    assert np.abs(ref["Ms"] - ref["Ms"].T).max() <= 1e-6 * np.abs(ref["Ms"]).max()
    if order == 1:
        assert (ref["Ms"][ref["ncontrib"] > 0] > 0).all() and (ref["Ms"].sum(1) > 0).all()
    # off the pattern nothing, and the magnitudes dominate
    for k in ("Kl", "Km", "Ms"):
        assert (ref[k][ref["ncontrib"] == 0] == 0).all()
        assert (ref[k + "_mag"] >= np.abs(ref[k])).all()


# ---------------------------------------------------------------------------------------------------------------- oracle

@pytest.mark.parametrize("name", ["box2-o1", "box2-o2", "box3-o1"])
def test_matches_oracle(meshes, refs, name):
    """Within 2e-6 (relative to the largest entry) of the oracle's fp32-gradient assembly: the distance the GPU parity test
    allows.  Measured 5e-8 ... 1.2e-7."""
    v, t, order = meshes[name]
    _, _, ref = refs[name]
    nv = v.shape[0]
    d = fem.OracleDeform(torch.from_numpy(v), torch.from_numpy(t), order)
    dense = lambda A: A.transpose(0, 2, 1, 3).reshape(3 * nv, 3 * nv)
    el = _rel(dense(ref["Kl"]), fem.assemble_stiffness(d, 1.0, 0.0).toarray())
    em = _rel(dense(ref["Km"]), fem.assemble_stiffness(d, 0.0, 1.0).toarray())
    _, Ms = fem.assemble_mass(torch.from_numpy(v), torch.from_numpy(t), order, RHO)
    es = _rel(ref["Ms"], Ms.toarray())
    print(f"{name} against the oracle: K_lambda {el:.2e} K_mu {em:.2e} M_s {es:.2e}")
    assert el < 2e-6 and em < 2e-6 and es < 2e-6


# ---------------------------------------------------------------------------------------------------------------- invariances

@pytest.mark.parametrize("name", ["box2-o1", "box2-o2"])
def test_renumbering_permutes_exactly(meshes, refs, name):
    v, t, order = meshes[name]
    _, _, ref = refs[name]
    nv = v.shape[0]
    perm = np.random.default_rng(5).permutation(nv)  # new -> old
    inv = np.empty_like(perm)
    inv[perm] = np.arange(nv)
    geo, _ = R.tet_geometry_exact(v[perm], inv[t], order)
    r2 = R.assemble_from_geometry(geo, inv[t], order, fem_tables.stiffness_table(order), fem_tables.mass_table(order, RHO), nv=nv)
    for k in ("Kl", "Km", "Ms", "Kl_mag", "Km_mag", "Ms_mag", "ncontrib"):
        assert np.array_equal(r2[k], ref[k][perm][:, perm]), k


@pytest.mark.parametrize("name", ["box2-o1", "box2-o2", "box3-o1", "graded"])
def test_element_symmetry(meshes, refs, name):
    """Swapping v1 <-> v2 in the local order of every third tet (P2: slots 0<->2, 3<->5, 6<->7) flips det and relabels the element:
    the result is that of the unflipped tets with the tables relabelled on those tets (``flip_twin``), within 8 * 2^-53 * mag.
    With the SAME tables it is not - they are symmetric under the swap only to their fp32 rounding - except for the P1 stiffness
    table, which is: there the flipped mesh equals the unflipped one."""
    v, t, order = meshes[name]
    geo, _, ref = refs[name]
    dtab, mtab = fem_tables.stiffness_table(order), fem_tables.mass_table(order, RHO)
    tf = R.flip_tets(t, order)
    mask = R.flip_mask(t.shape[0])
    d0, d1 = R.signed_dets(v, t, order), R.signed_dets(v, tf, order)
    assert np.array_equal(d1[mask], -d0[mask]) and np.array_equal(d1[~mask], d0[~mask])
    assert (d1 < 0).any() and (d1 > 0).any()  # both orientations in one mesh
    gf, _ = R.tet_geometry_exact(v, tf, order)
    assert np.array_equal(gf[:, 12], geo[:, 12])
    rf = R.assemble_from_geometry(gf, tf, order, dtab, mtab, nv=v.shape[0])
    twin = R.flip_twin(geo, t, order, dtab, mtab, mask, nv=v.shape[0])
    bounds = {k: 8 * R.U53 * twin[k + "_mag"] for k in ("Kl", "Km", "Ms")}
    ratios = R.block_ratios(rf, twin, bounds)
    print(f"{name} flipped against its twin (units of 8 * 2^-53 * mag): {ratios}")
    assert all(r[0] <= 1 for r in ratios.values())
    s, p = list(R.FLIP_SLOTS[order]), [1, 0, 2, 3]
    asym_d = _rel(dtab[s][:, p][:, :, s][:, :, :, p], dtab)
    asym_m = _rel(mtab[s][:, s], mtab)
    print(f"order {order}: asymmetry of the tables under the swap: dtab {asym_d:.2e} mtab {asym_m:.2e}")
    if order == 1:
        assert asym_d == 0
        plain = R.block_ratios(rf, ref, bounds)
        assert plain["Kl"][0] <= 1 and plain["Km"][0] <= 1


# ---------------------------------------------------------------------------------------------------------------- sensitivity
# The GPU checks, run here on wrong copies of the reference's own output.

def _copy(ref):
    return {k: ref[k].copy() for k in ("Kl", "Km", "Ms")}


def _trips(got, ref, which=("Kl", "Km", "Ms")):
    r = R.block_ratios(got, ref)
    return {k: r[k][0] for k in which}


@pytest.mark.parametrize("name", ["box2-o1", "box2-o2", "graded"])
def test_bounds_pass_on_the_reference_itself(refs, name):
    _, _, ref = refs[name]
    assert max(_trips(_copy(ref), ref).values()) == 0


@pytest.mark.parametrize("name", ["box2-o1", "box2-o2", "graded"])
def test_transposed_block_trips_the_block_check(refs, name):
    """Check (b) on a copy whose one block is transposed - the least asymmetric off-diagonal block that is asymmetric at all, the
    case a max-norm product check would hide."""
    _, _, ref = refs[name]
    for k in ("Kl", "Km"):
        asym = np.abs(ref[k] - np.swapaxes(ref[k], -1, -2)).max(axis=(-1, -2)) / np.maximum(ref[k + "_mag"].max(axis=(-1, -2)), 1e-300)
        cand = np.where(asym > 1e-6, asym, np.inf)
        a, b = np.unravel_index(int(np.argmin(cand)), cand.shape)
        got = _copy(ref)
        got[k][a, b] = got[k][a, b].T.copy()
        r = R.block_ratios(got, ref)[k]
        print(f"{name} {k}: block ({a}, {b}) transposed -> err / bound {r[0]:.2e} at {r[1]}")
        assert r[0] > 1e3 and r[1][:2] == (a, b)


@pytest.mark.parametrize("name", ["box2-o1", "box2-o2", "graded"])
def test_dropped_contribution_trips_the_block_check(meshes, refs, name):
    """Check (b) on a copy in which the slots of the last tet lost their last contribution (that tet's)."""
    v, t, order = meshes[name]
    geo, _, ref = refs[name]
    got = R.assemble_from_geometry(geo[:-1], t[:-1], order, fem_tables.stiffness_table(order), fem_tables.mass_table(order, RHO),
                                   nv=v.shape[0])
    bounds = R.block_bounds(ref)
    touched = np.zeros_like(ref["ncontrib"], dtype=bool)
    touched[np.ix_(t[-1], t[-1])] = True
    for k in ("Kl", "Km", "Ms"):
        err = np.abs(got[k] - ref[k])
        bad = err > bounds[k]
        blocks = bad if k == "Ms" else bad.any(axis=(-1, -2))
        assert blocks[touched].all(), k      # every slot of the last tet is caught
        assert not blocks[~touched].any(), k  # and no other
    # the smallest of the missing contributions, relative to the bound
    r = np.abs(got["Ms"] - ref["Ms"])[touched] / bounds["Ms"][touched]
    print(f"{name}: dropped contribution, smallest err / bound over the tet's slots of M_s {r.min():.2e}")
    assert r.min() > 1e3


@pytest.mark.parametrize("name", ["box2-o1", "box2-o2", "graded"])
def test_zeroed_last_slot_trips_the_block_check(refs, name):
    """Check (b) on a copy whose slot nnzb - 1 (last column of the last pattern row) is zero."""
    _, _, ref = refs[name]
    nz = np.argwhere(ref["ncontrib"] > 0)
    a, b = nz[-1]  # row-major order = pattern order
    got = _copy(ref)
    for k in got:
        got[k][a, b] = 0
    r = R.block_ratios(got, ref)
    print(f"{name}: slot ({a}, {b}) zeroed -> {r}")
    assert all(r[k][0] > 1e3 and r[k][1][:2] == (a, b) for k in r)


@pytest.mark.parametrize("name", ["box2-o2", "box3-o1"])
def test_signed_det_trips_the_flip_check(meshes, refs, name):
    """Check (d) - the flipped mesh against its twin within the sum of their block bounds and the allowance for their different
    geometry roundings - on a flipped assembly that integrates with det in the place of |det|."""
    v, t, order = meshes[name]
    geo, _, _ = refs[name]
    dtab, mtab = fem_tables.stiffness_table(order), fem_tables.mass_table(order, RHO)
    tf, mask = R.flip_tets(t, order), R.flip_mask(t.shape[0])
    gf, _ = R.tet_geometry_exact(v, tf, order)
    twin = R.flip_twin(geo, t, order, dtab, mtab, mask, nv=v.shape[0])
    good = R.assemble_from_geometry(gf, tf, order, dtab, mtab, nv=v.shape[0])
    bt, bg = R.block_bounds(twin), R.block_bounds(good)
    gb = refs[name][1]
    allow = R.flip_geometry_allowance((geo, gb, t), (gf, R.tet_geometry_exact(v, tf, order)[1], tf), order, dtab, mtab, mask,
                                      v.shape[0])
    bounds = {k: bt[k] + bg[k] + allow[k] for k in bt}
    assert max(r[0] for r in R.block_ratios(good, twin, bounds).values()) <= 1
    gs = gf.copy()
    gs[:, 12] = R.signed_dets(v, tf, order)
    wrong = R.assemble_from_geometry(gs, tf, order, dtab, mtab, nv=v.shape[0])
    r = R.block_ratios(wrong, twin, bounds)
    print(f"{name}: det for |det| -> {r}")
    assert all(x[0] > 1e3 for x in r.values())
