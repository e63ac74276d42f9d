"""tests/_bem_ref.py without a device, on every case of tests/test_bem_kernels_gpu.py: the per-entry scales bound the
entries they scale, no pair and no point sits in the borderline band of the near threshold, the fp64 restatement gives
the values it gave before it learnt to run in fp32 too, the fp32 run stays fp32 throughout, and the potential points hit
the branches they are there for."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _bem_ref as R  # noqa: E402

CASES = R.CASES_A + R.CASES_B + [("C", R.C_K, False)]
IDS = [R.case_id(c) for c in CASES]

# V[0, m-1], A[0, 1], A[m/2, m/3], rhs[m/2] and (cases A, B) the potential at points 0 and 200, as the fp64 functions of
# tests/test_bem_cpu.py gave them before they moved to _bem_ref.py (faces in internal_order, coefficients(m, 3), case C
# with 257 faces).  The moved functions gave the same bits on the machine that recorded these; the comparison below
# allows 1e-12 of the entry's scale, for another machine's exp, log and matrix product.
RECORDED = {
    "A-k0": [(1.1547824867691575e-06+0j), (-3.788469242834614e-05+0j), (-4.964359964577779e-06+0j), (-3.3031634949504076e-05-1.0410063051098317e-05j), (0.018150839339953352+0.016295291530670074j), (-0.08665536853200936-0.32798529953217836j)],
    "A-k1": [(1.1343231493890726e-06+2.1640383008099136e-07j), (-3.789749392438821e-05-3.373896774753592e-10j), (-5.030653028734792e-06-7.306417146549642e-09j), (-3.3718889443043e-05-1.1428680779579287e-05j), (0.018573486899860405+0.017016183711456197j), (-0.0864566384081312-0.3281018420477848j)],
    "A-k30": [(9.336364260864965e-07-6.776279122942397e-07j), (-4.536560326870571e-05-7.458020345677927e-06j), (2.2106538423041647e-05+9.718173224496647e-06j), (2.962813041325269e-06-4.786286828633156e-05j), (-0.13629106465280205-0.012926219355655655j), (-0.13075385518247315-0.0477350537529916j)],
    "A-k300": [(1.0504459000284844e-06-1.8246841876062457e-08j), (-4.241762619175626e-06-1.0649024556469699e-05j), (-3.3171629167594785e-06+8.692369656065602e-06j), (7.180439698890286e-06-4.244072917883537e-07j), (-0.09791228878576937+0.1707814687923624j), (-0.29600502371557524+0.16433942118502257j)],
    "A-k500": [(9.092136281022883e-07-7.7982704688973e-08j), (-5.431320497720014e-06+6.562022483489234e-06j), (-4.0894894638651076e-05+4.6463690191024635e-06j), (5.441909121076989e-06+2.0489929263026344e-06j), (0.01386817775027769+0.7295415931236043j), (-0.12506040710267008+0.5408751876588865j)],
    "A-k300-shifted": [(1.0504456950954733e-06-1.8251817740930816e-08j), (-4.241774216318938e-06-1.0649077332995675e-05j), (-3.317133985991839e-06+8.692351992121334e-06j), (7.180423998874577e-06-4.244289221391075e-07j), (-0.09791236570822673+0.17078168194458268j), (-0.29601195918638507+0.16432768995258565j)],
    "B-k0": [(3.296228480625449e-07+0j), (-2.5493988616486887e-05+0j), (-5.466209705409797e-08+0j), (1.920136469396445e-07+3.168835719156411e-07j), (0.0010953824350276727-0.01188804356944092j), (0.0008575653701547392-0.004465647655120093j)],
    "B-k30": [(1.6004966131578113e-07+2.5412839626651936e-07j), (-2.583759606683724e-05-8.157595943137314e-08j), (-7.656624204059535e-08-2.3472518493116873e-08j), (1.967352699161827e-07+3.700108845397092e-07j), (0.04406008232918116+0.0230836288547154j), (0.015387675636942646+0.002412132246981934j)],
    "B-k300": [(4.80128493588138e-10-1.379198513693575e-08j), (-2.291152397721956e-05-1.5500929941170067e-05j), (-7.629912403616113e-08-3.879330709598344e-08j), (-2.5546735759775527e-07-2.6582480249985363e-08j), (-0.08061310281083171-0.12877033040096733j), (-0.006121647273648071+0.00018481474244628457j)],
    "C-k30": [(-9.036434374638772e-09-8.47249492205647e-08j), (-3.661642776962795e-06-7.216267398909887e-07j), (-1.0130731623567071e-06-1.4117775042969049e-06j), (3.443947260566389e-06+3.850904270804031e-06j)],
}


@functools.lru_cache(maxsize=None)
def _truth(i):
    name, k, shifted = CASES[i]
    v, f = R.mesh(name, shifted)
    f = f[R.internal_order(v, f)]
    if name == "C":
        f = f[:max(R.C_SIZES)]
    gv, uv = R.coefficients(len(f), 3)
    return v, f, gv, uv, R.assembly_truth(v, f, k, gv)


@functools.lru_cache(maxsize=None)
def _points(i):
    v, f, gv, uv, t = _truth(i)
    k = CASES[i][1]
    pts, kinds = R.potential_points(t["g"], k)
    d2, t2 = R._point_d2_t2(t["g"], pts)
    return pts, kinds, d2 < t2


def test_mesh_sizes():
    assert len(R.mesh("A")[1]) == 80 and len(R.mesh("B")[1]) == 48 and len(R.mesh("C")[1]) == 320
    v, f = R.mesh("B")
    assert np.allclose(v.max(0) - v.min(0), R.PLATE)
    va, vs = R.mesh("A")[0], R.mesh("A", True)[0]
    assert np.abs(vs.astype(np.float64) - va - np.array(R.SHIFT)).max() <= 2.0 ** -24 * 1.2


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_scales_bound_their_entries_and_no_pair_is_borderline(i):
    *_, t = _truth(i)
    assert t["skip"].sum() == 0
    assert np.all(np.abs(t["V"]) <= t["sV"] * (1 + 1e-12))
    assert np.all(np.abs(t["K"]) <= t["sK"] * (1 + 1e-12))
    assert np.all(t["sV"] > 0) and np.all(t["sK"] > 0)
    assert t["near"].sum() > 0 and np.all(np.diag(t["near"]))
    assert (~t["near"]).sum() > 0  # both categories are met
    assert np.all(np.diag(t["K"]) == 0)


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_fp64_values_are_the_recorded_ones(i):
    v, f, gv, uv, t = _truth(i)
    m, k = len(f), CASES[i][1]
    got = [t["V"][0, m - 1], t["A"][0, 1], t["A"][m // 2, m // 3], t["rhs"][m // 2]]
    scale = [t["sV"][0, m - 1], t["sK"][0, 1], t["sK"][m // 2, m // 3], t["srhs"][m // 2]]
    if CASES[i][0] != "C":
        pts, kinds, near = _points(i)
        p = R.potential(t["g"], k, gv, uv, pts)
        s = R.point_scales(t["g"], k, pts, gv, uv, near)
        got += [p[0], p[200]]
        scale += [s[0], s[200]]
    for a, b, s in zip(got, RECORDED[IDS[i]], scale):
        assert abs(a - b) <= 1e-12 * s, (a, b)


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_fp32_run_stays_fp32_and_close(i):
    v, f, gv, uv, t = _truth(i)
    g32 = R.geometry(v, f, np.float32)
    assert all(a.dtype == np.float32 for a in g32.values())
    assert t["V32"].dtype == np.complex64 and t["K32"].dtype == np.complex64 and t["rhs32"].dtype == np.complex64
    x = g32["q"][:4, 0] + np.float32(0.01)
    s1, dl = R.static_integrals(x, g32["P"][:4], g32["n"][:4])
    vi, ki = R.near_inner(x, g32, np.arange(4), CASES[i][1], np.zeros(4, bool))
    assert s1.dtype == np.float32 and dl.dtype == np.float32 and vi.dtype == np.complex64 and ki.dtype == np.complex64
    assert all(a.dtype == np.float32 for a in R.rule6(np.float32) + R.split_rule(2, np.float32))
    # the level is a rounding level, not a disagreement: far below the 1e-3 that separates the quadrature rules
    lev = R.assembly_levels(t)
    print("LEVEL", IDS[i], " ".join(f"{q}/{c} {x:.3g}" for (q, c), x in lev.items()),
          f"rhs {R.worst(t['rhs32'], t['rhs'], t['srhs']):.3g}")
    assert 0 < max(lev.values()) < 1e-4, lev


@pytest.mark.parametrize("i", range(len(R.CASES_A + R.CASES_B)), ids=IDS[:-1])
def test_potential_points(i):
    v, f, gv, uv, t = _truth(i)
    k, g = CASES[i][1], t["g"]
    pts, kinds, near = _points(i)
    assert pts.shape == (257, 3) and np.array_equal(pts, pts.astype(np.float32).astype(np.float64))
    assert R.borderline_points(g, pts).sum() == 0
    want = {"offset", "skin", "edge-line", "in-plane"} | ({"far"} if k * 2 * R.RADIUS <= 100 else set())
    assert set(kinds) >= want, set(kinds)
    assert R.point_triangle_distance(pts, g["P"]).min() > 2e-4 * g["h"].min()  # off the surface
    for kind in ("skin", "edge-line", "in-plane"):
        assert near[kinds == kind].any(1).all(), kind  # each of them meets the closed forms
    far = np.linalg.norm(pts[kinds == "far"] - 0.5 * (v.min(0) + v.max(0)), axis=1)
    assert np.all(k * far <= 100 * (1 + 1e-6))
    p64 = R.potential(g, k, gv, uv, pts)
    s = R.point_scales(g, k, pts, gv, uv, near)
    assert np.all(np.abs(p64) <= s * (1 + 1e-12)) and np.all(s > 0)
    if CASES[i][0] == "B":  # axis-aligned faces: points exactly in a face's plane and exactly on an edge's line
        g32 = R.geometry(v, f, np.float32)
        x = pts.astype(np.float32)
        p, j = np.nonzero(near & np.isin(kinds, ("edge-line", "in-plane"))[:, None])
        a = g32["P"][j] - x[p][:, None, :]
        w = (g32["n"][j] * a[:, 0]).sum(1)
        assert (w == 0).sum() >= 10  # the aw == 0 branch
        d = a[:, 1] - a[:, 0]
        sdir = d / np.linalg.norm(d, axis=1, keepdims=True)
        t0 = (np.cross(sdir, g32["n"][j]) * a[:, 0]).sum(1)
        assert (t0 == 0).sum() >= 1  # the |t0| <= 1e-30 branch


def test_point_triangle_distance():
    P = np.array([[[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]])
    x = np.array([[0.2, 0.2, 0.5], [2.0, 0.0, 0.0], [-1.0, -1.0, 0.0], [0.5, -0.3, 0.4], [1.0, 1.0, 0.0]])
    want = [0.5, 1.0, np.sqrt(2.0), 0.5, np.sqrt(0.5)]
    assert np.allclose(R.point_triangle_distance(x, P)[:, 0], want, atol=1e-14)


def test_record_bounds_hold_for_the_fp32_restatement():
    """The counted bounds of ds_bem_geometry's record, tried on NumPy's fp32 geometry (another evaluation order of the
    same operations)."""
    for name, shifted in (("A", False), ("A", True), ("B", False), ("C", False)):
        v, f = R.mesh(name, shifted)
        g = R.geometry(v, f)
        rec32 = R.face_records(R.geometry(v, f, np.float32))
        err = np.abs(rec32 - R.face_records(g))
        b = R.record_bounds(g)
        assert np.all(err <= b), (name, shifted, (err / np.where(b > 0, b, 1))[b > 0].max())
        assert np.all(err[:, 32:] == 0)
