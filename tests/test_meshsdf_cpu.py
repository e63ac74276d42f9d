"""Mesh signed distance, the parts that need no GPU: an fp64 NumPy restatement of the formulas (the oracle of the GPU
tests and of tests/golden/make_golden_meshsdf.py), the .obj reader and writer, input validation and the drop-in
module names."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden

CASES = ("frog", "turtle", "spot")
FACE_COUNTS = {"frog": 348, "turtle": 366, "spot": 4588}


# ---------------------------------------------------------------------------------------------- fp64 restatement
def _dot(a, b):
    return (a * b).sum(-1)


def point_triangle_sqdist(p, a, b, c):
    """Squared distance from points p (P, 1, 3) to triangles a, b, c (1, F, 3) by the Voronoi regions of the triangle
    (Ericson, Real-Time Collision Detection, 5.1.5), fp64.  Divisions are guarded, but the regions of a zero-area
    triangle are not meaningful: ``restatement`` takes those from ``segment_sqdist``."""
    ab, ac, ap = b - a, c - a, p - a
    d1, d2 = _dot(ab, ap), _dot(ac, ap)
    bp = p - b
    d3, d4 = _dot(ab, bp), _dot(ac, bp)
    cp = p - c
    d5, d6 = _dot(ab, cp), _dot(ac, cp)
    vc = d1 * d4 - d3 * d2
    vb = d5 * d2 - d1 * d6
    va = d3 * d6 - d5 * d4

    def safe(num, den):
        return np.where(den != 0, num / np.where(den != 0, den, 1.0), 0.0)

    with np.errstate(invalid="ignore", divide="ignore"):
        t_ab = safe(d1, d1 - d3)
        t_ac = safe(d2, d2 - d6)
        t_bc = safe(d4 - d3, (d4 - d3) + (d5 - d6))
        den = va + vb + vc
        v, w = safe(vb, den), safe(vc, den)
    conds = [
        (d1 <= 0) & (d2 <= 0),
        (d3 >= 0) & (d4 <= d3),
        (vc <= 0) & (d1 >= 0) & (d3 <= 0),
        (d6 >= 0) & (d5 <= d6),
        (vb <= 0) & (d2 >= 0) & (d6 <= 0),
        (va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0),
    ]
    ones = np.ones(np.broadcast(p[..., :1], a[..., :1]).shape)
    cands = [
        a * ones,
        b * ones,
        a + t_ab[..., None] * ab,
        c * ones,
        a + t_ac[..., None] * ac,
        b + t_bc[..., None] * (c - b),
    ]
    q = a + v[..., None] * ab + w[..., None] * ac
    for cond, cand in zip(reversed(conds), reversed(cands)):  # the first true condition wins
        q = np.where(cond[..., None], cand, q)
    return _dot(p - q, p - q)


def segment_sqdist(p, u, v):
    """Squared distance from points p to the segments u -> v (a point when u == v), fp64."""
    d = v - u
    dd = _dot(d, d)
    t = np.clip(_dot(p - u, d) / np.where(dd > 0, dd, 1.0), 0.0, 1.0)
    q = u + t[..., None] * d
    return _dot(p - q, p - q)


def solid_angle_half(p, a, b, c):
    """atan2 form of Van Oosterom and Strackee (1983): half the signed solid angle of the triangle seen from p."""
    A, B, C = a - p, b - p, c - p
    la, lb, lc = np.sqrt(_dot(A, A)), np.sqrt(_dot(B, B)), np.sqrt(_dot(C, C))
    det = _dot(A, np.cross(B, C))
    den = la * lb * lc + _dot(A, B) * lc + _dot(A, C) * lb + _dot(B, C) * la
    area2 = np.cross(b - a, c - a)
    has_area = _dot(area2, area2) > 0
    return np.where(has_area, np.arctan2(det, den), 0.0)


def restatement(points, vertices, faces, max_pairs=1 << 21):
    """(unsigned distance, winding number, closest face) in fp64, lowest face index on equal squared distances."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    v = np.asarray(vertices, dtype=np.float64)
    f = np.asarray(faces, dtype=np.int64)
    a, b, c = v[f[:, 0]][None], v[f[:, 1]][None], v[f[:, 2]][None]
    dist, wind, face = np.empty(len(p)), np.empty(len(p)), np.empty(len(p), dtype=np.int64)
    n = np.cross(b - a, c - a)[0]
    flat = np.nonzero(_dot(n, n) == 0)[0]  # zero-area faces: the nearest of their three segments
    step = max(1, max_pairs // len(f))
    for s in range(0, len(p), step):
        q = p[s:s + step, None, :]
        d2 = point_triangle_sqdist(q, a, b, c)
        if len(flat):
            fa, fb, fc = a[:, flat], b[:, flat], c[:, flat]
            d2[:, flat] = np.minimum(np.minimum(segment_sqdist(q, fa, fb), segment_sqdist(q, fb, fc)),
                                     segment_sqdist(q, fc, fa))
        face[s:s + step] = d2.argmin(1)  # argmin returns the first minimum
        dist[s:s + step] = np.sqrt(d2.min(1))
        wind[s:s + step] = solid_angle_half(q, a, b, c).sum(1) / (2 * np.pi)
    return dist, wind, face


def signed_from(dist, wind):
    return np.where(wind > 0.5, -dist, dist)


def box_mesh(lo, hi):
    """An axis-aligned box as 12 outward-wound triangles."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    v = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    f = np.array([t for q in quads for t in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))], dtype=np.int64)
    return v, f


def box_sdf(points, lo, hi):
    """Analytic signed distance of the box, negative inside."""
    p = np.asarray(points, dtype=np.float64)
    centre, half = (np.asarray(lo) + np.asarray(hi)) / 2.0, (np.asarray(hi) - np.asarray(lo)) / 2.0
    q = np.abs(p - centre) - half
    return np.sqrt((np.maximum(q, 0.0) ** 2).sum(-1)) + np.minimum(q.max(-1), 0.0)


def box_points(seed=0, n=3000):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1.0, 1.0, size=(n, 3))


BOX = ((-0.4, -0.25, -0.6), (0.5, 0.35, 0.3))


# ---------------------------------------------------------------------------------------------- restatement checks
def test_restatement_matches_the_analytic_box():
    v, f = box_mesh(*BOX)
    assert f.shape == (12, 3)
    p = box_points()
    dist, wind, _ = restatement(p, v, f)
    assert np.abs(wind - np.round(wind)).max() < 1e-12 and set(np.round(wind)) == {0.0, 1.0}
    err = np.abs(signed_from(dist, wind) - box_sdf(p, *BOX)).max()
    print("restatement vs analytic box: max abs err", err)
    assert err < 1e-14


def test_restatement_handles_a_zero_area_face():
    v, f = box_mesh(*BOX)
    p = box_points(1, 500)
    d0, w0, _ = restatement(p, v, f)
    for extra in ([f[0, 0], f[0, 0], f[0, 1]], [f[0, 1], f[0, 2], f[0, 2]], [f[0, 0], f[0, 0], f[0, 0]]):
        d1, w1, _ = restatement(p, v, np.vstack([f, [extra]]))
        assert np.isfinite(d1).all() and np.isfinite(w1).all()
        assert np.abs(d0 - d1).max() < 1e-15 and np.array_equal(w0, w1)


@pytest.mark.parametrize("case", CASES)
def test_restatement_matches_the_fixture(case):
    g = load_golden("g11_meshsdf.npz")
    v, f, p = g[f"{case}_vertices"], g[f"{case}_faces"], g[f"{case}_points"]
    assert v.dtype == np.float32 and p.dtype == np.float32 and f.shape == (FACE_COUNTS[case], 3)
    dist, wind, face = restatement(p, v, f)
    assert np.abs(dist - g[f"{case}_unsigned"]).max() < 1e-13
    assert np.abs(wind - g[f"{case}_winding"]).max() < 1e-12
    same = face == g[f"{case}_face"]
    # BLAS-free NumPy sums are reproducible; allow a different face only where the two are equidistant
    assert same.all() or np.abs(dist[~same] - g[f"{case}_unsigned"][~same]).max() < 1e-13
    # what the generator asserted when it wrote the case
    assert np.abs(wind - np.round(wind)).max() < 1e-9
    assert (dist < 1e-5).mean() <= 0.01


# ---------------------------------------------------------------------------------------------- .obj files
OBJ_TEXT = """\
# a comment
mtllib ignored.mtl
o thing
v 0 0 0
v 1 0 0
v 1 1 0 0.5
v 0 1 0
vt 0.5 0.5
vn 0 0 1
v 0 0 1
s off
f 1 2 3
f 1/1 3/1 4/1
f 1//1 2//1 5//1
f 2/1/1 3/1/1 5/1/1
f 1 2 3 4
f -1 -2 -3
g group
l 1 2
"""


def test_read_obj_forms(tmp_path):
    from diffsound_amd.meshsdf import read_obj

    path = tmp_path / "t.obj"
    path.write_text(OBJ_TEXT)
    v, f = read_obj(str(path))
    assert v.dtype == np.float32 and f.dtype == np.int64
    assert np.array_equal(v, np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0, 0, 1]], dtype=np.float32))
    assert f.tolist() == [[0, 1, 2], [0, 2, 3], [0, 1, 4], [1, 2, 4], [0, 1, 2], [0, 2, 3], [4, 3, 2]]


def test_read_obj_negative_indices_count_from_the_vertices_read_so_far(tmp_path):
    from diffsound_amd.meshsdf import read_obj

    path = tmp_path / "t.obj"
    path.write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nf -3 -2 -1\nv 0 0 1\nf -1 -2 -3\n")
    _, f = read_obj(str(path))
    assert f.tolist() == [[0, 1, 2], [3, 2, 1]]


def test_read_obj_rejects_a_bad_index(tmp_path):
    from diffsound_amd.meshsdf import read_obj

    path = tmp_path / "t.obj"
    path.write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 4\n")
    with pytest.raises(ValueError):
        read_obj(str(path))


@pytest.mark.parametrize("case", CASES)
def test_read_obj_on_the_fixture_meshes(case, tmp_path):
    """The fixture's meshes (read from the reference's files by the generator's own parser) keep their face counts
    and survive write_obj -> read_obj bit for bit."""
    from diffsound_amd.meshsdf import read_obj, write_obj

    g = load_golden("g11_meshsdf.npz")
    v, f = g[f"{case}_vertices"], g[f"{case}_faces"]
    assert len(f) == FACE_COUNTS[case]
    path = tmp_path / f"{case}.obj"
    write_obj(str(path), v, f)
    v2, f2 = read_obj(str(path))
    assert np.array_equal(v2, v) and np.array_equal(f2, f)


def test_write_obj_round_trip_from_torch(tmp_path):
    from diffsound_amd.meshsdf import read_obj, write_obj

    rng = np.random.default_rng(3)
    v = torch.from_numpy(rng.standard_normal((20, 3)).astype(np.float32) * 1e3)
    f = torch.from_numpy(rng.integers(0, 20, size=(30, 3)))
    write_obj(str(tmp_path / "r.obj"), v, f)
    v2, f2 = read_obj(str(tmp_path / "r.obj"))
    assert np.array_equal(v2, v.numpy()) and np.array_equal(f2, f.numpy())


# ---------------------------------------------------------------------------------------------- validation
def _good():
    v, f = box_mesh(*BOX)
    return torch.from_numpy(v).float(), torch.from_numpy(f), torch.zeros(4, 3)


@pytest.mark.parametrize("kind", ["vertex_shape", "vertex_dtype", "face_shape", "face_dtype", "face_high", "face_negative",
                                  "vertex_nan", "vertex_inf", "no_faces", "no_vertices", "point_shape", "point_scalar",
                                  "point_nan", "point_dtype"])
def test_bad_input_raises_value_error_without_a_device(kind):
    from diffsound_amd import meshsdf

    v, f, p = _good()
    if kind == "vertex_shape":
        v = v[:, :2]
    elif kind == "vertex_dtype":
        v = v.long()
    elif kind == "face_shape":
        f = torch.cat([f, f[:, :1]], dim=1)
    elif kind == "face_dtype":
        f = f.float()
    elif kind == "face_high":
        f = f.clone()
        f[3, 1] = len(v)
    elif kind == "face_negative":
        f = f.clone()
        f[0, 0] = -1
    elif kind == "vertex_nan":
        v = v.clone()
        v[2, 1] = float("nan")
    elif kind == "vertex_inf":
        v = v.clone()
        v[0, 0] = float("inf")
    elif kind == "no_faces":
        f = f[:0]
    elif kind == "no_vertices":
        v, f = v[:0], f[:0]
    elif kind == "point_shape":
        p = torch.zeros(4, 2)
    elif kind == "point_scalar":
        p = torch.tensor(1.0)
    elif kind == "point_nan":
        p = p.clone()
        p[1, 2] = float("nan")
    elif kind == "point_dtype":
        p = p.long()
    with pytest.raises(ValueError):
        meshsdf.signed_distance(p, v, f)
    with pytest.raises(ValueError):  # numpy input takes the same checks
        meshsdf.signed_distance(p.numpy(), v.numpy(), f.numpy())


# ---------------------------------------------------------------------------------------------- drop-in names
def test_src_aliases_are_this_projects_classes():
    code = textwrap.dedent("""
        import src.dmtet.geometry.dmtet_thickness as th
        import src.dmtet.geometry.dmtet_interpolate as ip
        import diffsound_amd.dmtet as d
        assert th.DMTetGeometry is d.DMTetThicknessGeometry and th.DMTet is d.DMTetThickness
        assert ip.DMTetGeometry is d.DMTetInterpolateGeometry and ip.DMTet is d.DMTetInterpolate
        assert th.DMTetGeometry.__module__ == ip.DMTetGeometry.__module__ == "diffsound_amd.dmtet"
        for name in ("generate_edges", "getAABB", "getMesh", "get_largest_connected_component", "tick", "apply_sdf",
                     "parameters", "get_eigenvalues", "get_thickness"):
            assert callable(getattr(th.DMTetGeometry, name)) and callable(getattr(ip.DMTetGeometry, name)), name
        assert callable(ip.DMTetGeometry.apply_sdf2) and callable(ip.DMTetGeometry.init_coef)
    """)
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT))


def test_top_level_geometry_package_is_ours_and_the_rest_falls_through(tmp_path):
    """The thickness and morphing scripts do ``sys.path.append("src/dmtet/")`` and import the top-level packages
    ``geometry`` and ``render``.  With this tree's src/dmtet and root in front of a second tree, geometry.dmtet_thickness
    and geometry.dmtet_interpolate are ours; geometry.sdf and render come from the second tree."""
    second = tmp_path / "src" / "dmtet"
    (second / "geometry").mkdir(parents=True)
    (second / "render").mkdir()
    (tmp_path / "src" / "__init__.py").write_text("")
    (second / "geometry" / "sdf.py").write_text("WHOSE = 'second'\n")
    (second / "geometry" / "dmtet_thickness.py").write_text("raise ImportError('the second tree was imported')\n")
    (second / "render" / "__init__.py").write_text("")
    (second / "render" / "obj.py").write_text("WHOSE = 'second'\n")
    code = textwrap.dedent(f"""
        import sys
        sys.path.append("src/dmtet/")  # what the scripts do, from the second tree's root
        import geometry.dmtet_thickness as th
        import geometry.dmtet_interpolate as ip
        import geometry.sdf as sdf
        from render import obj
        assert th.__file__.startswith({ROOT!r}) and ip.__file__.startswith({ROOT!r}), (th.__file__, ip.__file__)
        assert th.DMTetGeometry.__module__ == ip.DMTetGeometry.__module__ == "diffsound_amd.dmtet"
        assert sdf.WHOSE == "second" and sdf.__file__.startswith({str(tmp_path)!r})
        assert obj.WHOSE == "second" and obj.__file__.startswith({str(tmp_path)!r})
    """)
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "src", "dmtet"), ROOT]))
    subprocess.run([sys.executable, "-c", code], check=True, cwd=str(tmp_path), env=env)
