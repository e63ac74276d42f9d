"""Mesh signed distance on the device (csrc/meshsdf.hip through diffsound_amd/meshsdf.py) against the fp64 restatement
of tests/test_meshsdf_cpu.py (tests/golden/g11_meshsdf.npz) and the analytic box, its launch shapes and determinism,
and the thickness / morphing geometry classes end to end.

DIST_TOL is 4x the largest absolute error of the kernel's distance against the fp64 restatement measured on the three
fixture cases and the box (profiles/meshsdf_bench.json): MEASURED_MAX_ERR below."""
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_meshsdf_cpu as ref  # noqa: E402
from conftest import load_golden  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
MEASURED_MAX_ERR = 1.217e-7
DIST_TOL = 4 * MEASURED_MAX_ERR
BAND = 1e-5  # points closer than this to the surface are left out of the sign check, at most 1 % of a case
EIG_RTOL = 2e-4  # two solves of one pencil: smoke() holds each within 1e-4 of the exact eigenvalues


@pytest.fixture(scope="module")
def g11():
    return load_golden("g11_meshsdf.npz")


def _query(v, f, p, **kw):
    from diffsound_amd.meshsdf import MeshDistance

    out = MeshDistance(v, f).query(p, unsigned=True, face=True, winding=True, **kw)
    return {k: t.cpu().numpy() for k, t in out.items()}


def _face_distance(p, v, f, face):
    """fp64 distance from each point to the one face the kernel named."""
    v = np.asarray(v, np.float64)
    t = np.asarray(f)[face]
    q = np.asarray(p, np.float64).reshape(-1, 1, 3)
    a, b, c = (v[t[:, k]][:, None, :] for k in range(3))
    return np.sqrt(ref.point_triangle_sqdist(q, a, b, c)[:, 0])


def _check(out, p, v, f, dist, wind, face, what, watertight=True):
    err = np.abs(out["unsigned"] - dist).max()
    print(f"{what}: P={len(dist)} F={len(f)} max |d - d64| = {err:.3e} (tol {DIST_TOL:.3e})")
    assert np.isfinite(out["signed"]).all() and np.isfinite(out["winding"]).all()
    assert err <= DIST_TOL, (what, err)
    assert np.array_equal(np.abs(out["signed"]), out["unsigned"])
    far = dist > BAND
    assert (~far).mean() <= 0.01, (what, (~far).mean())
    if watertight:
        wdev = np.abs(out["winding"] - np.round(wind)).max()
        print(f"{what}: max winding deviation {wdev:.3e}")
        assert wdev <= 1e-3, (what, wdev)
        assert np.array_equal((out["signed"] < 0)[far], (wind > 0.5)[far]), what
    else:
        assert np.abs(out["winding"] - wind).max() <= 1e-4, what
        sure = far & (np.abs(wind - 0.5) > 1e-3)
        assert np.array_equal((out["signed"] < 0)[sure], (wind > 0.5)[sure]), what
    other = out["face"] != face
    assert (out["face"] >= 0).all() and (out["face"] < len(f)).all()
    if other.any():
        dface = _face_distance(p.reshape(-1, 3)[other], v, f, out["face"][other])
        assert np.abs(dface - dist[other]).max() <= DIST_TOL, (what, np.abs(dface - dist[other]).max())


@pytest.mark.parametrize("case", ref.CASES)
def test_kernel_matches_the_fixture(g11, case):
    v, f, p = g11[f"{case}_vertices"], g11[f"{case}_faces"], g11[f"{case}_points"]
    out = _query(v, f, p)
    _check(out, p, v, f, g11[f"{case}_unsigned"], g11[f"{case}_winding"], g11[f"{case}_face"], case)


@pytest.mark.parametrize("case", ref.CASES)
def test_signed_distance_matches_open3d(g11, case):
    key = f"{case}_open3d_signed"
    if key not in g11.files:
        pytest.skip("open3d was not installed where g11_meshsdf.npz was generated: the fixture has no open3d output")
    from diffsound_amd.meshsdf import signed_distance

    got = signed_distance(g11[f"{case}_points"], g11[f"{case}_vertices"], g11[f"{case}_faces"]).cpu().numpy()
    far = g11[f"{case}_unsigned"] > BAND
    # open3d's distance is fp32 too: its own error is of the order of ours
    assert np.abs(got - g11[key])[far].max() <= 2 * DIST_TOL
    assert np.array_equal((got < 0)[far], (g11[key] < 0)[far])


def _box32():
    v, f = ref.box_mesh(*ref.BOX)
    v = v.astype(np.float32)
    return v, f, v.min(0).astype(np.float64), v.max(0).astype(np.float64)


def test_kernel_matches_the_analytic_box():
    v, f, lo, hi = _box32()
    p = ref.box_points().astype(np.float32)
    out = _query(v, f, p)
    sdf = ref.box_sdf(p, lo, hi)
    dist, wind, face = ref.restatement(p, v, f)
    assert np.abs(ref.signed_from(dist, wind) - sdf).max() < 1e-14
    _check(out, p, v, f, dist, wind, face, "box")
    err = np.abs(out["signed"] - sdf)[np.abs(sdf) > BAND].max()
    print(f"box: max |sdf - analytic| = {err:.3e}")
    assert err <= DIST_TOL


@pytest.mark.parametrize("F", [1, 127, 128, 129])
def test_shapes_that_cross_the_tiling(g11, F):
    from diffsound_amd.meshsdf import TILE, MeshDistance

    assert TILE == 128
    v, f = g11["spot_vertices"], g11["spot_faces"][:F]  # an open patch: the winding number is a fraction
    md = MeshDistance(v, f)
    pts = g11["spot_points"]
    for P in (1, 63, 64, 65, 127, 128, 129):
        p = pts[1000:1000 + P]
        dist, wind, face = ref.restatement(p, v, f)
        for split in (False, True):
            out = {k: t.cpu().numpy() for k, t in md.query(p, unsigned=True, face=True, winding=True, split=split).items()}
            assert out["signed"].shape == (P,)
            _check(out, p, v, f, dist, wind, face, f"F={F} P={P} split={split}", watertight=False)


@pytest.mark.parametrize("case", ["frog", "spot"])
def test_split_and_single_launch_agree_bit_for_bit(g11, case):
    from diffsound_amd.meshsdf import MeshDistance

    md = MeshDistance(g11[f"{case}_vertices"], g11[f"{case}_faces"])
    p = g11[f"{case}_points"]
    one = md.query(p, unsigned=True, face=True, winding=True, split=False)
    two = md.query(p, unsigned=True, face=True, winding=True, split=True)
    auto = md.query(p, unsigned=True, face=True, winding=True)
    for k in one:
        assert torch.equal(one[k], two[k]) and torch.equal(one[k], auto[k]), k


def test_results_are_deterministic_and_independent_of_the_batch(g11):
    from diffsound_amd.meshsdf import MeshDistance

    md = MeshDistance(g11["spot_vertices"], g11["spot_faces"])
    p = torch.from_numpy(g11["spot_points"]).to(DEV)
    kw = dict(unsigned=True, face=True, winding=True)
    a, b = md.query(p, **kw), md.query(p, **kw)
    perm = torch.randperm(len(p), generator=torch.Generator().manual_seed(5)).to(DEV)
    shuffled = md.query(p[perm], **kw)
    for k in a:
        assert torch.equal(a[k], b[k]), k
        assert torch.equal(a[k][perm], shuffled[k]), k
    for i in (0, 77, 2048, 4095):
        for split in (False, True):
            alone = md.query(p[i:i + 1], split=split, **kw)
            for k in a:
                assert torch.equal(alone[k][0], a[k][i]), (k, i, split)
    part = md.query(p[100:1333], **kw)
    for k in a:
        assert torch.equal(part[k], a[k][100:1333]), k


def test_a_zero_area_face_changes_nothing(g11):
    v, f, p = g11["frog_vertices"], g11["frog_faces"], g11["frog_points"]
    base = _query(v, f, p)
    for extra in ([f[0, 0], f[0, 0], f[0, 1]], [f[7, 1], f[7, 2], f[7, 2]], [f[3, 0], f[3, 0], f[3, 0]]):
        f2 = np.vstack([f[:100], [extra], f[100:]]).astype(f.dtype)
        out = _query(v, f2, p)
        for k in ("signed", "unsigned", "winding"):
            assert np.isfinite(out[k]).all(), k
        assert np.abs(out["unsigned"] - base["unsigned"]).max() <= DIST_TOL
        assert np.array_equal(out["signed"] < 0, base["signed"] < 0)
        assert np.abs(out["winding"] - base["winding"]).max() <= 1e-5
    # alone, such a face is its segment (or point): a finite distance and no solid angle
    a, b = v[f[0, 0]].astype(np.float64), v[f[0, 1]].astype(np.float64)
    out = _query(v, np.array([[f[0, 0], f[0, 0], f[0, 1]]]), p)
    seg = np.sqrt(ref.segment_sqdist(p.astype(np.float64), a, b))
    assert np.abs(out["unsigned"] - seg).max() <= DIST_TOL and (out["winding"] == 0).all() and (out["signed"] >= 0).all()


def test_leading_shapes_and_input_kinds(g11):
    from diffsound_amd.meshsdf import MeshDistance, signed_distance

    v, f = g11["frog_vertices"], g11["frog_faces"]
    p = g11["frog_points"][:2 * 3 * 4].reshape(2, 3, 4, 3)
    md_np = MeshDistance(v, f)
    md_t = MeshDistance(torch.from_numpy(v).to(DEV).double(), torch.from_numpy(f.astype(np.int64)))
    want = md_np.signed_distance(p.reshape(-1, 3)).reshape(2, 3, 4)
    for md in (md_np, md_t):
        for pts in (p, torch.from_numpy(p), torch.from_numpy(p).to(DEV), p.astype(np.float64)):
            s = md.signed_distance(pts)
            assert s.shape == (2, 3, 4) and s.dtype == torch.float32 and s.device == DEV
            assert torch.equal(s, want)
            assert torch.equal(md.unsigned_distance(pts), want.abs())
            w, o, c = md.winding_number(pts), md.occupancy(pts), md.closest_face(pts)
            assert w.shape == o.shape == c.shape == (2, 3, 4)
            assert o.dtype == torch.float32 and c.dtype == torch.int64
            assert torch.equal(o, (want < 0).float())
    assert torch.equal(signed_distance(p, v, f), want)
    assert md_np.signed_distance(np.zeros((0, 3), np.float32)).shape == (0,)
    assert md_np.signed_distance(np.zeros(3, np.float32)).shape == ()


# ---------------------------------------------------------------------------------------------- geometry classes
def _flags(tmp_path):
    return types.SimpleNamespace(mode_num=8, order=1, without_tensorboard=True, out_dir=str(tmp_path))


def _write_meshes(g11, tmp_path):
    from diffsound_amd.meshsdf import write_obj

    paths = {}
    for name in ("frog", "turtle"):
        paths[name] = str(tmp_path / f"{name}.obj")
        write_obj(paths[name], g11[f"{name}_vertices"], g11[f"{name}_faces"])
    return paths


def test_thickness_geometry_end_to_end(g11, tmp_path):
    """thickness_train.py's loop body: apply_sdf -> marching tets (shell) -> largest component -> DiffSoundObj ->
    eigenvalues -> loss -> backward to the thickness coefficient."""
    from diffsound_amd.dmtet import DMTetThickness, DMTetThicknessGeometry, TriangleMesh, kuhn_grid

    paths = _write_meshes(g11, tmp_path)
    torch.manual_seed(0)
    geo = DMTetThicknessGeometry(32, 1.5, _flags(tmp_path), grid=kuhn_grid(32))
    assert isinstance(geo.marching_tets, DMTetThickness) and not hasattr(geo, "writer")
    assert geo.verts.shape == (33 ** 3, 3) and geo.all_edges.shape[1] == 2
    lo, hi = geo.getAABB()
    assert torch.equal(lo, geo.verts.min(0).values) and torch.equal(hi, geo.verts.max(0).values)
    geo.apply_sdf(paths["frog"])
    assert geo.sdf.shape == (33 ** 3,) and geo.sdf.is_cuda
    assert torch.equal(geo.marching_tets.max_thickness, geo.sdf.max()) and float(geo.sdf.max()) > 0
    # positive inside: the reference's flip of open3d's sign
    dist, wind, _ = ref.restatement(geo.verts.cpu().numpy()[::37], g11["frog_vertices"], g11["frog_faces"])
    far = dist > BAND
    assert np.abs(geo.sdf.cpu().numpy()[::37] + ref.signed_from(dist, wind))[far].max() <= DIST_TOL
    vals = geo.get_eigenvalues(thickness_coef=1.0)
    assert vals.shape == (8, 1) and torch.isfinite(vals).all() and (vals > 0).all()
    tri = geo.getMesh(return_triangle=True, thickness_coef=1.0)
    assert isinstance(tri, TriangleMesh) and tri.v_pos.shape[1] == 3 and tri.t_pos_idx.shape[1] == 3
    assert int(tri.t_pos_idx.max()) < tri.v_pos.shape[0]
    params = list(geo.parameters())
    assert len(params) == 1 and params[0] is geo.marching_tets.thickness_coef.probablity
    assert 0 < float(geo.get_thickness()) < 1
    loss = geo.tick(vals * 1.1, 0, geo.FLAGS)
    loss.backward()
    grad = params[0].grad
    assert torch.isfinite(loss) and grad is not None and torch.isfinite(grad).all() and float(grad.abs().sum()) > 0


def test_morphing_geometry_end_to_end(g11, tmp_path):
    """morphing_train.py: apply_sdf2; interp_coef 1 / 0 give the first / second mesh alone."""
    from diffsound_amd.dmtet import DMTetInterpolateGeometry, kuhn_grid

    paths = _write_meshes(g11, tmp_path)
    torch.manual_seed(0)
    geo = DMTetInterpolateGeometry(32, 1.5, _flags(tmp_path), grid=kuhn_grid(32))
    geo.apply_sdf2(paths["frog"], paths["turtle"])
    both = {1.0: geo.get_eigenvalues(interp_coef=1.0), 0.0: geo.get_eigenvalues(interp_coef=0.0)}
    for coef, name in ((1.0, "frog"), (0.0, "turtle")):
        geo.apply_sdf(paths[name])
        assert torch.equal(geo.sdf, geo.sdf1 if coef == 1.0 else geo.sdf2)
        alone = geo.get_eigenvalues(using_interp=False)
        assert alone.shape == (8, 1) and torch.isfinite(alone).all() and (alone > 0).all()
        rel = float(((both[coef] - alone).abs() / alone).max())
        print(f"interp_coef={coef} vs {name} alone: max rel eigenvalue difference {rel:.3e}")
        assert rel <= EIG_RTOL, (name, rel)
    assert float((both[1.0] - both[0.0]).abs().max()) > 0  # two different shapes
    params = list(geo.parameters())
    assert len(params) == 1 and params[0] is geo.marching_tets.interp_coef.probablity
    loss = geo.tick(both[1.0], 0, geo.FLAGS)
    loss.backward()
    assert torch.isfinite(loss) and torch.isfinite(params[0].grad).all() and float(params[0].grad.abs().sum()) > 0
    geo.init_coef(0.25)
    assert abs(float(geo.get_thickness()) - 0.25) < 1e-3
