"""Differentiable marching tets (diffsound_amd/dmtet.py, csrc/dmtet.hip) without a device: a NumPy restatement of the
three reference variants, checked against the reference's outputs and VJPs (tests/golden/g10_dmtet.npz, written by
make_golden_dmtet.py); the drop-in import path; the jitter-free Kuhn grid.  tests/test_dmtet_gpu.py checks the kernels
against the same fixture and this restatement.

The restatement follows the kernels' scheme, not the reference's op chain: the crossing edges are numbered in the
static (a, b) order of the grid's edge list, the output tets are written section by section (1-tet classes, 3-tet
classes, inner tets, each in tet order), and the kept grid vertices come first in ascending order, then the edge
vertices.  That it reproduces the reference bit for bit is the ordering argument of DESIGN.md section 10."""
import json
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "g10_dmtet.npz")

# local edges of a tet in DMTet's order; slots 0-3 = tet vertices, 4-9 = points on these edges
EDGES = np.array([[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [2, 3]])
# class (bit k = vertex k inside) -> split tets, as rows of 4 local slots (DMTet / kaolin marching-tets table)
SPLIT = {
    1: [[0, 4, 5, 6]], 2: [[1, 4, 8, 7]], 4: [[2, 5, 7, 9]], 8: [[3, 6, 9, 8]],
    3: [[7, 1, 8, 6], [5, 1, 7, 6], [5, 0, 1, 6]], 5: [[4, 0, 6, 7], [9, 0, 7, 6], [7, 0, 9, 2]],
    6: [[4, 1, 9, 8], [5, 1, 9, 4], [5, 1, 2, 9]], 7: [[6, 0, 1, 2], [8, 6, 1, 2], [9, 6, 8, 2]],
    9: [[5, 0, 4, 8], [5, 0, 8, 3], [5, 8, 9, 3]], 10: [[1, 4, 7, 3], [4, 7, 6, 3], [9, 6, 7, 3]],
    11: [[0, 1, 5, 3], [5, 1, 9, 3], [5, 1, 7, 9]], 12: [[5, 2, 3, 7], [3, 6, 5, 8], [3, 5, 7, 8]],
    13: [[0, 4, 7, 8], [0, 3, 8, 7], [0, 3, 7, 2]], 14: [[4, 1, 2, 3], [4, 3, 2, 5], [4, 3, 5, 6]],
}
# class -> surface triangles as local edge ids
TRIS = {
    1: [[1, 0, 2]], 2: [[4, 0, 3]], 3: [[1, 4, 2], [1, 3, 4]], 4: [[3, 1, 5]], 5: [[2, 3, 0], [2, 5, 3]],
    6: [[1, 4, 0], [1, 5, 4]], 7: [[4, 2, 5]], 8: [[4, 5, 2]], 9: [[4, 1, 0], [4, 5, 1]], 10: [[3, 2, 0], [3, 5, 2]],
    11: [[1, 3, 5]], 12: [[4, 1, 2], [4, 3, 1]], 13: [[3, 0, 4]], 14: [[2, 0, 1]],
}


def grid_edges(tets):
    """Distinct edges (a < b) sorted by (a, b), and the (T, 6) edge id of each tet's local edges."""
    pairs = np.sort(tets[:, EDGES].reshape(-1, 2), axis=1)
    uniq, inv = np.unique(pairs, axis=0, return_inverse=True)
    return uniq[:, 0], uniq[:, 1], inv.reshape(-1, 6)


def restate(pos, sdf, tets, t=None, faces=False):
    """Marching tets of sdf on (pos, tets): inside = sdf > 0, or 0 < sdf <= t.  Returns a dict with verts, tets
    (and surf_verts, faces) plus what the VJP needs.  Arithmetic in pos's dtype (the reference's fp32 formula)."""
    dt = pos.dtype
    sdf = np.asarray(sdf, dt).reshape(-1)
    hi = np.inf if t is None else dt.type(t)
    inside = (sdf > 0) & (sdf <= hi)
    ea, eb, tet_edge = grid_edges(tets)
    cls = (inside[tets] * (1 << np.arange(4))).sum(1)
    cross = inside[ea] != inside[eb]
    has_edge = np.zeros(len(pos), bool)
    has_edge[ea] = has_edge[eb] = True
    used = inside & has_edge
    vid = np.cumsum(used) - 1
    eid = np.cumsum(cross) - 1
    n_used = int(used.sum())
    xa, xb = ea[cross], eb[cross]
    sa, sb = sdf[xa].copy(), sdf[xb].copy()
    shifted = np.zeros(len(xa), bool) if t is None else (sa > 0) & (sb > 0)
    sa[shifted] -= hi
    sb[shifted] -= hi
    d = sa + (-sb)
    wa, wb = (-sb) / d, sa / d
    ev = pos[xa] * wa[:, None] + pos[xb] * wb[:, None]
    verts = np.concatenate([pos[used], ev]).astype(dt)
    local = np.concatenate([vid[tets], n_used + eid[tet_edge]], axis=1)
    rows = []
    for group in ((1, 2, 4, 8), (3, 5, 6, 7, 9, 10, 11, 12, 13, 14)):  # 1-tet classes, then 3-tet classes
        sel = np.flatnonzero(np.isin(cls, group))
        for i in sel:
            rows.extend(local[i][np.array(SPLIT[cls[i]])])
    rows.extend(local[np.flatnonzero(cls == 15), :4])
    out = dict(verts=verts, tets=np.array(rows, dtype=np.int64).reshape(-1, 4), n_used=n_used, xa=xa, xb=xb,
               shifted=shifted, sa=sa, sb=sb, d=d, used=used)
    if faces:
        fr = []
        for ntri in (1, 2):
            for i in np.flatnonzero([len(TRIS.get(c, [])) == ntri for c in cls]):
                fr.extend(eid[tet_edge[i]][np.array(TRIS[cls[i]])])
        out["faces"] = np.array(fr, dtype=np.int64).reshape(-1, 3)
        out["surf_verts"] = ev.astype(dt)
    return out


def restate_vjp(pos, sdf, tets, gv, t=None):
    """Closed-form VJP in fp64: cotangent gv of the output verts -> (dpos, dsdf, dt)."""
    pos = np.asarray(pos, np.float64)
    r = restate(pos, sdf, tets, t)
    n, n_used = len(pos), r["n_used"]
    dpos, dsdf = np.zeros((n, 3)), np.zeros(n)
    dpos[np.flatnonzero(r["used"])] += gv[:n_used]
    g = gv[n_used:]
    xa, xb, sa, sb, d = r["xa"], r["xb"], r["sa"], r["sb"], r["d"]
    q = (g * (pos[xa] - pos[xb])).sum(1) / d / d
    np.add.at(dpos, xa, g * (-sb / d)[:, None])
    np.add.at(dpos, xb, g * (sa / d)[:, None])
    gsa, gsb = q * sb, -q * sa
    np.add.at(dsdf, xa, gsa)
    np.add.at(dsdf, xb, gsb)
    dth = -float((gsa + gsb)[r["shifted"]].sum())
    return dpos, dsdf, dth


@pytest.fixture(scope="module")
def g10():
    if not os.path.exists(FIXTURE):
        pytest.skip("fixture g10_dmtet.npz missing")
    return np.load(FIXTURE, allow_pickle=False)


def _cases(g):
    return [str(c) for c in g["cases"]]


def _close(a, b, rel):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape
    scale = max(np.abs(b).max(), 1e-30) if b.size else 1.0
    assert np.abs(a - b).max(initial=0.0) <= rel * scale, (np.abs(a - b).max(initial=0.0), scale)


def test_restatement_matches_reference_outputs(g10):
    tets = g10["grid_indices"]
    for c in _cases(g10):
        pos, sdf, t = g10[f"{c}/pos"], g10[f"{c}/sdf"], g10[f"{c}/t"]
        r = restate(pos, sdf, tets)
        assert np.array_equal(r["tets"], g10[f"{c}/plain/tets"]), c
        _close(r["verts"], g10[f"{c}/plain/verts"], 1e-6)
        r = restate(pos, sdf, tets, t=t, faces=True)
        assert np.array_equal(r["tets"], g10[f"{c}/thick/all_tets"]), c
        assert np.array_equal(r["faces"], g10[f"{c}/thick/faces"]), c
        _close(r["verts"], g10[f"{c}/thick/all_verts"], 1e-6)
        _close(r["surf_verts"], g10[f"{c}/thick/verts"], 1e-6)
        cc = g10[f"{c}/c"]
        blend = cc * sdf + (np.float32(1) - cc) * g10[f"{c}/sdf2"]
        r = restate(pos, blend, tets, faces=True)
        assert np.array_equal(r["tets"], g10[f"{c}/interp/all_tets"]), c
        assert np.array_equal(r["faces"], g10[f"{c}/interp/faces"]), c
        _close(r["verts"], g10[f"{c}/interp/all_verts"], 1e-6)


def test_restatement_vertices_are_the_reference_fp32_bits(g10):
    tets = g10["grid_indices"]
    for c in _cases(g10):
        r = restate(g10[f"{c}/pos"], g10[f"{c}/sdf"], tets, t=g10[f"{c}/t"])
        assert np.array_equal(r["verts"].view(np.uint32), g10[f"{c}/thick/all_verts"].view(np.uint32)), c


def test_restatement_vjp_matches_reference(g10):
    tets = g10["grid_indices"]
    for c in _cases(g10):
        pos, sdf, t = g10[f"{c}/pos"], g10[f"{c}/sdf"], float(g10[f"{c}/t"])
        dpos, dsdf, _ = restate_vjp(pos, sdf, tets, g10[f"{c}/plain/cot"].astype(np.float64))
        _close(dpos, g10[f"{c}/plain/dpos"], 1e-9)
        _close(dsdf, g10[f"{c}/plain/dsdf"], 1e-9)
        # thickness: cotangent on all_verts plus one on the surface verts (the tail of all_verts)
        r = restate(pos, sdf, tets, t=t)
        gv = g10[f"{c}/thick/cot_all"].astype(np.float64).copy()
        gv[r["n_used"]:] += g10[f"{c}/thick/cot_surf"]
        dpos, dsdf, dth = restate_vjp(pos, sdf, tets, gv, t=t)
        _close(dpos, g10[f"{c}/thick/dpos"], 1e-9)
        _close(dsdf, g10[f"{c}/thick/dsdf"], 1e-9)
        assert abs(dth - float(g10[f"{c}/thick/dt"])) <= 1e-9 * max(1.0, abs(float(g10[f"{c}/thick/dt"]))), c
        # interpolation: chain rule through the blend
        cc = float(g10[f"{c}/c"])
        s1, s2 = sdf.astype(np.float64), g10[f"{c}/sdf2"].astype(np.float64)
        blend32 = g10[f"{c}/c"] * sdf + (np.float32(1) - g10[f"{c}/c"]) * g10[f"{c}/sdf2"]
        dpos, dsdf, _ = restate_vjp(pos, blend32, tets, g10[f"{c}/interp/cot_all"].astype(np.float64))
        _close(dpos, g10[f"{c}/interp/dpos"], 1e-6)
        _close(cc * dsdf, g10[f"{c}/interp/dsdf"], 1e-6)
        _close((1 - cc) * dsdf, g10[f"{c}/interp/dsdf2"], 1e-6)
        dc = float((dsdf * (s1 - s2)).sum())
        assert abs(dc - float(g10[f"{c}/interp/dc"])) <= 1e-6 * max(1.0, abs(dc)), c


def test_all_outside_case_is_empty(g10):
    assert g10["outside/plain/tets"].shape == (0, 4) and g10["outside/plain/verts"].shape == (0, 3)
    assert not np.any(g10["outside/plain/dpos"]) and not np.any(g10["outside/plain/dsdf"])


def test_kuhn_grid_is_conforming_with_positive_volume():
    from diffsound_amd.dmtet import kuhn_grid

    v, t = kuhn_grid(5)
    assert v.dtype == np.float32 and t.dtype == np.int64 and t.shape == (6 * 125, 4) and len(v) == 216
    assert v.min() == -0.5 and v.max() == 0.5
    p = v.astype(np.float64)[t]
    vol = np.einsum("ij,ij->i", np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), p[:, 3] - p[:, 0]) / 6
    assert np.all(np.abs(vol) > 0)
    assert abs(np.abs(vol).sum() - 1.0) < 1e-9  # the tets tile the unit cube
    # conforming: every interior face is shared by exactly two tets, every boundary face lies on the cube's surface
    faces = np.sort(t[:, [[0, 1, 2], [0, 1, 3], [0, 2, 3], [1, 2, 3]]].reshape(-1, 3), axis=1)
    uf, cnt = np.unique(faces, axis=0, return_counts=True)
    assert cnt.max() == 2
    bnd = v[uf[cnt == 1]]
    on_surface = np.any(np.all(np.abs(np.abs(bnd) - 0.5) < 1e-7, axis=1), axis=1)
    assert on_surface.all()


def test_out_of_scope_import_now_resolves():
    with open(os.path.join(ROOT, "tests", "golden", "experiment_imports.json")) as f:
        entries = json.load(f)["out_of_scope"]
    code = "import importlib\n"
    for mod, names in entries.items():
        for name in names:
            code += f"assert getattr(importlib.import_module({mod!r}), {name!r}).__module__.startswith('diffsound_amd')\n"
    env = dict(os.environ, PYTHONPATH=ROOT)
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT, env=env)


def test_extend_path_falls_through_to_a_second_src_tree(tmp_path):
    """With this tree first and another ``src`` tree second on sys.path, modules this project does not have
    (src.dmtet.geometry.sdf) come from the second tree, and what they import from src.diffelastic is ours."""
    geo = tmp_path / "src" / "dmtet" / "geometry"
    geo.mkdir(parents=True)
    (tmp_path / "src" / "__init__.py").write_text("")
    (geo / "sdf.py").write_text("from src.diffelastic.diff_model import TetMesh\n")
    code = textwrap.dedent(f"""
        import sys
        sys.path[:0] = [{ROOT!r}, {str(tmp_path)!r}]
        import src.dmtet.geometry.sdf as sdf
        import src.dmtet.geometry.dmtet_geometry as dg
        assert sdf.__file__.startswith({str(tmp_path)!r}), sdf.__file__
        assert dg.DMTetGeometry.__module__ == "diffsound_amd.dmtet"
        assert sdf.TetMesh.__module__.startswith("diffsound_amd")
    """)
    subprocess.run([sys.executable, "-c", code], check=True, cwd=str(tmp_path))
