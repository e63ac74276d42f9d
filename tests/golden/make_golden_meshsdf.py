#!/usr/bin/env python3
"""Generate tests/golden/g11_meshsdf.npz: meshes, query points and the expected distance, winding number and closest
face for the mesh signed distance (diffsound_amd.meshsdf, csrc/meshsdf.hip).

Run only in the build container (needs the reference tree's data files, see _ref_harness.py):

    python tests/golden/make_golden_meshsdf.py

Stored (data only), per case ``frog``, ``turtle`` (data/mesh/*.obj) and ``spot`` (data/mesh/shape/spot_surf.obj):

* ``{case}_vertices`` (float32) and ``{case}_faces`` (int32), read by the minimal parser below (independent of
  diffsound_amd.meshsdf.read_obj, which the tests check against these arrays);
* ``{case}_points`` (float32): for frog and turtle the vertices of the reference's 32 tet grid times 1.5 (the float32
  product DMTetGeometry forms, dmtet_thickness.py:221-224); for spot the 16^3 lattice of
  experiments/geometry_train.py:156-167 around the mesh's bounding box;
* ``{case}_unsigned`` (float64), ``{case}_winding`` (float64), ``{case}_face`` (int32): the fp64 NumPy restatement of
  tests/test_meshsdf_cpu.py;
* ``{case}_open3d_signed`` (float32) only when open3d imports where this runs: its compute_signed_distance.

Every case must keep at most 1 % of its points within 1e-5 of the surface and every winding number within 1e-9 of 0 or 1
(the meshes are watertight); the generator fails otherwise.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import _ref_harness  # noqa: E402
from test_meshsdf_cpu import restatement  # noqa: E402

REF = _ref_harness.REFERENCE_ROOT


def parse_obj(path):
    """v and f records only; f tokens i, i/j, i//k, i/j/k with positive indices; triangles only."""
    v, f = [], []
    for line in open(path):
        t = line.split()
        if t[:1] == ["v"]:
            v.append([float(x) for x in t[1:4]])
        elif t[:1] == ["f"]:
            assert len(t) == 4, line
            f.append([int(x.split("/")[0]) - 1 for x in t[1:]])
    return np.array(v, dtype=np.float32), np.array(f, dtype=np.int32)


def lattice(vertices, voxel_num=16):
    """The query lattice of experiments/geometry_train.py:156-167."""
    min_bound, max_bound = vertices.min(0), vertices.max(0)
    center = (min_bound + max_bound) / 2
    size = (max_bound - min_bound).max()
    min_bound = center - size / 2 * 1.05
    max_bound = center + size / 2 * 1.05
    xyz_range = np.linspace(min_bound, max_bound, num=voxel_num)
    return np.stack(np.meshgrid(*xyz_range.T), axis=-1).astype(np.float32).reshape(-1, 3)


def main():
    grid = np.load(os.path.join(REF, "data", "tets", "32_tets.npz"))["vertices"].astype(np.float32)
    grid_points = (grid * np.float32(1.5)).astype(np.float32)
    cases = {"frog": "data/mesh/frog.obj", "turtle": "data/mesh/turtle.obj", "spot": "data/mesh/shape/spot_surf.obj"}
    try:
        import open3d as o3d
    except ImportError:
        o3d = None
    out = {}
    for name, rel in cases.items():
        v, f = parse_obj(os.path.join(REF, rel))
        p = lattice(v) if name == "spot" else grid_points
        dist, wind, face = restatement(p, v, f)
        near = float((dist < 1e-5).mean())
        wdev = float(np.abs(wind - np.round(wind)).max())
        print(f"{name}: V={len(v)} F={len(f)} P={len(p)} min dist {dist.min():.3e} within 1e-5: {near:.4f} "
              f"winding deviation {wdev:.2e} inside {int((wind > 0.5).sum())}")
        assert near <= 0.01, f"{name}: {near:.2%} of the points lie within 1e-5 of the surface"
        assert wdev < 1e-9 and set(np.round(wind)) <= {0.0, 1.0}, f"{name}: not watertight (winding deviation {wdev})"
        out[f"{name}_vertices"], out[f"{name}_faces"], out[f"{name}_points"] = v, f, p
        out[f"{name}_unsigned"], out[f"{name}_winding"], out[f"{name}_face"] = dist, wind, face.astype(np.int32)
        if o3d is not None:
            scene = o3d.t.geometry.RaycastingScene()
            scene.add_triangles(o3d.core.Tensor(v), o3d.core.Tensor(f.astype(np.uint32)))
            out[f"{name}_open3d_signed"] = scene.compute_signed_distance(o3d.core.Tensor(p)).numpy()
    path = os.path.join(HERE, "g11_meshsdf.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", "with" if o3d is not None else "without", "open3d")


if __name__ == "__main__":
    main()
