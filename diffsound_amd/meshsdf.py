"""Signed distance from a triangle mesh to points on the HIP device, and the .obj reading and writing around it.

The reference's thickness, morphing and shape-fitting loops get the signed distance of a mesh at the DMTet grid vertices
(or on a voxel lattice) from ``open3d.t.geometry.RaycastingScene.compute_signed_distance``
(src/dmtet/geometry/dmtet_thickness.py:301-314, dmtet_interpolate.py:318-351, experiments/geometry_train.py:170-197).
Here csrc/meshsdf.hip does it by brute force over all (point, face) pairs: the exact point-triangle distance and the
generalised winding number, whose test ``> 0.5`` gives the sign (negative inside, open3d's convention).  The faces must
be wound counter-clockwise seen from outside, as every mesh the reference ships is.

There is no autograd through the distance: the reference has none either (open3d returns constants).
"""
import numpy as np
import torch

from . import _hip

__all__ = ["read_obj", "write_obj", "MeshDistance", "signed_distance", "TILE"]

TILE = 128  # faces per LDS tile of csrc/meshsdf.hip (= points per workgroup); the tests cross it on purpose


def _obj_index(token, count):
    """The vertex index of one ``f`` token (``i``, ``i/j``, ``i//k`` or ``i/j/k``; 1-based, negative = from the end)."""
    i = int(token.split("/", 1)[0])
    if i == 0:
        raise ValueError("read_obj: vertex index 0 in an f record")
    return i - 1 if i > 0 else count + i


def read_obj(path):
    """Vertices (V, 3) float32 and faces (F, 3) int64 of a Wavefront .obj file.  Reads the ``v`` records (the first
    three numbers) and the ``f`` records in the forms ``i``, ``i/j``, ``i//k`` and ``i/j/k``; a negative index counts
    from the last vertex read so far; a polygon becomes a triangle fan; every other record is ignored."""
    verts, faces = [], []
    with open(path, "r") as fh:
        for line in fh:
            parts = line.split()
            if not parts:
                continue
            if parts[0] == "v":
                if len(parts) < 4:
                    raise ValueError(f"read_obj: {path}: a v record with fewer than three coordinates")
                verts.append((float(parts[1]), float(parts[2]), float(parts[3])))
            elif parts[0] == "f":
                idx = [_obj_index(t, len(verts)) for t in parts[1:]]
                if len(idx) < 3:
                    raise ValueError(f"read_obj: {path}: an f record with fewer than three vertices")
                for k in range(1, len(idx) - 1):
                    faces.append((idx[0], idx[k], idx[k + 1]))
    v = np.asarray(verts, dtype=np.float32).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    if f.size and (f.min() < 0 or f.max() >= len(v)):
        raise ValueError(f"read_obj: {path}: face index out of range")
    return v, f


def write_obj(path, vertices, faces):
    """Write ``v`` and ``f`` records (1-based).  Coordinates are written with 9 significant digits, enough to read
    a float32 back exactly."""
    v = _to_numpy(vertices).astype(np.float64).reshape(-1, 3)
    f = _to_numpy(faces).astype(np.int64).reshape(-1, 3)
    with open(path, "w") as fh:
        for x, y, z in v:
            fh.write(f"v {x:.9g} {y:.9g} {z:.9g}\n")
        for a, b, c in f:
            fh.write(f"f {a + 1} {b + 1} {c + 1}\n")


def _to_numpy(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _as_tensor(a, what):
    if isinstance(a, torch.Tensor):
        return a.detach()
    try:
        return torch.from_numpy(np.ascontiguousarray(np.asarray(a)))
    except TypeError as ex:
        raise ValueError(f"{what}: cannot be read as an array ({ex})") from None


def _check_mesh(vertices, faces):
    """(vertices, faces) as tensors on their own devices, validated: ValueError before any device work of ours."""
    v, f = _as_tensor(vertices, "vertices"), _as_tensor(faces, "faces")
    if v.dim() != 2 or v.shape[1] != 3 or not v.dtype.is_floating_point:
        raise ValueError(f"MeshDistance: vertices must be a floating (V, 3) array, got {tuple(v.shape)} {v.dtype}")
    if f.dim() != 2 or f.shape[1] != 3 or f.dtype not in (torch.int64, torch.int32, torch.int16, torch.uint8, torch.int8):
        raise ValueError(f"MeshDistance: faces must be an integer (F, 3) array, got {tuple(f.shape)} {f.dtype}")
    if v.shape[0] == 0 or f.shape[0] == 0:
        raise ValueError("MeshDistance: empty mesh")
    if f.shape[0] > 2 ** 30:
        raise ValueError("MeshDistance: more than 2^30 faces")
    if not bool(torch.isfinite(v).all()):
        raise ValueError("MeshDistance: non-finite vertex coordinate")
    if not bool(torch.isfinite(v.float()).all()):
        raise ValueError("MeshDistance: vertex coordinate outside the float32 range")
    lo, hi = int(f.min()), int(f.max())
    if lo < 0 or hi >= v.shape[0]:
        raise ValueError(f"MeshDistance: face index out of range [0, {v.shape[0]}): min {lo}, max {hi}")
    return v, f


def _check_points(points):
    p = _as_tensor(points, "points")
    if p.dim() < 1 or p.shape[-1] != 3 or not p.dtype.is_floating_point:
        raise ValueError(f"MeshDistance: points must be a floating (..., 3) array, got {tuple(p.shape)} {p.dtype}")
    if not bool(torch.isfinite(p.float()).all()):
        raise ValueError("MeshDistance: non-finite point coordinate (or one outside the float32 range)")
    return p


class MeshDistance:
    """Distance queries against one triangle mesh, packed once on the device (open3d: a RaycastingScene with one
    mesh).  ``vertices`` (V, 3) floating and ``faces`` (F, 3) integer may be numpy arrays or torch tensors on any
    device; ``device`` defaults to the current HIP device.  Every query takes points of shape (..., 3), numpy or
    torch, and returns a torch tensor of the leading shape on the device."""

    def __init__(self, vertices, faces, device=None):
        v, f = _check_mesh(vertices, faces)
        if device is None:
            if not torch.cuda.is_available():
                raise RuntimeError("diffsound_amd.meshsdf: no HIP device available (there is no CPU fallback)")
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("diffsound_amd.meshsdf: the mesh must live on a HIP device (there is no CPU fallback)")
        self.vertices = v.to(self.device, torch.float32).contiguous()
        self.faces = f.to(self.device, torch.int64).contiguous()
        self.num_faces = int(f.shape[0])
        f32 = self.faces.int().contiguous()
        self._records = torch.empty((self.num_faces, 16), dtype=torch.float32, device=self.device)
        _hip.launch("ds_mesh_sdf_pack", self.vertices.data_ptr(), f32.data_ptr(), self.vertices.shape[0], self.num_faces,
                    self._records.data_ptr(), device=self.device)

    def query(self, points, unsigned=False, face=False, winding=False, split=None):
        """All outputs of one pass as a dict: ``signed`` always, ``unsigned`` / ``face`` (int64) / ``winding`` on
        request.  ``split``: None lets the library choose the launch shape, True / False force the one that splits the
        faces across workgroups / the single launch (both give the same bits)."""
        p = _check_points(points)
        lead = tuple(p.shape[:-1])
        pts = p.to(self.device, torch.float32).reshape(-1, 3).contiguous()
        P = pts.shape[0]
        new = lambda dt: torch.empty(P, dtype=dt, device=self.device)
        out_s = new(torch.float32)
        out_u = new(torch.float32) if unsigned else None
        out_f = new(torch.int32) if face else None
        out_w = new(torch.float32) if winding else None
        work, nbytes = None, 0
        if split is None or split:
            # (not _hip.workspace: a negative answer is this query's refusal, and 0 means no workspace at all)
            nbytes = int(_hip.lib().ds_mesh_sdf_workspace_bytes(P, self.num_faces, 1 if split else 0))
            if nbytes < 0:
                raise ValueError(f"MeshDistance: too many points ({P})")
            if nbytes:
                work = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        _hip.launch("ds_mesh_sdf_query", pts.data_ptr(), P, self._records.data_ptr(), self.num_faces, out_s.data_ptr(), _hip.ptr(out_u),
                    _hip.ptr(out_f), _hip.ptr(out_w), _hip.ptr(work), nbytes, device=self.device)
        res = {"signed": out_s.reshape(lead)}
        if unsigned:
            res["unsigned"] = out_u.reshape(lead)
        if face:
            res["face"] = out_f.long().reshape(lead)
        if winding:
            res["winding"] = out_w.reshape(lead)
        return res

    def signed_distance(self, points):
        """Distance to the surface, negative inside (open3d's compute_signed_distance)."""
        return self.query(points)["signed"]

    def unsigned_distance(self, points):
        """Distance to the surface (open3d's compute_distance)."""
        return self.query(points, unsigned=True)["unsigned"]

    def winding_number(self, points):
        """Generalised winding number: 1 inside and 0 outside a watertight, outward-wound mesh."""
        return self.query(points, winding=True)["winding"]

    def occupancy(self, points):
        """1.0 inside, 0.0 outside (float32, open3d's compute_occupancy): winding number > 0.5."""
        return (self.query(points, winding=True)["winding"] > 0.5).float()

    def closest_face(self, points):
        """Index (int64) of the nearest face, the lowest one on equal squared distances."""
        return self.query(points, face=True)["face"]


def signed_distance(points, vertices, faces):
    """One-shot form: the signed distance (negative inside) of ``points`` (..., 3) to the mesh."""
    _check_points(points)
    return MeshDistance(vertices, faces).signed_distance(points)
