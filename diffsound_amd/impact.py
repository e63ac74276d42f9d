"""Impact position: the modal gains of a strike at a point of an object's surface, with gradients.

A strike at surface point p with direction d excites mode i with the gain c_i = d . u_i(p), u_i the mass-orthonormal
mode shape (a column of ``DiffSoundObj.U_hat``).  The reference never ties the oscillators' ``amp`` to the mode shapes
(src/ddsp/oscillator.py:76 is a free parameter); ``ContactSurface`` does: it evaluates the finite-element interpolant
of ``U_hat`` on the boundary triangles (csrc/modesample.hip) and differentiates the gains with respect to where the
object is struck and in which direction.  The result feeds the oscillator modules through their ``mode_gain`` keyword.

There is no gradient to ``U_hat`` or to the vertices: the eigenvectors are constants, as everywhere in this package.
There is no CPU fallback.
"""
import torch

from . import _hip, fem_tables
from .diffelastic import bem
from .meshsdf import MeshDistance

__all__ = ["ContactSurface", "face_owners"]

BARY_SUM_TOL = 1e-4


def face_owners(tetmesh, triangles):
    """For each boundary triangle (a, b, c) of ``bem.surface_of(tetmesh)``: the element that owns it and the local
    corners (0..3) of that element at a, b and c.  Returns (elem (F,) long, corner (F, 3) long) on the mesh's device;
    ValueError for a triangle that is the face of no element."""
    order = int(getattr(tetmesh, "order", 1))
    tets = tetmesh.tets.long()
    tri = triangles.long().to(tets.device)
    corners = tets[:, list(fem_tables.CORNER_SLOTS[order])]
    T, nv = tets.shape[0], int(tetmesh.vertices.shape[0])
    if nv >= 2 ** 21:
        raise ValueError(f"face_owners: {nv} nodes, a face key holds three ids below 2^21")
    loc = torch.tensor([[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2]], device=tets.device)  # face opposite local corner o
    key_of = lambda f: (torch.sort(f, dim=1).values * torch.tensor([nv * nv, nv, 1], device=f.device)).sum(1)
    fkey = key_of(corners[:, loc].reshape(-1, 3))  # (4 T): element e, face o at 4 e + o
    skey, order_ = torch.sort(fkey)
    tkey = key_of(tri)
    pos = torch.searchsorted(skey, tkey).clamp_(max=skey.numel() - 1)
    if not bool((skey[pos] == tkey).all()):
        raise ValueError("face_owners: a triangle is not the face of an element")
    elem = order_[pos] // 4
    corner = (corners[elem].unsqueeze(1) == tri.unsqueeze(2)).long().argmax(dim=2)  # (F, 3)
    return elem, corner


def _closest_barycentrics(x, p0, p1, p2):
    """Barycentrics (P, 3) of the point of the triangle (p0, p1, p2) closest to x, clamped to the triangle, in plain
    torch: the plane projection where it falls inside, else the nearest of the three edge projections (each clamped to
    its segment).  Differentiable in x; all (P, 3)."""
    e1, e2, r = p1 - p0, p2 - p0, x - p0
    d11, d12, d22 = (e1 * e1).sum(1), (e1 * e2).sum(1), (e2 * e2).sum(1)
    r1, r2 = (r * e1).sum(1), (r * e2).sum(1)
    det = d11 * d22 - d12 * d12
    v = (d22 * r1 - d12 * r2) / det
    w = (d11 * r2 - d12 * r1) / det
    inside = torch.stack([1 - v - w, v, w], 1)
    ok = (inside >= 0).all(dim=1)

    def on_edge(a, b, ia, ib):
        ab = b - a
        t = (((x - a) * ab).sum(1) / (ab * ab).sum(1)).clamp(0.0, 1.0)
        q = a + t.unsqueeze(1) * ab
        bc = torch.zeros_like(inside)
        bc[:, ia], bc[:, ib] = 1 - t, t
        return bc, ((x - q) ** 2).sum(1)

    cands, dists = zip(on_edge(p0, p1, 0, 1), on_edge(p1, p2, 1, 2), on_edge(p2, p0, 2, 0))
    best = torch.stack(dists, 1).detach().argmin(dim=1)
    edge = torch.stack(cands, 1)[torch.arange(x.shape[0], device=x.device), best]
    return torch.where(ok.unsqueeze(1), inside, edge)


class _ModeSample(torch.autograd.Function):
    """gains (P, m) fp64 of (bary3, direction) on fixed faces: ds_mode_sample_fwd / ds_mode_sample_bwd."""

    @staticmethod
    def forward(ctx, surf, face, bary3, direction):
        elem, corner = surf._elem32[face].contiguous(), surf._corner[face]
        L = torch.zeros((face.shape[0], 4), dtype=torch.float32, device=face.device)
        L.scatter_(1, corner, bary3.detach().float())  # the coordinate of the opposite corner stays 0
        d = direction.detach().float().contiguous()
        out = surf._launch_fwd(elem, L, d, want_out=True, want_vec=False)[0]
        ctx.surf, ctx.corner = surf, corner
        ctx.like = (bary3.dtype, direction.dtype)
        ctx.save_for_backward(elem, L, d)
        return out

    @staticmethod
    def backward(ctx, gout):
        elem, L, d = ctx.saved_tensors
        need_b, need_d = ctx.needs_input_grad[2], ctx.needs_input_grad[3]
        if not (need_b or need_d):
            return None, None, None, None
        gL, gdir = ctx.surf._launch_bwd(elem, L, d, gout.double().contiguous(), need_b, need_d)
        gb = gL.gather(1, ctx.corner).to(ctx.like[0]) if need_b else None
        return None, None, gb, (gdir.to(ctx.like[1]) if need_d else None)


class ContactSurface:
    """The boundary of a ``DiffSoundObj`` as a place to strike it.  Built after ``obj.eigen_decomposition()``; holds the
    boundary triangles (``bem.surface_of``), the element and local corners behind each one, the outward unit normals
    and a ``MeshDistance`` of the surface.  ``obj.U_hat`` is read at every call, so a new eigendecomposition of the same
    mesh is picked up.  Faces are numbered as ``surface_of`` returns them."""

    def __init__(self, obj):
        if getattr(obj, "U_hat", None) is None:
            raise ValueError("ContactSurface: obj.U_hat is missing - run obj.eigen_decomposition() first")
        mesh = obj.tetmesh
        _hip.require_gpu(mesh.vertices, mesh.tets)
        self.obj = obj
        self.device = mesh.vertices.device
        self.order = int(getattr(mesh, "order", 1))
        self.triangles, self.mids = bem.surface_of(mesh)
        self.num_faces = int(self.triangles.shape[0])
        elem, corner = face_owners(mesh, self.triangles)
        self._elem32, self._corner = elem.int().contiguous(), corner.contiguous()
        self._tets32 = mesh.tets.int().contiguous()
        self.num_tets, self.nodes_per_tet = self._tets32.shape
        self.num_nodes = int(mesh.vertices.shape[0])
        lo, hi = int(self._tets32.min()), int(self._tets32.max())
        if lo < 0 or hi >= self.num_nodes:  # (the kernels do not check node ids)
            raise ValueError(f"ContactSurface: node id out of range [0, {self.num_nodes}): min {lo}, max {hi}")
        x = mesh.vertices.detach().double()
        self._corners = x[self.triangles]  # (F, 3, 3) fp64
        cr = torch.linalg.cross(self._corners[:, 1] - self._corners[:, 0], self._corners[:, 2] - self._corners[:, 0])
        self.normals = cr / torch.linalg.vector_norm(cr, dim=1, keepdim=True)
        self.distance = MeshDistance(x, self.triangles, device=self.device)
        self._modes()

    # ------------------------------------------------------------------ validation
    def _modes(self):
        U = getattr(self.obj, "U_hat", None)
        if U is None:
            raise ValueError("ContactSurface: obj.U_hat is missing - run obj.eigen_decomposition() first")
        if U.dim() != 2 or U.shape[0] != 3 * self.num_nodes or U.shape[1] < 1:
            raise ValueError(f"ContactSurface: U_hat must be (3 * {self.num_nodes}, modes), got {tuple(U.shape)}")
        _hip.require_gpu(U)
        U = U.detach()
        if U.dtype != torch.float64 or U.stride(1) != 1 or U.stride(0) < U.shape[1]:
            U = U.double().contiguous()
        return U

    def _check(self, face, bary3, direction):
        """(face (P,) long, bary3 (P, 3), direction (P, 3)) validated: RuntimeError for CPU tensors, ValueError for bad
        shapes, face ids out of range, non-finite input and barycentrics that do not sum to 1."""
        if not isinstance(face, torch.Tensor) or not isinstance(bary3, torch.Tensor):
            raise ValueError("ContactSurface: face and bary3 must be torch tensors")
        _hip.require_gpu(face, bary3)
        if face.dim() != 1 or face.dtype not in (torch.int64, torch.int32) or face.shape[0] < 1:
            raise ValueError(f"ContactSurface: face must be a non-empty integer (P,) tensor, got {tuple(face.shape)} {face.dtype}")
        P = face.shape[0]
        if bary3.shape != (P, 3) or not bary3.dtype.is_floating_point:
            raise ValueError(f"ContactSurface: bary3 must be a floating ({P}, 3) tensor, got {tuple(bary3.shape)} {bary3.dtype}")
        lo, hi = int(face.min()), int(face.max())
        if lo < 0 or hi >= self.num_faces:
            raise ValueError(f"ContactSurface: face id out of range [0, {self.num_faces}): min {lo}, max {hi}")
        face = face.long()
        if not bool(torch.isfinite(bary3.detach().float()).all()):
            raise ValueError("ContactSurface: non-finite barycentric coordinate")
        worst = float((bary3.detach().double().sum(1) - 1).abs().max())
        if worst > BARY_SUM_TOL:
            raise ValueError(f"ContactSurface: barycentrics must sum to 1 within {BARY_SUM_TOL} (off by {worst:.3g})")
        if isinstance(direction, str):
            if direction != "normal":
                raise ValueError(f"ContactSurface: direction must be a tensor or 'normal', got {direction!r}")
            direction = self.normals[face]
        else:
            if not isinstance(direction, torch.Tensor) or not direction.dtype.is_floating_point:
                raise ValueError("ContactSurface: direction must be a floating (P, 3) or (3,) tensor, or 'normal'")
            _hip.require_gpu(direction)
            if direction.shape == (3,):
                direction = direction.unsqueeze(0).expand(P, 3)
            if direction.shape != (P, 3):
                raise ValueError(f"ContactSurface: direction must be ({P}, 3) or (3,), got {tuple(direction.shape)}")
            if not bool(torch.isfinite(direction.detach().float()).all()):
                raise ValueError("ContactSurface: non-finite direction (or one outside the float32 range)")
        return face, bary3, direction

    # ------------------------------------------------------------------ launches
    def _args(self, U, elem, L, d):
        p = _hip.ptr
        return (p(self._tets32), self.num_tets, self.nodes_per_tet, self.num_nodes, p(U), U.stride(0), U.shape[1], p(elem),
                p(L), p(d), elem.shape[0])

    def _launch_fwd(self, elem, L, d, want_out, want_vec):
        U = self._modes()
        P, m = elem.shape[0], U.shape[1]
        out = torch.empty((P, m), dtype=torch.float64, device=self.device) if want_out else None
        vec = torch.empty((P, m, 3), dtype=torch.float64, device=self.device) if want_vec else None
        _hip.launch("ds_mode_sample_fwd", *self._args(U, elem, L, d), _hip.ptr(out), _hip.ptr(vec), device=self.device)
        return out, vec

    def _launch_bwd(self, elem, L, d, gout, want_l, want_d):
        U = self._modes()
        P, m = elem.shape[0], U.shape[1]
        if gout.shape != (P, m):
            raise ValueError(f"ContactSurface: the gains' gradient must be ({P}, {m}), got {tuple(gout.shape)} - "
                             "U_hat changed between forward and backward")
        gL = torch.empty((P, 4), dtype=torch.float64, device=self.device) if want_l else None
        gdir = torch.empty((P, 3), dtype=torch.float64, device=self.device) if want_d else None
        _hip.launch("ds_mode_sample_bwd", *self._args(U, elem, L, d), _hip.ptr(gout), _hip.ptr(gL), _hip.ptr(gdir), device=self.device)
        return gL, gdir

    # ------------------------------------------------------------------ public interface
    def locate(self, points):
        """(face (P,) long, bary3 (P, 3)) of the surface points closest to ``points`` (P, 3): the closest face from
        ``MeshDistance.closest_face``, then the barycentrics of the closest point of that face, clamped to the
        triangle, in the dtype of ``points``.  For a fixed face ``bary3`` is differentiable in ``points``."""
        if not isinstance(points, torch.Tensor):
            raise ValueError("ContactSurface.locate: points must be a torch tensor")
        _hip.require_gpu(points)
        if points.dim() != 2 or points.shape[1] != 3 or points.shape[0] < 1 or not points.dtype.is_floating_point:
            raise ValueError(f"ContactSurface.locate: points must be a floating (P, 3) tensor, got {tuple(points.shape)}")
        if not bool(torch.isfinite(points.detach().float()).all()):
            raise ValueError("ContactSurface.locate: non-finite point coordinate (or one outside the float32 range)")
        face = self.distance.closest_face(points.detach())
        c = self._corners[face].to(points.dtype)
        return face, _closest_barycentrics(points, c[:, 0], c[:, 1], c[:, 2])

    def amplitudes(self, face, bary3, direction="normal"):
        """Gains (P, m) fp64 of a strike at the points (face, bary3) with ``direction``: a (P, 3) or (3,) tensor, or
        ``"normal"`` for the outward unit normal of the face.  Differentiable in ``bary3`` and ``direction``."""
        face, bary3, direction = self._check(face, bary3, direction)
        self._modes()
        return _ModeSample.apply(self, face, bary3, direction)

    def amplitudes_at(self, points, direction="normal"):
        """``amplitudes(*locate(points), direction)``: differentiable in ``points``."""
        return self.amplitudes(*self.locate(points), direction)

    def path_gains(self, points, direction="normal"):
        """Gains (A, K, m) fp64 along a contact path: ``points`` (K, 3) - one clip - or (A, K, 3), the contact point at K
        control frames.  ``amplitudes_at`` on all A K points at once, so differentiable in ``points``; the result is the
        3-D ``mode_gain`` of the oscillator modules and the ``gain`` of ``ddsp.bank.oscillator_bank_sliding``, which
        interpolate it linearly between the frames.  ``direction``: "normal", or a tensor shaped like ``points`` or (3,)."""
        if not isinstance(points, torch.Tensor) or points.dim() not in (2, 3) or points.shape[-1] != 3 or points.numel() == 0:
            raise ValueError("ContactSurface.path_gains: points must be a (K, 3) or (A, K, 3) tensor, got "
                             f"{tuple(points.shape) if isinstance(points, torch.Tensor) else type(points).__name__}")
        lead = (1, points.shape[0]) if points.dim() == 2 else tuple(points.shape[:2])
        if isinstance(direction, torch.Tensor) and direction.shape == points.shape:
            direction = direction.reshape(-1, 3)
        gains = self.amplitudes_at(points.reshape(-1, 3), direction)
        return gains.reshape(*lead, gains.shape[1])

    def amplitude_map(self, direction="normal"):
        """Gains (num_faces, m) fp64 at every face centroid, in one launch: the map to compare measured gains with."""
        face = torch.arange(self.num_faces, device=self.device)
        bary3 = torch.full((self.num_faces, 3), 1.0 / 3.0, dtype=torch.float64, device=self.device)
        return self.amplitudes(face, bary3, direction)

    def displacement(self, face, bary3):
        """Mode shapes (P, m, 3) fp64 at the points (face, bary3): the interpolated displacement of every mode, without
        the dot product.  Not differentiable."""
        face, bary3, _ = self._check(face, bary3, "normal")
        elem, corner = self._elem32[face].contiguous(), self._corner[face]
        L = torch.zeros((face.shape[0], 4), dtype=torch.float32, device=self.device)
        L.scatter_(1, corner, bary3.detach().float())
        return self._launch_fwd(elem, L, None, want_out=False, want_vec=True)[1]
