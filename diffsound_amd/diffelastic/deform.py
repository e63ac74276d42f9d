"""Deform - the deformation gradient at the Gauss points and the stress -> nodal force operator of a tet mesh
(reference src/diffelastic/deform.py:8-180), on csrc/deform.hip.

Same constructor, attributes and methods as the reference's class, with the reference's layouts, so a torch material
model sees the tensors it would see there:

  gradient_batch(u)            u (batch, nv, 3) -> F (batch, T*G, 3, 3),  F = sum_a u_a (x) B_a at every Gauss point
  stress_to_force_batch(P)     P (batch, T*G, 3, 3) -> f (batch, 3 nv),   f = sum_g w_g P_g B_g^T gathered per node
  gradient(u), stress_to_force(P)   the same for one column

What differs underneath: the two operators never read ``shape_func_deriv`` or ``stress_index``.  The reference keeps
B (T*G, N, 3) and an index map (T*G*N*3) resident (768 MB and 1.5 GB on the 105 456-element ord-2 mesh) and scatters
with atomics; the kernels rebuild inv(A_t) from the element's four corners, take dN/dL from a (G, N, 3) constant
table, and gather per node over an incidence list in a fixed order, so results are bitwise repeatable and a column's
result does not depend on the other columns of a call.  The three table attributes stay,
lazily, for API parity and for the tests.

Autograd: the operators are two ``torch.autograd.Function``s that are each other's adjoint - the backward of the
gradient is the force without the integration weights, the backward of the force is the gradient times them - so
gradients flow to ``u`` and to ``stress`` (any order of differentiation), in the operand's own dtype (the results are
float32 like the reference's whatever the operand's).  The vertices are CONSTANTS here: the
geometry loops differentiate through ``DiffSoundObj.get_vals`` (csrc/geomgrad.hip), not through these operators.

Memory: F and the stress are batch * T * G * 36 bytes each, and autograd keeps what the material model needs of
them; the force needs batch * T * N * 12 bytes of scratch.  HIP tensors only: there is no CPU fallback.
"""
import numpy as np
import torch

from .. import _hip, fem_tables
from .mesh import TetMesh

__all__ = ["Deform", "reference_tables"]


def reference_tables(order):
    """(D (G, N, 3) fp32, gauss_points (G, 4) fp32, gauss_weights (G,) fp32): D = dN/dL @ dL/dx of the reference
    (deform.py:47-67) at its (order+2)^3 Gauss points; dL/dx = [I3; -1 -1 -1], so D[..., k] = dN/dL_k - dN/dL_4,
    one fp32 rounding like the reference's matmul."""
    pts, w = fem_tables.gauss_rule(order)
    dn = fem_tables.shape_gradients(pts, order)  # fp32
    return np.ascontiguousarray(dn[:, :, :3] - dn[:, :, 3:4]), pts, w


class _Gradient(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, deform, weighted):
        ctx.deform, ctx.weighted, ctx.dtype = deform, weighted, u.dtype
        return deform._gradient(u, weighted)

    @staticmethod
    def backward(ctx, grad_F):
        d = ctx.deform
        g = _Force.apply(grad_F.contiguous(), d, ctx.weighted)
        return g.reshape(g.shape[0], -1, 3).to(ctx.dtype), None, None


class _Force(torch.autograd.Function):
    @staticmethod
    def forward(ctx, stress, deform, weighted):
        ctx.deform, ctx.weighted, ctx.dtype = deform, weighted, stress.dtype
        return deform._force(stress, weighted)

    @staticmethod
    def backward(ctx, grad_f):
        d = ctx.deform
        g = _Gradient.apply(grad_f.reshape(grad_f.shape[0], -1, 3).contiguous(), d, ctx.weighted)
        return g.to(ctx.dtype), None, None


class Deform:
    def __init__(self, tetmesh: TetMesh):
        v, t = tetmesh.vertices, tetmesh.tets
        if not (isinstance(v, torch.Tensor) and v.is_cuda and t.is_cuda):
            raise RuntimeError("diffsound_amd: Deform needs a mesh on the HIP device (there is no CPU fallback)")
        if tetmesh.order not in (1, 2) or t.dim() != 2 or t.shape[1] != fem_tables.NODES_PER_TET[tetmesh.order]:
            raise ValueError(f"Deform: order {tetmesh.order} with tets of shape {tuple(t.shape)} is not supported "
                             "(orders 1 and 2)")
        self.tetmesh = tetmesh
        self.device = tetmesh.device
        D, pts, w = reference_tables(tetmesh.order)
        self.gauss_points = torch.from_numpy(pts).to(self.device)  # (num_guass_points, 4)
        self.gauss_weights = torch.from_numpy(w).to(self.device)  # (num_guass_points)
        self.num_guass_points = self.gauss_points.shape[0]
        self.num_nodes_per_tet = t.shape[1]
        self.num_tets = t.shape[0]
        self._dtab = torch.from_numpy(D).to(self.device)
        nv, T, N = v.shape[0], self.num_tets, self.num_nodes_per_tet
        if T < 1 or nv < 1 or T >= 2 ** 31 // 30 or nv >= 2 ** 31 // 3:
            raise ValueError(f"Deform: unsupported mesh size (nv={nv}, T={T})")
        lo, hi = int(t.min()), int(t.max())
        if lo < 0 or hi >= nv:
            raise ValueError(f"Deform: node index out of range [0, {nv}): min {lo}, max {hi}")
        self._tets32 = t.to(torch.int32).contiguous()
        # node -> (tet, slot) incidences in CSR form, each node's entries in ascending t*N + a: the order of its sum
        flat = t.reshape(-1)
        self._inc = torch.sort(flat, stable=True).indices.to(torch.int32).contiguous()
        ptr = torch.zeros(nv + 1, dtype=torch.int64, device=self.device)
        ptr[1:] = torch.cumsum(torch.bincount(flat, minlength=nv), 0)
        self._inc_ptr = ptr.to(torch.int32).contiguous()
        self._checked = None
        self._verts()

    # ------------------------------------------------------------------ kernels
    def _verts(self):
        """The mesh's vertices as the kernels read them (fp32, contiguous).  The kernels do not guard against a
        singular A_t: the determinants are checked here, at construction and again whenever ``tetmesh.vertices`` is
        another tensor or has been written in place since the last check (its autograd version counter), so no call
        runs on shape gradients that were never checked; the lazy tables are dropped with them."""
        src = self.tetmesh.vertices
        if self._checked is not None and self._checked[0] is src and self._checked[1] == src._version:
            return self._checked[2]
        if src.device != self.device or src.dim() != 2 or src.shape[1] != 3 or int(self._inc_ptr.shape[0]) != src.shape[0] + 1:
            raise ValueError("Deform: the mesh's vertices changed shape or device after construction")
        v = src.detach().float().contiguous()
        self._checked = (src, src._version, v)
        for name in ("_shape_func_deriv", "_integration_weights"):
            self.__dict__.pop(name, None)
        det = torch.empty(self.num_tets, dtype=torch.float32, device=self.device)
        self._tables(det=det)
        if not bool(((det != 0) & torch.isfinite(det)).all()):
            self._checked = None
            bad = int(torch.nonzero((det == 0) | ~torch.isfinite(det))[0])
            raise ValueError(f"Deform: element {bad} is degenerate (det A = {float(det[bad])}): the shape gradients "
                             "inv(A) do not exist")
        return v

    def _mesh_args(self):
        v = self._verts()
        return v, (_hip.ptr(v), v.shape[0], _hip.ptr(self._tets32), self.num_tets, self.tetmesh.order,
                   _hip.ptr(self._dtab), _hip.ptr(self.gauss_weights))

    def _tables(self, sfd=None, intw=None, det=None):
        v, args = self._mesh_args()
        _hip.launch("ds_deform_tables", *args, _hip.ptr(sfd), _hip.ptr(intw), _hip.ptr(det), device=self.device)

    def _gradient(self, u, weighted):
        nv = self.tetmesh.vertices.shape[0]
        if not u.is_cuda or u.device != self.device:
            raise RuntimeError("diffsound_amd: Deform operands must live on the mesh's HIP device (no CPU fallback)")
        if u.dim() != 3 or u.shape[1] != nv or u.shape[2] != 3:
            raise ValueError(f"Deform.gradient_batch: u must be (batch, {nv}, 3), got {tuple(u.shape)}")
        u = u.detach().float().contiguous()
        F = torch.empty((u.shape[0], self.num_tets * self.num_guass_points, 3, 3), dtype=torch.float32, device=self.device)
        v, args = self._mesh_args()
        _hip.launch("ds_deform_gradient", *args, _hip.ptr(u), u.shape[0], int(bool(weighted)), _hip.ptr(F), device=self.device)
        return F

    def _force(self, stress, weighted):
        nv, tg = self.tetmesh.vertices.shape[0], self.num_tets * self.num_guass_points
        if not stress.is_cuda or stress.device != self.device:
            raise RuntimeError("diffsound_amd: Deform operands must live on the mesh's HIP device (no CPU fallback)")
        if stress.dim() != 4 or tuple(stress.shape[1:]) != (tg, 3, 3):
            raise ValueError(f"Deform.stress_to_force_batch: stress must be (batch, {tg}, 3, 3), got {tuple(stress.shape)}")
        P = stress.detach().float().contiguous()
        batch = P.shape[0]
        f = torch.empty((batch, 3 * nv), dtype=torch.float32, device=self.device)
        work = torch.empty(batch * self.num_tets * self.num_nodes_per_tet * 3, dtype=torch.float32, device=self.device)
        v, args = self._mesh_args()
        _hip.launch("ds_deform_force", *args, _hip.ptr(self._inc_ptr), _hip.ptr(self._inc), _hip.ptr(P), batch, int(bool(weighted)),
                    _hip.ptr(work), _hip.ptr(f), device=self.device)
        return f

    # ------------------------------------------------------------------ the reference's tables (lazy; not read above)
    @property
    def B_matrix(self):
        return self.shape_func_deriv

    @property
    def shape_func_deriv(self):
        """(num_tets*num_guass_points, num_nodes_per_tet, 3) float32 (reference :35-68)."""
        self._verts()  # drops a table of vertices that have changed since
        if not hasattr(self, "_shape_func_deriv"):
            B = torch.empty((self.num_tets * self.num_guass_points, self.num_nodes_per_tet, 3), dtype=torch.float32,
                            device=self.device)
            self._tables(sfd=B)
            self._shape_func_deriv = B
        return self._shape_func_deriv

    @property
    def integration_weights(self):
        """(num_tets*num_guass_points, 1, 1) float32 (reference :136-147)."""
        self._verts()
        if not hasattr(self, "_integration_weights"):
            w = torch.empty(self.num_tets * self.num_guass_points, dtype=torch.float32, device=self.device)
            self._tables(intw=w)
            self._integration_weights = w.reshape(-1, 1, 1)
        return self._integration_weights

    @property
    def stress_index(self):
        """(num_tets*num_guass_points*num_nodes_per_tet*3) long: global DOF of every entry of the reference's
        per-Gauss-point force tensor (reference :113-125)."""
        if not hasattr(self, "_stress_index"):
            base = self.tetmesh.tets.unsqueeze(1).expand(-1, self.num_guass_points, -1)
            idx = base.unsqueeze(-1) * 3 + torch.arange(3, device=self.device)
            self._stress_index = idx.reshape(-1).long()
        return self._stress_index

    # ------------------------------------------------------------------ operators
    def gradient_batch(self, u: torch.Tensor, weighted=False):
        """u (batch_num, num_nodes, 3) [or (num_nodes, 3)] -> (batch_num, num_tets*num_guass_points, 3, 3) float32.
        ``weighted`` (not in the reference) multiplies by the integration weights: the adjoint of the force."""
        if u.dim() == 2:
            u = u.unsqueeze(0)
        return _Gradient.apply(u, self, bool(weighted))

    def gradient(self, u: torch.Tensor):
        """u (num_nodes, 3) -> (num_tets*num_guass_points, 3, 3) float32."""
        return _Gradient.apply(u.unsqueeze(0), self, False).squeeze(0)

    def stress_to_force_batch(self, stress, weighted=True):
        """stress (batch_num, num_tets*num_guass_points, 3, 3) -> (batch_num, num_nodes*3) float32.
        ``weighted=False`` (not in the reference) drops the integration weights: the adjoint of the gradient."""
        return _Force.apply(stress, self, bool(weighted))

    def stress_to_force(self, stress):
        """stress (num_tets*num_guass_points, 3, 3) -> (num_nodes*3) float32."""
        return _Force.apply(stress.unsqueeze(0), self, True).squeeze(0)
