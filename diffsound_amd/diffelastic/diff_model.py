"""DiffSoundObj and material models - host-side mirror of reference src/diffelastic/diff_model.py.

Same names, constructor arguments, methods, attributes, return shapes/dtypes and autograd
behaviour (gradients reach ``material_model.{youngs,poisson}.probablity``), so
``experiments/material_*_train.py`` drop in.  What happens underneath is different:

  update_mass_matrix / update_stiff_matrix  -> one HIP assembly pass producing K_lambda, K_mu, M_s
       (K is exactly linear in the Lame parameters), reference :184-312
  eigen_decomposition_arpack (SciPy on the host, :335-369) -> device-resident block eigensolver with
       analytic rigid-mode deflation; same outputs: ``eigenvalues`` (mode_num,) fp64, ``U_hat``
       (n, mode_num) fp64 M-orthonormal, ``U_hat_full`` (n, mode_num+6) with the 6 rigid modes first
  get_undamped_freqs (:371-388)  ->  lambda_i + lam(theta) a_i + mu(theta) b_i - lambda_i m_i with the
       quadratic forms a_i = u^T K_lambda u, b_i = u^T K_mu u, m_i = u^T M u computed once per
       eigendecomposition (fp64) instead of a matrix-free (modes x Gauss points) sweep per epoch.

Custom material models.  ``mat_model`` may be any module with ``forward(F)`` and ``jacobian_F()`` like the reference's
(:314-328, :371-388).  A model WITHOUT a ``lame`` attribute is a custom model; the models above keep the path just
described.  For a custom model

  stiff_func          is the reference's chain ``deform.gradient_batch -> material_model(F) -> deform.stress_to_force_batch``
       on csrc/deform.hip: autograd reaches the model's parameters through torch and ``x`` through the kernels; the model
       is called with F of shape (batch, T*G, 3, 3) float32.  F and the stress take batch * T * G * 36 bytes each
       (G = (order+2)^3 Gauss points per element) and autograd keeps them, as in the reference; there is no chunking.
  update_stiff_matrix reads the tangent C = jacobian_F() at F = 0 (9x9, like :190) and needs it isotropic,
       C_ijkl = mu (d_ik d_jl + d_il d_jk) + lam d_ij d_kl (``isotropic_lame``); (lam, mu) then go through the same
       assembly and eigensolver as above.  Any other tangent raises NotImplementedError: the eigendecomposition with an
       anisotropic tangent is not built (``stiff_func`` works, and ``lobpcg_func(obj.stiff_func, obj.mass_matrix, ...)``
       takes a callable).
  get_undamped_freqs  is the reference's formula, lambda + diag(U^T stiff_func(U)) - lambda m, with U = U_hat.float().

Tangent models.  A model with a ``tangent()`` method (and no ``lame``) opts into the eigendecomposition with a general
constant tangent: ``tangent()`` returns the 9x9 d vec(P) / d vec(F) (row 3i+j, column 3k+l), ``elastic_tangent`` checks
that it is a valid elasticity tensor (finite, major and minor symmetry, positive definite Voigt matrix), and
``HipModalOps.set_tangent`` forms K_ab = C : H_ab from the geometry tensors the assembly already holds
(csrc/tangent.hip).  ``get_undamped_freqs`` is lambda + <C(theta), Q> - lambda m with the strain-energy moment tensors
Q_m (``HipModalOps.tangent_forms``) computed once per eigendecomposition: u^T K(C) u = <C, Q> exactly, so autograd
reaches the model's parameters through an 81-term dot product per mode.  ``stiff_func`` stays the matrix-free chain
above.  ``TrainableOrthotropic`` and ``fixed_tangent`` are such models.  The geometry gradient of ``get_vals`` is not
built for them (ds_geometry_grad is written for (lam, mu)); ``get_vals_differentiable`` has it.

Joint read-out.  In the reference both read-outs are differentiable in the vertices AND the material parameters at once
(:390-399 through ``stiff_matrix`` / ``mass_matrix`` of :184-220, :222-312; :371-388 through ``stiff_func``, the Deform
tables and ``transform_matrix``).  ``get_vals_differentiable`` is that bracket, lambda + u^T K(theta, x) u - lambda u^T
M(x) u, as ONE autograd node over (vertices, C or (lam, mu)): the material gradient is sum_i g_i Q_i (or g.a, g.b), the
vertex gradient comes from ds_geometry_grad_tangent (csrc/geomgrad.hip: any tangent, no atomics).
``get_undamped_freqs`` goes through it when the vertices require a gradient, so a shape - or a shape and a material
together - can be fitted through the oscillator and the spectral loss, for orthotropic models too.
"""
import numpy as np
import torch
import torch.nn as nn

from ..ddsp.oscillator import WeightedParam
from ..lobpcg.modal_solver import ModalSolver, SolverConfig, tuned_config
from ..hip_ops import HipModalOps, isotropic_tangent
from ..modal_ops import TetSystem
from .material_model import Material, MatSet
from .mesh import TetMesh


def _lame(E, nu):
    return E * nu / ((1 + nu) * (1 - 2 * nu)), E / (2 * (1 + nu))


class FixedLinear(nn.Module):
    """Linear elasticity with fixed (E, nu) (reference :17-48)."""

    def __init__(self, mat: Material):
        super().__init__()
        self.youngs = mat.youngs
        self.poisson = mat.poisson
        self.mat = mat

    def lame(self):
        return _lame(torch.tensor(float(self.youngs), dtype=torch.float64),
                     torch.tensor(float(self.poisson), dtype=torch.float64))

    def get_stress(self, F):
        lam, mu = _lame(self.youngs, self.poisson)
        tr = F.diagonal(dim1=-2, dim2=-1).sum(-1)
        return mu * (F + F.transpose(-1, -2)) + lam * tr[..., None, None] * torch.eye(3, device=F.device, dtype=F.dtype)

    def forward(self, F):
        return self.get_stress(F)

    def jacobian_F(self):
        """Constant d vec(P)/d vec(F), (1,3,3,1,3,3) like torch.autograd.functional.jacobian (:45-48)."""
        lam, mu = _lame(float(self.youngs), float(self.poisson))
        J = torch.zeros(3, 3, 3, 3, dtype=torch.float64)
        for i in range(3):
            for j in range(3):
                J[i, j, i, j] += mu
                J[i, j, j, i] += mu
                J[i, i, j, j] += lam
        return J.reshape(1, 3, 3, 1, 3, 3)


class TrainableLinear(nn.Module):
    """(E, nu) as softplus-weighted combinations of 16 bins (reference :51-96)."""

    def __init__(self, mat: Material, bin_num=16, baseline=False):
        super().__init__()
        self.youngs_list = torch.exp(torch.linspace(np.log(mat.youngs / 10), np.log(mat.youngs * 10), bin_num))
        if baseline:
            self.poisson_list = torch.linspace(mat.poisson, mat.poisson, 1)
        else:
            self.poisson_list = torch.linspace(0.01, 0.499, bin_num)
        self.youngs = WeightedParam(self.youngs_list)
        self.poisson = WeightedParam(self.poisson_list)
        self.mat = mat

    def lame(self):
        """(lambda_L, mu) as fp64 0-dim tensors carrying autograd to the bin logits."""
        return _lame(self.youngs().double(), self.poisson().double())

    def get_stress(self, F):
        lam, mu = _lame(self.youngs(), self.poisson())
        tr = F.diagonal(dim1=-2, dim2=-1).sum(-1)
        return mu * (F + F.transpose(-1, -2)) + lam * tr[..., None, None] * torch.eye(3, device=F.device, dtype=F.dtype)

    def forward(self, F):
        return self.get_stress(F)

    def jacobian_F(self):
        lam, mu = _lame(float(self.youngs()), float(self.poisson()))
        J = torch.zeros(3, 3, 3, 3, dtype=torch.float64)
        for i in range(3):
            for j in range(3):
                J[i, j, i, j] += mu
                J[i, j, j, i] += mu
                J[i, i, j, j] += lam
        return J.reshape(1, 3, 3, 1, 3, 3)


_ANISOTROPIC = ("diffsound_amd: the material model's tangent jacobian_F() is not isotropic ({why}); the "
                "eigendecomposition with an anisotropic tangent is not built.  stiff_func works for this model, and "
                "lobpcg_func(obj.stiff_func, obj.mass_matrix, ...) takes a callable.")


def isotropic_lame(C, rtol=1e-5):
    """(lam, mu) of a 9x9 tangent d vec(P) / d vec(F) (row 3i+j, column 3k+l) of the isotropic form
    C_ijkl = mu (d_ik d_jl + d_il d_jk) + lam d_ij d_kl: lam = the mean of C_iijj, mu = the mean of C_ijij over
    i != j.  Raises NotImplementedError when C differs from that form by more than rtol * max|C| anywhere - a test of
    form, not a measurement: the margin is for a model whose parameters are fp32.  Pure host arithmetic in fp64."""
    C = np.asarray(C.detach().cpu() if isinstance(C, torch.Tensor) else C, dtype=np.float64)
    if C.size != 81 or not np.isfinite(C).all():
        raise NotImplementedError(_ANISOTROPIC.format(why=f"81 finite entries expected, got shape {C.shape}"))
    C4 = C.reshape(3, 3, 3, 3)
    off = [(i, j) for i in range(3) for j in range(3) if i != j]
    lam = float(np.mean([C4[i, i, j, j] for i, j in off]))
    mu = float(np.mean([C4[i, j, i, j] for i, j in off]))
    d = np.eye(3)
    iso = mu * (np.einsum("ik,jl->ijkl", d, d) + np.einsum("il,jk->ijkl", d, d)) + lam * np.einsum("ij,kl->ijkl", d, d)
    scale = float(np.abs(C4).max())
    resid = float(np.abs(C4 - iso).max())
    if scale == 0.0 or resid > rtol * scale:
        raise NotImplementedError(_ANISOTROPIC.format(why=f"residual {resid:.3e} against max|C| = {scale:.3e}"))
    return lam, mu


class _TangentStress(torch.autograd.Function):
    """vec(P) = C vec(F) on (..., 9) rows in F's dtype, with the gradient on C summed in fp64: its 81 entries are sums over
    every Gauss point of every column (batch * T * G rows), which a float32 product loses digits on."""

    ROWS = 1 << 18  # rows per fp64 slice of the backward

    @staticmethod
    def forward(ctx, F9, C):
        Cf = C.to(F9.device, F9.dtype)
        ctx.save_for_backward(F9, Cf)
        ctx.c_like = (C.device, C.dtype)
        return F9 @ Cf.transpose(0, 1)

    @staticmethod
    def backward(ctx, g):
        F9, Cf = ctx.saved_tensors
        gF = g @ Cf if ctx.needs_input_grad[0] else None
        gC = None
        if ctx.needs_input_grad[1]:
            g2, f2 = g.reshape(-1, 9), F9.reshape(-1, 9)
            gC = torch.zeros((9, 9), dtype=torch.float64, device=g.device)
            for r0 in range(0, g2.shape[0], _TangentStress.ROWS):
                gC += g2[r0:r0 + _TangentStress.ROWS].double().transpose(0, 1) @ f2[r0:r0 + _TangentStress.ROWS].double()
            gC = gC.to(*ctx.c_like)
        return gF, gC


def _tangent_stress(F, C):
    return _TangentStress.apply(F.reshape(*F.shape[:-2], 9), C).reshape(F.shape)


_VOIGT_ROWS = (0, 4, 8, 5, 2, 1)  # 3i+j of (ij) = 11, 22, 33, 23, 13, 12
_VOIGT_OF = (0, 5, 4, 5, 1, 3, 4, 3, 2)  # the Voigt index of 3i+j


def elastic_tangent(C, rtol=1e-5):
    """Validate a 9x9 tangent d vec(P) / d vec(F) (row 3i+j, column 3k+l) for the eigensolver and return it as fp64
    NumPy, symmetrised exactly.  ValueError names the failed condition:
      (i)   81 finite entries, max|C| > 0;
      (ii)  major symmetry C_ijkl = C_klij within rtol * max|C| - without it K is not symmetric;
      (iii) minor symmetry C_ijkl = C_ijlk within rtol * max|C| - without it rotations are not in K's null space and the
            analytic rigid-mode deflation would be wrong;
      (iv)  the 6x6 Voigt matrix of C is positive definite (a Cholesky factorisation succeeds).
    ``rtol`` is a test of form, as ``isotropic_lame``'s: the margin is for a model whose parameters are fp32."""
    C = np.asarray(C.detach().cpu() if isinstance(C, torch.Tensor) else C, dtype=np.float64)
    if C.size != 81:
        raise ValueError(f"elastic_tangent: shape: a 9x9 tangent (81 entries) expected, got shape {C.shape}")
    C = C.reshape(9, 9)
    if not np.isfinite(C).all():
        raise ValueError("elastic_tangent: finite: the tangent has entries that are not finite")
    scale = float(np.abs(C).max())
    if scale == 0.0:
        raise ValueError("elastic_tangent: zero: max|C| = 0")
    C4 = C.reshape(3, 3, 3, 3)
    major = float(np.abs(C4 - C4.transpose(2, 3, 0, 1)).max())
    if major > rtol * scale:
        raise ValueError(f"elastic_tangent: major symmetry C_ijkl = C_klij broken by {major:.3e} against max|C| = "
                         f"{scale:.3e}: K would not be symmetric")
    minor = max(float(np.abs(C4 - C4.transpose(0, 1, 3, 2)).max()), float(np.abs(C4 - C4.transpose(1, 0, 2, 3)).max()))
    if minor > rtol * scale:
        raise ValueError(f"elastic_tangent: minor symmetry C_ijkl = C_ijlk broken by {minor:.3e} against max|C| = "
                         f"{scale:.3e}: rotations would not be in the null space of K")
    # exact symmetrisation: (ij), then (kl), then the pairs - every step is a commutative two-term mean
    C4 = 0.5 * (C4 + C4.transpose(1, 0, 2, 3))
    C4 = 0.5 * (C4 + C4.transpose(0, 1, 3, 2))
    C4 = 0.5 * (C4 + C4.transpose(2, 3, 0, 1))
    C = np.ascontiguousarray(C4.reshape(9, 9))
    voigt = C[np.ix_(_VOIGT_ROWS, _VOIGT_ROWS)]
    try:
        np.linalg.cholesky(voigt)
    except np.linalg.LinAlgError:
        raise ValueError("elastic_tangent: positive definite: the 6x6 Voigt matrix of the tangent has no Cholesky "
                         f"factor (smallest eigenvalue {float(np.linalg.eigvalsh(voigt)[0]):.3e})") from None
    return C


class TrainableOrthotropic(nn.Module):
    """Orthotropic linear elasticity with nine trainable engineering constants E1, E2, E3, nu12, nu13, nu23, G12, G13,
    G23 (``NAMES``), each its initial value times exp(log_scale[i]).  They start at the isotropic values of ``mat``
    (E, nu, G = E / (2 (1 + nu))), so at zero ``log_scale`` the tangent is the shipped isotropic one.  ``axes``: a 3x3
    rotation whose columns are the material axes in the mesh's frame (default: identity)."""

    NAMES = ("E1", "E2", "E3", "nu12", "nu13", "nu23", "G12", "G13", "G23")

    def __init__(self, mat: Material, axes=None):
        super().__init__()
        E, nu = float(mat.youngs), float(mat.poisson)
        G = E / (2 * (1 + nu))
        self.register_buffer("initial", torch.tensor([E, E, E, nu, nu, nu, G, G, G], dtype=torch.float64))
        self.register_buffer("axes", torch.eye(3, dtype=torch.float64) if axes is None
                             else torch.as_tensor(axes, dtype=torch.float64).reshape(3, 3).clone())
        self.log_scale = nn.Parameter(torch.zeros(9, dtype=torch.float64))
        self.mat = mat

    def constants(self):
        """The nine engineering constants (fp64, autograd to ``log_scale``), in the order of ``NAMES``."""
        return self.initial * torch.exp(self.log_scale)

    def tangent(self):
        """9x9 d vec(P) / d vec(F) in fp64 with autograd to ``log_scale``: the inverse of the 6x6 compliance, expanded
        with both minor symmetries and rotated by ``axes``."""
        E1, E2, E3, n12, n13, n23, G12, G13, G23 = self.constants().unbind(0)
        zero = torch.zeros((), dtype=torch.float64, device=E1.device)
        S = torch.stack([torch.stack([1 / E1, -n12 / E1, -n13 / E1, zero, zero, zero]),
                         torch.stack([-n12 / E1, 1 / E2, -n23 / E2, zero, zero, zero]),
                         torch.stack([-n13 / E1, -n23 / E2, 1 / E3, zero, zero, zero]),
                         torch.stack([zero, zero, zero, 1 / G23, zero, zero]),
                         torch.stack([zero, zero, zero, zero, 1 / G13, zero]),
                         torch.stack([zero, zero, zero, zero, zero, 1 / G12])])
        Cv = torch.linalg.inv(S)
        Cv = 0.5 * (Cv + Cv.transpose(0, 1))
        idx = torch.tensor(_VOIGT_OF, device=Cv.device)
        C4 = Cv[idx][:, idx].reshape(3, 3, 3, 3)
        R = self.axes
        return torch.einsum("ia,jb,kc,ld,abcd->ijkl", R, R, R, R, C4).reshape(9, 9)

    def forward(self, F):
        """P = C : F."""
        return _tangent_stress(F, self.tangent())

    def jacobian_F(self):
        return self.tangent().detach().reshape(1, 3, 3, 1, 3, 3)


def fixed_tangent(C):
    """A material-model class whose ``tangent()`` is the constant 9x9 tangent C (row 3i+j, column 3k+l):
    ``DiffSoundObj(..., mat_model=fixed_tangent(C))``."""
    C64 = torch.as_tensor(np.asarray(C.detach().cpu() if isinstance(C, torch.Tensor) else C, dtype=np.float64)).reshape(9, 9).clone()

    class FixedTangent(nn.Module):
        def __init__(self, mat: Material):
            super().__init__()
            self.register_buffer("C", C64.clone())
            self.mat = mat

        def tangent(self):
            return self.C

        def forward(self, F):
            return _tangent_stress(F, self.C)

        def jacobian_F(self):
            return self.C.detach().reshape(1, 3, 3, 1, 3, 3)

    return FixedTangent


def build_model(mesh_dir, mode_num, order, mat, task, vertices=None, tets=None, scale_range=None, init_scale=None):
    """reference :98-113."""
    if task == "material" or task == "mat_baseline":
        mat_model = TrainableLinear
    elif task == "gt":
        mat_model = FixedLinear
    else:
        raise ValueError("task not defined")
    model = DiffSoundObj(mesh_dir=mesh_dir, mode_num=mode_num, order=order, mat=mat, mat_model=mat_model, task=task,
                         vertices=vertices, tets=tets)
    if task == "material" or task == "mat_baseline":
        model.init_material_coeffs()
    return model


class _GetVals(torch.autograd.Function):
    """vals_i = lambda_i + u_i^T K(x) u_i - lambda_i u_i^T M(x) u_i with detached (lambda_i, u_i): forward from the
    solver's fp64 quadratic forms, backward to the node coordinates by the ds_geometry_grad kernel."""

    @staticmethod
    def forward(ctx, vertices, obj, vals):
        ctx.obj = obj
        return vals.clone()

    @staticmethod
    def backward(ctx, gout):
        obj = ctx.obj
        g = gout.reshape(-1).double()
        lam, mu = obj._ops.lame
        grad = obj.system.geometry_grad(obj.last_result.vectors, g, g * obj.eigenvalues, lam, mu)
        return grad.to(obj.tetmesh.vertices.dtype), None, None


class _Bracket(torch.autograd.Function):
    """bracket_i = lambda_i + u_i^T K(theta, x) u_i - lambda_i u_i^T M(x) u_i with detached (lambda_i, u_i), as one node
    over (vertices, material): ``mat`` is the 9 x 9 tangent C, or the pair (lam, mu).  Forward from the quadratic forms of
    the last eigendecomposition (Q, or a and b, and m).  Backward: sum_i g_i Q_i (or g.a, g.b) to the material, and to the
    vertices ds_geometry_grad_tangent with gk = g, gm = g * lambda and the detached C of the forward."""

    @staticmethod
    def forward(ctx, vertices, obj, *mat):
        ev, dev = obj.eigenvalues, obj.eigenvalues.device
        if len(mat) == 1:
            ctx.forms = (obj._Q,)
            ctx.C = mat[0].detach().cpu().double().numpy().reshape(9, 9).copy()
            form = (mat[0].detach().to(device=dev, dtype=torch.float64) * obj._Q).sum((-1, -2))
        else:
            lam, mu = (x.detach().to(device=dev, dtype=torch.float64) for x in mat)
            ctx.forms = (obj._a, obj._b)
            ctx.C = isotropic_tangent(float(lam), float(mu))
            form = lam * obj._a + mu * obj._b
        ctx.sys, ctx.ev, ctx.vectors = obj.system, ev, obj.last_result.vectors
        ctx.like = [(x.device, x.dtype, x.shape) for x in mat]
        ctx.vdtype = vertices.dtype
        return (ev + form - ev * obj._m).unsqueeze(1)

    @staticmethod
    def backward(ctx, gout):
        g = gout.reshape(-1).double()
        gv = None
        if ctx.needs_input_grad[0]:
            V = ctx.vectors.float().contiguous()  # the fp32 vectors the forms belong to
            gv = ctx.sys.geometry_grad_tangent(V, g, g * ctx.ev, ctx.C).to(ctx.vdtype)
        gmat = []
        for k, (dev, dtype, shape) in enumerate(ctx.like):
            if not ctx.needs_input_grad[2 + k]:
                gmat.append(None)
            elif len(ctx.like) == 1:
                gmat.append((g[:, None, None] * ctx.forms[0]).sum(0).reshape(shape).to(device=dev, dtype=dtype))
            else:
                gmat.append((g * ctx.forms[k]).sum().reshape(shape).to(device=dev, dtype=dtype))
        return (gv, None, *gmat)


class DiffSoundObj:
    def __init__(self, vertices=None, tets=None, mode_num=16, mat=MatSet.Ceramic, order=1, mat_model=FixedLinear,
                 task=None, mesh_dir=None, solver_config=None):
        if mesh_dir:
            self.mesh_dir = mesh_dir
            self.tetmesh = TetMesh.from_triangle_mesh(mesh_dir).to_high_order(order)
        else:
            if not vertices.is_cuda:
                raise RuntimeError("diffsound_amd: vertices/tets must be HIP tensors (there is no CPU fallback)")
            self.tetmesh = TetMesh(vertices, tets).to_high_order(order)
        if task == "mat_baseline":
            self.material_model = mat_model(Material(mat), baseline=True)
        else:
            self.material_model = mat_model(Material(mat))
        self.mode_num = mode_num
        self.U_hat_full = None
        self.task = task
        self.solver_config = solver_config or tuned_config(order)
        self._system = None
        self._ops = None
        self._warm = None
        self._sparse_cache = {}
        self.last_result = None
        self._deform = None

    # ------------------------------------------------------------------ parameters
    def parameters(self):
        if self.task == "material":
            return self.material_model.parameters()
        if self.task == "mat_baseline":
            return self.material_model.youngs.parameters()
        return None

    def init_material_coeffs(self, steps=5000):
        """Fit the bin logits so that (E, nu) start at the material-table values (reference :154-180)."""
        opt = torch.optim.Adam(self.material_model.parameters(), lr=5e-3)
        gt_y, gt_p = self.material_model.mat.youngs, self.material_model.mat.poisson
        for _ in range(steps):
            opt.zero_grad()
            loss = (self.material_model.youngs() - gt_y) ** 2 / gt_y ** 2 + \
                   (self.material_model.poisson() - gt_p) ** 2 / gt_p ** 2
            loss.backward()
            opt.step()

    # ------------------------------------------------------------------ assembly
    @property
    def system(self):
        if self._system is None:
            self._system = TetSystem(self.tetmesh.vertices, self.tetmesh.tets, self.tetmesh.order,
                                     self.material_model.mat.density)
        return self._system

    @property
    def deform(self):
        """The Deform operators of the current ``tetmesh`` (reference :135), built on first use."""
        if self._deform is None or self._deform.tetmesh is not self.tetmesh:
            from .deform import Deform

            self._deform = Deform(self.tetmesh)
        return self._deform

    @property
    def _custom_material(self):
        return not hasattr(self.material_model, "lame")

    @property
    def _tangent_model(self):
        """A model with ``tangent()`` and no ``lame``: the eigendecomposition with a general tangent."""
        return self._custom_material and hasattr(self.material_model, "tangent")

    def _current_lame(self):
        if self._custom_material:  # the tangent at F = 0, as the reference's assembly reads it (:190)
            return isotropic_lame(self.material_model.jacobian_F().reshape(9, 9).double())
        lam, mu = self.material_model.lame()
        return float(lam), float(mu)

    def update_mass_matrix(self, density=None):
        """Numeric assembly (M_s together with K_lambda, K_mu) (reference :222-312)."""
        if density is not None and self._system is not None and density != self._system.density:
            self._system = None
        if self._system is None:
            _ = self.system
        else:
            self._system.assemble(self.tetmesh.vertices)
        self._sparse_cache.clear()

    def update_stiff_matrix(self, assemble_batch_size=None):
        """K = lam K_lambda + mu K_mu for the current material (reference :184-220)."""
        if self._tangent_model:  # validated on the host before anything is launched
            C = elastic_tangent(self.material_model.tangent())
            if self._ops is None or self._ops.sys is not self.system:
                self._ops = HipModalOps(self.system, tangent=C)
            else:
                self._ops.set_tangent(C)
            self._sparse_cache.clear()
            return
        lam, mu = self._current_lame()
        if self._ops is None or self._ops.sys is not self.system:
            self._ops = HipModalOps(self.system, lam, mu)
        else:
            self._ops.set_material(lam, mu)
        self._sparse_cache.clear()

    def _bsr_to_sparse(self, which):
        """torch sparse CSR fp64 view of the assembled matrices (API compatibility: callers read
        ``stiff_matrix`` / ``mass_matrix`` as torch sparse tensors)."""
        if which not in self._sparse_cache:
            s = self.system
            if which == "K" and self._ops is not None and self._ops.lame is None:  # a tangent: the blocks of C : H
                blocks = self._ops.k64c.reshape(-1, 3, 3)
            elif which == "K":
                lam, mu = self._ops.lame if self._ops is not None else self._current_lame()
                blocks = (lam * s.klam + mu * s.kmu).reshape(-1, 3, 3)
            else:
                blocks = s.ms[:, None, None] * torch.eye(3, dtype=torch.float64, device=s.device)
            coo = torch.sparse_bsr_tensor(s.rowptr.long(), s.colidx.long(), blocks, size=(s.n, s.n)).to_sparse_coo().coalesce()
            if s.perm is not None:  # internal (Morton) -> the caller's DOF numbering
                idx = coo.indices()
                ext = 3 * s.perm[idx // 3] + idx % 3
                coo = torch.sparse_coo_tensor(ext, coo.values(), (s.n, s.n))
            self._sparse_cache[which] = coo.coalesce()
        return self._sparse_cache[which]

    @property
    def stiff_matrix(self):
        return self._bsr_to_sparse("K")

    @property
    def mass_matrix(self):
        return self._bsr_to_sparse("M")

    # ------------------------------------------------------------------ eigen decomposition
    def eigen_decomposition(self):
        """reference :330-369 (assembly + eigsh(k=mode_num+6, sigma=20000) + drop 6 rigid pairs)."""
        self.update_mass_matrix(self.material_model.mat.density)
        self.update_stiff_matrix()
        self.eigen_decomposition_arpack()

    def eigen_decomposition_arpack(self):
        """Name kept for drop-in compatibility; runs the device-resident block eigensolver."""
        ops = self._ops
        solver = ModalSolver(ops, self.solver_config)
        solver.vector_forms = True  # (the quadratic forms below belong to the fp32 vectors U_hat is made of)
        res = solver.solve(self.mode_num, X0=self._warm)
        self._warm = res.block_vectors
        self.last_result = res
        self.eigenvalues = res.eigenvalues
        # the solver works in the system's internal (Morton) node order; hand modes back in the caller's
        self.U_hat = self.system.rows_to_external(res.vectors).double()
        rigid = self.system.rows_to_external(ops.rigid[:, :6]).double()
        self.U_hat_full = torch.cat([rigid, self.U_hat], dim=1)
        self._a, self._b, self._m = res.a_lambda, res.b_mu, res.m_diag
        if self._tangent_model:
            # Q and m of the SAME fp32 vectors: the bracket <C, Q> - lambda m is then second order in their error
            # (an fp64 refinement returns fp64 vectors: their fp32 rounding, what U_hat.float() holds)
            V = res.vectors.float().contiguous()
            self._Q = ops.tangent_forms(V)
            MV = torch.empty(V.shape, dtype=torch.float64, device=V.device)
            ops._spmm(3, ops.sys.ms, V, MV)
            self._m = (V.double() * MV).sum(0)

    # ------------------------------------------------------------------ differentiable read-outs
    def get_vals_differentiable(self):
        """The bracket lambda + u^T K(theta, x) u - lambda u^T M(x) u of the last eigendecomposition, (mode_num, 1) float64,
        with gradient to the material parameters and, when ``tetmesh.vertices.requires_grad``, to the vertices - both at
        once, as in the reference (:371-399).  For the shipped (lam, mu) models and for tangent models."""
        if self._custom_material and not self._tangent_model:
            raise NotImplementedError("diffsound_amd: get_vals_differentiable() needs a model with lame() or tangent(): the "
                                      "joint vertex / material read-out of a custom model whose stiffness is only known "
                                      "through forward(F) is not built (get_undamped_freqs() reaches its parameters)")
        mat = (self.material_model.tangent(),) if self._tangent_model else tuple(self.material_model.lame())
        return _Bracket.apply(self.tetmesh.vertices, self, *mat)

    def get_undamped_freqs(self):
        """(mode_num, 1) float32; gradient -> material parameters (reference :371-388) and, when the vertices require a
        gradient (and the model has ``lame`` or ``tangent``), to the vertices as well: ``get_vals_differentiable``."""
        pred = self.eigenvalues
        if self.task != "gt" and self.tetmesh.vertices.requires_grad and (self._tangent_model or not self._custom_material):
            pred = self.get_vals_differentiable().squeeze(1)
        elif self.task != "gt" and self._tangent_model:  # lambda + <C(theta), Q> - lambda m: autograd through torch alone
            C = self.material_model.tangent().to(device=pred.device, dtype=torch.float64)
            pred = pred + (C * self._Q).sum((-1, -2)) - pred * self._m
        elif self.task != "gt" and self._custom_material:  # the reference's matrix-free bracket (:381-387)
            U = self.U_hat.float()
            pred = pred + (U * self.stiff_func(U)).sum(0) - pred * self._m
        elif self.task != "gt":
            lam, mu = self.material_model.lame()  # autograd leaves live on the host like the reference's
            dev = pred.device
            pred = pred + (lam.to(dev) * self._a + mu.to(dev) * self._b) - pred * self._m
        return (torch.sqrt(pred) / 2 / np.pi).float().unsqueeze(1)

    def get_vals(self):
        """lambda + diag(U^T K U) - lambda diag(U^T M U), (mode_num, 1) float32 (reference :390-399).  Gradient to the
        vertices for (lam, mu) models only; ``get_vals_differentiable`` is the same bracket with gradient to the vertices
        and the material parameters, for tangent models too."""
        if self._tangent_model:
            if self.tetmesh.vertices.requires_grad:
                raise NotImplementedError("diffsound_amd: get_vals() of a tangent model has no gradient to the vertices: "
                                          "the geometry gradient (ds_geometry_grad) is written for (lam, mu), and that of an "
                                          "anisotropic tangent is not built")
            C = self.material_model.tangent().detach().to(device=self.eigenvalues.device, dtype=torch.float64)
            return (self.eigenvalues + (C * self._Q).sum((-1, -2)) - self.eigenvalues * self._m).float().unsqueeze(1)
        lam, mu = self._ops.lame
        pred = (self.eigenvalues + (lam * self._a + mu * self._b) - self.eigenvalues * self._m).float().unsqueeze(1)
        if self.tetmesh.vertices.requires_grad:  # geometry tasks: gradient -> vertices
            pred = _GetVals.apply(self.tetmesh.vertices, self, pred)
        return pred

    def stiff_func(self, x_in):
        """K(theta) x with autograd to the material parameters (reference :314-328, matrix-free there)."""
        x = x_in.unsqueeze(1) if x_in.dim() == 1 else x_in
        if self._custom_material:  # the reference's chain; F and the stress are x.shape[1] * T * G * 36 bytes each
            F = self.deform.gradient_batch(x.transpose(0, 1).reshape(x.shape[1], -1, 3))
            force = self.deform.stress_to_force_batch(self.material_model(F)).transpose(0, 1)
            return force.squeeze(1) if x_in.dim() == 1 else force
        ops = self._ops
        xf = self.system.rows_to_internal(x.detach().float()).contiguous()
        pad = (-xf.shape[1]) % 4
        if pad:
            xf = torch.cat([xf, torch.zeros((xf.shape[0], pad), device=xf.device)], dim=1).contiguous()
        yl = torch.empty(xf.shape, dtype=torch.float64, device=xf.device)
        ym = torch.empty_like(yl)
        ops._spmm(2, ops.sys.klam, xf, yl)
        ops._spmm(2, ops.sys.kmu, xf, ym)
        lam, mu = self.material_model.lame()
        out = self.system.rows_to_external(lam.to(yl.device) * yl + mu.to(yl.device) * ym)[:, : x.shape[1]].to(x_in.dtype)
        return out.squeeze(1) if x_in.dim() == 1 else out
