"""Helmholtz boundary elements for sound radiation: drop-in for the reference's ``src/diffelastic/bem.py``.

The reference builds its operators with bempp-cl (+ numba); here the three hot paths are HIP kernels of
``libdiffsound_hip.so`` (csrc/bem.hip): per-face geometry, the Galerkin assembly of ``A = -1/2 M + K`` together
with ``rhs = V g``, the dense complex GEMV of the GMRES and the potential at listener points.

Formulation (as the reference's, bem.py:36-61): exterior Neumann problem in direct form, piecewise-constant
("DP0") space, one coefficient per triangle, normals by the right-hand rule on the vertex order,

    (-1/2 M + K) u = V g           on the surface,   g = du/dn (given), u the surface pressure,
    u(p) = -S g (p) + D u (p)      at a point p off the surface,

with ``G = e^{ikr} / (4 pi r)``.  Like the reference's, the equation is singular at the interior Dirichlet
eigenfrequencies of the object (on a sphere of radius a: ka = pi, 4.493, 2 pi, ...): near them the solve needs
many more GMRES iterations and the solution is polluted by the interior resonance.  Burton-Miller or CHIEF is not
implemented (DESIGN.md "Sound radiation (BEM)").

GMRES: restarted GMRES(``GMRES_RESTART``) on the device, on the strong form ``diag(1/area) A`` (the same
solution), relative tolerance 1e-6 as the reference's, at most ``GMRES_MAXITER`` iterations; ``gmres_info`` keeps
the iteration count and the final true relative residual.  A solve that does not converge warns.

Faces are kept in Morton order of their centroids inside the model (near pairs cluster, so the closed-form branch
of the assembly stays in a few waves per row band); everything the caller sees is in the caller's face order.

Beyond the reference: ``surface_of`` (boundary triangles of a tet mesh), ``mode_neumann`` (normal velocity of the
modes per face) and ``modal_transfer`` (complex pressure at listener points per mode of a ``DiffSoundObj``).
"""
import warnings

import numpy as np
import torch

from .. import _hip

GMRES_RESTART = 60
GMRES_MAXITER = 2000
GMRES_TOL = 1e-6
# the dense N x N complex64 operator (8 N^2 bytes) may use at most this much device memory: 8 GiB, N <= 32 768 faces
# (there is no hierarchical-matrix path)
BEM_MEMORY_BUDGET_BYTES = 8 << 30
FACE_RECORD = 48  # DS_BEM_FACE_RECORD of include/diffsound_hip.h


class Grid:
    """The surface as the reference's ``obj_to_grid`` hands it to bempp: ``vertices`` (3, n) float64 and
    ``elements`` (3, m) uint32 (bempp's layout), already validated."""

    def __init__(self, vertices, elements):
        self.vertices = vertices
        self.elements = elements

    @property
    def number_of_elements(self):
        return self.elements.shape[1]

    @property
    def number_of_vertices(self):
        return self.vertices.shape[1]


class GridFunction:
    """Face data of a DP0 space: ``coefficients`` is an (m,) complex array in the caller's face order."""

    def __init__(self, grid, coefficients):
        self.grid = grid
        self.coefficients = coefficients


class DP0Space:
    def __init__(self, grid):
        self.grid = grid
        self.global_dof_count = grid.number_of_elements


def _to_numpy(a):
    if isinstance(a, torch.Tensor):
        return a.detach().cpu().numpy()
    return np.asarray(a)


def obj_to_grid(vertices, elements):
    """(n, 3) vertices and (m, 3) triangles (numpy or torch) -> ``Grid``.  ValueError on wrong shapes, indices out of
    range, non-finite coordinates or degenerate triangles."""
    v = _to_numpy(vertices)
    e = _to_numpy(elements)
    if v.ndim != 2 or v.shape[1] != 3 or v.shape[0] < 3:
        raise ValueError(f"obj_to_grid: vertices must be an (n, 3) array with n >= 3, got shape {v.shape}")
    if e.ndim != 2 or e.shape[1] != 3 or e.shape[0] < 1:
        raise ValueError(f"obj_to_grid: elements must be an (m, 3) array with m >= 1, got shape {e.shape}")
    if not np.issubdtype(e.dtype, np.integer):
        raise ValueError(f"obj_to_grid: elements must be integer indices, got {e.dtype}")
    v = v.astype(np.float64)
    if not np.isfinite(v).all():
        raise ValueError("obj_to_grid: vertices hold non-finite coordinates")
    e = e.astype(np.int64)
    if e.min() < 0 or e.max() >= v.shape[0]:
        raise ValueError(f"obj_to_grid: element indices out of range [0, {v.shape[0]})")
    p = v[e]
    cr = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    twice_area = np.linalg.norm(cr, axis=1)
    h2 = np.max(np.stack([((p[:, a] - p[:, b]) ** 2).sum(1) for a, b in ((0, 1), (1, 2), (2, 0))]), axis=0)
    bad = ~(twice_area > 1e-6 * h2) | (h2 <= 0)
    if bad.any():
        raise ValueError(f"obj_to_grid: {int(bad.sum())} degenerate triangle(s), first at index {int(np.argmax(bad))}")
    return Grid(np.ascontiguousarray(v.T), np.ascontiguousarray(e.T.astype(np.uint32)))


def _morton_order(c):
    """Permutation that puts the (m, 3) centroids ``c`` (torch) in Morton (Z-curve) order, 10 bits per axis."""
    lo, hi = c.min(0).values, c.max(0).values
    q = ((c - lo) / torch.clamp(hi - lo, min=1e-30) * 1023).round().long().clamp(0, 1023)
    code = torch.zeros(c.shape[0], dtype=torch.long, device=c.device)
    for b in range(10):
        for a in range(3):
            code |= ((q[:, a] >> b) & 1) << (3 * b + a)
    return torch.sort(code, stable=True).indices


class BEMModel:
    """Exterior Helmholtz problem on a closed triangle surface (reference ``BEMModel``, bem.py:16-63)."""

    def __init__(self, vertices, elements, device=None):
        """vertices: (n, 3), elements: (m, 3) - numpy or torch."""
        self.grid = obj_to_grid(vertices, elements)
        self.dp0_space = DP0Space(self.grid)
        self.dirichlet_fun = None
        self.neumann_fun = None
        self.k = None
        self.gmres_info = None
        m = self.grid.number_of_elements
        lda = m + (m & 1)
        if 8 * m * lda > BEM_MEMORY_BUDGET_BYTES:
            raise MemoryError(f"BEMModel: {m} faces need {8 * m * lda / 2 ** 30:.1f} GiB for the dense operator, above the "
                              f"budget of {BEM_MEMORY_BUDGET_BYTES / 2 ** 30:.1f} GiB (BEM_MEMORY_BUDGET_BYTES); coarsen the "
                              "surface (there is no hierarchical-matrix path)")
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if self.device.type != "cuda":
            raise RuntimeError("diffsound_amd: BEMModel runs on the HIP device (there is no CPU fallback)")
        self.m, self._lda = m, lda
        v = torch.from_numpy(self.grid.vertices.T.astype(np.float32)).to(self.device).contiguous()
        t = torch.from_numpy(self.grid.elements.T.astype(np.int64)).to(self.device)
        perm = _morton_order(v[t].mean(1))
        self._perm = perm  # internal face i = caller's face perm[i]
        self._tris = t[perm].to(torch.int32).contiguous()
        self._verts = v
        self.rec = torch.empty((m, FACE_RECORD), dtype=torch.float32, device=self.device)
        _hip.launch("ds_bem_geometry", v.data_ptr(), v.shape[0], self._tris.data_ptr(), m, self.rec.data_ptr(), device=self.device)
        self.area = self.rec[:, 31].contiguous()
        self._inv_area = (1.0 / self.area).contiguous()
        self._work, _ = _hip.workspace("ds_bem_assemble_workspace_bytes", m, device=self.device)
        self._g = None
        self._u = None

    # ------------------------------------------------------------------ order conversion
    def _to_internal(self, coeff, name):
        c = coeff
        if isinstance(c, torch.Tensor):
            c = c.detach().to(self.device)
        else:
            c = torch.from_numpy(np.asarray(c)).to(self.device)
        if c.dim() != 1 or c.shape[0] != self.m:
            raise ValueError(f"BEMModel: {name} must have shape ({self.m},), got {tuple(c.shape)}")
        c = c.to(torch.complex64)
        if not bool(torch.isfinite(torch.view_as_real(c)).all()):
            raise ValueError(f"BEMModel: {name} holds non-finite values")
        return c[self._perm].contiguous()

    def _to_external(self, c):
        out = torch.empty_like(c)
        out[self._perm] = c
        return out.cpu().numpy()

    @staticmethod
    def _check_k(wave_number):
        k = float(wave_number)
        if not np.isfinite(k) or k < 0:
            raise ValueError(f"BEMModel: wave_number must be finite and >= 0, got {wave_number!r}")
        return k

    # ------------------------------------------------------------------ native calls
    def assemble(self, wave_number, g_internal, want_V=False):
        """(A, rhs, V or None) for the wave number and the internal-order complex64 Neumann data: ds_bem_assemble.
        A and V are (m, lda) with lda = m rounded up to even; the columns >= m are not written."""
        k = self._check_k(wave_number)
        m, lda = self.m, self._lda
        A = torch.empty((m, lda), dtype=torch.complex64, device=self.device)
        V = torch.empty((m, lda), dtype=torch.complex64, device=self.device) if want_V else None
        rhs = torch.empty(m, dtype=torch.complex64, device=self.device)
        _hip.launch("ds_bem_assemble", self.rec.data_ptr(), m, k, g_internal.data_ptr(), A.data_ptr(), lda, _hip.ptr(V), lda,
                    rhs.data_ptr(), self._work.data_ptr(), device=self.device)
        return A, rhs, V

    def cgemv(self, A, x, scale=None, out=None):
        """y = diag(scale) A x (ds_bem_cgemv); x a 16-byte aligned complex64 vector of length >= m."""
        y = out if out is not None else torch.empty(self.m, dtype=torch.complex64, device=self.device)
        _hip.launch("ds_bem_cgemv", A.data_ptr(), A.stride(0), x.data_ptr(), self.m, _hip.ptr(scale), y.data_ptr(), device=self.device)
        return y

    def _potential(self, k, g, u, points):
        p = points
        if isinstance(p, torch.Tensor):
            p = p.detach()
        else:
            p = torch.from_numpy(np.asarray(p, dtype=np.float64))
        if p.dim() != 2 or p.shape[1] != 3 or p.shape[0] < 1:
            raise ValueError(f"potential_solve: points must be a (P, 3) array, got shape {tuple(p.shape)}")
        p = p.to(self.device, torch.float32).contiguous()
        if not bool(torch.isfinite(p).all()):
            raise ValueError("potential_solve: points hold non-finite coordinates")
        out = torch.empty(p.shape[0], dtype=torch.complex64, device=self.device)
        _hip.launch("ds_bem_potential", self.rec.data_ptr(), self.m, k, g.data_ptr(), u.data_ptr(), p.data_ptr(), p.shape[0],
                    out.data_ptr(), device=self.device)
        return out

    # ------------------------------------------------------------------ GMRES
    def _gmres(self, A, b, tol=GMRES_TOL, restart=GMRES_RESTART, maxiter=GMRES_MAXITER):
        """Restarted GMRES on diag(1/area) A x = diag(1/area) b.  Krylov basis on the device (complex64, classical
        Gram-Schmidt twice, sums in torch's fixed reduction order), Hessenberg and Givens rotations on the host in
        complex128.  Returns (x, info)."""
        m, dev = self.m, self.device
        npad = m + (m & 1)  # 16-byte aligned rows for ds_bem_cgemv
        Q = torch.zeros((restart + 1, npad), dtype=torch.complex64, device=dev)
        bs = b * self._inv_area
        bnorm = float(torch.linalg.vector_norm(bs))
        x = torch.zeros(m, dtype=torch.complex64, device=dev)
        xin = torch.zeros(npad, dtype=torch.complex64, device=dev)
        w = torch.empty(m, dtype=torch.complex64, device=dev)
        info = dict(iterations=0, residual=0.0, converged=True, restart=restart, tol=tol)
        if bnorm == 0.0:
            return x, info
        r = bs.clone()
        its, est = 0, 1.0
        while True:
            beta = float(torch.linalg.vector_norm(r))
            if beta / bnorm <= tol or its >= maxiter:
                break
            Q[0, :m] = r / beta
            H = np.zeros((restart + 1, restart), dtype=np.complex128)
            cs = np.zeros(restart, dtype=np.complex128)
            sn = np.zeros(restart, dtype=np.complex128)
            e = np.zeros(restart + 1, dtype=np.complex128)
            e[0] = beta
            j_used = 0
            for j in range(restart):
                self.cgemv(A, Q[j], self._inv_area, out=w)
                Qj = Q[:j + 1, :m]
                h = (Qj.conj() * w).sum(1)
                w -= (Qj * h[:, None]).sum(0)
                h2 = (Qj.conj() * w).sum(1)
                w -= (Qj * h2[:, None]).sum(0)
                h = h + h2
                hn = torch.linalg.vector_norm(w)
                hh = torch.cat([h.to(torch.complex128), hn.to(torch.complex128).reshape(1)]).cpu().numpy()
                H[:j + 1, j] = hh[:j + 1]
                hnv = float(hh[j + 1].real)
                H[j + 1, j] = hnv
                if hnv > 0:
                    Q[j + 1, :m] = w / hnv
                for i in range(j):  # apply the earlier rotations to the new column
                    t = cs[i] * H[i, j] + sn[i] * H[i + 1, j]
                    H[i + 1, j] = -np.conj(sn[i]) * H[i, j] + cs[i] * H[i + 1, j]
                    H[i, j] = t
                a_, b_ = H[j, j], H[j + 1, j]
                den = np.sqrt(abs(a_) ** 2 + abs(b_) ** 2)
                if den == 0:
                    cs[j], sn[j] = 1.0, 0.0
                else:
                    cs[j] = abs(a_) / den
                    sn[j] = (a_ / abs(a_) if abs(a_) > 0 else 1.0) * np.conj(b_) / den
                H[j, j] = cs[j] * a_ + sn[j] * b_
                H[j + 1, j] = 0.0
                e[j + 1] = -np.conj(sn[j]) * e[j]
                e[j] = cs[j] * e[j]
                its += 1
                j_used = j + 1
                est = abs(e[j + 1]) / bnorm
                if est <= tol or hnv == 0 or its >= maxiter:
                    break
            y = np.zeros(j_used, dtype=np.complex128)
            for i in range(j_used - 1, -1, -1):
                y[i] = (e[i] - H[i, i + 1:j_used] @ y[i + 1:]) / H[i, i]
            yd = torch.from_numpy(y.astype(np.complex64)).to(dev)
            x += (Q[:j_used, :m] * yd[:, None]).sum(0)
            xin[:m] = x
            self.cgemv(A, xin, self._inv_area, out=w)
            r = bs - w
        res = float(torch.linalg.vector_norm(r)) / bnorm
        # fp32 operator: the true residual can sit a little above the Arnoldi estimate that stopped the iteration
        info.update(iterations=its, residual=res, converged=res <= tol or (est <= tol and res <= 10 * tol))
        return x, info

    # ------------------------------------------------------------------ reference API
    def boundary_equation_solve(self, neumann_coeff, wave_number):
        """neumann_coeff: (m,) normal derivative per face; wave_number: k >= 0.  Solves (-1/2 M + K) u = V g and
        stores ``k``, ``neumann_fun``, ``dirichlet_fun`` and ``gmres_info`` (reference bem.py:27-47)."""
        k = self._check_k(wave_number)
        g = self._to_internal(neumann_coeff, "neumann_coeff")
        A, rhs, _ = self.assemble(k, g)
        u, info = self._gmres(A, rhs)
        del A
        self.k = k
        self.neumann_fun = GridFunction(self.grid, self._to_external(g))
        self.dirichlet_fun = GridFunction(self.grid, self._to_external(u))
        self._g, self._u = g, u
        self.gmres_info = info
        if not info["converged"]:
            warnings.warn(f"BEMModel: GMRES did not converge at k = {k:g} ({info['iterations']} iterations, relative "
                          f"residual {info['residual']:.2e} > {info['tol']:g}); k may be near an interior Dirichlet "
                          "eigenfrequency of the object, where the direct formulation is singular", RuntimeWarning)

    def potential_solve(self, points):
        """points: (P, 3) -> (P,) complex pressure u(p) = -S g + D u (reference bem.py:50-61)."""
        if self._u is None:
            raise RuntimeError("potential_solve: call boundary_equation_solve first")
        return self._potential(self.k, self._g, self._u, points).cpu().numpy()

    def export_neumann(self, filename):
        self._export(filename, self.neumann_fun, "neumann")

    def export_dirichlet(self, filename):
        self._export(filename, self.dirichlet_fun, "dirichlet")

    def _export(self, filename, fun, name):
        if fun is None:
            raise RuntimeError(f"export_{name}: call boundary_equation_solve first")
        write_gmsh22_surface(filename, self.grid.vertices.T, self.grid.elements.T, {f"{name}.real": fun.coefficients.real,
                                                                                    f"{name}.imag": fun.coefficients.imag})


def write_gmsh22_surface(path, vertices, triangles, element_data):
    """Gmsh 2.2 ASCII: $Nodes, $Elements (3-node triangles, type 2, tags: physical 1, elementary 1), then one
    $ElementData view per entry of ``element_data`` (name -> (m,) real values): string tag = the name, real tag =
    time 0, integer tags = (time step 0, 1 component, m values), lines "element-id value"."""
    v = np.asarray(vertices, dtype=np.float64)
    t = np.asarray(triangles, dtype=np.int64)
    with open(path, "w") as f:
        f.write("$MeshFormat\n2.2 0 8\n$EndMeshFormat\n")
        f.write(f"$Nodes\n{len(v)}\n")
        f.write("".join(f"{i + 1} {x!r} {y!r} {z!r}\n" for i, (x, y, z) in enumerate(v.tolist())))
        f.write(f"$EndNodes\n$Elements\n{len(t)}\n")
        f.write("".join(f"{i + 1} 2 2 1 1 {a + 1} {b + 1} {c + 1}\n" for i, (a, b, c) in enumerate(t.tolist())))
        f.write("$EndElements\n")
        for name, vals in element_data.items():
            vals = np.asarray(vals, dtype=np.float64).reshape(-1)
            f.write(f'$ElementData\n1\n"{name}"\n1\n0.0\n3\n0\n1\n{len(vals)}\n')
            f.write("".join(f"{i + 1} {x!r}\n" for i, x in enumerate(vals.tolist())))
            f.write("$EndElementData\n")


# ---------------------------------------------------------------------- helpers beyond the reference
_CORNER_SLOTS = {1: (0, 1, 2, 3), 2: (0, 2, 4, 9)}  # corner nodes in the element's node list (mesh.py to_high_order)
_EDGE_SLOT = {(0, 1): 1, (1, 2): 3, (0, 2): 5, (0, 3): 6, (1, 3): 7, (2, 3): 8}  # mid-edge node slots of ord-2


def surface_of(tetmesh):
    """Boundary triangles of the corner mesh of ``tetmesh`` (a TetMesh, ord 1 or 2): the faces that belong to exactly
    one tet, oriented outward (away from the tet's opposite vertex).  Returns (triangles (m, 3) long, mids) on the
    mesh's device; ``mids`` is (m, 3) long with the mid-edge node ids of the edges (a,b), (b,c), (c,a) of each
    triangle (a,b,c) for an ord-2 mesh, None for ord-1.  Node ids index ``tetmesh.vertices``."""
    order = int(getattr(tetmesh, "order", 1))
    tets = tetmesh.tets.long()
    if order not in _CORNER_SLOTS or tets.dim() != 2 or tets.shape[1] != (4 if order == 1 else 10):
        raise ValueError(f"surface_of: need an ord-1 (T, 4) or ord-2 (T, 10) mesh, got order {order}, tets {tuple(tets.shape)}")
    x = tetmesh.vertices.detach().double()
    corners = tets[:, list(_CORNER_SLOTS[order])]
    T, dev = tets.shape[0], tets.device
    loc = torch.tensor([[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2]], device=dev)  # face opposite local corner o
    opp = torch.arange(4, device=dev)
    f_loc = loc.unsqueeze(0).expand(T, 4, 3).reshape(-1, 3)
    f_opp = opp.unsqueeze(0).expand(T, 4).reshape(-1)
    f_tet = torch.arange(T, device=dev).repeat_interleave(4)
    f_nodes = torch.gather(corners[f_tet], 1, f_loc)
    key = torch.sort(f_nodes, dim=1).values
    uniq, inv, cnt = torch.unique(key, dim=0, return_inverse=True, return_counts=True)
    bnd = cnt[inv] == 1
    idx = torch.nonzero(bnd).reshape(-1)
    idx = idx[torch.argsort(inv[idx])]  # in the order of the sorted face keys
    fl, ft, fo = f_loc[idx], f_tet[idx], f_opp[idx]
    tri = f_nodes[idx]
    p0, p1, p2 = x[tri[:, 0]], x[tri[:, 1]], x[tri[:, 2]]
    po = x[corners[ft, fo]]
    flip = (torch.linalg.cross(p1 - p0, p2 - p0) * (po - p0)).sum(1) > 0
    fl = torch.where(flip.unsqueeze(1), fl[:, [0, 2, 1]], fl)
    tri = torch.gather(corners[ft], 1, fl)
    mids = None
    if order == 2:
        table = torch.zeros((4, 4), dtype=torch.long, device=dev)
        for (a, b), s in _EDGE_SLOT.items():
            table[a, b] = table[b, a] = s
        slots = torch.stack([table[fl[:, 0], fl[:, 1]], table[fl[:, 1], fl[:, 2]], table[fl[:, 2], fl[:, 0]]], 1)
        mids = torch.gather(tets[ft], 1, slots)
    return tri, mids


def mode_neumann(obj, surface):
    """(m, mode_num) face means of U_hat . n for the modes of a DiffSoundObj (after its eigen decomposition).
    ``U_hat`` rows are 3 * node + component in ``obj.tetmesh``'s node numbering (DiffSoundObj maps the solver's
    internal order back with ``rows_to_external``).  ord-1: the mean over the 3 corner nodes (exact face average of the
    P1 field); ord-2: the mean over the 3 mid-edge nodes (exact face average of the P2 field).  fp64, on the device."""
    tri, mids = surface
    mesh = obj.tetmesh
    U = obj.U_hat
    nv = mesh.vertices.shape[0]
    if U.dim() != 2 or U.shape[0] != 3 * nv:
        raise ValueError(f"mode_neumann: U_hat must be (3 * {nv}, modes), got {tuple(U.shape)}")
    order = int(getattr(mesh, "order", 1))
    nodes = mids if order == 2 else tri
    if nodes is None:
        raise ValueError("mode_neumann: an ord-2 mesh needs the mid-edge nodes of surface_of")
    x = mesh.vertices.detach().double()
    cr = torch.linalg.cross(x[tri[:, 1]] - x[tri[:, 0]], x[tri[:, 2]] - x[tri[:, 0]])
    n = cr / torch.linalg.vector_norm(cr, dim=1, keepdim=True)
    Un = U.detach().double().reshape(nv, 3, -1)
    mean = Un[nodes.to(U.device)].mean(dim=1)  # (m, 3, modes)
    return torch.einsum("mc,mck->mk", n.to(U.device), mean)


def modal_transfer(obj, points, c=343.0, rho=1.225):
    """Complex pressure amplitudes (P, mode_num) at ``points`` (P, 3) for unit modal amplitudes of a DiffSoundObj:
    per mode k = omega / c with omega = sqrt(eigenvalue) and the Neumann data dp/dn = rho omega^2 u_n (e^{-i omega t}
    convention), one BEM solve and one potential evaluation.  The surface model and its per-face geometry are built
    once.  Modes whose k falls near an interior Dirichlet eigenfrequency of the object are not detected (that is not
    cheap for a general shape); GMRES warns when such a solve does not converge."""
    if getattr(obj, "U_hat", None) is None:
        obj.eigen_decomposition()
    surf = surface_of(obj.tetmesh)
    model = BEMModel(obj.tetmesh.vertices.detach(), surf[0], device=obj.tetmesh.vertices.device)
    un = mode_neumann(obj, surf)
    lam = obj.eigenvalues.detach().double().reshape(-1).cpu().numpy()
    pts = _to_numpy(points)
    out = np.empty((pts.shape[0], lam.shape[0]), dtype=np.complex64)
    for j, ev in enumerate(lam):
        omega = float(np.sqrt(max(ev, 0.0)))
        model.boundary_equation_solve(rho * omega ** 2 * un[:, j], omega / c)
        out[:, j] = model.potential_solve(pts)
    return out
