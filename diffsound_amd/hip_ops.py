"""The HIP implementations of the eigensolver's ``ops`` protocol: the MATERIAL side of the operator layer.

``HipModalOps``  one material hypothesis on a TetSystem - (lam, mu): fp32 K = lam K_lambda + mu K_mu, or a general 9 x 9
                 tangent C (``set_tangent``): K_ab = C : H_ab on the same geometry tensors -, block-Jacobi blocks, rigid-body
                 basis, and every large operation the solver needs, each one a call into libdiffsound_hip.so.
``HipSparseOps`` a generic pencil (A, B) of torch sparse tensors, re-blocked into 3 x 3 node blocks.
The mesh side - node ordering, union and MFMA tables, assembly, geometry gradients - is ``TetSystem`` in modal_ops.py, which this
module imports and which never imports this one at load time.  Nothing here decides memory traffic: the benchmark keys its
traffic records by a hash that covers modal_ops.py and not this file, so an edit here leaves those records valid.
No operation here has a CPU implementation; tensors must be HIP tensors.
"""
import numpy as np
import torch

from . import _hip
from .block_ops import _HipBlockOps, _ld
from .modal_ops import MF32_BATCH, MF32_G, MF_BATCH, TetSystem, _mode_block, _tangent_array


def isotropic_tangent(lam, mu):
    """The 9 x 9 tangent d vec(P) / d vec(F) (row 3i+j, column 3k+l) of P = mu (F + F^T) + lam tr(F) I, fp64 on the host
    (reference src/diffelastic/diff_model.py:34-48)."""
    C = np.zeros((3, 3, 3, 3), dtype=np.float64)
    for i in range(3):
        for j in range(3):
            C[i, j, i, j] += mu
            C[i, j, j, i] += mu
            C[i, i, j, j] += lam
    return C.reshape(9, 9)


class HipModalOps(_HipBlockOps):
    """One material hypothesis (lam, mu) on a TetSystem."""

    # nodes per wavefront of the MFMA form of the preconditioner's bf16 terms on (fine level, corner-node level): 8, or 0 =
    # the VALU kernel (ds_spmm_union16).  Both levels since round 3: with 16-entry batches on the fine level and 32-entry
    # batches on levels smaller than the device's wave slots, the corner-node level's term takes 17.7 us instead of 22.1.
    mfma_groups = (8, 8)

    # the level's own fp32 products (K W, M W, M X of the eigensolver) on the matrix cores (ds_spmm_union32m) instead of
    # the VALU neighbour-union kernel.  OFF: built, parity-green and measured in round 4 - at C3 K X takes 263 us against
    # 229 us (M X 246 against 151): v_mfma_f32_16x16x4_f32 runs at the fp32 VECTOR rate and the 16 x 4 tile of 3x3 blocks on
    # a 4-node union is 3/4 x 0.43 full, so the matrix pipe needs 125-150 us for what the VALU does in 40, on top of the
    # LDS staging the form requires (profiles/r04_mfma32_*.txt)
    mfma32 = False

    # the corner-node level's polynomial on the group-block Jacobi (``group_jacobi`` of that level's operator object): 8 or 0
    coarse_group_jacobi = 8
    # the same for the ONE-level polynomial of an ord-1 mesh's operator object (no corner-node level): 8 or 0
    one_level_group_jacobi = 0

    k64c = None     # tangent mode: (nnzb, 9) fp64, the blocks of K = C : H as ds_combine_tangent wrote them
    tangent = None  # tangent mode: the 9 x 9 fp64 tangent (host array); None for a (lam, mu) material

    def __init__(self, system: TetSystem, lam=None, mu=None, two_level=None, _level=0, mfma_groups=None, mfma32=None,
                 coarse_group_jacobi=None, one_level_group_jacobi=None, tangent=None):
        """two_level: build the corner-node level for the two-level preconditioner (ord-2 meshes; default on).
        tangent: a 9 x 9 tangent d vec(P) / d vec(F) in the place of (lam, mu) (``set_tangent``)."""
        if (tangent is None) == (lam is None or mu is None):
            raise ValueError("HipModalOps: give either (lam, mu) or tangent=C")
        self.sys = system
        self._level_tag = min(int(_level), 1)
        if coarse_group_jacobi is not None:
            self.coarse_group_jacobi = int(coarse_group_jacobi)
        if one_level_group_jacobi is not None:
            self.one_level_group_jacobi = int(one_level_group_jacobi)
        if self.coarse_group_jacobi not in (0, 8) or self.one_level_group_jacobi not in (0, 8):
            raise ValueError("coarse_group_jacobi / one_level_group_jacobi: groups of 8 nodes, or 0 for the node blocks")
        if mfma_groups is not None:
            self.mfma_groups = tuple(mfma_groups)
        if mfma32 is not None:
            self.mfma32 = bool(mfma32)
        self._init_common(system.rowptr, system.colidx, system.nv, system.device)
        dev = self.device
        self.k32 = torch.empty((system.nnzb, 9), dtype=torch.float32, device=dev)
        self.k32t = torch.empty((system.nnzb, 9), dtype=torch.float32, device=dev)  # blocks transposed
        self.ms32 = torch.empty((system.nnzb,), dtype=torch.float32, device=dev)
        self.dinv = torch.empty((system.nv, 9), dtype=torch.float32, device=dev)
        if two_level is None:
            two_level = True
        if two_level and _level == 0 and system.order == 2:
            lvl = system.coarse_level()
            if lvl is not None:
                self._xfer = lvl
                self.coarse = HipModalOps(lvl["sys"], lam, mu, two_level=False, _level=1, mfma_groups=self.mfma_groups,
                                          mfma32=self.mfma32, coarse_group_jacobi=self.coarse_group_jacobi, tangent=tangent)
        G = self.mfma_groups[min(_level, 1)]
        if G not in (0, 8):
            raise ValueError("mfma_groups: 8 nodes per wavefront, or 0 for the VALU kernel")
        if G and system.groups is not None and system.nnzb * 24 < 0x7F000000:
            mt = system.mfma_tables(G)
            if mt["max_entries"] <= 256 and mt["max_batch_blocks"] <= MF_BATCH * G:  # what ds_spmm_union16m serves
                self._mfma = mt
                if (((_level == 1 and self.coarse_group_jacobi == G) or
                     (_level == 0 and system.order == 1 and self.one_level_group_jacobi == G)) and system.nv >= 4 * G):
                    md = system.mfma_tables_dense(G)
                    if md["nblocks"] * 24 < 0x7F000000:
                        self._mfma_dense, self.group_jacobi = md, G
        if self.mfma32 and system.groups is not None and system.nnzb * 36 + 16 < 0x7F000000:
            m4 = system.mfma_tables(MF32_G, MF32_BATCH)
            if m4["max_entries"] <= 256 and m4["max_batch_blocks"] <= MF32_BATCH * MF32_G:  # what ds_spmm_union32m serves
                self._mfma32 = m4
        self._rigid_generation = system.geometry_generation  # the geometry the rigid-body basis below is formed on
        if tangent is None:
            self.set_material(lam, mu)
        else:
            self.set_tangent(tangent)
        self.rigid = self._rigid_basis() if _level == 0 else None

    def group_T(self, X):
        """T_g X with the group-block Jacobi's blocks, fp32 in and out (ds_group_apply16): the power iteration's 8 columns and the
        Python path of the polynomial; the bf16 cycle applies T_g to its right-hand side inside the native driver."""
        X = X if (X.stride(1) == 1 and (X.data_ptr() | (X.stride(0) * 4)) % 16 == 0) else X.contiguous()
        Y = torch.empty((X.shape[0], X.shape[1]), dtype=torch.float32, device=X.device)
        for c0 in range(0, X.shape[1], 256):
            c1 = min(X.shape[1], c0 + 256)
            _hip.launch("ds_group_apply16", _hip.ptr(self.tgrp), self.group_jacobi, X[:, c0:c1].data_ptr(), 1, _ld(X),
                        Y[:, c0:c1].data_ptr(), 1, _ld(Y), self.nv, c1 - c0)
        return Y

    def probe_products(self, G0):
        """(K_lambda G0, K_mu G0, M G0) in fp64 for an fp32 probe block G0 of a multiple of 4 columns - ONE walk of the pattern
        (ds_spmm_f64_polish).  Geometry only: the solver keeps them per geometry generation and forms ||K G0|| of every material
        as ||lam K_lambda G0 + mu K_mu G0||.  None when the operator is not of that two-term form."""
        Y3 = self._polish_walk(self.polish_terms(), G0, lambda shape: torch.empty(shape, dtype=torch.float64, device=self.device))
        if Y3 is None:
            return None
        c = G0.shape[1]
        return Y3[:, :c], Y3[:, c:2 * c], Y3[:, 2 * c:]

    def norm_probe_key(self):
        """What the solver's cached norm probe (random block, ||M G0|| / ||G0||) is valid for: this system's geometry."""
        return (id(self.sys), self.sys.geometry_generation)

    def set_material(self, lam, mu):
        if self.coarse is not None:
            self.coarse.set_material(lam, mu)
        self._combine((float(lam), float(mu)), None)

    def set_tangent(self, C):
        """K = C : H for a 9 x 9 tangent d vec(P) / d vec(F) (row 3i+j, column 3k+l; fp64, host tensor or array) in the place of
        lam K_lambda + mu K_mu: ds_combine_tangent, then what ``set_material`` does after its combine step.  The caller
        validates C (diffelastic.diff_model.elastic_tangent: both symmetries, a positive definite Voigt matrix)."""
        C = _tangent_array(C, "set_tangent")
        if self.coarse is not None:
            self.coarse.set_tangent(C)
        self._combine(None, C)

    def _combine(self, lame, C):
        """This level's operator of a (lam, mu) material (``lame``) or of a tangent (``C``, else None)."""
        s = self.sys
        # New coordinates (TetSystem.assemble(vertices)) since the rigid-body basis was formed: the rotations are fields of the
        # coordinates and the basis is M-orthonormal in the OLD mass matrix - re-form it (round 5; until then an operator object that
        # outlived a geometry update deflated the previous geometry's rotations).  The corner-node level forms its basis on demand.
        gen = s.geometry_generation
        regen = self._rigid_generation != gen
        # (the solver's kept norm probe of a (lam, mu) material holds K_lambda G0 and K_mu G0, that of a tangent has no per-term
        # products: neither serves the other kind)
        if (self.tangent is None) != (C is None):
            self._norm_probe = None
        self.combined_k64(False)  # (a combined fp64 K array of the previous material must never outlive it)
        self.lame = lame
        p = _hip.ptr
        if C is None:
            self.tangent = self.k64c = None
            _hip.launch("ds_combine_material", p(s.klam), p(s.kmu), p(s.ms), s.nnzb, p(s.diagidx), s.nv, lame[0], lame[1],
                        p(self.k32), p(self.k32t), p(self.ms32), p(self.dinv))
        else:
            self.tangent = C.copy()
            if self.k64c is None:
                self.k64c = torch.empty((s.nnzb, 9), dtype=torch.float64, device=self.device)
            _hip.launch("ds_combine_tangent", p(s.klam), p(s.ms), s.nnzb, p(s.diagidx), s.nv, C.ctypes.data, p(self.k64c),
                        p(self.k32), p(self.k32t), p(self.ms32), p(self.dinv))
        self._after_combine(regen, gen)

    def tangent_forms(self, U):
        """(m, 9, 9) fp64: Q[c][3i+j][3k+l] = sum_ab u_a,i H_ab[j][l] u_b,k of every column of the fp32 block U (n x m, the
        system's internal node order), so that u^T K(C) u = (C * Q[c]).sum() for any tangent C (ds_tangent_forms)."""
        U = _mode_block(U, self.n, "tangent_forms")
        s, m = self.sys, U.shape[1]
        Q = torch.empty((m, 9, 9), dtype=torch.float64, device=self.device)
        need = _hip.lib().ds_tangent_forms_workspace_bytes(s.nv, m)
        ws = self._scratch("tangent_forms_ws", ((need + 7) // 8,), torch.float64)
        p = _hip.ptr
        _hip.launch("ds_tangent_forms", p(s.rowptr), p(s.colidx), p(s.klam), s.nv, p(U), _ld(U), m, p(Q), p(ws), ws.numel() * 8)
        return Q

    def geometry_grad(self, U, gk, gm):
        """d/dx sum_i gk_i u_i^T K u_i - gm_i u_i^T M u_i for the operator's CURRENT stiffness - its tangent, or after
        ``set_material`` the tangent of (lam, mu) - on the system's current geometry: (nv, 3) fp64 in the caller's node
        numbering (``TetSystem.geometry_grad_tangent``).  U: (n, m) float32 in the system's internal order."""
        C = self.tangent if self.tangent is not None else isotropic_tangent(*self.lame)
        return self.sys.geometry_grad_tangent(U, gk, gm, C)

    def _after_combine(self, regen, gen):
        """What follows the combine step of ``set_material`` / ``set_tangent``: everything below reads k32 / k32t / ms32 and
        knows nothing of the material."""
        s = self.sys
        p = _hip.ptr
        if s.groups is not None:
            if self.kgrp is None:
                self.kgrp = torch.empty((s.nnzb, 9), dtype=torch.float32, device=self.device)
            _hip.launch("ds_pack_groups", p(self.k32t), p(s.groups["kperm"]), s.nnzb, p(self.kgrp))
            if self.m_kind == 1:
                self.mgrp = self.ms32[s.groups["kperm64"]].contiguous()  # node-scalar mass values in group order
            if self._mfma is not None:
                if self.kc is None:
                    self.kc = torch.empty((s.nnzb, 3, 4), dtype=torch.bfloat16, device=self.device)
                _hip.launch("ds_pack_kc", p(self.k32), p(self._mfma["kperm"]), s.nnzb, p(self.kc))
            if self.group_jacobi and self._mfma is not None:
                md = self._mfma_dense
                if self.tgrp is None:
                    ng = md["ngroups"]
                    self.tgrp = torch.empty((ng, 3 * self.group_jacobi, 3 * self.group_jacobi), dtype=torch.float32, device=self.device)
                    self.kc_dense = torch.zeros((md["nblocks"], 3, 4), dtype=torch.bfloat16, device=self.device)
                    self.dinv_id = torch.eye(3, dtype=torch.float32, device=self.device).reshape(1, 9).repeat(s.nv, 1).contiguous()
                _hip.launch("ds_group_inverse", p(s.rowptr), p(s.colidx), p(self.k32), s.nv, self.group_jacobi, p(self.tgrp))
                mt_ = self._mfma
                _hip.launch("ds_group_pack_kc", p(self.k32), p(self.tgrp), p(mt_["gptr"]), p(mt_["gmeta"]), p(mt_["gbase"]),
                            p(mt_["kperm"]), self.group_jacobi, s.nv, p(self.kc_dense))
            if self._mfma32 is not None:
                if self.k4 is None:  # (zeros: the 16 bytes of slack behind the last block are read and must be finite)
                    self.k4 = torch.zeros((s.nnzb * 9 + 4,), dtype=torch.float32, device=self.device)
                    self._kperm4 = self._mfma32["kperm"].long()
                _hip.launch("ds_pack_groups", p(self.k32), p(self._mfma32["kperm"]), s.nnzb, p(self.k4))
                if self.m_kind == 1:
                    if self.m4 is None:
                        self.m4 = torch.zeros((s.nnzb + 4,), dtype=torch.float32, device=self.device)
                    torch.index_select(self.ms32, 0, self._kperm4, out=self.m4[:s.nnzb])
        if regen:  # (the new mass values are in place)
            self._rigid_generation = gen
            self.rigid = self._rigid_basis() if self._level_tag == 0 else None

    def _rigid_fields(self):
        """Translations + rotations about the centroid, (n, 8) fp64 with two zero pad columns so every kernel sees a multiple of
        4 columns."""
        v = self.sys.vertices.double()
        c = v - v.mean(0, keepdim=True)
        Y = torch.zeros((self.n, 8), dtype=torch.float64, device=self.device)
        for a in range(3):
            Y[a::3, a] = 1
        Y[0::3, 3], Y[1::3, 3] = -c[:, 1], c[:, 0]
        Y[1::3, 4], Y[2::3, 4] = -c[:, 2], c[:, 1]
        Y[2::3, 5], Y[0::3, 5] = -c[:, 0], c[:, 2]
        return Y

    def _m_orthonormal(self, Y, mass, store):
        """The six rigid fields Y (n, 8; two zero pad columns) M-orthonormalised in two passes of M Y -> 6 x 6 Gram -> Cholesky
        -> triangular solve; the second pass removes the rounding of the first.  ``mass(Y, MY)`` writes the fp64 product M Y;
        ``store`` rounds a pass's fp64 result to Y's storage precision.  Returns a block of Y's type."""
        MY = torch.empty((self.n, 8), dtype=torch.float64, device=self.device)
        for _ in range(2):
            mass(Y, MY)
            G = self.gram(Y, MY)[:6, :6]  # (a 6 x n by n x 6 fp64 product takes rocBLAS 24 ms at the benchmark size)
            Lc = torch.linalg.cholesky(0.5 * (G + G.T))
            Y6 = torch.linalg.solve_triangular(Lc, Y.double()[:, :6].T, upper=False).T
            Y = torch.zeros_like(Y)
            Y[:, :6] = store(Y6)
        return Y

    def _rigid_basis(self):
        """The six rigid-body modes, M-orthonormalised in fp64; stored (n, 8) fp32."""
        return self._m_orthonormal(self._rigid_fields().float(), lambda Y, MY: self._spmm(3, self.sys.ms, Y, MY), torch.Tensor.float)

    def polish_terms(self):
        if self.lame is None:  # tangent mode: one term, the blocks ds_combine_tangent wrote
            return [(2, self.k64c, 1.0)], (3, self.sys.ms)
        lam, mu = self.lame
        return [(2, self.sys.klam, lam), (2, self.sys.kmu, mu)], (3, self.sys.ms)

    def rigid64(self):
        """The six rigid-body modes in fp64 (n x 8, two zero pad columns), M-orthonormal to fp64 accuracy."""
        if self.rigid is None:
            return None
        return self._m_orthonormal(self._rigid_fields(), self.apply_M64, lambda Y6: Y6)


def _coo_to_bsr3(A, nv, pattern=None):
    """torch sparse (COO/CSR) (3nv x 3nv) -> (rowptr, colidx, blocks (nnzb,9) fp64) on A's device,
    on the union pattern ``pattern`` = (rowptr, colidx) if given."""
    A = A.to_sparse_coo().coalesce()
    idx, val = A.indices(), A.values().double()
    bkey = (idx[0] // 3) * nv + (idx[1] // 3)
    if pattern is None:
        keys = torch.unique(bkey)
    else:
        keys = pattern
    slot = torch.searchsorted(keys, bkey)
    if not bool((keys[slot.clamp(max=keys.numel() - 1)] == bkey).all()):
        raise ValueError("sparse matrix has entries outside the common block pattern")
    blocks = torch.zeros((keys.numel(), 9), dtype=torch.float64, device=val.device)
    blocks.view(-1).index_add_(0, slot * 9 + (idx[0] % 3) * 3 + (idx[1] % 3), val)
    return keys, blocks


class HipSparseOps(_HipBlockOps):
    """Generic pencil (A, B) given as torch sparse tensors on the HIP device (the ``lobpcg_func`` entry).
    Both are re-blocked into 3x3 node blocks on their common pattern; no rigid-mode deflation."""

    m_kind = 0

    def __init__(self, A, B):
        _hip.require_gpu(A, B)
        n = B.shape[-1]
        if n % 3 != 0 or tuple(A.shape) != (n, n) or tuple(B.shape) != (n, n):
            raise ValueError("HipSparseOps: A and B must be square with a row count divisible by 3 "
                             "(3 DOFs per node); got {} and {}".format(tuple(A.shape), tuple(B.shape)))
        nv = n // 3
        dev = B.device
        ka, _ = _coo_to_bsr3(A, nv)
        kb, _ = _coo_to_bsr3(B, nv)
        keys = torch.unique(torch.cat([ka, kb, torch.arange(nv, device=dev) * (nv + 1)]))
        _, self.a64 = _coo_to_bsr3(A, nv, keys)
        _, self.b64 = _coo_to_bsr3(B, nv, keys)
        rows = keys // nv
        rowptr = torch.zeros(nv + 1, dtype=torch.int64, device=dev)
        rowptr[1:] = torch.cumsum(torch.bincount(rows, minlength=nv), 0)
        self._init_common(rowptr.to(torch.int32), (keys % nv).to(torch.int32), nv, dev)
        # arbitrary pencils (no deflation, possibly -A for the largest end, no preconditioner): keep the Gram exact
        self.gram_exact = True
        self.k32 = self.a64.float().contiguous()
        self.k32t = self.k32.reshape(-1, 3, 3).transpose(1, 2).reshape(-1, 9).contiguous()
        self.ms32 = self.b64.float().contiguous()
        diag = self.a64[torch.searchsorted(keys, torch.arange(nv, device=dev) * (nv + 1))].reshape(nv, 3, 3)
        eye = torch.eye(3, dtype=torch.float64, device=dev)
        bad = torch.linalg.det(diag).abs() < 1e-300
        diag = torch.where(bad[:, None, None], eye, diag)
        dinv64 = torch.linalg.inv(diag)
        self.dinv = dinv64.float().reshape(nv, 9).contiguous()
        # rigorous bound of lambda_max(T A), T = the inverse diagonal blocks: the block-infinity norm max_i sum_j ||T_i A_ij||_F
        # (an operator norm for the vector norm max_i ||x_i||_2).  The Chebyshev polynomial of lobpcg_func takes it as the end of
        # its interval: a power-iteration estimate that falls short of the true value makes the polynomial blow up on the top of
        # the spectrum, and on pencils that are not FEM matrices 30 steps x 1.2 do fall short (round 6, tests/test_api_gpu.py)
        rows_ = torch.repeat_interleave(torch.arange(nv, device=dev), (rowptr[1:] - rowptr[:-1]))
        ta = torch.linalg.matrix_norm(dinv64[rows_] @ self.a64.reshape(-1, 3, 3))
        self.lmax_bound = float(torch.zeros(nv, dtype=torch.float64, device=dev).index_add_(0, rows_, ta).max())
        self.rigid = None
        self.lame = None

    def polish_terms(self):
        return [(2, self.a64, 1.0)], (2, self.b64)
