"""HIP implementation of the eigensolver's ``ops`` protocol on a BSR-3 pattern: the part ``HipModalOps`` and ``HipSparseOps``
(hip_ops.py) share.  Every product, Gram, mix, residual and both native drivers are one call into libdiffsound_hip.so here;
what decides node ordering and tables stays in modal_ops.py.
No operation here has a CPU implementation; tensors must be HIP tensors.
"""
import ctypes

import torch

from . import _hip

DS_F32, DS_F64 = 0, 1


def _ld(t):
    if t.dim() != 2 or t.stride(1) != 1:
        raise ValueError("block must be a 2-D row-major view (unit column stride)")
    return t.stride(0)


_MFMA_KEYS32 = ("gptr", "gcol", "gmeta", "gbase")  # what the fp32 form (ds_spmm_union32m) takes
_MFMA_KEYS = _MFMA_KEYS32 + ("ghead",)  # ... and the bf16 term kernel (ds_spmm_union16m)


def _mfma_ptrs(mt, keys=_MFMA_KEYS):
    """The topology arrays of an MFMA table dict (TetSystem.mfma_tables / mfma_tables_dense) as pointers, in the order the
    kernels and ds_level_t take them."""
    return tuple(mt[k].data_ptr() for k in keys)


def _wire_cycle_scratch(d, D, AD, Rr, Wc, Rc, Ec, Dc, ADc, R16):
    """The scratch blocks of the two-level cycle into a ds_twolevel_t; ``R16`` given: bf16 storage."""
    d.D, d.ldd, d.AD, d.lda = D.data_ptr(), D.stride(0), AD.data_ptr(), AD.stride(0)
    d.Rr, d.ldrr = Rr.data_ptr(), Rr.stride(0)
    d.Rc, d.Ec, d.Dc, d.ADc, d.ldc = Rc.data_ptr(), Ec.data_ptr(), Dc.data_ptr(), ADc.data_ptr(), Rc.stride(0)
    d.Wc, d.ldwc = Wc.data_ptr(), Wc.stride(0)
    d.storage = 0 if R16 is None else 1
    d.R16, d.ldr16 = (None, 0) if R16 is None else (R16.data_ptr(), R16.stride(0))


class _HipBlockOps:
    """HIP implementation of the solver's ``ops`` protocol on a BSR-3 pattern (shared part).

    Subclasses provide: rowptr, colidx, nv, k32 (nnzb x 9 f32), ms32 (+ m_kind), dinv, rigid,
    lame and polish_terms()."""

    dtype = torch.float32
    m_kind = 1  # 1: M = M_s (x) I3 (one scalar per block), 0: general 3x3 blocks
    sys = None  # the TetSystem behind the operator (HipModalOps); None: no node-group tables (HipSparseOps)
    k32t = None
    kgrp = None  # transposed blocks in node-group order (neighbour-union SpMM)
    mgrp = None  # node-scalar mass values in node-group order (neighbour-union SpMM, epilogue 3)
    coarse = None  # ops of the corner-node level (HipModalOps on an ord-2 mesh sets it)
    _tl_desc = None  # the ds_twolevel_t of twolevel_apply, its transfer tables filled in on first use
    _mfma = None  # tables of the MFMA form of the bf16 terms (TetSystem.mfma_tables), None: the VALU kernel
    # GROUP-block Jacobi of the level's bf16 polynomial (round 6; the corner-node level only): 8 = T is the inverse of the 24 x 24
    # diagonal block of every group of 8 nodes of the matrix-core tables, 0 = the 3 x 3 node blocks (dinv).  tgrp (ng, 24, 24) fp32,
    # kc_dense the blocks of T_g K on TetSystem.mfma_tables_dense, dinv_id an identity per node - all per material (set_material).
    group_jacobi = 0
    tgrp = kc_dense = dinv_id = _mfma_dense = None
    kc = None     # (nnzb, 3, 4) bf16: the 3x3 blocks in the order of those tables (ds_pack_kc)
    _mfma32 = None  # tables of the fp32 MFMA form of the level's own products K X / M X (groups of 4 nodes), None: VALU
    k4 = None     # (nnzb * 9 + 4,) fp32: the 3x3 blocks (row-major) in the order of those tables, 16 bytes of slack
    m4 = None     # (nnzb + 4,) fp32: the node-scalar mass values in that order
    _level_tag = 0  # 0: fine level, 1: corner-node level (selects kernel symbols, nothing else)
    # fp64 refinement, inside a combined_k64(True) ... combined_k64(False) bracket: K = sum c_i K_i as ONE fp64 block array, formed
    # on the bracket's first product - in the union tables' group order (_k64grp, with the mass scalars _m64grp beside it) when
    # that product's block qualifies for ds_spmm_f64_union, and in BSR order (_k64) for a block that does not.  All None outside.
    _k64_on = False
    _k64 = _k64grp = _m64grp = None
    host_wait_mode = -1  # how the native iteration waits for its stream (pipeline.set_wait_mode); -1: the process default
    # The fused polish walk's three results are fp64 blocks.  ``polish_f32_blocks`` (round 5, OFF): the same fp64 sums stored as
    # fp32 blocks - half the bytes written there and read by the Gram launch, which then takes the fp32 matrix-core path (1.10 ->
    # ~0.7 ms per pass at the benchmark size, 1.8 % of a pass).  Built, tested (tests/test_hip_kernels.py) and NOT adopted: the
    # polish then returns eigenvalues and quadratic forms with ~3e-8 of relative noise instead of values accurate to second order
    # in the iteration error (two solves whose fp32 blocks differ in rounding agreed to 3.6e-8 instead of < 1e-9) - inside the
    # stated 1e-4, but a precision cut in the one stage whose job is precision
    polish_f32_blocks = False

    def _init_common(self, rowptr, colidx, nv, device):
        self.rowptr, self.colidx = rowptr, colidx
        self.nv = nv
        self.n = 3 * nv
        self.device = device
        _hip.lib()  # (a missing or stale library is reported when the operator is built, not at its first launch)
        self._gram_ws = None
        self._native_ws = {}
        self.gram_exact = False
        self._tmp = {}
        self._nrm = torch.empty((2, 1024), dtype=torch.float64, device=device)
        self.counts = dict(apply_K_cols=0, apply_M_cols=0, gram=0, mix=0, mix64=0)

    # ------------------------------------------------------------------ sparse products
    def _spmm_chunks(self, kind, vals, vt, X, out, maxc):
        """out <- A X through ds_spmm_bsr3, ``maxc`` columns per launch."""
        p = _hip.ptr
        for c0 in range(0, X.shape[1], maxc):
            c1 = min(X.shape[1], c0 + maxc)
            xs, os_ = X[:, c0:c1], out[:, c0:c1]
            _hip.launch("ds_spmm_bsr3", kind, p(self.rowptr), p(self.colidx), p(vals), p(vt), self.nv, p(xs), _ld(xs), p(os_), _ld(os_),
                        c1 - c0)

    def _spmm(self, kind, vals, X, out):
        if out.shape != X.shape:
            raise ValueError("spmm: shape mismatch")
        vt = self.k32t if (kind == 0 and vals is self.k32) else None
        self._spmm_chunks(kind, vals, vt, X, out, 256 if kind < 2 else 128)

    @staticmethod
    def col_slices(c):
        """Column ranges of at most 84 columns (multiples of 4, as equal as possible) that tile a c-column block: what the
        neighbour-union kernels take per launch.  136 -> (0, 68), (68, 136); 240 -> three of 80.  (The same rule as for_col_slices of
        csrc/lobpcg.cpp, which tiles the native loop's products: change both or neither.)"""
        if c <= 84:
            return [(0, c)]
        k = -(-c // 84)
        w = -(-(-(-c // k)) // 4) * 4
        return [(c0, min(c, c0 + w)) for c0 in range(0, c, w)]

    def _groups(self):
        """The node-group tables of the system behind this operator, None without one."""
        return None if self.sys is None else self.sys.groups

    def _union_groups(self):
        """The node-group tables of this level when it has neighbour-union tables and its blocks in their order, else None."""
        g = self._groups()
        return None if (g is None or g.get("union") is None or self.kgrp is None) else g

    def _union_tabs(self):
        """(utab or None, ctab, ngroups, cap_blocks, gent): the leading arguments of every neighbour-union kernel.  utab is None
        when every group is one chunk."""
        g = self.sys.groups
        u = g["union"]
        return (None if u.get("single") else u["utab"].data_ptr()), u["ctab"].data_ptr(), u["ngroups"], u["capb"], g["gent"].data_ptr()

    def _union_ok(self, X, *others, wide=False):
        if self._union_groups() is None or (X.shape[1] > 84 and not wide) or X.shape[1] % 4:
            return False
        # every operand is read / written 16 bytes at a time (blocks of 2 GB and more take the kernel's per-panel
        # descriptor variant; the dinv table and the value array stay under one descriptor: nv * 36, nnzb * 36 < 4 GB)
        if self.nv * 36 >= 0x7F000000 or self.kgrp.shape[0] * 36 >= (1 << 32):
            return False
        for T in (X,) + others:
            if T is not None:
                ld = T.stride(0)
                if ld % 4 or T.data_ptr() % 16 or T.stride(1) != 1:
                    return False
        return True

    def level_desc(self, d, degree, lmax, lmin):
        """Fill a ds_level_t with this level's neighbour-union tables (None when the level has none)."""
        if self._union_groups() is None:
            return None
        d.utab, d.ctab, d.ngroups, d.cap_blocks, d.gent = self._union_tabs()
        d.kgrp, d.nnzb, d.nv, d.dinv = self.kgrp.data_ptr(), self.kgrp.shape[0], self.nv, self.dinv.data_ptr()
        d.degree, d.lmax, d.lmin = int(degree), float(lmax), float(lmin)
        d.level_tag = self._level_tag
        d.tgrp, d.mf_nblocks = None, 0
        mt, kc = self._mfma, self.kc  # the level's bf16 terms on the matrix cores (ds_spmm_union16m) ...
        if self.group_jacobi and self.tgrp is not None:
            # ... or group-block Jacobi: the blocks of T_g K on the dense tables, an identity for dinv, T_g for the right-hand side
            mt, kc = self._mfma_dense, self.kc_dense
            d.mf_nblocks, d.tgrp, d.dinv = mt["nblocks"], self.tgrp.data_ptr(), self.dinv_id.data_ptr()
        if mt is not None and kc is not None:
            d.mf_group_nodes, d.mf_max_entries, d.mf_max_batch_blocks = mt["G"], mt["max_entries"], mt["max_batch_blocks"]
            d.mf_gptr, d.mf_gcol, d.mf_gmeta, d.mf_gbase, d.mf_ghead = _mfma_ptrs(mt)
            d.mf_kc = kc.data_ptr()
        else:
            d.mf_group_nodes = 0
        m4 = self._mfma32
        if m4 is not None and self.k4 is not None:  # the level's own fp32 products run on the matrix cores (ds_spmm_union32m)
            d.m32_max_entries, d.m32_max_batch_blocks = m4["max_entries"], m4["max_batch_blocks"]
            d.m32_gptr, d.m32_gcol, d.m32_gmeta, d.m32_gbase = _mfma_ptrs(m4, _MFMA_KEYS32)
            d.m32_k = self.k4.data_ptr()
            d.m32_m = None if self.m4 is None else self.m4.data_ptr()
        else:
            d.m32_gptr = None
        return d

    def _union32_ok(self, X, out):
        return (self._mfma32 is not None and self.k4 is not None and self._union_ok(X, out)
                and 3 * self.nv * X.stride(0) * 4 < 0x7F000000)

    def _union32(self, epilogue, X, Y):
        pp = _hip.ptr
        m4 = self._mfma32
        vals = self.m4 if epilogue == 3 else self.k4
        _hip.launch("ds_spmm_union32m", epilogue, self._level_tag, *_mfma_ptrs(m4, _MFMA_KEYS32), pp(vals), vals.numel() * 4,
                    self.colidx.shape[0], m4["ngroups"], m4["max_entries"], m4["max_batch_blocks"], self.nv, pp(X), _ld(X), pp(Y),
                    _ld(Y), X.shape[1])

    def twolevel_apply(self, smooth, coarse, R, W, D, AD, Rr, Rc, Ec, Dc, ADc, Wc, R16=None, prepared=False):
        """The whole two-level V-cycle W = B R through the native driver (ds_twolevel_apply): one call instead of
        ~45 launches issued one by one.  ``smooth`` / ``coarse``: (degree, lmax, lmin) of the two Chebyshev operators.
        R16 given: every scratch block (D ... Wc, R16) is bf16 and the cycle runs on bf16 iterates (R, W stay fp32).
        ``prepared`` (bf16 cycle): R16 and the smoother's first iterate (in D; in Wc for a degree-1 smoother) are already there -
        residual_fused_pre wrote them - and the cycle starts at its first term; R is not read.
        Returns False (nothing done) when a level or a block does not qualify for the neighbour-union kernels."""
        co = self.coarse
        if co is None:
            return False
        if R16 is not None:
            blocks = (D, AD, Rr, Wc, R16, Rc, Ec, Dc, ADc)
            ok = all(t.dtype == torch.bfloat16 and t.stride(1) == 1 and t.stride(0) % 4 == 0 and t.data_ptr() % 8 == 0
                     for t in blocks) and self._union_ok(R, W) and self.kgrp is not None and co.kgrp is not None
            if not ok:
                return False
        elif not (self._union_ok(R, W, D, AD, Rr, Wc) and co._union_ok(Rc, Ec, Dc, ADc)):
            return False
        d = self._tl_desc
        if d is None:
            d = self._tl_desc = self._transfer_desc()
        if self.level_desc(d.fine, *smooth) is None or co.level_desc(d.coarse, *coarse) is None:
            return False
        if not (Rc.stride(0) == Ec.stride(0) == Dc.stride(0) == ADc.stride(0) and
                Wc.stride(0) == D.stride(0) == AD.stride(0)):
            return False
        d.R, d.ldr, d.W, d.ldw = R.data_ptr(), R.stride(0), W.data_ptr(), W.stride(0)
        d.ncols = R.shape[1]
        _wire_cycle_scratch(d, D, AD, Rr, Wc, Rc, Ec, Dc, ADc, R16)
        if prepared:
            d.storage |= _hip.TL_PREPARED
        _hip.launch("ds_twolevel_apply", ctypes.byref(d))
        c = R.shape[1]
        self.counts["apply_K_cols"] += c * (max(smooth[0] - 1, 0) + 1 + smooth[0])
        co.counts["apply_K_cols"] += c * (coarse[0] - 1)
        return True

    def _transfer_desc(self):
        """A ds_twolevel_t with the restriction / prolongation tables between this level and its corner-node level filled in."""
        d, t = _hip.TwoLevelDesc(), self._xfer
        d.rptr, d.rcol, d.rw = t["rptr"].data_ptr(), t["rcol"].data_ptr(), t["rw"].data_ptr()
        d.pptr, d.pcol, d.pw = t["pptr"].data_ptr(), t["pcol"].data_ptr(), t["pw"].data_ptr()
        return d

    def chebyshev_apply16(self, precond, R, W):
        """W <- p(T K) T R through the native one-level driver on bf16 iterates (ds_chebyshev_apply16: the launches the native
        iteration issues for the same preconditioner) for blocks of <= 84 columns; False when the level or block does not qualify."""
        d = _hip.LevelDesc()
        if (precond.degree < 2 or R.shape[1] > 84 or R.shape[1] % 4 or not self._union_ok(R, W)
                or self.level_desc(d, precond.degree, precond.lmax, precond.lmin) is None or self._mfma is None or self.kc is None):
            return False
        b = R.shape[1]
        scr = self._scratch("native_cheb", (3, self.n, b), torch.bfloat16)
        _hip.launch("ds_chebyshev_apply16", ctypes.byref(d), R.data_ptr(), _ld(R), W.data_ptr(), _ld(W), scr[0].data_ptr(),
                    scr[1].data_ptr(), scr[2].data_ptr(), b, b)
        self.counts["apply_K_cols"] += b * (precond.degree - 1)
        return True

    # ------------------------------------------------------------------ native iteration driver
    def _native_ok(self, b, ny, R, MX, MW, S, KS):
        """What ds_lobpcg_iterate serves: node-scalar mass on the neighbour-union tables, blocks of <= 160 columns."""
        return (self._union_groups() is not None and self.mgrp is not None and self.m_kind == 1
                and b <= 160 and b % 4 == 0 and ny % 4 == 0 and self._union_ok(R, MX, MW, S[:, ny:ny + b], KS[:, :b], wide=True))

    def _native_precond(self, d, precond, cfg, b):
        """The preconditioner of the ds_lobpcg_t ``d`` - the level, the two-level cycle or the one-level polynomial's scratch,
        in fp32 or bf16 storage - for blocks of ``b`` columns.  Returns what the descriptor points into (to be kept alive until
        the call returns), or None for a preconditioner that stays on the Python loop."""
        from .lobpcg.precond import ChebyshevBlockJacobi, TwoLevelChebyshev

        if isinstance(precond, TwoLevelChebyshev):
            co = self.coarse
            if co is None or precond.ops is not self:
                return None
            tl = self._transfer_desc()
            sm, cs = precond.smooth, precond.coarse
            if (self.level_desc(tl.fine, sm.degree, sm.lmax, sm.lmin) is None
                    or co.level_desc(tl.coarse, cs.degree, cs.lmax, cs.lmin) is None):
                return None
            bf = cfg.precond_storage == "bf16"
            if cs.group and not bf:
                return None  # (the group-block Jacobi lives on the bf16 cycle: an fp32 cycle goes through the Python loop)
            sdt = torch.bfloat16 if bf else torch.float32
            scr = self._scratch("native_tl_fine", (5, self.n, b), sdt)  # Wc, D, AD, Rr, R16
            scc = co._scratch("native_tl_coarse", (4, co.n, b), sdt)  # Rc, Ec, Dc, ADc
            _wire_cycle_scratch(tl, scr[1], scr[2], scr[3], scr[0], scc[0], scc[1], scc[2], scc[3], scr[4] if bf else None)
            if bf and not getattr(cfg, "residual_handoff", True):
                tl.storage |= _hip.TL_OWN_INIT  # (the iteration's residual walk leaves this cycle its own first launch)
            tl.R = tl.W = 1  # (set per application by the driver; non-null for its argument check)
            d.twolevel = ctypes.pointer(tl)
            self.level_desc(d.level, sm.degree, sm.lmax, sm.lmin)
            return [tl, scr, scc]
        if isinstance(precond, ChebyshevBlockJacobi):
            if precond.ops is not self or self.level_desc(d.level, precond.degree, precond.lmax, precond.lmin) is None:
                return None
            bf = cfg.precond_storage == "bf16" and precond.degree >= 2
            if precond.group and not bf:
                return None
            scr = self._scratch("native_cheb", (3, self.n, b), torch.bfloat16 if bf else torch.float32)
            d.pa, d.pb, d.ldp = scr[0].data_ptr(), scr[1].data_ptr(), b
            d.pr16 = scr[2].data_ptr() if bf else None
            return [scr]
        return None

    def _native_workspace(self, d, cfg, b, ny):
        """The iteration's device buffers and the Gram / fused-residual workspaces into ``d``."""
        m = ny + 3 * b
        gbuf = self._scratch("native_g", (m * 3 * b,), torch.float64)
        cbuf = self._scratch("native_c", (8 * m * 2 * b,), torch.float32)
        lam_dev = self._scratch("native_lam", (b,), torch.float64)
        key = (self.n, b, ny)
        need = self._native_ws.get(key)
        if need is None:  # the split count depends on the shape: take the largest need over every shape the driver forms
            # (q: the active width na, 2 na for [K W | M W] of the Ritz step on the raw basis, p itself for the full refresh)
            need = max(_hip.lib().ds_gram_workspace_bytes(self.n, p_, q_)
                       for p_ in range(4, m + 1, 4) for q_ in sorted(set(range(4, 2 * b + 1, 4)) | {p_}) if q_ <= 3 * b)
            self._native_ws[key] = need
        self._gram_workspace(need)
        d.gbuf, d.cbuf, d.nrm, d.lam_dev = gbuf.data_ptr(), cbuf.data_ptr(), self._nrm.data_ptr(), lam_dev.data_ptr()
        d.gram_work, d.gram_work_bytes = self._gram_ws.data_ptr(), self._gram_ws.numel()
        if cfg.fused_residual and cfg.kx_fresh:
            rws = self._residual_ws(b)
            d.res_work, d.res_work_bytes = rws.data_ptr(), rws.numel()
        else:
            d.res_work, d.res_work_bytes = None, 0

    def native_lobpcg(self, precond, cfg, k, b, ny, S, S2, KS, KS2, R, MX, MW, lam, A_norm, B_norm, tol):
        """Run the eigensolver's iteration through ds_lobpcg_iterate (csrc/lobpcg.cpp).  Returns None when this
        configuration has to stay on the Python loop (block wider than the union kernels take, a mass matrix that is
        not node-scalar, a preconditioner the driver does not know), else
        (iterations, result_in_s2, lam (b,) fp64 device, rerr (b,) fp64 device, history [(it, worst backward error)])."""
        if not self._native_ok(b, ny, R, MX, MW, S, KS):
            return None
        d = _hip.LobpcgDesc()
        keep = self._native_precond(d, precond, cfg, b)  # tensors the descriptor points into
        if keep is None:
            return None
        d.n, d.nv, d.b, d.k, d.ny = self.n, self.nv, b, k, ny
        d.maxit, d.lock, d.ortho_passes, d.rr_refresh = cfg.maxit, int(cfg.lock), cfg.ortho_passes, cfg.rr_refresh
        d.gram_exact = int(bool(self.gram_exact))
        d.kx_fresh = int(bool(cfg.kx_fresh))
        d.raw_rr = int(bool(cfg.raw_rr))
        d.tol, d.ortho_tol, d.A_norm, d.B_norm = float(tol), float(cfg.ortho_tol), A_norm, B_norm
        d.ritz_tol = float(cfg.ritz_tol)
        d.wait_mode = int(self.host_wait_mode)  # (this operator object's - i.e. this lane's - own setting)
        d.S, d.S2, d.KS, d.KS2 = S.data_ptr(), S2.data_ptr(), KS.data_ptr(), KS2.data_ptr()
        d.R, d.MX, d.MW = R.data_ptr(), MX.data_ptr(), MW.data_ptr()
        d.lds, d.ldks, d.ldr = S.stride(0), KS.stride(0), R.stride(0)
        if not (S2.stride(0) == d.lds and KS2.stride(0) == d.ldks and MX.stride(0) == d.ldr and MW.stride(0) == d.ldr):
            return None
        d.mgrp = self.mgrp.data_ptr()
        d.rowptr, d.colidx, d.k32, d.k32t = (self.rowptr.data_ptr(), self.colidx.data_ptr(), self.k32.data_ptr(),
                                             self.k32t.data_ptr())
        self._native_workspace(d, cfg, b, ny)
        lam_h = (ctypes.c_double * b)(*lam.detach().double().cpu().tolist())
        rerr_h = (ctypes.c_double * b)()
        hist_h = (ctypes.c_double * (cfg.maxit + 1))()
        d.lam, d.rerr, d.history, d.history_cap = lam_h, rerr_h, hist_h, cfg.maxit + 1
        with _hip.blas_one_thread():
            _hip.launch("ds_lobpcg_iterate", ctypes.byref(d), ctypes.byref(_hip.lapack_table()))
        it = int(d.iterations)
        lam_t = torch.tensor(list(lam_h), dtype=torch.float64, device=self.device)
        rel_t = torch.tensor(list(rerr_h), dtype=torch.float64, device=self.device)
        history = [(i, hist_h[i]) for i in range(min(it + 1, cfg.maxit + 1))]
        del keep
        return it, bool(d.result_in_s2), lam_t, rel_t, history

    def _union(self, epilogue, X, Y, R0=None, c1=0.0, c2=0.0, first=False, Wprev=None):
        pp = _hip.ptr
        vals = self.mgrp if epilogue == 3 else self.kgrp
        _hip.launch("ds_spmm_union", epilogue, self._level_tag, *self._union_tabs(), pp(vals), vals.shape[0], self.nv, pp(X), _ld(X),
                    pp(Y), _ld(Y), pp(R0), 0 if R0 is None else _ld(R0), pp(self.dinv) if epilogue == 1 else None, X.shape[1],
                    float(c1), float(c2), int(bool(first)), pp(Wprev), 0 if Wprev is None else _ld(Wprev))

    def _narrow(self, kind, X, Y):
        """<= 16 columns: the kernel that deals a wave's lanes over the union's entries (ds_spmm_union_narrow)."""
        pp = _hip.ptr
        utab, ctab, ngroups, _, gent = self._union_tabs()
        vals = self.mgrp if kind == 3 else self.kgrp
        _hip.launch("ds_spmm_union_narrow", kind, self._level_tag, utab, ctab, ngroups, gent, pp(vals), vals.shape[0], self.nv,
                    pp(X), _ld(X), pp(Y), _ld(Y), X.shape[1])

    def apply_K(self, X, out):
        if self._union32_ok(X, out):
            self._union32(0, X, out)
        elif X.shape[1] <= 16 and self._level_tag == 0 and self._union_ok(X, out):
            # (fine level only: 131 -> 115 us on 8 columns at C3; the corner-node level's production launch is as short as a wave's
            # life either way, and the node-scalar product M X is faster on the production kernel: profiles/r05_mb_narrow.txt)
            self._narrow(0, X, out)
        elif self._union_ok(X, out):
            self._union(0, X, out)
        elif self._union_ok(X, out, wide=True):
            # wider than one launch takes (configs[4]'s 136-column block, the periodic refresh K [X P W]): column slices through the
            # same kernel - the wave-per-node kernel this used to fall to runs at 21 % of STREAM on the 1M-tet mesh, the slices at ~40 %
            for c0, c1 in self.col_slices(X.shape[1]):
                self._union(0, X[:, c0:c1], out[:, c0:c1])
        else:
            self._spmm(0, self.k32, X, out)
        self.counts["apply_K_cols"] += X.shape[1]

    def apply_KM_ok(self, X, KX, MX):
        return self.m_kind == 1 and self.mgrp is not None and self._union_ok(X, KX, MX, wide=True)

    def apply_KM(self, X, KX, MX):
        """KX <- K X and MX <- M X in ONE walk of the neighbour unions (ds_spmm_union_km): X is gathered once; each product
        equals what apply_K / apply_M give bit for bit."""
        pp = _hip.ptr
        tabs = self._union_tabs()
        for c0, c1 in self.col_slices(X.shape[1]):
            xs, ks, ms = X[:, c0:c1], KX[:, c0:c1], MX[:, c0:c1]
            _hip.launch("ds_spmm_union_km", self._level_tag, *tabs, pp(self.kgrp), pp(self.mgrp), self.kgrp.shape[0], self.nv,
                        pp(xs), _ld(xs), pp(ks), _ld(ks), pp(ms), _ld(ms), c1 - c0)
        self.counts["apply_K_cols"] += X.shape[1]
        self.counts["apply_M_cols"] += X.shape[1]

    def apply_M(self, X, out):
        if self.m_kind == 1 and self.m4 is not None and self._union32_ok(X, out):
            self._union32(3, X, out)
        elif self.m_kind == 1 and self.mgrp is not None and self._union_ok(X, out):
            self._union(3, X, out)
        elif self.m_kind == 1 and self.mgrp is not None and self._union_ok(X, out, wide=True):
            for c0, c1 in self.col_slices(X.shape[1]):
                self._union(3, X[:, c0:c1], out[:, c0:c1])
        else:
            self._spmm(self.m_kind, self.ms32, X, out)
        self.counts["apply_M_cols"] += X.shape[1]

    # ------------------------------------------------------------------ tall-skinny dense
    def _gram_workspace(self, need):
        """The Gram kernels' split-K workspace, grown to at least ``need`` bytes."""
        if self._gram_ws is None or self._gram_ws.numel() < need:
            self._gram_ws = torch.empty((need,), dtype=torch.uint8, device=self.device)
        return self._gram_ws

    def gram(self, A, B, symmetric=False, exact=False):
        """G = A^T B in fp64.  exact=False: fp32 MFMA folded into fp64 every 48 rows (~1e-9 of |A_i||B_j| at the
        benchmark's row count, ~1e-7 on a few hundred rows); ops with gram_exact set always take the fp64 MFMA."""
        exact = exact or self.gram_exact
        p, q = A.shape[1], B.shape[1]
        self._gram_workspace(_hip.lib().ds_gram_workspace_bytes(self.n, p, q))
        G = torch.empty((p, q), dtype=torch.float64, device=self.device)
        adt = DS_F64 if A.dtype == torch.float64 else DS_F32
        bdt = DS_F64 if B.dtype == torch.float64 else DS_F32
        pp = _hip.ptr
        _hip.launch("ds_gram", pp(A), adt, _ld(A), p, pp(B), bdt, _ld(B), q, self.n, int(bool(symmetric)) | (2 if exact else 0), pp(G),
                    pp(self._gram_ws), self._gram_ws.numel())
        self.counts["gram"] += 1
        return G

    def gram_blocks(self, A_blocks, B_blocks, symmetric=False):
        """G = [A_0 | A_1 | ...]^T [B_0 | B_1 | ...] in fp64 (ds_gram64_blocks) for bases held as LISTS of (n x p) fp64
        blocks: one pass over the rows for all pairs of blocks.  ``symmetric``: B = K A with a symmetric K and the same
        widths on both sides - only the tiles on and above the diagonal are computed.  At most 4 blocks per side."""
        def table(blocks):
            arr, off = (_hip.Block64 * len(blocks))(), 0
            for d, blk in zip(arr, blocks):
                if blk.dtype != torch.float64 or blk.shape[0] != self.n or blk.stride(1) != 1:
                    raise ValueError("gram_blocks: blocks are (n x p) fp64 with unit column stride")
                d.a, d.lda, d.p, d.offset = _hip.ptr(blk), _ld(blk), blk.shape[1], off
                off += blk.shape[1]
            return arr, off
        (ta, p), (tb, q) = table(A_blocks), table(B_blocks)
        self._gram_workspace(_hip.lib().ds_gram_workspace_bytes(self.n, p, q))
        G = torch.empty((p, q), dtype=torch.float64, device=self.device)
        _hip.launch("ds_gram64_blocks", len(A_blocks), ctypes.addressof(ta), len(B_blocks), ctypes.addressof(tb), self.n,
                    int(bool(symmetric)), _hip.ptr(G), _hip.ptr(self._gram_ws), self._gram_ws.numel())
        self.counts["gram"] += 1
        return G

    def _scratch(self, key, shape, dtype):
        t = self._tmp.get(key)
        if t is None or t.shape != tuple(shape) or t.dtype != dtype:
            t = torch.empty(tuple(shape), dtype=dtype, device=self.device)
            self._tmp[key] = t
        return t

    def mix(self, A, C, out, alpha=1.0, beta=0.0):
        p, q = C.shape
        if A.shape[1] != p or out.shape[1] != q:
            raise ValueError("mix: shape mismatch")
        C32 = C.to(torch.float32).contiguous()
        pp = _hip.ptr
        _hip.launch("ds_mix", pp(A), _ld(A), p, pp(C32), q, pp(out), _ld(out), self.n, float(alpha), float(beta))
        self.counts["mix"] += 1

    def mix64(self, blocks, C, out=None, alpha=1.0, beta=0.0):
        """out <- alpha * [blocks[0] | blocks[1] | ...] C + beta * out in fp64 (ds_mix64): the basis is a LIST of (n x p_i)
        fp64 blocks - never concatenated - and C their stacked (sum p_i) x q coefficients; every block is read once and
        the result written once.  An entry of ``blocks`` is a block - its coefficients are the rows of C that follow the
        previous entry's - or a ``(block, first_row)`` tuple that addresses its rows of C explicitly (rows of C no entry
        names are skipped).  ``out`` must not share memory with a block or with C."""
        C = C.contiguous()
        if C.dtype != torch.float64:
            raise ValueError("mix64: fp64 coefficients")
        q = C.shape[1]
        items, row = [], 0
        for blk in blocks:
            if isinstance(blk, tuple):
                blk, row = blk
            if blk.dtype != torch.float64 or blk.shape[0] != self.n or blk.stride(1) != 1:
                raise ValueError("mix64: blocks are (n x p) fp64 with unit column stride")
            items.append((blk, row))
            row += blk.shape[1]
        if max(r + b.shape[1] for b, r in items) > C.shape[0]:
            raise ValueError("mix64: the blocks need more coefficient rows than C has")
        if out is None:
            out = torch.empty((self.n, q), dtype=torch.float64, device=self.device)
            if beta != 0.0:
                raise ValueError("mix64: beta != 0 needs an out")
        if out.dtype != torch.float64 or out.shape != (self.n, q) or out.stride(1) != 1:
            raise ValueError("mix64: out is (n x q) fp64 with unit column stride")
        pp = _hip.ptr
        nmax = 4  # DS_MIX64_MAX_BLOCKS
        for i0 in range(0, len(items), nmax):
            part = items[i0:i0 + nmax]
            arr = (_hip.Block64 * len(part))()
            for d, (blk, r) in zip(arr, part):
                d.a, d.lda, d.p, d.offset = pp(blk), _ld(blk), blk.shape[1], r
            _hip.launch("ds_mix64", len(part), ctypes.addressof(arr), pp(C), _ld(C), q, pp(out), _ld(out), self.n, float(alpha),
                        float(beta if i0 == 0 else 1.0))
        self.counts["mix64"] += 1
        return out

    # ------------------------------------------------------------------ fp64 refinement: fused element-wise passes
    def residual64(self, KX, MX, X, lam):
        """(||K x_j - lam_j M x_j||^2, ||x_j||^2) of every column of the fp64 blocks in ONE pass (ds_residual64_norms)."""
        b = X.shape[1]
        if b % 2 or b > 512 or any(t.dtype != torch.float64 or t.stride(1) != 1 or (t.data_ptr() | (t.stride(0) * 8)) % 16
                                   for t in (KX, MX, X)):
            R = torch.addcmul(KX, MX, lam[None, :], value=-1.0)
            return (R * R).sum(0), (X * X).sum(0)
        pp = _hip.ptr
        need = _hip.lib().ds_residual64_workspace_doubles(b)
        ws = self._scratch("residual64_ws", (need,), torch.float64)
        out = torch.empty((2, b), dtype=torch.float64, device=self.device)
        lam = lam.to(torch.float64).contiguous()
        _hip.launch("ds_residual64_norms", pp(KX), _ld(KX), pp(MX), _ld(MX), pp(X), _ld(X), pp(lam), self.n, b, pp(ws), need,
                    pp(out[0]), pp(out[1]))
        return out[0], out[1]

    def residual64_scaled(self, KX, MX, lam, scale, idx, out=None):
        """(n x len(idx)) fp32 block of the residual columns ``idx`` of the fp64 blocks, each times ``scale[col]``
        (ds_residual64_scaled): the scaled input of the fp32 preconditioner, without an fp64 residual block in between."""
        nact = int(idx.numel())
        if nact % 4:
            raise ValueError("residual64_scaled: a multiple of 4 columns")
        pp = _hip.ptr
        R = torch.empty((self.n, nact), dtype=torch.float32, device=self.device) if out is None else out
        if R.dtype != torch.float32 or R.shape != (self.n, nact) or R.stride(1) != 1:
            raise ValueError("residual64_scaled: out is (n x len(idx)) fp32 with unit column stride")
        cols = idx.to(torch.int32).contiguous()
        lam, scale = lam.to(torch.float64).contiguous(), scale.to(torch.float64).contiguous()
        _hip.launch("ds_residual64_scaled", pp(KX), _ld(KX), pp(MX), _ld(MX), pp(lam), pp(scale), pp(cols), nact, pp(R), _ld(R), self.n)
        return R

    def mix_inplace(self, W, T):
        if T.shape[1] <= 160:  # ds_mix reads a row tile completely before writing it
            self.mix(W, T, W)
            return
        tmp = self._scratch("mix_inplace", W.shape, W.dtype)
        self.mix(W, T, tmp)
        W.copy_(tmp)

    # ------------------------------------------------------------------ fused elementwise
    def _residual_ws(self, ncols):
        u = self.sys.groups["union"]
        need = _hip.lib().ds_union_residual_workspace_bytes(u["ngroups"], ncols)
        ws = self._tmp.get("residual_ws")
        if ws is None or ws.numel() < need:
            ws = self._tmp["residual_ws"] = torch.empty((need,), dtype=torch.uint8, device=self.device)
        return ws

    def _norms(self, b):
        """(||R_j||^2, ||X_j||^2) of the first ``b`` columns, as a residual kernel left them in the norm buffer."""
        return self._nrm[0, :b].clone(), self._nrm[1, :b].clone()

    def residual_fused_ok(self, X, R):
        # (operand blocks of 2 GB and more - configs[4]'s basis buffer - take the kernel's per-panel descriptor variant, as every
        # other epilogue does: tests/test_hip_kernels.py::test_union_spmm_operands_beyond_2gb)
        return self.m_kind == 1 and self.mgrp is not None and self._union_ok(X, R, wide=True)

    def residual_fused(self, X, lam, R):
        """R <- K X - (M X) diag(lam) and (||R_j||^2, ||X_j||^2) in ONE walk of the neighbour unions (ds_union_residual): K X
        and M X are never written.  R equals what apply_K + apply_M + residual give bit for bit."""
        b = X.shape[1]
        lam64 = lam.to(torch.float64).contiguous()
        pp = _hip.ptr
        tabs = self._union_tabs()
        slices = self.col_slices(b)  # (a block wider than one launch takes: column slices, each with its share of the norms)
        ws = self._residual_ws(max(c1 - c0 for c0, c1 in slices))
        for c0, c1 in slices:
            xs, rs = X[:, c0:c1], R[:, c0:c1]
            _hip.launch("ds_union_residual", self._level_tag, *tabs, pp(self.kgrp), pp(self.mgrp), self.kgrp.shape[0], self.nv,
                        pp(xs), _ld(xs), pp(lam64[c0:]), pp(rs), _ld(rs), c1 - c0, pp(ws), ws.numel(), pp(self._nrm[0, c0:]),
                        pp(self._nrm[1, c0:]))
        self.counts["apply_K_cols"] += b
        self.counts["apply_M_cols"] += b
        return self._norms(b)

    def residual_fused_pre(self, X, lam, c, R16, W1):
        """The walk of residual_fused for an iteration whose preconditioner is the bf16 two-level cycle (ds_union_residual_pre; one
        launch: <= 84 columns, fine level): instead of the fp32 R it writes the bf16 copy ``R16`` of R and the smoother's first
        iterate ``W1`` = c T R (bf16), bit for bit what residual_fused followed by ds_cheb_init16 write.  Returns the norms."""
        b = X.shape[1]
        lam64 = lam.to(torch.float64).contiguous()
        pp = _hip.ptr
        ws = self._residual_ws(b)
        _hip.launch("ds_union_residual_pre", self._level_tag, *self._union_tabs(), pp(self.kgrp), pp(self.mgrp), self.kgrp.shape[0],
                    self.nv, pp(X), _ld(X), pp(lam64), pp(self.dinv), float(c), pp(R16), _ld(R16), pp(W1), _ld(W1), b, pp(ws),
                    ws.numel(), pp(self._nrm[0]), pp(self._nrm[1]))
        self.counts["apply_K_cols"] += b
        self.counts["apply_M_cols"] += b
        return self._norms(b)

    def residual(self, R, MX, X, lam, src=None):
        """R <- src - MX diag(lam) (src = K X; None: R holds it already), returns (||R_j||^2, ||X_j||^2) in fp64."""
        b = R.shape[1]
        lam64 = lam.to(torch.float64).contiguous()
        pp = _hip.ptr
        src = R if src is None else src
        _hip.launch("ds_residual", pp(src), _ld(src), pp(R), _ld(R), pp(MX), _ld(MX), pp(X), _ld(X), pp(lam64), self.n, b,
                    pp(self._nrm[0]), pp(self._nrm[1]))
        return self._norms(b)

    def cheb_init(self, R, D, W, c):
        pp = _hip.ptr
        _hip.launch("ds_cheb_init", pp(R), _ld(R), pp(D), _ld(D), pp(W), _ld(W), pp(self.dinv), self.nv, R.shape[1], float(c))

    def cheb_step(self, AD, R, D, W, c1, c2):
        pp = _hip.ptr
        _hip.launch("ds_cheb_step", pp(AD), _ld(AD), pp(R), _ld(R), pp(D), _ld(D), pp(W), _ld(W), pp(self.dinv), self.nv, R.shape[1],
                    float(c1), float(c2))

    def cheb_spmm(self, Wk, Wprev, R0, c1, c2, first):
        """Wprev <- Wk + c1 (Wk - Wprev) + c2 T (R0 - K Wk): one fused launch per polynomial term."""
        if self._union_ok(Wk, Wprev, R0):
            self._union(1, Wk, Wprev, R0, c1, c2, first)
        else:
            pp = _hip.ptr
            _hip.launch("ds_cheb_spmm", pp(self.rowptr), pp(self.colidx), pp(self.k32), self.nv, pp(Wk), _ld(Wk), pp(Wprev), _ld(Wprev),
                        pp(R0), _ld(R0), pp(self.dinv), Wk.shape[1], float(c1), float(c2), int(bool(first)))
        self.counts["apply_K_cols"] += Wk.shape[1]

    _cheb_spmm_launch = cheb_spmm  # (the name the benchmark's roofline and tools/mb_*.py time the launch under)

    def cheb_term_bytes(self, ncols, first=False, elem_bytes=4):
        """ALGORITHMIC bytes of one fused Chebyshev-term launch, SURVEY.md section 8(d)'s BSR-3 count: 9 values and one int32
        column id per block, the row pointers, the block-Jacobi blocks T, and the vector streams - W_k (gathered, counted
        once), R0 and W_{k-1} read (W_{k-1} = 0 is not read when ``first``), W_{k+1} written; ``elem_bytes`` = 2 for the bf16
        blocks of the production preconditioner.  The values count at the width the kernel multiplies with: 2 bytes where
        the term runs on the matrix cores (3x3 blocks rounded to bf16: 18 B of payload per block), else 4.  What the kernels
        actually fetch beyond that - the 24-byte padded block rows and the two table words per union entry of the MFMA form,
        re-gathered panels - is traffic, not algorithm: it shows in the PMC figure beside this one."""
        nnzb = self.colidx.shape[0]
        vec = (3 if first else 4) * self.n * ncols * elem_bytes
        vbytes = 2 if (elem_bytes == 2 and self._mfma is not None and self.kc is not None) else 4
        return nnzb * (9 * vbytes + 4) + (self.nv + 1) * 4 + self.nv * 36 + vec

    def cheb_spmm16(self, Wk, Wprev, R0, c1, c2, first):
        """The fused term on bf16 blocks, in place on W_prev: what the bf16 V-cycle launches (ds_spmm_union16m when the
        level carries the MFMA tables, else ds_spmm_union16)."""
        pp = _hip.ptr
        mt = self._mfma
        tail = (self.nv, pp(Wk), _ld(Wk), pp(Wprev), _ld(Wprev), 0, pp(R0), _ld(R0), pp(self.dinv), Wk.shape[1], float(c1), float(c2),
                int(bool(first)), None, 0)
        if mt is not None and self.kc is not None:
            _hip.launch("ds_spmm_union16m", 1, mt["G"], self._level_tag, *_mfma_ptrs(mt), pp(self.kc), self.kc.shape[0], mt["ngroups"],
                        mt["max_entries"], mt["max_batch_blocks"], *tail)
        else:
            _hip.launch("ds_spmm_union16", 1, *self._union_tabs(), pp(self.kgrp), self.kgrp.shape[0], *tail)

    # ------------------------------------------------------------------ two-level preconditioner pieces
    def spmm_residual(self, X, R0, Y):
        """Y <- R0 - K X (<= 84 columns, one fused launch)."""
        if self._union_ok(X, Y, R0):
            self._union(2, X, Y, R0)
        else:
            pp = _hip.ptr
            _hip.launch("ds_spmm_residual", pp(self.rowptr), pp(self.colidx), pp(self.k32), self.nv, pp(X), _ld(X), pp(R0), _ld(R0),
                        pp(Y), _ld(Y), X.shape[1])
        self.counts["apply_K_cols"] += X.shape[1]

    def _transfer(self, ptr_, col, w, nrows, X, Y, beta):
        pp = _hip.ptr
        _hip.launch("ds_scalar_csr_spmm", pp(ptr_), pp(col), pp(w), nrows, pp(X), _ld(X), pp(Y), _ld(Y), X.shape[1], float(beta))

    def restrict(self, Rf, Rc):
        """Rc <- P^T Rf (fine block -> corner-node level)."""
        t = self._xfer
        self._transfer(t["rptr"], t["rcol"], t["rw"], self.coarse.nv, Rf, Rc, 0.0)

    def prolong_add(self, Ec, Wf):
        """Wf <- Wf + P Ec."""
        t = self._xfer
        self._transfer(t["pptr"], t["pcol"], t["pw"], self.nv, Ec, Wf, 1.0)

    def prolong(self, Ec, Wf):
        """Wf <- P Ec (nothing of Wf is read: the nested start writes its block straight into the solver's basis buffer)."""
        t = self._xfer
        self._transfer(t["pptr"], t["pcol"], t["pw"], self.nv, Ec, Wf, 0.0)

    # ------------------------------------------------------------------ fp64 iterates (refinement phase)
    def _spmm64(self, kind, vals, X, out):
        """out (fp64) <- A X for an fp64 block X, in chunks of <= 80 columns (kinds 4 / 5 of ds_spmm_bsr3)."""
        if X.dtype != torch.float64 or out.dtype != torch.float64 or X.shape != out.shape:
            raise ValueError("_spmm64: fp64 blocks of equal shape expected")
        self._spmm_chunks(kind + 2, vals, None, X, out, 80)

    def combined_k64(self, on):
        """fp64 refinement: while ``on``, ``apply_K64`` multiplies by ONE fp64 block array K = sum c_i K_i, formed on the
        first product (configs[4]: 2.7 GB), instead of one product per term - half the matrix traffic of every K W.
        The caller brackets a phase in which neither the material nor the assembled terms change, and switches it off
        afterwards (the array is released)."""
        self._k64_on = bool(on)
        self._k64 = self._k64grp = self._m64grp = None

    def _combined_k64_values(self):
        """sum c_i K_i of ``polish_terms()``: (nnzb, 9) fp64 in BSR order, a new array."""
        kterms, _ = self.polish_terms()
        k = kterms[0][1] * float(kterms[0][2])
        for _, vals, c in kterms[1:]:
            k.add_(vals, alpha=float(c))
        return k

    def _union64_ok(self, X, out):
        g = self._groups()
        return (g is not None and g.get("union") is not None and X.dtype == torch.float64 and out.dtype == torch.float64
                and X.shape == out.shape and X.shape[1] % 4 == 0 and X.stride(1) == 1 and out.stride(1) == 1
                and (X.data_ptr() | (X.stride(0) * 8) | out.data_ptr() | (out.stride(0) * 8)) % 16 == 0)

    def _union64(self, kind, vals_grp, X, out):
        """out (fp64) <- A X on the neighbour-union tables (ds_spmm_f64_union), values in group order; column slices of <= 84."""
        pp = _hip.ptr
        tabs = self._union_tabs()
        for c0, c1 in self.col_slices(X.shape[1]):
            xs, os_ = X[:, c0:c1], out[:, c0:c1]
            _hip.launch("ds_spmm_f64_union", kind, 1, *tabs, pp(vals_grp), vals_grp.shape[0], self.nv, pp(xs), _ld(xs), pp(os_), _ld(os_),
                        c1 - c0)

    def apply_K64(self, X, out, terms=False):
        """out <- K X, all fp64 (fp64 block values).  ``terms``: also return the list of the separate K_i X."""
        kterms, _ = self.polish_terms()
        if self._k64_on and not terms and len({kt[0] for kt in kterms}) == 1:
            kind = kterms[0][0]
            if self._k64 is None and self._k64grp is None:  # the phase's first product forms the array
                k = self._combined_k64_values()
                if kind == 2 and self._union64_ok(X, out):
                    # round 5: the combined array in the union tables' group order, blocks transposed - the refinement's K W then
                    # walks the unions of 4 rows (ds_spmm_f64_union) instead of gathering every neighbour's panel once per row
                    # (the BSR-order array is not kept beside it)
                    kp = self.sys.groups["kperm64"]
                    self._k64grp = k[kp].reshape(-1, 3, 3).transpose(1, 2).reshape(-1, 9).contiguous()
                else:
                    self._k64 = k
            if self._k64 is None and self._union64_ok(X, out):
                self._union64(0, self._k64grp, X, out)
                return []
            if self._k64 is None:  # (a block the union kernel does not take: the BSR-order array after all, and from here on)
                self._k64 = self._combined_k64_values()
            self._spmm64(kind, self._k64, X, out)
            return []
        tmp = self._scratch("k64tmp", X.shape, torch.float64)
        parts = []
        out.zero_()
        for kind, vals, c in kterms:
            self._spmm64(kind, vals, X, tmp)
            out.add_(tmp, alpha=float(c))
            if terms:
                parts.append(tmp.clone())
        return parts

    def apply_M64(self, X, out):
        _, (mkind, mvals) = self.polish_terms()
        if mkind == 3 and self._k64grp is not None and self._union64_ok(X, out):
            if self._m64grp is None:  # (inside a combined_k64 phase the assembled terms do not change)
                self._m64grp = mvals[self.sys.groups["kperm64"]].contiguous()
            self._union64(1, self._m64grp, X, out)
            return
        self._spmm64(mkind, mvals, X, out)

    def rigid64(self):
        return None

    def vector_forms(self, U):
        """([u^T K_i u], u^T M u) of every column of the fp32 block U, (k,) fp64 each, for the terms of ``polish_terms()``:
        fp64 values, fp64 products and sums.  The forms of exactly the vectors handed in."""
        kterms, (mkind, mvals) = self.polish_terms()
        k = U.shape[1]
        pad = (-k) % 4
        Up = U.contiguous() if not pad else torch.cat([U, torch.zeros((U.shape[0], pad), dtype=U.dtype, device=U.device)], 1).contiguous()
        Y = self._scratch("vector_forms", Up.shape, torch.float64)
        U64 = Up.double()
        out = []
        for kind, vals in [(kd, v) for kd, v, _ in kterms] + [(mkind, mvals)]:
            self._spmm(kind, vals, Up, Y)
            out.append((U64 * Y).sum(0)[:k].clone())
        return out[:-1], out[-1]

    # ------------------------------------------------------------------ fp64 polish
    def _polish_walk(self, terms, X, block):
        """K_lambda X, K_mu X and M_s X in one walk of the pattern (ds_spmm_f64_polish): one gather of X instead of three; the
        three results sit side by side in ONE (n x 3c) block, ``block(shape)`` - fp64, or fp32 for the f32out form -, so that their
        Gram products with X are one launch that reads X once (round 4; three launches before).  None, and no block asked for,
        when the operator (``terms`` = polish_terms()) is not of that two-term form or X does not qualify."""
        kterms, (mkind, mvals) = terms
        c = X.shape[1]
        if not (len(kterms) == 2 and kterms[0][0] == 2 and kterms[1][0] == 2 and mkind == 3 and X.dtype == torch.float32
                and c % 4 == 0 and c <= 84 and X.stride(1) == 1 and (X.data_ptr() | (X.stride(0) * 4)) % 16 == 0):
            return None
        Y3 = block((X.shape[0], 3 * c))
        p = _hip.ptr
        _hip.launch("ds_spmm_f64_polish" if Y3.dtype == torch.float64 else "ds_spmm_f64_polish_f32out", p(self.rowptr), p(self.colidx),
                    p(kterms[0][1]), p(kterms[1][1]), p(mvals), self.nv, p(X), _ld(X), p(Y3[:, :c]), p(Y3[:, c:2 * c]), p(Y3[:, 2 * c:]),
                    3 * c, c)
        return Y3

    def polish_products(self, X):
        """fp64 Gram matrices of the terms of K and of M on the block X (fp64 values, fp64
        accumulation, fp32 X): returns ([X^T K_i X], [c_i], X^T M X) with K = sum c_i K_i."""
        terms = kterms, (mkind, mvals) = self.polish_terms()
        dt = torch.float32 if self.polish_f32_blocks else torch.float64
        Y3 = self._polish_walk(terms, X, lambda shape: self._scratch("polish3", shape, dt))
        if Y3 is not None:
            c = X.shape[1]
            G3 = self.gram(X, Y3)
            return ([G3[:, :c].contiguous(), G3[:, c:2 * c].contiguous()], [kterms[0][2], kterms[1][2]],
                    G3[:, 2 * c:].contiguous())
        Y = self._scratch("polish", X.shape, torch.float64)
        GK, coef = [], []
        for kind, vals, c in kterms:
            self._spmm(kind, vals, X, Y)
            GK.append(self.gram(X, Y))
            coef.append(c)
        self._spmm(mkind, mvals, X, Y)
        return GK, coef, self.gram(X, Y)
