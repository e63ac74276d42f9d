"""Device-resident block eigensolver for  K u = lambda M u  (lowest elastic modes of a free body).

This is the engine behind ``lobpcg_func`` / ``DiffSoundObj.eigen_decomposition``.  It is the
"ortho" LOBPCG of Duersch et al. 2018 that the reference's ``src/lobpcg/_lobpcg.py:433-477``
implements, re-designed for MI355X:

  * the search basis  S = [X | P | W]  lives in ONE row-major (n x 3b) fp32 buffer so that the
    stiffness product  K S  is a single BSR-3 block-SpMM launch (the HBM-roofline kernel) and
    the Rayleigh-Ritz matrix  S^T (K S)  is a single tall-skinny MFMA Gram launch with fp64
    accumulation;
  * the six rigid-body modes are deflated analytically (the reference instead asks for k+6
    pairs and drops six, src/utils/utils.py:80-90, and does not converge - SURVEY.md 0.4);
  * the preconditioner is a Chebyshev polynomial in (block-Jacobi)^-1 K, i.e. only more SpMMs;
  * all large operations go through an ``ops`` object (HIP kernels in the product); the small
    (<= 3b x 3b) dense algebra is fp64 ``torch.linalg`` on the same device;
  * a final fp64 Rayleigh-Ritz "polish" on the converged block returns eigenvalues accurate to
    second order in the fp32 iteration error together with the quadratic forms
    u^T K_lambda u, u^T K_mu u needed by the differentiable read-out.

The module is split by concern: ``config.py`` (SolverConfig, tuned_config, ModalResult, SolverState), ``dense.py`` (the small
host algebra and its one-thread guard), ``precond.py`` (the preconditioners), ``refine.py`` (the fp64 refinement behind
``ModalSolver.refine64``, in named phases); every name stays importable from here.

The ``ops`` protocol (``diffsound_amd/hip_ops.py`` on ``block_ops.py``: the HIP implementation; ``oracle/ops_cpu.py``: the CPU stand-in).

Required:
  n, device, dtype, rigid (n x 6 M-orthonormal, or None), counts,
  apply_K(X, out), apply_M(X, out), gram(A, B, symmetric=, exact=) -> fp64, mix(A, C, out, alpha=, beta=), mix_inplace(W, T),
  residual(R, MX, X, lam, src=) -> (||R_j||^2, ||X_j||^2), polish_products(X) -> (Gram matrices of K's terms, their
  coefficients, X^T M X); for the built-in preconditioners cheb_init, cheb_step; for SolverConfig.refine_tol apply_K64,
  apply_M64, rigid64, mix64, gram_blocks.

Optional - the solver probes for each (``getattr`` / ``hasattr``: CpuModalOps and the HIP operators implement subsets) and takes
its plain route without it; where a guard method is named, the capability is used only when the guard accepts the operands:
  apply_KM, guard apply_KM_ok         K X and M X in one walk: the start block and the Ritz step in coefficients (raw_start, raw_rr)
  residual_fused, guard residual_fused_ok   R = K X - M X diag(lam) and its norms in one walk (fused_residual)
  native_lobpcg                       the whole iteration as one native call (returns None to decline)
  chebyshev_apply16                   the one-level polynomial on bf16 iterates (start sweeps; returns False to decline)
  probe_products, norm_probe_key      the operator-norm probe's products in one walk / the geometry's generation: the key of the
                                      probe's per-geometry cache and of the warm power iteration's block
  prolong, prolong_add, coarse        the corner-node level: its operators, the embedding into a given block / added to one
                                      (two-level V-cycle, nested start); restrict, spmm_residual, twolevel_apply go with it
  cheb_spmm                           a fused Chebyshev term (else cheb_step); group_jacobi, group_T: the group-block Jacobi
  combined_k64, residual64, residual64_scaled   the fp64 refinement's fused forms
  vector_forms                        the quadratic forms of the returned fp32 vectors (ModalSolver.vector_forms)
  gram_exact                          flag: Gram products are always fp64 (the Ritz step then stays on the explicit route)
"""
from typing import Callable, Optional

import torch

from .config import ModalResult, SolverConfig, SolverState, tuned_config  # noqa: F401
from .dense import (_basic_ritz, _gen_eigh, _one_thread, _orthonormal_columns, _orthonormalizer_q,  # noqa: F401
                    _project_in_coefficients, _raw_basis_transform, _rr_step, _small, _svqb_transform, _sym,
                    _thread_local_setters, one_blas_thread_for_this_thread, storage_eps)
from .precond import ChebyshevBlockJacobi, TwoLevelChebyshev, _stats  # noqa: F401
from .refine import refine64


def _check_size(n, b, nrigid):
    if n < 3 * b + nrigid:
        raise ValueError(
            "LPBPCG algorithm is not applicable when the number of A rows (={})"
            " is smaller than 3 x the number of requested eigenpairs (={})".format(n, b))


def _fill_start_block(X, X0, generator):
    """X <- [X0 | noise]: the caller's start vectors (already in place when X0 IS X), the remaining columns drawn from
    ``generator``.  Returns the number of columns X0 supplied."""
    n, b = X.shape
    nx0 = 0 if X0 is None else X0.shape[1]
    if nx0 and X0 is not X:
        X[:, :nx0].copy_(X0.to(X.dtype))
    if nx0 < b:
        X[:, nx0:].copy_(torch.randn((n, b - nx0), generator=generator, dtype=torch.float32, device=X.device).to(X.dtype))
    return nx0


def _converged(rel, lam, lam_prev, k, tol, ritz_tol):
    """Number of LEADING wanted pairs that pass the convergence test."""
    conv = rel[:k] < tol
    if ritz_tol > 0.0:  # ... and settled: |theta - theta_before| <= ritz_tol |theta|  (never at the start block's own Ritz values)
        conv = (conv & ((lam[:k] - lam_prev[:k]).abs() <= ritz_tol * lam[:k].abs())) if lam_prev is not None else torch.zeros_like(conv)
    # leading converged pairs only, to keep strict ordering (reference _lobpcg.py:321-328)
    return int(torch.cumprod(conv.to(torch.int32), 0).sum())


def _stagnated(it, worst, best_worst):
    # A tolerance below what the iterates' precision can reach never locks anything; the block then sits converged to
    # rounding while [X P W] degenerates (W and P are noise), the residuals creep up again and, a few iterations later,
    # the block collapses (seen on a random pencil with tol = 1e-6 in fp32: 4e-7 at iteration 22, 3e-4 at 28, garbage at
    # 29).  Stop at the first clear rise above the best residual reached - the block is still good to ~10 x that floor.
    return it > 10 and worst > 10.0 * best_worst and best_worst < 1e-3


class _Basis:
    """The n-sized blocks of one solve.  S = [Y | X | P | W] is one row-major buffer: the rigid basis rides in front of the
    search basis so the projection against [Y, X, P] is ONE Gram + ONE update launch; the active basis S[:, ny:] is what
    the stiffness SpMM and the Rayleigh-Ritz Gram see.  KS holds K times columns of the active basis; S2 / KS2 are the buffers
    an update writes (``swap_S`` / ``swap_KS`` make them current); R, MX, MW are b-column work blocks."""

    def __init__(self, ops, b):
        self.n, self.b = ops.n, b
        self.device, self.dtype = dev, dt = ops.device, ops.dtype
        Y = ops.rigid
        ny = 0 if Y is None else Y.shape[1]
        # Round 5: on the device the rigid block takes 16 columns (its 6 vectors + zero columns) instead of 8, so that X, P and W
        # - 80-column blocks in the benchmark - start at byte offsets 64, 384 and 704 of a 1 KiB row: every 320-byte row piece
        # the neighbour-union products gather is then five whole 64-byte sectors (with 8 columns in front they started 32 bytes
        # into a sector and touched six: K W drew 1.31 x its algorithmic bytes from memory on these operands against 1.17 x
        # on compact blocks, profiles/r04_spmm_pmc_kx.json).  The zero columns cost the Gram / update kernels 3 % more columns.
        if ny and ny % 16 and dev.type == "cuda" and dt == torch.float32 and b % 16 == 0:
            ny = -(-ny // 16) * 16
        self.ny = ny
        self.S, self.S2 = self.wide(ny + 3 * b), self.wide(ny + 3 * b)
        if ny:
            for buf in (self.S, self.S2):
                buf[:, :Y.shape[1]].copy_(Y)
                if ny > Y.shape[1]:
                    buf[:, Y.shape[1]:ny].zero_()
        self.KS, self.KS2 = self.wide(3 * b), self.wide(3 * b)
        self.R, self.MX, self.MW = (torch.empty((self.n, b), dtype=dt, device=dev) for _ in range(3))

    def wide(self, cols):
        """(n x cols) block inside a buffer whose rows are a multiple of 1 KiB apart (fp32 on the device): every 3-row
        panel of a column range then starts at the same offset inside a cache line - the neighbour-union products gather
        such panels, and on the benchmark mesh K X takes 186 us on an 80-column range of a 256-column buffer against 196 us
        with 248 columns (M X 152 against 164; profiles/r04_mb_kx_strided.txt)."""
        ld = cols if (self.device.type != "cuda" or self.dtype != torch.float32) else -(-cols // 256) * 256
        return torch.empty((self.n, ld), dtype=self.dtype, device=self.device)[:, :cols]

    @property
    def X(self):
        return self.S[:, self.ny:self.ny + self.b]

    def swap_S(self):
        self.S, self.S2 = self.S2, self.S

    def swap_KS(self):
        self.KS, self.KS2 = self.KS2, self.KS


def _start_block_transform(G_, ny, b, ortho_tol, eps):
    """The start block's first Ritz step in coefficients (host, fp64; ds_host_start_block of csrc/host_dense.cpp is the same algebra):
    G_ = [Y X0]^T [K X0 | M X0].  Returns (Ritz values, coefficients of X in [Y X0], those in X0 alone, amp) or None."""
    Gyk, Cy = G_[:ny, :b], G_[:ny, b:]
    A = _sym(G_[ny:, :b])
    got = _project_in_coefficients(Cy, _sym(G_[ny:, b:]))
    if got is None:
        return None
    T, _, amp = got
    if not (ortho_tol > 0.0 and eps * amp < ortho_tol):
        return None  # (one sweep would leave eps * amp in the block's orthogonality: the explicit route repairs it)
    A1 = A - Cy.transpose(0, 1) @ Gyk - Gyk.transpose(0, 1) @ Cy
    E_, Z_ = torch.linalg.eigh(_sym(T.transpose(0, 1) @ A1 @ T))
    Cx = T @ Z_
    return E_, torch.cat([-(Cy @ Cx), Cx], 0).contiguous(), Cx.contiguous(), amp


def _ritz_step(GA, Gxp, whole, na, nxp, Q, dev):
    """Rayleigh-Ritz on the active basis [X_a P W] (host, fp64, one LAPACK thread).  GA: its Ritz matrix when ``whole``, else
    the columns [X P W]^T K W alone - the Gram blocks among X and P are then Gxp, the last step's.  Q (or None): the
    active basis in coordinates of the raw basis [Y X P W] (_raw_basis_transform); the coefficients returned are then those of
    [X' P'] in the raw basis.  Returns (Ritz values and coefficients on ``dev``, [X' P']^T K [X' P'] on the host)."""

    def ritz(GA_):
        if whole:
            G = _sym(GA_)
        else:
            G = torch.empty((GA_.shape[0], GA_.shape[0]), dtype=GA_.dtype)
            G[:nxp, :nxp] = Gxp
            G[:, nxp:] = GA_
            G[nxp:, :nxp] = GA_[:nxp].transpose(0, 1)
            G = _sym(G)
        E_, Z1_, Zp_ = _rr_step(G, na)
        ZZ_ = torch.cat([Z1_, Zp_], 1).contiguous()
        Gxp_ = _sym(ZZ_.transpose(0, 1) @ G @ ZZ_)  # [X' P']^T K [X' P'] of the new basis
        if Q is not None:
            ZZ_ = (Q @ ZZ_).contiguous()  # coefficients of [X' P'] in the raw basis [Y X P W]
        return E_, ZZ_, Gxp_

    if dev.type != "cuda":
        return ritz(GA)
    host = GA.cpu()
    with _one_thread():
        Ea, ZZ, Gxp = ritz(host)
    return Ea.to(dev, non_blocking=True), ZZ.to(dev, non_blocking=True), Gxp


class ModalSolver:
    # ``ModalResult.block_vectors`` - the whole converged block, rotated to its Ritz basis: what a warm start of the next solve takes.
    # A caller that starts every solve cold switches it off and saves one (n x b) update per solve.
    keep_block = True
    # ``ModalResult.a_lambda / b_mu / m_diag`` as the fp64 quadratic forms of the fp32 ``vectors`` the result RETURNS (one more
    # walk of the pattern per term, ``ops.vector_forms``) instead of those of the exact combination of the block that the vectors
    # are the fp32 rounding of: the two differ by that rounding, 2^-24 per entry.  DiffSoundObj switches it on - its callers read
    # the forms together with U_hat -; the hypothesis lanes keep the forms the polish has for free.
    vector_forms = False

    def __init__(self, ops, cfg: Optional[SolverConfig] = None, precond=None, precond_object=None):
        """precond: optional callable (R, W) -> None writing the preconditioned residual into W
        (the ``iK`` argument of the reference API); default Chebyshev block-Jacobi.  precond_object: an already built
        ChebyshevBlockJacobi / TwoLevelChebyshev on these ops (its power iteration is then not repeated)."""
        self.ops = ops
        self.cfg = cfg or SolverConfig()
        self.ortho_log = []
        if precond_object is not None:
            self.precond = precond_object
            self.precond_apply = precond_object.apply
        elif precond is not None:
            self.precond_apply = precond
            self.precond = None
        else:
            two = self.cfg.precond == "twolevel" or (self.cfg.precond == "auto" and getattr(ops, "coarse", None) is not None)
            if two and getattr(ops, "coarse", None) is None:
                raise ValueError("precond='twolevel' needs ops with a coarse level (an ord-2 mesh)")
            if two:
                self.precond = TwoLevelChebyshev(ops, self.cfg)
            else:
                grp = bool(getattr(ops, "group_jacobi", 0))
                self.precond = ChebyshevBlockJacobi(ops, self.cfg.cheb_group_degree if grp else self.cfg.cheb_degree,
                                                    self.cfg.cheb_group_ratio if grp else self.cfg.cheb_ratio,
                                                    self.cfg.power_iters, self.cfg.seed, self.cfg.lmax_safety,
                                                    self.cfg.lmax_cap, warm_iters=self.cfg.warm_power_iters,
                                                    warm_spread=self.cfg.warm_power_spread)
            self.precond_apply = self.precond.apply

    # ------------------------------------------------------------------ helpers
    def _orthonormalize(self, W, V, MW, VW=None):
        """Make W M-orthogonal to the block V (may be None) and M-orthonormal (reference _get_ortho,
        _lobpcg.py:587-679, with a fixed number of passes instead of host-synchronising norms).

        VW: the contiguous block [V | W] when W directly follows V in memory (it does in the solver's basis
        buffer).  V is M-orthonormal, so ONE product M W and ONE Gram launch [V W]^T (M W) give both the
        projection coefficients C = V^T M W and, as G0 - C^T C, the Gram matrix of the projected block; the
        projection and the Cholesky-QR transform are then one update W <- [V W] [-C T; T].  The closed form is used
        for the first sweep only and abandoned when a column turns out to lie (numerically) in span(V); the repair
        sweep, when one is needed, is the explicit project / re-multiply / Cholesky-QR sequence."""
        ops, cfg = self.ops, self.cfg
        eps = storage_eps(ops.dtype)
        nv_ = 0 if V is None else V.shape[1]
        for ip in range(cfg.ortho_passes):
            ops.apply_M(W, MW)
            done = False
            if nv_ > 0 and VW is not None and ip == 0:
                G = ops.gram(VW, MW)  # rows :nv_ = V^T M W, rows nv_: = W^T M W

                def transform(G_, nv=nv_):
                    C = G_[:nv]
                    got = _project_in_coefficients(C, _sym(G_[nv:]), cholesky_gate=True)
                    if got is None:  # the closed form has broken down: take the explicit route for this sweep
                        return None, float("inf")
                    T, _, amp = got
                    return torch.cat([-(C @ T), T], 0).contiguous(), amp

                coef, amp = _small(transform, ops.device, G)
                if coef is not None:
                    ops.mix(VW, coef, W)  # in place: W is the trailing column range of VW (ds_mix allows it)
                    done = True
            if not done:
                if nv_ > 0:
                    C = ops.gram(V, MW)
                    ops.mix(V, C, W, alpha=-1.0, beta=1.0)
                    rem = (C * C).sum(0)  # ||V C_j||_M^2 (V is M-orthonormal): what the projection removed
                    ops.apply_M(W, MW)
                G = ops.gram(W, MW, symmetric=True)
                if nv_ > 0:
                    G = torch.cat([G, rem[None, :].to(G.dtype)], 0)
                T, amp = _small(_orthonormalizer_q, ops.device, G)
                ops.mix_inplace(W, T)
            self.ortho_log.append(amp)
            # a further pass only repairs what this one lost to rounding: eps * amp in the orthogonality of W
            if cfg.ortho_tol > 0.0 and eps * amp < cfg.ortho_tol:
                break

    def _block_width(self, k, X0, rounding):
        """SolverConfig.block, else k rounded up to a multiple of ``rounding``; a wider start block widens it."""
        b = self.cfg.block or ((k + rounding - 1) // rounding) * rounding
        if X0 is not None and X0.shape[1] > b:
            b = ((X0.shape[1] + 3) // 4) * 4
        return b

    def _tolerance(self):
        return self.cfg.tol or (2e-6 if self.ops.dtype == torch.float32 else 1e-10)

    def _lock_width(self, nconv):
        """Locked (converged) leading columns, kept a multiple of 4 for 16-byte aligned slices."""
        return (nconv // 4) * 4 if self.cfg.lock else 0

    def _report(self, state, it, nconv, relk, lam, X, tracker):
        """Publish the step to ``state``, call the tracker; True when the iteration has to stop here."""
        state.ivars.update(istep=it, converged_count=nconv, iterations_left=self.cfg.maxit - it)
        state.tvars["rerr"] = relk
        state.E, state.X = lam, X
        if tracker is not None:
            tracker(state)
        return nconv >= relk.shape[0] or it == self.cfg.maxit or state.bvars.get("force_stop", False)

    # ------------------------------------------------------------------ main entry
    def _nested_start(self, k, b, out=None):
        """Start block of the fine solve from a short solve on the corner-node level (see SolverConfig.nested_tol)."""
        ops, cfg = self.ops, self.cfg
        co = ops.coarse
        if co.rigid is None:
            co.rigid = co._rigid_basis()
        grp = bool(getattr(co, "group_jacobi", 0))
        ccfg = SolverConfig(block=b, guard=cfg.guard, tol=cfg.nested_tol, maxit=cfg.nested_maxit, seed=cfg.seed,
                            cheb_degree=cfg.group_degree if grp else cfg.nested_cheb_degree,
                            cheb_ratio=cfg.group_ratio if grp else cfg.nested_cheb_ratio,
                            cheb_group_degree=cfg.group_degree, cheb_group_ratio=cfg.group_ratio,
                            power_iters=cfg.power_iters, lmax_safety=cfg.lmax_safety,
                            lmax_cap=min(cfg.lmax_cap, 4.0) if cfg.lmax_cap > 0 else 0.0, precond="chebyshev",
                            raw_rr=cfg.raw_rr, raw_start=cfg.raw_start, warm_power_iters=cfg.warm_power_iters,
                            warm_power_spread=cfg.warm_power_spread, start_sweeps=cfg.start_sweeps,
                            start_sweeps_fp32=cfg.start_sweeps_fp32, start_sweeps_qr=cfg.start_sweeps_qr,
                            ritz_tol=cfg.nested_ritz_tol,
                            precond_sweeps=cfg.nested_precond_sweeps, native=cfg.native)
        pre = self.precond.coarse if isinstance(self.precond, TwoLevelChebyshev) else None
        if pre is not None and (pre.degree != ccfg.cheb_degree
                                or abs(pre.lmax / pre.lmin - ccfg.cheb_ratio) > 1e-6 * ccfg.cheb_ratio):
            pre = None  # the V-cycle's corner-level polynomial is reused when it is the one asked for
        cs = ModalSolver(co, ccfg, precond_object=pre)
        rc = cs.solve(k, polish=False)
        self.nested_iterations = rc.iterations
        if out is not None and hasattr(ops, "prolong") and out.dtype == ops.dtype:
            ops.prolong(rc.block_vectors, out)
            return out
        X0 = torch.zeros((ops.n, b), dtype=ops.dtype, device=ops.device)
        ops.prolong_add(rc.block_vectors, X0)
        return X0

    def _sweep_start_block(self, basis, X):
        """Pass the random start block through the preconditioner ``start_sweeps`` times (rigid modes projected out after each)."""
        # ``start_sweeps`` (round 6): the RANDOM start block is passed through the preconditioner before its first Ritz step - steps of
        # a preconditioned inverse subspace iteration without the Ritz algebra.  White noise holds every frequency alike; after two
        # sweeps the block is dominated by the low end of the spectrum and the corner-node level of a nested start reaches its
        # tolerance in 3 iterations instead of 5 (profiles/r06_start_sweeps.txt) - two sweeps are 0.7 ms of device work, two
        # iterations 1 ms of device work plus 3.2 ms of Rayleigh-Ritz on the host thread.
        # ONLY in the corner-node phase of a nested start (the caller's ``polish`` False): the fine level projects and orthonormalises that
        # phase's result again.  A solve that nothing follows keeps its plain random start - on a small problem the swept block collapses
        # onto a few low modes, what is left of its other columns is rounding noise with rigid-body remnants in it, and the start block's
        # normalisation scales that up (two spurious low "eigenvalues" on a 4^3 ord-1 cube when this ran on one-level solves).
        ops, cfg = self.ops, self.cfg
        Y, ny, b = ops.rigid, basis.ny, basis.b
        R, MW, S = basis.R, basis.MW, basis.S
        for _ in range(cfg.start_sweeps):
            R.copy_(X)
            native_sweep = getattr(ops, "chebyshev_apply16", None)
            if not (native_sweep is not None and isinstance(self.precond, ChebyshevBlockJacobi) and cfg.precond_storage == "bf16"
                    and ops.dtype == torch.float32 and not cfg.start_sweeps_fp32 and native_sweep(self.precond, R, X)):
                self.precond_apply(R, X)
            # (every sweep scales the block by ~1 / ||K||: 1e-10 on the benchmark's stiffness - three of them would leave the range
            # the preconditioner's bf16 blocks can hold; back to unit size after each)
            X.mul_(1.0 / X.abs().max().clamp(min=1e-30))
            # ... and the rigid modes leave after each: the preconditioner approximates K^-1, so the null vectors of K are amplified by
            # p(0) - on a small mesh, whose lowest elastic modes lie INSIDE the polynomial's interval, ~30 x more per sweep than
            # anything wanted; two sweeps later the block is rigid motion with the elastic content in its last fp32 digits, and the
            # start block's projection in coefficients cannot recover it (six ~zero "eigenvalues" came back on a 4^3 ord-1 cube:
            # tests/test_api_gpu.py::test_shape_loop_on_one_object_matches_fresh_objects).  X <- X - Y (Y^T M X), Y M-orthonormal.
            if Y is not None:
                ops.apply_M(X, MW)
                ops.mix(Y, ops.gram(Y, MW), X, alpha=-1.0, beta=1.0)
            if cfg.start_sweeps_qr:  # (experiment: M-orthonormalise between the sweeps - a true block inverse iteration)
                self._orthonormalize(X, S[:, :ny] if ny else None, MW, VW=S[:, :ny + b] if ny else None)

    def _operator_norms(self, generator, drawn, cache=True):
        """(||K||, ||M||) estimated with a random 8-column block, as the reference does (_lobpcg.py:280-285); ``drawn``: the number
        of columns the start block took from ``generator`` before."""
        # (The probe block is the same every time - same seed, same number of columns drawn before it - and ||M G0|| depends on
        # the geometry only: operators that can name their geometry's generation keep the block, its norm and ||M G0|| / ||G0||
        # from one solve to the next; a pass then multiplies the block by K alone.  Same numbers, bit for bit.)
        # ``cache`` False (solve_basic): a fresh probe whatever the operators offer, K before M - each caller keeps the order of
        # the two products it always had (tests/test_solver_cpu.py compares the call traces).
        ops, cfg = self.ops, self.cfg
        n, dev, dt = ops.n, ops.device, ops.dtype

        def probe():
            G0 = torch.randn((n, 8), generator=generator, dtype=torch.float32, device=dev).to(dt)
            return G0, torch.linalg.vector_norm(G0.double())

        def norm_of(apply, G0, gn):
            G1 = torch.empty_like(G0)
            apply(G0, G1)
            return torch.linalg.vector_norm(G1.double()) / gn

        if not cache:
            G0, gn = probe()
            return norm_of(ops.apply_K, G0, gn), norm_of(ops.apply_M, G0, gn)
        pkey = getattr(ops, "norm_probe_key", None)
        pkey = None if pkey is None else (pkey(), cfg.seed, drawn, n, str(dt))
        kept = getattr(ops, "_norm_probe", None)
        terms = None
        if pkey is not None and kept is not None and kept[0] == pkey:
            _, G0, gn, B_norm, terms = kept
        else:
            G0, gn = probe()
            # operators of the form K = sum c_i K_i with geometry-only terms (the linear material: lam K_lambda + mu K_mu) hand over
            # K_i G0 and M G0 of ONE walk; ||K G0|| of every material on this geometry is then a small vector operation
            prods = ops.probe_products(G0) if pkey is not None and hasattr(ops, "probe_products") else None
            if prods is not None:
                terms = (prods[0], prods[1])
                B_norm = torch.linalg.vector_norm(prods[2]) / gn
            else:
                B_norm = norm_of(ops.apply_M, G0, gn)
            if pkey is not None:
                ops._norm_probe = (pkey, G0, gn, B_norm, terms)
        if terms is not None:
            cl, cm = ops.lame
            A_norm = torch.linalg.vector_norm(torch.add(terms[0] * float(cl), terms[1], alpha=float(cm))) / gn
        else:
            A_norm = norm_of(ops.apply_K, G0, gn)
        return A_norm, B_norm

    def _start_ritz_raw(self, basis):
        """The start block's first Ritz step in coefficients.  Returns the Ritz values with ``basis`` holding the rotated block (and its
        K X where the iteration reads it), or None - nothing rotated - when the operators or the block call for ``_start_ritz_explicit``."""
        # The start block's projection against Y, its M-orthonormalisation and its first Ritz step IN COEFFICIENTS (round 5,
        # the raw-basis idea of the iteration applied to the start): K X0 and M X0 in ONE walk, [Y X0]^T [K X0 | M X0] in ONE
        # Gram launch, then on the host C = Y^T M X0, B = X0^T M X0 - C^T C, the Cholesky-QR transform T of B, the Ritz pairs
        # of T^T (X0^T K X0 - C^T (Y^T K X0) - (Y^T K X0)^T C) T, and ONE update X = [Y X0] [-C T Z; T Z] (K X = (K X0) T Z:
        # K Y = 0).  Before: M X0, a Gram, an update, K X, a Gram, two updates - and twice the first three when the block
        # was far from orthonormal.  A block too ill-conditioned for one sweep takes that explicit route as before.
        ops, cfg = self.ops, self.cfg
        dev, dt, ny, b = ops.device, ops.dtype, basis.ny, basis.b
        X, KS = basis.X, basis.KS
        if not (cfg.raw_rr and cfg.raw_start and ny and getattr(ops, "apply_KM_ok", None) is not None and b % 4 == 0
                and ops.apply_KM_ok(X, KS[:, :b], KS[:, b:2 * b])):
            return None
        ops.apply_KM(X, KS[:, :b], KS[:, b:2 * b])
        eps_ = storage_eps(dt)
        Gs = ops.gram(basis.S[:, :ny + b], KS[:, :2 * b])
        if dev.type == "cuda" and cfg.native and dt == torch.float32:
            # (the same algebra on the host thread in ONE native call with the solver loop's LAPACK table - ds_host_start_block, csrc/host_dense.cpp -
            # instead of ~30 torch calls on 80 x 80 CPU tensors: 0.65 -> 0.3 ms per start block, two per pass; round 6)
            from .. import _hip

            got = _hip.host_start_block(Gs.cpu(), ny, b, cfg.ortho_tol, eps_)
            if got is not None:
                got = (got[0].to(dev), got[1].to(dev), got[2].to(dev), got[3])
        else:
            got = _small(lambda G_: _start_block_transform(G_, ny, b, cfg.ortho_tol, eps_), dev, Gs)
        _stats(ops, "raw_start_stats")[0 if got is not None else 1] += 1  # (diagnostic counters: taken, handed to the explicit route)
        if got is None:
            return None
        lam, coef, Cx, amp = got
        lam = lam.clone()
        self.ortho_log.append(amp)
        ops.mix(basis.S[:, :ny + b], coef, basis.S2[:, ny:ny + b])
        basis.swap_S()
        # K X of the new block (K Y = 0) - which nobody reads when the iteration forms its residuals in one walk of the
        # unions (fused_residual with kx_fresh: K X' is formed inside that kernel): the update is skipped then (round 6)
        if not (cfg.fused_residual and cfg.kx_fresh and cfg.rr_refresh > 0 and hasattr(ops, "residual_fused")
                and ops.residual_fused_ok(basis.X, basis.R)):
            ops.mix(KS[:, :b], Cx, basis.KS2[:, :b])
            basis.swap_KS()
        return lam

    def _start_ritz_explicit(self, basis):
        """The start block made M-orthogonal to Y and M-orthonormal by explicit sweeps, then rotated to its Ritz basis: returns the
        Ritz values with ``basis`` holding the rotated block and its K X."""
        ops, ny, b = self.ops, basis.ny, basis.b
        X, KS = basis.X, basis.KS
        self._orthonormalize(X, basis.S[:, :ny], basis.MW, VW=basis.S[:, :ny + b] if ny else None)
        ops.apply_K(X, KS[:, :b])
        lam, Z = _small(lambda G: torch.linalg.eigh(_sym(G)), ops.device, ops.gram(X, KS[:, :b], symmetric=True))
        lam = lam.clone()
        ops.mix(X, Z, basis.S2[:, ny:ny + b])
        basis.swap_S()
        ops.mix(KS[:, :b], Z, basis.KS2[:, :b])  # K X of the rotated block
        basis.swap_KS()
        return lam

    def _iterate_native(self, basis, k, lam, A_norm, B_norm, tol, state):
        """The iteration as one native call: (iterations, lam, rel, history) with ``basis`` holding the result, or None when the
        Python loop has to run."""
        # The iteration as ONE native call (ds_lobpcg_iterate) when the ops offer it and nothing needs the interpreter
        # between iterations (no tracker callback - the caller's test -, the built-in preconditioners): same kernels, same dense
        # steps, but a hypothesis lane then runs its whole solve without the interpreter lock.
        ops, cfg = self.ops, self.cfg
        if not (cfg.native and self.precond is not None and ops.dtype == torch.float32 and hasattr(ops, "native_lobpcg")):
            return None
        native = ops.native_lobpcg(self.precond, cfg, k, basis.b, basis.ny, basis.S, basis.S2, basis.KS, basis.KS2, basis.R,
                                   basis.MX, basis.MW, lam, float(A_norm), float(B_norm), tol)
        if native is None:
            return None
        it, in_s2, lam, rel, history = native
        if in_s2:
            basis.swap_S()
            basis.swap_KS()
        state.ivars.update(istep=it, converged_count=int((rel[:k] < tol).sum()), iterations_left=cfg.maxit - it)
        state.tvars["rerr"] = rel[:k]
        state.E, state.X = lam, basis.X
        return it, lam, rel, history

    def _update_basis(self, basis, ZZ, raw, fused, ncl, npc, k0):
        """[X' P'] = S_a ZZ into the other buffer (and their products with K where the configuration keeps them), which then
        becomes current.  S_a = the active basis [X_a P W], or with ``raw`` the whole raw basis [Y X P W]."""
        ops, cfg = self.ops, self.cfg
        ny, b = basis.ny, basis.b
        S, S2, KS, KS2 = basis.S, basis.S2, basis.KS, basis.KS2
        na = b - ncl
        sz = na + npc + na
        if ncl:
            S2[:, ny:ny + ncl].copy_(S[:, ny:ny + ncl])
        Sa = S[:, :ny + b + npc + na] if raw else S[:, ny + ncl:ny + ncl + sz]
        KSa = KS[:, k0:k0 + sz]
        # X_new | P_new (and K X_new | K P_new) are adjacent column ranges: ONE update [X' P'] = [X P W] [Z1 Zp]
        # per product reads the 240-column operand once instead of twice (the LDS-staged mix kernel holds the
        # 240 x 160 coefficient image; with the first, register-only kernel one wide launch was slower than two)
        if 2 * na <= 160:
            ops.mix(Sa, ZZ, S2[:, ny + ncl:ny + b + na])
            if not cfg.kx_fresh:
                ops.mix(KSa, ZZ, KS2[:, :2 * na])
        else:
            Z1, Zp = ZZ[:, :na], ZZ[:, na:]
            ops.mix(Sa, Z1, S2[:, ny + ncl:ny + b])
            ops.mix(Sa, Zp, S2[:, ny + b:ny + b + na])
            if not cfg.kx_fresh:
                ops.mix(KSa, Z1, KS2[:, :na])  # K X_new
                ops.mix(KSa, Zp, KS2[:, na:2 * na])  # K P_new
        if cfg.kx_fresh and not fused:
            ops.apply_K(S2[:, ny + ncl:ny + b], KS2[:, :na])  # K X_new, fresh (K P_new is never needed)
        basis.swap_S()
        basis.swap_KS()

    def _iterate_python(self, basis, k, lam, A_norm, B_norm, tol, state, tracker):
        """The iteration in the interpreter: residuals and the convergence test, locking, W = B R, Rayleigh-Ritz on [X_a P W], the
        update - until the wanted pairs have converged.  Returns (iterations, lam, rel, history) with ``basis`` holding the block."""
        ops, cfg = self.ops, self.cfg
        dev, ny, b = ops.device, basis.ny, basis.b
        R, MX, MW = basis.R, basis.MX, basis.MW
        history = []
        it = 0
        ncl = 0  # locked (converged) leading columns, kept a multiple of 4 for 16-byte aligned slices
        npc = 0  # columns of P
        k0 = 0  # first column of K X_active inside KS (columns locked since the last Ritz step are skipped)
        # Gram blocks of the part of the basis that the last Ritz step produced: [X_a P]^T K [X_a P] (host, fp64)
        Gxp = torch.diag(lam.detach().to(torch.float64).cpu()) if dev.type == "cuda" else torch.diag(lam.to(torch.float64))
        since_refresh = 0
        best_worst = float("inf")
        rel = torch.full((b,), float("inf"), dtype=torch.float64, device=dev)
        lam_prev = None  # Ritz values of the step before (cfg.ritz_tol)
        for it in range(cfg.maxit + 1):
            S, KS = basis.S, basis.KS
            na = b - ncl
            X = basis.X
            Xa = X[:, ncl:]
            fused = (cfg.fused_residual and cfg.kx_fresh and hasattr(ops, "residual_fused")
                     and ops.residual_fused_ok(Xa, R[:, :na]))
            if fused:
                rn2, xn2 = ops.residual_fused(Xa, lam[ncl:], R[:, :na])
            else:
                ops.apply_M(Xa, MX[:, :na])
                # R <- K X - M X lam on the active columns (K X_active sits at column k0 = 0 of KS here: the Ritz step
                # has just rewritten it), with ||R_j||^2 and ||X_j||^2 in fp64
                rn2, xn2 = ops.residual(R[:, :na], MX[:, :na], Xa, lam[ncl:], src=KS[:, k0:k0 + na])
            rel[ncl:] = torch.sqrt(rn2 / xn2) / (A_norm + lam[ncl:].abs() * B_norm)
            relk = rel[:k]
            nconv = _converged(rel, lam, lam_prev, k, tol, cfg.ritz_tol)
            history.append((it, float(relk.max())))
            if self._report(state, it, nconv, relk, lam, X, tracker):
                break
            best_worst = min(best_worst, history[-1][1])
            if _stagnated(it, history[-1][1], best_worst):
                state.bvars["stagnated"] = True
                break
            # hard locking as in the reference (S_ = S[:, nc:ns], _lobpcg.py:458): converged leading columns
            # leave the Rayleigh-Ritz problem, the residual block and the preconditioner; they stay in V
            new_ncl = self._lock_width(nconv)
            if new_ncl > ncl:
                shift = new_ncl - ncl
                R[:, :na - shift].copy_(R[:, shift:na].clone())
                Gxp = Gxp[shift:, shift:]
                k0 += shift
                ncl = new_ncl
                na = b - ncl
            w0 = ny + b + npc
            W = S[:, w0:w0 + na]
            self.precond_apply(R[:, :na], W)
            for _ in range(max(0, cfg.precond_sweeps - 1)):  # (experiment: W <- W + B (R - K W))
                ops.apply_K(W, MW[:, :na])
                torch.sub(R[:, :na], MW[:, :na], out=MX[:, :na])
                self.precond_apply(MX[:, :na], MW[:, :na])
                W += MW[:, :na]
            sz = na + npc + na
            Sa = S[:, ny + ncl:ny + ncl + sz]
            KSa = KS[:, k0:k0 + sz]
            full = cfg.rr_refresh <= 0 or since_refresh >= cfg.rr_refresh
            rawQ = None  # Rayleigh-Ritz on the raw basis (SolverConfig.raw_rr): (G, Q) of _raw_basis_transform
            if (cfg.raw_rr and fused and not full and hasattr(ops, "apply_KM") and not getattr(ops, "gram_exact", False)
                    and ops.apply_KM_ok(W, KS[:, :na], KS[:, na:2 * na])):
                ops.apply_KM(W, KS[:, :na], KS[:, na:2 * na])
                GG = ops.gram(S[:, :w0 + na], KS[:, :2 * na])
                eps_ = storage_eps(ops.dtype)
                lam_l = lam[:ncl].detach().to(torch.float64).cpu()
                if dev.type == "cuda":
                    with _one_thread():
                        rawQ = _raw_basis_transform(GG.cpu(), Gxp, lam_l, ny, ncl, na + npc, na, cfg.ortho_tol, eps_)
                else:
                    rawQ = _raw_basis_transform(GG, Gxp, lam_l, ny, ncl, na + npc, na, cfg.ortho_tol, eps_)
                if rawQ is not None:
                    since_refresh += 1
            if rawQ is None:
                self._orthonormalize(W, S[:, :w0], MW[:, :na], VW=S[:, :w0 + na])
            if rawQ is not None:
                GA = rawQ[0]
            elif full:
                ops.apply_K(Sa, KSa)
                GA = ops.gram(Sa, KSa, symmetric=True)
                since_refresh = 0
            else:
                # only the new columns meet K; the Gram blocks among X and P come from the last Ritz step
                ops.apply_K(W, KSa[:, na + npc:])
                GA = ops.gram(Sa, KSa[:, na + npc:])  # (sz x na) = [X P W]^T K W
                since_refresh += 1
            Ea, ZZ, Gxp = _ritz_step(GA, Gxp, full or rawQ is not None, na, na + npc, None if rawQ is None else rawQ[1], dev)
            if cfg.ritz_tol > 0.0:
                lam_prev = lam.clone()
            lam[ncl:] = Ea
            self._update_basis(basis, ZZ, rawQ is not None, fused, ncl, npc, k0)
            k0 = 0
            npc = na
        return it, lam, rel, history

    def solve(self, k: int, X0: Optional[torch.Tensor] = None, tracker: Optional[Callable] = None,
              state: Optional[SolverState] = None, polish: bool = True) -> ModalResult:
        """The lowest k elastic eigenpairs: buffers, start block (a nested start's, the caller's X0, noise), operator norms, the
        start block's first Ritz step, the iteration (native or in the interpreter), the fp64 polish and, when asked, the fp64
        refinement."""
        ops, cfg = self.ops, self.cfg
        n = ops.n
        b = self._block_width(k + cfg.guard, X0, 8)
        self.nested_iterations = 0
        nested = (X0 is None and cfg.nested_tol > 0.0 and getattr(ops, "coarse", None) is not None
                  and hasattr(ops, "prolong_add") and ops.coarse.n >= 3 * b + 6)
        _check_size(n, b, 0 if ops.rigid is None else 6)
        state = state or SolverState({"niter": cfg.maxit, "k": k, "n": b, "m": n}, {}, {})
        basis = _Basis(ops, b)
        X = basis.X
        g = torch.Generator(device=ops.device).manual_seed(cfg.seed)
        if nested:  # (the prolongated corner-level block goes straight into the basis buffer)
            X0 = self._nested_start(k, b, out=X)
        nx0 = _fill_start_block(X, X0, g)
        if X0 is None and not polish:  # (the corner-node phase of a nested start only: see _sweep_start_block)
            self._sweep_start_block(basis, X)
        A_norm, B_norm = self._operator_norms(g, b - nx0)
        state.fvars.update(A_norm=float(A_norm), B_norm=float(B_norm))
        tol = self._tolerance()
        lam = self._start_ritz_raw(basis)
        if lam is None:
            lam = self._start_ritz_explicit(basis)
        done = self._iterate_native(basis, k, lam, A_norm, B_norm, tol, state) if tracker is None else None
        if done is None:
            done = self._iterate_python(basis, k, lam, A_norm, B_norm, tol, state, tracker)
        it, lam, rel, history = done
        X = basis.X
        if not polish:  # (the corner-level phase of a nested start: the rotated fp32 block is all that is wanted)
            return ModalResult(lam[:k].clone(), X[:, :k], None, None, None, iterations=it, rerr=rel[:k].clone(),
                               history=history, block_vectors=X.contiguous())
        res = self._polish(X, k, it, rel[:k].clone(), history)
        res.coarse_iterations = self.nested_iterations
        if cfg.refine_tol > 0.0:
            res = self.refine64(res, k, float(A_norm), float(B_norm))
            # (the refinement has released the combined fp64 K array itself, also when a step raised; this second release is the
            # one the recorded call trace has after the read-out - tests/golden/solver_call_traces.json)
            if hasattr(self.ops, "combined_k64"):
                self.ops.combined_k64(False)
        return res

    # ------------------------------------------------------------------ the reference's "basic" method
    def solve_basic(self, k, X0=None, tracker=None, state=None):
        """``method='basic'`` of the reference API (src/lobpcg/_lobpcg.py:390-431, ``_update_basic``): NO explicit orthogonalisation of
        the search directions - every step's basis S = [X_active | P | W] goes through the Rayleigh-Ritz transform
        Ri = D^-1/2 chol(D^-1/2 S^T B S D^-1/2)^-T (``_get_rayleigh_ritz_transform``, :479-525) and the eigenvectors of
        Ri^T (S^T A S) Ri give X' = S Ri Z[:, :n - nc] and P' = S Ri Z[:, n : 2n - nc].  Same convergence test and hard locking of the
        leading converged pairs as the ortho iteration.  It is the textbook LOBPCG: cheaper per step than 'ortho' and less robust
        (the Gram matrix of a nearly dependent [X P W] loses its Cholesky factor close to convergence: the step is then repeated
        without P, and without progress the iteration stops) - the product's own solves use 'ortho'; this exists so that a caller of
        the reference API who asks for 'basic' gets that iteration (round 6; rounds 1-5 served it by the ortho iteration).  Large
        operations through ``ops`` (HIP kernels), the <= 3n x 3n dense steps in fp64 on the host.  No rigid-mode deflation."""
        ops, cfg = self.ops, self.cfg
        n, dev, dt = ops.n, ops.device, ops.dtype
        b = self._block_width(k, X0, 4)
        _check_size(n, b, 0)
        state = state or SolverState({"niter": cfg.maxit, "k": k, "n": b, "m": n}, {}, {})
        g = torch.Generator(device=dev).manual_seed(cfg.seed)
        S = torch.empty((n, 3 * b), dtype=dt, device=dev)
        AS, BS = torch.empty_like(S), torch.empty_like(S)
        S2 = torch.empty((n, 2 * b), dtype=dt, device=dev)
        R = torch.empty((n, b), dtype=dt, device=dev)
        nx0 = _fill_start_block(S[:, :b], X0, g)
        A_norm, B_norm = (float(t) for t in self._operator_norms(g, b - nx0, cache=False))
        state.fvars.update(A_norm=A_norm, B_norm=B_norm)
        tol = self._tolerance()
        eps = storage_eps(dt)

        lam = torch.zeros(b, dtype=torch.float64, device=dev)
        rel = torch.full((b,), float("inf"), dtype=torch.float64, device=dev)
        nc, npc, ns = 0, 0, b  # converged leading columns, columns of P, columns of S in use
        history = []
        it = 0
        for it in range(cfg.maxit + 1):
            Sa = S[:, nc:ns]
            w = ns - nc
            ops.apply_K(Sa, AS[:, :w])
            ops.apply_M(Sa, BS[:, :w])
            GA, GB = ops.gram(Sa, AS[:, :w], exact=True), ops.gram(Sa, BS[:, :w], exact=True)
            na = b - nc
            keep = na if it == 0 else min(w, 2 * na)
            out = _small(lambda a_, b_, keep_=keep: _basic_ritz(a_, b_, eps, keep_), dev, GA, GB)
            if out is None and npc:  # [X P W] numerically dependent: the step without P
                idx = torch.cat([torch.arange(0, na, device=dev), torch.arange(na + npc, w, device=dev)])
                keep = na
                out = _small(lambda a_, b_, keep_=keep: _basic_ritz(a_, b_, eps, keep_), dev, GA[idx][:, idx].contiguous(), GB[idx][:, idx].contiguous())
                if out is not None:
                    Zf = torch.zeros((w, keep), dtype=torch.float64, device=dev)
                    Zf[idx] = out[1]
                    out = (out[0], Zf)
            if out is None:
                break  # (no factorisation even without P: the block has collapsed; what has converged so far is returned)
            E_, C = out
            lam[nc:] = E_[:na]
            # X' | P' = S_ (Ri Z): one update into the other buffer, then back (the locked columns stay where they are)
            ops.mix(Sa, C, S2[:, :keep])
            npc = keep - na
            S[:, nc:nc + keep].copy_(S2[:, :keep])  # (X' over the active X, P' behind it: S = [X_locked | X' | P' | W])
            Xa = S[:, nc:b]
            ops.apply_K(Xa, AS[:, :na])
            ops.apply_M(Xa, BS[:, :na])
            rn2, xn2 = ops.residual(R[:, :na], BS[:, :na], Xa, lam[nc:], src=AS[:, :na])
            rel[nc:] = torch.sqrt(rn2 / xn2) / (A_norm + lam[nc:].abs() * B_norm)
            relk = rel[:k]
            nconv = _converged(rel, lam, None, k, tol, 0.0)
            history.append((it, float(relk.max())))
            if self._report(state, it, nconv, relk, lam, S[:, :b], tracker):
                break
            new_nc = self._lock_width(nconv)
            shift = new_nc - nc
            if shift > 0:  # newly converged leading columns leave the active set (X_active = S[:, nc:b]; P stays at S[:, b:])
                nc = new_nc
                na = b - nc
            Wc = S[:, b + npc:b + npc + na]
            if shift > 0:
                Rn = R[:, shift:shift + na].contiguous()
            else:
                Rn = R[:, :na]
            self.precond_apply(Rn, Wc)
            ns = b + npc + na
            # layout for the next step: S[:, nc:ns] = [X_active (na) | P (npc) | W (na)]
        X = S[:, :b]
        res = self._polish(X, k, it, rel[:k].clone(), history)
        return res

    # ------------------------------------------------------------------ fp64 refinement
    def refine64(self, res, k, A_norm, B_norm):
        """Continue from the converged fp32 block with fp64 vectors (see SolverConfig.refine_tol): lobpcg/refine.py."""
        return refine64(self, res, k, A_norm, B_norm)

    # ------------------------------------------------------------------ fp64 Rayleigh-Ritz polish
    def _polish(self, X, k, it, rerr, history):
        ops = self.ops
        GK, coef, GM = ops.polish_products(X)  # fp64 (b x b) Gram matrices of the terms of K, and of M
        coef = [float(c) for c in coef]

        def small(GM_, *GK_):
            # everything (b x b) on the host, fp64, one LAPACK thread: the generalised Ritz problem and the quadratic forms
            # u^T K_i u, u^T M u of the wanted pairs.  (Until round 5 the quadratic forms were torch matmuls on the device: eight
            # more tiny launches per pass, and rocBLAS is free to sum a split-K product with atomics - the one place of a pass whose
            # last bits were not tied down; tests/test_fullsize_gpu.py compares two 8-lane runs bit for bit.)
            GB_ = _sym(GM_)
            E_, C_ = _gen_eigh(_sym(sum(c * G for c, G in zip(coef, GK_))), GB_)  # generalized eigenvectors, C^T GB C = I
            Ck_ = C_[:, :k].contiguous()
            quad = lambda G: ((Ck_.transpose(0, 1) @ _sym(G)) * Ck_.transpose(0, 1)).sum(1)
            qs = torch.stack([quad(G) for G in GK_] + [quad(GB_)])
            return E_[:k].clone(), C_, Ck_, qs

        if ops.device.type == "cuda" and self.cfg.native and ops.dtype == torch.float32:
            # (ds_host_polish, csrc/host_dense.cpp: the same algebra in one native call on the host thread, 1.1 -> 0.5 ms per pass; round 6)
            from .. import _hip

            try:
                E, C, qs = _hip.host_polish([G.cpu() for G in GK], coef, GM.cpu(), k)
            except RuntimeError as ex:  # (X^T M X not positive definite: the error the torch form raises)
                raise torch.linalg.LinAlgError(str(ex)) from ex
            Ck = C[:, :k].contiguous()
            dev_ = ops.device
            E, C, Ck, qs = E.to(dev_), C.to(dev_), Ck.to(dev_), qs.to(dev_)
        else:
            E, C, Ck, qs = _small(small, ops.device, GM, *GK)
        U = torch.empty((ops.n, k), dtype=ops.dtype, device=ops.device)
        ops.mix(X, Ck, U)
        a = qs[0]
        bq = qs[1] if len(GK) > 1 else None
        m = qs[-1]
        if self.vector_forms and hasattr(ops, "vector_forms"):
            forms, m = ops.vector_forms(U)
            a, bq = forms[0], (forms[1] if len(forms) > 1 else None)
        Xb = None
        if self.keep_block or self.cfg.refine_tol > 0.0:  # (the whole rotated block: a warm start's or the refinement's input)
            Xb = torch.empty_like(X)
            ops.mix(X, C, Xb)
        return ModalResult(E, U, a, bq, m, iterations=it, rerr=rerr, history=history, block_vectors=Xb)
