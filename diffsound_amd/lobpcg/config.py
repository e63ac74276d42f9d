"""Settings, result and tracker state of the modal eigensolver (lobpcg/modal_solver.py)."""
from dataclasses import dataclass, field
from typing import Optional

import torch


@dataclass
class SolverConfig:
    block: int = 0  # search block width b (0 -> k rounded up to a multiple of 8, plus guards)
    guard: int = 8
    # backward-stable criterion of the reference (_lobpcg.py:307-333):
    #   ||K x - lambda M x|| / (||x|| (||K|| + lambda ||M||)) < tol   per wanted pair.
    # fp32 iterates stored in HBM carry rounding noise that K amplifies to ~3 eps32 = 3.5e-7 on this
    # scale, so 2e-6 is ~6x above the floor; the fp64 polish then yields eigenvalues good to ~1e-8.
    tol: float = 0.0  # 0 -> 2e-6 for fp32 iterates, 1e-10 for fp64
    maxit: int = 400
    ortho_passes: int = 2  # at most; a pass is skipped when the previous one left eps * amplification < ortho_tol
    ortho_tol: float = 2e-6
    lock: bool = True  # hard-lock converged leading columns (reference S_ = S[:, nc:ns])
    seed: int = 0
    cheb_degree: int = 8  # terms of the Chebyshev polynomial preconditioner (1 = plain block-Jacobi)
    cheb_ratio: float = 100.0  # the polynomial targets the interval [lmax/ratio, lmax] of T K
    power_iters: int = 30
    # estimates from the previous material's dominant block (same geometry): stop when two successive estimates agree to
    # ``warm_power_spread`` (at least two steps); spread 0: exactly ``warm_power_iters`` steps
    warm_power_iters: int = 3
    warm_power_spread: float = 0.003
    lmax_safety: float = 1.2
    lmax_cap: float = 0.0  # rigorous bound lambda_max(T K) <= nodes per element (4 / 10); 0 = none
    # Two-level preconditioner (ops with a ``coarse`` level, i.e. ord-2 meshes): symmetric V-cycle with a
    # Chebyshev block-Jacobi smoother on the fine level and a Chebyshev polynomial solve on the corner-node level.
    precond: str = "auto"  # "auto" (two-level when the ops offer a coarse level) | "chebyshev" | "twolevel"
    smooth_degree: int = 3  # terms of the fine smoother (pre: degree-1 SpMMs from a zero guess, post: degree)
    smooth_ratio: float = 10.0  # the smoother damps [lmax/ratio, lmax] of T K
    coarse_degree: int = 24
    coarse_ratio: float = 400.0
    # Rayleigh-Ritz by recurrence: K X and K P of the new basis are the same linear combinations of
    # K [X P W] as X and P themselves, and X^T K X, X^T K P, P^T K P follow from the small Ritz algebra, so
    # an iteration multiplies only the b new columns W by K and forms only the [X P W]^T (K W) block of
    # the Gram matrix (a third of the SpMM columns, half of the Gram flops).  Every ``rr_refresh``-th
    # iteration recomputes K [X P W] and the whole Gram matrix from the vectors (0 = every iteration).
    rr_refresh: int = 8
    # K X' of the new Ritz block by ONE product K X' (b columns, 0.19 ms at the benchmark size) instead of the update
    # [K X' | K P'] = K [X P W] [Z1 Zp] (a 3b -> 2b column mix, 0.37 ms): K P is then never formed - the Gram blocks among X
    # and P come from the small Ritz algebra and only the residual needs K X - and K X' carries no recurrence error
    kx_fresh: bool = True
    # ... and then K X' and M X' feed nothing but the residual: ops that offer ``residual_fused`` form R = K X' - (M X') diag(lam)
    # and its column norms in ONE walk of the neighbour unions - neither product is written, X' is gathered once instead of
    # twice, and the separate residual pass over three blocks is gone (needs kx_fresh)
    fused_residual: bool = True
    # ... and in the native iteration, when the preconditioner is the bf16 two-level cycle with node blocks on the fine level, that
    # walk writes the cycle's inputs - the bf16 copy of R and the smoother's first iterate - instead of the fp32 R, and the cycle
    # starts at its first term: the same iterates bit for bit, one launch and one pass over the residual block less per iteration
    # (False: the two launches, for comparison)
    residual_handoff: bool = True
    # Round 5 - Rayleigh-Ritz on the RAW basis [Y X P W] (needs fused_residual): W stays as the preconditioner left it; K W and
    # M W come out of ONE walk of the unions (ops.apply_KM), [Y X P W]^T [K W | M W] out of ONE Gram launch; [Y X P] is
    # M-orthonormal, so the projected Cholesky-QR transform of W is known in coefficients only, every block of the Ritz matrix
    # follows from those Gram rows and the recurrence's [X P]^T K [X P], and ONE update [X' P'] = [Y X P W] Z_raw writes the new
    # basis.  Per iteration: [K W | M W], Gram, update - instead of M W, Gram, update of W, K W, Gram, update.  An iteration whose
    # W is too ill-conditioned for a single sweep (eps x amplification >= ortho_tol) takes the explicit route.
    raw_rr: bool = True
    # ... and the same for the START block (round 5): its projection against the rigid block, its M-orthonormalisation and its first
    # Ritz step from ONE [K X0 | M X0] walk, ONE Gram launch and ONE update (needs raw_rr's operators; a start block too
    # ill-conditioned for one sweep takes the explicit route)
    raw_start: bool = True
    # storage of the preconditioner's internal blocks (V-cycle iterates, residuals, corner-level vectors): "bf16" halves
    # the bytes of every fused term - the cycle is bound by them - and leaves the outer iteration counts unchanged
    # (fp32 arithmetic in registers; the cycle's input R and output W stay fp32); "fp32" keeps everything in fp32
    precond_storage: str = "bf16"
    native: bool = True  # run the iteration through ds_lobpcg_iterate when possible (False: the Python loop below)
    # Nested iteration (ops with a ``coarse`` level, cold starts only): the random start block is first iterated on the
    # corner-node (P1) level - 14x fewer non-zeros, the same block width - to ``nested_tol``, and its prolongation
    # P X_c starts the fine solve.  The P1 spectrum is ~6 % off the P2 one, so a loose coarse tolerance is enough;
    # the fine solve then needs ~4 iterations fewer.  0 = off.
    # fp64 refinement (BASELINE.json configs[4], "fp64 eigenvalues"): after the fp32 iteration has converged, the block
    # is iterated further with fp64 vectors and fp64 block values - Rayleigh-Ritz on [Y | X | W], W the (fp32) two-level
    # preconditioner applied to the fp64 residual - until the backward error of every wanted pair is below this
    # (1e-10).  0 = off (the fp64 Rayleigh-Ritz polish of the fp32 block is the result).
    refine_tol: float = 0.0
    refine_maxit: int = 40
    refine_refresh: int = 8  # every this many fp64 steps all Gram blocks are recomputed from the vectors (else by recurrence)
    refine_sweeps: int = 2   # preconditioner sweeps per fp64 step (2: W = B R + B (R - K B R); C5: 21 -> 17 steps, 4.3 -> 3.8 s)
    # Round 6: Rayleigh-Ritz steps (host-bound for one hypothesis alone) traded for preconditioner sweeps (device work).
    # ``start_sweeps`` applications of the preconditioner to the RANDOM start block of a nested start's corner-node phase before its
    # first Ritz step (inverse-power steps: the block arrives dominated by the low end of the spectrum; solves without a nested
    # start ignore it - nothing would project their swept block again).
    # ``precond_sweeps`` / ``nested_precond_sweeps`` - W = B R + B (R - K B R) per iteration on the fine / corner-node level: measured
    # and NOT adopted (one iteration less for twice the cycle: profiles/r06_start_sweeps.txt); Python loop only.
    start_sweeps: int = 0
    # ``ritz_tol`` > 0: a pair counts as converged (and is locked) only when, besides its backward error < tol, its Ritz value moved by
    # less than this (relative) in the last step; ``nested_ritz_tol`` is the corner-node phase's.  The backward error is relative to
    # ||K|| + lambda ||M||, ~1e3 x the wanted eigenvalues: a SMOOTH vector passes the corner phase's loose 3e-3 whatever its Rayleigh
    # quotient is.  A random start block never met that case (its error is high-frequency until the wanted pairs have settled); a swept
    # one did - with 32 modes in a block of 40 the first 16 columns were locked at the first test with Ritz values 2 x off (1.1e10
    # for 5.6e9), the corner phase ran to its iteration cap and the fine level took 10 iterations instead of 5
    # (profiles/r06_start_sweeps.txt).  With the settled test the sweeps help at every block width measured there; any value forbids a
    # lock at the FIRST test, which is what went wrong - 0.05 .. 0.4 measure alike, 0.2 keeps the benchmark's block of 80 at the
    # time it had without the test (0.05 locks one step later there: +1 ms on one hypothesis).
    ritz_tol: float = 0.0
    nested_ritz_tol: float = 0.2
    start_sweeps_fp32: bool = False  # (experiment: the sweeps through the fp32 preconditioner kernels instead of the bf16 driver)
    start_sweeps_qr: bool = False    # (experiment: M-orthonormalise the block after every sweep)
    precond_sweeps: int = 1
    nested_precond_sweeps: int = 1
    # Corner-node levels whose operator object runs the GROUP-block Jacobi (HipModalOps.group_jacobi = 8: T = the inverse of the
    # 24 x 24 diagonal block of every 8-node group of the matrix-core tables): degree and interval ratio of that level's polynomial -
    # in the V-cycle and in the nested start's corner phase - in the place of coarse_degree / coarse_ratio and nested_cheb_*.
    # Chebyshev(14, 150) in T_g K follows Chebyshev(22, 350) in the node blocks' T K iteration for iteration
    # (profiles/r06_group_block_jacobi_gpu.txt).
    group_degree: int = 14
    group_ratio: float = 150.0
    # ... and of the ONE-level polynomial of an operator object that runs the group blocks itself (HipModalOps.one_level_group_jacobi,
    # ord-1 meshes), in the place of cheb_degree / cheb_ratio
    cheb_group_degree: int = 16
    cheb_group_ratio: float = 300.0
    nested_tol: float = 0.0
    nested_maxit: int = 8
    nested_cheb_degree: int = 28
    nested_cheb_ratio: float = 550.0


def tuned_config(order, **over):
    """The eigensolver settings the benchmarks measure (bench.py) as the library's suggestion for a tet mesh of this order:
    the rigorous bound lambda_max(T K) <= nodes per element caps the Chebyshev intervals; on ord-2 meshes the two-level
    V-cycle with Chebyshev(22, ratio 350) on the corner-node level, a nested start to 3e-3 whose random block takes two
    preconditioner sweeps before its first Ritz step; on ord-1 meshes the one-level polynomial Chebyshev(24, ratio 600) (round 6,
    the shape loop of bench.py --workload geom at 50k tets / 32 modes: 10 iterations and 13.0 ms per eigendecomposition against 19
    and 17.6 with the library's plain default Chebyshev(8, 100); start sweeps apply to the corner-node phase of a nested start only: ModalSolver.solve).  ``DiffSoundObj`` uses it when the caller gives no
    ``solver_config`` - a script written against the reference (build_model(...); model.eigen_decomposition()) then runs the
    configuration whose numbers DESIGN.md quotes; ``tol`` stays the library default (2e-6) unless overridden."""
    o2 = int(order) == 2
    cfg = SolverConfig(lmax_cap=float({1: 4, 2: 10}.get(int(order), 0)), coarse_degree=22, coarse_ratio=350.0,
                       nested_tol=3e-3 if o2 else 0.0, nested_maxit=8, nested_cheb_degree=22, nested_cheb_ratio=350.0,
                       start_sweeps=2 if o2 else 0, cheb_degree=8 if o2 else 24, cheb_ratio=100.0 if o2 else 600.0)
    for k_, v_ in over.items():
        if not hasattr(cfg, k_):
            raise TypeError(f"tuned_config: SolverConfig has no field {k_!r}")
        setattr(cfg, k_, v_)
    return cfg


@dataclass
class ModalResult:
    eigenvalues: torch.Tensor  # (k,) fp64, ascending
    vectors: torch.Tensor  # (n, k) M-orthonormal
    a_lambda: torch.Tensor  # (k,) u^T K_lambda u   fp64
    b_mu: torch.Tensor  # (k,) u^T K_mu u       fp64
    m_diag: torch.Tensor  # (k,) u^T M u          fp64 (== 1 up to rounding)
    iterations: int = 0
    rerr: Optional[torch.Tensor] = None  # (k,) last relative residuals
    history: list = field(default_factory=list)
    block_vectors: Optional[torch.Tensor] = None  # (n, b) whole converged block (warm start)
    coarse_iterations: int = 0  # iterations of the corner-node phase of a nested start
    refine_iterations: int = 0  # fp64 refinement steps (SolverConfig.refine_tol)
    refine_history: list = field(default_factory=list)


class SolverState:
    """What a ``tracker`` callback sees after every iteration - the same fields the reference's worker
    exposes (src/lobpcg/_lobpcg.py:246-256, 335-342): ``ivars['istep']``, ``ivars['converged_count']``,
    ``tvars['rerr']``, ``E``, ``X`` and the writable ``bvars['force_stop']``."""

    def __init__(self, iparams, fparams, bparams):
        self.iparams, self.fparams, self.bparams = iparams, fparams, bparams
        self.ivars = {"istep": 0, "converged_count": 0, "iterations_left": iparams.get("niter", 0)}
        self.fvars = {}
        self.bvars = {"force_stop": False}
        self.tvars = {}
        self.E = None
        self.X = None
