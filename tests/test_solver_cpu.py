"""The solver driver (host logic of diffsound_amd.lobpcg.modal_solver) on CPU, with the oracle's
CpuModalOps standing in for the HIP kernels: convergence to ARPACK's eigenvalues, tracker contract,
force_stop, warm start, the reference's ValueError."""
import numpy as np
import pytest
import scipy.sparse.linalg as spla
import torch

from diffsound_amd import meshgen
from diffsound_amd.lobpcg.modal_solver import ModalSolver, SolverConfig
from oracle import fem
from oracle.ops_cpu import CpuModalOps

MAT = (2700.0, 5e10, 0.25)


@pytest.fixture(scope="module")
def cube():
    v, t = meshgen.kuhn_box(4)
    v, t = fem.to_high_order(torch.from_numpy(v), torch.from_numpy(t).long(), 2)
    d = fem.OracleDeform(v, t, 2)
    Kl, Km = fem.assemble_stiffness(d, 1.0, 0.0), fem.assemble_stiffness(d, 0.0, 1.0)
    M3, _ = fem.assemble_mass(v, t, 2, MAT[0])
    lam, mu = fem.lame(MAT[1], MAT[2])
    K = (lam * Kl + mu * Km).tocsr()
    ref = np.sort(spla.eigsh(K, M=M3, k=16 + 6, sigma=20000, return_eigenvectors=False))[6:]
    return dict(Kl=Kl, Km=Km, M3=M3, v=v.numpy(), lam=lam, mu=mu, ref=ref, K=K)


@pytest.mark.parametrize("dtype,tol_eig", [(torch.float32, 1e-6), (torch.float64, 1e-9)])
def test_converges_to_arpack(cube, dtype, tol_eig):
    ops = CpuModalOps(cube["Kl"], cube["Km"], cube["M3"], cube["v"], cube["lam"], cube["mu"], dtype=dtype)
    # The oracle's K restates the reference's fp32 shape-function gradients, so its rigid modes are only
    # null vectors to ~1e-8 ||K||; with the ANALYTIC rigid basis deflated, the backward
    # residual of the fp64 run therefore floors near 1e-8 (the HIP assembly is fp64 and has no such floor).
    tol = 0.0 if dtype == torch.float32 else 5e-8
    res = ModalSolver(ops, SolverConfig(block=24, lmax_cap=10.0, tol=tol)).solve(16)
    ev = res.eigenvalues.numpy()
    assert np.abs(ev - cube["ref"]).max() / cube["ref"].max() < tol_eig
    assert np.abs(ev / cube["ref"] - 1).max() < 100 * tol_eig
    assert res.iterations < 60
    lam, mu = cube["lam"], cube["mu"]
    assert np.abs((lam * res.a_lambda + mu * res.b_mu).numpy() / ev - 1).max() < 1e-9
    U = res.vectors.double().numpy()
    assert np.abs(U.T @ (cube["M3"] @ U) - np.eye(16)).max() < 1e-5
    # rigid modes were deflated: modes are M-orthogonal to the rigid basis
    Y = ops.rigid.double().numpy()
    assert np.abs(Y.T @ (cube["M3"] @ U)).max() < 1e-5


def test_tracker_contract_and_force_stop(cube):
    ops = CpuModalOps(cube["Kl"], cube["Km"], cube["M3"], cube["v"], cube["lam"], cube["mu"])
    seen = []

    def tracker(w):
        seen.append((w.ivars["istep"], w.ivars["converged_count"], w.tvars["rerr"].shape[0]))
        if w.ivars["istep"] == 3:
            w.bvars["force_stop"] = True

    res = ModalSolver(ops, SolverConfig(block=24)).solve(16, tracker=tracker)
    assert [s[0] for s in seen] == [0, 1, 2, 3] and res.iterations == 3
    assert all(s[2] == 16 for s in seen)
    counts = [s[1] for s in seen]
    assert counts == sorted(counts)


def test_warm_start_needs_fewer_iterations(cube):
    ops = CpuModalOps(cube["Kl"], cube["Km"], cube["M3"], cube["v"], cube["lam"], cube["mu"])
    cold = ModalSolver(ops, SolverConfig(block=24)).solve(16)
    lam2, mu2 = fem.lame(MAT[1] * 1.05, MAT[2] + 0.01)
    ops2 = CpuModalOps(cube["Kl"], cube["Km"], cube["M3"], cube["v"], lam2, mu2)
    warm = ModalSolver(ops2, SolverConfig(block=24)).solve(16, X0=cold.block_vectors)
    cold2 = ModalSolver(ops2, SolverConfig(block=24)).solve(16)
    assert warm.iterations < cold2.iterations
    assert np.abs(warm.eigenvalues.numpy() / cold2.eigenvalues.numpy() - 1).max() < 1e-6


def test_too_small_problem_raises_like_the_reference(cube):
    ops = CpuModalOps(cube["Kl"], cube["Km"], cube["M3"], cube["v"], cube["lam"], cube["mu"])
    with pytest.raises(ValueError, match="not applicable"):
        ModalSolver(ops, SolverConfig(block=ops.n // 3 + 8)).solve(ops.n // 3)


def test_underestimated_lmax_is_guarded(cube):
    """The power-iteration estimate of lambda_max(T K) times its safety factor bounds the true value."""
    ops = CpuModalOps(cube["Kl"], cube["Km"], cube["M3"], cube["v"], cube["lam"], cube["mu"], dtype=torch.float64)
    s = ModalSolver(ops, SolverConfig(block=24))
    n = ops.n
    import scipy.sparse as sp

    Dinv = sp.block_diag([b for b in ops.Dinv.numpy()], format="csr")
    true = spla.eigs(Dinv @ cube["K"], k=1, which="LM", return_eigenvectors=False, tol=1e-6).real.max()
    assert s.precond.lmax >= true
    assert s.precond.lmax <= 10.0 * 1.2


def test_two_level_preconditioner(cube):
    """Two-level V-cycle (Chebyshev smoother + corner-node level) on the oracle ops: same eigenvalues, fewer fine
    SpMM columns than the one-level polynomial; the cycle is a symmetric positive definite operator."""
    from diffsound_amd.lobpcg.modal_solver import TwoLevelChebyshev

    v, t = meshgen.kuhn_box(4)
    _, t2 = fem.to_high_order(torch.from_numpy(v), torch.from_numpy(t).long(), 2)
    mk = lambda **kw: CpuModalOps(cube["Kl"], cube["Km"], cube["M3"], cube["v"], cube["lam"], cube["mu"], **kw)
    ops2, ops1 = mk(tets=t2.numpy()), mk()
    assert ops2.coarse is not None and ops2.coarse.n == 3 * 125
    cfg = SolverConfig(block=24, lmax_cap=10.0, cheb_degree=16, cheb_ratio=100.0, smooth_degree=3, coarse_degree=12,
                       coarse_ratio=50.0)
    r2 = ModalSolver(ops2, cfg).solve(16)
    r1 = ModalSolver(ops1, cfg).solve(16)
    assert np.abs(r2.eigenvalues.numpy() / cube["ref"] - 1).max() < 1e-4
    assert np.abs(r2.eigenvalues.numpy() / r1.eigenvalues.numpy() - 1).max() < 1e-5
    assert r2.iterations <= r1.iterations + 4
    assert ops2.counts["apply_K_cols"] < 0.7 * ops1.counts["apply_K_cols"]
    with pytest.raises(ValueError):
        ModalSolver(ops1, SolverConfig(block=24, precond="twolevel"))
    # B = the V-cycle as a matrix: symmetric, positive definite
    ops64 = mk(tets=t2.numpy(), dtype=torch.float64)
    pre = TwoLevelChebyshev(ops64, cfg)
    g = torch.Generator().manual_seed(0)
    R = torch.randn((ops64.n, 8), generator=g, dtype=torch.float64)
    W = torch.empty_like(R)
    pre.apply(R.clone(), W)
    G = (R.double().T @ W.double()).numpy()
    assert np.abs(G - G.T).max() < 1e-9 * np.abs(G).max()
    assert np.linalg.eigvalsh(0.5 * (G + G.T)).min() > 0


def test_fp64_refinement_reaches_1e10_backward_error(cube):
    """configs[4]'s precision path on the CPU stand-in: fp32 iterates first, then the fp64 refinement
    (SolverConfig.refine_tol) until ||K u - lambda M u|| / (||u|| (||K|| + lambda ||M||)) < 1e-10 for every pair;
    eigenvalues against ARPACK (fp64 shift-invert) to 1e-9."""
    ops = CpuModalOps(cube["Kl"], cube["Km"], cube["M3"], cube["v"], cube["lam"], cube["mu"], dtype=torch.float32,
                      tets=None)
    cfg = SolverConfig(block=24, lmax_cap=10.0, refine_tol=1e-10)
    res = ModalSolver(ops, cfg).solve(16)
    assert res.vectors.dtype == torch.float64 and res.eigenvalues.dtype == torch.float64
    assert 1 <= res.refine_iterations <= cfg.refine_maxit and float(res.rerr.max()) < 1e-10
    assert res.refine_history[0] > 1e-8 and res.refine_history == sorted(res.refine_history, reverse=True)
    ev = res.eigenvalues.numpy()
    assert np.abs(ev / cube["ref"] - 1).max() < 1e-9
    # independent residual check
    U = res.vectors.numpy()
    R = cube["K"] @ U - (cube["M3"] @ U) * ev[None, :]
    g = np.random.default_rng(0).standard_normal((cube["K"].shape[0], 4))
    An = np.linalg.norm(cube["K"] @ g) / np.linalg.norm(g)
    Bn = np.linalg.norm(cube["M3"] @ g) / np.linalg.norm(g)
    assert (np.linalg.norm(R, axis=0) / (np.linalg.norm(U, axis=0) * (An + ev * Bn))).max() < 2e-10
    assert np.abs(U.T @ (cube["M3"] @ U) - np.eye(16)).max() < 1e-9
    lam, mu = cube["lam"], cube["mu"]
    assert np.abs((lam * res.a_lambda + mu * res.b_mu).numpy() / ev - 1).max() < 1e-9


@pytest.mark.parametrize("dtype,tol_eig", [(torch.float32, 1e-6), (torch.float64, 1e-9)])
def test_rayleigh_ritz_on_the_raw_basis_on_the_cpu(cube, dtype, tol_eig):
    """Round 5: SolverConfig.raw_rr through the Python loop with the CPU stand-in of the fused operators - K W and M W of the
    raw preconditioned residuals, ONE Gram product [Y X P W]^T [K W | M W], the orthonormalisation folded into the small
    algebra (modal_solver._raw_basis_transform) and ONE update from the raw basis: converges to ARPACK's eigenvalues like the
    explicit route, in the same number of iterations (within one), and really issues fewer Gram products and updates."""
    res, counts = {}, {}
    for raw in (False, True):
        ops = CpuModalOps(cube["Kl"], cube["Km"], cube["M3"], cube["v"], cube["lam"], cube["mu"], dtype=dtype)
        ops.fused = True
        tol = 0.0 if dtype == torch.float32 else 5e-8
        res[raw] = ModalSolver(ops, SolverConfig(block=24, lmax_cap=10.0, tol=tol, raw_rr=raw)).solve(16)
        counts[raw] = dict(ops.counts)
        ev = res[raw].eigenvalues.numpy()
        assert np.abs(ev / cube["ref"] - 1).max() < 100 * tol_eig, raw
        U = res[raw].vectors.double().numpy()
        assert np.abs(U.T @ (cube["M3"] @ U) - np.eye(16)).max() < 1e-5
    assert abs(res[True].iterations - res[False].iterations) <= 1
    assert counts[True]["gram"] < counts[False]["gram"] and counts[True]["mix"] < counts[False]["mix"]


def test_raw_basis_transform_equals_the_explicit_orthonormalisation():
    """modal_solver._raw_basis_transform against the explicit sequence on dense random data: for an M-orthonormal V = [Y X_l X_a P]
    and a raw block W, the Gram rows [V W]^T [K W | M W] must give the same Ritz matrix S_a^T K S_a, S_a = [X_a P W_o], as forming
    W_o = (W - V V^T M W) T explicitly - when K Y = 0 and the locked columns are exact eigenvectors, as the solver assumes."""
    from diffsound_amd.lobpcg.modal_solver import _raw_basis_transform

    rng = np.random.default_rng(5)
    n, ny, ncl, nxp, na = 400, 2, 4, 12, 8
    A = rng.standard_normal((n, n))
    M = A @ A.T / n + np.eye(n)
    Lm = np.linalg.cholesky(M)
    # a K with a null space Y and eigenvectors X_l: K = M Q diag(d) Q^T M with Q M-orthonormal, d = 0 on Y
    Q = np.linalg.solve(Lm.T, np.linalg.qr(rng.standard_normal((n, n)))[0])      # Q^T M Q = I
    d = np.concatenate([np.zeros(ny), np.sort(rng.uniform(1, 2, ncl)), rng.uniform(3, 50, n - ny - ncl)])
    K = M @ Q @ np.diag(d) @ Q.T @ M
    Y, Xl = Q[:, :ny], Q[:, ny:ny + ncl]
    rest = Q[:, ny + ncl:]
    XP = rest @ np.linalg.qr(rng.standard_normal((rest.shape[1], nxp)))[0]       # M-orthonormal, M-orthogonal to Y and X_l
    V = np.concatenate([Y, Xl, XP], 1)
    W = rng.standard_normal((n, na)) + V @ rng.standard_normal((V.shape[1], na))  # a raw block with components in span(V)
    S = np.concatenate([V, W], 1)
    GG = torch.from_numpy(np.concatenate([S.T @ K @ W, S.T @ M @ W], 1))
    Gxp = torch.from_numpy(XP.T @ K @ XP)
    out = _raw_basis_transform(GG, Gxp, torch.from_numpy(d[ny:ny + ncl]), ny, ncl, nxp, na, 0.0, 1e-16)
    assert out is not None
    G, Qc = out
    Sa = S @ Qc.numpy()                                                            # [X_a P W_o] in coordinates of the raw basis
    assert np.abs(Sa[:, :nxp] - XP).max() < 1e-12
    assert np.abs(Sa.T @ M @ Sa - np.eye(nxp + na)).max() < 1e-9                   # M-orthonormal
    assert np.abs(V.T @ M @ Sa[:, nxp:]).max() < 1e-9                              # W_o is M-orthogonal to [Y X_l X_a P]
    ref = Sa.T @ K @ Sa
    assert np.abs(G.numpy() - ref).max() < 1e-9 * np.abs(ref).max()


def test_warm_power_iteration_stops_when_the_block_is_still_converged(cube):
    """The Chebyshev interval's end lambda_max(T K) from the previous estimate's block: TWO steps when successive estimates agree
    (same operator: the block is converged), a fixed count when the early exit is switched off, and as many steps as the estimate
    keeps moving when the block is far from the new operator's dominant vectors - the estimate stays within the 1.2 safety
    factor of the cold one.  The counters live on the operator object (round 6), not on the class."""
    from diffsound_amd.lobpcg.modal_solver import ChebyshevBlockJacobi as C

    ops = CpuModalOps(cube["Kl"], cube["Km"], cube["M3"], cube["v"], cube["lam"], cube["mu"])
    cold = C(ops, 4, 100.0, power_iters=400)  # (long enough for every column of the block to sit in the top of the spectrum)
    assert getattr(ops, "_power_block", None) is not None
    assert getattr(ops, "warm_stats", None) is None and not hasattr(C, "warm_stats")  # (cold: nothing counted; no class counters)
    warm = C(ops, 4, 100.0, power_iters=30)
    assert ops.warm_stats == [1, 2]  # one estimate, two steps (the second confirms the first)
    assert abs(warm.lmax / cold.lmax - 1) < 0.02
    C(ops, 4, 100.0, power_iters=30, warm_spread=0.0, warm_iters=3)
    assert ops.warm_stats == [2, 5]
    # a block that has nothing to do with the operator (fresh noise handed over as if it were warm): its estimate keeps rising
    # from step to step and the iteration goes on until it has settled
    g = torch.Generator().manual_seed(5)
    ops._power_block = torch.randn((ops.n, 8), generator=g, dtype=ops.dtype)
    stale = C(ops, 4, 100.0, power_iters=30)
    assert ops.warm_stats[0] == 3 and ops.warm_stats[1] - 5 > 3
    assert 0.9 * cold.lmax < stale.lmax <= 1.001 * cold.lmax  # (a power iteration's estimate is a lower bound of the true one)


def test_warm_power_iteration_after_an_extreme_material_jump(cube):
    """columns that have collapsed onto the OLD dominant vector agree with each other under any operator, so their
    agreement says nothing about the new material.  After nu 0.49 -> 0.05 (and back) the warm estimate, which now compares
    successive estimates, stays within 10 % below the converged value (measured 6 %: the power iteration crawls on this small mesh) - inside the 1.2 safety factor - where a single step
    would have been accepted at whatever it gave."""
    from diffsound_amd.lobpcg.modal_solver import ChebyshevBlockJacobi as C

    E = 5e10
    lame = lambda nu: (E * nu / ((1 + nu) * (1 - 2 * nu)), E / (2 * (1 + nu)))
    for nu0, nu1 in ((0.49, 0.05), (0.05, 0.49)):
        ops = CpuModalOps(cube["Kl"], cube["Km"], cube["M3"], cube["v"], *lame(nu0))
        C(ops, 4, 100.0, power_iters=400)
        new = CpuModalOps(cube["Kl"], cube["Km"], cube["M3"], cube["v"], *lame(nu1))
        truth = C(new, 4, 100.0, power_iters=600, safety=1.0).lmax
        new._power_block, new._power_block_key = ops._power_block, getattr(ops, "_power_block_key", None)
        one = C(new, 4, 100.0, power_iters=30, safety=1.0, warm_spread=0.0, warm_iters=1).lmax
        new._power_block = ops._power_block
        warm = C(new, 4, 100.0, power_iters=30, safety=1.0).lmax
        assert warm <= truth * (1 + 1e-9) and warm > 0.90 * truth, (nu0, nu1, one / truth, warm / truth)
        assert warm >= one


@pytest.mark.parametrize("dtype,tol_eig", [(torch.float64, 1e-7), (torch.float32, 2e-5)])
def test_start_block_in_coefficients_on_the_cpu(cube, dtype, tol_eig):
    """SolverConfig.raw_start on the oracle's operators: the start block orthonormalised against the rigid block and rotated to
    its Ritz basis in coefficients (one [K X0 | M X0] product, one Gram product, one update) converges to ARPACK's eigenvalues like
    the explicit sequence, in the same number of iterations (within two)."""
    res = {}
    for raw in (True, False):
        ops = CpuModalOps(cube["Kl"], cube["Km"], cube["M3"], cube["v"], cube["lam"], cube["mu"], dtype=dtype)
        ops.fused = True  # (the CPU stand-ins of the fused operators the raw forms need)
        tol = 0.0 if dtype == torch.float32 else 5e-8
        res[raw] = ModalSolver(ops, SolverConfig(block=24, lmax_cap=10.0, tol=tol, raw_start=raw)).solve(16)
        st = getattr(ops, "raw_start_stats", [0, 0])  # (the counters of THIS operator object)
        assert (sum(st) > 0) == raw
        if raw and dtype == torch.float64:  # (a random fp32 block may be too ill-conditioned for one sweep: the explicit route then)
            assert st[0] > 0
        assert np.abs(res[raw].eigenvalues.numpy() / cube["ref"] - 1).max() < 100 * tol_eig, raw
    assert abs(res[True].iterations - res[False].iterations) <= 2


@pytest.mark.parametrize("dtype,tol_eig", [(torch.float64, 1e-8), (torch.float32, 1e-5)])
def test_basic_method_on_the_cpu(cube, dtype, tol_eig):
    """ModalSolver.solve_basic - the reference's ``method='basic'`` (_lobpcg.py:390-431: Rayleigh-Ritz through the transform of
    the basis' Gram matrix, no explicit orthogonalisation, no deflation) - on the oracle's operators: the six rigid modes come
    out as ~zero eigenvalues in front, the elastic ones match ARPACK, the vectors are M-orthonormal."""
    ops = CpuModalOps(cube["Kl"], cube["Km"], cube["M3"], cube["v"], cube["lam"], cube["mu"], dtype=dtype)
    seen = []
    res = ModalSolver(ops, SolverConfig(block=28, lmax_cap=10.0, tol=1e-7 if dtype == torch.float64 else 0.0, maxit=200)).solve_basic(
        20, tracker=lambda st: seen.append((st.ivars["istep"], st.ivars["converged_count"])))
    ev = res.eigenvalues.numpy()
    assert np.abs(ev[:6]).max() < 1e-6 * cube["ref"][0]
    assert np.abs(ev[6:] / cube["ref"][:14] - 1).max() < tol_eig
    assert res.iterations < 60 and seen and seen[0][0] == 0 and seen[-1][1] >= 20
    U = res.vectors.double().numpy()
    assert np.abs(U.T @ (cube["M3"] @ U) - np.eye(20)).max() < 1e-5
    with pytest.raises(ValueError, match="not applicable"):
        ModalSolver(ops, SolverConfig(block=ops.n // 2)).solve_basic(8)


def test_settled_ritz_values_are_part_of_the_convergence_test_when_asked(cube):
    """SolverConfig.ritz_tol: a pair counts as converged only when its Ritz value has also stopped moving.  On a cold start it changes
    nothing that matters (the same eigenvalues, at most one iteration more); a converged block handed back as the start - which the
    backward error alone accepts at its first test, iteration 0 - has to take one step to show that its values stand still."""
    mk = lambda: CpuModalOps(cube["Kl"], cube["Km"], cube["M3"], cube["v"], cube["lam"], cube["mu"], dtype=torch.float64)
    a = ModalSolver(mk(), SolverConfig(block=24, lmax_cap=10.0, tol=5e-8)).solve(16)
    b = ModalSolver(mk(), SolverConfig(block=24, lmax_cap=10.0, tol=5e-8, ritz_tol=1e-3)).solve(16)
    assert a.iterations <= b.iterations <= a.iterations + 1
    assert np.abs(b.eigenvalues.numpy() / cube["ref"] - 1).max() < 1e-7
    w0 = ModalSolver(mk(), SolverConfig(block=24, lmax_cap=10.0, tol=5e-8)).solve(16, X0=a.block_vectors)
    w1 = ModalSolver(mk(), SolverConfig(block=24, lmax_cap=10.0, tol=5e-8, ritz_tol=1e-3)).solve(16, X0=a.block_vectors)
    assert w0.iterations == 0 and w1.iterations == 1
    assert np.abs(w1.eigenvalues.numpy() / cube["ref"] - 1).max() < 1e-7


def test_start_sweeps_are_ignored_without_a_nested_start(cube):
    """SolverConfig.start_sweeps (round 6) belongs to the corner-node phase of a nested start (the GPU suite runs it through the
    benchmark's configuration: tests/test_parity_gpu.py, tests/test_modal_gpu.py).  A solve that nothing follows ignores the
    setting - its swept block would have nobody to project it again: the same iterates, bit for bit."""
    mk = lambda: CpuModalOps(cube["Kl"], cube["Km"], cube["M3"], cube["v"], cube["lam"], cube["mu"], dtype=torch.float64)
    a = ModalSolver(mk(), SolverConfig(block=24, lmax_cap=10.0, tol=5e-8, start_sweeps=0)).solve(16)
    b = ModalSolver(mk(), SolverConfig(block=24, lmax_cap=10.0, tol=5e-8, start_sweeps=3)).solve(16)  # (fresh operators: no warm estimate)
    assert a.iterations == b.iterations and torch.equal(a.eigenvalues, b.eigenvalues)
    assert np.abs(a.eigenvalues.numpy() / cube["ref"] - 1).max() < 1e-7


# ---------------------------------------------------------------------------------------------------------------------
# Call traces: which ``ops`` members a solve calls, in which order, on how many columns.  Recorded once
# (tests/golden/solver_call_traces.json) and compared for equality: restructuring the solver's host code must not change what it
# launches.  The fp32 cases are stopped by their tracker at step 3, so no trace of theirs depends on how many pairs have converged
# by then; the two refinement cases run their fp32 phase to convergence and three fp64 steps (the recording script watches their
# margins).
_TRACED = ("apply_K", "apply_M", "apply_KM", "gram", "mix", "mix_inplace", "residual", "residual_fused",
           "apply_K64", "apply_M64", "gram_blocks", "mix64")  # (... and the fp64 refinement's)
_TRACED_FUSED64 = ("residual64", "residual64_scaled", "combined_k64")


def _columns(arg):
    """What a trace entry says of one argument: a tensor's last dimension; of a LIST of blocks (mix64, gram_blocks) the number
    of blocks and every block's columns - for a ``(block, first row)`` item the row too."""
    if torch.is_tensor(arg):
        return [int(arg.shape[-1])]
    if isinstance(arg, (list, tuple)):
        return [len(arg)] + [int(x) for blk in arg for x in ((blk[0].shape[1], blk[1]) if isinstance(blk, tuple) else blk.shape[1:])]
    return []


class _RecordingOps(CpuModalOps):
    """CpuModalOps that appends [level + member, last dimension of every tensor argument ...] to ``log`` at each traced call."""

    def __init__(self, log, level, *args, **kw):
        super().__init__(*args, **kw)
        self.log, self.level = log, level


class _RecordingOpsFused64(_RecordingOps):
    """... offering the fp64 refinement's fused forms as plain torch stand-ins (the contracts of HipModalOps' members,
    block_ops.py): the branches the solver takes on the device, traceable without one."""

    def residual64(self, KX, MX, X, lam):
        R = torch.addcmul(KX, MX, lam[None, :], value=-1.0)
        return (R * R).sum(0), (X * X).sum(0)

    def residual64_scaled(self, KX, MX, lam, scale, idx, out=None):
        R = (KX[:, idx] - MX[:, idx] * lam[idx][None, :]) * scale[idx][None, :]
        return R.float() if out is None else out.copy_(R)

    def combined_k64(self, on):
        pass  # (the HIP operators keep / release one combined fp64 K array: here only the call is recorded)


def _traced(cls, name):
    inner = getattr(cls, name)

    def call(self, *args, **kw):
        flag = [int(a) for a in args if isinstance(a, bool)]  # (combined_k64's; the others' keyword flags are not in the record)
        self.log.append([self.level + name] + [c for a in args + tuple(kw.values()) for c in _columns(a)] + flag)
        return inner(self, *args, **kw)

    return call


for _name in _TRACED:
    setattr(_RecordingOps, _name, _traced(CpuModalOps, _name))
for _name in _TRACED_FUSED64:
    setattr(_RecordingOpsFused64, _name, _traced(_RecordingOpsFused64, _name))


def _recording_ops(cube, log, two_level=False, fused=False, fused64=False):
    """The cube's operators with every traced call logged.  ``fused64``: offering the refinement's fused forms.  ``two_level``: with a corner-node level that implements the WHOLE
    protocol (the Galerkin products P^T K P, P^T M P and the rigid basis of the corner nodes) - CpuModalOps' own coarse level
    serves the V-cycle only, and a nested start solves an eigenproblem on that level."""
    from oracle.ops_cpu import corner_embedding
    import scipy.sparse as sp

    args = (cube["Kl"], cube["Km"], cube["M3"], cube["v"], cube["lam"], cube["mu"])
    if not two_level:
        ops = (_RecordingOpsFused64 if fused64 else _RecordingOps)(log, "", *args)
    else:
        v, t = meshgen.kuhn_box(4)
        t2 = fem.to_high_order(torch.from_numpy(v), torch.from_numpy(t).long(), 2)[1].numpy()
        ops = _RecordingOps(log, "", *args, tets=t2)
        P = sp.kron(corner_embedding(t2, ops.n // 3), sp.identity(3), format="csr")
        corners = np.unique(t2[:, [0, 2, 4, 9]])
        ops.coarse = _RecordingOps(log, "coarse.", *((P.T @ A @ P).tocsr() for A in args[:3]), cube["v"][corners], *args[4:])
        ops.coarse.fused = fused
    ops.fused = fused
    return ops


_REFINE3 = dict(lmax_cap=10.0, refine_tol=1e-10, refine_maxit=3, seed=4)  # (the seed: see make_solver_call_traces.py)


def _call_traces(cube, monkeypatch, report=None):
    """{case: trace} of the cases below; ``report(case, solver)`` sees every finished solver (the recording script's margins)."""
    from diffsound_amd.lobpcg import modal_solver as ms

    log = []
    for cls in (ms.ChebyshevBlockJacobi, ms.TwoLevelChebyshev):  # every preconditioner application, the nested start's included
        def apply(self, R, W, *a, _inner=cls.apply, _name=cls.__name__, **kw):
            log.append([getattr(self.ops, "level", "") + _name, int(R.shape[1]), int(W.shape[1])])
            return _inner(self, R, W, *a, **kw)

        monkeypatch.setattr(cls, "apply", apply)

    def stop_at_3(state):
        if state.ivars["istep"] == 3:
            state.bvars["force_stop"] = True

    cases = {
        "solve": (dict(), dict(), "solve"),
        "solve_nested_two_level": (dict(two_level=True), dict(nested_tol=3e-3, start_sweeps=2), "solve"),
        "solve_basic": (dict(), dict(), "solve_basic"),
        # ... and the same with the fused operators offered: the start block and the Ritz steps in coefficients
        "solve_fused": (dict(fused=True), dict(), "solve"),
        "solve_nested_two_level_fused": (dict(two_level=True, fused=True), dict(nested_tol=3e-3, start_sweeps=2), "solve"),
        # the fp64 refinement behind a converged fp32 phase (no tracker), three steps: the pencil formed from the vectors on
        # [Y X W], then twice by recurrence on [Y X P W] (the blocks among [Y X P] that a step leaves have the next step's shape, so
        # P's arrival forces no refresh) - plain, and with the fused forms the HIP operators offer
        "solve_refine": (dict(), _REFINE3, "solve"),
        "solve_refine_fused": (dict(fused64=True), _REFINE3, "solve"),
    }
    traces = {}
    for case, (ops_kw, cfg_kw, method) in cases.items():
        ops = _recording_ops(cube, log, **ops_kw)
        solver = ModalSolver(ops, SolverConfig(block=24, **cfg_kw))
        del log[:]  # (the trace is the solve's: the constructor's power iterations are not part of it)
        if cfg_kw is _REFINE3:
            res = solver.solve(16)
            assert res.refine_iterations == 3
        else:
            res = getattr(solver, method)(16, tracker=stop_at_3)
            assert res.iterations == 3
        traces[case] = [list(e) for e in log]
        if report is not None:
            report(case, solver)
    return traces


def test_call_traces_equal_the_recorded_ones(cube, monkeypatch):
    """The sequence of operator calls and preconditioner applications of ``solve`` (one-level; two-level with a nested start and
    start sweeps; each also with the fused operators), of ``solve_basic`` and of ``solve`` with three steps of the fp64 refinement
    (plain, and with its fused forms) on the 4^3 ord-2 cube, k = 16, block = 24, against the sequences recorded before the solver -
    and, later, the refinement - was split into phases (tests/golden/make_solver_call_traces.py)."""
    import json
    import os

    with open(os.path.join(os.path.dirname(__file__), "golden", "solver_call_traces.json")) as f:
        want = json.load(f)
    got = _call_traces(cube, monkeypatch)
    assert sorted(got) == sorted(want)
    for case in want:
        assert got[case] == want[case], case


# ---------------------------------------------------------------------------------------------------------------------
# The fp64 refinement's pure phases (diffsound_amd/lobpcg/refine.py) and the generalised Ritz step they share with the polish.
def test_active_columns_keep_the_guards_and_pad_to_a_multiple_of_4_with_the_worst_of_the_rest():
    from diffsound_amd.lobpcg.refine import active_columns

    k, tol = 4, 1e-10
    hi, lo = 1e-9, 1e-12  # misses / passes 0.3 * tol
    # nothing wanted is active: the four guard columns are, whatever their own backward errors
    rel = torch.tensor([lo, lo, lo, lo, lo, hi, lo, lo], dtype=torch.float64)
    assert active_columns(rel.clone(), k, tol).tolist() == [4, 5, 6, 7]
    # a count that is already a multiple of 4 is left alone: all eight
    assert active_columns(torch.full((8,), hi, dtype=torch.float64), k, tol).tolist() == list(range(8))
    # one wanted column + four guards = 5: padded to 8 with the three largest of the inactive, sorted
    rel = torch.tensor([3e-12, hi, 1e-12, 2e-12, lo, lo, lo, lo], dtype=torch.float64)
    assert active_columns(rel.clone(), k, tol).tolist() == list(range(8))
    # (at b = 8 the three largest are all that is left.)  A case where the padding has to choose: k = 8 of b = 12, columns 1 and 5
    # active + 4 guards = 6 -> 8 with the two worst of the six others, 3 (9e-12) and 6 (8e-12)
    rel = torch.tensor([5e-12, hi, 1e-12, 9e-12, 2e-12, hi, 8e-12, 3e-12, lo, lo, lo, lo], dtype=torch.float64)
    assert active_columns(rel.clone(), 8, tol).tolist() == [1, 3, 5, 6, 8, 9, 10, 11]


def _spd_pencil(m, g):
    """(GA, GB, E): GB SPD and well conditioned, GA with the generalised eigenvalues E = 1 ... m exactly separated by 1."""
    A = torch.randn((m, m), generator=g, dtype=torch.float64)
    GB = A @ A.T / m + torch.eye(m, dtype=torch.float64)
    L = torch.linalg.cholesky(GB)
    Q = torch.linalg.qr(torch.randn((m, m), generator=g, dtype=torch.float64)).Q
    E = torch.arange(1, m + 1, dtype=torch.float64)
    H = L @ Q
    GA = H @ torch.diag(E) @ H.T
    return 0.5 * (GA + GA.T), GB, E


def test_ritz_pencil_with_p_equals_scipy():
    """An SPD pencil on S = [Y (6) | X (8) | P (4) | W (4)] with eigenvalues 1 ... 22: rounding reaches the result as
    eps x cond(GB) x |E| / gap, a few 1e-14 here, so 1e-12 holds for values and (sign-aligned) vectors alike."""
    import scipy.linalg as sla

    from diffsound_amd.lobpcg.refine import ritz_pencil

    GA, GB, _ = _spd_pencil(22, torch.Generator().manual_seed(0))
    E, Z = ritz_pencil(GA, GB, [0, 6, 14, 18, 22], True)
    Er, Zr = sla.eigh(GA.numpy(), GB.numpy())
    assert np.abs(E.numpy() - Er).max() < 1e-12 * np.abs(Er).max()
    Zr = Zr * np.sign((Zr * Z.numpy()).sum(0))[None, :]
    assert np.abs(Z.numpy() - Zr).max() < 1e-12


def test_ritz_pencil_repeats_without_p_when_the_gram_matrix_is_singular():
    """P duplicates W's columns: S^T M S = R^T R with R = the 18 x 18 Cholesky factor of [Y X W]'s Gram matrix and W's columns
    once more.  R has small integer entries, so the factorisation runs in exact arithmetic and meets pivots that are exactly 0
    at W: LinAlgError, whatever the LAPACK.  The fallback's eigenvalues are those of the pencil without P (1e-12) and its
    coefficients have zero rows at P; without a P to drop the error stands."""
    import scipy.linalg as sla

    from diffsound_amd.lobpcg.refine import ritz_pencil

    g = torch.Generator().manual_seed(1)
    R0 = torch.triu(torch.randint(-1, 2, (18, 18), generator=g).double(), 1) + 4.0 * torch.eye(18, dtype=torch.float64)
    cols = list(range(14)) + [14, 15, 16, 17] + [14, 15, 16, 17]  # [Y X | P = W | W]
    R = R0[:, cols]
    GB = R.T @ R
    A0 = _spd_pencil(18, g)[0]
    GA = A0[cols][:, cols]
    offs = [0, 6, 14, 18, 22]
    with pytest.raises(torch.linalg.LinAlgError):
        torch.linalg.cholesky(GB)
    E, Z = ritz_pencil(GA, GB, offs, True)
    keep = list(range(14)) + list(range(18, 22))
    Er = sla.eigh(GA[keep][:, keep].numpy(), GB[keep][:, keep].numpy(), eigvals_only=True)
    assert E.shape == (18,) and Z.shape == (22, 18)
    assert np.abs(E.numpy() - Er).max() < 1e-12 * np.abs(Er).max()
    assert torch.equal(Z[14:18], torch.zeros((4, 18), dtype=torch.float64))
    assert float((Z.T @ GB @ Z - torch.eye(18, dtype=torch.float64)).abs().max()) < 1e-12
    # no P: offs names [Y | X | W] with the SAME singular matrix (W's last columns duplicated inside it)
    with pytest.raises(torch.linalg.LinAlgError):
        ritz_pencil(GA, GB, [0, 6, 18, 22], False)


def test_gen_eigh_is_the_polish_algebra_bit_for_bit():
    """``dense._gen_eigh`` against the lines ModalSolver._polish carried inline until the refinement moved to refine.py."""
    from diffsound_amd.lobpcg.dense import _gen_eigh, _sym

    GA_, GB_, _ = _spd_pencil(24, torch.Generator().manual_seed(2))
    GA_, GB_ = _sym(GA_), _sym(GB_)  # (as _polish hands them over)
    L = torch.linalg.cholesky(GB_)
    Li = torch.linalg.solve_triangular(L, torch.eye(L.shape[0], dtype=L.dtype), upper=False)
    E_, Zt = torch.linalg.eigh(_sym(Li @ GA_ @ Li.transpose(0, 1)))
    C_ = (Li.transpose(0, 1) @ Zt).contiguous()
    E, C = _gen_eigh(GA_, GB_)
    assert torch.equal(E, E_) and torch.equal(C, C_)
    assert float((C.T @ GB_ @ C - torch.eye(24, dtype=torch.float64)).abs().max()) < 1e-12
