"""The fp64 refinement of the modal eigensolver (``SolverConfig.refine_tol``, ``ModalSolver.refine64``): LOBPCG steps on fp64
vectors, continued from the converged fp32 block.

One step = K W, M W for the new block (fp64 SpMM), one Rayleigh-Ritz on S = [Y | X | P | W] through the generalised
(3b + 6)-dimensional pencil (S^T K S, S^T M S) - the rigid modes come out as its six ~zero eigenvalues and are dropped - and X, P
and their products with K and M for the next step by linearity.
RAYLEIGH-RITZ BY RECURRENCE, as in the fp32 iteration: only the NEW columns meet the vectors - the Gram blocks S^T K W and
S^T M W (ONE pass over the rows of S, K W and M W per step: ds_gram64_blocks) - while the blocks among Y, X and P follow from the
last step's eigenvector matrix by (3b + 6)-dimensional algebra; every ``refine_refresh``-th step recomputes all blocks from the
vectors.  The n x b updates are ``ops.mix64`` (ds_mix64, fp64 MFMA) over the LIST of blocks of S: one pass per result, no
temporaries of the size of a block.

``_Refinement.steps`` names a step's phases in order; ``active_columns``, ``ritz_pencil`` and ``update_coefficients`` are pure."""
import torch

from .config import ModalResult
from .dense import _gen_eigh, _small, _sym


def active_columns(rel, k, refine_tol):
    """Soft locking: only the pairs that still miss the tolerance (with a margin) and the guard columns (k and up) get a new
    search direction; the others stay in X and take part in every Rayleigh-Ritz step, nothing else.  Sorted indices, padded to
    a multiple of 4 (the preconditioner's kernels take such blocks) with the worst of the remaining columns."""
    act = rel >= 0.3 * refine_tol
    act[k:] = True
    idx = torch.nonzero(act).reshape(-1)
    if idx.numel() % 4:
        rest = torch.nonzero(~act).reshape(-1)
        pad = rest[torch.argsort(rel[rest], descending=True)[:4 - idx.numel() % 4]]
        idx = torch.sort(torch.cat([idx, pad])).values
    return idx


def ritz_pencil(GA, GB, offs, has_p):
    """(E, Z) of the pencil on S = [Y | X | P | W] (host, fp64; ``offs``: the column offsets of its blocks, the total last).
    Should the Gram matrix of S be numerically singular (P and W nearly dependent close to convergence), the step is repeated
    without P - Z then has zero rows there and as many columns fewer; without a P to drop, the LinAlgError stands."""
    try:
        return _gen_eigh(GA, GB)
    except torch.linalg.LinAlgError:
        if not has_p:
            raise
    keep = torch.cat([torch.arange(0, offs[-3]), torch.arange(offs[-2], offs[-1])])
    E, Zk = _gen_eigh(GA[keep][:, keep].contiguous(), GB[keep][:, keep].contiguous())
    Z = torch.zeros((offs[-1], Zk.shape[1]), dtype=GA.dtype)
    Z[keep] = Zk
    return E, Z


def update_coefficients(E, Z, GA, GB, wn, idx, ny, b):
    """From the Ritz pairs of the pencil (W's rows and columns scaled by ``wn``): (lam, Zu, Tu, G0A, G0B) - the new Ritz values,
    the coefficients in S, with the W held in memory (not scaled), of the new X and of the new P on the columns ``idx``, and the
    Gram blocks among [Y | X_new | P_new] for the next step."""
    m, m0 = Z.shape[0], Z.shape[0] - wn.shape[0]
    Zs = Z[:, ny:ny + b].contiguous()  # the six lowest pairs are the rigid modes
    lam = E[ny:ny + b].contiguous()
    # update directions: everything of the new X that is not the old X (whose rows of S start at ny).  Their scale (unit M-norm)
    # comes from the small algebra (Pn = S Zr), so the coefficients of the scaled directions in S are known before any n-sized
    # work, and every result is ONE pass over the blocks of S
    Zr = Zs.clone()
    Zr[ny:ny + b] = 0.0
    pn2 = ((Zr.transpose(0, 1) @ GB) * Zr.transpose(0, 1)).sum(1)[idx].clamp(min=1e-300)
    Tp = (Zr[:, idx] * torch.rsqrt(pn2)[None, :]).contiguous()
    Zu, Tu = Zs.clone(), Tp.clone()
    Zu[m0:] *= wn[:, None]
    Tu[m0:] *= wn[:, None]
    # T^T G T with T the coefficients of [Y | X_new | P_new] in S
    T = torch.zeros((m, ny + b + idx.numel()), dtype=Z.dtype, device=Z.device)
    if ny:
        T[:ny, :ny] = torch.eye(ny, dtype=Z.dtype, device=Z.device)
    T[:, ny:ny + b] = Zs
    T[:, ny + b:] = Tp
    return lam, Zu, Tu, _sym(T.transpose(0, 1) @ GA @ T), _sym(T.transpose(0, 1) @ GB @ T)


class _Refinement:
    """The n-sized state of one refinement: the triples (block, K block, M block) of Y, X and P, and the buffer pool."""

    def __init__(self, solver, k, A_norm, B_norm):
        self.ops, self.cfg, self.precond_apply = solver.ops, solver.cfg, solver.precond_apply
        self.k, self.A_norm, self.B_norm = k, A_norm, B_norm
        self.fused = hasattr(self.ops, "residual64")  # (the HIP operators: norms in one pass, no fp64 residual block)
        self.pool = {}
        self.Y = self.X = self.P = None

    def buf(self, name, cols, dtype=torch.float64):
        # Every n-sized block of a step lives in a POOL of (n x b) buffers allocated once and used through column views (round 5):
        # the number of active columns changes from step to step, and blocks of ever new sizes - 2 to 4.5 GB each at configs[4] -
        # made the caching allocator release and re-request device memory in the middle of the steps (0.3 s of run-to-run spread)
        t = self.pool.get(name)
        if t is None:
            t = self.pool[name] = torch.empty((self.n, self.b), dtype=dtype, device=self.ops.device)
        return t[:, :cols]

    def start(self, X):
        """K X, M X (and K Y, M Y) of the fp32 block, promoted, and the Rayleigh-Ritz on that block alone: the pairs whose residual
        is tested first, and an X that is K-diagonal / M-orthonormal - which every later step's X is by construction."""
        ops = self.ops
        self.n, self.b = X.shape
        Y = ops.rigid64()
        KX, MX = (torch.empty((self.n, self.b), dtype=torch.float64, device=ops.device) for _ in range(2))
        ops.apply_K64(X, KX)
        ops.apply_M64(X, MX)
        if Y is not None:
            MY, KY = torch.empty_like(Y), torch.empty_like(Y)
            ops.apply_M64(Y, MY)
            ops.apply_K64(Y, KY)  # ~ eps ||K|| (the rigid modes are null vectors of K); kept, not assumed zero
            self.Y = (Y[:, :6], KY[:, :6], MY[:, :6])
        lam, C = _small(_gen_eigh, ops.device, ops.gram(X, KX), ops.gram(X, MX))
        self.X = (ops.mix64([X], C), ops.mix64([KX], C), ops.mix64([MX], C))
        return lam

    def backward_errors(self, lam):
        """(rel, rn, R): the backward errors and residual norms of X's columns; R = K X - M X diag(lam), or None on the fused route."""
        X, KX, MX = self.X
        if self.fused:
            rn2, xn2 = self.ops.residual64(KX, MX, X, lam)
            rn, xn, R = torch.sqrt(rn2), torch.sqrt(xn2), None
        else:
            R = torch.addcmul(KX, MX, lam[None, :], value=-1.0)
            rn, xn = torch.linalg.vector_norm(R, dim=0), torch.linalg.vector_norm(X, dim=0)
        return rn / (xn * (self.A_norm + lam.abs() * self.B_norm)), rn, R

    def search_block(self, lam, rn, R, idx):
        """(W, K W, M W) for the columns ``idx``: W = B R in fp32 (columns scaled to unit norm: the preconditioner is linear),
        promoted to fp64."""
        ops, buf, nact = self.ops, self.buf, int(idx.numel())
        R32 = buf("R32", nact, torch.float32)
        if self.fused:
            ops.residual64_scaled(self.X[1], self.X[2], lam, 1.0 / rn.clamp(min=1e-300), idx, out=R32)
        else:
            R32.copy_(R[:, idx] / rn[idx].clamp(min=1e-300)[None, :])
        W32 = buf("W32", nact, torch.float32)
        self.precond_apply(R32, W32)
        for _ in range(max(0, int(self.cfg.refine_sweeps) - 1)):
            # one more sweep of the preconditioned Richardson iteration: W <- W + B (R - K W), all fp32.  A step of
            # the fp64 phase is dominated by its dense n x b products, not by the preconditioner: a stronger
            # correction per step buys fewer steps
            T32, D32 = buf("T32", nact, torch.float32), buf("D32", nact, torch.float32)
            ops.apply_K(W32, T32)
            torch.sub(R32, T32, out=T32)
            self.precond_apply(T32, D32)
            W32 += D32
        W, KW, MW = buf("W", nact), buf("KW", nact), buf("MW", nact)
        W.copy_(W32)
        ops.apply_M64(W, MW)
        ops.apply_K64(W, KW)
        return W, KW, MW

    def pencil(self, S, m0, G0):
        """(S^T K S, S^T M S, wn) on S = [Y | X | P | W].  G0 None: all pairs of blocks from the vectors, one pass over the rows each;
        else only the new columns meet the vectors - S^T [K W | M W] in one pass - and G0 holds the blocks among [Y | X | P]."""
        blocks, na = [blk[0] for blk in S], S[-1][0].shape[1]
        if G0 is None:
            GA, GB = (self.ops.gram_blocks(blocks, [blk[i] for blk in S], symmetric=True) for i in (1, 2))
            strips = GA[:, m0:], GB[:, m0:]
        else:
            Gw = self.ops.gram_blocks(blocks, list(S[-1][1:]))
            strips = Gw[:, :na], Gw[:, na:]
            GA, GB = (torch.zeros((m0 + na, m0 + na), dtype=Gw.dtype, device=Gw.device) for _ in range(2))
        # unit M-norm columns of W - a well scaled pencil - without touching the vectors: the scale wn comes off the diagonal of
        # W^T M W, goes into the small matrices here and into the coefficients of the update (update_coefficients)
        wn = torch.rsqrt(torch.diagonal(strips[1][m0:]).clamp(min=1e-300))
        for i, (G, strip) in enumerate(zip((GA, GB), strips)):
            strip *= wn[None, :]
            strip[m0:] *= wn[:, None]
            if G0 is None:
                G[m0:, :m0] *= wn[:, None]
            else:
                G[:m0, :m0], G[:, m0:], G[m0:, :m0] = G0[i], strip, strip[:m0].transpose(0, 1)
        return _sym(GA), _sym(GB), wn

    def update_blocks(self, S, offs, Zu, Tu, it):
        """X' = S Zu and P' = S Tu, and their products with K and M by linearity: ONE pass over the blocks of S per result
        (ds_mix64: each block read once, the result written once, no n x b temporaries)."""
        xi = 0 if self.Y is None else 1  # position of X in S: its rows of Tu are zero, and P' skips the block
        news = []
        for which in range(3):  # the vectors, their K-products, their M-products
            parts = [blk[which] for blk in S]
            # (two sets of pool buffers, alternating: a step reads the set the previous one wrote)
            Xn = self.ops.mix64(parts, Zu, out=self.buf(f"X{which}_{it & 1}", self.b))
            Pd = self.ops.mix64([(blk, offs[i]) for i, blk in enumerate(parts) if i != xi], Tu,
                                out=self.buf(f"P{which}_{it & 1}", Tu.shape[1]))
            news.append((Xn, Pd))
        self.X, self.P = tuple(n_[0] for n_ in news), tuple(n_[1] for n_ in news)

    def steps(self, lam):
        """The steps, until the wanted pairs pass ``refine_tol`` or ``refine_maxit``: (lam, rel, history of the worst backward error)."""
        cfg, k, ny = self.cfg, self.k, 0 if self.Y is None else 6
        G0 = None  # Gram blocks among [Y | X | P] of the current basis (fp64, m0 x m0), by recurrence
        refresh = max(1, int(cfg.refine_refresh))
        since = refresh  # the first step forms everything from the vectors
        hist = []
        for it in range(cfg.refine_maxit + 1):
            rel, rn, R = self.backward_errors(lam)
            hist.append(float(rel[:k].max()))
            if hist[-1] < cfg.refine_tol or it == cfg.refine_maxit:
                break
            idx = active_columns(rel, k, cfg.refine_tol)
            # S = [Y | X | P | W]  (P: the previous step's update directions - the locally optimal 3-term recurrence; without
            # it the pairs next to the guard vectors crawl)
            S = [blk for blk in (self.Y, self.X, self.P) if blk is not None] + [self.search_block(lam, rn, R, idx)]
            del R
            offs = [sum(blk[0].shape[1] for blk in S[:i]) for i in range(len(S) + 1)]
            m0, has_p = offs[-2], self.P is not None
            full = since >= refresh or G0 is None or G0[0].shape[0] != m0
            GA, GB, wn = self.pencil(S, m0, None if full else G0)
            since = 1 if full else since + 1
            E, Z = _small(lambda GA_, GB_: ritz_pencil(GA_, GB_, offs, has_p), self.ops.device, GA, GB)
            lam, Zu, Tu, *G0 = update_coefficients(E, Z, GA, GB, wn, idx, ny, self.b)
            self.update_blocks(S, offs, Zu, Tu, it)
        return lam, rel, hist

    def read_out(self, res, lam, rel, hist):
        """The wanted pairs with their quadratic forms u^T K_lambda u, u^T K_mu u, u^T M u, as a ModalResult that continues ``res``."""
        ops, k, X = self.ops, self.k, self.X[0]
        U = X[:, :k].contiguous()
        kparts = ops.apply_K64(U, torch.empty_like(U), terms=True)
        MU = torch.empty_like(U)
        ops.apply_M64(U, MU)
        a = (U * kparts[0]).sum(0)
        bq = (U * kparts[1]).sum(0) if len(kparts) > 1 else None
        out = ModalResult(lam[:k].clone(), U, a, bq, (U * MU).sum(0), iterations=res.iterations, rerr=rel[:k].clone(),
                          history=res.history, block_vectors=X)
        out.coarse_iterations = res.coarse_iterations
        out.refine_iterations = len(hist) - 1
        out.refine_history = hist
        return out


def refine64(solver, res, k, A_norm, B_norm):
    """``ModalSolver.refine64``: the refinement of ``res`` (the polish's, with its ``block_vectors``) to ``cfg.refine_tol``."""
    run = _Refinement(solver, k, A_norm, B_norm)
    combined_k64 = getattr(solver.ops, "combined_k64", None)
    if combined_k64 is not None:
        combined_k64(True)  # one fp64 block array for K during the steps
    try:
        lam, rel, hist = run.steps(run.start(res.block_vectors.double()))
    finally:  # (a step that raises must not leave the combined array cached for a later material)
        if combined_k64 is not None:
            combined_k64(False)
    return run.read_out(res, lam, rel, hist)
