"""The eigensolver's preconditioners: a Chebyshev polynomial in (block-Jacobi)^-1 K and the two-level V-cycle built on it
(lobpcg/modal_solver.py)."""
import torch


def _stats(ops, name):
    """The two diagnostic counters ``name`` of an operator object (created on first use).  They live on the OPERATORS - one
    object per hypothesis lane, touched by that lane's thread only - not on a class: round 5 kept them as class attributes that
    eight lane threads incremented without a lock and that two pipelines in one process would have shared."""
    st = getattr(ops, name, None)
    if st is None:
        st = [0, 0]
        try:
            setattr(ops, name, st)
        except AttributeError:
            pass
    return st


class ChebyshevBlockJacobi:
    """W = p(T K) T R with T = inverse 3x3 diagonal blocks of K and p the degree-(d-1) Chebyshev
    polynomial that approximates 1/x on [lmax/ratio, lmax] (Saad, Iterative Methods, Alg. 12.1).
    Costs d-1 block-SpMMs with K per application; symmetric and fixed, as LOBPCG requires."""

    def __init__(self, ops, degree, ratio, power_iters=30, seed=0, safety=1.2, cap=0.0, warm_iters=None, warm_spread=None):
        """``warm_iters`` / ``warm_spread``: SolverConfig.warm_power_iters / warm_power_spread of the solve this preconditioner
        belongs to (None: the class defaults) - per solver, nothing process-wide (round 6: bench.py used to write the class
        attributes, which two pipelines in one process would have fought over)."""
        self.ops = ops
        self.degree = max(1, int(degree))
        # T of this polynomial: the operator object's group-block Jacobi (HipModalOps.group_jacobi, the corner-node level) or its
        # 3 x 3 node blocks.  The native bf16 cycle reads it off the level descriptor; here: the power iteration and the Python path.
        self.group = int(getattr(ops, "group_jacobi", 0) or 0)
        warm_iters = ChebyshevBlockJacobi.warm_power_iters if warm_iters is None else int(warm_iters)
        warm_spread = ChebyshevBlockJacobi.warm_spread if warm_spread is None else float(warm_spread)
        if power_iters <= 0:  # no estimate: the rigorous bound lambda_max(T K) <= nodes per element is the interval's end
            if cap <= 0.0:
                raise ValueError("ChebyshevBlockJacobi: power_iters = 0 needs a rigorous bound (lmax_cap)")
            self.lmax = float(cap)
            self.lmin = self.lmax / float(ratio)
            self._D = self._AD = None
            return
        n, dev, dt = ops.n, ops.device, ops.dtype
        # The dominant vectors of T K barely move when the material changes, so an ops object that already went
        # through a power iteration hands its block over and a few steps re-converge the bound (the
        # eigensolve itself still starts cold; only this spectral bound of the preconditioner is warm).
        x = getattr(ops, "_power_block", None)
        # (warm only on the geometry the block was iterated on: new coordinates take the full count again)
        pkey = getattr(ops, "norm_probe_key", None)
        pkey = None if pkey is None else pkey()
        warm = x is not None and x.shape == (n, 8) and x.dtype == dt and getattr(ops, "_power_block_key", None) == pkey
        if not warm:
            g = torch.Generator(device=dev).manual_seed(seed + 17)  # device-side RNG: no 100 MB host round trip
            x = torch.randn((n, 8), generator=g, dtype=torch.float32, device=dev).to(dt)
        y = torch.empty_like(x)
        z = torch.empty_like(x)
        lm = prev = None
        for i in range(power_iters):  # largest eigenvalue of T K by block power iteration
            ops.apply_K(x, y)
            if self.group:
                x = ops.group_T(y)
            else:
                ops.cheb_init(y, z, x, 1.0)  # x = T y
            nrm = torch.linalg.vector_norm(x.double(), dim=0)
            lm = nrm.max()
            x = (x / nrm.to(dt)[None, :]).contiguous()
            # A warm block stops as soon as the estimate has stopped moving: SUCCESSIVE estimates (the growth factor of step i
            # against step i - 1) agree to ``warm_spread``, after at least two steps and at least ``warm_iters`` unless they
            # agree earlier.  Round 5 took the agreement AMONG the 8 columns after one step as the sign of convergence - but the
            # columns, never orthogonalised, have all collapsed onto the previous material's dominant vector, and vectors that are
            # equal agree under ANY operator: a jump nu 0.45 -> 0.12 left the one-step estimate at 0.878 of
            # lambda_max, 1.05 x under the safety factor.  The growth factor of a block that the new material has left behind
            # keeps rising from step to step; it is compared with itself.  (The host reads one number per step.)
            if warm and warm_spread > 0.0:
                if i == 0:
                    first = lm  # (not read yet: the first two estimates travel to the host together - one wait instead of two)
                    continue
                if i == 1:
                    prev, cur = torch.stack((first, lm)).tolist()
                else:
                    cur = float(lm)
                if abs(cur - prev) < warm_spread * cur:
                    lm = cur
                    break
                prev = cur
            elif warm and i + 1 >= max(1, warm_iters):
                break
        if warm:  # (diagnostic counters of THIS operator object, read by bench.py: estimates from a warm block, steps they took)
            st = _stats(ops, "warm_stats")
            st[0] += 1
            st[1] += i + 1
        try:
            ops._power_block, ops._power_block_key = x, pkey
        except AttributeError:
            pass
        # power iteration under-estimates; an under-estimated lmax makes the polynomial blow up on
        # the top of the spectrum (measured: 2% low -> no convergence), an over-estimate costs little
        self.lmax = safety * float(lm)
        if cap > 0.0:
            self.lmax = min(self.lmax, cap)
        self.lmin = self.lmax / float(ratio)
        self._D = None
        self._AD = None

    _CHUNK = 80  # columns per fused launch (the fused kernel takes <= 84)
    # power iterations when the ops hand over the block of an earlier estimate (another material on the same mesh):
    # lambda_max(T K) depends on the Poisson ratio only, and mildly (3.1 ... 3.6 over nu = 0.12 ... 0.38 on the
    # benchmark mesh), the dominant vectors hardly at all
    warm_power_iters = 3  # steps of a warm estimate when ``warm_spread`` is 0 (7, 4, 2 and 1 give the same outer iteration counts on the benchmark)
    warm_spread = 0.003   # a warm estimate stops when two successive estimates agree to this (at least two steps); 0: warm_power_iters steps

    def apply(self, R, W, from_guess=False):
        """W <- p(T K) T R (R may be destroyed).  ``from_guess``: W holds an initial guess W_0 and the same
        number of terms of the Chebyshev ITERATION for K W = R is run from it (W <- W_0 + p(T K) T (R - K W_0));
        this is the post-smoother of the two-level cycle and needs the fused-term op."""
        ops = self.ops
        if self.group:
            return self._apply_group(R, W, from_guess)
        if hasattr(ops, "cheb_spmm") and (self.degree > 1 or from_guess):
            for c0 in range(0, R.shape[1], self._CHUNK):  # columns are independent: wide blocks go in chunks
                c1 = min(R.shape[1], c0 + self._CHUNK)
                self._fused(R[:, c0:c1], W[:, c0:c1], from_guess)
            return
        if from_guess:
            raise RuntimeError("Chebyshev iteration from an initial guess needs ops.cheb_spmm")
        theta = 0.5 * (self.lmax + self.lmin)
        delta = 0.5 * (self.lmax - self.lmin)
        D, AD = self._buffers(R)
        ops.cheb_init(R, D, W, 1.0 / theta)  # D = T R / theta ; W = D
        sigma1 = theta / delta
        rho = 1.0 / sigma1
        for _ in range(self.degree - 1):
            ops.apply_K(D, AD)
            rho_new = 1.0 / (2.0 * sigma1 - rho)
            ops.cheb_step(AD, R, D, W, rho_new * rho, 2.0 * rho_new / delta)  # R-=AD; D=c1 D+c2 T R; W+=D
            rho = rho_new

    def _apply_group(self, R, W, from_guess):
        """The polynomial in T_g K in torch on the level's fp32 product - the Python path of the group-block Jacobi (a tracker
        callback, fp32 storage, the tests' comparisons); the product path is the native bf16 cycle."""
        if from_guess:
            raise RuntimeError("the group-block Jacobi serves the polynomial from a zero guess (the corner-node level)")
        ops = self.ops
        theta, delta = 0.5 * (self.lmax + self.lmin), 0.5 * (self.lmax - self.lmin)
        z = ops.group_T(R.contiguous())
        x = z / theta
        d = x.clone()
        sigma1 = theta / delta
        rho = 1.0 / sigma1
        kx = torch.empty_like(x)
        for _ in range(self.degree - 1):
            ops.apply_K(x, kx)
            rho_new = 1.0 / (2.0 * sigma1 - rho)
            d = (rho_new * rho) * d + (2.0 * rho_new / delta) * (z - ops.group_T(kx))
            x = x + d
            rho = rho_new
        W.copy_(x)

    def _buffers(self, R):
        if self._D is None or self._D.shape != R.shape:
            self._D = torch.empty(R.shape, dtype=R.dtype, device=R.device)
            self._AD = torch.empty(R.shape, dtype=R.dtype, device=R.device)
        return self._D, self._AD

    def _fused(self, R, W, from_guess):
        # three-term form W_{k+1} = W_k + c1 (W_k - W_{k-1}) + c2 T (R0 - K W_k): one fused launch per term,
        # ping-ponging between W and a scratch block; R is only read
        ops = self.ops
        theta = 0.5 * (self.lmax + self.lmin)
        delta = 0.5 * (self.lmax - self.lmin)
        D, AD = self._buffers(R)
        sigma1 = theta / delta
        rho = 1.0 / sigma1
        if from_guess:
            terms = self.degree
            cur, oth = W, D
        else:
            terms = self.degree - 1
            cur, oth = (W, D) if terms % 2 == 0 else (D, W)  # so that the last term lands in W
            ops.cheb_init(R, AD, cur, 1.0 / theta)  # W_1 = T R0 / theta  (W_0 = 0)
        for k in range(terms):
            if from_guess and k == 0:
                ops.cheb_spmm(cur, oth, R, 0.0, 1.0 / theta, first=True)  # W_1 = W_0 + T (R0 - K W_0) / theta
            else:
                rho_new = 1.0 / (2.0 * sigma1 - rho)
                ops.cheb_spmm(cur, oth, R, rho_new * rho, 2.0 * rho_new / delta, first=(k == 0))
                rho = rho_new
            cur, oth = oth, cur
        if cur is not W:
            W.copy_(cur)


class TwoLevelChebyshev:
    """Symmetric two-level V-cycle for ord-2 meshes:
         W1 = S R ;  W2 = W1 + P C P^T (R - K W1) ;  W = W2 + S (R - K W2)
    S: Chebyshev block-Jacobi smoother on the fine level (damps [lmax/smooth_ratio, lmax]); P: embedding of the
    corner-node P1 space; C: Chebyshev block-Jacobi polynomial for the P1 operator P^T K P (an ord-1 assembly of
    the corner sub-mesh, ~14x fewer non-zeros).  The smooth modes that the one-level polynomial needs a high
    degree for are handled on the cheap level: ~6 fine SpMMs per application instead of ~48 at the same
    outer iteration count.  Fixed, symmetric positive definite, as LOBPCG requires."""

    use_native = True  # run the cycle through ops.twolevel_apply (one native call) when the ops offer it

    def __init__(self, ops, cfg):
        self.ops = ops
        self.storage = cfg.precond_storage
        self._buf16 = None
        args = (cfg.power_iters, cfg.seed, cfg.lmax_safety)
        warm = dict(warm_iters=cfg.warm_power_iters, warm_spread=cfg.warm_power_spread)
        self.smooth = ChebyshevBlockJacobi(ops, cfg.smooth_degree, cfg.smooth_ratio, *args, cap=cfg.lmax_cap, **warm)
        grp = bool(getattr(ops.coarse, "group_jacobi", 0))
        self.coarse = ChebyshevBlockJacobi(ops.coarse, cfg.group_degree if grp else cfg.coarse_degree,
                                           cfg.group_ratio if grp else cfg.coarse_ratio, *args,
                                           cap=min(cfg.lmax_cap, 4.0) if cfg.lmax_cap > 0 else 0.0, **warm)
        self.lmax = self.smooth.lmax
        self._buf = None

    def apply(self, R, W):
        ops = self.ops
        nc = ops.coarse.n
        ch = ChebyshevBlockJacobi._CHUNK
        for c0 in range(0, R.shape[1], ch):
            Rs, Ws = R[:, c0:c0 + ch], W[:, c0:c0 + ch]
            w = Rs.shape[1]
            if self._buf is None or self._buf[0].shape[1] != w:
                mk = lambda rows: torch.empty((rows, w), dtype=R.dtype, device=R.device)
                self._buf = (mk(R.shape[0]), mk(nc), mk(nc), mk(R.shape[0]))
            Rr, Rc, Ec, Wc = self._buf
            native = getattr(ops, "twolevel_apply", None)
            form = getattr(self, "cycle_form", "symmetric")
            if form != "symmetric":  # (experiment, Python path only: tools/experiments/cycle_forms.py)
                if form == "post":        # W = C' R, then post-smoothing from that guess
                    ops.restrict(Rs, Rc)
                    self.coarse.apply(Rc, Ec)
                    Ws.zero_()
                    ops.prolong_add(Ec, Ws)
                    self.smooth.apply(Rs, Ws, from_guess=True)
                elif form == "pre":       # pre-smoothing, then the corner-level correction of its residual
                    Rr.copy_(Rs)
                    self.smooth.apply(Rr, Ws)
                    ops.spmm_residual(Ws, Rs, Rr)
                    ops.restrict(Rr, Rc)
                    self.coarse.apply(Rc, Ec)
                    ops.prolong_add(Ec, Ws)
                elif form == "additive":  # W = S R + P C P^T R
                    ops.restrict(Rs, Rc)
                    self.coarse.apply(Rc, Ec)
                    Rr.copy_(Rs)
                    self.smooth.apply(Rr, Ws)
                    ops.prolong_add(Ec, Ws)
                else:
                    raise ValueError(form)
                continue
            if native is not None and self.use_native and self.storage == "bf16" and R.is_cuda:
                if self._buf16 is None or self._buf16[0].shape[2] != w:
                    mk = lambda cnt, rows: torch.empty((cnt, rows, w), dtype=torch.bfloat16, device=R.device)
                    self._buf16 = (mk(5, R.shape[0]), mk(4, nc))
                f16, c16 = self._buf16
                if native((self.smooth.degree, self.smooth.lmax, self.smooth.lmin),
                          (self.coarse.degree, self.coarse.lmax, self.coarse.lmin), Rs, Ws, f16[1], f16[2], f16[3], c16[0],
                          c16[1], c16[2], c16[3], f16[0], R16=f16[4]):
                    continue
            if native is not None and self.use_native and not self.coarse.group:  # (the fp32 cycle knows the node blocks only)
                D, AD = self.smooth._buffers(Rs)
                Dc, ADc = self.coarse._buffers(Rc)
                if native((self.smooth.degree, self.smooth.lmax, self.smooth.lmin),
                          (self.coarse.degree, self.coarse.lmax, self.coarse.lmin), Rs, Ws, D, AD, Rr, Rc, Ec, Dc, ADc,
                          Wc):
                    continue
            self.smooth.apply(Rs, Ws)
            ops.spmm_residual(Ws, Rs, Rr)
            ops.restrict(Rr, Rc)
            self.coarse.apply(Rc, Ec)
            ops.prolong_add(Ec, Ws)
            self.smooth.apply(Rs, Ws, from_guess=True)

