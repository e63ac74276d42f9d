"""The small (<= 3b x 3b) dense algebra of the modal eigensolver - fp64, on the host - and the guard that keeps its LAPACK calls
on one thread (lobpcg/modal_solver.py).  csrc/host_dense.cpp is its twin for the native loop: the functions there carry the same
names without the underscore, and tests/test_cabi_cpu.py checks one against the other.  ``_gen_eigh`` - the generalised Ritz step
of the fp64 polish and of the fp64 refinement (lobpcg/refine.py) - is the algebra ds_host_polish says there for the native
polish; ``_basic_transform`` / ``_basic_ritz``, the Rayleigh-Ritz transform of ``ModalSolver.solve_basic``, have no twin: that
iteration runs in the interpreter only."""
import os
import threading

import torch


def storage_eps(dtype):
    """Unit roundoff of the dtype the iterates are stored in (what a sweep's amplification ``amp`` multiplies)."""
    return 6e-8 if dtype == torch.float32 else 1.1e-16


def _sym(G):
    return 0.5 * (G + G.transpose(0, 1))


def _gen_eigh(GA, GB):
    """(E, C) of the pencil (GA, GB), ascending, with C^T GB C = I: Cholesky factor of GB, its triangular inverse, ``eigh`` of the
    transformed GA, back-transform.  Both are symmetrised first; a GB that is not positive definite raises LinAlgError."""
    L = torch.linalg.cholesky(_sym(GB))
    Li = torch.linalg.solve_triangular(L, torch.eye(L.shape[0], dtype=L.dtype), upper=False)
    E, Zt = torch.linalg.eigh(_sym(Li @ _sym(GA) @ Li.transpose(0, 1)))
    return E, (Li.transpose(0, 1) @ Zt).contiguous()


def _basic_transform(GB, eps):
    """Ri = D^-1/2 chol(D^-1/2 S^T B S D^-1/2)^-T of the reference's 'basic' method (``_get_rayleigh_ritz_transform``,
    _lobpcg.py:479-525): None when the scaled Gram matrix has no Cholesky factor - or one so ill-conditioned that
    S Ri would come out of the fp32 update visibly non-orthonormal (eps x cond(S^T B S) >= 1e-3: the vectors are stored with unit
    roundoff ``eps``; the reference, which has no such test, then iterates on a basis that is no longer one).  A transform of its
    own: ``_gen_eigh`` neither scales nor gates."""
    GB = _sym(GB)
    d = torch.rsqrt(torch.clamp(GB.diagonal(), min=1e-300))
    L, info = torch.linalg.cholesky_ex(GB * d[:, None] * d[None, :])
    if int(info) != 0 or not bool(torch.isfinite(L).all()):
        return None
    if eps / max(float(L.diagonal().min()), 1e-300) ** 2 >= 1e-3:
        return None
    Li = torch.linalg.solve_triangular(L, torch.eye(L.shape[0], dtype=L.dtype), upper=False)
    return d[:, None] * Li.transpose(0, 1)


def _basic_ritz(GA, GB, eps, keep=None):
    """(Ritz values, the first ``keep`` columns of Ri Z) of the 'basic' method's step, or None without a transform."""
    keep = GA.shape[0] if keep is None else keep
    Ri = _basic_transform(GB, eps)
    if Ri is None:
        return None
    E_, Z = torch.linalg.eigh(_sym(Ri.transpose(0, 1) @ _sym(GA) @ Ri))
    return E_, (Ri @ Z[:, :keep]).contiguous()


def _svqb_transform(G, tau=1e-12):
    """T such that (W T)^T M (W T) = I given G = W^T M W  (reference _get_svqb, _lobpcg.py:527-585,
    non-dropping branch: tiny eigenvalues are clamped, not removed)."""
    d = torch.rsqrt(torch.clamp(G.diagonal(), min=1e-300))
    E, Z = torch.linalg.eigh(_sym(G) * d[:, None] * d[None, :])
    E = torch.clamp(E, min=tau * E.abs().max())
    return (d[:, None] * Z) * torch.rsqrt(E)[None, :]


def _orthonormalizer_q(G):
    """(T, amp): T with (W T)^T M (W T) = I from G = W^T M W - Cholesky-QR on the diagonally scaled Gram matrix (one potrf + one
    small triangular solve), falling back to the clamped-eigenvalue transform of the reference's svqb when the factorisation
    breaks down (rank-deficient block); ``amp`` (python float) estimates by how much the storage rounding of W is amplified in the orthogonality of the result, amp = max(1 / min diag(chol) (a lower bound of the
    scaled block's condition), sqrt(removed / kept) per column).  An optional extra last row of G carries the
    squared M-norms of what the preceding projection removed from each column."""
    rem = None
    if G.shape[0] == G.shape[1] + 1:
        G, rem = G[:-1], G[-1]
    G = _sym(G)
    diag = torch.clamp(G.diagonal(), min=1e-300)
    d = torch.rsqrt(diag)
    L, info = torch.linalg.cholesky_ex(G * d[:, None] * d[None, :])
    if int(info) != 0 or not bool(torch.isfinite(L).all()):
        return _svqb_transform(G), float("inf")
    amp = 1.0 / max(float(L.diagonal().min()), 1e-300)
    if rem is not None:
        amp = max(amp, float(torch.sqrt(rem / diag).max()))
    Li = torch.linalg.solve_triangular(L, torch.eye(L.shape[0], dtype=L.dtype, device=L.device), upper=False)
    return d[:, None] * Li.transpose(0, 1), amp


def _project_in_coefficients(C, G0, cholesky_gate=False):
    """W projected against an M-orthonormal V and M-orthonormalised, in coefficients: from C = V^T M W and G0 = W^T M W
    (symmetric) the Gram matrix of the projected block is G0 - C^T C, and (T, C^T C, amp) is its ``_orthonormalizer_q`` transform
    - W_o = (W - V C) T - with what the projection removed counted into ``amp``.  None when the closed form has broken down:
    a column (numerically) inside span(V) leaves nothing of itself in G0 - C^T C but cancellation noise (the caller then takes
    its explicit route); ``cholesky_gate``: ... or when G0 - C^T C, unscaled, has no Cholesky factor."""
    CtC = C.transpose(0, 1) @ C
    Gp = G0 - CtC
    if bool((Gp.diagonal() <= 1e-9 * G0.diagonal().abs()).any()) or not bool(torch.isfinite(Gp).all()):
        return None
    if cholesky_gate and int(torch.linalg.cholesky_ex(Gp)[1]) != 0:
        return None
    T, amp = _orthonormalizer_q(torch.cat([Gp, CtC.diagonal()[None, :]], 0))
    return T, CtC, amp


def _orthonormal_columns(Tm):
    """Orthonormal basis (Euclidean, coefficient space) of the columns of the small dense Tm (r x c):
    scaled Cholesky-QR applied twice (one pass leaves an orthogonality error eps*cond^2, which would
    put a 1e-8 floor under the fp64 residuals), with a Householder-QR fallback."""
    Q = Tm
    for _ in range(2):
        G = Q.transpose(0, 1) @ Q
        d = torch.rsqrt(torch.clamp(G.diagonal(), min=1e-300))
        L, info = torch.linalg.cholesky_ex(_sym(G) * d[:, None] * d[None, :])
        if int(info) != 0 or not bool(torch.isfinite(L).all()):
            return torch.linalg.qr(Tm).Q
        Li = torch.linalg.solve_triangular(L, torch.eye(L.shape[0], dtype=L.dtype, device=L.device), upper=False)
        Q = Q @ (d[:, None] * Li.transpose(0, 1))
    return Q


def _thread_local_setters():
    """(mkl_set_num_threads_local, omp_set_num_threads, omp_get_max_threads) of the libraries torch's CPU kernels run on, or None.
    All three act on the CALLING THREAD only - unlike ``torch.set_num_threads``, which also stores a process-wide default and
    re-creates torch's pthreadpool with the new thread count on every call."""
    global _TLS_SETTERS
    if _TLS_SETTERS is False:
        _TLS_SETTERS = None
        try:
            import ctypes

            lib = ctypes.CDLL(os.path.join(os.path.dirname(torch.__file__), "lib", "libtorch_cpu.so"))
            # (the C interface: the lower-case mkl_set_num_threads_local is the Fortran one and takes a pointer)
            mkl, oset, oget = lib.MKL_Set_Num_Threads_Local, lib.omp_set_num_threads, lib.omp_get_max_threads
            mkl.restype, mkl.argtypes = ctypes.c_int, [ctypes.c_int]
            oset.restype, oset.argtypes = None, [ctypes.c_int]
            oget.restype, oget.argtypes = ctypes.c_int, []
            _TLS_SETTERS = (mkl, oset, oget)
        except (OSError, AttributeError):
            pass
    return _TLS_SETTERS


_TLS_SETTERS = False


class _one_thread:
    """LAPACK on <= 3b x 3b matrices is fastest single-threaded (measured on the MI355X host: 240 x 240
    fp64 eigh 2.5 ms with 1 thread, no faster with 2-8, 150 ms with the default 128 threads; rocSOLVER's
    launch-bound syevd takes 5.7 ms).  Every thread that enters lowers ITS OWN MKL / OpenMP thread count
    (``mkl_set_num_threads_local``, ``omp_set_num_threads``: per-thread settings) and restores its own previous values when it
    leaves; re-entrant; nothing process-wide is touched.
    History: until round 4 only the first thread to enter lowered a count - the reason two identical 8-lane runs could differ in
    the last bits of a gradient (tests/test_fullsize_gpu.py::test_c3_eight_lanes_are_bit_identical_from_run_to_run).  Round 4
    saved ONE value for all threads and restored it from the last thread to leave, which could leave 1 as the process-wide
    default - and, as a side effect, kept the hypothesis lanes' threads at one thread for good; the lanes now
    pin themselves (``one_blas_thread_for_this_thread`` from the lane pool's initializer), this guard only brackets the dense steps."""

    _tls = threading.local()

    def __enter__(self):
        st = _one_thread._tls
        depth = getattr(st, "depth", 0)
        if depth == 0:
            fns = _thread_local_setters()
            if fns is not None:
                mkl, oset, oget = fns
                torch.get_num_threads()  # (a thread's first torch call sizes its OpenMP team from MKL's count: before we lower it)
                st.saved = (mkl(1), oget())  # (MKL_Set_Num_Threads_Local returns the previous local value; 0 = unset)
                oset(1)
            else:  # another BLAS behind torch: its own (heavier) switch, and only when there is something to lower
                st.saved = torch.get_num_threads()
                if st.saved != 1:
                    torch.set_num_threads(1)
        st.depth = depth + 1

    def __exit__(self, *a):
        st = _one_thread._tls
        st.depth -= 1
        if st.depth == 0:
            fns = _thread_local_setters()
            if fns is not None:
                fns[0](st.saved[0])
                fns[1](st.saved[1])
            elif st.saved != 1:
                torch.set_num_threads(st.saved)


def one_blas_thread_for_this_thread():
    """For a private worker thread (a hypothesis lane): one MKL / OpenMP thread for its whole life, thread-local settings only.
    (It limits the thread's BLAS / OpenMP team, not the cores it may run on - which CPUs a rank's threads use is decided once per
    process by diffsound_amd.hostcpu.bind_rank_to_device_numa.  Until round 6 its name promised a core, which it never pinned.)
    A lane issues launches and solves <= 3b x 3b dense problems; left at the host's full thread count (256 hardware threads on
    the GPU box) any OpenMP region it enters would spin up a team of that size next to the other lanes' teams."""
    fns = _thread_local_setters()
    if fns is not None:
        torch.get_num_threads()  # (sizes the thread's team first, see _one_thread)
        fns[0](1)
        fns[1](1)
    else:
        torch.set_num_threads(1)



def _small(fn, dev, *mats):
    """Run the small dense step ``fn`` on host copies of ``mats`` (fp64) and return its results on ``dev``."""
    if dev.type != "cuda":
        return fn(*mats)
    host = [m.cpu() for m in mats]
    with _one_thread():
        out = fn(*host)
    if out is None:
        return None
    if isinstance(out, tuple):
        return tuple(o.to(dev, non_blocking=True) if torch.is_tensor(o) else o for o in out)
    return out.to(dev, non_blocking=True)



def _raw_basis_transform(GG, Gxp, lam_locked, ny, ncl, nxp, na, ortho_tol, eps):
    """Round 5, Rayleigh-Ritz on the raw basis (host, fp64; raw_basis_transform of csrc/host_dense.cpp is the same
    algebra, without the Cholesky gate).  GG = [Y X P W]^T [K W | M W]
    ((w0 + na) x 2 na, w0 = ny + ncl + nxp columns of the M-orthonormal V = [Y | X_locked | X_active P]).  Returns (G, Q):
    G = S_a^T K S_a for S_a = [X_a P W_o] (W_o = the M-orthonormalised projection of W) and Q = S_a in coordinates of the raw
    basis - or None when a single sweep would not be enough for this W."""
    w0 = ny + ncl + nxp
    pr = w0 + na
    GK, GM = GG[:, :na], GG[:, na:]
    C = GM[:w0]
    got = _project_in_coefficients(C, _sym(GM[w0:]), cholesky_gate=True)
    if got is None:
        return None
    T, _, amp = got
    if not (amp < float("inf")) or (ortho_tol > 0.0 and eps * amp >= ortho_tol):
        return None
    CT = C @ T
    GKraw = torch.zeros((pr, pr), dtype=GG.dtype)
    if ncl:
        GKraw[ny:ny + ncl, ny:ny + ncl] = torch.diag(lam_locked)
    GKraw[ny + ncl:w0, ny + ncl:w0] = Gxp
    GKraw[:w0, w0:] = GK[:w0]
    GKraw[w0:, :w0] = GK[:w0].transpose(0, 1)
    GKraw[w0:, w0:] = _sym(GK[w0:])
    Q = torch.zeros((pr, nxp + na), dtype=GG.dtype)
    Q[ny + ncl:w0, :nxp] = torch.eye(nxp, dtype=GG.dtype)
    Q[:w0, nxp:] = -CT
    Q[w0:, nxp:] = T
    return Q.transpose(0, 1) @ GKraw @ Q, Q


def _rr_step(GA, na):
    """Rayleigh-Ritz on the active basis: lowest na Ritz pairs and the coefficient block of the new P."""
    E_, Z = torch.linalg.eigh(_sym(GA))
    Z1 = Z[:, :na].contiguous()
    # P spans (I - Z1 Z1^T) E_x: the part of the old active X that left the new Ritz block - the same space
    # as the reference's S Z2 basis((Z[:b, b:])^T) (_lobpcg.py:466), but it needs only the wanted Ritz
    # vectors and a small Cholesky instead of a Householder QR of a (2b x b) matrix.
    Tm = -Z1 @ Z1[:na, :].transpose(0, 1)
    Tm[:na] += torch.eye(na, dtype=GA.dtype, device=GA.device)
    return E_[:na].contiguous(), Z1, _orthonormal_columns(Tm).contiguous()

