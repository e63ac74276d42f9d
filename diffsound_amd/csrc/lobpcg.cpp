// Native driver of the block eigensolver's iteration - the loop of ModalSolver._iterate_python (lobpcg/modal_solver.py) as ONE
// call per eigensolve.  It issues the same kernels (ds_spmm_union, ds_gram, ds_mix, ds_residual, ...) on the caller's stream and
// does the <= 3b x 3b dense steps on the calling host thread (LAPACK dsyevd / BLAS dgemm supplied by the embedding application
// through ds_lapack_t - the Python binding passes SciPy's), so a hypothesis lane spends its whole solve outside the interpreter:
// no interpreter lock between its launches, none between the lanes.  tests/test_modal_gpu.py runs both loops and compares.
//
// The dense steps live in host_dense.{h,cpp}, the twin of lobpcg/dense.py: project_in_coefficients, raw_basis_transform, rr_step
// and orthonormal_columns carry the same names in both, and tests/test_cabi_cpu.py checks one against the other without a device.
// What stays here is what touches the device: the stream-wait policy, the pinned staging ring, the device operations of a solve
// (Ctx) and the loop, whose phases are named after the pieces of the Python loop:
//   Solve::wait_residual_norms, converged   rel[] = ..., _converged
//   Solve::lock_width, lock                 ModalSolver._lock_width and the `if new_ncl > ncl` block
//   Solve::precondition                     precond_apply
//   Solve::ritz_problem_raw                 the `cfg.raw_rr` branch: apply_KM, one Gram, dense._raw_basis_transform
//   Solve::ritz_problem_explicit            ModalSolver._orthonormalize, then the `full` / recurrence branches and the assembly of
//                                           G at the top of modal_solver._ritz_step
//   rr_step (host_dense)                    dense._rr_step
//   Solve::update_basis                     ModalSolver._update_basis (raw, 2 na <= 160, split)
//   Solve::launch_residual                  the residual at the top of the Python loop, issued at the END of the iteration here
//   next_projected_K (host_dense)           Gxp_ of modal_solver._ritz_step - run on the host behind that launch
// Reference: the iteration of src/lobpcg/_lobpcg.py:344-376, 433-477 (LOBPCG.run / _update_ortho), whose per-iteration host
// synchronisations (float(torch.norm(..)) :655,663; the Python loop over a device tensor :323-328) are the two small
// device-to-host copies of this loop (residual norms, Gram blocks).
#include <atomic>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "ds_common.h"
#include "host_dense.h"

using namespace ds::dense;

namespace {
// How the host thread of a solve waits for its stream (ds_host_wait_mode; process-wide).  0: hipStreamSynchronize - under the
// runtime's default policy a SPIN whenever the host has more cores than devices.  1: a short poll, then a sleep on an event created
// with hipEventBlockingSync.  Eight hypothesis lanes spend four fifths of their time waiting for the device: spinning, they hold
// eight cores for nothing, and on a host that has only a few to give (a container under CPU quota beside busy neighbours) the
// lanes' dense steps queue behind the spinners - 52 passes/s against 60 with sleeping waits on four cores; with cores to spare
// the wake-up latency of a sleep costs 2 % (profiles/r05_host_wait_mode.txt).  One solve at a time keeps the spin.
std::atomic<int> g_wait_mode{0};

// One blocking event per (host thread, device), created on the device of the stream it first records and destroyed when the
// thread ends (a single thread_local event belonged to whatever device was current at its creation - a thread that
// later solved on a stream of another device got hipErrorInvalidResourceHandle - and was never destroyed: one leaked event per
// replaced lane pool).
struct WaitEvents {
    static constexpr int MAX_DEV = 64;
    hipEvent_t ev[MAX_DEV] = {};
    ~WaitEvents() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};
thread_local WaitEvents g_wait_events;

thread_local int g_solve_wait_mode = -1;  // wait mode of the solve running on this thread (ds_lobpcg_t.wait_mode); -1: the process default

hipError_t wait_for_stream(hipStream_t st) {
    const int mode = g_solve_wait_mode >= 0 ? g_solve_wait_mode : g_wait_mode.load(std::memory_order_relaxed);
    if (mode == 0) return hipStreamSynchronize(st);
    int dev = 0;
    hipError_t e = hipStreamGetDevice(st, &dev);  // (the stream's own device, not the thread's current one)
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= WaitEvents::MAX_DEV) return hipStreamSynchronize(st);
    hipEvent_t& ev = g_wait_events.ev[dev];
    if (!ev) {
        int cur = 0;
        if ((e = hipGetDevice(&cur)) != hipSuccess) return e;
        if (cur != dev && (e = hipSetDevice(dev)) != hipSuccess) return e;
        e = hipEventCreateWithFlags(&ev, hipEventBlockingSync | hipEventDisableTiming);
        if (cur != dev) (void)hipSetDevice(cur);
        if (e != hipSuccess) return e;
    }
    e = hipEventRecord(ev, st);
    if (e != hipSuccess) return e;
    const double t0 = now_s();
    while ((e = hipEventQuery(ev)) == hipErrorNotReady && now_s() - t0 < 20e-6) {}  // (what is about to finish needs no sleep)
    if (e != hipErrorNotReady) return e;
    return hipEventSynchronize(ev);
}

// column ranges of at most 84 columns (multiples of 4, as equal as possible) that tile a c-column block: what one launch of
// the neighbour-union kernels takes (the same rule as _HipBlockOps.col_slices of block_ops.py, which tiles the Python loop's
// products: change both or neither)
template <typename F>
int for_col_slices(int c, F&& fn) {
    if (c <= 84) return fn(0, c);
    const int k = (c + 83) / 84;
    const int w = (((c + k - 1) / k) + 3) / 4 * 4;
    for (int c0 = 0; c0 < c; c0 += w) {
        const int rc = fn(c0, std::min(c, c0 + w));
        if (rc != DS_OK) return rc;
    }
    return DS_OK;
}

// ---------------------------------------------------------------------------------------------------------------
constexpr double STORAGE_EPS = 6e-8;  // unit roundoff of the fp32 iterates (dense.storage_eps)
constexpr int COEF_SLOTS = 8;
// The device writes the squared column norms of a residual block to p->nrm: ||r_j||^2 at [j], ||x_j||^2 at [NORM_STRIDE + j].
// The pinned device-to-host staging area mirrors them and adds the Ritz values on their way to the device and the Gram block:
constexpr int NORM_STRIDE = 1024;
constexpr size_t BACK_NORMS = 0, BACK_LAM = 2 * NORM_STRIDE;  // [0, 2048): norms | [2048, 2048 + LAM_SLOT): Ritz values
constexpr int LAM_SLOT = 256;                                  // (>= the widest block, 160)
constexpr size_t BACK_GRAM = BACK_LAM + LAM_SLOT;              // | from there: one Gram block, <= (ny + 3 b) x 3 b

struct PinnedRing {  // per host thread, grown on demand, released when the thread ends
    ~PinnedRing() {
        if (host) (void)hipHostFree(host);
        if (back) (void)hipHostFree(back);
    }
    float* host = nullptr;
    size_t slot_floats = 0;
    double* back = nullptr;  // device-to-host staging (Gram blocks, residual norms): a pageable destination would
    size_t back_doubles = 0; // send the "asynchronous" copy through the runtime's shared staging path
    template <typename T>
    static int grow(T*& buf, size_t& have, size_t want, size_t copies, const char* what) {
        if (want <= have) return DS_OK;
        if (buf) (void)hipHostFree(buf);
        buf = nullptr, have = 0;
        const int rc = ds::check_hip(hipHostMalloc(reinterpret_cast<void**>(&buf), want * copies * sizeof(T), 0), what);
        if (rc == DS_OK) have = want;
        return rc;
    }
    int reserve_back(size_t doubles) { return grow(back, back_doubles, doubles, 1, "hipHostMalloc(result staging)"); }
    int reserve(size_t floats_per_slot) { return grow(host, slot_floats, floats_per_slot, COEF_SLOTS, "hipHostMalloc(coefficient staging)"); }
};
thread_local PinnedRing g_ring;

// The device operations of one solve
struct Ctx {
    ds_lobpcg_t* p;
    hipStream_t st;
    ds_stream_t stream;
    const ds_lapack_t& la;
    float *S, *S2, *KS, *KS2;
    PinnedRing* ring = &g_ring;
    int slot = 0;
    double sync_s = 0;  // host time spent waiting for the stream, and how often (DS_EXP_TIMING=1)
    int nsync = 0;

    int hip(hipError_t e, const char* what) { return ds::check_hip(e, what); }

    int wait() {
        const double t0 = now_s();
        const int rc = hip(wait_for_stream(st), "ds_lobpcg_iterate: stream synchronise");
        sync_s += now_s() - t0;
        ++nsync;
        return rc;
    }

    int gram(const float* A, int64_t lda, int pc, const float* B, int64_t ldb, int qc, bool sym, Mat& out) {
        const int flags = (sym ? DS_GRAM_SYMMETRIC : 0) | (p->gram_exact ? DS_GRAM_EXACT : 0);
        int rc = ds_gram(A, DS_F32, lda, pc, B, DS_F32, ldb, qc, p->n, flags, p->gbuf, p->gram_work, p->gram_work_bytes,
                         stream);
        if (rc != DS_OK) return rc;
        out = Mat(pc, qc);
        double* stage = ring->back + BACK_GRAM;
        rc = hip(hipMemcpyAsync(stage, p->gbuf, sizeof(double) * (size_t)pc * qc, hipMemcpyDeviceToHost, st),
                 "ds_lobpcg_iterate: Gram block to host");
        if (rc != DS_OK) return rc;
        if ((rc = wait()) == DS_OK) std::memcpy(out.a.data(), stage, sizeof(double) * (size_t)pc * qc);
        return rc;
    }

    // coefficient matrices travel through a ring of pinned host slots and matching device slots: an asynchronous copy
    // may read its source after the call returns, and a slot is reused only after >= 8 further updates - every
    // iteration synchronises the stream (Gram blocks) at least twice in between
    int mix(const float* A, int64_t lda, int pc, const Mat& C, float* Out, int64_t ldo, float alpha = 1.f, float beta = 0.f) {
        const size_t cnt = (size_t)C.r * C.c;
        const size_t stride = (size_t)(p->ny + 3 * p->b) * 2 * p->b;  // slot size of THIS solve (the ring may be larger)
        float* h = ring->host + (size_t)slot * stride;
        float* dv = p->cbuf + (size_t)slot * stride;
        slot = (slot + 1) % COEF_SLOTS;
        for (size_t i = 0; i < cnt; ++i) h[i] = (float)C.a[i];
        int rc = hip(hipMemcpyAsync(dv, h, sizeof(float) * cnt, hipMemcpyHostToDevice, st),
                     "ds_lobpcg_iterate: coefficients to device");
        if (rc != DS_OK) return rc;
        return ds_mix(A, lda, pc, dv, C.c, Out, ldo, p->n, alpha, beta, stream);
    }

    // (blocks wider than one launch of the neighbour-union kernels takes - a 136-column block, the periodic refresh K [X P W] -
    // go in column slices through the same kernels)
    int apply_K(const float* X, int64_t ldx, float* Y, int64_t ldy, int ncols) {
        const ds_level_t& L = p->level;
        if (ncols <= 84 && ncols % 4 == 0 && L.m32_gptr && L.m32_k && 3 * L.nv * ldx * 4 < (int64_t)0x7f000000)
            return ds_spmm_union32m(0, L.level_tag, L.m32_gptr, L.m32_gcol, L.m32_gmeta, L.m32_gbase, L.m32_k, L.nnzb * 36 + 16,
                                    L.nnzb, (L.nv + 3) / 4, L.m32_max_entries, L.m32_max_batch_blocks, L.nv, X, ldx, Y, ldy,
                                    ncols, stream);
        if (ncols % 4 == 0)
            return for_col_slices(ncols, [&](int c0, int c1) {
                return ds_spmm_union(0, L.level_tag, L.utab, L.ctab, L.ngroups, L.cap_blocks, L.gent, L.kgrp, L.nnzb, L.nv, X + c0, ldx,
                                     Y + c0, ldy, nullptr, 0, nullptr, c1 - c0, 0.f, 0.f, 0, nullptr, 0, stream);
            });
        for (int c0 = 0; c0 < ncols; c0 += 256) {  // odd widths: wave-per-node kernels
            const int c1 = std::min(ncols, c0 + 256);
            int rc = ds_spmm_bsr3(0, p->rowptr, p->colidx, p->k32, p->k32t, p->nv, X + c0, ldx, Y + c0, ldy, c1 - c0, stream);
            if (rc != DS_OK) return rc;
        }
        return DS_OK;
    }

    int apply_M(const float* X, int64_t ldx, float* Y, int64_t ldy, int ncols) {
        const ds_level_t& L = p->level;
        if (ncols <= 84 && L.m32_gptr && L.m32_m && 3 * L.nv * ldx * 4 < (int64_t)0x7f000000)
            return ds_spmm_union32m(3, L.level_tag, L.m32_gptr, L.m32_gcol, L.m32_gmeta, L.m32_gbase, L.m32_m, L.nnzb * 4 + 16,
                                    L.nnzb, (L.nv + 3) / 4, L.m32_max_entries, L.m32_max_batch_blocks, L.nv, X, ldx, Y, ldy,
                                    ncols, stream);
        return for_col_slices(ncols, [&](int c0, int c1) {
            return ds_spmm_union(3, L.level_tag, L.utab, L.ctab, L.ngroups, L.cap_blocks, L.gent, p->mgrp, L.nnzb, L.nv, X + c0, ldx,
                                 Y + c0, ldy, nullptr, 0, nullptr, c1 - c0, 0.f, 0.f, 0, nullptr, 0, stream);
        });
    }

    // K X -> KX and M X -> MX of one block in one walk of the unions
    int apply_KM(const float* X, int64_t ldx, float* KX, int64_t ldk, float* MX, int64_t ldm, int ncols) {
        const ds_level_t& L = p->level;
        return for_col_slices(ncols, [&](int c0, int c1) {
            return ds_spmm_union_km(L.level_tag, L.utab, L.ctab, L.ngroups, L.cap_blocks, L.gent, L.kgrp, p->mgrp, L.nnzb, L.nv,
                                    X + c0, ldx, KX + c0, ldk, MX + c0, ldm, c1 - c0, stream);
        });
    }

    // R = K X - (M X) diag(lam) and the column norms (nrm, nrm + NORM_STRIDE) in one walk of the unions per column slice
    int residual_fused(const float* X, int64_t ldx, float* R, int64_t ldr_, int ncols) {
        const ds_level_t& L = p->level;
        return for_col_slices(ncols, [&](int c0, int c1) {
            return ds_union_residual(L.level_tag, L.utab, L.ctab, L.ngroups, L.cap_blocks, L.gent, L.kgrp, p->mgrp, L.nnzb, L.nv,
                                     X + c0, ldx, p->lam_dev + c0, R + c0, ldr_, c1 - c0, p->res_work, p->res_work_bytes, p->nrm + c0,
                                     p->nrm + NORM_STRIDE + c0, stream);
        });
    }

    // The same walk handing the bf16 two-level cycle its inputs instead of the fp32 R (ds_union_residual_pre; <= 84 columns):
    // R16, and the fine smoother's first iterate in the block its first term reads (chebyshev16: D, or Wc when no term follows)
    int residual_handoff(const float* X, int64_t ldx, int ncols) {
        const ds_level_t& L = p->level;
        const ds_twolevel_t& t = *p->twolevel;
        const double theta = 0.5 * (t.fine.lmax + t.fine.lmin);
        void* w1 = t.fine.degree >= 2 ? static_cast<void*>(t.D) : static_cast<void*>(t.Wc);
        return ds_union_residual_pre(L.level_tag, L.utab, L.ctab, L.ngroups, L.cap_blocks, L.gent, L.kgrp, p->mgrp, L.nnzb, L.nv, X, ldx,
                                     p->lam_dev, t.fine.dinv, (float)(1.0 / theta), t.R16, t.ldr16, w1, t.ldd, ncols, p->res_work,
                                     p->res_work_bytes, p->nrm, p->nrm + NORM_STRIDE, stream);
    }

    int copy_cols(float* dst, int64_t ldd, const float* src, int64_t lds_, int ncols) {
        if (ncols <= 0) return DS_OK;
        return hip(hipMemcpy2DAsync(dst, (size_t)ldd * 4, src, (size_t)lds_ * 4, (size_t)ncols * 4, (size_t)p->n,
                                    hipMemcpyDeviceToDevice, st),
                   "ds_lobpcg_iterate: column copy");
    }

    // W <- B R  (two-level V-cycle, or the one-level Chebyshev polynomial W = p(T K) T R); columns are independent: blocks wider
    // than the fused kernels take go in slices that share the scratch blocks (stream order)
    // handed >= 0: the residual walk wrote the cycle's inputs (residual_handoff) and `handed` leading columns of them have been
    // locked since: the cycle starts at its first term, on the bf16 blocks from that column on (a multiple of 4: 8-byte steps,
    // which is what the term kernels ask of their bf16 operands)
    int precond(float* R, int na, float* W, int64_t ldw, int handed = -1) {
        return for_col_slices(na, [&](int c0, int c1) {
            if (p->twolevel) {
                ds_twolevel_t d = *p->twolevel;
                d.R = R + c0, d.ldr = p->ldr, d.W = W + c0, d.ldw = ldw, d.ncols = c1 - c0;
                if (handed >= 0) {
                    auto skip = [&](void* blk) { return static_cast<void*>(static_cast<uint16_t*>(blk) + handed); };
                    d.storage |= DS_TL_PREPARED;
                    d.R16 = skip(d.R16);
                    if (d.fine.degree >= 2) d.D = static_cast<float*>(skip(d.D));
                    else d.Wc = static_cast<float*>(skip(d.Wc));
                }
                return ds_twolevel_apply(&d, stream);
            }
            if (p->pr16)
                return ds_chebyshev_apply16(&p->level, R + c0, p->ldr, W + c0, ldw, p->pa, p->pb, p->pr16, p->ldp, c1 - c0, stream);
            return ds_chebyshev_apply(&p->level, R + c0, p->ldr, W + c0, ldw, p->pa, p->pb, p->ldp, c1 - c0, stream);
        });
    }

    // W (n x na, column range [w0, w0 + na) of S) M-orthogonal to V = S[:, :w0] and M-orthonormal (ModalSolver._orthonormalize)
    int orthonormalize(int w0, int na) {
        float* W = S + w0;
        const int64_t ld = p->lds;
        const auto lapack_failed = [] {
            ds::set_error("ds_lobpcg_iterate: dsyevd failed in the orthonormalisation");
            return DS_ERR_ARG;
        };
        for (int ip = 0; ip < p->ortho_passes; ++ip) {
            int rc = apply_M(W, ld, p->MW, p->ldr, na);
            if (rc != DS_OK) return rc;
            bool done = false;
            double amp = 0.0;
            if (w0 > 0 && ip == 0) {  // projection and orthonormalisation in ONE update, in coefficients
                Mat G;
                if ((rc = gram(S, ld, w0 + na, p->MW, p->ldr, na, false, G)) != DS_OK) return rc;
                const Mat C = G.block(0, 0, w0, na);
                Mat G0 = G.block(w0, 0, na, na), T, CtC;
                symmetrize(G0);
                // (with the Cholesky gate: a block it turns away is projected and orthonormalised explicitly below)
                const Projected got = project_in_coefficients(la, C, G0, true, T, CtC, amp);
                if (got == Projected::LapackFailed) return lapack_failed();
                if (got == Projected::Ok) {
                    Mat CT = gemm(la, C, false, T, false);
                    for (double& v : CT.a) v = -v;
                    Mat coef(w0 + na, na);
                    coef.set_block(0, 0, CT);
                    coef.set_block(w0, 0, T);
                    if ((rc = mix(S, ld, w0 + na, coef, W, ld)) != DS_OK) return rc;  // in place (W trails V in S)
                    done = true;
                }
            }
            if (!done) {
                std::vector<double> rem;
                if (w0 > 0) {
                    Mat C;
                    if ((rc = gram(S, ld, w0, p->MW, p->ldr, na, false, C)) != DS_OK) return rc;
                    if ((rc = mix(S, ld, w0, C, W, ld, -1.f, 1.f)) != DS_OK) return rc;
                    rem.assign(na, 0.0);
                    for (int i = 0; i < w0; ++i)
                        for (int j = 0; j < na; ++j) rem[j] += C(i, j) * C(i, j);
                    if ((rc = apply_M(W, ld, p->MW, p->ldr, na)) != DS_OK) return rc;
                }
                Mat G;
                if ((rc = gram(W, ld, na, p->MW, p->ldr, na, true, G)) != DS_OK) return rc;
                Mat T;
                if (!orthonormalizer_q(la, G, w0 > 0 ? &rem : nullptr, T, amp)) return lapack_failed();
                if ((rc = mix(W, ld, na, T, W, ld)) != DS_OK) return rc;  // in place: na <= b <= 160 columns, what ds_mix takes aliased
            }
            if (p->ortho_tol > 0.0 && STORAGE_EPS * amp < p->ortho_tol) break;
        }
        return DS_OK;
    }
};

// One solve: the state the phases of the iteration share (the locals of ModalSolver._iterate_python) and the phases themselves.
// Layout of the basis buffer: S = [Y (ny) | X_locked (ncl) | X_a (na) | P (npc) | W (na)], the active basis S_a = [X_a P W].
struct Solve {
    Ctx c;
    ds_lobpcg_t* const p = c.p;
    const ds_lapack_t& la = c.la;
    const int b = p->b, k = p->k, ny = p->ny;
    const int64_t lds = p->lds, ldks = p->ldks, ldr = p->ldr;
    // the fused residual needs the operands the neighbour-union kernel takes (one descriptor per operand block) and replaces
    // the fresh K X' of kx_fresh - without kx_fresh K X' comes out of the recurrence and is there anyway
    const bool fused_res = p->res_work && p->kx_fresh &&
                           p->res_work_bytes >= ds_union_residual_workspace_bytes(p->level.ngroups, std::min(b, 84));
    // Rayleigh-Ritz on the raw basis: K X' must not be needed from K [X P W] (kx_fresh) and comes from the fused residual
    const bool raw = p->raw_rr && fused_res && !p->gram_exact;
    // the residual walk hands the preconditioner its inputs: the bf16 two-level cycle with node blocks on the fine level, whose first
    // launch would only convert R and apply the node blocks to it - nobody else reads the fp32 R on this route
    const bool handoff = fused_res && p->twolevel && p->twolevel->storage == DS_TL_BF16 && p->twolevel->R16 &&
                         !p->twolevel->fine.tgrp && p->twolevel->fine.dinv && p->twolevel->fine.nv == p->level.nv &&
                         p->level.level_tag == 0;

    std::vector<double> lam = std::vector<double>(p->lam, p->lam + b);
    // Ritz values of the step before (p->ritz_tol > 0: a pair also has to have SETTLED to count as converged - see the header)
    std::vector<double> lam_prev = std::vector<double>(b, std::numeric_limits<double>::infinity());
    std::vector<double> rel = std::vector<double>(b, std::numeric_limits<double>::infinity());
    Mat Gxp;                // [X_a P]^T K [X_a P] of the basis the last Ritz step produced (at the start: diag(lam))
    int ncl = 0;            // locked (converged) leading columns, a multiple of 4
    int npc = 0;            // columns of P
    int k0 = 0;             // first column of K X_a inside KS (columns locked since the last Ritz step are skipped)
    int since_refresh = 0;  // Ritz steps since [X P W]^T K [X P W] was last measured whole
    bool handed = false;    // the residual in flight was launched in the hand-off form

    int na() const { return b - ncl; }
    int nxp() const { return na() + npc; }
    int sz() const { return nxp() + na(); }
    int w0() const { return ny + b + npc; }
    float* Xa() const { return c.S + ny + ncl; }  // (where S_a starts, too)
    float* W() const { return c.S + w0(); }
    float* KSa() const { return c.KS + k0; }

    // The residual R = K X - (M X) diag(lam) of the CURRENT Ritz block and its norms: launched at the end of an iteration, right
    // behind the update that wrote the block (and once before the loop) - next_projected_K, which only the NEXT Ritz step needs,
    // then runs on the host while the device works on the update and this residual (one lane alone is bound by the host's steps)
    int launch_residual() {
        const int na = this->na();
        double* lam_pin = c.ring->back + BACK_LAM;  // (the previous iteration's copy completed before its last synchronise)
        std::memcpy(lam_pin, lam.data() + ncl, sizeof(double) * na);
        int rc = c.hip(hipMemcpyAsync(p->lam_dev, lam_pin, sizeof(double) * na, hipMemcpyHostToDevice, c.st),
                       "ds_lobpcg_iterate: Ritz values to device");
        if (rc != DS_OK) return rc;
        if (fused_res) {  // R = K X - (M X) diag(lam) and the norms in one walk of the unions; K X, M X never reach memory
            handed = handoff && na <= 84;  // (one launch of the walk, one application of the cycle)
            if ((rc = handed ? c.residual_handoff(Xa(), lds, na) : c.residual_fused(Xa(), lds, p->R, ldr, na)) != DS_OK) return rc;
        } else {
            if ((rc = c.apply_M(Xa(), lds, p->MX, ldr, na)) != DS_OK) return rc;
            if ((rc = ds_residual(KSa(), ldks, p->R, ldr, p->MX, ldr, Xa(), lds, p->lam_dev, p->n, na, p->nrm, p->nrm + NORM_STRIDE,
                                  c.stream)) != DS_OK)
                return rc;
        }
        return c.hip(hipMemcpyAsync(c.ring->back + BACK_NORMS, p->nrm, sizeof(double) * 2 * NORM_STRIDE, hipMemcpyDeviceToHost, c.st),
                     "ds_lobpcg_iterate: residual norms to host");
    }

    // waits for the residual in flight: rel = ||K x - lam M x|| / (||x|| (A_norm + |lam| B_norm)) of the active columns
    int wait_residual_norms() {
        const int rc = c.wait();
        if (rc != DS_OK) return rc;
        const double* nrm = c.ring->back + BACK_NORMS;
        for (int j = 0; j < na(); ++j)
            rel[ncl + j] = std::sqrt(nrm[j] / nrm[NORM_STRIDE + j]) / (p->A_norm + std::fabs(lam[ncl + j]) * p->B_norm);
        return DS_OK;
    }

    // number of LEADING wanted pairs that pass the convergence test (reference _lobpcg.py:321-328)
    int converged() const {
        int nconv = 0;
        while (nconv < k && rel[nconv] < p->tol &&
               (p->ritz_tol <= 0.0 || std::fabs(lam[nconv] - lam_prev[nconv]) <= p->ritz_tol * std::fabs(lam[nconv])))
            ++nconv;
        return nconv;
    }

    double worst() const {  // max backward error of the wanted pairs
        double w = 0.0;
        for (int j = 0; j < k; ++j) w = std::max(w, rel[j]);
        return w;
    }

    int lock_width(int nconv) const { return p->lock ? (nconv / 4) * 4 : 0; }

    // hard locking: converged leading columns leave the Ritz problem, the residual block and the preconditioner.
    // Returns in `shift` how many columns were locked now.
    int lock(int new_ncl, int& shift) {
        shift = std::max(0, new_ncl - ncl);
        if (shift == 0) return DS_OK;
        // the newly locked columns leave the residual block by a pointer offset (precondition: a multiple of 4 columns, 16-byte
        // aligned) and enter the OTHER basis buffer once, here - from then on both buffers hold them
        const int rc = c.copy_cols(c.S2 + ny + ncl, lds, c.S + ny + ncl, lds, shift);
        if (rc != DS_OK) return rc;
        Gxp = Gxp.block(shift, shift, Gxp.r - shift, Gxp.c - shift);
        k0 += shift;
        ncl = new_ncl;
        return DS_OK;
    }

    // W = B R on the residual columns of the pairs that stay active (the bf16 blocks of a handed-off residual are skipped by the
    // same offset: Ctx::precond)
    int precondition(int locked_now) { return c.precond(p->R + locked_now, na(), W(), lds, handed ? locked_now : -1); }

    bool refresh_due() const { return p->rr_refresh <= 0 || since_refresh >= p->rr_refresh; }

    // The Ritz problem on the RAW basis (p->raw_rr): W stays as the preconditioner left it.  K W and M W come out of one walk of
    // the unions, [Y X P W]^T [K W | M W] out of ONE Gram launch, and raw_basis_transform folds the projection of W against the
    // M-orthonormal [Y X P] and its orthonormalisation into coefficients (an iteration was M W, Gram, update, K W, Gram, update; it
    // is [K W | M W], Gram, update).  taken = false: this W is too ill-conditioned for a single sweep - the explicit route below.
    int ritz_problem_raw(Mat& G, Mat& Qw, bool& taken) {
        const int na = this->na();
        int rc = c.apply_KM(W(), lds, c.KS, ldks, c.KS + na, ldks, na);
        if (rc != DS_OK) return rc;
        Mat GG;
        if ((rc = c.gram(c.S, lds, w0() + na, c.KS, ldks, 2 * na, false, GG)) != DS_OK) return rc;
        taken = raw_basis_transform(la, GG, Gxp, lam.data(), ny, ncl, nxp(), na, p->ortho_tol, STORAGE_EPS, G, Qw);
        if (taken) ++since_refresh;
        return DS_OK;
    }

    // The Ritz problem on the orthonormalised basis: W is projected against [Y X P] and M-orthonormalised on the device, then
    // G = S_a^T K S_a is measured whole (`full`, the periodic refresh) or only its new columns S_a^T K W are, the blocks among
    // X_a and P coming from the last Ritz step (Gxp)
    int ritz_problem_explicit(bool full, Mat& G) {
        const int na = this->na(), nxp = this->nxp(), sz = this->sz();
        int rc = c.orthonormalize(w0(), na);
        if (rc != DS_OK) return rc;
        if (full) {
            if ((rc = c.apply_K(Xa(), lds, KSa(), ldks, sz)) != DS_OK) return rc;
            since_refresh = 0;
            return c.gram(Xa(), lds, sz, KSa(), ldks, sz, true, G);
        }
        if ((rc = c.apply_K(W(), lds, KSa() + nxp, ldks, na)) != DS_OK) return rc;
        Mat GA;
        if ((rc = c.gram(Xa(), lds, sz, KSa() + nxp, ldks, na, false, GA)) != DS_OK) return rc;
        G = Mat(sz, sz);
        G.set_block(0, 0, Gxp);
        G.set_block(0, nxp, GA);
        G.set_block_T(nxp, 0, GA.block(0, 0, nxp, na));
        ++since_refresh;
        return DS_OK;
    }

    void take_ritz_values(const std::vector<double>& E) {
        for (int j = 0; j < na(); ++j) lam_prev[ncl + j] = lam[ncl + j], lam[ncl + j] = E[j];
    }

    // [X' P'] = S_a [Z1 Zp] into the other buffer (and K X', K P' where the configuration keeps them), which then becomes current.
    // Three shapes: with Qw the operand is the whole raw basis [Y X P W] and the coefficients are [E | Qw] [Z1 Zp]; X' and P' are
    // adjacent column ranges, so 2 na <= 160 columns go in ONE update per operand; wider blocks are split into X' and P'.
    int update_basis(const Mat& Z1, const Mat& Zp, const Mat* Qw) {
        const int na = this->na();
        const auto mix_xp = [&](const float* A, int64_t lda, int rows, const Mat& Z, float* X2, float* P2, int64_t ldo) {
            if (2 * na <= 160) return c.mix(A, lda, rows, Z, X2, ldo);
            const int rc = c.mix(A, lda, rows, Z.block(0, 0, rows, na), X2, ldo);
            return rc != DS_OK ? rc : c.mix(A, lda, rows, Z.block(0, na, rows, na), P2, ldo);
        };
        float *X2 = c.S2 + ny + ncl, *P2 = c.S2 + ny + b;
        const Mat ZZ = hcat(Z1, Zp);
        int rc;
        if (Qw) {
            rc = mix_xp(c.S, lds, w0() + na, raw_update_coefficients(la, *Qw, ZZ, ny, ncl, nxp(), na), X2, P2, lds);
        } else {
            rc = mix_xp(Xa(), lds, sz(), ZZ, X2, P2, lds);
            if (rc == DS_OK && !p->kx_fresh) rc = mix_xp(KSa(), ldks, sz(), ZZ, c.KS2, c.KS2 + na, ldks);
        }
        if (rc != DS_OK) return rc;
        // K X' fresh: one b-column product instead of the 3b -> 2b column update of K [X P W] (K P' is never needed)
        // (with the fused residual the next iteration forms K X' inside its residual kernel and nobody else reads it)
        if (p->kx_fresh && !fused_res && (rc = c.apply_K(X2, lds, c.KS2, ldks, na)) != DS_OK) return rc;
        std::swap(c.S, c.S2);
        std::swap(c.KS, c.KS2);
        k0 = 0;
        npc = na;
        return DS_OK;
    }
};

}  // namespace

extern "C" int ds_host_wait_mode(int mode) {
    DS_REQUIRE(mode == 0 || mode == 1, "ds_host_wait_mode: 0 (the runtime's stream synchronisation) or 1 (poll, then sleep on a blocking event)");
    g_wait_mode.store(mode, std::memory_order_relaxed);
    return DS_OK;
}

extern "C" int ds_lobpcg_iterate(ds_lobpcg_t* p, const ds_lapack_t* lapack, ds_stream_t stream) {
    DS_REQUIRE(p && lapack && lapack->dsyevd && lapack->dgemm, "ds_lobpcg_iterate: null descriptor or LAPACK table");
    DS_REQUIRE((!lapack->dsytrd) == (!lapack->dstedc) && (!lapack->dsytrd) == (!lapack->dormtr),
               "ds_lobpcg_iterate: the staged eigensolver needs dsytrd, dstedc and dormtr together (or none of them)");
    DS_REQUIRE(p->S && p->S2 && p->KS && p->KS2 && p->R && p->MX && p->MW && p->lam && p->rerr && p->gbuf && p->cbuf &&
                   p->nrm && p->lam_dev && p->gram_work && p->mgrp,
               "ds_lobpcg_iterate: null buffer");
    // (<= 160: the in-place updates of the orthonormalisation go through ds_mix, which takes an aliased result only up to 160
    // columns - blocks of 164 / 168 columns stay on the Python loop, which splits that update)
    DS_REQUIRE(p->b > 0 && p->b <= 160 && p->b % 4 == 0 && p->k > 0 && p->k <= p->b && (p->ny == 0 || p->ny % 4 == 0),
               "ds_lobpcg_iterate: block width must be a multiple of 4 <= 160 (got %d)", p->b);
    DS_REQUIRE(p->n == 3 * p->nv && p->n >= 3 * p->b + p->ny, "ds_lobpcg_iterate: bad problem size");
    DS_REQUIRE(p->twolevel || (p->pa && p->pb), "ds_lobpcg_iterate: no preconditioner scratch");
    DS_REQUIRE(p->wait_mode >= -1 && p->wait_mode <= 1, "ds_lobpcg_iterate: wait_mode is -1 (the process default), 0 or 1");
    struct WaitScope {  // this solve's own way of waiting for its stream (per solve, i.e. per hypothesis lane)
        int saved;
        explicit WaitScope(int m) : saved(g_solve_wait_mode) { g_solve_wait_mode = m; }
        ~WaitScope() { g_solve_wait_mode = saved; }
    } wait_scope(p->wait_mode);
    const int b = p->b, k = p->k, ny = p->ny;
    int rc;
    // cbuf holds COEF_SLOTS slots of (ny + 3 b) x 2 b floats; the result staging: norms | Ritz values | Gram block
    if ((rc = g_ring.reserve((size_t)(ny + 3 * b) * 2 * b)) != DS_OK) return rc;
    if ((rc = g_ring.reserve_back(BACK_GRAM + (size_t)(ny + 3 * b) * 3 * b)) != DS_OK) return rc;
    g_timers = Timers();
    const double t_begin = now_s();
    // (the periodic full refresh multiplies K by [X P W], up to 3 b columns, in column slices through the union kernels: the
    // plain BSR arrays are no longer needed for it - every width the loop forms is a multiple of 4)
    Solve s{Ctx{p, ds::as_stream(stream), stream, *lapack, p->S, p->S2, p->KS, p->KS2}};
    s.Gxp = Mat(b, b);
    for (int i = 0; i < b; ++i) s.Gxp(i, i) = s.lam[i];
    if ((rc = s.launch_residual()) != DS_OK) return rc;
    int it;
    for (it = 0; it <= p->maxit; ++it) {
        if ((rc = s.wait_residual_norms()) != DS_OK) return rc;
        const int nconv = s.converged();
        if (p->history && it < p->history_cap) p->history[it] = s.worst();
        if (nconv >= k || it == p->maxit) break;
        int locked_now;
        if ((rc = s.lock(s.lock_width(nconv), locked_now)) != DS_OK) return rc;
        if ((rc = s.precondition(locked_now)) != DS_OK) return rc;
        const bool full = s.refresh_due();
        Mat G, Qw;  // S_a^T K S_a of the active basis S_a = [X_a P W_o]; by the raw route also W_o in the raw basis [Y X P W]
        bool by_raw = false;
        if (s.raw && !full && (rc = s.ritz_problem_raw(G, Qw, by_raw)) != DS_OK) return rc;
        if (!by_raw && (rc = s.ritz_problem_explicit(full, G)) != DS_OK) return rc;
        // Rayleigh-Ritz: lowest na pairs, and P = the part of the old active X that left the new Ritz block
        std::vector<double> E;
        Mat Z1, Zp;
        if (!rr_step(*lapack, G, s.na(), E, Z1, Zp)) return DS_ERR_ARG;
        s.take_ritz_values(E);
        if ((rc = s.update_basis(Z1, Zp, by_raw ? &Qw : nullptr)) != DS_OK) return rc;
        if ((rc = s.launch_residual()) != DS_OK) return rc;  // (of the block just written: the next iteration's first wait)
        // behind the launches, while the device runs the update and the residual:
        s.Gxp = next_projected_K(*lapack, G, E, Z1, Zp);
    }
    if (getenv("DS_EXP_TIMING")) {
        const double total = now_s() - t_begin;
        fprintf(stderr, "lobpcg n=%lld b=%d: %d iterations, host total %.2f ms: waiting for the stream %.2f ms (%d syncs), dsyevd %.2f ms (%d calls), dgemm %.2f ms, rest (launch calls, Cholesky, copies) %.2f ms\n",
                (long long)p->n, b, it, total * 1e3, s.c.sync_s * 1e3, s.c.nsync, g_timers.eigh * 1e3, g_timers.neigh, g_timers.dense * 1e3,
                (total - s.c.sync_s - g_timers.eigh - g_timers.dense) * 1e3);
    }
    p->iterations = it;
    p->result_in_s2 = (s.c.S == p->S) ? 0 : 1;
    std::memcpy(p->lam, s.lam.data(), sizeof(double) * b);
    std::memcpy(p->rerr, s.rel.data(), sizeof(double) * b);
    return DS_OK;
}
