// Neighbour-union SpMM on the tables of 4-node groups: the production walk with its epilogues (spmm_union.inc), its form for
// narrow blocks (spmm_narrow.inc), the packing of the block values into group order and the two norm reductions behind the fused
// residual, with their entry points.  Exports ds_pack_groups, ds_spmm_union, ds_spmm_union_narrow,
// ds_union_residual_workspace_bytes, ds_union_residual, ds_union_residual_pre, ds_spmm_union_km, ds_spmm_union16.
#include <algorithm>
#include <cstdint>
#include <type_traits>

#include "spmm_device.h"

namespace {
#include "spmm_union.inc"
#include "spmm_narrow.inc"
}  // namespace

// ------------------------------------------------------------------------------------------------
// Pack the (transposed) blocks into the entry-major / node-minor order of the neighbour-union tables.
__global__ void pack_groups_kernel(const float* __restrict__ vals_t, const int32_t* __restrict__ kperm, int64_t nnzb,
                                   float* __restrict__ kgrp) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nnzb * 9) return;
    const int64_t p = i / 9;
    kgrp[i] = vals_t[(int64_t)kperm[p] * 9 + (i - p * 9)];
}

extern "C" int ds_pack_groups(const float* vals_t, const int32_t* kperm, int64_t nnzb, float* kgrp,
                              ds_stream_t stream) {
    DS_REQUIRE(vals_t && kperm && kgrp && nnzb > 0, "ds_pack_groups: bad argument");
    pack_groups_kernel<<<(unsigned)ds::ceil_div(nnzb * 9, 256), 256, 0, ds::as_stream(stream)>>>(vals_t, kperm, nnzb,
                                                                                                kgrp);
    DS_LAUNCH_CHECK("pack_groups_kernel");
    return DS_OK;
}

// What every walk of the <= 84-column unions refuses alike, under its caller's name: a group count or a column count the tables
// and the lane layout do not fit, and chunks larger than the kernel's LDS image.  (cap_note: what ds_spmm_union adds to the
// second message.)  The narrow walk has a column range of its own and no LDS image of the chunks.
static int check_union_shape(const char* who, int64_t ngroups, int cap_blocks, int64_t nnzb, int64_t nv, int ncols,
                             const char* cap_note = "") {
    DS_REQUIRE(nv > 0 && ngroups == (nv + 3) / 4 && nnzb > 0 && ncols > 0 && ncols % 4 == 0 && ncols <= 84,
               "%s: ncols must be a multiple of 4 <= 84 and ngroups = ceil(nv / 4)", who);
    DS_REQUIRE(cap_blocks > 0 && cap_blocks <= UN_CAPB, "%s: a chunk of %d blocks exceeds the LDS image%s", who, cap_blocks, cap_note);
    return DS_OK;
}

extern "C" int ds_spmm_union(int epilogue, int level_tag, const int32_t* utab, const int32_t* ctab, int64_t ngroups, int cap_blocks,
                             const int32_t* gent,
                             const float* kgrp, int64_t nnzb, int64_t nv, const float* X, int64_t ldx, float* Y,
                             int64_t ldy, const float* R0, int64_t ldr, const float* dinv, int ncols, float c1, float c2,
                             int first, const float* Wprev, int64_t ldp, ds_stream_t stream) {
    DS_REQUIRE(ctab && gent && kgrp && X && Y, "ds_spmm_union: null pointer");
    DS_REQUIRE(epilogue >= 0 && epilogue <= 3, "ds_spmm_union: bad epilogue %d", epilogue);
    DS_REQUIRE(level_tag == 0 || level_tag == 1, "ds_spmm_union: level_tag must be 0 (fine) or 1 (corner-node level)");
    DS_REQUIRE(epilogue == 0 || epilogue == 3 || R0, "ds_spmm_union: the epilogue needs R0");
    DS_REQUIRE(epilogue != 1 || dinv, "ds_spmm_union: the Chebyshev epilogue needs dinv");
    if (int rc = check_union_shape("ds_spmm_union", ngroups, cap_blocks, nnzb, nv, ncols, " (DS_UNION_CAP = 140)")) return rc;
    DS_REQUIRE(ldx >= ncols && ldy >= ncols && (epilogue == 0 || epilogue == 3 || ldr >= ncols),
               "ds_spmm_union: leading dimension smaller than ncols");
    DS_REQUIRE(X != Y, "ds_spmm_union: X and Y must be different buffers");
    DS_REQUIRE(ldx * 12 < (int64_t)PIPE_OOB && ldy * 12 < (int64_t)PIPE_OOB && ldr * 12 < (int64_t)PIPE_OOB &&
                   nv * 36 < (int64_t)PIPE_OOB,
               "ds_spmm_union: a 3-row panel of %lld bytes exceeds the descriptor range", (long long)(ldx * 12));
    DS_REQUIRE(nnzb * 36 < ((int64_t)1 << 32), "ds_spmm_union: value array exceeds the descriptor range");
    uintptr_t al = reinterpret_cast<uintptr_t>(X) | reinterpret_cast<uintptr_t>(Y) | (uintptr_t)(ldx * 4) |
                   (uintptr_t)(ldy * 4) | reinterpret_cast<uintptr_t>(kgrp) | reinterpret_cast<uintptr_t>(ctab);
    if (epilogue == 1 || epilogue == 2) al |= reinterpret_cast<uintptr_t>(R0) | (uintptr_t)(ldr * 4);
    DS_REQUIRE((al & 15) == 0, "ds_spmm_union: rows, kgrp and ctab must be 16-byte aligned");
    hipStream_t st = ds::as_stream(stream);
    ChebEpilogue epi{R0, ldr, dinv, c1, c2, first};
    if (Wprev && epilogue == 1) {
        DS_REQUIRE(ldp >= ncols && ldp * 12 < (int64_t)PIPE_OOB &&
                       ((reinterpret_cast<uintptr_t>(Wprev) | (uintptr_t)(ldp * 4)) & 15) == 0 && Wprev != X,
                   "ds_spmm_union: bad W_prev block");
        epi.wprev = Wprev, epi.ldp = ldp;
    }
    const int lpn = ncols / 4;
    // (kinds of the timing hook: the fused term, Y = K X, Y = M_s X; the residual epilogue 2 is not recorded)
    const int pkind = epilogue == 1 ? DS_PROF_TERM : (epilogue == 0 ? DS_PROF_KX : (epilogue == 3 ? DS_PROF_MX : -1));
    ds::ProfScope prof(pkind < 0 ? nullptr : stream, pkind < 0 ? 0 : pkind, nv, nnzb, ncols, (first ? 1 : 0) | (4 << 8));
#define DS_U(L, E) return launch_union<L, E>(utab, ctab, ngroups, cap_blocks, gent, kgrp, nnzb, nv, X, ldx, Y, ldy, lpn, st, epi)
#define DS_UL(L, E) do { if (level_tag == 1) return launch_union<L, E, false, true, 1>(utab, ctab, ngroups, cap_blocks, gent, kgrp, nnzb, nv, X, ldx, Y, ldy, lpn, st, epi); \
                         return launch_union<L, E, false, true, 0>(utab, ctab, ngroups, cap_blocks, gent, kgrp, nnzb, nv, X, ldx, Y, ldy, lpn, st, epi); } while (0)
    if (lpn == 20) {
        if (epilogue == 1) DS_U(20, 1);
        if (epilogue == 2) DS_U(20, 2);
        if (epilogue == 3) DS_UL(20, 3);
        DS_UL(20, 0);
    }
    if (epilogue == 1) DS_U(0, 1);
    if (epilogue == 2) DS_U(0, 2);
    if (epilogue == 3) DS_UL(0, 3);
    DS_UL(0, 0);
#undef DS_UL
#undef DS_U
}

// Narrow blocks (<= 16 columns): the lanes dealt over the union's entries (spmm_narrow.inc)
extern "C" int ds_spmm_union_narrow(int kind, int level_tag, const int32_t* utab, const int32_t* ctab, int64_t ngroups,
                                    const int32_t* gent, const float* vals, int64_t nnzb, int64_t nv, const float* X, int64_t ldx,
                                    float* Y, int64_t ldy, int ncols, ds_stream_t stream) {
    DS_REQUIRE(ctab && gent && vals && X && Y, "ds_spmm_union_narrow: null pointer");
    DS_REQUIRE(kind == 0 || kind == 3, "ds_spmm_union_narrow: kind must be 0 (3x3 blocks) or 3 (node-scalar values)");
    DS_REQUIRE(level_tag == 0 || level_tag == 1, "ds_spmm_union_narrow: level_tag must be 0 (fine) or 1 (corner-node level)");
    DS_REQUIRE(nv > 0 && ngroups == (nv + 3) / 4 && nnzb > 0 && ncols > 0 && ncols % 4 == 0 && ncols <= 16,
               "ds_spmm_union_narrow: ncols must be a multiple of 4 <= 16 and ngroups = ceil(nv / 4)");
    DS_REQUIRE(ldx >= ncols && ldy >= ncols, "ds_spmm_union_narrow: leading dimension smaller than ncols");
    DS_REQUIRE(X != Y, "ds_spmm_union_narrow: X and Y must be different buffers");
    const uintptr_t al = reinterpret_cast<uintptr_t>(X) | reinterpret_cast<uintptr_t>(Y) | (uintptr_t)(ldx * 4) | (uintptr_t)(ldy * 4) |
                         reinterpret_cast<uintptr_t>(ctab);
    DS_REQUIRE((al & 15) == 0, "ds_spmm_union_narrow: rows and ctab must be 16-byte aligned");
    hipStream_t st = ds::as_stream(stream);
    const unsigned nwg = (unsigned)ds::ceil_div(ngroups, 4);
    ds::ProfScope prof(stream, kind == 0 ? DS_PROF_KX : DS_PROF_MX, nv, nnzb, ncols, 4 << 8);
#define DS_UN(S, V) spmm_union_narrow_kernel<S, V><<<nwg, 256, 0, st>>>(reinterpret_cast<const int2*>(utab), reinterpret_cast<const int4*>(ctab), \
                                                                       (unsigned)ngroups, gent, vals, nv, X, ldx, Y, ldy, ncols, nwg)
    if (kind == 0) {
        if (level_tag == 1) DS_UN(false, 1);
        else DS_UN(false, 0);
    } else {
        if (level_tag == 1) DS_UN(true, 1);
        else DS_UN(true, 0);
    }
#undef DS_UN
    DS_LAUNCH_CHECK("spmm_union_narrow_kernel");
    return DS_OK;
}

// The eigensolver's residual in ONE walk of the unions (spmm_union.inc, epilogue 4): R = K X - (M_s (x) I3) X diag(lam) and
// the column norms ||R_j||^2, ||X_j||^2, with neither K X nor M X written to memory.
extern "C" int64_t ds_union_residual_workspace_bytes(int64_t ngroups, int ncols) {
    return ngroups * 2 * (int64_t)ncols * 4 + (int64_t)UN_NORM_BLOCKS * 2 * ncols * 8;
}

// (R16 == nullptr: epilogue 4, the fp32 rows of R; else epilogue 6, the bf16 cycle's inputs R16 and W1 in their place)
static int union_residual(const char* who, int level_tag, const int32_t* utab, const int32_t* ctab, int64_t ngroups, int cap_blocks,
                          const int32_t* gent, const float* kgrp, const float* mgrp, int64_t nnzb, int64_t nv, const float* X,
                          int64_t ldx, const double* lam, float* R, int64_t ldr, const float* dinv, float c, void* R16,
                          int64_t ldr16, void* W1, int64_t ldw1, int ncols, void* work, int64_t work_bytes, double* rn2,
                          double* xn2, ds_stream_t stream) {
    const bool pre = R16 != nullptr;
    DS_REQUIRE(ctab && gent && kgrp && mgrp && X && lam && (pre ? (W1 && dinv) : R != nullptr) && work && rn2 && xn2, "%s: null pointer", who);
    DS_REQUIRE(level_tag == 0 || (level_tag == 1 && !pre), "%s: level_tag must be 0 (fine)%s", who, pre ? "" : " or 1 (corner-node level)");
    if (int rc = check_union_shape(who, ngroups, cap_blocks, nnzb, nv, ncols)) return rc;
    uintptr_t al = reinterpret_cast<uintptr_t>(X) | (uintptr_t)(ldx * 4) | reinterpret_cast<uintptr_t>(kgrp) |
                   reinterpret_cast<uintptr_t>(ctab) | reinterpret_cast<uintptr_t>(work);
    if (pre) {
        DS_REQUIRE(ldx >= ncols && ldr16 >= ncols && ldw1 >= ncols, "%s: leading dimension smaller than ncols", who);
        DS_REQUIRE(R16 != W1 && R16 != X && W1 != X, "%s: X, R16 and W1 must be different buffers", who);
        DS_REQUIRE(ldx * 12 < (int64_t)PIPE_OOB && nv * 36 < (int64_t)PIPE_OOB && nnzb * 36 < ((int64_t)1 << 32),
                   "%s: operand beyond the descriptor range", who);
        const uintptr_t al8 = reinterpret_cast<uintptr_t>(R16) | reinterpret_cast<uintptr_t>(W1) | (uintptr_t)(ldr16 * 2) | (uintptr_t)(ldw1 * 2);
        DS_REQUIRE((al8 & 7) == 0 && (reinterpret_cast<uintptr_t>(dinv) & 3) == 0, "%s: bf16 rows must be 8-byte aligned", who);
    } else {
        DS_REQUIRE(ldx >= ncols && ldr >= ncols, "%s: leading dimension smaller than ncols", who);
        DS_REQUIRE(X != R, "%s: X and R must be different buffers", who);
        DS_REQUIRE(ldx * 12 < (int64_t)PIPE_OOB && ldr * 12 < (int64_t)PIPE_OOB && nnzb * 36 < ((int64_t)1 << 32),
                   "%s: operand beyond the descriptor range", who);
        al |= reinterpret_cast<uintptr_t>(R) | (uintptr_t)(ldr * 4);
    }
    DS_REQUIRE((al & 15) == 0, "%s: rows, kgrp, ctab and the workspace must be 16-byte aligned", who);
    DS_REQUIRE(work_bytes >= ds_union_residual_workspace_bytes(ngroups, ncols), "%s: workspace of %lld bytes needed", who,
               (long long)ds_union_residual_workspace_bytes(ngroups, ncols));
    hipStream_t st = ds::as_stream(stream);
    ChebEpilogue epi{nullptr, 0, pre ? dinv : nullptr, 0.f, pre ? c : 0.f, 0};
    epi.mvals = mgrp, epi.lam = lam, epi.nwork = static_cast<float*>(work);
    epi.w1 = W1, epi.ldw1 = ldw1;
    float* Y = pre ? static_cast<float*>(R16) : R;  // (epilogue 6: bf16 rows, leading dimension in elements)
    const int64_t ldy = pre ? ldr16 : ldr;
    const int lpn = ncols / 4;
    int rc;
    {
    ds::ProfScope prof(stream, DS_PROF_RESID, nv, nnzb, ncols, 4 << 8);  // (the walk of the unions; the two norm reductions follow)
#define DS_UR(L, E, V) rc = launch_union<L, E, false, true, V>(utab, ctab, ngroups, cap_blocks, gent, kgrp, nnzb, nv, X, ldx, Y, ldy, lpn, st, epi)
    if (lpn == 20) {
        if (pre) DS_UR(20, 6, 0);
        else if (level_tag == 1) DS_UR(20, 4, 1);
        else DS_UR(20, 4, 0);
    } else {
        if (pre) DS_UR(0, 6, 0);
        else if (level_tag == 1) DS_UR(0, 4, 1);
        else DS_UR(0, 4, 0);
    }
#undef DS_UR
    }
    if (rc != DS_OK) return rc;
    double* partial = reinterpret_cast<double*>(static_cast<char*>(work) + ngroups * 2 * (int64_t)ncols * 4);
    union_norm_partial_kernel<<<UN_NORM_BLOCKS, 256, 0, st>>>(static_cast<const float*>(work), (unsigned)ngroups, 2 * ncols, partial);
    DS_LAUNCH_CHECK("union_norm_partial_kernel");
    union_norm_final_kernel<<<(unsigned)(2 * ncols), 256, 0, st>>>(partial, ncols, rn2, xn2);
    DS_LAUNCH_CHECK("union_norm_final_kernel");
    return DS_OK;
}

extern "C" int ds_union_residual(int level_tag, const int32_t* utab, const int32_t* ctab, int64_t ngroups, int cap_blocks,
                                 const int32_t* gent, const float* kgrp, const float* mgrp, int64_t nnzb, int64_t nv,
                                 const float* X, int64_t ldx, const double* lam, float* R, int64_t ldr, int ncols, void* work,
                                 int64_t work_bytes, double* rn2, double* xn2, ds_stream_t stream) {
    return union_residual("ds_union_residual", level_tag, utab, ctab, ngroups, cap_blocks, gent, kgrp, mgrp, nnzb, nv, X, ldx, lam, R,
                          ldr, nullptr, 0.f, nullptr, 0, nullptr, 0, ncols, work, work_bytes, rn2, xn2, stream);
}

// The same walk for an iteration preconditioned by the bf16 two-level cycle (spmm_union.inc, epilogue 6): instead of the fp32
// R it writes the cycle's inputs - the bf16 copy R16 and the first Chebyshev iterate W1 = c T R - so that ds_twolevel_apply
// (DS_TL_PREPARED) starts at its first term.
extern "C" int ds_union_residual_pre(int level_tag, const int32_t* utab, const int32_t* ctab, int64_t ngroups, int cap_blocks,
                                     const int32_t* gent, const float* kgrp, const float* mgrp, int64_t nnzb, int64_t nv,
                                     const float* X, int64_t ldx, const double* lam, const float* dinv, float c, void* R16,
                                     int64_t ldr16, void* W1, int64_t ldw1, int ncols, void* work, int64_t work_bytes,
                                     double* rn2, double* xn2, ds_stream_t stream) {
    DS_REQUIRE(R16, "ds_union_residual_pre: null pointer");
    return union_residual("ds_union_residual_pre", level_tag, utab, ctab, ngroups, cap_blocks, gent, kgrp, mgrp, nnzb, nv, X, ldx, lam,
                          nullptr, 0, dinv, c, R16, ldr16, W1, ldw1, ncols, work, work_bytes, rn2, xn2, stream);
}

// Y = K X and Y2 = (M_s (x) I3) X of ONE block in one walk of the unions (spmm_union.inc, epilogue 5): the eigensolver's
// products of the raw preconditioned residuals W (round 5: Rayleigh-Ritz on the raw basis, csrc/lobpcg.cpp).
extern "C" int ds_spmm_union_km(int level_tag, const int32_t* utab, const int32_t* ctab, int64_t ngroups, int cap_blocks,
                                const int32_t* gent, const float* kgrp, const float* mgrp, int64_t nnzb, int64_t nv,
                                const float* X, int64_t ldx, float* KX, int64_t ldk, float* MX, int64_t ldm, int ncols,
                                ds_stream_t stream) {
    DS_REQUIRE(ctab && gent && kgrp && mgrp && X && KX && MX, "ds_spmm_union_km: null pointer");
    DS_REQUIRE(level_tag == 0 || level_tag == 1, "ds_spmm_union_km: level_tag must be 0 (fine) or 1 (corner-node level)");
    if (int rc = check_union_shape("ds_spmm_union_km", ngroups, cap_blocks, nnzb, nv, ncols)) return rc;
    DS_REQUIRE(ldx >= ncols && ldk >= ncols && ldm >= ncols, "ds_spmm_union_km: leading dimension smaller than ncols");
    DS_REQUIRE(X != KX && X != MX && KX != MX, "ds_spmm_union_km: X, KX and MX must be different buffers");
    DS_REQUIRE(ldx * 12 < (int64_t)PIPE_OOB && nnzb * 36 < ((int64_t)1 << 32), "ds_spmm_union_km: operand beyond the descriptor range");
    const uintptr_t al = reinterpret_cast<uintptr_t>(X) | reinterpret_cast<uintptr_t>(KX) | reinterpret_cast<uintptr_t>(MX) |
                         (uintptr_t)(ldx * 4) | (uintptr_t)(ldk * 4) | (uintptr_t)(ldm * 4) | reinterpret_cast<uintptr_t>(kgrp) |
                         reinterpret_cast<uintptr_t>(ctab);
    DS_REQUIRE((al & 15) == 0, "ds_spmm_union_km: rows, kgrp and ctab must be 16-byte aligned");
    hipStream_t st = ds::as_stream(stream);
    ChebEpilogue epi{nullptr, ldm, nullptr, 0.f, 0.f, 0};
    epi.mvals = mgrp, epi.nwork = MX;
    const int lpn = ncols / 4;
    ds::ProfScope prof(stream, DS_PROF_KM, nv, nnzb, ncols, 4 << 8);
#define DS_UKM(L, V) return launch_union<L, 5, false, true, V>(utab, ctab, ngroups, cap_blocks, gent, kgrp, nnzb, nv, X, ldx, KX, ldk, lpn, st, epi)
    if (lpn == 20) {
        if (level_tag == 1) DS_UKM(20, 1);
        DS_UKM(20, 0);
    }
    if (level_tag == 1) DS_UKM(0, 1);
    DS_UKM(0, 0);
#undef DS_UKM
}

// bf16-block form of the two preconditioner epilogues (the V-cycle's iterates are stored in bf16, arithmetic in fp32):
// X, R0, W_prev bf16; Y bf16, or fp32 when y_f32 (the last term of a cycle, written into the solver's basis buffer).
extern "C" int ds_spmm_union16(int epilogue, const int32_t* utab, const int32_t* ctab, int64_t ngroups, int cap_blocks,
                               const int32_t* gent, const float* kgrp, int64_t nnzb, int64_t nv, const void* X,
                               int64_t ldx, void* Y, int64_t ldy, int y_f32, const void* R0, int64_t ldr,
                               const float* dinv, int ncols, float c1, float c2, int first, const void* Wprev,
                               int64_t ldp, ds_stream_t stream) {
    DS_REQUIRE(ctab && gent && kgrp && X && Y && R0, "ds_spmm_union16: null pointer");
    DS_REQUIRE(epilogue == 1 || epilogue == 2, "ds_spmm_union16: epilogue must be 1 (Chebyshev term) or 2 (residual)");
    DS_REQUIRE(epilogue != 1 || dinv, "ds_spmm_union16: the Chebyshev epilogue needs dinv");
    if (int rc = check_union_shape("ds_spmm_union16", ngroups, cap_blocks, nnzb, nv, ncols)) return rc;
    DS_REQUIRE(ldx >= ncols && ldy >= ncols && ldr >= ncols, "ds_spmm_union16: leading dimension smaller than ncols");
    DS_REQUIRE(X != Y, "ds_spmm_union16: X and Y must be different buffers");
    // (the bf16 inputs go through buffer descriptors; the result is stored through plain 64-bit addresses)
    DS_REQUIRE(3 * nv * std::max(std::max(ldx, ldr), ldp) * 2 < (int64_t)PIPE_OOB && nv * 36 < (int64_t)PIPE_OOB,
               "ds_spmm_union16: a bf16 operand block of %lld bytes exceeds the descriptor range",
               (long long)(3 * nv * std::max(std::max(ldx, ldr), ldp) * 2));
    DS_REQUIRE(nnzb * 36 < ((int64_t)1 << 32), "ds_spmm_union16: value array exceeds the descriptor range");
    uintptr_t al = reinterpret_cast<uintptr_t>(X) | reinterpret_cast<uintptr_t>(R0) | (uintptr_t)(ldx * 2) | (uintptr_t)(ldr * 2);
    al |= reinterpret_cast<uintptr_t>(Y) | (uintptr_t)(ldy * (y_f32 ? 4 : 2));
    DS_REQUIRE((al & 7) == 0 && (!y_f32 || ((reinterpret_cast<uintptr_t>(Y) | (uintptr_t)(ldy * 4)) & 15) == 0) &&
                   ((reinterpret_cast<uintptr_t>(kgrp) | reinterpret_cast<uintptr_t>(ctab)) & 15) == 0,
               "ds_spmm_union16: bf16 rows must be 8-byte aligned (fp32 output rows, kgrp and ctab 16-byte)");
    hipStream_t st = ds::as_stream(stream);
    ChebEpilogue epi{static_cast<const float*>(R0), ldr, dinv, c1, c2, first};
    if (Wprev && epilogue == 1) {
        DS_REQUIRE(ldp >= ncols && ((reinterpret_cast<uintptr_t>(Wprev) | (uintptr_t)(ldp * 2)) & 7) == 0 && Wprev != X,
                   "ds_spmm_union16: bad W_prev block");
        epi.wprev = static_cast<const float*>(Wprev), epi.ldp = ldp;
    }
    DS_REQUIRE(!y_f32 || epilogue == 1, "ds_spmm_union16: an fp32 result is the Chebyshev term's only");
    const float* Xf = static_cast<const float*>(X);
    float* Yf = static_cast<float*>(Y);
    const int lpn = ncols / 4;
    // (the bf16-in / bf16-out term: the launch the benchmark's roofline figure is about)
    ds::ProfScope prof((epilogue == 1 && !y_f32) ? stream : nullptr, DS_PROF_TERM, nv, nnzb, ncols, (first ? 1 : 0) | (2 << 8));
#define DS_U16(L, E, O) return launch_union<L, E, true, O>(utab, ctab, ngroups, cap_blocks, gent, kgrp, nnzb, nv, Xf, ldx, Yf, ldy, lpn, st, epi)
    if (lpn == 20) {
        if (epilogue == 2) DS_U16(20, 2, false);
        if (y_f32) DS_U16(20, 1, true);
        DS_U16(20, 1, false);
    }
    if (epilogue == 2) DS_U16(0, 2, false);
    if (y_f32) DS_U16(0, 1, true);
    DS_U16(0, 1, false);
#undef DS_U16
}
