// MFMA form of the preconditioner's bf16 terms on the neighbour unions of 8-node groups: the kernels (spmm_mfma.inc) and their
// entry points.  Exports ds_pack_kc, ds_spmm_union16m (and ds_mf_diag in a DS_DIAG build).
#include <algorithm>

#include "ds_diag.h"
#include "spmm_device.h"

namespace {
#include "spmm_mfma.inc"
}  // namespace

extern "C" int ds_pack_kc(const float* k32, const int32_t* kperm, int64_t nnzb, void* kc, ds_stream_t stream) {
    DS_REQUIRE(k32 && kperm && kc && nnzb > 0, "ds_pack_kc: bad argument");
    DS_REQUIRE((reinterpret_cast<uintptr_t>(kc) & 7) == 0, "ds_pack_kc: kc must be 8-byte aligned");
    pack_kc_kernel<<<(unsigned)ds::ceil_div(nnzb * 3, 256), 256, 0, ds::as_stream(stream)>>>(k32, kperm, nnzb,
                                                                                            static_cast<i2s*>(kc));
    DS_LAUNCH_CHECK("pack_kc_kernel");
    return DS_OK;
}

template <int G, int NT, int BATCH, int LVL, int TAIL>
static int launch_mfma(int epilogue, int y_f32, const int32_t* gptr, const int32_t* gcol, const int32_t* gmeta,
                       const int32_t* gbase, const int32_t* ghead, const void* kc, int64_t nnzb, int64_t ngroups, int64_t nv, const float* X,
                       int64_t ldx, float* Y, int64_t ldy, int lpn, int acap, hipStream_t st, const ChebEpilogue& epi) {
    const char* kcp = static_cast<const char*>(kc);
    const size_t lds = (size_t)mf_panel_bytes(lpn * 4, G, BATCH, TAIL) + (size_t)acap + 32;
    if (epilogue == 2)
        spmm_union_mfma_kernel<G, NT, 2, false, BATCH, LVL, TAIL><<<(unsigned)ngroups, 64, lds, st>>>(gptr, gcol, gmeta, gbase, ghead, kcp, nnzb, (unsigned)ngroups, nv, X, ldx, Y, ldy, lpn, acap, epi);
    else if (y_f32)
        spmm_union_mfma_kernel<G, NT, 1, true, BATCH, LVL, TAIL><<<(unsigned)ngroups, 64, lds, st>>>(gptr, gcol, gmeta, gbase, ghead, kcp, nnzb, (unsigned)ngroups, nv, X, ldx, Y, ldy, lpn, acap, epi);
    else
        spmm_union_mfma_kernel<G, NT, 1, false, BATCH, LVL, TAIL><<<(unsigned)ngroups, 64, lds, st>>>(gptr, gcol, gmeta, gbase, ghead, kcp, nnzb, (unsigned)ngroups, nv, X, ldx, Y, ldy, lpn, acap, epi);
    DS_LAUNCH_CHECK("spmm_union_mfma_kernel");
    return DS_OK;
}

// entries per batch on the corner-node level (level_tag 1): DS_MF_BATCH, or twice that (one wave's chain of dependent round
// trips is what a level with about as many groups as the device has wave slots is made of; measured at C3's corner level,
// 2 461 groups: see profiles/r04_corner_batch_ab.txt)
#ifndef DS_MF_CORNER_BATCH
#define DS_MF_CORNER_BATCH DS_MF_BATCH
#endif

extern "C" int ds_spmm_union16m(int epilogue, int group_nodes, int level_tag, const int32_t* gptr, const int32_t* gcol,
                                const int32_t* gmeta, const int32_t* gbase, const int32_t* ghead, const void* kc, int64_t nnzb,
                                int64_t ngroups, int max_entries, int max_batch_blocks, int64_t nv, const void* X,
                                int64_t ldx, void* Y,
                                int64_t ldy, int y_f32, const void* R0, int64_t ldr, const float* dinv, int ncols,
                                float c1, float c2, int first, const void* Wprev, int64_t ldp, ds_stream_t stream) {
    DS_REQUIRE(gptr && gcol && gmeta && gbase && ghead && kc && X && Y && R0, "ds_spmm_union16m: null pointer");
    DS_REQUIRE((reinterpret_cast<uintptr_t>(ghead) & 3) == 0 && ngroups * 512 < (int64_t)1 << 40, "ds_spmm_union16m: bad ghead");
    DS_REQUIRE(epilogue == 1 || epilogue == 2, "ds_spmm_union16m: epilogue must be 1 (Chebyshev term) or 2 (residual)");
    DS_REQUIRE(epilogue != 1 || dinv, "ds_spmm_union16m: the Chebyshev epilogue needs dinv");
    // (4-node groups were slower on both levels; only the 8-node kernel is built)
    DS_REQUIRE(group_nodes == 8, "ds_spmm_union16m: groups of 8 nodes");
    DS_REQUIRE(level_tag == 0 || level_tag == 1, "ds_spmm_union16m: level_tag must be 0 (fine) or 1 (corner-node level)");
    DS_REQUIRE(nv > 0 && ngroups == (nv + group_nodes - 1) / group_nodes && ncols > 0 && ncols % 4 == 0 && ncols <= 84,
               "ds_spmm_union16m: ncols must be a multiple of 4 <= 84 and ngroups = ceil(nv / group_nodes)");
    DS_REQUIRE(max_entries > 0 && max_entries <= 256, "ds_spmm_union16m: a group with %d union entries exceeds 256", max_entries);
    DS_REQUIRE(max_batch_blocks > 0 && max_batch_blocks <= DS_MF_BATCH * group_nodes,
               "ds_spmm_union16m: max_batch_blocks must be in (0, DS_MF_BATCH x group_nodes]");
    DS_REQUIRE(nnzb > 0 && nnzb * 24 < (int64_t)PIPE_OOB, "ds_spmm_union16m: the block array exceeds the descriptor range");
    DS_REQUIRE(ldx >= ncols && ldy >= ncols && ldr >= ncols, "ds_spmm_union16m: leading dimension smaller than ncols");
    DS_REQUIRE(X != Y, "ds_spmm_union16m: X and Y must be different buffers");
    DS_REQUIRE(3 * nv * std::max(std::max(ldx, ldr), ldp) * 2 < (int64_t)PIPE_OOB && nv * 36 < (int64_t)PIPE_OOB,
               "ds_spmm_union16m: a bf16 operand block exceeds the descriptor range");
    uintptr_t al = reinterpret_cast<uintptr_t>(X) | reinterpret_cast<uintptr_t>(R0) | (uintptr_t)(ldx * 2) | (uintptr_t)(ldr * 2);
    al |= reinterpret_cast<uintptr_t>(Y) | (uintptr_t)(ldy * (y_f32 ? 4 : 2)) | reinterpret_cast<uintptr_t>(kc);
    DS_REQUIRE((al & 7) == 0 && (!y_f32 || ((reinterpret_cast<uintptr_t>(Y) | (uintptr_t)(ldy * 4)) & 15) == 0),
               "ds_spmm_union16m: bf16 rows and kc must be 8-byte aligned (fp32 output rows 16-byte)");
    DS_REQUIRE(!y_f32 || epilogue == 1, "ds_spmm_union16m: an fp32 result is the Chebyshev term's only");
    hipStream_t st = ds::as_stream(stream);
    ChebEpilogue epi{static_cast<const float*>(R0), ldr, dinv, c1, c2, first};
    if (Wprev && epilogue == 1) {
        DS_REQUIRE(ldp >= ncols && ((reinterpret_cast<uintptr_t>(Wprev) | (uintptr_t)(ldp * 2)) & 7) == 0 && Wprev != X,
                   "ds_spmm_union16m: bad W_prev block");
        epi.wprev = static_cast<const float*>(Wprev), epi.ldp = ldp;
    }
    const float* Xf = static_cast<const float*>(X);
    float* Yf = static_cast<float*>(Y);
    const int lpn = ncols / 4;
    const int nt = (ncols + 15) / 16;
    // two batches of DS_MF_BATCH entries never hold more blocks than 2 x max_batch_blocks
    constexpr int CB = DS_MF_CORNER_BATCH;
    const int acap = ((max_batch_blocks * 24 + 1023) / 1024) * 1024;  // whole 1 KiB staging pieces
    const int acapc = (((CB / DS_MF_BATCH) * max_batch_blocks * 24 + 1023) / 1024) * 1024;
    // groups of at most 128 entries: the form whose last batch takes DS_MF_TAIL entries more (see spmm_mfma.inc)
    const bool tail = max_entries <= 128 && max_batch_blocks * 24 <= 2048;
    constexpr int CT = CB == DS_MF_BATCH ? DS_MF_TAIL : 0;
#define DS_MF_ARGS(ACAP) epilogue, y_f32, gptr, gcol, gmeta, gbase, ghead, kc, nnzb, ngroups, nv, Xf, ldx, Yf, ldy, lpn, ACAP, st, epi
    // (blocks of >= 49 columns only: with fewer accumulator tiles the compiler spills the tail form at three waves per SIMD)
#define DS_MF_GO(N) return tail ? launch_mfma<8, N, DS_MF_BATCH, 0, (N >= 4 ? DS_MF_TAIL : 0)>(DS_MF_ARGS(acap)) : launch_mfma<8, N, DS_MF_BATCH, 0, 0>(DS_MF_ARGS(acap))
#define DS_MF_GOC(N) return tail ? launch_mfma<8, N, CB, 1, (N >= 4 ? CT : 0)>(DS_MF_ARGS(acapc)) : launch_mfma<8, N, CB, 1, 0>(DS_MF_ARGS(acapc))
    auto go = [&]() -> int {
        if (level_tag == 1) {
            switch (nt) {
                case 1: DS_MF_GOC(1); case 2: DS_MF_GOC(2); case 3: DS_MF_GOC(3);
                case 4: DS_MF_GOC(4); case 5: DS_MF_GOC(5); default: DS_MF_GOC(6);
            }
        }
        switch (nt) {
            case 1: DS_MF_GO(1); case 2: DS_MF_GO(2); case 3: DS_MF_GO(3);
            case 4: DS_MF_GO(4); case 5: DS_MF_GO(5); default: DS_MF_GO(6);
        }
    };
#undef DS_MF_GO
#undef DS_MF_GOC
#undef DS_MF_ARGS
    ds::ProfScope prof((epilogue == 1 && !y_f32) ? stream : nullptr, DS_PROF_TERM, nv, nnzb, ncols, (first ? 1 : 0) | (2 << 8));
    return go();
}

#ifdef DS_DIAG
extern "C" int ds_mf_diag(unsigned long long* out, int nwaves) {  // the bf16 term kernel's records
    return ds::check_hip(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_mf_dbg), (size_t)nwaves * 8 * sizeof(unsigned long long)), "ds_mf_diag read");
}
#endif
