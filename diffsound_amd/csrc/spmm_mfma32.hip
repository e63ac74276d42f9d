// fp32 matrix-core form of the eigensolver's own products on the neighbour unions of 4-node groups: the kernel
// (spmm_mfma32.inc) and its entry point.  Exports ds_spmm_union32m (and ds_m32_diag in a DS_DIAG build).
#include "ds_diag.h"
#include "spmm_device.h"

namespace {
#include "spmm_mfma32.inc"
}  // namespace

#ifndef DS_MF32_BATCH
#define DS_MF32_BATCH 8
#endif
template <int NT, int EPI, int LVL>
static int launch_mfma32(const int32_t* gptr, const int32_t* gcol, const int32_t* gmeta, const int32_t* gbase, const float* vals,
                         unsigned vals_bytes, int64_t ngroups, int64_t nv, const float* X, int64_t ldx, float* Y, int64_t ldy,
                         int lpn, hipStream_t st) {
    constexpr int EB = DS_MF32_BATCH;
    constexpr int acap = ((EB * MF32_G * (EPI == 3 ? 4 : 36) + 1023) / 1024) * 1024;  // whole 1 KiB staging pieces
    const size_t lds = (size_t)mf32_panel_bytes(NT, EB) + acap + 48;
    spmm_union_mfma32_kernel<NT, EPI, EB, LVL><<<(unsigned)ngroups, 64, lds, st>>>(gptr, gcol, gmeta, gbase, vals, vals_bytes,
                                                                                  (unsigned)ngroups, nv, X, ldx, Y, ldy, lpn, acap);
    DS_LAUNCH_CHECK("spmm_union_mfma32_kernel");
    return DS_OK;
}

extern "C" int ds_spmm_union32m(int epilogue, int level_tag, const int32_t* gptr, const int32_t* gcol, const int32_t* gmeta,
                                const int32_t* gbase, const float* vals, int64_t vals_bytes, int64_t nblocks, int64_t ngroups,
                                int max_entries, int max_batch_blocks, int64_t nv, const float* X, int64_t ldx, float* Y,
                                int64_t ldy, int ncols, ds_stream_t stream) {
    DS_REQUIRE(gptr && gcol && gmeta && gbase && vals && X && Y, "ds_spmm_union32m: null pointer");
    DS_REQUIRE(epilogue == 0 || epilogue == 3, "ds_spmm_union32m: epilogue must be 0 (3x3 blocks) or 3 (node-scalar values)");
    DS_REQUIRE(level_tag == 0 || level_tag == 1, "ds_spmm_union32m: level_tag must be 0 (fine) or 1 (corner-node level)");
    DS_REQUIRE(nv > 0 && ngroups == (nv + MF32_G - 1) / MF32_G && ncols > 0 && ncols % 4 == 0 && ncols <= 84,
               "ds_spmm_union32m: ncols must be a multiple of 4 <= 84 and ngroups = ceil(nv / 4)");
    DS_REQUIRE(max_entries > 0 && max_entries <= 256, "ds_spmm_union32m: a group with %d union entries exceeds 256", max_entries);
    DS_REQUIRE(max_batch_blocks > 0 && max_batch_blocks <= DS_MF32_BATCH * MF32_G,
               "ds_spmm_union32m: max_batch_blocks must be in (0, DS_MF32_BATCH x 4]");
    const int64_t vb = epilogue == 3 ? 4 : 36;
    // (the value stream is read in 16-byte pieces: the array carries 16 bytes of slack behind its last block)
    DS_REQUIRE(nblocks > 0 && vals_bytes >= nblocks * vb + 16 && vals_bytes < (int64_t)PIPE_OOB,
               "ds_spmm_union32m: the value array must hold nblocks x %d bytes + 16 of slack, under the descriptor range", (int)vb);
    DS_REQUIRE(ldx >= ncols && ldy >= ncols, "ds_spmm_union32m: leading dimension smaller than ncols");
    DS_REQUIRE(X != Y, "ds_spmm_union32m: X and Y must be different buffers");
    DS_REQUIRE(3 * nv * ldx * 4 < (int64_t)PIPE_OOB, "ds_spmm_union32m: the operand block exceeds the descriptor range");
    const uintptr_t al = reinterpret_cast<uintptr_t>(X) | reinterpret_cast<uintptr_t>(Y) | (uintptr_t)(ldx * 4) | (uintptr_t)(ldy * 4);
    DS_REQUIRE((al & 15) == 0 && (reinterpret_cast<uintptr_t>(vals) & 3) == 0, "ds_spmm_union32m: rows must be 16-byte aligned");
    hipStream_t st = ds::as_stream(stream);
    const int lpn = ncols / 4, nt = (ncols + 15) / 16;
#define DS_M32_GO(N, E, L) return launch_mfma32<N, E, L>(gptr, gcol, gmeta, gbase, vals, (unsigned)vals_bytes, ngroups, nv, X, ldx, Y, ldy, lpn, st)
#define DS_M32_NT(E, L)                                                                     \
    switch (nt) {                                                                           \
        case 1: DS_M32_GO(1, E, L); case 2: DS_M32_GO(2, E, L); case 3: DS_M32_GO(3, E, L); \
        case 4: DS_M32_GO(4, E, L); case 5: DS_M32_GO(5, E, L); default: DS_M32_GO(6, E, L); \
    }
    if (epilogue == 0) {
        if (level_tag == 0) DS_M32_NT(0, 0)
        DS_M32_NT(0, 1)
    }
    if (level_tag == 0) DS_M32_NT(3, 0)
    DS_M32_NT(3, 1)
#undef DS_M32_NT
#undef DS_M32_GO
}

#ifdef DS_DIAG
extern "C" int ds_m32_diag(unsigned long long* out, int nwaves) {  // diagnostic build only: out[nwaves][8]
    return ds::check_hip(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_m32_dbg), (size_t)nwaves * 8 * sizeof(unsigned long long)), "ds_m32_diag read");
}
#endif
