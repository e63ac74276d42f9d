// Internal helpers shared by the translation units of libdiffsound_hip.so.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>

#include "diffsound_hip.h"

namespace ds {

void set_error(const char* fmt, ...);

inline int check_hip(hipError_t e, const char* what) {
    if (e == hipSuccess) return DS_OK;
    set_error("%s: %s", what, hipGetErrorString(e));
    return DS_ERR_HIP;
}

inline hipStream_t as_stream(ds_stream_t s) { return reinterpret_cast<hipStream_t>(s); }

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// p is a multiple of a (a power of two); a null pointer is aligned
inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// Workgroups are dealt round-robin over the 8 XCDs (blocks b and b+8 share one L2).  Give each
// XCD a contiguous slice of the logical work list so neighbouring rows share an L2 (bijective for
// any grid size).  Speed only, never correctness.
__device__ __forceinline__ unsigned xcd_remap(unsigned bid, unsigned nblk) {
    const unsigned q = nblk >> 3, r = nblk & 7u;
    const unsigned xcd = bid & 7u, idx = bid >> 3;
    const unsigned base = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return base + idx;
}

// Sum of v over the 64 lanes of a wavefront, in every lane (xor butterfly: the same bits in all of them).
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// One row of the first Chebyshev iterate W1 = c T R of the block-Jacobi polynomial: c (da r0 + db r1 + dc r2) on a lane's four
// columns, (da, db, dc) the row of the node's 3 x 3 block T.  cheb_init16_kernel (precond16.hip) and the residual walk that
// hands the cycle its inputs (spmm_union.inc, epilogue 6) both call it and must agree to the last bit, so the multiply-adds are
// spelled out - db r1 first, then the r0 and r2 terms fused onto it, which is how the compiler contracted the plain expression
// in cheb_init16_kernel - and nothing is left for the compiler to contract one way here and another way there.
using f32x4 = __attribute__((ext_vector_type(4))) float;
__device__ __forceinline__ f32x4 cheb_first_row(float c, float da, float db, float dc, f32x4 r0, f32x4 r1, f32x4 r2) {
    f32x4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = c * __builtin_fmaf(dc, r2[k], __builtin_fmaf(da, r0[k], db * r1[k]));
    return o;
}

// Launch timing hook (include/diffsound_hip.h: ds_profile_stream / ds_profile_kinds / ds_profile_collect).  A scope brackets
// the launches issued inside it with HIP events when `stream` is the registered one and `kind` is enabled - else it does
// nothing (one relaxed load).  Kinds: DS_PROF_* of the public header; (a, b, c, d) = the launch's shape as that header lists.
struct ProfScope {
    ProfScope(ds_stream_t stream, int kind, int64_t a, int64_t b, int c, int d);
    ~ProfScope();
    ProfScope(const ProfScope&) = delete;
    ProfScope& operator=(const ProfScope&) = delete;
    void* rec_ = nullptr;
    hipStream_t st_ = nullptr;
};

}  // namespace ds

#define DS_REQUIRE(cond, ...)            \
    do {                                 \
        if (!(cond)) {                   \
            ds::set_error(__VA_ARGS__);  \
            return DS_ERR_ARG;           \
        }                                \
    } while (0)

// the check behind a launch, as a value (for a launch that is the last thing a function or a lambda does) and as a statement
#define DS_LAUNCHED(name) ds::check_hip(hipGetLastError(), name " launch")

#define DS_LAUNCH_CHECK(name)            \
    do {                                 \
        int _rc = DS_LAUNCHED(name);     \
        if (_rc != DS_OK) return _rc;    \
    } while (0)
