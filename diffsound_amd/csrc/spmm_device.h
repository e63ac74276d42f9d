// Device helpers shared by more than one SpMM translation unit (spmm.hip, spmm_union.hip with its .inc files,
// spmm_mfma.hip, spmm_mfma32.hip): vector types, the buffer-descriptor words, the bf16 pack / unpack, the non-temporal stream hints and
// the epilogue arguments.  What a single unit uses lives in that unit.  Self-contained: it may be a unit's first include.
#pragma once
#include "ds_common.h"

// (an anonymous namespace in a header, on purpose: ChebEpilogue is a kernel parameter, so its namespace is part of the
// kernels' mangled names - the names rocprofv3 tables and tests/test_cabi_cpu.py know; every helper is inlined)
namespace {

constexpr int PIPE_OOB = 0x7f000000;  // byte offset no block reaches: a load at it is answered with zeros, no request
// NON-TEMPORAL HINTS on what a wave touches once (round 5; A/B of four builds on one box, profiles/r05_nt_hint_ab.txt): result rows
// are STORED non-temporal on both levels (K W 182 -> 177 us, M W 149 -> 130, [K W | M W] 228 -> 224, fused residual 241 -> 236: the
// rows written no longer push the gathered panels, which the neighbouring groups re-use, out of the L2), and the value / table
// streams are LOADED non-temporal on the FINE level only (bf16 term 117 -> 112 us; with both hints K W 169, M W 129; the
// corner-node level re-reads its 7 MB of values 21 times per polynomial out of the L2 and loses 4 % with the hint).
#define DS_STREAM_LOAD(LVL_, p) ((LVL_) == 0 ? __builtin_nontemporal_load(p) : *(p))
#define DS_STREAM_STORE(p, v) __builtin_nontemporal_store(v, p)
// (the load half has one user, spmm_union.inc; it stays beside the store half and the measurement that covers both)

using f4v = __attribute__((ext_vector_type(4))) float;
using i4s = __attribute__((ext_vector_type(4))) int;
using f3v = __attribute__((ext_vector_type(3))) float;
// the four words of a raw buffer descriptor over [p, p + bytes): stride 0, offsets past `bytes` read as zero
__device__ __forceinline__ i4s make_rsrc_words(const void* p, unsigned bytes) {
    const uint64_t a = reinterpret_cast<uint64_t>(p);
    i4s r;
    r.x = __builtin_amdgcn_readfirstlane((int)(unsigned)a);
    r.y = __builtin_amdgcn_readfirstlane((int)((unsigned)(a >> 32) & 0xffffu));  // stride 0
    r.z = __builtin_amdgcn_readfirstlane((int)bytes);
    r.w = 0x00020000;
    // The words were written by v_readfirstlane (VALU -> SGPR); a VMEM instruction must not read such an SGPR within
    // 5 wait states, and the compiler cannot pad inline-asm loads.  Passing the words through this asm pins the
    // readfirstlanes BEFORE it (they cannot be re-materialised next to a later use) and pays the wait states once.
    asm volatile("s_nop 4" : "+s"(r));
    return r;
}
// bf16 storage of the preconditioner's iterates (the V-cycle is insensitive to 8-bit mantissas - same outer iteration
// counts - and its fused terms are bound by the bytes of the four vector streams): two bf16 per dword, fp32 arithmetic
using i2s = __attribute__((ext_vector_type(2))) int;
__device__ __forceinline__ f4v unpack_bf16x4(i2s w) {
    f4v r;
    r.x = __builtin_bit_cast(float, w.x << 16);
    r.y = __builtin_bit_cast(float, w.x & (int)0xffff0000);
    r.z = __builtin_bit_cast(float, w.y << 16);
    r.w = __builtin_bit_cast(float, w.y & (int)0xffff0000);
    return r;
}
__device__ __forceinline__ i2s pack_bf16x4(f4v v) {  // round to nearest even (v_cvt_pk_bf16_f32)
    using bf2 = __attribute__((ext_vector_type(2))) __bf16;
    using f2_ = __attribute__((ext_vector_type(2))) float;
    const bf2 lo = __builtin_convertvector(f2_{v.x, v.y}, bf2), hi = __builtin_convertvector(f2_{v.z, v.w}, bf2);
    return i2s{__builtin_bit_cast(int, lo), __builtin_bit_cast(int, hi)};
}

// Optional fused epilogue (EPI = 1, KIND 0, RS 3): one term of the Chebyshev block-Jacobi polynomial,
//   Y_i <- X_i + c1 (X_i - Y_i) + c2 T_i (R0_i - (K X)_i)        (Y holds W_{k-1} on entry, W_{k+1} on exit)
// so a preconditioner term is ONE launch and the product K X never goes to HBM.
struct ChebEpilogue {
    const float* r0;
    int64_t ldr;
    const float* dinv;
    float c1, c2;
    int first;  // W_{k-1} = 0: Y is not read
    // neighbour-union kernel only: W_{k-1} read from here instead of from Y (nullptr: from Y, the in-place form) - the
    // last term of a polynomial run on compact scratch blocks can then land in a column range of a wider buffer
    const float* wprev = nullptr;
    int64_t ldp = 0;
    // neighbour-union kernel, epilogue 4 (fused residual R = K X - (M X) diag(lam)): node-scalar mass values in group order,
    // the Ritz values (device, fp64, one per column) and the per-group partial column norms (ngroups x 2 x ncols floats)
    const float* mvals = nullptr;
    const double* lam = nullptr;
    float* nwork = nullptr;
    // neighbour-union kernel, epilogue 6 (the residual that hands the bf16 cycle its inputs): the first Chebyshev iterate
    // W1 = c2 T R as bf16 goes here (leading dimension in elements); the bf16 copy of R goes to Y
    void* w1 = nullptr;
    int64_t ldw1 = 0;
};

}  // namespace
