// Block SpMM  Y = A X  on the BSR-3 node pattern - gfx950.  The HBM-roofline kernel of the path.
//
// Replaces torch.sparse.mm(A, X) of the reference (src/lobpcg/_linalg_utils.py:36-37; also
// src/diffelastic/diff_model.py:385, 395-397) where A is a scalar COO matrix.  Exploits what the
// reference's matrices guarantee: K is made of full 3x3 node blocks and M = M_s (x) I3, so the
// index stream shrinks 9x (one int32 per block) and M needs one scalar per block.
//
// Mapping: X, Y are row-major (3 nv x ncols).  A group of LPN = ceil(ncols/VEC) lanes owns one
// node (3 rows of Y); each lane owns VEC consecutive columns, so every X access is a contiguous
// 16-byte (f32) load and a wave reads whole 3-row panels of a neighbour node (coalesced).  64/LPN
// node groups share a wave.  Block values are fetched by all lanes of a group from the same
// address (hardware broadcast).  Accumulation in registers, one store per output element.
// Algorithmic bytes per launch: nnzb*(vals + 4) + (nv+1)*4 + 2*3nv*ncols*sizeof(T).
//
// This unit: the row-wise family - the generic lane-per-columns kernel (spmm_bsr3_kernel), the wave-per-node fast path of the
// fp32 products with its fused Chebyshev / residual epilogues (spmm_wave_node_kernel) and the wave-per-node fp64-value kernel
// that ds_spmm_bsr3 dispatches to (spmm_f64_node_kernel).  Exports ds_spmm_bsr3, ds_cheb_spmm, ds_spmm_residual.  The other
// families are units of their own: the neighbour-union walk (spmm_union.hip), the read-out's and the refinement's fp64-value
// products (spmm_f64.hip), the matrix-core forms (spmm_mfma.hip, spmm_mfma32.hip); the launch timing hook is profile.cpp.
#include <cstdint>

#include "spmm_device.h"

namespace {

template <typename T, int V>
struct Vec;
template <>
struct Vec<float, 4> {
    using type = float4;
};
template <>
struct Vec<float, 2> {
    using type = float2;
};
template <>
struct Vec<double, 2> {
    using type = double2;
};

// KIND: 0 = 3x3 blocks, 1 = scalar (x I3).  TV value type, TX input type, TY output/accumulator.
// LPN_CT: lanes per node known at compile time (0 = run-time value).  The solver's block widths
// (b = 72/80 columns and 3b) get their own instantiations: the lane->(node, column) split becomes
// constant arithmetic, and rocprofv3 reports those launches under their own kernel names.
template <int KIND, typename TV, typename TX, typename TY, int VEC, int LPN_CT>
__global__ void __launch_bounds__(256)
    spmm_bsr3_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colidx,
                     const TV* __restrict__ vals, int64_t nv, const TX* __restrict__ X, int64_t ldx,
                     TY* __restrict__ Y, int64_t ldy, int ncols, int lpn_rt, int npw_rt, unsigned nblk) {
    const int lpn = LPN_CT ? LPN_CT : lpn_rt;
    const int npw = LPN_CT ? 64 / LPN_CT : npw_rt;
    const unsigned bid = ds::xcd_remap(blockIdx.x, nblk);
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int sub = lane / lpn;
    const int cl = lane - sub * lpn;
    const int64_t node = ((int64_t)bid * 4 + wave) * npw + sub;
    const int c0 = cl * VEC;
    if (sub >= npw || node >= nv || c0 >= ncols) return;
    // ncols is a multiple of VEC (checked on the host), so a lane is either fully in or out
    TY acc[3][VEC];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[r][v] = (TY)0;

    const int kb = rowptr[node], ke = rowptr[node + 1];
    using XV = typename Vec<TX, VEC>::type;
#pragma unroll 2
    for (int k = kb; k < ke; ++k) {
        const int64_t col = colidx[k];
        const TX* xp = X + (col * 3) * ldx + c0;
        const XV x0 = *reinterpret_cast<const XV*>(xp);
        const XV x1 = *reinterpret_cast<const XV*>(xp + ldx);
        const XV x2 = *reinterpret_cast<const XV*>(xp + 2 * ldx);
        const TX* x0p = reinterpret_cast<const TX*>(&x0);
        const TX* x1p = reinterpret_cast<const TX*>(&x1);
        const TX* x2p = reinterpret_cast<const TX*>(&x2);
        if (KIND == 0) {
            const TV* a = vals + (int64_t)k * 9;
            TY av[9];
#pragma unroll
            for (int q = 0; q < 9; ++q) av[q] = (TY)a[q];
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                const TY xa = (TY)x0p[v], xb = (TY)x1p[v], xc = (TY)x2p[v];
#pragma unroll
                for (int r = 0; r < 3; ++r)
                    acc[r][v] = fma(av[r * 3 + 0], xa, fma(av[r * 3 + 1], xb, fma(av[r * 3 + 2], xc, acc[r][v])));
            }
        } else {
            const TY m = (TY)vals[k];
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                acc[0][v] = fma(m, (TY)x0p[v], acc[0][v]);
                acc[1][v] = fma(m, (TY)x1p[v], acc[1][v]);
                acc[2][v] = fma(m, (TY)x2p[v], acc[2][v]);
            }
        }
    }
    using YV = typename Vec<TY, VEC>::type;
    TY* yp = Y + (node * 3) * ldy + c0;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        YV o;
        TY* op = reinterpret_cast<TY*>(&o);
#pragma unroll
        for (int v = 0; v < VEC; ++v) op[v] = acc[r][v];
        *reinterpret_cast<YV*>(yp + r * ldy) = o;
    }
}

template <int KIND, typename TV, typename TX, typename TY, int VEC, int LPN_CT>
int launch_ct(const int32_t* rowptr, const int32_t* colidx, const void* vals, int64_t nv, const void* X, int64_t ldx,
              void* Y, int64_t ldy, int ncols, int lpn, hipStream_t st) {
    const int npw = 64 / lpn;  // nodes per wave
    const int64_t nblk = ds::ceil_div(nv, (int64_t)npw * 4);
    spmm_bsr3_kernel<KIND, TV, TX, TY, VEC, LPN_CT><<<(unsigned)nblk, 256, 0, st>>>(
        rowptr, colidx, static_cast<const TV*>(vals), nv, static_cast<const TX*>(X), ldx, static_cast<TY*>(Y), ldy,
        ncols, lpn, npw, (unsigned)nblk);
    DS_LAUNCH_CHECK("spmm_bsr3_kernel");
    return DS_OK;
}

template <int KIND, typename TV, typename TX, typename TY, int VEC>
int launch(const int32_t* rowptr, const int32_t* colidx, const void* vals, int64_t nv, const void* X, int64_t ldx,
           void* Y, int64_t ldy, int ncols, hipStream_t st) {
    const int lpn = (ncols + VEC - 1) / VEC;  // lanes per node
    if (KIND == 0 && VEC == 4) {              // the eigensolver's stiffness products
        switch (lpn) {
            case 18: return launch_ct<KIND, TV, TX, TY, VEC, 18>(rowptr, colidx, vals, nv, X, ldx, Y, ldy, ncols, lpn, st);
            case 20: return launch_ct<KIND, TV, TX, TY, VEC, 20>(rowptr, colidx, vals, nv, X, ldx, Y, ldy, ncols, lpn, st);
            case 54: return launch_ct<KIND, TV, TX, TY, VEC, 54>(rowptr, colidx, vals, nv, X, ldx, Y, ldy, ncols, lpn, st);
            case 60: return launch_ct<KIND, TV, TX, TY, VEC, 60>(rowptr, colidx, vals, nv, X, ldx, Y, ldy, ncols, lpn, st);
            default: break;
        }
    }
    return launch_ct<KIND, TV, TX, TY, VEC, 0>(rowptr, colidx, vals, nv, X, ldx, Y, ldy, ncols, lpn, st);
}

// ------------------------------------------------------------------------------------------------
// Fast path for the f32 products of the eigensolver: ONE WAVE PER NODE, block metadata on the scalar
// path.  The node index is wave-uniform, so rowptr / colidx / the 3x3 values come through s_load
// (scalar cache, no vector-memory instructions, no dependent vector round trip before the X loads).
// RS = 3 (ncols <= 84): lane (cl, r) loads the 16 bytes [cl*4, cl*4+4) of input row r of the
//   neighbour, i.e. ONE 16-byte load instruction per block fetches the whole 3 x ncols panel; each
//   lane accumulates its row's contribution to all three output rows and the three lane groups are
//   merged by two cross-lane shuffles at the end (KIND 1, M = M_s (x) I3, needs no merge: row r only
//   feeds row r).
// RS = 1 (ncols <= 256): lane cl loads its 16 bytes of all three rows (three loads per block).
// Row metadata is fetched COOPERATIVELY once per row: lane l loads neighbour id l of the row (one
// coalesced load) and the row's 3x3 values stream into a per-wave LDS slab with coalesced loads; per
// block, the id comes back with v_readlane (scalar address arithmetic) and the coefficients with LDS
// broadcast reads.  The vector-memory pipe then carries only the X panels.  (Two earlier versions:
// s_load per block -> nine dependent scalar round trips per four blocks; per-lane vector loads of the
// coefficients -> 720 redundant bytes per block through the texture-addresser, as much as the X panel.
// Both sat at 1.3 TB/s.)
constexpr int WN_CHUNK = 64;  // blocks of a row staged per pass

// X panels are fetched with buffer loads: the lane's byte offset inside a 3-row panel is loop-invariant
// (voffset) and the neighbour's panel start is a wave-uniform scalar (soffset = id * panel bytes), so the
// per-block address arithmetic is one s_mul_i32 instead of a 64-bit multiply-add per lane.
__device__ __forceinline__ f4v buf_load4(__amdgpu_buffer_rsrc_t rsrc, int voff, int soff) {
    return __builtin_bit_cast(f4v, __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff, soff, 0));
}

template <int KIND, int RS, int LPN_CT, int EPI>
__global__ void __launch_bounds__(256)
    spmm_wave_node_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colidx,
                          const float* __restrict__ vals, const float* __restrict__ vals_t, int64_t nv,
                          const float* __restrict__ X, int64_t ldx, float* __restrict__ Y, int64_t ldy, int lpn_rt,
                          unsigned nblk, ChebEpilogue epi, int big) {
    using f4 = __attribute__((ext_vector_type(4))) float;
    __shared__ float s_vals[4][WN_CHUNK * 9];
    const int lpn = LPN_CT ? LPN_CT : lpn_rt;
    const unsigned bid = ds::xcd_remap(blockIdx.x, nblk);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t node = (int64_t)bid * 4 + wave;
    if (node >= nv) return;  // wave-uniform
    const int r_raw = RS == 3 ? lane / lpn : 0;
    const int cl_raw = lane - r_raw * lpn;
    const bool active = r_raw < RS && cl_raw < lpn;
    // idle lanes shadow a valid lane (no exec-mask branches inside the loop); they never store
    const int r = active ? r_raw : 0;
    const int cl = active ? cl_raw : 0;
    const int c0 = cl * 4;
    const float* xbase = X + (int64_t)r * ldx + c0;
    const int64_t ldx3 = 3 * ldx;
    // whole X block as one buffer (host guarantees 3 nv ldx 4 < 2^32)
    const __amdgpu_buffer_rsrc_t xrsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(X), 0, big ? 0 : (int)(unsigned)(3 * nv * ldx * 4), 0x00020000);
    const int xvoff = (int)(((int64_t)r * ldx + c0) * 4);
    const int panel_bytes = (int)(ldx3 * 4);
    const int kb = rowptr[node], ke = rowptr[node + 1];
    float* sv = s_vals[wave];
    f4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = acc0, acc2 = acc0;
    for (int kc = kb; kc < ke; kc += WN_CHUNK) {
        const int cnt = min(WN_CHUNK, ke - kc);  // wave-uniform
        const int colreg = lane < cnt ? colidx[kc + lane] : 0;
        float mreg = 0.f;
        if (KIND == 1) {
            mreg = lane < cnt ? vals[kc + lane] : 0.f;
        } else if (RS == 3) {
            const float* vsrc = vals + (int64_t)kc * 9;
            for (int t = lane; t < cnt * 9; t += 64) sv[t] = vsrc[t];
            // same-wave LDS write -> read: order them without a workgroup barrier (rows differ in length)
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
        int u = 0;
        // UX panel loads in flight per wave before the first use: the kernel is latency-bound (72 % of wave
        // cycles parked in s_waitcnt with 4 in flight), so depth, not bandwidth, is what to raise
        constexpr int UX = RS == 3 ? 8 : 4;
        for (; u + UX <= cnt; u += UX) {
            f4 xa[UX], xb[UX], xc[UX];
#pragma unroll
            for (int q = 0; q < UX; ++q) {
                const int j = __builtin_amdgcn_readlane(colreg, u + q);
                if (!big) {  // wave-uniform: blocks under 4 GiB go through the buffer descriptor
                    const int soff = j * panel_bytes;
                    xa[q] = buf_load4(xrsrc, xvoff, soff);
                    if (RS == 1) {
                        xb[q] = buf_load4(xrsrc, xvoff + (int)(ldx * 4), soff);
                        xc[q] = buf_load4(xrsrc, xvoff + (int)(ldx * 8), soff);
                    }
                } else {
                    const float* p = xbase + (int64_t)j * ldx3;
                    xa[q] = *reinterpret_cast<const f4*>(p);
                    if (RS == 1) {
                        xb[q] = *reinterpret_cast<const f4*>(p + ldx);
                        xc[q] = *reinterpret_cast<const f4*>(p + 2 * ldx);
                    }
                }
            }
#pragma unroll
            for (int q = 0; q < UX; ++q) {
                if (KIND == 1) {
                    const float m = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, mreg), u + q));
                    acc0 += m * xa[q];
                    if (RS == 1) {
                        acc1 += m * xb[q];
                        acc2 += m * xc[q];
                    }
                } else if (RS == 3) {
                    const float* a = sv + (u + q) * 9 + r;  // column r of the block
                    acc0 += a[0] * xa[q];
                    acc1 += a[3] * xa[q];
                    acc2 += a[6] * xa[q];
                } else {
                    const float* a = vals + (int64_t)(kc + u + q) * 9;  // same address in every lane: one request
                    acc0 += a[0] * xa[q] + a[1] * xb[q] + a[2] * xc[q];
                    acc1 += a[3] * xa[q] + a[4] * xb[q] + a[5] * xc[q];
                    acc2 += a[6] * xa[q] + a[7] * xb[q] + a[8] * xc[q];
                }
            }
        }
        for (; u < cnt; ++u) {
            const int j = __builtin_amdgcn_readlane(colreg, u);
            const float* p = xbase + (int64_t)j * ldx3;
            const f4 x0 = *reinterpret_cast<const f4*>(p);
            if (KIND == 1) {
                const float m = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, mreg), u));
                acc0 += m * x0;
                if (RS == 1) {
                    acc1 += m * *reinterpret_cast<const f4*>(p + ldx);
                    acc2 += m * *reinterpret_cast<const f4*>(p + 2 * ldx);
                }
            } else if (RS == 3) {
                const float* a = sv + u * 9 + r;
                acc0 += a[0] * x0;
                acc1 += a[3] * x0;
                acc2 += a[6] * x0;
            } else {
                const float* a = vals + (int64_t)(kc + u) * 9;
                const f4 x1 = *reinterpret_cast<const f4*>(p + ldx);
                const f4 x2 = *reinterpret_cast<const f4*>(p + 2 * ldx);
                acc0 += a[0] * x0 + a[1] * x1 + a[2] * x2;
                acc1 += a[3] * x0 + a[4] * x1 + a[5] * x2;
                acc2 += a[6] * x0 + a[7] * x1 + a[8] * x2;
            }
        }
        if (KIND == 0 && RS == 3 && kc + WN_CHUNK < ke) {  // the slab is rewritten by the next pass
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
    }
    if (RS == 3 && KIND == 0) {
        // merge the three row groups: lanes [0,lpn) += lanes [lpn,2lpn) + lanes [2lpn,3lpn)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            acc0[v] += __shfl(acc0[v], lane + lpn) + __shfl(acc0[v], lane + 2 * lpn);
            acc1[v] += __shfl(acc1[v], lane + lpn) + __shfl(acc1[v], lane + 2 * lpn);
            acc2[v] += __shfl(acc2[v], lane + lpn) + __shfl(acc2[v], lane + 2 * lpn);
        }
    }
    float* yp = Y + (node * 3) * ldy + c0;
    if (EPI == 1) {
        if (active && r_raw == 0) {
            const float* rp = epi.r0 + (node * 3) * epi.ldr + c0;
            const float* xp = X + (node * 3) * ldx + c0;
            const float* d = epi.dinv + node * 9;
            const f4 q0 = *reinterpret_cast<const f4*>(rp) - acc0;
            const f4 q1 = *reinterpret_cast<const f4*>(rp + epi.ldr) - acc1;
            const f4 q2 = *reinterpret_cast<const f4*>(rp + 2 * epi.ldr) - acc2;
            const f4 t0 = d[0] * q0 + d[1] * q1 + d[2] * q2;
            const f4 t1 = d[3] * q0 + d[4] * q1 + d[5] * q2;
            const f4 t2 = d[6] * q0 + d[7] * q1 + d[8] * q2;
            const f4 w0 = *reinterpret_cast<const f4*>(xp);
            const f4 w1 = *reinterpret_cast<const f4*>(xp + ldx);
            const f4 w2 = *reinterpret_cast<const f4*>(xp + 2 * ldx);
            f4 o0 = w0 + epi.c2 * t0, o1 = w1 + epi.c2 * t1, o2 = w2 + epi.c2 * t2;
            if (!epi.first) {
                o0 += epi.c1 * (w0 - *reinterpret_cast<const f4*>(yp));
                o1 += epi.c1 * (w1 - *reinterpret_cast<const f4*>(yp + ldy));
                o2 += epi.c1 * (w2 - *reinterpret_cast<const f4*>(yp + 2 * ldy));
            } else {  // W_prev = 0 (not read)
                o0 += epi.c1 * w0;
                o1 += epi.c1 * w1;
                o2 += epi.c1 * w2;
            }
            *reinterpret_cast<f4*>(yp) = o0;
            *reinterpret_cast<f4*>(yp + ldy) = o1;
            *reinterpret_cast<f4*>(yp + 2 * ldy) = o2;
        }
    } else if (EPI == 2) {  // Y = R0 - K X (block residual feeding the coarse-level restriction)
        if (active && r_raw == 0) {
            const float* rp = epi.r0 + (node * 3) * epi.ldr + c0;
            *reinterpret_cast<f4*>(yp) = *reinterpret_cast<const f4*>(rp) - acc0;
            *reinterpret_cast<f4*>(yp + ldy) = *reinterpret_cast<const f4*>(rp + epi.ldr) - acc1;
            *reinterpret_cast<f4*>(yp + 2 * ldy) = *reinterpret_cast<const f4*>(rp + 2 * epi.ldr) - acc2;
        }
    } else if (RS == 3 && KIND == 1) {
        if (active) *reinterpret_cast<f4*>(yp + (int64_t)r * ldy) = acc0;
    } else if (active && r_raw == 0) {
        *reinterpret_cast<f4*>(yp) = acc0;
        *reinterpret_cast<f4*>(yp + ldy) = acc1;
        *reinterpret_cast<f4*>(yp + 2 * ldy) = acc2;
    }
}

template <int KIND, int RS, int LPN_CT, int EPI = 0>
int launch_wn(const int32_t* rowptr, const int32_t* colidx, const void* vals, const void* vals_t, int64_t nv,
              const void* X, int64_t ldx, void* Y, int64_t ldy, int lpn, hipStream_t st,
              ChebEpilogue epi = ChebEpilogue{nullptr, 0, nullptr, 0.f, 0.f, 0}) {
    const int64_t nblk = ds::ceil_div(nv, 4);
    spmm_wave_node_kernel<KIND, RS, LPN_CT, EPI><<<(unsigned)nblk, 256, 0, st>>>(
        rowptr, colidx, static_cast<const float*>(vals), static_cast<const float*>(vals_t), nv,
        static_cast<const float*>(X), ldx, static_cast<float*>(Y), ldy, lpn, (unsigned)nblk, epi,
        (3 * nv * ldx * 4 >= ((int64_t)1 << 32)) ? 1 : 0);
    DS_LAUNCH_CHECK("spmm_wave_node_kernel");
    return DS_OK;
}

template <int KIND>
int launch_fast(const int32_t* rowptr, const int32_t* colidx, const void* vals, const void* vals_t, int64_t nv,
                const void* X, int64_t ldx, void* Y, int64_t ldy, int ncols, hipStream_t st) {
    const int lpn = ncols / 4;
    if (lpn <= 21) {
        switch (lpn) {  // the solver's block widths get compile-time lane splits and their own kernel names
            case 18: return launch_wn<KIND, 3, 18>(rowptr, colidx, vals, vals_t, nv, X, ldx, Y, ldy, lpn, st);
            case 20: return launch_wn<KIND, 3, 20>(rowptr, colidx, vals, vals_t, nv, X, ldx, Y, ldy, lpn, st);
            default: return launch_wn<KIND, 3, 0>(rowptr, colidx, vals, vals_t, nv, X, ldx, Y, ldy, lpn, st);
        }
    }
    switch (lpn) {
        case 54: return launch_wn<KIND, 1, 54>(rowptr, colidx, vals, vals_t, nv, X, ldx, Y, ldy, lpn, st);
        case 60: return launch_wn<KIND, 1, 60>(rowptr, colidx, vals, vals_t, nv, X, ldx, Y, ldy, lpn, st);
        default: return launch_wn<KIND, 1, 0>(rowptr, colidx, vals, vals_t, nv, X, ldx, Y, ldy, lpn, st);
    }
}

// ------------------------------------------------------------------------------------------------
// fp64-value products of the read-out (X^T K_lambda X, X^T K_mu X, X^T M X on the converged block: kinds 2 / 3,
// fp64 values and result, fp32 X) for <= 84 columns: ONE WAVEFRONT PER NODE in the lane layout of the fp32
// kernels above - lane (g, cl) loads 16 bytes of row g of every neighbour panel and, for 3x3 blocks, column g of
// the block (3 doubles), accumulates its share of all three output rows in fp64 and the three lane groups are
// merged at the end.  The generic kernel above gives a lane 2 columns of one node and makes it load all 9 values
// of every block itself: 12 dependent-address loads per block and lane, 1.17 ms per 64-column product on the
// benchmark mesh; this one issues 4.
// (round 4: the row's fp64 coefficients are staged per chunk in LDS with coalesced loads and the neighbour ids come back with
// v_readlane, as in spmm_f64_polish_kernel (spmm_f64.hip) - three dependent-address global loads per block and lane fewer; same sums in
// the same order)
constexpr int F64_CHUNK = 32;  // blocks of a row staged per pass
constexpr int F64_WIN = 8;     // neighbour panels in flight per wave
template <int KIND, typename TX>
__global__ void __launch_bounds__(256)
    spmm_f64_node_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colidx,
                         const double* __restrict__ vals, int64_t nv, const TX* __restrict__ X, int64_t ldx,
                         double* __restrict__ Y, int64_t ldy, int lpn, unsigned nblk) {
    using d2 = __attribute__((ext_vector_type(2))) double;
    using xv4 = __attribute__((ext_vector_type(4))) TX;  // 16 bytes of an f32 row, 32 bytes of an f64 row
    __shared__ double s_v[4][F64_CHUNK * (KIND == 0 ? 9 : 1)];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t node = (int64_t)ds::xcd_remap(blockIdx.x, nblk) * 4 + wave;
    if (node >= nv) return;  // wave-uniform
    const int g = lane / lpn, cl = lane - g * lpn;
    const bool active = g < 3;
    const int ga = active ? g : 0;
    const int kb = __builtin_amdgcn_readfirstlane(rowptr[node]), ke = __builtin_amdgcn_readfirstlane(rowptr[node + 1]);
    const TX* xb = X + (int64_t)ga * ldx + cl * 4;
    double* sv = s_v[wave];
    double acc[3][4];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int v = 0; v < 4; ++v) acc[r][v] = 0.0;
    if (KIND == 1) {  // node scalars: index and value of a block are wave-uniform loads (the scalar path): nothing to stage
#pragma unroll 4
        for (int k = kb; k < ke; ++k) {
            const int64_t col = colidx[k];
            const xv4 x = *reinterpret_cast<const xv4*>(xb + col * 3 * ldx);
            const double m = vals[k];
#pragma unroll
            for (int v = 0; v < 4; ++v) acc[0][v] = fma(m, (double)x[v], acc[0][v]);  // m I3: row g feeds row g only
        }
    } else {
        for (int kc = kb; kc < ke; kc += F64_CHUNK) {
            const int cnt = min(F64_CHUNK, ke - kc);  // wave-uniform
            const int colreg = colidx[kc + min(lane, cnt - 1)];
            const double* pv = vals + (int64_t)kc * 9;
            // (all the chunk's coefficient loads in flight at once, clamped instead of predicated: a loop of one load per
            // trip met every load with a full wait)
            constexpr int NSL = (F64_CHUNK * 9 + 63) / 64;
            double stg[NSL];
#pragma unroll
            for (int i = 0; i < NSL; ++i) stg[i] = __builtin_nontemporal_load(pv + min(lane + 64 * i, cnt * 9 - 1));  // (read once: spmm_union.inc)
#pragma unroll
            for (int i = 0; i < NSL; ++i)
                if (lane + 64 * i < cnt * 9) sv[lane + 64 * i] = stg[i];
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            // The gathers of F64_WIN neighbour panels are in flight before the first of them is used (the loop used to
            // issue one and wait for it: every block of a row paid a full L2 round trip).  Slots past the chunk's last
            // block re-read it and are skipped; the sums and their order are unchanged.
            for (int u0 = 0; u0 < cnt; u0 += F64_WIN) {
                xv4 xs[F64_WIN];
#pragma unroll
                for (int j = 0; j < F64_WIN; ++j) {
                    const int64_t col = __builtin_amdgcn_readlane(colreg, min(u0 + j, cnt - 1));
                    xs[j] = *reinterpret_cast<const xv4*>(xb + col * 3 * ldx);
                }
#pragma unroll
                for (int j = 0; j < F64_WIN; ++j) {
                    if (u0 + j < cnt) {  // wave-uniform
                        const double* a = sv + (u0 + j) * 9 + ga;  // column g of the block
                        const double a0 = a[0], a1 = a[3], a2 = a[6];
#pragma unroll
                        for (int v = 0; v < 4; ++v) {
                            const double xv = (double)xs[j][v];
                            acc[0][v] = fma(a0, xv, acc[0][v]);
                            acc[1][v] = fma(a1, xv, acc[1][v]);
                            acc[2][v] = fma(a2, xv, acc[2][v]);
                        }
                    }
                }
            }
            if (kc + F64_CHUNK < ke) {  // the slab is rewritten by the next pass
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
            }
        }
    }
    double out[4];
    if (KIND == 0) {
        // lane (g, cl) ends with output row g: its own share plus the shares of the two other groups, which send
        // their row (g_src + s) mod 3 to the group s steps ahead
#pragma unroll
        for (int v = 0; v < 4; ++v) out[v] = ga == 0 ? acc[0][v] : (ga == 1 ? acc[1][v] : acc[2][v]);
#pragma unroll
        for (int s_ = 1; s_ <= 2; ++s_) {
            const int to_row = (ga + s_) % 3;
            int src_g = ga - s_;
            if (src_g < 0) src_g += 3;
            const int src_lane = active ? src_g * lpn + cl : lane;
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const double send = to_row == 0 ? acc[0][v] : (to_row == 1 ? acc[1][v] : acc[2][v]);
                out[v] += __shfl(send, src_lane, 64);
            }
        }
    } else {
#pragma unroll
        for (int v = 0; v < 4; ++v) out[v] = acc[0][v];
    }
    if (active) {
        double* yp = Y + (node * 3 + g) * ldy + cl * 4;
        __builtin_nontemporal_store(d2{out[0], out[1]}, reinterpret_cast<d2*>(yp));  // (written once)
        __builtin_nontemporal_store(d2{out[2], out[3]}, reinterpret_cast<d2*>(yp + 2));
    }
}

}  // namespace

extern "C" int ds_spmm_bsr3(int kind, const int32_t* rowptr, const int32_t* colidx, const void* vals,
                            const void* vals_t, int64_t nv, const void* X, int64_t ldx, void* Y, int64_t ldy,
                            int ncols, ds_stream_t stream) {
    DS_REQUIRE(rowptr && colidx && vals && X && Y, "ds_spmm_bsr3: null pointer");
    DS_REQUIRE(nv > 0 && ncols > 0, "ds_spmm_bsr3: empty problem");
    DS_REQUIRE(kind >= 0 && kind <= 5, "ds_spmm_bsr3: unknown kind %d", kind);
    DS_REQUIRE(ldx >= ncols && ldy >= ncols, "ds_spmm_bsr3: leading dimension smaller than ncols");
    hipStream_t st = ds::as_stream(stream);
    const bool f64out = kind >= 2, f64in = kind >= 4;
    const int xalign = (int)(reinterpret_cast<uintptr_t>(X) | (uintptr_t)(ldx * (f64in ? 8 : 4)));
    const int yalign = (int)(reinterpret_cast<uintptr_t>(Y) | (uintptr_t)(ldy * (f64out ? 8 : 4)));
    if (!f64out) {
        // float4 path needs 16-byte aligned rows; float2 path 8-byte
        if (ncols % 4 == 0 && ncols <= 256 && (xalign & 15) == 0 && (yalign & 15) == 0) {
            // (the fast path addresses X through one buffer descriptor: 32-bit byte offsets)
            return kind == 0 ? launch_fast<0>(rowptr, colidx, vals, vals_t, nv, X, ldx, Y, ldy, ncols, st)
                             : launch_fast<1>(rowptr, colidx, vals, vals_t, nv, X, ldx, Y, ldy, ncols, st);
        }
        DS_REQUIRE(ncols % 2 == 0 && ncols <= 128 && (xalign & 7) == 0 && (yalign & 7) == 0,
                   "ds_spmm_bsr3: f32 blocks need an even column count <= 256 (multiple of 4 above 128) and "
                   "8/16-byte aligned rows (ncols=%d ldx=%lld ldy=%lld)",
                   ncols, (long long)ldx, (long long)ldy);
        return kind == 0 ? launch<0, float, float, float, 2>(rowptr, colidx, vals, nv, X, ldx, Y, ldy, ncols, st)
                         : launch<1, float, float, float, 2>(rowptr, colidx, vals, nv, X, ldx, Y, ldy, ncols, st);
    }
    const unsigned nblk = (unsigned)ds::ceil_div(nv, 4);
    const double* dv = static_cast<const double*>(vals);
    double* dy = static_cast<double*>(Y);
    if (f64in) {  // fp64 iterates of the refinement phase: the wave-per-node kernel only
        DS_REQUIRE(ncols % 4 == 0 && ncols <= 84 && (xalign & 31) == 0 && (yalign & 15) == 0,
                   "ds_spmm_bsr3: f64-input blocks need a column count that is a multiple of 4, <= 84, and 32-byte "
                   "aligned rows (ncols=%d)", ncols);
        const double* dx = static_cast<const double*>(X);
        if (kind == 4)
            spmm_f64_node_kernel<0, double><<<nblk, 256, 0, st>>>(rowptr, colidx, dv, nv, dx, ldx, dy, ldy, ncols / 4, nblk);
        else
            spmm_f64_node_kernel<1, double><<<nblk, 256, 0, st>>>(rowptr, colidx, dv, nv, dx, ldx, dy, ldy, ncols / 4, nblk);
        DS_LAUNCH_CHECK("spmm_f64_node_kernel<double>");
        return DS_OK;
    }
    DS_REQUIRE(ncols % 2 == 0 && ncols <= 128 && (xalign & 7) == 0 && (yalign & 15) == 0,
               "ds_spmm_bsr3: f64-output blocks need an even column count <= 128 and aligned rows (ncols=%d)", ncols);
    if (ncols % 4 == 0 && ncols <= 84 && (xalign & 15) == 0) {
        const float* fx = static_cast<const float*>(X);
        if (kind == 2)
            spmm_f64_node_kernel<0, float><<<nblk, 256, 0, st>>>(rowptr, colidx, dv, nv, fx, ldx, dy, ldy, ncols / 4, nblk);
        else
            spmm_f64_node_kernel<1, float><<<nblk, 256, 0, st>>>(rowptr, colidx, dv, nv, fx, ldx, dy, ldy, ncols / 4, nblk);
        DS_LAUNCH_CHECK("spmm_f64_node_kernel");
        return DS_OK;
    }
    return kind == 2 ? launch<0, double, float, double, 2>(rowptr, colidx, vals, nv, X, ldx, Y, ldy, ncols, st)
                     : launch<1, double, float, double, 2>(rowptr, colidx, vals, nv, X, ldx, Y, ldy, ncols, st);
}

extern "C" int ds_cheb_spmm(const int32_t* rowptr, const int32_t* colidx, const float* vals, int64_t nv, const float* W,
                            int64_t ldw, float* Wprev, int64_t ldp, const float* R0, int64_t ldr, const float* dinv,
                            int ncols, float c1, float c2, int first, ds_stream_t stream) {
    DS_REQUIRE(rowptr && colidx && vals && W && Wprev && R0 && dinv, "ds_cheb_spmm: null pointer");
    DS_REQUIRE(nv > 0 && ncols > 0 && ncols % 4 == 0 && ncols <= 84, "ds_cheb_spmm: ncols must be a multiple of 4 <= 84");
    DS_REQUIRE(ldw >= ncols && ldp >= ncols && ldr >= ncols, "ds_cheb_spmm: leading dimension smaller than ncols");
    const uintptr_t al = reinterpret_cast<uintptr_t>(W) | reinterpret_cast<uintptr_t>(Wprev) |
                         reinterpret_cast<uintptr_t>(R0) | (uintptr_t)(ldw * 4) | (uintptr_t)(ldp * 4) |
                         (uintptr_t)(ldr * 4);
    DS_REQUIRE((al & 15) == 0, "ds_cheb_spmm: rows must be 16-byte aligned");
    DS_REQUIRE(W != Wprev, "ds_cheb_spmm: W and Wprev must be different buffers");
    hipStream_t st = ds::as_stream(stream);
    const ChebEpilogue epi{R0, ldr, dinv, c1, c2, first};
    const int lpn = ncols / 4;
    switch (lpn) {
        case 18: return launch_wn<0, 3, 18, 1>(rowptr, colidx, vals, nullptr, nv, W, ldw, Wprev, ldp, lpn, st, epi);
        case 20: return launch_wn<0, 3, 20, 1>(rowptr, colidx, vals, nullptr, nv, W, ldw, Wprev, ldp, lpn, st, epi);
        default: return launch_wn<0, 3, 0, 1>(rowptr, colidx, vals, nullptr, nv, W, ldw, Wprev, ldp, lpn, st, epi);
    }
}

// Y = R0 - K X on a block of <= 84 columns: the residual the two-level preconditioner restricts to the
// corner-node (P1) level, produced without writing K X to HBM.
extern "C" int ds_spmm_residual(const int32_t* rowptr, const int32_t* colidx, const float* vals, int64_t nv,
                                const float* X, int64_t ldx, const float* R0, int64_t ldr, float* Y, int64_t ldy,
                                int ncols, ds_stream_t stream) {
    DS_REQUIRE(rowptr && colidx && vals && X && R0 && Y, "ds_spmm_residual: null pointer");
    DS_REQUIRE(nv > 0 && ncols > 0 && ncols % 4 == 0 && ncols <= 84, "ds_spmm_residual: ncols must be a multiple of 4 <= 84");
    DS_REQUIRE(ldx >= ncols && ldy >= ncols && ldr >= ncols, "ds_spmm_residual: leading dimension smaller than ncols");
    const uintptr_t al = reinterpret_cast<uintptr_t>(X) | reinterpret_cast<uintptr_t>(Y) |
                         reinterpret_cast<uintptr_t>(R0) | (uintptr_t)(ldx * 4) | (uintptr_t)(ldy * 4) |
                         (uintptr_t)(ldr * 4);
    DS_REQUIRE((al & 15) == 0, "ds_spmm_residual: rows must be 16-byte aligned");
    DS_REQUIRE(X != Y, "ds_spmm_residual: X and Y must be different buffers");
    hipStream_t st = ds::as_stream(stream);
    const ChebEpilogue epi{R0, ldr, nullptr, 0.f, 0.f, 0};
    const int lpn = ncols / 4;
    switch (lpn) {
        case 20: return launch_wn<0, 3, 20, 2>(rowptr, colidx, vals, nullptr, nv, X, ldx, Y, ldy, lpn, st, epi);
        default: return launch_wn<0, 3, 0, 2>(rowptr, colidx, vals, nullptr, nv, X, ldx, Y, ldy, lpn, st, epi);
    }
}
