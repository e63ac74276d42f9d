// fp64-value SpMM of the read-out and the fp64 refinement: the read-out's three products in one walk of the node pattern
// (spmm_f64_polish_kernel) and the refinement's products on the neighbour-union tables (spmm_f64_union.inc), with their entry
// points.  Exports ds_spmm_f64_union, ds_spmm_f64_polish, ds_spmm_f64_polish_f32out.
#include <cstdint>

#include "ds_common.h"

namespace {

// The read-out's three fp64-value products in ONE walk of the pattern: Ya = A X, Yb = B X (3x3 fp64 blocks: K_lambda and
// K_mu) and Ym = (m (x) I3) X (the node-scalar mass values) share every gathered panel of the fp32 block X.  Three
// launches of spmm_f64_node_kernel (spmm.hip) are bound by exactly those gathers (3.2 GB out of L2 per 64-column product at the
// benchmark size: 0.63 + 0.63 + 0.22 ms); per output the arithmetic and its order are theirs, so the results are
// bit-identical.
// Round 4: the row's fp64 coefficients (9 + 9 + 1 doubles per block) no longer come through seven dependent-address global
// loads per block and lane (the kernel was bound by vector-memory ISSUE: 33 M wave-loads for 4.1 M blocks) but are staged per
// chunk of the row in LDS with coalesced 8-byte loads and read back as broadcasts; the neighbour ids of the chunk sit in one
// register (a coalesced load) and come back with v_readlane, so a panel's address is scalar arithmetic.  The sums and their
// order are unchanged: results bit-identical to the three separate launches, as before.
constexpr int PL_CHUNK = 32;  // blocks of a row staged per pass
constexpr int PL_WIN = 4;     // panels per gather window (two windows: 8 in flight)
// TY: the type the three results are STORED in - double, or float (round 5: the sums are formed in fp64 either way and rounded
// once; the fp32 blocks halve the 0.86 GB the kernel writes and the Gram launch behind it reads, and that Gram then runs on the
// fp32 matrix-core path; a result entry carries 6e-8 of relative rounding, the Gram entries ~1e-10 - see polish_products)
template <typename TY>
__global__ void __launch_bounds__(256)
    spmm_f64_polish_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colidx,
                           const double* __restrict__ va, const double* __restrict__ vb, const double* __restrict__ vm,
                           int64_t nv, const float* __restrict__ X, int64_t ldx, TY* __restrict__ Ya,
                           TY* __restrict__ Yb, TY* __restrict__ Ym, int64_t ldy, int lpn, unsigned nblk) {
    using d2 = __attribute__((ext_vector_type(2))) double;
    using xv4 = __attribute__((ext_vector_type(4))) float;
    __shared__ double s_a[4][PL_CHUNK * 9], s_b[4][PL_CHUNK * 9], s_m[4][PL_CHUNK];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t node = (int64_t)ds::xcd_remap(blockIdx.x, nblk) * 4 + wave;
    if (node >= nv) return;  // wave-uniform
    const int g = lane / lpn, cl = lane - g * lpn;
    const bool active = g < 3;
    const int ga = active ? g : 0;
    const int kb = __builtin_amdgcn_readfirstlane(rowptr[node]), ke = __builtin_amdgcn_readfirstlane(rowptr[node + 1]);
    const float* xb = X + (int64_t)ga * ldx + cl * 4;
    double* sa = s_a[wave];
    double* sb = s_b[wave];
    double* sm = s_m[wave];
    double aa[3][4], ab[3][4], am[4];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        am[v] = 0.0;
#pragma unroll
        for (int r = 0; r < 3; ++r) aa[r][v] = ab[r][v] = 0.0;
    }
    for (int kc = kb; kc < ke; kc += PL_CHUNK) {
        const int cnt = min(PL_CHUNK, ke - kc);  // wave-uniform
        const int colreg = colidx[kc + min(lane, cnt - 1)];
        const double* pa = va + (int64_t)kc * 9;
        const double* pb = vb + (int64_t)kc * 9;
        {  // all the chunk's coefficient loads in flight at once (clamped, not predicated)
            constexpr int NSL = (PL_CHUNK * 9 + 63) / 64;
            double ra[NSL], rb[NSL];
#pragma unroll
            for (int i = 0; i < NSL; ++i) {
                const int t = min(lane + 64 * i, cnt * 9 - 1);
                ra[i] = __builtin_nontemporal_load(pa + t), rb[i] = __builtin_nontemporal_load(pb + t);  // (read once)
            }
            const double rm = vm[kc + min(lane, cnt - 1)];
#pragma unroll
            for (int i = 0; i < NSL; ++i)
                if (lane + 64 * i < cnt * 9) sa[lane + 64 * i] = ra[i], sb[lane + 64 * i] = rb[i];
            if (lane < cnt) sm[lane] = rm;
        }
        // same-wave LDS write -> read (rows differ in length: no workgroup barrier)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        // Two windows of PL_WIN panel gathers: the next window is requested before the current one is used (see
        // spmm_f64_node_kernel, spmm.hip); same sums, same order
        auto issue = [&](xv4 (&xs)[PL_WIN], int u0) {
#pragma unroll
            for (int j = 0; j < PL_WIN; ++j) {
                const int64_t col = __builtin_amdgcn_readlane(colreg, min(u0 + j, cnt - 1));
                xs[j] = *reinterpret_cast<const xv4*>(xb + col * 3 * ldx);
            }
        };
        auto consume = [&](const xv4 (&xs)[PL_WIN], int u0) {
#pragma unroll
            for (int j = 0; j < PL_WIN; ++j) {
                if (u0 + j < cnt) {  // wave-uniform
                    const int u = u0 + j;
                    const double* ca = sa + u * 9 + ga;  // column g of the blocks
                    const double* cb = sb + u * 9 + ga;
                    const double a0 = ca[0], a1 = ca[3], a2 = ca[6], b0 = cb[0], b1 = cb[3], b2 = cb[6], m = sm[u];
#pragma unroll
                    for (int v = 0; v < 4; ++v) {
                        const double xv = (double)xs[j][v];
                        aa[0][v] = fma(a0, xv, aa[0][v]);
                        aa[1][v] = fma(a1, xv, aa[1][v]);
                        aa[2][v] = fma(a2, xv, aa[2][v]);
                        ab[0][v] = fma(b0, xv, ab[0][v]);
                        ab[1][v] = fma(b1, xv, ab[1][v]);
                        ab[2][v] = fma(b2, xv, ab[2][v]);
                        am[v] = fma(m, xv, am[v]);
                    }
                }
            }
        };
        xv4 x0[PL_WIN], x1[PL_WIN];
        issue(x0, 0);
        for (int u0 = 0; u0 < cnt; u0 += 2 * PL_WIN) {
            issue(x1, u0 + PL_WIN);  // (a window past the chunk re-reads its last panel and is skipped)
            consume(x0, u0);
            issue(x0, u0 + 2 * PL_WIN);
            consume(x1, u0 + PL_WIN);
        }
        if (kc + PL_CHUNK < ke) {  // the slabs are rewritten by the next pass
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
    }
    // lane (g, cl) ends with output row g: its own share plus the shares of the two other groups (as the node kernel)
    double oa[4], ob[4];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        oa[v] = ga == 0 ? aa[0][v] : (ga == 1 ? aa[1][v] : aa[2][v]);
        ob[v] = ga == 0 ? ab[0][v] : (ga == 1 ? ab[1][v] : ab[2][v]);
    }
#pragma unroll
    for (int s_ = 1; s_ <= 2; ++s_) {
        const int to_row = (ga + s_) % 3;
        int src_g = ga - s_;
        if (src_g < 0) src_g += 3;
        const int src_lane = active ? src_g * lpn + cl : lane;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const double sa = to_row == 0 ? aa[0][v] : (to_row == 1 ? aa[1][v] : aa[2][v]);
            const double sb = to_row == 0 ? ab[0][v] : (to_row == 1 ? ab[1][v] : ab[2][v]);
            oa[v] += __shfl(sa, src_lane, 64);
            ob[v] += __shfl(sb, src_lane, 64);
        }
    }
    if (active) {
        const int64_t o = (node * 3 + g) * ldy + cl * 4;
        if constexpr (sizeof(TY) == 8) {
            __builtin_nontemporal_store(d2{oa[0], oa[1]}, reinterpret_cast<d2*>(Ya + o));  // (written once)
            __builtin_nontemporal_store(d2{oa[2], oa[3]}, reinterpret_cast<d2*>(Ya + o + 2));
            __builtin_nontemporal_store(d2{ob[0], ob[1]}, reinterpret_cast<d2*>(Yb + o));
            __builtin_nontemporal_store(d2{ob[2], ob[3]}, reinterpret_cast<d2*>(Yb + o + 2));
            __builtin_nontemporal_store(d2{am[0], am[1]}, reinterpret_cast<d2*>(Ym + o));
            __builtin_nontemporal_store(d2{am[2], am[3]}, reinterpret_cast<d2*>(Ym + o + 2));
        } else {
            *reinterpret_cast<xv4*>(Ya + o) = xv4{(float)oa[0], (float)oa[1], (float)oa[2], (float)oa[3]};
            *reinterpret_cast<xv4*>(Yb + o) = xv4{(float)ob[0], (float)ob[1], (float)ob[2], (float)ob[3]};
            *reinterpret_cast<xv4*>(Ym + o) = xv4{(float)am[0], (float)am[1], (float)am[2], (float)am[3]};
        }
    }
}

#include "spmm_f64_union.inc"

}  // namespace

// fp64 values (and fp64 or fp32 vectors) on the neighbour-union tables (spmm_f64_union.inc): the fp64 refinement's K W / M W
extern "C" int ds_spmm_f64_union(int kind, int x_f64, const int32_t* utab, const int32_t* ctab, int64_t ngroups, int cap_blocks,
                                 const int32_t* gent, const double* vals, int64_t nnzb, int64_t nv, const void* X, int64_t ldx,
                                 double* Y, int64_t ldy, int ncols, ds_stream_t stream) {
    DS_REQUIRE(ctab && gent && vals && X && Y, "ds_spmm_f64_union: null pointer");
    DS_REQUIRE(kind == 0 || kind == 1, "ds_spmm_f64_union: kind must be 0 (3x3 blocks in group order, transposed) or 1 (node scalars)");
    DS_REQUIRE(nv > 0 && ngroups == (nv + 3) / 4 && nnzb > 0 && ncols > 0 && ncols % 4 == 0 && ncols <= 84,
               "ds_spmm_f64_union: ncols must be a multiple of 4 <= 84 and ngroups = ceil(nv / 4)");
    DS_REQUIRE(cap_blocks > 0 && cap_blocks <= DS_UNION_CAP, "ds_spmm_f64_union: a chunk of %d blocks exceeds the LDS image", cap_blocks);
    DS_REQUIRE(ldx >= ncols && ldy >= ncols, "ds_spmm_f64_union: leading dimension smaller than ncols");
    DS_REQUIRE(static_cast<const void*>(Y) != X, "ds_spmm_f64_union: X and Y must be different buffers");
    const int xb = x_f64 ? 8 : 4;
    DS_REQUIRE(((reinterpret_cast<uintptr_t>(X) | (uintptr_t)(ldx * xb) | reinterpret_cast<uintptr_t>(Y) | (uintptr_t)(ldy * 8) |
                 reinterpret_cast<uintptr_t>(ctab)) & 15) == 0, "ds_spmm_f64_union: rows and ctab must be 16-byte aligned");
    hipStream_t st = ds::as_stream(stream);
    const unsigned nwg = (unsigned)ds::ceil_div(ngroups, 4);
    const int lpn = ncols / 4;
    const int2* ut = reinterpret_cast<const int2*>(utab);
    const int4* ct = reinterpret_cast<const int4*>(ctab);
#define DS_F64U(K, T) spmm_f64_union_kernel<K, T><<<nwg, 256, 0, st>>>(ut, ct, (unsigned)ngroups, gent, vals, nv, static_cast<const T*>(X), ldx, Y, ldy, lpn, nwg)
    if (kind == 0) {
        if (x_f64) DS_F64U(0, double);
        else DS_F64U(0, float);
    } else {
        if (x_f64) DS_F64U(1, double);
        else DS_F64U(1, float);
    }
#undef DS_F64U
    DS_LAUNCH_CHECK("spmm_f64_union_kernel");
    return DS_OK;
}

// Ya = A X, Yb = B X (fp64 3x3 block values), Ym = (m (x) I3) X (fp64 node scalars) for one fp32 block X in one walk.
extern "C" int ds_spmm_f64_polish(const int32_t* rowptr, const int32_t* colidx, const double* a, const double* b,
                                  const double* m, int64_t nv, const float* X, int64_t ldx, double* Ya, double* Yb,
                                  double* Ym, int64_t ldy, int ncols, ds_stream_t stream) {
    DS_REQUIRE(rowptr && colidx && a && b && m && X && Ya && Yb && Ym, "ds_spmm_f64_polish: null pointer");
    DS_REQUIRE(nv > 0 && ncols > 0 && ncols % 4 == 0 && ncols <= 84, "ds_spmm_f64_polish: ncols must be a multiple of 4 <= 84");
    DS_REQUIRE(ldx >= ncols && ldy >= ncols, "ds_spmm_f64_polish: leading dimension smaller than ncols");
    const uintptr_t ya = reinterpret_cast<uintptr_t>(Ya) | reinterpret_cast<uintptr_t>(Yb) | reinterpret_cast<uintptr_t>(Ym) |
                         (uintptr_t)(ldy * 8);
    DS_REQUIRE(((reinterpret_cast<uintptr_t>(X) | (uintptr_t)(ldx * 4) | ya) & 15) == 0,
               "ds_spmm_f64_polish: rows must be 16-byte aligned");
    DS_REQUIRE(Ya != Yb && Ya != Ym && Yb != Ym, "ds_spmm_f64_polish: the three results must be different buffers");
    const unsigned nblk = (unsigned)ds::ceil_div(nv, 4);
    spmm_f64_polish_kernel<double><<<nblk, 256, 0, ds::as_stream(stream)>>>(rowptr, colidx, a, b, m, nv, X, ldx, Ya, Yb, Ym, ldy,
                                                                            ncols / 4, nblk);
    DS_LAUNCH_CHECK("spmm_f64_polish_kernel");
    return DS_OK;
}

// the same products, stored as fp32 blocks (sums in fp64, one rounding)
extern "C" int ds_spmm_f64_polish_f32out(const int32_t* rowptr, const int32_t* colidx, const double* a, const double* b,
                                         const double* m, int64_t nv, const float* X, int64_t ldx, float* Ya, float* Yb,
                                         float* Ym, int64_t ldy, int ncols, ds_stream_t stream) {
    DS_REQUIRE(rowptr && colidx && a && b && m && X && Ya && Yb && Ym, "ds_spmm_f64_polish_f32out: null pointer");
    DS_REQUIRE(nv > 0 && ncols > 0 && ncols % 4 == 0 && ncols <= 84, "ds_spmm_f64_polish_f32out: ncols must be a multiple of 4 <= 84");
    DS_REQUIRE(ldx >= ncols && ldy >= ncols, "ds_spmm_f64_polish_f32out: leading dimension smaller than ncols");
    const uintptr_t ya = reinterpret_cast<uintptr_t>(Ya) | reinterpret_cast<uintptr_t>(Yb) | reinterpret_cast<uintptr_t>(Ym) |
                         (uintptr_t)(ldy * 4);
    DS_REQUIRE(((reinterpret_cast<uintptr_t>(X) | (uintptr_t)(ldx * 4) | ya) & 15) == 0,
               "ds_spmm_f64_polish_f32out: rows must be 16-byte aligned");
    DS_REQUIRE(Ya != Yb && Ya != Ym && Yb != Ym && Ya != X && Yb != X && Ym != X,
               "ds_spmm_f64_polish_f32out: X and the three results must be different buffers");
    const unsigned nblk = (unsigned)ds::ceil_div(nv, 4);
    spmm_f64_polish_kernel<float><<<nblk, 256, 0, ds::as_stream(stream)>>>(rowptr, colidx, a, b, m, nv, X, ldx, Ya, Yb, Ym, ldy,
                                                                           ncols / 4, nblk);
    DS_LAUNCH_CHECK("spmm_f64_polish_kernel<float>");
    return DS_OK;
}
