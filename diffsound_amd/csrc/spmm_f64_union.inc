// fp64 neighbour-union SpMM (round 5): Y = A X with fp64 values AND fp64 (or fp32) vectors, one wave per group of 4 consecutive nodes.
// Included from spmm_f64.hip inside its anonymous namespace.
//
// The fp64 refinement's K W / M W (configs[4]) ran on spmm_f64_node_kernel - one wave per NODE, which gathers the 1 920-byte fp64
// panel of every neighbour of every row: 53 KB of panels per node against 2 KB of coefficients, 73 GB through the L2s per
// 80-column product at the 1M-tet mesh (4.7 ms, 28 % of STREAM on the algorithmic bytes).  The rows of 4 Morton-consecutive
// nodes share most neighbours (the union holds 0.46 of their blocks): this kernel walks the UNION, as the fp32 production
// kernel does - same tables (gent = col | mask << 28, chunk rows ctab, utab), values in group order (transposed blocks
// vals[p][g][i] = A_block[i][g], or node scalars) - and feeds every gathered panel to up to four accumulator sets.
// Plain C++ (no hand-scheduled window): the fp64 FMAs of a panel (up to 48 per lane) cover the next panels' latency with the
// four-deep prefetch below.  Sums per output element in union order, three row groups added at the end: equal to the node
// kernel's results to fp64 rounding, not bit for bit.
// neighbour panels per prefetch window (two windows in flight).  fp64 panels with 3x3 blocks: 96 accumulator registers + 8 per
// panel piece - a window of 4 costs 202 registers (2 waves per SIMD), a window of 2 fits 3 waves
template <int KIND, typename TX>
constexpr int f64u_win() { return (KIND == 0 && sizeof(TX) == 8) ? 2 : 4; }

template <int KIND, typename TX>  // KIND 0: 3x3 blocks, 1: node scalars (A = a (x) I3)
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(KIND == 0 ? 3 : 4)))
    spmm_f64_union_kernel(const int2* __restrict__ utab, const int4* __restrict__ ctab, unsigned ngroups,
                          const int32_t* __restrict__ gent, const double* __restrict__ vals, int64_t nv,
                          const TX* __restrict__ X, int64_t ldx, double* __restrict__ Y, int64_t ldy, int lpn, unsigned nwg) {
    using d2 = __attribute__((ext_vector_type(2))) double;
    using xv4 = __attribute__((ext_vector_type(4))) TX;
    constexpr int CAPB = DS_UNION_CAP, NE = DS_UNION_CAP + 4;
    constexpr int F64U_WIN = f64u_win<KIND, TX>();
    __shared__ int s_ent[4][NE];
    __shared__ double s_val[4][KIND == 0 ? CAPB * 9 : CAPB];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const unsigned grp = ds::xcd_remap(blockIdx.x, nwg) * 4 + wave;
    if (grp >= ngroups) return;  // wave-uniform; no workgroup barrier in this kernel
    int ch0 = (int)grp, ch1 = (int)grp + 1;
    if (utab) {
        const int2 ut = utab[grp];
        ch0 = __builtin_amdgcn_readfirstlane(ut.x), ch1 = __builtin_amdgcn_readfirstlane(ut.y);
    }
    const int g = lane / lpn, cl = lane - g * lpn;
    const bool active = g < 3;
    const int ga = active ? g : 0;
    const TX* xb = X + (int64_t)ga * ldx + cl * 4;
    int* se = s_ent[wave];
    double* sv = s_val[wave];
    double acc[4][KIND == 0 ? 3 : 1][4];
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int i = 0; i < (KIND == 0 ? 3 : 1); ++i)
#pragma unroll
            for (int v = 0; v < 4; ++v) acc[s][i][v] = 0.0;
    for (int ch = ch0; ch < ch1; ++ch) {  // almost always one chunk; the accumulators carry over
        const int4 ct = ctab[ch];
        const int e0 = __builtin_amdgcn_readfirstlane(ct.x), ne = __builtin_amdgcn_readfirstlane(ct.y) - e0;
        const int b0 = __builtin_amdgcn_readfirstlane(ct.z), nbk = __builtin_amdgcn_readfirstlane(ct.w) - b0;
        // entries and coefficients of the chunk -> LDS (coalesced loads, read once: non-temporal)
        for (int t = lane; t < ne; t += 64) se[t] = __builtin_nontemporal_load(gent + e0 + t);
        {
            constexpr int PER = KIND == 0 ? 9 : 1;
            const double* pv = vals + (int64_t)b0 * PER;
            const int cntv = nbk * PER;
            constexpr int NSL = (CAPB * PER + 63) / 64;
            double stg[NSL];
#pragma unroll
            for (int i = 0; i < NSL; ++i) stg[i] = __builtin_nontemporal_load(pv + min(lane + 64 * i, cntv - 1));
#pragma unroll
            for (int i = 0; i < NSL; ++i)
                if (lane + 64 * i < cntv) sv[lane + 64 * i] = stg[i];
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        int blk = 0;  // next block of the chunk (wave-uniform: the masks are)
        auto issue = [&](xv4 (&xs)[F64U_WIN], int u0) {
#pragma unroll
            for (int j = 0; j < F64U_WIN; ++j) {
                const int64_t col = se[min(u0 + j, ne - 1)] & 0x0fffffff;
                xs[j] = *reinterpret_cast<const xv4*>(xb + col * 3 * ldx);
            }
        };
        auto consume = [&](const xv4 (&xs)[F64U_WIN], int u0) {
#pragma unroll
            for (int j = 0; j < F64U_WIN; ++j) {
                if (u0 + j < ne) {  // wave-uniform
                    const unsigned m = (unsigned)__builtin_amdgcn_readfirstlane(se[u0 + j]) >> 28;
                    double xv[4];
#pragma unroll
                    for (int v = 0; v < 4; ++v) xv[v] = (double)xs[j][v];
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        if (m & (1u << s)) {  // wave-uniform
                            if constexpr (KIND == 0) {
                                const double* a = sv + blk * 9 + ga * 3;  // A_block[0..2][g]
                                const double a0 = a[0], a1 = a[1], a2 = a[2];
#pragma unroll
                                for (int v = 0; v < 4; ++v) {
                                    acc[s][0][v] = fma(a0, xv[v], acc[s][0][v]);
                                    acc[s][1][v] = fma(a1, xv[v], acc[s][1][v]);
                                    acc[s][2][v] = fma(a2, xv[v], acc[s][2][v]);
                                }
                            } else {
                                const double a = sv[blk];
#pragma unroll
                                for (int v = 0; v < 4; ++v) acc[s][0][v] = fma(a, xv[v], acc[s][0][v]);
                            }
                            ++blk;
                        }
                    }
                }
            }
        };
        xv4 x0[F64U_WIN], x1[F64U_WIN];
        if (ne > 0) issue(x0, 0);
        for (int u0 = 0; u0 < ne; u0 += 2 * F64U_WIN) {
            issue(x1, u0 + F64U_WIN);  // (a window past the chunk re-reads its last panel and is skipped)
            consume(x0, u0);
            issue(x0, u0 + 2 * F64U_WIN);
            consume(x1, u0 + F64U_WIN);
        }
        (void)nbk;
        if (ch + 1 < ch1) {  // the images are rewritten by the next chunk
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
    }
    const int64_t n0 = (int64_t)grp * 4;
    const int nn = (int)min<int64_t>(4, nv - n0);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        if (s < nn) {  // wave-uniform
            double out[4];
            if constexpr (KIND == 0) {
                // lane (g, cl) ends with output row g: its own share plus the shares of the two other row groups
#pragma unroll
                for (int v = 0; v < 4; ++v) out[v] = ga == 0 ? acc[s][0][v] : (ga == 1 ? acc[s][1][v] : acc[s][2][v]);
#pragma unroll
                for (int st = 1; st <= 2; ++st) {
                    const int to_row = (ga + st) % 3;
                    int src_g = ga - st;
                    if (src_g < 0) src_g += 3;
                    const int src_lane = active ? src_g * lpn + cl : lane;
#pragma unroll
                    for (int v = 0; v < 4; ++v) {
                        const double send = to_row == 0 ? acc[s][0][v] : (to_row == 1 ? acc[s][1][v] : acc[s][2][v]);
                        out[v] += __shfl(send, src_lane, 64);
                    }
                }
            } else {
#pragma unroll
                for (int v = 0; v < 4; ++v) out[v] = acc[s][0][v];
            }
            if (active) {
                double* yp = Y + ((n0 + s) * 3 + g) * ldy + cl * 4;
                __builtin_nontemporal_store(d2{out[0], out[1]}, reinterpret_cast<d2*>(yp));
                __builtin_nontemporal_store(d2{out[2], out[3]}, reinterpret_cast<d2*>(yp + 2));
            }
        }
    }
}
