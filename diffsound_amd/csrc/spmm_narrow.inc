// Neighbour-union SpMM for NARROW blocks (<= 16 columns): Y = K X (3x3 blocks) or Y = (M_s (x) I3) X.  Included from
// spmm_union.hip inside its anonymous namespace, after spmm_union.inc.
//
// The production kernel (spmm_union.inc) walks a group's union entries ONE AFTER THE OTHER with all 64 lanes on one entry -
// 3 panel rows x (columns / 4) lanes; on an 8-column block that is 6 busy lanes and a chain of ~62 dependent steps per
// wave: the eigensolver's 8-column products (the block power iteration for the Chebyshev interval, the operator-norm
// estimates; four launches per pass) took 140-150 us each on the benchmark mesh, as long as an 80-column product, 4.8 % of
// a pass's kernel time (profiles/r05a_bench_lanes1_kernel_stats.csv).  Here the lanes are dealt over the ENTRIES: a lane
// (entry slot es, column quad cl) loads the three panel rows of its entries itself, multiplies them by the blocks of the up
// to four nodes that have that neighbour, and the slots are summed by a butterfly at the end - a chain of
// ceil(entries / slots) steps (2-4) instead of ~62.  Same tables as the production kernel (gent, ctab / utab, values in group
// order); per output element the products are summed in another ORDER than there (per slot, then across slots): results
// agree to fp32 rounding, not bit for bit - ds_spmm_union keeps serving every width, this is a separate entry point
// (ds_spmm_union_narrow) that the operators' apply_K / apply_M take for <= 16 columns.
constexpr int NARROW_TILE = 320;  // union entries per LDS tile of a wave (a group of the benchmark mesh has ~62, at most 140)

template <bool SCALAR, int LVL>
__global__ void __launch_bounds__(256)
    spmm_union_narrow_kernel(const int2* __restrict__ utab, const int4* __restrict__ ctab, unsigned ngroups,
                             const int32_t* __restrict__ gent, const float* __restrict__ vals, int64_t nv,
                             const float* __restrict__ X, int64_t ldx, float* __restrict__ Y, int64_t ldy, int ncols, unsigned nwg) {
    using f4 = __attribute__((ext_vector_type(4))) float;
    __shared__ int s_ent[4][NARROW_TILE];
    __shared__ int s_pre[4][NARROW_TILE];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const unsigned grp = ds::xcd_remap(blockIdx.x, nwg) * 4 + wave;
    if (grp >= ngroups) return;  // wave-uniform; the kernel has no workgroup barrier
    int ch0 = (int)grp, ch1 = (int)grp + 1;
    if (utab) {
        const int2 ut = utab[grp];
        ch0 = __builtin_amdgcn_readfirstlane(ut.x), ch1 = __builtin_amdgcn_readfirstlane(ut.y);
    }
    // the chunks of a group are consecutive runs of its entries and blocks: the group = [first chunk's start, last chunk's end)
    const int4 cf = ctab[ch0];
    const int e0 = __builtin_amdgcn_readfirstlane(cf.x);
    const int b0 = __builtin_amdgcn_readfirstlane(cf.z);
    const int e1 = ch1 - 1 == ch0 ? __builtin_amdgcn_readfirstlane(cf.y) : __builtin_amdgcn_readfirstlane(ctab[ch1 - 1].y);
    const int ne = e1 - e0;
    const int cq = ncols >> 2;                    // column quads in use: 1 .. 4
    const int sh = cq == 1 ? 0 : (cq == 2 ? 1 : 2);  // lanes per entry slot = 1 << sh (three quads take four lanes, one idle)
    const int cl = lane & ((1 << sh) - 1), es = lane >> sh, nslot = 64 >> sh;
    const bool active = cl < cq;
    int* se = s_ent[wave];
    int* sp = s_pre[wave];
    f4 acc[4][3];
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int i = 0; i < 3; ++i) acc[s][i] = f4{0.f, 0.f, 0.f, 0.f};
    int base_blk = b0;
    for (int t0 = 0; t0 < ne; t0 += NARROW_TILE) {
        const int nt = min(NARROW_TILE, ne - t0);
        // entries of the tile -> LDS with the number of blocks in front of each (exclusive prefix of the masks' popcounts)
        int running = 0;
        for (int i = 0; i < nt; i += 64) {
            const int idx = i + lane;
            const int ent = idx < nt ? gent[e0 + t0 + idx] : 0;
            const int pc = __builtin_popcount((unsigned)ent >> 28);
            int incl = pc;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int v = __shfl_up(incl, d);
                if (lane >= d) incl += v;
            }
            if (idx < nt) se[idx] = ent, sp[idx] = running + incl - pc;
            running += __shfl(incl, 63);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        for (int e = es; e < nt; e += nslot) {
            const int ent = se[e];
            const unsigned m = (unsigned)ent >> 28;
            const int64_t col = ent & 0x0fffffff;
            int64_t blk = base_blk + sp[e];
            f4 x0 = {0.f, 0.f, 0.f, 0.f}, x1 = x0, x2 = x0;
            if (active) {
                const float* xp = X + col * 3 * ldx + cl * 4;
                x0 = *reinterpret_cast<const f4*>(xp);
                x1 = *reinterpret_cast<const f4*>(xp + ldx);
                x2 = *reinterpret_cast<const f4*>(xp + 2 * ldx);
            }
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                if (m & (1u << s)) {
                    if constexpr (SCALAR) {
                        const float c = vals[blk];
                        acc[s][0] += c * x0, acc[s][1] += c * x1, acc[s][2] += c * x2;
                    } else {
                        // transposed block of the group order: k[g * 3 + i] = K_block[i][g]
                        const float* k = vals + blk * 9;
                        float kk[9];
#pragma unroll
                        for (int j = 0; j < 9; ++j) kk[j] = k[j];
#pragma unroll
                        for (int i = 0; i < 3; ++i) acc[s][i] += kk[i] * x0 + kk[3 + i] * x1 + kk[6 + i] * x2;
                    }
                    ++blk;
                }
            }
        }
        base_blk += running;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();  // (the next tile overwrites the images)
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    // sum over the entry slots: lanes with equal cl, butterfly over the slot bits
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        if (d >= (1 << sh)) {  // wave-uniform
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int i = 0; i < 3; ++i)
#pragma unroll
                    for (int c = 0; c < 4; ++c) acc[s][i][c] += __shfl_xor(acc[s][i][c], d);
        }
    }
    const int64_t n0 = (int64_t)grp * 4;
    const int nn = (int)min<int64_t>(4, nv - n0);
    if (es == 0 && active) {
#pragma unroll
        for (int s = 0; s < 4; ++s)
            if (s < nn) {
#pragma unroll
                for (int i = 0; i < 3; ++i) *reinterpret_cast<f4*>(Y + ((n0 + s) * 3 + i) * ldy + cl * 4) = acc[s][i];
            }
    }
}
