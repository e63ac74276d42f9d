// Neighbour-union SpMM (the production kernel of the <= 84-column products on both levels) and its inline-asm load /
// wait helpers.  Included from spmm_union.hip inside its anonymous namespace, after spmm_device.h.
// Phase B issues its loads through inline asm and waits with explicit counted s_waitcnt: left to the
// compiler, the FMAs sink below the re-issued loads, the window is renamed into fresh registers and copied
// back behind a vmcnt(0) at the loop latch (seen in the ISA of the first version of this kernel).  The loaded
// registers are tied in/out operands ("+v"): uses of the old value cannot move past the load, the new value
// cannot be read before the wait that carries it.  vmcnt retires in order, so "at most N younger operations
// outstanding" proves a load complete whatever else (stores, the other waves' traffic) is in the queue -
// PROVIDED every load of the phase is a buffer_load: global_load_* operand loads mixed into the window were
// overtaken by younger buffer loads on gfx950 (first nodes of a batch read stale operands; found with
// tools/dbg_cheb1.py), so the epilogue operands go through descriptors as well.
// descriptor of panel `idx` (wave-uniform) of a block whose descriptor words are `base`: base address + idx * bytes
__device__ __forceinline__ i4s rebase_rsrc(i4s base, int idx, int bytes) {
    const uint64_t a = ((uint64_t)(unsigned)base.x | ((uint64_t)(unsigned)(base.y & 0xffff) << 32)) +
                       (uint64_t)(unsigned)idx * (uint64_t)(unsigned)bytes;
    i4s r = base;
    r.x = (int)(unsigned)a;
    r.y = (int)((unsigned)(a >> 32) & 0xffffu);
    asm volatile("s_nop 4" : "+s"(r));  // (should the compiler route the arithmetic through the vector unit)
    return r;
}
#define DS_BUF_LOAD4(dst, voff, rsrc, soff) \
    asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 offen" : "+v"(dst) : "v"(voff), "s"(rsrc), "s"(soff) : "memory")
// the same with the accumulators as (unused) inputs: the FMAs that consumed the old value of dst produce them,
// so they cannot sink below the load (which would keep the old value alive in a COPY made before our wait)
#define DS_BUF_LOAD4_AFTER(dst, voff, rsrc, soff, a0, a1, a2)                    \
    asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 offen"                       \
                 : "+v"(dst)                                                      \
                 : "v"(voff), "s"(rsrc), "s"(soff), "v"(a0), "v"(a1), "v"(a2)     \
                 : "memory")
#define DS_WAIT_VM(n, reg) asm volatile("s_waitcnt vmcnt(%1)" : "+v"(reg) : "n"(n) : "memory")

// ------------------------------------------------------------------------------------------------
// Neighbour-union kernel for <= 84 columns: ONE WAVE PER GROUP OF 4 CONSECUTIVE NODES.
// The products above are bound by the bytes a CU gathers (DESIGN.md section 6).  Morton-consecutive nodes share
// neighbours: the union of the rows of 4 nodes has 0.58 x as many entries as the rows have blocks, so a wave
// that walks the union loads every shared panel ONCE and feeds it to up to 4 accumulator sets.
// Host tables (ds_groups_build): per group the sorted union entries gent = col | mask << 28 (mask: which of
// the 4 nodes have that neighbour), the blocks in entry-major / node-minor order (kgrp = TRANSPOSED blocks packed
// by ds_pack_groups), and utab[g] = (e0, e1, b0, b1) entry / block ranges.
// Phase A stages the group's entries and coefficients in LDS (as the batched kernel); phase B runs the rolling
// window over the ENTRIES; per entry the set bits of its mask are walked (wave-uniform), each consuming the next
// block of the linear coefficient stream (read one block ahead) into the accumulators of its node.  The wave then
// merges / finishes / stores its 4 nodes; their epilogue operands are fetched only then (nothing useful is left in
// flight at that point: one group per wave; touching those rows during phase A to warm the L2 cost 6 %).
constexpr int UN_G = 4;
// blocks (and entries) per chunk: the size of the LDS images.  140 since round 4 (116 before): with the nodes ordered in bricks
// aligned to the mesh's node planes the groups of the benchmark mesh hold at most 138 blocks, so EVERY group is one chunk (42 %
// of them were cut in two at 116: a second staging round trip each, and one dependent table read more for all) - and
// 4 x (152 entries + 152 x 48 B of coefficients) = 31.6 KB per workgroup still lets five workgroups share a CU's LDS
constexpr int UN_CAPB = DS_UNION_CAP;
static_assert(5 * 4 * ((DS_UNION_CAP + 12) * 4 + (DS_UNION_CAP + 12) * 48) <= 160 * 1024, "five workgroups per CU");
constexpr int UN_PAD = 12;  // readable entries / blocks behind the images (>= UX + 2)

// Where the time of this kernel goes (round 3, knock-out builds of the sources of commit 81379de, C3, K X on 80 columns;
// bits: 1 no FMAs, 2 no coefficient reads, 4 no panel gathers, 8 no block-value loads; profiles/r03_union_knockout.txt):
// whole 248 us; without FMAs 201, without coefficient reads 221, without gathers 174, without FMAs and gathers 143, with none
// of the three 92, skeleton (tables, loop control, merge, stores) 78.  The parts ADD UP - a wave's chain, not a saturated
// unit: the gathers alone run at 24 TB/s out of the L2 with this kernel's XCD-contiguous group ranges (tools/gather_probe.hip
// mode 7: 94 us; 10.5 TB/s with workgroups dealt round-robin over the XCDs, which is what round 3 first mistook for the
// bound).  What followed from it: coefficients read one block ahead (above), the staging offsets of phase A recomputed per
// chunk (84 VGPRs instead of 96 + spills): K X 249 -> 231-237 us, M X 164 -> 150, fp32 fused term 257 -> 245 on one box.
// Six waves per SIMD (80 VGPRs, 40 B of scratch per lane): 285 us.
// waves (= node groups) per workgroup
#ifndef DS_UNION_WPB
#define DS_UNION_WPB 4
#endif
#ifndef DS_UNION_WAVES
// (epilogues 4 - 6 carry 16 more accumulators: 4 waves per SIMD, <= 128 registers)
#define DS_UNION_WAVES(EPI, BF) ((EPI) >= 4 ? 4 : 5)
#endif
// LVL (0: fine level, 1: corner-node level) changes nothing but the kernel's SYMBOL (see spmm_mfma.inc): the eigensolver's own
// products K X / M X (epilogues 0 and 3) carry it, so a rocprofv3 kernel table separates the two levels' launches
template <int LPN_CT, int EPI, int CAPB, bool BIG = false, bool BF = false, bool OUT32 = true, int LVL = 0>
// Five waves per SIMD (<= 96 VGPRs) with a window of four loads beat four waves with a window of eight on both levels
// (round 2): fine level K X 0.266 -> 0.245 ms, fused term 0.275 -> 0.263 ms; corner-node level (4 921 waves: one occupancy
// round instead of two) 30.4 -> 25.2 us.
__global__ void __launch_bounds__(64 * DS_UNION_WPB) __attribute__((amdgpu_waves_per_eu(DS_UNION_WAVES(EPI, BF))))
    spmm_union_kernel(const int2* __restrict__ utab, const int4* __restrict__ ctab, unsigned ngroups,
                      const int32_t* __restrict__ gent,
                      const float* __restrict__ kgrp, int64_t nnzb, int64_t nv, const float* __restrict__ X, int64_t ldx,
                      float* __restrict__ Y, int64_t ldy, int lpn_rt, unsigned nwg, ChebEpilogue epi) {
    // BF: X, R0, W_prev (and Y unless OUT32) are bf16 blocks (the float pointers are reinterpreted; leading dimensions
    // in elements); a lane's piece of a row is 4 columns = 8 bytes
    static_assert(!BF || (EPI == 1 || EPI == 2), "bf16 blocks: preconditioner epilogues only");
    static_assert(EPI >= 0 && EPI <= 6, "epilogues 0 .. 6");
    static_assert(EPI != 6 || (!BF && LVL == 0), "epilogue 6: fp32 operand, fine level");
    static_assert(!(BF && BIG), "bf16 blocks stay under one descriptor");
    constexpr int EB = BF ? 2 : 4;  // bytes per element of the vector blocks
    using f4 = __attribute__((ext_vector_type(4))) float;
    // panel loads in flight per wave (a power of two).  Measured on the bf16 variant, whose window registers are half
    // the size: 8 loads in flight at five waves per SIMD 0.251 ms against 0.246 ms with 4 - the term is not bound by
    // bytes in flight; six waves per SIMD (80 VGPRs, 64 bytes of scratch) 0.300 ms
    // (epilogue 4 at four waves per SIMD has the registers for a window of eight: measured 285 against 280 us, stays four)
    constexpr int UX = 4;
    // (the main loop runs without bounds tests: the highest entry index it touches is (last entry) + 3 UX - 1, and every index behind
    // a chunk's last entry must lie in the zero-filled tail of the LDS image)
    constexpr int PADE = UX > 4 ? 24 : UN_PAD;  // (a window of eight looks 23 entries ahead)
    static_assert(PADE >= 3 * UX - 1, "the zero tail of the entry image must cover the window's look-ahead");
    constexpr int NE = CAPB + PADE;          // entries of a group never exceed its blocks
    constexpr int NV16 = (CAPB + PADE) * 3;  // one 16-byte slot per (block, g)
    constexpr int NCI = (NE + 63) / 64;
    constexpr int NVI = (NV16 + 63) / 64;
    __shared__ int s_ent[DS_UNION_WPB][NE];
    // (node-scalar values need one float per block: 4 KB of LDS per workgroup instead of 27 KB, more waves per CU)
    __shared__ __attribute__((aligned(16))) float s_val[DS_UNION_WPB][EPI == 3 ? ((NE + 3) & ~3) : NV16 * 4];
    const int lpn = LPN_CT ? LPN_CT : lpn_rt;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const unsigned grp = ds::xcd_remap(blockIdx.x, nwg) * DS_UNION_WPB + wave;
    if (grp >= ngroups) return;  // wave-uniform
    // chunk range of the group: a chunk = a run of whole entries that fits the LDS images.  utab == nullptr: every
    // group is ONE chunk (ctab[grp]) - one dependent table read less at the head of every wave, which is what the
    // small corner-node level is made of
    int ch0 = (int)grp, ch1 = (int)grp + 1;
    if (utab) {
        const int2 ut = utab[grp];
        ch0 = __builtin_amdgcn_readfirstlane(ut.x), ch1 = __builtin_amdgcn_readfirstlane(ut.y);
    }
    const int64_t n0 = (int64_t)grp * UN_G;
    const int nn = (int)min<int64_t>(UN_G, nv - n0);
    const int g = lane / lpn;
    const int cl = lane - g * lpn;
    const bool active = g < 3;
    const int ga = active ? g : 0;
    const int c0 = cl * 4;
    // BIG: an operand block of >= 2 GB cannot be addressed by 32-bit offsets from ONE descriptor; every panel load then
    // gets its own descriptor (base = block + panel index * panel bytes, computed on the scalar unit; range = one
    // panel, so padding lanes at voffset PIPE_OOB still read zeros)
    const i4s xrsrc = make_rsrc_words(X, BIG ? (unsigned)(ldx * 12) : (unsigned)(3 * nv * ldx * EB));
    // ldx as ONE opaque scalar: left to itself the compiler sank the truncation of the 64-bit argument into both arms of the `active`
    // branch below, the phi that joined them counted as divergent, and panel_bytes - the SCALAR offset operand of every panel
    // load - was computed in a VGPR (an assembler error in the object build; an -S build shows nothing)
    int ldx32 = (int)ldx;
    asm volatile("" : "+s"(ldx32));
    const unsigned xvoff = active ? (unsigned)((g * ldx32 + c0) * EB) : (unsigned)PIPE_OOB;  // (a row of 3 panels fits 32 bits)
    const int panel_bytes = ldx32 * 3 * EB;
    constexpr bool SCALAR = EPI == 3;  // node-scalar values (M = M_s (x) I3): Y <- A X, one float per block
    // EPI 4, the eigensolver's residual in ONE walk of the unions (round 4): both K X and (M_s (x) I3) X of the same block X are
    // accumulated - the blocks' fourth coefficient slot carries the block's mass scalar - and the epilogue forms
    // R = K X - (M X) diag(lam) and this group's share of the column norms ||R_j||^2, ||X_j||^2: K X' and M X' of a new Ritz
    // block are consumed by nothing but the residual (kx_fresh), so neither goes to HBM, X' is gathered once instead of twice
    // and the separate residual pass over three blocks is gone.  Per output the K and M sums are formed exactly as epilogues 0
    // and 3 form them, so R equals the three-launch result bit for bit.
    // EPI 6: epilogue 4 for an iteration whose preconditioner is the bf16 two-level cycle.  Same walk, same sums, same norm partials;
    // instead of the fp32 rows of R it stores what the cycle's first launch (cheb_init16_kernel, precond16.hip) would make of them:
    // the bf16 copy R16 (in Y, leading dimension ldy in ELEMENTS) and the first Chebyshev iterate W1 = c T R as bf16 (epi.w1 /
    // epi.ldw1; T = the node's 3 x 3 block epi.dinv, c = epi.c2).  Nobody else reads the fp32 R on that route, so the init launch's
    // pass over it - 143 MB written here and read back there at 80 columns - is gone.  Both values equal the two-launch result
    // bit for bit: the same fp32 R, rounded by the same conversion, and ds::cheb_first_row on both sides.
    constexpr bool PRE = EPI == 6;
    constexpr bool RESID = EPI == 4 || PRE;
    // EPI 5 (round 5): the same two accumulations, both WRITTEN - Y = K X and Y2 = (M_s (x) I3) X of one block in one walk (the
    // eigensolver multiplies the raw preconditioned residuals by K and by M: one gather of W instead of two); Y2 / its leading
    // dimension travel in epi.nwork / epi.ldr.  Each product is formed exactly as epilogues 0 and 3 form it.
    constexpr bool BOTH = EPI == 5;
    constexpr bool KM = RESID || BOTH;  // the blocks' fourth coefficient slot carries the mass scalar
    const i4s rrsrc = make_rsrc_words(epi.r0, (EPI == 1 || EPI == 2) ? (BIG ? (unsigned)(epi.ldr * 12) : (unsigned)(3 * nv * epi.ldr * EB)) : 0u);
    const float* pvp = (EPI == 1 && epi.wprev) ? epi.wprev : Y;  // where W_{k-1} is read from
    const int64_t ldpv = (EPI == 1 && epi.wprev) ? epi.ldp : ldy;
    const i4s yrsrc = make_rsrc_words(pvp, BIG ? (unsigned)(ldpv * 12) : (unsigned)(3 * nv * ldpv * EB));
    const i4s drsrc = make_rsrc_words(epi.dinv, (EPI == 1 || PRE) ? (unsigned)(nv * 36) : 0u);
    const int rpanel_bytes = (int)(epi.ldr * 3 * EB), ypanel_bytes = (int)(ldpv * 3 * EB);
    int* se = s_ent[wave];
    float* svl = s_val[wave];

    // accumulators: they are only ever updated by inline-asm v_fma_f32 with a tied operand, so a
    // value never changes registers at a join (C++ FMAs under wave-uniform branches made the compiler hoist the
    // products out of the branches and merge / copy the accumulator vectors at every join)
    using f2 = __attribute__((ext_vector_type(2))) float;
    // NO PACKED FP32 (see DS_UFMA below): the accumulators are single floats, each a tied operand of its v_fma_f32
    float acc1[UN_G][3][4];
#pragma unroll
    for (int s_ = 0; s_ < UN_G; ++s_)
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int k = 0; k < 4; ++k) acc1[s_][i][k] = 0.f;
    float accm[UN_G][4];  // EPI 4: (M X) of the lane's own row (row g feeds row g only)
#pragma unroll
    for (int s_ = 0; s_ < UN_G; ++s_)
#pragma unroll
        for (int k = 0; k < 4; ++k) accm[s_][k] = 0.f;
    for (int ch = ch0; ch < ch1; ++ch) {  // almost always one chunk; the accumulators carry over
    const int4 ct = ctab[ch];
    const int e0 = __builtin_amdgcn_readfirstlane(ct.x);
    const int ne = __builtin_amdgcn_readfirstlane(ct.y) - e0;
    const int b0 = __builtin_amdgcn_readfirstlane(ct.z);
    const int nbk = __builtin_amdgcn_readfirstlane(ct.w) - b0;
    // ---------------- phase A: entries and coefficients of the group -> LDS
    // (a fresh lane id per chunk, opaque to the compiler: derived from the kernel's `lane` the staging offsets below were hoisted
    // out of the chunk loop and stayed live through phase B - a dozen VGPRs of the 96 that five waves per SIMD allow)
    int lane_a;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane_a));
    int es[NCI];
#pragma unroll
    for (int i = 0; i < NCI; ++i) {
        const int t = lane_a + 64 * i;
        es[i] = t < ne ? DS_STREAM_LOAD(LVL, gent + e0 + t) : 0;  // padding: mask 0 (no blocks), id 0
    }
    if (SCALAR) {  // one float per block; blocks behind the group's last (window padding) read as zero
        float ms_[NCI];
#pragma unroll
        for (int i = 0; i < NCI; ++i) {
            const int t = lane_a + 64 * i;
            ms_[i] = t < nbk ? DS_STREAM_LOAD(LVL, kgrp + (int64_t)b0 + t) : 0.f;
        }
#pragma unroll
        for (int i = 0; i < NCI; ++i)
            if (lane_a + 64 * i < NE) svl[lane_a + 64 * i] = ms_[i];
    } else {
        const int64_t vb = (int64_t)b0 * 36;
        const int64_t avail = nnzb * 36 - vb;
        const int want = (nbk + PADE) * 36;
        const i4s vw = make_rsrc_words(reinterpret_cast<const char*>(kgrp) + vb, (unsigned)(avail < want ? avail : want));
        f3v st[NVI];
#pragma unroll
        for (int i = 0; i < NVI; ++i) {
            const int vo = (lane_a + 64 * i) * 12;
            // (s_nop: descriptor words come from v_readfirstlane, see the batched kernel)
            if constexpr (LVL == 0)
                asm volatile("s_nop 4\n\tbuffer_load_dwordx3 %0, %1, %2, 0 offen nt" : "=v"(st[i]) : "v"(vo), "s"(vw) : "memory");
            else
                asm volatile("s_nop 4\n\tbuffer_load_dwordx3 %0, %1, %2, 0 offen" : "=v"(st[i]) : "v"(vo), "s"(vw) : "memory");
        }
        float mst[NVI];
        if (KM) {  // the block's mass scalar rides in the fourth float of each of its three coefficient slots (same round trip)
#pragma unroll
            for (int i = 0; i < NVI; ++i) {
                const int blk = (lane_a + 64 * i) / 3;
                mst[i] = blk < nbk ? DS_STREAM_LOAD(LVL, epi.mvals + (int64_t)b0 + blk) : 0.f;
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
        for (int i = 0; i < NVI; ++i) asm volatile("" : "+v"(st[i]));
#pragma unroll
        for (int i = 0; i < NVI; ++i)
            if (lane_a + 64 * i < NV16)
                reinterpret_cast<f4*>(svl)[lane_a + 64 * i] = f4{st[i][0], st[i][1], st[i][2], KM ? mst[i] : 0.f};
    }
#pragma unroll
    for (int i = 0; i < NCI; ++i)
        if (lane_a + 64 * i < NE) se[lane_a + 64 * i] = es[i];
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    // (a use of the entry registers on EVERY path: the compiler's wait for these loads sits inside the conditional store above,
    // and on the path around it its bookkeeping kept them "in flight" - it then put an s_waitcnt vmcnt(0) in front of every later
    // write to those registers, i.e. into the main loop, draining the gather window)
#pragma unroll
    for (int i = 0; i < NCI; ++i) asm volatile("" ::"v"(es[i]));
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

    // ---------------- phase B: rolling window over the union entries
    using xw_t = typename std::conditional<BF, i2s, f4>::type;  // a lane's piece of a panel row as loaded
    xw_t x[UX];
#pragma unroll
    for (int q = 0; q < UX; ++q) x[q] = xw_t{};
    auto load_ents = [&](int base) { return se[base + (lane & (UX - 1))]; };  // base + 7 < NE always
#define DS_UISSUE(q, entreg, lim)                                                                         \
    do {                                                                                                  \
        /* entries behind the chunk's last one are ZERO in the LDS image (mask 0, panel 0): their loads are ordinary in-range */ \
        /* loads of a hot panel, no bounds test and no special offset needed (round 3: ~8 scalar instructions per entry less) */  \
        const int e_ = __builtin_amdgcn_readlane(entreg, q) & 0x0fffffff;                                 \
        const unsigned vo_ = xvoff;                                                                       \
        if (BIG) {                                                                                        \
            const i4s rs_ = rebase_rsrc(xrsrc, e_, panel_bytes);                                          \
            asm volatile("buffer_load_dwordx4 %0, %1, %2, 0 offen" : "+v"(x[q]) : "v"(vo_), "s"(rs_) : "memory"); \
        } else if (BF) {                                                                                  \
            const int j_ = e_ * panel_bytes;                                                              \
            asm volatile("buffer_load_dwordx2 %0, %1, %2, %3 offen" : "+v"(x[q]) : "v"(vo_), "s"(xrsrc), "s"(j_) : "memory"); \
        } else {                                                                                          \
            const int j_ = e_ * panel_bytes;                                                              \
            asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 offen" : "+v"(x[q]) : "v"(vo_), "s"(xrsrc), "s"(j_) : "memory"); \
        }                                                                                                 \
    } while (0)
// acc_i += c_i * x for the three output rows: c = (c0, c1, c2, -) of one block, x the entry's panel piece
// Plain v_fma_f32, no v_pk_fma_f32: on gfx950 a v_mfma_f32_16x16x32_bf16 in flight in ANOTHER wave of the compute unit
// changes results of packed-FP32 instructions (tests/probes/mfma_probe.hip reproduces it with register-only kernels: a chain of
// v_pk_fma_f32 beside a spin of that MFMA returns wrong values, the same chain of v_fma_f32 never does;
// profiles/r03_mfma_interference_matrix.txt).  This library issues no such MFMA, but it cannot know what else runs on the
// device (a bf16 GEMM of another stream or process): its accumulation must not depend on that.
#define DS_UFMA1(a, xv, cv) asm volatile("v_fma_f32 %0, %1, %2, %0" : "+v"(a) : "v"(xv), "v"(cv))
#define DS_UFMA(S, c, xl, xh)                                                                                         \
    do {                                                                                                              \
        const float c0_ = c[0], c1_ = c[1], c2_ = c[2], x0_ = xl[0], x1_ = xl[1], x2_ = xh[0], x3_ = xh[1];           \
        DS_UFMA1(acc1[S][0][0], x0_, c0_); DS_UFMA1(acc1[S][0][1], x1_, c0_);                                          \
        DS_UFMA1(acc1[S][0][2], x2_, c0_); DS_UFMA1(acc1[S][0][3], x3_, c0_);                                          \
        DS_UFMA1(acc1[S][1][0], x0_, c1_); DS_UFMA1(acc1[S][1][1], x1_, c1_);                                          \
        DS_UFMA1(acc1[S][1][2], x2_, c1_); DS_UFMA1(acc1[S][1][3], x3_, c1_);                                          \
        DS_UFMA1(acc1[S][2][0], x0_, c2_); DS_UFMA1(acc1[S][2][1], x1_, c2_);                                          \
        DS_UFMA1(acc1[S][2][2], x2_, c2_); DS_UFMA1(acc1[S][2][3], x3_, c2_);                                          \
    } while (0)
#define DS_UFMA_S(S, m, xl, xh)                                                                                       \
    do {                                                                                                              \
        const float m_ = m, x0_ = xl[0], x1_ = xl[1], x2_ = xh[0], x3_ = xh[1];                                       \
        DS_UFMA1(acc1[S][0][0], x0_, m_); DS_UFMA1(acc1[S][0][1], x1_, m_);                                            \
        DS_UFMA1(acc1[S][0][2], x2_, m_); DS_UFMA1(acc1[S][0][3], x3_, m_);                                            \
    } while (0)
    int entC = load_ents(0);                   // entries being consumed (issued in the prologue)
    int entA = load_ents(min(UX, NE - UX));    // entries to issue during the first consume group
    asm volatile("s_nop 4" ::: "memory");
#pragma unroll
    for (int q = 0; q < UX; ++q) DS_UISSUE(q, entC, ne);
    // coefficient stream: the blocks of a chunk are consumed strictly in the order they are stored (entry-major, node-minor), so the
    // NEXT block's coefficients are always the next LDS slot, whichever node and entry it belongs to: they are read one block
    // ahead, during the FMAs of the current block (a read issued and waited for per block cost its full LDS latency every time:
    // profiles/r03_union_knockout.txt), and no block index has to be computed from the masks
    const f4* cptr = reinterpret_cast<const f4*>(svl) + ga;  // this lane's (c0, c1, c2) of the next block to fetch
    const float* sptr = svl;
    f3v cn = f3v{0.f, 0.f, 0.f};
    float sn = 0.f;
    if (SCALAR) sn = *sptr++;
    else if (KM) { const f4 c4_ = *cptr; cn = f3v{c4_[0], c4_[1], c4_[2]}, sn = c4_[3], cptr += 3; }
    else cn = *reinterpret_cast<const f3v*>(cptr), cptr += 3;
#define DS_CNEXT()                                                                                        \
    do {                                                                                                  \
        if (KM) { const f4 c4_ = *cptr; cn = f3v{c4_[0], c4_[1], c4_[2]}, sn = c4_[3]; }                  \
        else cn = *reinterpret_cast<const f3v*>(cptr);                                                    \
        cptr += 3;                                                                                        \
    } while (0)
#define DS_UFMA_M(S, m, xl, xh)                                                                           \
    do {                                                                                                  \
        const float m_ = m, x0_ = xl[0], x1_ = xl[1], x2_ = xh[0], x3_ = xh[1];                           \
        DS_UFMA1(accm[S][0], x0_, m_); DS_UFMA1(accm[S][1], x1_, m_);                                     \
        DS_UFMA1(accm[S][2], x2_, m_); DS_UFMA1(accm[S][3], x3_, m_);                                     \
    } while (0)
#define DS_SNEXT() do { sn = *sptr++; } while (0)
    for (int eu = 0; eu < ne; eu += UX) {
        const int entB = load_ents(min(eu + 2 * UX, NE - UX));
#pragma unroll
        for (int q = 0; q < UX; ++q) {
            const unsigned m = (unsigned)__builtin_amdgcn_readlane(entC, q) >> 28;  // (0 behind the last entry)
            DS_WAIT_VM(UX - 1, x[q]);
            f2 xl, xh;
            if constexpr (BF) {
                const f4 xf = unpack_bf16x4(x[q]);
                xl = __builtin_shufflevector(xf, xf, 0, 1), xh = __builtin_shufflevector(xf, xf, 2, 3);
            } else {
                xl = __builtin_shufflevector(x[q], x[q], 0, 1), xh = __builtin_shufflevector(x[q], x[q], 2, 3);
            }
            if (SCALAR) {
                if (m & 1u) { const float c = sn; DS_SNEXT(); DS_UFMA_S(0, c, xl, xh); }
                if (m & 2u) { const float c = sn; DS_SNEXT(); DS_UFMA_S(1, c, xl, xh); }
                if (m & 4u) { const float c = sn; DS_SNEXT(); DS_UFMA_S(2, c, xl, xh); }
                if (m & 8u) { const float c = sn; DS_SNEXT(); DS_UFMA_S(3, c, xl, xh); }
            } else {
                // (tried: the copy out of the prefetch registers as asm moves at the START of the block, so that the wait for the read
                // comes a whole block later - same time: the kernel is VALU-issue bound, not waiting on LDS any more)
                if constexpr (KM) {
                    if (m & 1u) { const f3v c = cn; const float cm = sn; DS_CNEXT(); DS_UFMA(0, c, xl, xh); DS_UFMA_M(0, cm, xl, xh); }
                    if (m & 2u) { const f3v c = cn; const float cm = sn; DS_CNEXT(); DS_UFMA(1, c, xl, xh); DS_UFMA_M(1, cm, xl, xh); }
                    if (m & 4u) { const f3v c = cn; const float cm = sn; DS_CNEXT(); DS_UFMA(2, c, xl, xh); DS_UFMA_M(2, cm, xl, xh); }
                    if (m & 8u) { const f3v c = cn; const float cm = sn; DS_CNEXT(); DS_UFMA(3, c, xl, xh); DS_UFMA_M(3, cm, xl, xh); }
                } else {
                if (m & 1u) { const f3v c = cn; DS_CNEXT(); DS_UFMA(0, c, xl, xh); }
                if (m & 2u) { const f3v c = cn; DS_CNEXT(); DS_UFMA(1, c, xl, xh); }
                if (m & 4u) { const f3v c = cn; DS_CNEXT(); DS_UFMA(2, c, xl, xh); }
                if (m & 8u) { const f3v c = cn; DS_CNEXT(); DS_UFMA(3, c, xl, xh); }
                }
            }
            DS_UISSUE(q, entA, ne - eu - UX);
            __builtin_amdgcn_sched_barrier(0);
        }
        entC = entA;
        entA = entB;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // trailing padding loads (and the window registers are free again)
    }  // chunks
#undef DS_UISSUE
#undef DS_CNEXT
#undef DS_SNEXT
#undef DS_UFMA
#undef DS_UFMA_S
#undef DS_UFMA_M
#undef DS_UFMA1

    // ---------------- the group's nodes: merge the row groups, epilogue, store
    {  // (a scope of its own: the names below shadow the head's)
    // The epilogue's lane constants are recomputed HERE from a fresh lane id (v_mbcnt: opaque, not hoistable): defined at
    // the head of the kernel they stayed live through the main loop, at 96 VGPRs two 64-bit address pairs of them went to
    // scratch (20 B per lane in every fp32 instantiation of rounds 1-2)
    int lane_e;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane_e));
    const int g = (lane_e >= lpn ? 1 : 0) + (lane_e >= 2 * lpn ? 1 : 0) + (lane_e >= 3 * lpn ? 1 : 0);  // (shadows the head's)
    const bool active = g < 3;
    const int ga = active ? g : 0;
    const int c0 = (lane_e - g * lpn) * 4;
    const unsigned rvoff = active ? (unsigned)((g * (int)epi.ldr + c0) * EB) : (unsigned)PIPE_OOB;
    const unsigned yvoff = active ? (unsigned)((g * (int)ldpv + c0) * EB) : (unsigned)PIPE_OOB;
    const unsigned dvoff = active ? (unsigned)(g * 12) : (unsigned)PIPE_OOB;
    int s1 = lane_e + lpn, s2 = lane_e + 2 * lpn;
    if (s1 >= 3 * lpn) s1 -= 3 * lpn;
    if (s2 >= 3 * lpn) s2 -= 3 * lpn;
    if (!active) s1 = s2 = lane_e;
    auto pull = [&](const f4& v, int src) -> f4 {
        f4 o;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float e = v[c];
            o[c] = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(src * 4, __builtin_bit_cast(int, e)));
        }
        return o;
    };
    f4 lamv = {0.f, 0.f, 0.f, 0.f}, nr2 = lamv, nx2 = lamv;  // EPI 4: Ritz values of the lane's columns; its share of the norms
    if constexpr (RESID) {
        if (active) {
#pragma unroll
            for (int c = 0; c < 4; ++c) lamv[c] = (float)epi.lam[c0 + c];
        }
    }
    // Epilogue operands: straight-line, unconditional loads into fresh registers ("=v").  Any branch or
    // zero-initialisation here makes the compiler merge values at a join, i.e. COPY registers whose load is still
    // in flight (seen in the ISA of the first version: wrong operands for slot 0).  A group with fewer than 4 nodes
    // re-reads its last node; W_prev is read even when it is not used (first term).  Two nodes at a time, to keep
    // the register peak of the kernel in the main loop.
#pragma unroll
    for (int h = 0; h < UN_G; h += 2) {
        f4 r0v[2], pv[2], wv[2];
        f3v drow[2];
        if constexpr (RESID) {  // the group's own rows of X (for ||X_j||^2), two nodes at a time
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int node = (int)n0 + min(h + k, nn - 1);
                if (BIG) {
                    const i4s rx_ = rebase_rsrc(xrsrc, node, panel_bytes);
                    asm volatile("buffer_load_dwordx4 %0, %1, %2, 0 offen" : "=v"(wv[k]) : "v"(xvoff), "s"(rx_) : "memory");
                } else {
                    const int sx = node * panel_bytes;
                    asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 offen" : "=v"(wv[k]) : "v"(xvoff), "s"(xrsrc), "s"(sx) : "memory");
                }
                if constexpr (PRE) {  // the lane's row of the node's block T
                    const int sd = node * 36;
                    asm volatile("buffer_load_dwordx3 %0, %1, %2, %3 offen" : "=v"(drow[k]) : "v"(dvoff), "s"(drsrc), "s"(sd) : "memory");
                }
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                asm volatile("" : "+v"(wv[k]));
                if constexpr (PRE) asm volatile("" : "+v"(drow[k]));
            }
        }
        if (EPI == 1 || EPI == 2) {
            if constexpr (BF) {  // 8-byte pieces, unpacked after the wait
                i2s r0w[2], pw[2], ww[2];
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    const int node = (int)n0 + min(h + k, nn - 1);
                    const int sd = node * 36, so = node * rpanel_bytes;
                    asm volatile("buffer_load_dwordx2 %0, %1, %2, %3 offen" : "=v"(r0w[k]) : "v"(rvoff), "s"(rrsrc), "s"(so) : "memory");
                    if (EPI == 1) {
                        const int sy = node * ypanel_bytes, sx = node * panel_bytes;
                        asm volatile("buffer_load_dwordx2 %0, %1, %2, %3 offen" : "=v"(pw[k]) : "v"(yvoff), "s"(yrsrc), "s"(sy) : "memory");
                        asm volatile("buffer_load_dwordx2 %0, %1, %2, %3 offen" : "=v"(ww[k]) : "v"(xvoff), "s"(xrsrc), "s"(sx) : "memory");
                        asm volatile("buffer_load_dwordx3 %0, %1, %2, %3 offen" : "=v"(drow[k]) : "v"(dvoff), "s"(drsrc), "s"(sd) : "memory");
                    }
                }
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    asm volatile("" : "+v"(r0w[k]));
                    if (EPI == 1) asm volatile("" : "+v"(pw[k]), "+v"(ww[k]), "+v"(drow[k]));
                    r0v[k] = unpack_bf16x4(r0w[k]);
                    if (EPI == 1) pv[k] = unpack_bf16x4(pw[k]), wv[k] = unpack_bf16x4(ww[k]);
                }
            } else {
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int node = (int)n0 + min(h + k, nn - 1);
                const int sd = node * 36;
                if (BIG) {
                    const i4s rr_ = rebase_rsrc(rrsrc, node, rpanel_bytes);
                    asm volatile("buffer_load_dwordx4 %0, %1, %2, 0 offen" : "=v"(r0v[k]) : "v"(rvoff), "s"(rr_) : "memory");
                    if (EPI == 1) {
                        const i4s ry_ = rebase_rsrc(yrsrc, node, ypanel_bytes), rx_ = rebase_rsrc(xrsrc, node, panel_bytes);
                        asm volatile("buffer_load_dwordx4 %0, %1, %2, 0 offen" : "=v"(pv[k]) : "v"(yvoff), "s"(ry_) : "memory");
                        asm volatile("buffer_load_dwordx4 %0, %1, %2, 0 offen" : "=v"(wv[k]) : "v"(xvoff), "s"(rx_) : "memory");
                        asm volatile("buffer_load_dwordx3 %0, %1, %2, %3 offen" : "=v"(drow[k]) : "v"(dvoff), "s"(drsrc), "s"(sd) : "memory");
                    }
                } else {
                    const int so = node * rpanel_bytes;
                    asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 offen" : "=v"(r0v[k]) : "v"(rvoff), "s"(rrsrc), "s"(so) : "memory");
                    if (EPI == 1) {
                        const int sy = node * ypanel_bytes, sx = node * panel_bytes;
                        asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 offen" : "=v"(pv[k]) : "v"(yvoff), "s"(yrsrc), "s"(sy) : "memory");
                        asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 offen" : "=v"(wv[k]) : "v"(xvoff), "s"(xrsrc), "s"(sx) : "memory");
                        asm volatile("buffer_load_dwordx3 %0, %1, %2, %3 offen" : "=v"(drow[k]) : "v"(dvoff), "s"(drsrc), "s"(sd) : "memory");
                    }
                }
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                asm volatile("" : "+v"(r0v[k]));
                if (EPI == 1) asm volatile("" : "+v"(pv[k]), "+v"(wv[k]), "+v"(drow[k]));
            }
            }
        }
        // a lane's piece of its output row: 16 bytes of an fp32 block, 8 bytes of a bf16 block
        auto store_piece = [&](int s_, const f4& v) {
            if constexpr (BF && !OUT32) {
                i2s* yp16 = reinterpret_cast<i2s*>(reinterpret_cast<char*>(Y) + (((n0 + s_) * 3 + ga) * ldy + c0) * 2);
                if (active) DS_STREAM_STORE(yp16, pack_bf16x4(v));
            } else {
                float* yp = Y + ((n0 + s_) * 3 + ga) * ldy + c0;
                if (active) DS_STREAM_STORE(reinterpret_cast<f4*>(yp), v);
            }
        };
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int s_ = h + k;
            if (s_ < nn) {  // wave-uniform
                const f4 a0 = {acc1[s_][0][0], acc1[s_][0][1], acc1[s_][0][2], acc1[s_][0][3]};
                const f4 a1 = {acc1[s_][1][0], acc1[s_][1][1], acc1[s_][1][2], acc1[s_][1][3]};
                const f4 a2 = {acc1[s_][2][0], acc1[s_][2][1], acc1[s_][2][2], acc1[s_][2][3]};
                if (SCALAR) {  // lane group g holds row g of the result already
                    store_piece(s_, a0);
                    continue;
                }
                const f4 own = g == 0 ? a0 : (g == 1 ? a1 : a2);
                const f4 pub1 = g == 0 ? a2 : (g == 1 ? a0 : a1);
                const f4 pub2 = g == 0 ? a1 : (g == 1 ? a2 : a0);
                const f4 tot = own + pull(pub1, s1) + pull(pub2, s2);
                if (EPI == 1) {
                    const f3v dr = drow[k];
                    const float d0 = g == 0 ? dr[0] : (g == 1 ? dr[1] : dr[2]);
                    const float d1 = g == 0 ? dr[1] : (g == 1 ? dr[2] : dr[0]);
                    const float d2 = g == 0 ? dr[2] : (g == 1 ? dr[0] : dr[1]);
                    const f4 q0 = r0v[k] - tot;
                    const f4 q1 = pull(q0, s1), q2 = pull(q0, s2);
                    const f4 t = d0 * q0 + d1 * q1 + d2 * q2;
                    f4 o = wv[k] + epi.c2 * t;
                    o += epi.first ? epi.c1 * wv[k] : epi.c1 * (wv[k] - pv[k]);
                    store_piece(s_, o);
                } else if (EPI == 2) {
                    store_piece(s_, r0v[k] - tot);
                } else if (BOTH) {
                    store_piece(s_, tot);
                    float* y2 = epi.nwork + ((n0 + s_) * 3 + ga) * epi.ldr + c0;
                    if (active) *reinterpret_cast<f4*>(y2) = f4{accm[s_][0], accm[s_][1], accm[s_][2], accm[s_][3]};
                } else if (RESID) {
                    // r = K x - lam (M x), formed as ds_residual forms it from the stored products (one fused multiply-add)
                    f4 r;
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        r[c] = __builtin_fmaf(-accm[s_][c], lamv[c], tot[c]);
                        nr2[c] += r[c] * r[c];
                        nx2[c] += wv[k][c] * wv[k][c];
                    }
                    if constexpr (PRE) {
                        // rows 0, 1, 2 of the node in every lane (the lane holds row g; s1 / s2 hold rows g + 1 / g + 2 mod 3)
                        const f4 p1 = pull(r, s1), p2 = pull(r, s2);
                        const f4 ra = g == 0 ? r : (g == 1 ? p2 : p1);
                        const f4 rb = g == 0 ? p1 : (g == 1 ? r : p2);
                        const f4 rc = g == 0 ? p2 : (g == 1 ? p1 : r);
                        const f3v dr = drow[k];
                        const f4 w = ds::cheb_first_row(epi.c2, dr[0], dr[1], dr[2], ra, rb, rc);
                        const int64_t row = (n0 + s_) * 3 + ga;
                        i2s* r16 = reinterpret_cast<i2s*>(reinterpret_cast<char*>(Y) + (row * ldy + c0) * 2);
                        i2s* w16 = reinterpret_cast<i2s*>(reinterpret_cast<char*>(epi.w1) + (row * epi.ldw1 + c0) * 2);
                        if (active) {
                            DS_STREAM_STORE(r16, pack_bf16x4(r));
                            DS_STREAM_STORE(w16, pack_bf16x4(w));
                        }
                    } else {
                        store_piece(s_, r);
                    }
                } else {
                    store_piece(s_, tot);
                }
            }
        }
    }
    if constexpr (RESID) {
        // the group's share of ||R_j||^2 and ||X_j||^2: the three row groups are added (lanes of row group 0 end with the
        // totals) and go to this group's row of the workspace - summed over the groups in a fixed order by
        // union_norm_reduce_kernel: no atomics, the norms are reproducible to the last bit (ds_residual's are not)
        const f4 tr = nr2 + pull(nr2, s1) + pull(nr2, s2), tx = nx2 + pull(nx2, s1) + pull(nx2, s2);
        if (active && g == 0) {
            const int ncols = lpn * 4;
            float* w = epi.nwork + (size_t)grp * 2 * ncols + c0;
            *reinterpret_cast<f4*>(w) = tr;
            *reinterpret_cast<f4*>(w + ncols) = tx;
        }
    }
    }  // epilogue scope
}

// column norms of the fused residual: partial[b][j] = sum over a contiguous share of the groups of work[grp][j] (fp64 sums of
// fp32 partials, j over the 2 x ncols columns), then out[j] = sum_b partial[b][j] - every sum in a fixed order.  A thread owns
// four columns (16-byte loads of coalesced rows) and every (256 / (ncols2 / 4))-th row of its block's share; the row lanes are
// added through LDS in lane order.  (First version: one thread per column walking 145 rows one dependent load after the other:
// 32 us per call, 1.5 % of a pass.)
constexpr int UN_NORM_BLOCKS = 256;
__global__ void __launch_bounds__(256) union_norm_partial_kernel(const float* __restrict__ work, unsigned ngroups, int ncols2,
                                                                 double* __restrict__ partial) {
    using f4 = __attribute__((ext_vector_type(4))) float;
    __shared__ double sm[256 * 4];
    const unsigned per = (ngroups + UN_NORM_BLOCKS - 1) / UN_NORM_BLOCKS;
    const unsigned g0 = blockIdx.x * per, g1 = min(ngroups, g0 + per);
    const int cg = ncols2 / 4, nrl = 256 / cg;  // column groups (ncols2 <= 168: at least 6 row lanes)
    const int rl = threadIdx.x / cg, c4 = threadIdx.x - rl * cg;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    if (rl < nrl)
        for (unsigned gi = g0 + rl; gi < g1; gi += nrl) {
            const f4 v = *reinterpret_cast<const f4*>(work + (size_t)gi * ncols2 + c4 * 4);
#pragma unroll
            for (int c = 0; c < 4; ++c) s[c] += (double)v[c];
        }
#pragma unroll
    for (int c = 0; c < 4; ++c) sm[threadIdx.x * 4 + c] = s[c];
    __syncthreads();
    for (int j = threadIdx.x; j < ncols2; j += blockDim.x) {
        double t = 0.0;
        for (int r = 0; r < nrl; ++r) t += sm[(r * cg + j / 4) * 4 + (j & 3)];
        partial[(size_t)blockIdx.x * ncols2 + j] = t;
    }
}
__global__ void __launch_bounds__(256) union_norm_final_kernel(const double* __restrict__ partial, int ncols, double* __restrict__ rn2,
                                                               double* __restrict__ xn2) {
    // one workgroup per output column: 256 partials, one per thread, added by a fixed tree
    __shared__ double sm[256];
    const int j = blockIdx.x;
    sm[threadIdx.x] = threadIdx.x < UN_NORM_BLOCKS ? partial[(size_t)threadIdx.x * 2 * ncols + j] : 0.0;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sm[threadIdx.x] += sm[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (j < ncols) rn2[j] = sm[0];
        else xn2[j - ncols] = sm[0];
    }
}

template <int LPN_CT, int EPI, bool BF = false, bool OUT32 = true, int LVL = 0>
int launch_union(const int32_t* utab, const int32_t* ctab, int64_t ngroups, int capb, const int32_t* gent, const float* kgrp, int64_t nnzb,
                 int64_t nv, const float* X, int64_t ldx, float* Y, int64_t ldy, int lpn, hipStream_t st, ChebEpilogue epi) {
    const int64_t nwg = ds::ceil_div(ngroups, DS_UNION_WPB);
    // (capb <= UN_CAPB is checked by the entry point: groups with more blocks are cut into chunks by the host tables)
    const int64_t ldmax = std::max(std::max(ldx, epi.ldr), std::max(ldy, epi.ldp));
    if constexpr (BF) {
        spmm_union_kernel<LPN_CT, EPI, UN_CAPB, false, true, OUT32, LVL><<<(unsigned)nwg, 64 * DS_UNION_WPB, 0, st>>>(
            reinterpret_cast<const int2*>(utab), reinterpret_cast<const int4*>(ctab), (unsigned)ngroups, gent, kgrp, nnzb,
            nv, X, ldx, Y, ldy, lpn, (unsigned)nwg, epi);
    } else if (3 * nv * ldmax * 4 >= (int64_t)PIPE_OOB) {  // an operand block beyond the reach of one descriptor
        spmm_union_kernel<LPN_CT, EPI, UN_CAPB, true, false, true, LVL><<<(unsigned)nwg, 64 * DS_UNION_WPB, 0, st>>>(
            reinterpret_cast<const int2*>(utab), reinterpret_cast<const int4*>(ctab), (unsigned)ngroups, gent, kgrp, nnzb,
            nv, X, ldx, Y, ldy, lpn, (unsigned)nwg, epi);
    } else {
        spmm_union_kernel<LPN_CT, EPI, UN_CAPB, false, false, true, LVL><<<(unsigned)nwg, 64 * DS_UNION_WPB, 0, st>>>(
            reinterpret_cast<const int2*>(utab), reinterpret_cast<const int4*>(ctab), (unsigned)ngroups, gent, kgrp, nnzb,
            nv, X, ldx, Y, ldy, lpn, (unsigned)nwg, epi);
    }
    DS_LAUNCH_CHECK("spmm_union_kernel");
    return DS_OK;
}
