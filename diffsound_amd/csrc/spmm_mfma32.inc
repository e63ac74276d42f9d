// fp32 matrix-core form of the eigensolver's OWN products: K W (3x3 blocks) and M W / M X (node-scalar mass values) on
// blocks of <= 84 columns.  Included from spmm_mfma32.hip (inside its anonymous namespace, after spmm_device.h whose vector
// types and load helpers it uses).  Replaces torch.sparse.mm(A, X) of the reference's solver
// (src/lobpcg/_linalg_utils.py:36-37) for the fp32 iterates.
//
// Why: the VALU neighbour-union kernel (spmm_union.inc) runs K W at 26.5 % of the HBM peak and its knock-out builds
// (profiles/r03_union_knockout.txt) show a serial per-wave chain - wait for a panel, test four mask bits, read a block's
// coefficients, 12 FMAs - with no unit saturated.  Here the chain is cut per BATCH of entries instead of per entry and
// the multiplications leave the vector unit:
//     D (16 x ncols) += A (16 x 4) B (4 x ncols)        v_mfma_f32_16x16x4_f32, exact fp32 (one rounding per product,
//                                                       a k-ordered fmaf chain: cdna_hip_programming.md, section 3)
//   rows  4 s + i : node s of the group of G = 4 consecutive nodes, output row i (i = 3: padding);
//   K index kg = 3 e + r : panel row r of union entry e, DENSELY packed - 4 entries fill 3 K-steps exactly, and the LDS
//           image of a batch (row-major panels, 3 rows per entry) IS the B operand: lane (k = lane >> 4, n = lane & 15)
//           reads row 4 j + k, column 16 t + n with one ds_read_b32 (rows 320 B apart: conflict-free), no transposed read;
//   A lane (m = lane & 15, k = lane >> 4) = K(s, e)[i][r] from the batch's compact fp32 blocks staged in LDS (36 B per
//           block, group / entry / node order: the tables of TetSystem.mfma_tables(4)), found through the entry's meta
//           word (presence mask | first block << 8); a zero slot where node s lacks neighbour e.  Node-scalar values
//           (EPI 3): A = m(s, e) [i == r], one float per block.
// WHAT IT COSTS.  The instruction runs at the fp32 VECTOR rate (64 FLOP per clock and SIMD), and the 16 x 4 A tile is
// mostly padding: one output row in four, and the union of 4 Morton-consecutive rows is filled to 0.43 (1.72 of 4 nodes
// per entry).  At C3 (2.40 M entries, 80 columns): 2.40 M x 3/4 K-steps x 5 column tiles = 9.0 M MFMAs x 32 cycles / 1 024
// SIMDs = 117 us at 2.4 GHz - this kernel is MATRIX-PIPE bound, not "free" (the 6 GFLOP of useful work are 38 us).  The
// 8-node unions of the bf16 kernel would need 13.4 M MFMAs (174 us): 4-node groups on purpose.  What the form buys is that
// the bound is a pipe that several waves keep busy, not a chain: the gathers (94 us alone), the LDS traffic and the
// address arithmetic of one wave run under the MFMAs of the others.
// Numerics: per output element the products are accumulated in the order kg = 0, 1, 2, ... (entry-major, panel row
// minor) in ONE fp32 chain; the VALU kernel keeps three chains (one per panel row) and adds them at the end.  Same
// arithmetic precision, different summation order: results agree to fp32 rounding (tests compare both with an fp64
// product), not bit for bit.
constexpr int MF32_G = 4;
// (knock-out builds - no MFMAs / no panel gathers / no B-fragment reads / no A-fragment chain - were made from the sources
// of the commit that introduced this file; their timings are profiles/r04_mfma32_knockout.txt)
#define DS_M32_PANEL_LOAD(dst, voff, rsrc, soff) \
    asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 offen" : "+v"(dst) : "v"(voff), "s"(rsrc), "s"(soff) : "memory")
// LDS is written as 16-byte pieces and read back as single floats: every LDS access of the kernel goes through
// may_alias types, so type-based alias analysis cannot move a read above the write that feeds it
typedef float __attribute__((may_alias)) mf32_f1;
typedef i4s __attribute__((may_alias)) mf32_i4;
typedef __attribute__((ext_vector_type(4))) float __attribute__((may_alias)) mf32_f4;
__host__ __device__ constexpr int mf32_row_stride(int nt) { return (nt | 1) * 64; }  // bytes; odd multiple of 64: rows k, k+1 on different banks
__host__ __device__ constexpr int mf32_panel_bytes(int nt, int eb) { return 3 * eb * mf32_row_stride(nt); }

constexpr int M32_DIAG_WAVES = 40000;
DS_DIAG_DECL(g_m32_dbg, M32_DIAG_WAVES)
template <int NT, int EPI, int EB, int LVL>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, EB == 8 ? 4 : 3)))
    spmm_union_mfma32_kernel(const int32_t* __restrict__ gptr, const int32_t* __restrict__ gcol,
                             const int32_t* __restrict__ gmeta, const int32_t* __restrict__ gbase,
                             const float* __restrict__ kv, unsigned kv_bytes, unsigned ngroups, int64_t nv,
                             const float* __restrict__ X, int64_t ldx, float* __restrict__ Y, int64_t ldy, int lpn,
                             int acap) {
    static_assert(EPI == 0 || EPI == 3, "fp32 MFMA form: plain products only (3x3 blocks or node scalars)");
    static_assert(EB == 8 || EB == 16, "batches of 8 or 16 entries");
    using f4 = __attribute__((ext_vector_type(4))) float;
    constexpr int G = MF32_G;
    constexpr int RS = mf32_row_stride(NT);      // LDS row stride of the panel image
    constexpr int PIMG = mf32_panel_bytes(NT, EB);
    constexpr int KSTEPS = 3 * EB / 4;           // K-steps of a full batch
    constexpr int VB = EPI == 3 ? 4 : 36;        // bytes per block of the value stream
    constexpr int NSTG = (EB * G * VB + 1023) / 1024;  // 16-byte staging pieces per lane
    constexpr int BPR = 64 / EB;                 // batches per 64-lane entry register
    static_assert(12 * NT * 64 <= PIMG, "the D exchange must fit the panel image");
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int lane = threadIdx.x;
    DS_DIAG_BEGIN();
    const unsigned grp = ds::xcd_remap(blockIdx.x, ngroups);
    const int e0 = __builtin_amdgcn_readfirstlane(gptr[grp]);
    const int ne = __builtin_amdgcn_readfirstlane(gptr[grp + 1]) - e0;
    const int b0 = __builtin_amdgcn_readfirstlane(gbase[grp]);
    const int64_t n0 = (int64_t)grp * G;
    const int nn = (int)min<int64_t>(G, nv - n0);
    // loader role: lane (g, cl) moves 16 bytes of row g of every panel
    const int g = lane / lpn;
    const int cl = lane - g * lpn;
    const bool active = g < 3;
    const int ga = active ? g : 0;
    const int c0 = cl * 4;
    const i4s xrsrc = make_rsrc_words(X, (unsigned)(3 * nv * ldx * 4));
    int ldx32 = (int)ldx;
    asm volatile("" : "+s"(ldx32));
    const unsigned xvoff = active ? (unsigned)((g * ldx32 + c0) * 4) : (unsigned)PIPE_OOB;
    const unsigned padvoff = lane == 0 ? 0u : (unsigned)PIPE_OOB;  // (a padding load keeps one lane in range: spmm_mfma.inc)
    const int panel_bytes = ldx32 * 12;
    const i4s krsrc = make_rsrc_words(kv, kv_bytes);
    // LDS traffic is plain C++ here (the compiler then counts every LDS operation in its own lgkmcnt waits); only the
    // vector-memory window is inline assembly.  Where this lane's piece of panel q goes: wr_off + q * wr_step; the four
    // idle lanes write to a trash slot behind the images (no EXEC games around the writes)
    const int wr_off = active ? ga * RS + cl * 16 : PIMG + acap + 16;
    const int wr_step = active ? 3 * RS : 0;
    // matrix-core role
    const int kq = lane >> 4, n_ = lane & 15, sn = n_ >> 2, ir = n_ & 3;
    const unsigned lbase = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)lds;  // LDS byte address of the image
    const unsigned baddr = lbase + (unsigned)(kq * RS + n_ * 4);
    // (the batch's blocks sit at PIMG, 16 zero bytes behind them at PIMG + acap)
    if (lane < 4) reinterpret_cast<mf32_f1*>(lds + PIMG + acap)[lane] = 0.f;
    // per phase ph of a super-step of 4 entries (3 K-steps): this lane's K index 4 ph + kq = 3 (entry) + (panel row)
    int eo[3], rr[3];
#pragma unroll
    for (int ph = 0; ph < 3; ++ph) {
        const int kg = 4 * ph + kq;
        eo[ph] = (kg * 11) >> 5;  // kg / 3 for kg < 12
        rr[ph] = kg - 3 * eo[ph];
    }

    f4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = f4{0.f, 0.f, 0.f, 0.f};

    // the group's union entries (column ids, meta words), up to 256: lane l of register i holds entry 64 i + l
    const i4s ersrc = make_rsrc_words(gcol + e0, (unsigned)(ne * 4));
    const i4s mrsrc = make_rsrc_words(gmeta + e0, (unsigned)(ne * 4));
    int ent0, ent1, ent2, ent3, met0, met1, met2, met3;
    {
        const unsigned v0 = (unsigned)(lane * 4), v1 = v0 + 256u, v2 = v0 + 512u, v3 = v0 + 768u;
        asm volatile("buffer_load_dword %0, %1, %2, 0 offen" : "=v"(ent0) : "v"(v0), "s"(ersrc) : "memory");
        asm volatile("buffer_load_dword %0, %1, %2, 0 offen" : "=v"(met0) : "v"(v0), "s"(mrsrc) : "memory");
        asm volatile("buffer_load_dword %0, %1, %2, 0 offen" : "=v"(ent1) : "v"(v1), "s"(ersrc) : "memory");
        asm volatile("buffer_load_dword %0, %1, %2, 0 offen" : "=v"(met1) : "v"(v1), "s"(mrsrc) : "memory");
        asm volatile("buffer_load_dword %0, %1, %2, 0 offen" : "=v"(ent2) : "v"(v2), "s"(ersrc) : "memory");
        asm volatile("buffer_load_dword %0, %1, %2, 0 offen" : "=v"(met2) : "v"(v2), "s"(mrsrc) : "memory");
        asm volatile("buffer_load_dword %0, %1, %2, 0 offen" : "=v"(ent3) : "v"(v3), "s"(ersrc) : "memory");
        asm volatile("buffer_load_dword %0, %1, %2, 0 offen" : "=v"(met3) : "v"(v3), "s"(mrsrc) : "memory");
        asm volatile("s_waitcnt vmcnt(0)"
                     : "+v"(ent0), "+v"(ent1), "+v"(ent2), "+v"(ent3), "+v"(met0), "+v"(met1), "+v"(met2), "+v"(met3)
                     :
                     : "memory");
    }
    const int nb = (ne + EB - 1) / EB;
    // Software pipeline as in spmm_mfma.inc: the loads of batch b + 1 (its blocks, then its panels) are issued as soon as
    // batch b sits in LDS and fly under batch b's fragment reads and MFMAs; the window registers are tied operands of their
    // loads, so a value never changes registers while its load is in flight.  (TWO batches deep - two register windows, 152
    // registers, three waves per SIMD - was built and measured: 292 us against 263; the waves still waited ~1 900 cycles per
    // batch: with more loads in flight a round trip only takes longer, profiles/r04_m32_diag.txt.)
    i4s sa[NSTG];
    i4s xa[EB];
#pragma unroll
    for (int i = 0; i < NSTG; ++i) sa[i] = i4s{0, 0, 0, 0};
#pragma unroll
    for (int q = 0; q < EB; ++q) xa[q] = i4s{0, 0, 0, 0};
#define DS_M32_ISSUE(BB, XW, SW)                                                                                         \
    do {                                                                                                                 \
        const int b_ = (BB);                                                                                             \
        const int cnt_ = min(EB, ne - b_ * EB);                                                                          \
        const int entreg_ = b_ < BPR ? ent0 : (b_ < 2 * BPR ? ent1 : (b_ < 3 * BPR ? ent2 : ent3));                      \
        const int metreg_ = b_ < BPR ? met0 : (b_ < 2 * BPR ? met1 : (b_ < 3 * BPR ? met2 : met3));                      \
        const int lq_ = (b_ & (BPR - 1)) * EB;                                                                           \
        const unsigned mf_ = (unsigned)__builtin_amdgcn_readlane(metreg_, lq_);                                          \
        const unsigned ml_ = (unsigned)__builtin_amdgcn_readlane(metreg_, lq_ + cnt_ - 1);                               \
        const int blk0_ = (int)(mf_ >> 8);                                                                               \
        const int abytes_ = ((int)(ml_ >> 8) + __builtin_popcount(ml_ & 0xffu) - blk0_) * VB;                            \
        _Pragma("unroll") for (int i = 0; i < NSTG; ++i) {                                                               \
            const int c = (lane + 64 * i) * 16;                                                                          \
            const unsigned vo = c < abytes_ ? (unsigned)((b0 + blk0_) * VB + c) : padvoff;                               \
            asm volatile("buffer_load_dwordx4 %0, %1, %2, 0 offen" : "+v"(SW[i]) : "v"(vo), "s"(krsrc) : "memory");      \
        }                                                                                                                \
        _Pragma("unroll") for (int q = 0; q < EB; ++q) {                                                                 \
            /* behind the batch's last entry: that entry's panel again (an ordinary in-range load of a hot panel, under  */ \
            /* zeros of A) - no padding offsets, and a NaN can only reach a group from its own neighbours                */ \
            const int e_ = __builtin_amdgcn_readlane(entreg_, lq_ + min(q, cnt_ - 1));                                   \
            const int so_ = e_ * panel_bytes;                                                                            \
            DS_M32_PANEL_LOAD(XW[q], xvoff, xrsrc, so_);                                                                 \
        }                                                                                                                \
    } while (0)
    // batch BB has landed: its panels and blocks go to LDS, then the window is free for batch BB + 1
#define DS_M32_LAND(BB, XW, SW)                                                                                          \
    do {                                                                                                                 \
        const int bl_ = (BB);                                                                                             \
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                                                 \
        _Pragma("unroll") for (int q = 0; q < EB; ++q) {                                                                 \
            asm volatile("" : "+v"(XW[q]));                                                                              \
            *reinterpret_cast<mf32_i4*>(lds + wr_off + q * wr_step) = XW[q];                                             \
        }                                                                                                                \
        const int abytes_l = batch_bytes(bl_);                                                                            \
        _Pragma("unroll") for (int i = 0; i < NSTG; ++i) {                                                               \
            asm volatile("" : "+v"(SW[i]));                                                                              \
            if (i * 1024 < abytes_l) /* wave-uniform */                                                                  \
                *reinterpret_cast<mf32_i4*>(lds + PIMG + (lane + 64 * i) * 16) = SW[i];                                  \
        }                                                                                                                \
        if (bl_ + 1 < nb) DS_M32_ISSUE(bl_ + 1, XW, SW); /* wave-uniform */                                                \
    } while (0)
    auto batch_meta = [&](int b_) { return b_ < BPR ? met0 : (b_ < 2 * BPR ? met1 : (b_ < 3 * BPR ? met2 : met3)); };
    auto batch_blk0 = [&](int b_) {
        return (int)((unsigned)__builtin_amdgcn_readlane(batch_meta(b_), (b_ & (BPR - 1)) * EB) >> 8);
    };
    auto batch_bytes = [&](int b_) {
        const int cnt = min(EB, ne - b_ * EB);
        const unsigned ml = (unsigned)__builtin_amdgcn_readlane(batch_meta(b_), (b_ & (BPR - 1)) * EB + cnt - 1);
        return ((int)(ml >> 8) + __builtin_popcount(ml & 0xffu) - batch_blk0(b_)) * VB;
    };
    // the multiplication of one landed batch (LDS -> fragments -> matrix cores); touches no window register
    auto multiply = [&](int b) __attribute__((always_inline)) {
        const int metreg = batch_meta(b);
        const int lbase_q = (b & (BPR - 1)) * EB;
        const int blk0 = batch_blk0(b);
        // A fragments of every K-step of the batch: the meta word of the lane's entry (cross-lane), then one LDS read.
        // THE FRAGMENT READS ARE INLINE ASSEMBLY WITH COUNTED WAITS: written as C++ loads, the compiler's scheduler folds any
        // read-ahead back into "read, wait, two MFMAs, read, wait ..." (it minimises live registers), every K-step then pays
        // three exposed LDS round trips and a wave spends ~3 700 cycles on the 960 cycles of MFMAs of a batch - four waves per
        // SIMD kept the matrix pipe 47 % busy (profiles/r04_mfma32_knockout.txt, first version: 263 us).
        unsigned mw[KSTEPS];
#pragma unroll
        for (int j = 0; j < KSTEPS; ++j)
            mw[j] = (unsigned)__builtin_amdgcn_ds_bpermute((lbase_q + 4 * (j / 3) + eo[j % 3]) * 4, metreg);
        float av[KSTEPS];
#pragma unroll
        for (int j = 0; j < KSTEPS; ++j) {
            const unsigned m_ = mw[j];
            const unsigned bit = 1u << sn;
            const int pos = (int)(m_ >> 8) - blk0 + __builtin_popcount(m_ & 0xfu & (bit - 1u));
            const bool have = (m_ & bit) != 0u && (EPI == 3 ? ir == rr[j % 3] : ir < 3);
            const int off = EPI == 3 ? pos * 4 : pos * 36 + (3 * ir + rr[j % 3]) * 4;
            const unsigned aa_ = lbase + (unsigned)(PIMG + (have ? off : acap));
            asm volatile("ds_read_b32 %0, %1" : "=v"(av[j]) : "v"(aa_) : "memory");
        }
        // B fragments: K-step j's NT reads are issued two steps ahead of its MFMAs into a ring of three register sets; before
        // step j's MFMAs at most the NT reads of step j + 1 may still be outstanding (LDS operations return in order, so that
        // also covers the A reads above).  Every K-step of every batch runs, branch-free: behind the batch's last entry A is
        // zero and B a finite panel (a wave-uniform skip per K-step made the compiler keep the accumulators in VGPRs and copy
        // them to the accumulator registers and back around every MFMA group).
        float bv[3][NT];
#define DS_M32_RD1(BUF, J, T)                                                                                   \
        if constexpr (NT > T)                                                                                      \
            asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(bv[BUF][T]) : "v"(baddr), "n"(4 * (J) * RS + (T) * 64) : "memory");
#define DS_M32_RD(J)                                                                                            \
        if constexpr ((J) < KSTEPS) {                                                                              \
            DS_M32_RD1((J) % 3, J, 0) DS_M32_RD1((J) % 3, J, 1) DS_M32_RD1((J) % 3, J, 2)                            \
            DS_M32_RD1((J) % 3, J, 3) DS_M32_RD1((J) % 3, J, 4) DS_M32_RD1((J) % 3, J, 5)                            \
        }
#define DS_M32_MFMA(A, B, C) C = __builtin_amdgcn_mfma_f32_16x16x4f32(A, B, C, 0, 0, 0)
#define DS_M32_STEP(J)                                                                                          \
        if constexpr ((J) < KSTEPS) {                                                                              \
            if constexpr ((J) + 1 < KSTEPS) asm volatile("s_waitcnt lgkmcnt(%0)" : : "n"(NT) : "memory");          \
            else asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                                \
            asm volatile("" : "+v"(av[J]));                                                                        \
            _Pragma("unroll") for (int t = 0; t < NT; ++t) asm volatile("" : "+v"(bv[(J) % 3][t]));                \
            _Pragma("unroll") for (int t = 0; t < NT; ++t) DS_M32_MFMA(av[J], bv[(J) % 3][t], acc[t]);             \
            DS_M32_RD((J) + 2)                                                                                     \
        }
        DS_M32_RD(0)
        DS_M32_RD(1)
        DS_M32_STEP(0) DS_M32_STEP(1) DS_M32_STEP(2) DS_M32_STEP(3) DS_M32_STEP(4) DS_M32_STEP(5)
        DS_M32_STEP(6) DS_M32_STEP(7) DS_M32_STEP(8) DS_M32_STEP(9) DS_M32_STEP(10) DS_M32_STEP(11)
#undef DS_M32_STEP
#undef DS_M32_RD
#undef DS_M32_RD1
    };
    if (nb > 0) DS_M32_ISSUE(0, xa, sa);
    DS_DIAG_MARK(0);
    for (int b = 0; b < nb; ++b) {
        DS_DIAG_MARK(1);
        DS_M32_LAND(b, xa, sa);
        DS_DIAG_MARK(2);
        multiply(b);
        // (the next batch's LDS writes cannot overtake these reads: LDS operations of one wave execute in order)
        DS_DIAG_MARK(3);
        DS_DIAG_ADD(0, 1, 2);  // wait for the batch + LDS writes + issue of the next
        DS_DIAG_ADD(2, 2, 3);  // fragments + MFMAs
    }
    DS_DIAG_MARK(3);
#undef DS_M32_LAND
#undef DS_M32_ISSUE
    // ---------------- D -> LDS in row-piece order (row 3 s + i of the group at byte (3 s + i) * DS_), then one 16-byte
    // piece per lane and node, as the epilogue of the other union kernels
    constexpr int DS_ = NT * 64;
    {
        mf32_f1* dl = reinterpret_cast<mf32_f1*>(lds);
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int j = 0; j < 3; ++j) dl[(3 * kq + j) * (DS_ / 4) + t * 16 + n_] = acc[t][j];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
#pragma unroll
    for (int s_ = 0; s_ < G; ++s_) {
        if (s_ < nn && active) {
            const f4 tot = *reinterpret_cast<const mf32_f4*>(lds + (3 * s_ + ga) * DS_ + c0 * 4);
            *reinterpret_cast<f4*>(Y + ((n0 + s_) * 3 + ga) * ldy + c0) = tot;
        }
    }
    DS_DIAG_END(g_m32_dbg, M32_DIAG_WAVES, lane);
}
