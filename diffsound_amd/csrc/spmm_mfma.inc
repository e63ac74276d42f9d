// MFMA form of the preconditioner's bf16 terms.  Included from spmm_mfma.hip (inside its anonymous namespace, after
// spmm_device.h whose descriptor and bf16 helpers it uses).
//
// The VALU kernel (spmm_union.inc) spends about as long multiplying as gathering: ~40 wave-instructions per union
// entry (10 packed FMAs, the coefficient reads, the bf16 unpack, the mask walk), ~90 us of vector-unit time per
// fine-level launch beside ~90 us of panel gathers and ~75 us of streams, and the three overlap badly.  Here the
// products run on the matrix cores: per group of G = 8 consecutive nodes (two 16-row tiles; G = 4: one)
//     D (16 x ncols) += A (16 x 32) B (32 x ncols),   K index  k = 4 e + r  (entry e of the group's union, panel row r,
//                                                     r = 3: padding), 8 entries per K-step, issued as two
//     v_mfma_f32_16x16x16_bf16 (see the note on the instruction choice below)
//   B = the gathered panels, bf16, from an LDS image of whole panels (row-major, 3 rows per entry) read with
//       ds_read_b64_tr_b16, which delivers the k-contiguous fragment the MFMA wants from the column-contiguous rows
//       (the lanes that stand for r = 3 point at row 2: finite numbers under a zero of A);
//   A = the group's 3x3 blocks spread over the union: row 4 s + i (node s of the tile, output row i; i = 3 zero),
//       column k, zero where node s does not have neighbour e.  A lane's fragment is two 8-byte rows
//       K(s, e)[i][0..3] (bf16, r = 3 zero) of the COMPACT block array kc (group / entry / node order, ds_pack_kc), found
//       through the entry's meta word (presence mask | first block << 8): no zero-padded image in HBM;
//   D lane (n, q): rows 4 q .. 4 q + 3 = node q of the tile, column n of each 16-column tile; it goes through LDS once
//       to reach the row-piece layout of the epilogue shared with the VALU kernel.
// One wave per workgroup and group; panels arrive in batches of MF_BATCH entries.  The union of 8
// Morton-consecutive rows has 0.43 x as many entries as the rows have blocks (0.58 x for 4).
// BATCH SIZE = OCCUPANCY.  Production runs DS_MF_BATCH = 16 (2 K-steps per batch): 128 VGPRs + 40 accumulator AGPRs = 3
// waves per SIMD and 10.6 KB of LDS per wave, against 212 + 40 registers = 2 waves with batches of 32.  Measured at C3,
// 80 columns, alone on the device: 171 us (32) -> 145 us (16) -> 144 us (8, four waves per SIMD: nothing more).  What
// did NOT help (round 3): persistent waves that walk a share of the groups and fetch the next group's header and
// entries under the current group's last batch (two of the four dependent round trips of a group gone): 174 / 155 us -
// the hardware's own dispatch of one-group workgroups hides those round trips as well and balances the groups better.
// INSTRUCTION CHOICE.  With v_mfma_f32_16x16x32_bf16 (gfx950's double-rate form) this kernel passed every test and yet
// the eigensolver's results changed from run to run once several hypothesis lanes shared the device: kernels of OTHER
// streams that accumulate with inline-asm v_pk_fma_f32 (the VALU neighbour-union kernels: K X, M X, the corner-node
// level's terms) returned results with one packed-FMA component wrong for a run of lanes while these MFMAs were in flight
// on the same CU.  Bisected with tools/stress_mix.py (profiles/r02_mfma_interference.txt): the corruption needs the
// MFMA instructions themselves (not the transposed reads, loads, LDS traffic or epilogue), it is independent of register
// allocation, LDS size and wait counts, and it disappears - 0 of 1 600 paired launches, bench loss bit-identical in 6 of
// 6 runs - with the 16x16x16 form, which costs 4 % of this kernel's time (the MFMAs are a small part of it).
using sh4v = __attribute__((ext_vector_type(4))) short;
// entries per LDS batch: a template parameter MF_BATCH (32: 4 K-steps per batch, two waves per SIMD; 16: 2 K-steps, half
// the load window and LDS image, three waves per SIMD; 8: one K-step, four waves)
// LDS of a wave (dynamic, 10 - 11 KB at 80 columns: the CU holds the 12 waves its registers allow):
// [panels: (MF_BATCH + TAIL) x 3 rows of the block's columns + slack | the batch's blocks: acap bytes | 8 zero bytes | trash]
__host__ __device__ inline int mf_panel_bytes(int ncols, int G, int MF_BATCH, int TAIL = 0) {
    const int p = (MF_BATCH + TAIL) * 3 * ncols * 2 + 128, d = 3 * G * ((ncols + 15) / 16) * 64;  // (D goes through the same space)
    return ((p > d ? p : d) + 15) & ~15;
}

// LVL (0: fine level, 1: corner-node level) changes nothing but the kernel's SYMBOL: a rocprofv3 kernel table then
// separates the two levels' launches (~150 us against ~17 us at C3) and their average durations mean something.
constexpr int MF_DIAG_WAVES = 40000;
DS_DIAG_DECL(g_mf_dbg, MF_DIAG_WAVES)
// TAIL (round 5): THE LAST BATCH OF A GROUP TAKES UP TO TAIL ENTRIES MORE THAN MF_BATCH.  89 % of the benchmark mesh's groups
// have 65 or 66 union entries: four full batches of 16 and a fifth for one or two entries - a whole dependent round trip for 3 %
// of the group's bytes (a build that simply dropped the entries behind the 64th ran 94 us against 106: profiles/
// r05_mf_tail.txt).  With TAIL = 2 the window holds 18 panel loads, of which the last two are padding loads in every batch but
// a group's last, the LDS image 18 panels, and the last batch runs a third K-step whose first two entry slots are the tail
// (the other six: zero blocks over the rows of slot 16).  Every entry keeps its K-step slot and its place in the order of
// accumulation, so results are bit-identical.  The registers come from the entry registers 2 and 3 (the TAIL form serves groups of
// up to 128 entries) and from one of the three staging pieces of the blocks (it stages 2 KiB per batch: 85 blocks); the entry point
// picks the form from max_entries and max_batch_blocks, TAIL = 0 serves up to 256 entries and 128 blocks per batch as before, and
// blocks of <= 48 columns (with fewer accumulator tiles the compiler spills the tail form at three waves per SIMD).
// The window's registers must be the SAME at both issue sites (in front of the loop, inside it): the index of the last trip is kept
// opaque so that the compiler cannot peel that trip off and join it through moves of registers whose loads are in flight
// (tests/test_cabi_cpu.py checks the shipped ISA).
// What did NOT help on top of it (profiles/r05_mf_tail.txt (5) - (7)): the epilogue's streamed operands asked for at the head of
// the wave by dropped loads (fine level 100 -> 107 us: the lines wait in the L2 in the place of re-used panels); the same operands
// asked for in the last trip's issue slot into the window's registers (live around the back edge BESIDE the window: 184 registers
// or spills).  A build whose epilogue reads nothing bounds any such work at 12 %.
template <int G, int NT, int EPI, bool OUT32, int MF_BATCH = 32, int LVL = 0, int TAIL = 0>
// (two waves per SIMD: the register file is there to be used - the compiler otherwise settles on 128 registers and
// spills the load window, whose registers must not move while their loads are in flight)
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu((MF_BATCH == 8 && NT < 6) ? 4 : ((TAIL > 0 && NT < 6) ? 3 : 1), MF_BATCH == 32 ? 2 : (MF_BATCH == 16 ? 3 : 4))))
    spmm_union_mfma_kernel(const int32_t* __restrict__ gptr, const int32_t* __restrict__ gcol,
                           const int32_t* __restrict__ gmeta, const int32_t* __restrict__ gbase,
                           const int32_t* __restrict__ ghead, const char* __restrict__ kc, int64_t nnzb, unsigned ngroups, int64_t nv,
                           const float* __restrict__ X, int64_t ldx, float* __restrict__ Y, int64_t ldy, int lpn,
                           int acap, ChebEpilogue epi) {
    using f4 = __attribute__((ext_vector_type(4))) float;
    constexpr int MT = G / 4;  // 16-row tiles of the group
    // the blocks of one batch: at most 8 nodes x MF_BATCH entries x 24 bytes; the TAIL form stages 2 KiB (85 blocks - the
    // benchmark mesh's fullest batch of 18 entries has 83; the entry point sends tables with fuller batches to TAIL = 0):
    // the staging piece it saves pays for the window's two extra loads
    constexpr int MF_ABYTES = TAIL ? 2048 : MF_BATCH * 8 * 24;
    constexpr int NSTG = (MF_ABYTES + 1023) / 1024;  // 16-byte staging pieces per lane
    constexpr int KS = MF_BATCH / 8;              // K-steps per batch
    constexpr int BPR = 64 / MF_BATCH;            // batches per 64-lane entry register
    constexpr int WIN = MF_BATCH + TAIL;          // panel loads of a batch
    static_assert(TAIL == 0 || (TAIL > 0 && TAIL <= 8 && MF_BATCH == 16), "a tail rides on batches of 16");
    // entry register that holds entry `gi` of the group (wave-uniform index)
#define DS_MF_ENT(gi) (TAIL ? ((gi) < 64 ? ent0 : ent1) : ((gi) < 64 ? ent0 : ((gi) < 128 ? ent1 : ((gi) < 192 ? ent2 : ent3))))
#define DS_MF_MET(gi) (TAIL ? ((gi) < 64 ? met0 : met1) : ((gi) < 64 ? met0 : ((gi) < 128 ? met1 : ((gi) < 192 ? met2 : met3))))
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int lane = threadIdx.x;
    DS_DIAG_BEGIN();
    const unsigned grp = ds::xcd_remap(blockIdx.x, ngroups);
#define DS_MF_TAB_LOAD(dst, voff, rsrc)                                                                                  \
    do {                                                                                                                 \
        if constexpr (LVL == 0)                                                                                          \
            asm volatile("buffer_load_dword %0, %1, %2, 0 offen nt" : "+v"(dst) : "v"(voff), "s"(rsrc) : "memory");      \
        else                                                                                                             \
            asm volatile("buffer_load_dword %0, %1, %2, 0 offen" : "+v"(dst) : "v"(voff), "s"(rsrc) : "memory");         \
    } while (0)
    // THE HEAD OF A WAVE IS ONE ROUND TRIP (round 5).  The group's first 64 union entries - column ids and meta words - sit in a
    // record of FIXED stride (ghead: 64 ids, 64 meta words, zero behind the group's last entry), so their loads need nothing but
    // the group's number and fly beside the scalar loads of the header (first entry, entry count, first block).  Until round 5
    // the entry loads waited for the header: two dependent round trips, 18 % of a wave's life (profiles/r04_m32_diag.txt),
    // before the first panel was asked for.  Entries 64 .. 255 of a larger group come from the compact arrays as before,
    // asked for when the header is there and needed from the fifth batch on.
    int ent0 = 0, ent1 = 0, ent2 = 0, ent3 = 0, met0 = 0, met1 = 0, met2 = 0, met3 = 0;
    {
        const i4s hrsrc = make_rsrc_words(ghead + (size_t)grp * 128, 512u);
        const unsigned v0 = (unsigned)(lane * 4), v1 = v0 + 256u;
        DS_MF_TAB_LOAD(ent0, v0, hrsrc);
        DS_MF_TAB_LOAD(met0, v1, hrsrc);
    }
    const int e0 = __builtin_amdgcn_readfirstlane(gptr[grp]);
#ifdef DS_MF_TRUNC  // TIMING EXPERIMENT ONLY (wrong results): what a group's time is without its last, nearly empty batch
    const int ne = min(__builtin_amdgcn_readfirstlane(gptr[grp + 1]) - e0, DS_MF_TRUNC);
#else
    const int ne = __builtin_amdgcn_readfirstlane(gptr[grp + 1]) - e0;
#endif
    const int b0 = __builtin_amdgcn_readfirstlane(gbase[grp]);
    const int64_t n0 = (int64_t)grp * G;
    const int nn = (int)min<int64_t>(G, nv - n0);
    const int g = lane / lpn;
    const int cl = lane - g * lpn;
    const bool active = g < 3;
    const int ga = active ? g : 0;
    const int c0 = cl * 4;
    const int ncols = lpn * 4;
    const int RS = ncols * 2;  // LDS row stride: the block's columns, compact
    const i4s xrsrc = make_rsrc_words(X, (unsigned)(3 * nv * ldx * 2));
    const unsigned xvoff = active ? (unsigned)(((int64_t)g * ldx + c0) * 2) : (unsigned)PIPE_OOB;
    // Padding loads must stay in the in-order return stream that the counted waits rely on: a load whose lanes are ALL
    // out of range makes no memory request and retires at once, ahead of older loads (seen as results that changed from
    // run to run when other kernels shared the device).  Lane 0 of a padding load reads offset 0 of its operand instead.
    const unsigned padvoff = lane == 0 ? 0u : (unsigned)PIPE_OOB;
    const int panel_bytes = (int)(ldx * 6);
    const i4s rrsrc = make_rsrc_words(epi.r0, (unsigned)(3 * nv * epi.ldr * 2));
    const float* pvp = (EPI == 1 && epi.wprev) ? epi.wprev : Y;
    const int64_t ldpv = (EPI == 1 && epi.wprev) ? epi.ldp : ldy;
    const i4s yrsrc = make_rsrc_words(pvp, (unsigned)(3 * nv * ldpv * 2));
    const i4s drsrc = make_rsrc_words(epi.dinv, EPI == 1 ? (unsigned)(nv * 36) : 0u);
    const i4s krsrc = make_rsrc_words(kc, (unsigned)(nnzb * 24));
    const unsigned rvoff = active ? (unsigned)(((int64_t)g * epi.ldr + c0) * 2) : (unsigned)PIPE_OOB;
    const unsigned yvoff = active ? (unsigned)(((int64_t)g * ldpv + c0) * 2) : (unsigned)PIPE_OOB;
    const unsigned dvoff = active ? (unsigned)(g * 12) : (unsigned)PIPE_OOB;
    const int rpanel_bytes = (int)(epi.ldr * 6), ypanel_bytes = (int)(ldpv * 6);
    const unsigned lbase = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)lds;  // LDS byte address of the image
    // where this lane's piece of panel `slot` goes: wr_addr + slot * wr_step; the four idle lanes write to a trash slot
    // behind the images (no EXEC games around the writes)
    const int pbytes = mf_panel_bytes(ncols, G, MF_BATCH, TAIL);
    const unsigned wr_addr = active ? lbase + (unsigned)(ga * RS + cl * 8) : lbase + (unsigned)(pbytes + acap + 8);
    const unsigned wr_step = active ? (unsigned)(3 * RS) : 0u;
    // transposed read: lane 4 q + p of the 16-lane group kq supplies row q of entry 2 kq (+ 1 for the second half),
    // columns 4 p .. 4 p + 3; q = 3 (the padding row of K) re-reads row 2
    const int kq = lane >> 4, tq = (lane >> 2) & 3, tp = lane & 3;
    const unsigned tr_addr = lbase + (unsigned)((6 * kq + min(tq, 2)) * RS + tp * 8);
    // A fragment: this lane holds row ir of the blocks of node sn of each tile
    const int sn = (lane & 15) >> 2, ir = lane & 3;
    const unsigned a_addr = lbase + (unsigned)pbytes;  // the batch's blocks; 8 zero bytes behind them
    if (lane == 0) *reinterpret_cast<int2*>(lds + pbytes + acap) = int2{0, 0};

    f4 acc[MT][NT];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[m][t] = f4{0.f, 0.f, 0.f, 0.f};

    // entries 64 .. 255 (lane l of register i holds entry 64 i + l; beyond the group's last entry the loads return zeros:
    // meta 0 = no blocks).  Only registers that hold an entry are asked for: a load whose lanes are ALL out of range retires
    // at once, ahead of older loads, and the counted wait below would then let the head loads through unfinished.
    const int nreg = (ne + 63) >> 6;  // wave-uniform
    if (nreg > 1) {
        const i4s ersrc = make_rsrc_words(gcol + e0, (unsigned)(ne * 4));
        const i4s mrsrc = make_rsrc_words(gmeta + e0, (unsigned)(ne * 4));
        const unsigned v1 = (unsigned)(lane * 4) + 256u, v2 = v1 + 256u, v3 = v2 + 256u;
        DS_MF_TAB_LOAD(ent1, v1, ersrc);
        DS_MF_TAB_LOAD(met1, v1, mrsrc);
        if constexpr (TAIL == 0) {
            if (nreg > 2) {
                DS_MF_TAB_LOAD(ent2, v2, ersrc);
                DS_MF_TAB_LOAD(met2, v2, mrsrc);
            }
            if (nreg > 3) {
                DS_MF_TAB_LOAD(ent3, v3, ersrc);
                DS_MF_TAB_LOAD(met3, v3, mrsrc);
            }
        }
    }
    // the head's two loads have landed when at most the 2 (nreg - 1) younger ones are outstanding (in-order return)
    // (the waits carry NO operands: with the registers tied to them the compiler joins the branches through copies - made
    // BEFORE the wait, of registers whose load is still in flight; the one statement behind the join marks the new values)
    if (nreg <= 1)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    else if (nreg == 2)
        asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
    else if (nreg == 3)
        asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else
        asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    asm volatile("" : "+v"(ent0), "+v"(met0) : : "memory");
    // batches: MF_BATCH entries each; the last one takes what is left, up to MF_BATCH + TAIL
    const int nb = ne <= 0 ? 0 : max(1, (ne - TAIL + MF_BATCH - 1) / MF_BATCH);
    // (the index of the last batch as an OPAQUE scalar: knowing that it is the loop's last trip the compiler peels that trip off -
    // and joins the peeled copy to the loop through moves of the window's registers, whose loads are in flight)
    int lastb = nb - 1;
    asm volatile("" : "+s"(lastb));
    // Software pipeline: the loads of batch b + 1 (its blocks, then its panels) are issued as soon as batch b sits in LDS
    // and fly under batch b's fragment reads and MFMAs.  The window registers are tied operands ("+v") of the loads: a
    // value never changes registers at the loop latch (a copy there would read registers whose load is still in flight).
    i4s stg[NSTG];
    i2s x[WIN];
#pragma unroll
    for (int i = 0; i < NSTG; ++i) stg[i] = i4s{0, 0, 0, 0};
#pragma unroll
    for (int q = 0; q < WIN; ++q) x[q] = i2s{0, 0};
    // (a macro, not a lambda: captured by reference the window arrays end up in scratch memory)
#define DS_MF_ISSUE(BB)                                                                                                  \
    do {                                                                                                                 \
        const int b_ = (BB);                                                                                             \
        const int cnt_ = min(MF_BATCH + (b_ == lastb ? TAIL : 0), ne - b_ * MF_BATCH);                                  \
        const int entreg_ = DS_MF_ENT(b_ * MF_BATCH);                                                                    \
        const int metreg_ = DS_MF_MET(b_ * MF_BATCH);                                                                    \
        const int lq_ = (b_ & (BPR - 1)) * MF_BATCH;                                                                     \
        const int gl_ = b_ * MF_BATCH + cnt_ - 1; /* the batch's last entry (a tail entry may sit in the next register) */ \
        /* the batch's blocks are contiguous in kc (entry-major order): coalesced 16-byte loads, staged through LDS; */  \
        /* the fragments are then 8-byte LDS reads (direct 8-byte gathers from HBM ran the address unit dry)         */  \
        const unsigned mf_ = (unsigned)__builtin_amdgcn_readlane(metreg_, lq_);                                          \
        const unsigned ml_ = (unsigned)__builtin_amdgcn_readlane(DS_MF_MET(gl_), gl_ & 63);                              \
        const int blk0_ = (int)(mf_ >> 8);                                                                               \
        const int abytes_ = ((int)(ml_ >> 8) + __builtin_popcount(ml_ & 0xffu) - blk0_) * 24;                            \
        int cntv_ = cnt_;                                                                                                \
        asm volatile("" : "+v"(cntv_));                                                                                  \
        _Pragma("unroll") for (int i = 0; i < NSTG; ++i) {                                                   \
            const int c = (lane + 64 * i) * 16;                                                                          \
            const unsigned vo = c < abytes_ ? (unsigned)((b0 + blk0_) * 24 + c) : padvoff;                              \
            if constexpr (LVL == 0)  /* (the value stream is read once per launch: non-temporal, see spmm_union.inc) */           \
                asm volatile("buffer_load_dwordx4 %0, %1, %2, 0 offen nt" : "+v"(stg[i]) : "v"(vo), "s"(krsrc) : "memory");      \
            else                                                                                                              \
                asm volatile("buffer_load_dwordx4 %0, %1, %2, 0 offen" : "+v"(stg[i]) : "v"(vo), "s"(krsrc) : "memory");         \
        }                                                                                                                \
        _Pragma("unroll") for (int q = 0; q < WIN; ++q) {                                                                \
            /* entries beyond the batch's last: a padding load (finite B rows under zero A); the compare is on a VECTOR */ \
            /* copy of the count so that it becomes a v_cndmask, not a branch per load                                   */ \
            const int gq_ = b_ * MF_BATCH + q;                                                                           \
            const int e_ = q < MF_BATCH ? __builtin_amdgcn_readlane(entreg_, lq_ + q)                                    \
                                        : __builtin_amdgcn_readlane(DS_MF_ENT(gq_), gq_ & 63);                           \
            const unsigned vo_ = q < cntv_ ? xvoff : padvoff;                                                            \
            const int so_ = e_ * panel_bytes;                                                                            \
            asm volatile("buffer_load_dwordx2 %0, %1, %2, %3 offen" : "+v"(x[q]) : "v"(vo_), "s"(xrsrc), "s"(so_) : "memory"); \
        }                                                                                                                \
    } while (0)
    if (nb > 0) DS_MF_ISSUE(0);
    DS_DIAG_MARK(0);
    for (int b = 0; b < nb; ++b) {
        DS_DIAG_MARK(1);
        const int cnt = min(MF_BATCH + (b == lastb ? TAIL : 0), ne - b * MF_BATCH);
        const int kst = (cnt + 7) >> 3;  // K-steps of this batch: 8 entries each
        const int metreg = DS_MF_MET(b * MF_BATCH);
        const int lbase_q = (b & (BPR - 1)) * MF_BATCH;
        const int gl = b * MF_BATCH + cnt - 1;
        const unsigned mf = (unsigned)__builtin_amdgcn_readlane(metreg, lbase_q);
        const unsigned ml = (unsigned)__builtin_amdgcn_readlane(DS_MF_MET(gl), gl & 63);
        const int blk0 = (int)(mf >> 8);
        const int abytes = ((int)(ml >> 8) + __builtin_popcount(ml & 0xffu) - blk0) * 24;
        // panels -> LDS as they land (in-order return: "at most N younger loads outstanding" proves a load complete)
#define DS_MF_WRITE8(Q0, N)                                                                         \
        asm volatile("s_waitcnt vmcnt(%0)" : : "n"(N) : "memory");                                     \
        _Pragma("unroll") for (int q = Q0; q < Q0 + 8; ++q) {                                          \
            asm volatile("" : "+v"(x[q]));                                                             \
            const unsigned a_ = wr_addr + (unsigned)(q * wr_step);                                     \
            asm volatile("ds_write_b64 %0, %1" : : "v"(a_), "v"(x[q]) : "memory");                     \
        }
        if constexpr (MF_BATCH == 32) {
            DS_MF_WRITE8(0, 24)
            DS_MF_WRITE8(8, 16)
            DS_MF_WRITE8(16, 8)
            DS_MF_WRITE8(24, 0)
        } else if constexpr (MF_BATCH == 16) {
            DS_MF_WRITE8(0, 8 + TAIL)
            DS_MF_WRITE8(8, TAIL)
            if constexpr (TAIL > 0) {
                // the tail slots: real panels in a group's last batch only.  That batch also waits for its padding loads: behind
                // the loop the window's registers are dead to the compiler, and nothing may still be in flight into them
                if (b == lastb) {  // wave-uniform
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    if (cnt > MF_BATCH) {
#pragma unroll
                        for (int q = MF_BATCH; q < WIN; ++q) {
                            asm volatile("" : "+v"(x[q]));
                            const unsigned a_ = wr_addr + (unsigned)(q * wr_step);
                            asm volatile("ds_write_b64 %0, %1" : : "v"(a_), "v"(x[q]) : "memory");
                        }
                    }
                }
            }
        } else {
            DS_MF_WRITE8(0, 0)
        }
#undef DS_MF_WRITE8
        // (everything older than this batch's panels has landed too: the entry registers 1 .. 3 are valid from here on)
        if constexpr (TAIL == 0)
            asm volatile("" : "+v"(ent1), "+v"(ent2), "+v"(ent3), "+v"(met1), "+v"(met2), "+v"(met3));
        else
            asm volatile("" : "+v"(ent1), "+v"(met1));
#pragma unroll
        for (int i = 0; i < NSTG; ++i) {
            asm volatile("" : "+v"(stg[i]));
            if (i * 1024 < abytes) {  // wave-uniform
                const unsigned a_ = a_addr + (unsigned)((lane + 64 * i) * 16);
                asm volatile("ds_write_b128 %0, %1" : : "v"(a_), "v"(stg[i]) : "memory");
            }
        }
        if (b + 1 < nb) DS_MF_ISSUE(b + 1);  // wave-uniform
        DS_DIAG_MARK(2);
        // A fragments: per K-step and half the meta word of the lane's entry, then per tile the 8-byte row of the block of
        // (node, entry) - or the zero slot when the node does not have that neighbour
        i2s alo[KS][MT], ahi[KS][MT];
        unsigned mw[2 * KS];  // (all the cross-lane reads first: issued one by one each waits for its own result)
#pragma unroll
        for (int j = 0; j < 2 * KS; ++j)
            mw[j] = (unsigned)__builtin_amdgcn_ds_bpermute((lbase_q + 8 * (j >> 1) + 2 * kq + (j & 1)) * 4, metreg);
#pragma unroll
        for (int s_ = 0; s_ < KS; ++s_)
#pragma unroll
            for (int hh = 0; hh < 2; ++hh) {
                const unsigned mwj = mw[2 * s_ + hh];  // meta word of this lane's entry 8 s + 2 kq + hh of the batch
#pragma unroll
                for (int m = 0; m < MT; ++m) {
                    const unsigned bit = 1u << (4 * m + sn);
                    const int pos = (int)(mwj >> 8) - blk0 + __builtin_popcount(mwj & (bit - 1u));
                    const bool have = (mwj & bit) != 0u && ir < 3 && s_ < kst;
                    const unsigned la = have ? a_addr + (unsigned)(pos * 24 + ir * 8) : a_addr + (unsigned)acap;
                    if (hh == 0)
                        asm volatile("ds_read_b64 %0, %1" : "=v"(alo[s_][m]) : "v"(la) : "memory");
                    else
                        asm volatile("ds_read_b64 %0, %1" : "=v"(ahi[s_][m]) : "v"(la) : "memory");
                }
            }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
        for (int s_ = 0; s_ < KS; ++s_)
#pragma unroll
            for (int m = 0; m < MT; ++m) asm volatile("" : "+v"(alo[s_][m]), "+v"(ahi[s_][m]));
#pragma unroll
        for (int s_ = 0; s_ < KS; ++s_) {
            if (s_ < kst) {  // wave-uniform: EXEC stays all ones for the transposed reads
                const unsigned r0a = tr_addr + (unsigned)(s_ * 24 * RS), r1a = r0a + (unsigned)(3 * RS);
                i2s blo[NT], bhi[NT];
#define DS_MF_TR(T)                                                                                          \
                if constexpr (NT > T) {                                                                         \
                    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(blo[T]) : "v"(r0a), "n"(T * 32) : "memory"); \
                    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(bhi[T]) : "v"(r1a), "n"(T * 32) : "memory"); \
                }
                DS_MF_TR(0) DS_MF_TR(1) DS_MF_TR(2) DS_MF_TR(3) DS_MF_TR(4) DS_MF_TR(5)
#undef DS_MF_TR
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    asm volatile("" : "+v"(blo[t]), "+v"(bhi[t]));
#pragma unroll
                    for (int m = 0; m < MT; ++m) {
                        acc[m][t] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(__builtin_bit_cast(sh4v, alo[s_][m]),
                                                                              __builtin_bit_cast(sh4v, blo[t]), acc[m][t], 0, 0, 0);
                        acc[m][t] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(__builtin_bit_cast(sh4v, ahi[s_][m]),
                                                                              __builtin_bit_cast(sh4v, bhi[t]), acc[m][t], 0, 0, 0);
                    }
                }
            }
        }
        if constexpr (TAIL > 0) {
            if (cnt > MF_BATCH) {  // wave-uniform: the tail K-step of a group's last batch
                // entry slots MF_BATCH .. MF_BATCH + 7 of the batch: the first TAIL hold the tail (lanes with kq = 0), the others
                // zero blocks; every 16-lane group reads the rows of slots MF_BATCH, MF_BATCH + 1 (finite numbers under the zeros)
                const int gt = b * MF_BATCH + MF_BATCH;
                const int treg = DS_MF_MET(gt);
                i2s tlo[MT], thi[MT];
#pragma unroll
                for (int hh = 0; hh < 2; ++hh) {
                    const unsigned mwj = (unsigned)__builtin_amdgcn_ds_bpermute(((gt & 63) + 2 * kq + hh) * 4, treg);
#pragma unroll
                    for (int m = 0; m < MT; ++m) {
                        const unsigned bit = 1u << (4 * m + sn);
                        const int pos = (int)(mwj >> 8) - blk0 + __builtin_popcount(mwj & (bit - 1u));
                        const bool have = (mwj & bit) != 0u && ir < 3 && 2 * kq + hh < TAIL;
                        const unsigned la = have ? a_addr + (unsigned)(pos * 24 + ir * 8) : a_addr + (unsigned)acap;
                        if (hh == 0)
                            asm volatile("ds_read_b64 %0, %1" : "=v"(tlo[m]) : "v"(la) : "memory");
                        else
                            asm volatile("ds_read_b64 %0, %1" : "=v"(thi[m]) : "v"(la) : "memory");
                    }
                }
                const unsigned t0a = lbase + (unsigned)((3 * MF_BATCH + min(tq, 2)) * RS + tp * 8), t1a = t0a + (unsigned)(3 * RS);
                i2s blo[NT], bhi[NT];
#define DS_MF_TR(T)                                                                                          \
                if constexpr (NT > T) {                                                                         \
                    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(blo[T]) : "v"(t0a), "n"(T * 32) : "memory"); \
                    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(bhi[T]) : "v"(t1a), "n"(T * 32) : "memory"); \
                }
                DS_MF_TR(0) DS_MF_TR(1) DS_MF_TR(2) DS_MF_TR(3) DS_MF_TR(4) DS_MF_TR(5)
#undef DS_MF_TR
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
                for (int m = 0; m < MT; ++m) asm volatile("" : "+v"(tlo[m]), "+v"(thi[m]));
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    asm volatile("" : "+v"(blo[t]), "+v"(bhi[t]));
#pragma unroll
                    for (int m = 0; m < MT; ++m) {
                        acc[m][t] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(__builtin_bit_cast(sh4v, tlo[m]),
                                                                              __builtin_bit_cast(sh4v, blo[t]), acc[m][t], 0, 0, 0);
                        acc[m][t] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(__builtin_bit_cast(sh4v, thi[m]),
                                                                              __builtin_bit_cast(sh4v, bhi[t]), acc[m][t], 0, 0, 0);
                    }
                }
            }
        }
        DS_DIAG_MARK(3);
        DS_DIAG_ADD(0, 1, 2);  // wait for the batch + LDS writes + issue of the next
        DS_DIAG_ADD(2, 2, 3);  // fragments + MFMAs
    }
#undef DS_MF_ISSUE
#undef DS_MF_ENT
#undef DS_MF_MET
    DS_DIAG_MARK(3);
    // Epilogue operands of all the group's nodes (R0, W_prev, W, T) in ONE round trip, under the exchange of D through
    // LDS (issued at the head of the kernel they cost 72 registers for its whole length and one wave per SIMD, and gained
    // nothing).  A group with fewer than G nodes re-reads its last node.
    i2s r0w[G], pw[G], ww[G];
    f3v drow[G];
#pragma unroll
    for (int k = 0; k < G; ++k) {
        const int node = (int)n0 + min(k, nn - 1);
        const int sd = node * 36, so = node * rpanel_bytes;
        // (R0 and W_prev are read once per launch, but a non-temporal hint on THESE loads costs 6 % on the fine level and on the
        // corner-node level: profiles/r05_nt_epi_ab.txt - the hint stays on the value / table streams and on the stores)
        asm volatile("buffer_load_dwordx2 %0, %1, %2, %3 offen" : "=v"(r0w[k]) : "v"(rvoff), "s"(rrsrc), "s"(so) : "memory");
        if (EPI == 1) {
            const int sy = node * ypanel_bytes, sx = node * panel_bytes;
            asm volatile("buffer_load_dwordx2 %0, %1, %2, %3 offen" : "=v"(pw[k]) : "v"(yvoff), "s"(yrsrc), "s"(sy) : "memory");
            asm volatile("buffer_load_dwordx2 %0, %1, %2, %3 offen" : "=v"(ww[k]) : "v"(xvoff), "s"(xrsrc), "s"(sx) : "memory");
            asm volatile("buffer_load_dwordx3 %0, %1, %2, %3 offen" : "=v"(drow[k]) : "v"(dvoff), "s"(drsrc), "s"(sd) : "memory");
        }
    }
    // ---------------- D -> LDS in row-piece order: row 3 s + i of the group at byte (3 s + i) * DS
    constexpr int DS_ = NT * 16 * 4;
    {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        float* dl = reinterpret_cast<float*>(lds);
        const int n_ = lane & 15;
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int j = 0; j < 3; ++j) dl[(3 * (4 * m + kq) + j) * (DS_ / 4) + t * 16 + n_] = acc[m][t][j];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    int s1 = lane + lpn, s2 = lane + 2 * lpn;
    if (s1 >= 3 * lpn) s1 -= 3 * lpn;
    if (s2 >= 3 * lpn) s2 -= 3 * lpn;
    if (!active) s1 = s2 = lane;
    auto pull = [&](const f4& v, int src) -> f4 {
        f4 o;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float e = v[c];
            o[c] = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(src * 4, __builtin_bit_cast(int, e)));
        }
        return o;
    };
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
    for (int k = 0; k < G; ++k) {
        asm volatile("" : "+v"(r0w[k]));
        if (EPI == 1) asm volatile("" : "+v"(pw[k]), "+v"(ww[k]), "+v"(drow[k]));
    }
    auto store_piece = [&](int s_, const f4& v) {
        if constexpr (!OUT32) {
            i2s* yp16 = reinterpret_cast<i2s*>(reinterpret_cast<char*>(Y) + (((n0 + s_) * 3 + ga) * ldy + c0) * 2);
            if (active) DS_STREAM_STORE(yp16, pack_bf16x4(v));
        } else {
            float* yp = Y + ((n0 + s_) * 3 + ga) * ldy + c0;
            if (active) DS_STREAM_STORE(reinterpret_cast<f4*>(yp), v);
        }
    };
#pragma unroll
    for (int s_ = 0; s_ < G; ++s_) {
        if (s_ < nn) {  // wave-uniform
            const f4 tot = *reinterpret_cast<const f4*>(lds + (3 * s_ + ga) * DS_ + c0 * 4);
            const f4 r0v = unpack_bf16x4(r0w[s_]);
            if (EPI == 1) {
                const f4 pv = unpack_bf16x4(pw[s_]), wv = unpack_bf16x4(ww[s_]);
                const f3v dr = drow[s_];
                const float d0 = g == 0 ? dr[0] : (g == 1 ? dr[1] : dr[2]);
                const float d1 = g == 0 ? dr[1] : (g == 1 ? dr[2] : dr[0]);
                const float d2 = g == 0 ? dr[2] : (g == 1 ? dr[0] : dr[1]);
                const f4 q0 = r0v - tot;
                const f4 q1 = pull(q0, s1), q2 = pull(q0, s2);
                const f4 t = d0 * q0 + d1 * q1 + d2 * q2;
                f4 o = wv + epi.c2 * t;
                o += epi.first ? epi.c1 * wv : epi.c1 * (wv - pv);
                store_piece(s_, o);
            } else {
                store_piece(s_, r0v - tot);
            }
        }
    }
    DS_DIAG_END(g_mf_dbg, MF_DIAG_WAVES, lane);
}

// Compact bf16 blocks for the MFMA form: kc[p][i][0..3] = (bf16) K(block kperm[p])[i][0..2], 0 - the blocks in group /
// entry / node order (kperm from the topology tables), every 3-element row padded to 8 bytes.
__global__ void pack_kc_kernel(const float* __restrict__ k32, const int32_t* __restrict__ kperm, int64_t nnzb,
                               i2s* __restrict__ kc) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nnzb * 3) return;
    const int64_t p = t / 3;
    const int i = (int)(t - 3 * p);
    const float* src = k32 + (int64_t)kperm[p] * 9 + 3 * i;
    const unsigned a = __builtin_bit_cast(unsigned short, (__bf16)src[0]), b = __builtin_bit_cast(unsigned short, (__bf16)src[1]),
                   c = __builtin_bit_cast(unsigned short, (__bf16)src[2]);
    kc[t] = i2s{(int)(a | (b << 16)), (int)c};
}
