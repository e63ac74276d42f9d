// Point clouds of the early-phase spectral loss - gfx950: what the reference's spec2point (src/ddsp/mss_loss.py:19-48)
// makes of a power spectrogram on the 'geomloss' path (:104-117), for the linear and the log cloud of one scale at once,
// and the gradient to the mode frequencies.  P (B x F x T) f32 is what ds_stft_power left; no log spectrogram is written.
//
//   lin (B x F x 4), log (B x fclip x 4), fclip = int(F * scale) rows of the same P:
//     columns 0..2  F.interpolate(row, size=3, mode='linear', align_corners=False) of x = P (lin) or of
//                   x = (log2(P + eps) - log2(eps)) / 40 (log; the logarithm BEFORE the interpolation, evaluated at the at
//                   most six samples a row needs):  src_i = max((i + 0.5) T / 3 - 0.5, 0), i0 = floor(src_i),
//                   i1 = min(i0 + 1, T - 1), l = src_i - i0, value = (1 - l) x[i0] + l x[i1].
//     column 3      row / bins, bins the cloud's own row count (F or fclip) - then, with freq[E], the reference's writes
//                   replayed: pos = bins / (sample_rate // 2) * freq[e]; rounds w = 2, 1, 0, in each cur = pos - w first,
//                   cur = pos + w second; an entry writes cur / bins into row trunc(cur) of every batch when
//                   0 <= trunc(cur) < bins (truncation toward zero: cur in (-1, 0) lands in row 0); non-finite cur writes
//                   nothing.  A later write overrides an earlier one; inside one write the highest flat index wins - what a
//                   sequential index_put does (torch's device scatter leaves it undefined; this unit defines it).
//
//   spec_points_winner_kernel   one thread per entry (grid-stride): its 6 candidates per cloud, key = (write + 1) << 56 | e
//       (write = 2 round + (0: minus, 1: plus), rounds in the reference's order), a vector atomicMax into the row's word of
//       the winner table win[F + fclip] (lin rows, then log rows; zeroed by a memset node in front).  max does not depend on
//       arrival order: the table is the same on every call.  A plain read in front skips candidates that have already lost.
//   spec_points_gather_kernel   one thread per (cloud row, batch): features, and column 3 from the row's winner (the entry's
//       cur is recomputed - the same instructions, the same bits), one 16-byte store per point.
//   spec_points_bwd_kernel      one thread per entry: g_freq[e] = gscale sum over clouds of (c / bins) sum over the writes q of e
//       whose row belongs to write q of sum_b g[b, row, 3], batches ascending, in fp64, rounded once.  This is what autograd
//       gives through the reference: the backward of index_put_ gathers the row's gradient for EVERY entry of the write that
//       owns the row (it is zeroed only for earlier writes), so two entries that share a row inside one write are both
//       credited, and every copy of an expanded view is.  gscale = the number of copies the caller collapsed into one entry.
//       A gather: no atomics, the same bits on every call.  No gradient goes to P (the reference detaches it).
//
// Arithmetic (tests/_spec_points_ref.py mirrors column 3 and derives the feature bound from this paragraph).
//   * Column 3 is the fp32 operations torch performs on DEVICE tensors, in torch's order, each correctly rounded and none
//     contracted: c = (float)((double)bins / (sample_rate / 2)) on the host, pos = c * f, cur = pos -+ (float)w, and the
//     division by the Python scalar bins as torch's device kernel does it, a product with r = 1.0f / (float)bins (formed on the
//     host): value = cur * r, row * r.  (On CPU tensors torch divides; the two differ by an ulp unless bins is a power of two.)
//     A fused multiply-subtract could move an entry to another row at an integer boundary.
//   * Features are fp32 as torch's upsample kernel forms them: scale = (float)T / 3, src = fma(scale, i + 0.5, -0.5) clamped at
//     0, l = src - i0 (exact), (1 - l) x0 + l x1 with at most four roundings; log samples a = P + eps, log2f(a) - (float)log2(eps),
//     the difference / 40.
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "ds_common.h"

namespace {

constexpr int SP_THREADS = 256;
constexpr int SP_MAX_BLOCKS = 2048;
constexpr unsigned long long SP_ENTRY_MASK = (1ull << 56) - 1ull;

struct SpCloud {
    int bins;      // rows of the cloud
    float c;       // (float)(bins / (sample_rate // 2))
    float fbins;   // (float)bins
    float rbins;   // 1.0f / (float)bins: torch divides a device tensor by a scalar as x * (1 / scalar)
};

// cur of write q (0..5: rounds w = 2, 1, 0; even = pos - w, odd = pos + w) of frequency f; torch's operations, uncontracted
__device__ __forceinline__ float sp_cur(float c, float f, int q) {
#pragma clang fp contract(off)  // (__fmul_rn / __fsub_rn are plain operators to this compiler and fuse into one v_fma_f32)
    const float pos = c * f;
    const float w = (float)(2 - (q >> 1));
    return (q & 1) ? pos + w : pos - w;
}

// row that cur writes, or -1: 0 <= trunc(cur) < bins  <=>  -1 < cur < bins (false for NaN and +-inf)
__device__ __forceinline__ int sp_row(float cur, const SpCloud& cl) {
    return (cur > -1.0f && cur < cl.fbins) ? (int)cur : -1;
}

__global__ void __launch_bounds__(SP_THREADS)
    spec_points_winner_kernel(const float* __restrict__ freq, int64_t E, SpCloud lin, SpCloud lg, unsigned long long* win) {
    const int64_t stride = (int64_t)gridDim.x * SP_THREADS;
    for (int64_t e = (int64_t)blockIdx.x * SP_THREADS + threadIdx.x; e < E; e += stride) {
        const float f = freq[e];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const SpCloud cl = k ? lg : lin;
            unsigned long long* w = win + (k ? lin.bins : 0);
#pragma unroll
            for (int q = 0; q < 6; ++q) {
                const int row = sp_row(sp_cur(cl.c, f, q), cl);
                if (row < 0) continue;
                const unsigned long long key = ((unsigned long long)(q + 1) << 56) | (unsigned long long)e;
                if (__atomic_load_n(&w[row], __ATOMIC_RELAXED) < key) atomicMax(&w[row], key);  // the word only grows
            }
        }
    }
}

__device__ __forceinline__ float sp_log_sample(float p, float eps, float log2eps) {
    return __fdiv_rn(__fsub_rn(log2f(__fadd_rn(p, eps)), log2eps), 40.0f);
}

__global__ void __launch_bounds__(SP_THREADS)
    spec_points_gather_kernel(const float* __restrict__ P, int B, int F, int T, float eps, float log2eps, SpCloud lin, SpCloud lg,
                              const float* __restrict__ freq, const unsigned long long* __restrict__ win,
                              float* __restrict__ out_lin, float* __restrict__ out_log) {
    const int rows = lin.bins + lg.bins;
    const int64_t total = (int64_t)B * rows;
    const int64_t i = (int64_t)blockIdx.x * SP_THREADS + threadIdx.x;
    if (i >= total) return;
    const int b = (int)(i / rows), r = (int)(i % rows);
    const bool is_log = r >= lin.bins;
    const int row = is_log ? r - lin.bins : r;
    const SpCloud cl = is_log ? lg : lin;
    const float* x = P + ((int64_t)b * F + row) * T;
    const float scale = __fdiv_rn((float)T, 3.0f);
    float4 pt;
    float* v = &pt.x;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float src = fmaxf(__builtin_fmaf(scale, (float)k + 0.5f, -0.5f), 0.0f);
        const int i0 = min((int)src, T - 1);
        const int i1 = min(i0 + 1, T - 1);
        const float l1 = src - (float)i0, l0 = 1.0f - l1;
        float x0 = x[i0], x1 = x[i1];
        if (is_log) {
            x0 = sp_log_sample(x0, eps, log2eps);
            x1 = sp_log_sample(x1, eps, log2eps);
        }
        v[k] = l0 * x0 + l1 * x1;
    }
    float pos = __fmul_rn((float)row, cl.rbins);
    if (win) {
        const unsigned long long key = win[r];
        if (key) pos = __fmul_rn(sp_cur(cl.c, freq[key & SP_ENTRY_MASK], (int)(key >> 56) - 1), cl.rbins);
    }
    pt.w = pos;
    float* out = is_log ? out_log : out_lin;
    *reinterpret_cast<float4*>(out + ((int64_t)b * cl.bins + row) * 4) = pt;
}

__global__ void __launch_bounds__(SP_THREADS)
    spec_points_bwd_kernel(const float* __restrict__ freq, int64_t E, int B, SpCloud lin, SpCloud lg,
                           const unsigned long long* __restrict__ win, const float* __restrict__ g_lin,
                           const float* __restrict__ g_log, double gscale, float* __restrict__ g_freq) {
    const int64_t stride = (int64_t)gridDim.x * SP_THREADS;
    for (int64_t e = (int64_t)blockIdx.x * SP_THREADS + threadIdx.x; e < E; e += stride) {
        const float f = freq[e];
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const SpCloud cl = k ? lg : lin;
            const float* g = k ? g_log : g_lin;
            if (!g) continue;
            const unsigned long long* w = win + (k ? lin.bins : 0);
            double s = 0.0;
            for (int q = 0; q < 6; ++q) {
                const int row = sp_row(sp_cur(cl.c, f, q), cl);
                if (row < 0) continue;
                if ((int)(w[row] >> 56) != q + 1) continue;  // the row belongs to a later write (or, never, to an earlier one)
                for (int b = 0; b < B; ++b) s += (double)g[((int64_t)b * cl.bins + row) * 4 + 3];
            }
            acc += s * ((double)cl.c * (double)cl.rbins);
        }
        g_freq[e] = (float)(gscale * acc);
    }
}

int sp_shape_ok(const char* fn, int B, int F, int fclip) {
    DS_REQUIRE(B >= 1 && F >= 1, "%s: B = %d, F = %d, need B, F >= 1", fn, B, F);
    DS_REQUIRE(fclip >= 1 && fclip <= F, "%s: fclip = %d outside [1, F = %d]", fn, fclip, F);
    return DS_OK;
}

int sp_freq_ok(const char* fn, int64_t E, int sample_rate) {
    DS_REQUIRE(E >= 1 && E <= (int64_t)SP_ENTRY_MASK, "%s: E = %lld outside [1, 2^56)", fn, (long long)E);
    DS_REQUIRE(sample_rate >= 2, "%s: sample_rate = %d, need sample_rate // 2 >= 1", fn, sample_rate);
    return DS_OK;
}

SpCloud sp_cloud(int bins, int sample_rate) {
    SpCloud cl;
    cl.bins = bins;
    cl.c = sample_rate >= 2 ? (float)((double)bins / (double)(sample_rate / 2)) : 0.0f;
    cl.fbins = (float)bins;
    cl.rbins = 1.0f / (float)bins;
    return cl;
}

unsigned sp_entry_blocks(int64_t E) { return (unsigned)std::min<int64_t>(ds::ceil_div(E, SP_THREADS), SP_MAX_BLOCKS); }

}  // namespace

extern "C" int ds_spec_points_fwd(const float* P, int B, int F, int T, float eps, int fclip, const float* freq, int64_t E,
                                  int sample_rate, unsigned long long* win, float* lin, float* logc, ds_stream_t stream) {
    DS_REQUIRE(P && lin && logc, "ds_spec_points_fwd: null pointer");
    if (int rc = sp_shape_ok("ds_spec_points_fwd", B, F, fclip)) return rc;
    DS_REQUIRE(T >= 1, "ds_spec_points_fwd: T = %d, need T >= 1", T);
    DS_REQUIRE(eps > 0.0f && std::isfinite(eps), "ds_spec_points_fwd: eps = %g must be positive and finite", (double)eps);
    DS_REQUIRE((freq == nullptr) == (win == nullptr), "ds_spec_points_fwd: freq and the winner table come together");
    DS_REQUIRE((reinterpret_cast<uintptr_t>(lin) | reinterpret_cast<uintptr_t>(logc)) % 16 == 0,
               "ds_spec_points_fwd: the clouds must be 16-byte aligned");
    hipStream_t st = ds::as_stream(stream);
    const SpCloud cl = sp_cloud(F, freq ? sample_rate : 0), cg = sp_cloud(fclip, freq ? sample_rate : 0);
    if (freq) {
        if (int rc = sp_freq_ok("ds_spec_points_fwd", E, sample_rate)) return rc;
        DS_REQUIRE(reinterpret_cast<uintptr_t>(win) % 8 == 0, "ds_spec_points_fwd: the winner table must be 8-byte aligned");
        if (int rc = ds::check_hip(hipMemsetAsync(win, 0, sizeof(unsigned long long) * (size_t)(F + fclip), st), "winner table memset"))
            return rc;
        spec_points_winner_kernel<<<sp_entry_blocks(E), SP_THREADS, 0, st>>>(freq, E, cl, cg, win);
        DS_LAUNCH_CHECK("spec_points_winner_kernel");
    }
    const int64_t total = (int64_t)B * (F + fclip);
    DS_REQUIRE(ds::ceil_div(total, SP_THREADS) <= 0x7fffffff, "ds_spec_points_fwd: B (F + fclip) = %lld too large", (long long)total);
    spec_points_gather_kernel<<<(unsigned)ds::ceil_div(total, SP_THREADS), SP_THREADS, 0, st>>>(
        P, B, F, T, eps, (float)std::log2((double)eps), cl, cg, freq, win, lin, logc);
    DS_LAUNCH_CHECK("spec_points_gather_kernel");
    return DS_OK;
}

extern "C" int ds_spec_points_bwd(const float* g_lin, const float* g_log, int B, int F, int fclip, const float* freq, int64_t E,
                                  int sample_rate, const unsigned long long* win, double gscale, float* g_freq, ds_stream_t stream) {
    DS_REQUIRE(freq && win && g_freq, "ds_spec_points_bwd: null pointer");
    if (int rc = sp_shape_ok("ds_spec_points_bwd", B, F, fclip)) return rc;
    if (int rc = sp_freq_ok("ds_spec_points_bwd", E, sample_rate)) return rc;
    spec_points_bwd_kernel<<<sp_entry_blocks(E), SP_THREADS, 0, ds::as_stream(stream)>>>(
        freq, E, B, sp_cloud(F, sample_rate), sp_cloud(fclip, sample_rate), win, g_lin, g_log, gscale, g_freq);
    DS_LAUNCH_CHECK("spec_points_bwd_kernel");
    return DS_OK;
}
