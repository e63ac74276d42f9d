// Filtered-noise branch of the oscillator modules - gfx950: time-varying filtered white noise (reference
// src/ddsp/filtered_noise.py:20-67), forward and backward, one launch each.
//
// The reference turns, per frame of F samples, L learnable logits into a magnitude response, that into a zero-phase
// impulse response by an irfft of odd length T = 2 L - 1, rolls it by L - 1, windows it (periodic Hann), convolves a
// fresh white-noise frame with it by FFTs of length T + F - 1, and overlap-adds the frames at stride F; autograd mirrors
// all of it.  The arithmetic is tiny, so both directions are direct sums here.  With nf = S / F + 1 frames:
//   mag[k] = 2 sigmoid(c[k])^2.3 + 1e-6                                      k < L
//   z[n]   = (mag[0] + 2 sum_{k=1..L-1} mag[k] cos(2 pi ((k n) mod T) / T)) / T    n < T
//   h[j]   = z[(j - (L - 1)) mod T] w[j],   w[j] = 0.5 - 0.5 cos(2 pi j / T)        j < T
//   out[b, o] = gain sum_f sum_t noise[b, f, t] h_{b,f}[o - f F - t]                o < S  (linear, nothing wraps)
//
//   ds_filtered_noise_fwd  one workgroup per (chunk of m F <= 256 output samples, clip), one thread per sample.  The
//       workgroup walks the frames that reach its chunk - m + ceil((T + F - 1) / F) - 1 of them - in ascending order;
//       per frame it forms mag, then h, in LDS and every thread adds the frame's terms to its sample, t ascending.
//       A GATHER: every element of out is written exactly once, no atomics, no zero-fill, the same bits on every call.
//   ds_filtered_noise_bwd  the adjoint, one workgroup per (frame, clip):
//       gh[j] = sum_t noise[t] gy[b, f F + t + j]   (gy read as 0 from index S on),  gz[(j - (L - 1)) mod T] = gh[j] w[j],
//       gmag[k] = (c_k / T) sum_n gz[n] cos(2 pi ((k n) mod T) / T),  c_0 = 1, c_k = 2,
//       gc[b, f, k] = gain gmag[k] 4.6 sigmoid^2.3 (1 - sigmoid).
//       It is linear in h and needs no impulse response: the forward saves nothing but its inputs.  Every gc[b, f, k]
//       is written exactly once; a frame that starts at or after S gets exact zeros.
//
// Arithmetic (tests/_filtered_noise_ref.py derives its bounds from this paragraph).  Storage is fp32.
//   * No fp32 transcendental: sigmoid, the power 2.3, and the cosines are fp64 (exp, pow, cospi) and round to fp32 ONCE:
//     mag, the twiddle table cos(2 pi m / T) (m < T; the integer k n is reduced mod T by an add-and-wrap, so the argument
//     is exact) and the window w[j] = (float)(0.5 - 0.5 cospi(2 j / T)).
//   * fp64 sums: the cosine sums for z (L terms, fp64 fma of exact fp32 products) and for gmag (T terms); z / T in fp64,
//     then z rounds to fp32 once; h = z w is one fp32 product.  gmag, the derivative factor and gain stay fp64 until the
//     one rounding of the store.
//   * fp32 sums: the convolution - one fp32 fma per term into ONE accumulator per output sample that runs through all
//     its frames (at most min(F, T) ceil((T + F - 1) / F) terms); out = (float)(gain (double)acc).  In the backward
//     gh[j] is F fp32 fmas (t ascending, zeros included) and gh[j] w[j] one fp32 product.
//   * LDS: in both convolutions the lanes of a wave read ONE noise[t] (a broadcast) and consecutive words of h / gy
//     (lane l reads word base + l): no bank conflict.  The twiddle gathers cos[(k n) mod T] are the usual DFT pattern.
#include <algorithm>
#include <cmath>

#include "ds_common.h"

namespace {

constexpr int FN_MAXL = 129;               // filter_coeff_length
constexpr int FN_MAXT = 2 * FN_MAXL - 1;   // taps
constexpr int FN_MAXF = 256;               // frame_length
constexpr int FN_THREADS = 256;

__device__ __forceinline__ double fn_sigmoid(float c) { return 1.0 / (1.0 + exp(-(double)c)); }

// cos(2 pi m / T) and the periodic Hann window, rounded to fp32 once each
__device__ __forceinline__ void fn_tables(int T, float* s_cos, float* s_win) {
    for (int m = threadIdx.x; m < T; m += FN_THREADS) {
        const double cs = cospi(2.0 * m / T);
        s_cos[m] = (float)cs;
        s_win[m] = (float)(0.5 - 0.5 * cs);
    }
}

__global__ void __launch_bounds__(FN_THREADS)
    filtered_noise_fwd_kernel(const float* __restrict__ c, const float* __restrict__ noise, int S, int L, int F, int m,
                              double gain, float* __restrict__ out) {
    __shared__ float s_cos[FN_MAXT];
    __shared__ float s_win[FN_MAXT];
    __shared__ float s_mag[FN_MAXL];
    __shared__ float s_h[FN_MAXT];
    __shared__ float s_n[FN_MAXF];
    const int T = 2 * L - 1, nf = S / F + 1, C = m * F;  // C <= 256
    const int b = blockIdx.y, tid = threadIdx.x;
    const int64_t o0 = (int64_t)blockIdx.x * C;          // < S
    const int64_t o = o0 + tid;
    const bool mine = tid < C && o < S;
    const int reach = (T + F - 2) / F;                   // a frame reaches samples of the reach following frames' spans
    const int f_lo = max(0, (int)blockIdx.x * m - reach);
    const int f_hi = (int)((min((int64_t)S, o0 + C) - 1) / F);  // <= nf - 1
    fn_tables(T, s_cos, s_win);
    float acc = 0.f;
    for (int f = f_lo; f <= f_hi; ++f) {
        const int64_t row = (int64_t)b * nf + f;
        if (tid < L) {
            const double sg = fn_sigmoid(c[row * L + tid]);
            s_mag[tid] = (float)(2.0 * pow(sg, 2.3) + 1e-6);
        }
        if (tid < F) s_n[tid] = noise[row * F + tid];
        __syncthreads();
        for (int j = tid; j < T; j += FN_THREADS) {  // T <= 257: thread 0 takes a second tap at L = 129
            int n = j - (L - 1);
            if (n < 0) n += T;
            double zs = 0.0;
            int ph = n;  // (k n) mod T, from k = 1 on
            for (int k = 1; k < L; ++k) {
                zs = fma((double)s_mag[k], (double)s_cos[ph], zs);
                ph += n;
                if (ph >= T) ph -= T;
            }
            const float z = (float)(((double)s_mag[0] + 2.0 * zs) / T);
            s_h[j] = z * s_win[j];
        }
        __syncthreads();
        const int64_t s = o - (int64_t)f * F;
        if (mine && s >= 0 && s <= T + F - 2) {
            const int si = (int)s, t1 = min(F - 1, si);
            for (int t = max(0, si - T + 1); t <= t1; ++t) acc = __builtin_fmaf(s_n[t], s_h[si - t], acc);
        }
        __syncthreads();  // s_n and s_mag are rewritten by the next frame
    }
    if (mine) out[(int64_t)b * S + o] = (float)(gain * (double)acc);
}

__global__ void __launch_bounds__(FN_THREADS)
    filtered_noise_bwd_kernel(const float* __restrict__ gy, const float* __restrict__ c, const float* __restrict__ noise,
                              int S, int L, int F, double gain, float* __restrict__ gc) {
    __shared__ float s_cos[FN_MAXT];
    __shared__ float s_win[FN_MAXT];
    __shared__ float s_gz[FN_MAXT];
    __shared__ float s_n[FN_MAXF];
    __shared__ float s_gy[FN_MAXT + FN_MAXF - 1];
    const int T = 2 * L - 1, nf = S / F + 1;
    const int f = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int64_t row = (int64_t)b * nf + f;
    const int64_t start = (int64_t)f * F;
    if (start >= S) {  // the last frame when F divides S: no sample of out depends on it
        if (tid < L) gc[row * L + tid] = 0.f;
        return;
    }
    fn_tables(T, s_cos, s_win);
    if (tid < F) s_n[tid] = noise[row * F + tid];
    for (int i = tid; i < T + F - 1; i += FN_THREADS) s_gy[i] = start + i < S ? gy[(int64_t)b * S + start + i] : 0.f;
    __syncthreads();
    for (int j = tid; j < T; j += FN_THREADS) {
        float gh = 0.f;
        for (int t = 0; t < F; ++t) gh = __builtin_fmaf(s_n[t], s_gy[t + j], gh);
        int n = j - (L - 1);
        if (n < 0) n += T;
        s_gz[n] = gh * s_win[j];
    }
    __syncthreads();
    if (tid < L) {
        const int k = tid;
        double a = 0.0;
        int ph = 0;
        for (int n = 0; n < T; ++n) {
            a = fma((double)s_gz[n], (double)s_cos[ph], a);
            ph += k;
            if (ph >= T) ph -= T;
        }
        const double sg = fn_sigmoid(c[row * L + k]);
        const double dmag = 4.6 * pow(sg, 2.3) * (1.0 - sg);
        gc[row * L + k] = (float)(gain * (a * (k == 0 ? 1.0 : 2.0) / T) * dmag);
    }
}

int fn_shape_ok(const char* fn, int B, int S, int L, int F) {
    DS_REQUIRE(L >= 2 && L <= FN_MAXL, "%s: L (filter_coeff_length) = %d outside [2, %d]", fn, L, FN_MAXL);
    DS_REQUIRE(F >= 1 && F <= FN_MAXF, "%s: F (frame_length) = %d outside [1, %d]", fn, F, FN_MAXF);
    DS_REQUIRE(S >= 1, "%s: S (sample_num) = %d, need S >= 1", fn, S);
    DS_REQUIRE(B >= 1 && B <= 65535, "%s: B (noise_num) = %d outside [1, 65535]", fn, B);
    return DS_OK;
}

}  // namespace

extern "C" int ds_filtered_noise_fwd(const float* c, const float* noise, int B, int S, int L, int F, double gain, float* out,
                                     ds_stream_t stream) {
    DS_REQUIRE(c && noise && out, "ds_filtered_noise_fwd: null pointer");
    if (int rc = fn_shape_ok("ds_filtered_noise_fwd", B, S, L, F)) return rc;
    const int m = std::max(1, FN_THREADS / F);  // frames' spans per workgroup: m F <= 256 samples, one thread each
    const unsigned chunks = (unsigned)ds::ceil_div(S, (int64_t)m * F);
    filtered_noise_fwd_kernel<<<dim3(chunks, (unsigned)B), FN_THREADS, 0, ds::as_stream(stream)>>>(c, noise, S, L, F, m, gain, out);
    DS_LAUNCH_CHECK("filtered_noise_fwd_kernel");
    return DS_OK;
}

extern "C" int ds_filtered_noise_bwd(const float* gy, const float* c, const float* noise, int B, int S, int L, int F, double gain,
                                     float* gc, ds_stream_t stream) {
    DS_REQUIRE(gy && c && noise && gc, "ds_filtered_noise_bwd: null pointer");
    if (int rc = fn_shape_ok("ds_filtered_noise_bwd", B, S, L, F)) return rc;
    filtered_noise_bwd_kernel<<<dim3((unsigned)(S / F + 1), (unsigned)B), FN_THREADS, 0, ds::as_stream(stream)>>>(gy, c, noise, S, L, F,
                                                                                                                 gain, gc);
    DS_LAUNCH_CHECK("filtered_noise_bwd_kernel");
    return DS_OK;
}
