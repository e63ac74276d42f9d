// Propagation delay: a time-varying fractional delay line with gradients to the signal and to the delay - gfx950.
//
// A source at rest heard by a receiver on a path x(t) is s(t - r(t) / c): onset time, the envelope's delay and the Doppler
// shift at once.  Per row b (a clip's channel) and with the frames of osc_slide.hip / osc_listen.hip
// (k = min(t / hop, K-1), th = (t - k hop) / hop, th = 0 where t / hop >= K-1: the last frame held):
//     tau(t) = tau[b,k] + th (tau[b,min(k+1, K-1)] - tau[b,k])      = (1 - th) tau_k + th tau_k+1; equal frames give their
//                                                                    value exactly, whatever th
//     p(t)   = t - tau(t),  n = floor(p),  f = p - n                 (all of it fp64)
//     h(u)   = sinc(u) cos^2(pi u / (2 R)) for |u| < R, 0 outside,  R = DS_DELAY_HALF_TAPS
//     y[b,t] = sum_{i = -R+1 .. R} h(f - i) s[b, n + i],  s = 0 outside [0, S).
// h(-i) = delta_i: f = 0 copies s[n], bit for bit (a branch of its own: no 0 s products, no -0 turned into +0).  h is C1,
// value and slope vanish at +-R, so d y / d tau is continuous where p crosses an integer.  sin(pi f) is formed once per
// output: sinc(f - i) = (-1)^i sin(pi f) / (pi (f - i)), and the window's cos(pi (f - i) / R) by the addition theorem from
// cos, sin(pi f / R) and a table of cos, sin(pi i / R).
// Backward (no conjugate, no approximation):
//     gs[b,j]   = sum_t gy[b,t] h(p(t) - j)                                         a GATHER: with frames that differ by at
//                 most hop DS_DELAY_MAX_SLOPE, p rises by 0.5 .. 1.5 a sample, and the t that reach j are one run of <= 4R + 1
//     gtau[b,k] = - sum_t hat_k(t) gy[b,t] sum_j s[b,j] h'(p(t) - j),               hat_k the two interpolation weights
//                 exactly 0 for a frame that no sample t < S touches.
//   gs        workgroup = (tile of GT inputs j, row): the first t with p(t) > j0 - R by bisection on p (every lane the same
//             loads), then n, f, sin(pi f), cos / sin(pi f / R) and gy of the <= 2 (GT + 2R) + 1 samples that can reach the
//             tile go to LDS once - 3 sin / cos calls a SAMPLE, not a tap - and a lane finds its own first sample by
//             bisection in LDS and adds its run in order of t.
//   gtau      q[b,t] = gy[b,t] sum_j s h'(p(t) - j) into the workspace (one thread a sample, the forward's 16 taps), then one
//             wavefront per (row, frame) adds its two segments - the held frame its whole tail - lane by lane in order of t
//             and joins the lanes with a butterfly.
// Every address comes from an index that was range-checked in fp64 BEFORE its conversion to an integer: a p outside
// [-R, S + R) gives 0, a non-finite tau(t) NaN in y and nothing in gs / gtau, without a memory access.  A violated slope
// bound makes gs unspecified (a run may be cut off at the tile's LDS image) but every index stays inside [0, S).
// No atomics, the same bits from the same inputs.  The signal is read straight from L1 / L2 (a wave's 16 taps cover a
// contiguous span of <= 1.5 * 64 + 2R floats); only the gather stages through LDS.
#include <cmath>
#include <cstdint>

#include "ds_common.h"

namespace {

constexpr int R = DS_DELAY_HALF_TAPS;
constexpr int T = 256;                   // outputs per workgroup, one a thread
constexpr int GT = 256;                  // inputs j per workgroup of the gather
constexpr int GE = 2 * (GT + 2 * R) + 8; // samples a gather tile keeps in LDS (2 (GT - 1 + 2R) + 1 can reach it)
constexpr double PI = 3.14159265358979323846;
static_assert(R == 8, "the window table below is cos, sin(pi i / 8)");
static_assert(DS_DELAY_MAX_SLOPE == 0.5, "GE and the run of 4R + 1 samples assume p' >= 0.5");

#define C1 0.92387953251128674
#define C2 0.70710678118654752
#define C3 0.38268343236508977
// cos(pi i / R), sin(pi i / R) for i = -R+1 .. R at index i + R - 1
__device__ const double WIN_C[2 * R] = {-C1, -C2, -C3, 0.0, C3, C2, C1, 1.0, C1, C2, C3, 0.0, -C3, -C2, -C1, -1.0};
__device__ const double WIN_S[2 * R] = {-C3, -C2, -C1, -1.0, -C1, -C2, -C3, 0.0, C3, C2, C1, 1.0, C1, C2, C3, 0.0};
#undef C1
#undef C2
#undef C3

// tau(t) of one row; false where it is not finite
__device__ __forceinline__ bool tau_at(const double* __restrict__ trow, int K, int hop, double inv_hop, int64_t t, double& tau) {
    const int64_t kk = t / hop;
    if (kk >= K - 1) {
        tau = trow[K - 1];
    } else {
        const double a = trow[kk], b = trow[kk + 1];
        tau = a + ((double)(t - kk * hop) * inv_hop) * (b - a);
    }
    return isfinite(tau);
}

// what a sample t knows of its read position: n = floor(p) (as a double, range-checked), f, sin(pi f), cos(pi f) and
// sin, cos(pi f / R)
struct frac {
    double f, sp, cp, sr, cr;
};

__device__ __forceinline__ frac frac_of(double f) {
    frac q;
    q.f = f;
    sincospi(f, &q.sp, &q.cp);
    sincospi(f * (1.0 / R), &q.sr, &q.cr);
    return q;
}

// h(f - i) for -R < i <= R; wc, ws = cos, sin(pi i / R)
__device__ __forceinline__ double tap(const frac& q, int i, double wc, double ws) {
    const double u = q.f - (double)i;
    if (u == 0.0) return 1.0;
    const double sinc = ((i & 1) ? -q.sp : q.sp) / (PI * u);
    return sinc * (0.5 * (1.0 + (q.cr * wc + q.sr * ws)));
}

// h'(f - i).  sinc'(u) = (cos(pi u) - sinc(u)) / u loses |u|^-1 ulps to cancellation: below |u| = 1/8 the series
// -pi^2 u (1/3 - x/30 + x^2/840 - ...), x = (pi u)^2, term k = 2k / (2k+1)!, through k = 7 (the next is below 1e-19)
__device__ __forceinline__ double dtap(const frac& q, int i, double wc, double ws) {
    const double u = q.f - (double)i;
    double sinc, dsinc;
    if (fabs(u) < 0.125) {
        const double x = (PI * u) * (PI * u);
        dsinc = -(PI * PI * u) *
                (1.0 / 3.0 - x * (1.0 / 30.0 - x * (1.0 / 840.0 - x * (1.0 / 45360.0 - x * (1.0 / 3991680.0 - x * (1.0 / 518918400.0 -
                                                                                                             x * (1.0 / 93405312000.0)))))));
        sinc = u == 0.0 ? 1.0 : ((i & 1) ? -q.sp : q.sp) / (PI * u);
    } else {
        sinc = ((i & 1) ? -q.sp : q.sp) / (PI * u);
        dsinc = (((i & 1) ? -q.cp : q.cp) - sinc) / u;
    }
    const double win = 0.5 * (1.0 + (q.cr * wc + q.sr * ws));
    const double dwin = (-PI / (2.0 * R)) * (q.sr * wc - q.cr * ws);  // -pi / (2R) sin(pi u / R)
    return dsinc * win + sinc * dwin;
}

// 1. y[b,t]: one thread an output
__global__ void __launch_bounds__(T)
    delay_fwd_kernel(const float* __restrict__ s, const double* __restrict__ tau, int S, int K, int hop, float* __restrict__ y) {
    const int64_t t = (int64_t)blockIdx.x * T + threadIdx.x;
    if (t >= S) return;
    const int b = blockIdx.y;
    const float* srow = s + (int64_t)b * S;
    float* yo = y + (int64_t)b * S + t;
    double tv;
    if (!tau_at(tau + (int64_t)b * K, K, hop, 1.0 / (double)hop, t, tv)) {
        *yo = __builtin_nanf("");
        return;
    }
    const double p = (double)t - tv;
    if (!(p >= -(double)R && p < (double)S + R)) {  // (fp64, before any integer is formed)
        *yo = 0.f;
        return;
    }
    const double fl = floor(p);
    const int64_t n = (int64_t)fl;
    const double f = p - fl;
    if (f == 0.0) {  // an integer delay is a shift
        *yo = (n >= 0 && n < S) ? srow[n] : 0.f;
        return;
    }
    const frac q = frac_of(f);
    double acc = 0.0;
#pragma unroll
    for (int i = -R + 1; i <= R; ++i) {
        const int64_t j = n + i;
        const double v = (j >= 0 && j < S) ? (double)srow[j] : 0.0;
        acc += tap(q, i, WIN_C[i + R - 1], WIN_S[i + R - 1]) * v;
    }
    *yo = (float)acc;
}

// 2. q[b,t] = gy[b,t] sum_j s[b,j] h'(p(t) - j), 0 where the forward reads nothing
__global__ void __launch_bounds__(T)
    delay_slope_kernel(const float* __restrict__ gy, const float* __restrict__ s, const double* __restrict__ tau, int S, int K,
                       int hop, double* __restrict__ qout) {
    const int64_t t = (int64_t)blockIdx.x * T + threadIdx.x;
    if (t >= S) return;
    const int b = blockIdx.y;
    const float* srow = s + (int64_t)b * S;
    double* qo = qout + (int64_t)b * S + t;
    double tv;
    *qo = 0.0;
    if (!tau_at(tau + (int64_t)b * K, K, hop, 1.0 / (double)hop, t, tv)) return;
    const double p = (double)t - tv;
    if (!(p >= -(double)R && p < (double)S + R)) return;
    const double fl = floor(p);
    const int64_t n = (int64_t)fl;
    const frac q = frac_of(p - fl);
    double acc = 0.0;
#pragma unroll
    for (int i = -R + 1; i <= R; ++i) {
        const int64_t j = n + i;
        const double v = (j >= 0 && j < S) ? (double)srow[j] : 0.0;
        acc += dtap(q, i, WIN_C[i + R - 1], WIN_S[i + R - 1]) * v;
    }
    *qo = (double)gy[(int64_t)b * S + t] * acc;
}

// 3. one wavefront per (frame, row): gtau[b,k] = -(sum over segment k-1 of th q + sum over segment k of (1 - th) q), the held
// frame K-1 with weight 1 on everything from (K-1) hop on; lane l adds t = start + l, + 64, ... in order
__global__ void __launch_bounds__(64)
    delay_gtau_kernel(const double* __restrict__ q, int S, int K, int hop, double* __restrict__ gtau) {
    const int k = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
    const double* qrow = q + (int64_t)b * S;
    const double inv_hop = 1.0 / (double)hop;
    const int64_t t1 = (int64_t)k * hop, t0 = t1 - hop;
    const int64_t t2 = (k == K - 1) ? (int64_t)S : (t1 + hop < S ? t1 + hop : (int64_t)S);
    double acc = 0.0;
    if (k > 0)
        for (int64_t t = t0 + lane; t < t1 && t < S; t += 64) acc += ((double)(t - t0) * inv_hop) * qrow[t];
    for (int64_t t = t1 + lane; t < t2; t += 64) {
        const double th = (k == K - 1) ? 0.0 : (double)(t - t1) * inv_hop;
        acc += (1.0 - th) * qrow[t];
    }
    acc = ds::wave_sum(acc);
    if (lane == 0) gtau[(int64_t)b * K + k] = 0.0 - acc;
}

// 4. workgroup = (tile of GT inputs, row): gs[b,j] = sum_t gy[b,t] h(p(t) - j)
__global__ void __launch_bounds__(GT)
    delay_gather_kernel(const float* __restrict__ gy, const double* __restrict__ tau, int S, int K, int hop,
                        float* __restrict__ gs) {
    __shared__ double e_n[GE], e_f[GE], e_sp[GE], e_sr[GE], e_cr[GE], e_g[GE];
    __shared__ double w_c[2 * R], w_s[2 * R];
    const int b = blockIdx.y;
    const int64_t j0 = (int64_t)blockIdx.x * GT;
    const double* trow = tau + (int64_t)b * K;
    const float* grow = gy + (int64_t)b * S;
    const double inv_hop = 1.0 / (double)hop;
    if (threadIdx.x < 2 * R) {
        w_c[threadIdx.x] = WIN_C[threadIdx.x];
        w_s[threadIdx.x] = WIN_S[threadIdx.x];
    }
    // the first sample whose p exceeds j0 - R: in [0, S] whatever tau holds (a NaN compares false and moves lo up)
    int64_t lo = 0, hi = S;
    const double x0 = (double)j0 - R;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        double tv;
        const bool ok = tau_at(trow, K, hop, inv_hop, mid, tv);
        if (ok && (double)mid - tv > x0)
            hi = mid;
        else
            lo = mid + 1;
    }
    const int64_t tb = lo;
    const int cnt = (int)(S - tb < GE ? S - tb : GE);
    for (int e = threadIdx.x; e < cnt; e += GT) {
        const int64_t t = tb + e;
        double tv, n = -1e300, f = 0.0, sp = 0.0, sr = 0.0, cr = 0.0, g = 0.0;  // (n = -1e300: a sample that reaches nothing)
        if (tau_at(trow, K, hop, inv_hop, t, tv)) {
            const double p = (double)t - tv;
            if (p >= (double)S + R) {
                n = 1e300;  // past every input: ends a lane's run
            } else if (p >= -(double)R) {
                n = floor(p);
                const frac q = frac_of(p - n);
                f = q.f, sp = q.sp, sr = q.sr, cr = q.cr;
                g = (double)grow[t];
            }
        }
        e_n[e] = n, e_f[e] = f, e_sp[e] = sp, e_sr[e] = sr, e_cr[e] = cr, e_g[e] = g;
    }
    __syncthreads();
    const int64_t j = j0 + threadIdx.x;
    if (j >= S) return;
    const double dj = (double)j;
    int a = 0, z = cnt;  // the first sample with n >= j - R
    while (a < z) {
        const int mid = (a + z) >> 1;
        if (e_n[mid] >= dj - R)
            z = mid;
        else
            a = mid + 1;
    }
    double acc = 0.0;
    for (int e = a; e < cnt; ++e) {
        const double di = dj - e_n[e];  // i = j - n: the tap of sample e that reads input j
        if (di > (double)R) continue;
        if (di < (double)(-R + 1)) break;
        const int i = (int)di;
        frac q;
        q.f = e_f[e], q.sp = e_sp[e], q.sr = e_sr[e], q.cr = e_cr[e], q.cp = 0.0;
        acc += e_g[e] * tap(q, i, w_c[i + R - 1], w_s[i + R - 1]);
    }
    gs[(int64_t)b * S + j] = (float)acc;
}

using ds::aligned;

int check_args(const char* fn, bool pointers, int B, int S, int K, int hop) {
    DS_REQUIRE(pointers, "%s: null pointer", fn);
    DS_REQUIRE(B > 0 && S > 0 && K > 0, "%s: empty problem (B %d, S %d, K %d)", fn, B, S, K);
    DS_REQUIRE(B <= DS_DELAY_MAX_ROWS, "%s: B = %d above %d", fn, B, DS_DELAY_MAX_ROWS);
    DS_REQUIRE(hop > 0, "%s: hop = %d is not positive", fn, hop);
    return DS_OK;
}

}  // namespace

extern "C" int64_t ds_delay_workspace_bytes(int B, int S, int K, int hop) {
    if (B <= 0 || B > DS_DELAY_MAX_ROWS || S <= 0 || K <= 0 || hop <= 0) return 0;
    return (int64_t)sizeof(double) * B * S;
}

extern "C" int ds_delay_fwd(const float* s, const double* tau, int B, int S, int K, int hop, float* y, ds_stream_t stream) {
    if (int rc = check_args("ds_delay_fwd", s && tau && y, B, S, K, hop)) return rc;
    DS_REQUIRE(aligned(s, 4) && aligned(tau, 8) && aligned(y, 4), "ds_delay_fwd: misaligned operand");
    delay_fwd_kernel<<<dim3((unsigned)ds::ceil_div(S, T), (unsigned)B), T, 0, ds::as_stream(stream)>>>(s, tau, S, K, hop, y);
    DS_LAUNCH_CHECK("delay_fwd_kernel");
    return DS_OK;
}

extern "C" int ds_delay_bwd(const float* gy, const float* s, const double* tau, int B, int S, int K, int hop, void* work,
                            int64_t work_bytes, float* gs, double* gtau, ds_stream_t stream) {
    if (int rc = check_args("ds_delay_bwd", gy && s && tau && work, B, S, K, hop)) return rc;
    DS_REQUIRE(work_bytes >= ds_delay_workspace_bytes(B, S, K, hop), "ds_delay_bwd: workspace of %lld bytes, %lld needed",
               (long long)work_bytes, (long long)ds_delay_workspace_bytes(B, S, K, hop));
    DS_REQUIRE(aligned(work, 16), "ds_delay_bwd: work not 16-byte aligned");
    DS_REQUIRE(aligned(gy, 4) && aligned(s, 4) && aligned(tau, 8) && aligned(gs, 4) && aligned(gtau, 8),
               "ds_delay_bwd: misaligned operand");
    hipStream_t st = ds::as_stream(stream);
    if (gs) {
        delay_gather_kernel<<<dim3((unsigned)ds::ceil_div(S, GT), (unsigned)B), GT, 0, st>>>(gy, tau, S, K, hop, gs);
        DS_LAUNCH_CHECK("delay_gather_kernel");
    }
    if (gtau) {
        double* q = static_cast<double*>(work);
        delay_slope_kernel<<<dim3((unsigned)ds::ceil_div(S, T), (unsigned)B), T, 0, st>>>(gy, s, tau, S, K, hop, q);
        DS_LAUNCH_CHECK("delay_slope_kernel");
        delay_gtau_kernel<<<dim3((unsigned)K, (unsigned)B), 64, 0, st>>>(q, S, K, hop, gtau);
        DS_LAUNCH_CHECK("delay_gtau_kernel");
    }
    return DS_OK;
}
