// Recording chain: a cascade of S second-order sections (biquads) over rendered rows, with gradients to the signal and to
// every coefficient - gfx950.
//
// Per section, zero initial state, coefficients (b0 b1 b2 a1 a2), a0 = 1 (direct form II):
//     w[n] = u[n] - a1 w[n-1] - a2 w[n-2] ;   v[n] = b0 w[n] + b1 w[n-1] + b2 w[n-2] ;   section s + 1 reads the v of section s.
// Backward, sections in reverse order, g the gradient at a section's output:
//     lam[n] = sum_k b_k g[n+k] - a1 lam[n+1] - a2 lam[n+2]   (the gradient at the section's input) ;
//     gb_k = sum_n g[n] w[n-k] ;   ga_k = - sum_n lam[n] w[n-k].
// The all-pole part and the three taps are both shift-invariant and start from rest, so they commute: lam is formed as
//     mu[n] = g[n] - a1 mu[n+1] - a2 mu[n+2] ;   lam[n] = b0 mu[n] + b1 mu[n+1] + b2 mu[n+2],
// which is the forward's section run down in time - the same lane code with REV = true.
//
// One wavefront owns a clip and walks it in tiles of 64 RUN samples (osc_scan::RUN a lane).  A lane keeps its RUN samples in
// registers and ALL sections run on the tile before the next one is loaded: x is read once, y written once.  Per section
// and tile, with the state s[n] = (w[n], w[n-1]) and the companion matrix A = [[-a1, -a2], [1, 0]], s[n] = A s[n-1] + (u[n], 0):
//     1. every lane runs its samples from the zero state -> its end state e_q ;
//     2. a 6-step shuffle scan joins them, v_q = sum_{p <= q} A^(RUN (q - p)) e_p, step o with the power A^(RUN o) ;
//     3. the state entering lane q is v_{q-1} + A^(RUN q) c, c the state the tile was entered with ;
//     4. the lane runs again from that state and forms its outputs; the tile leaves v_63 + A^(64 RUN) c to the next.
// The powers come from repeated squaring alone, once per (clip, section) at kernel entry: log2(RUN) squarings give A^RUN,
// six more A^(RUN 2^k) and A^(64 RUN), and lane q multiplies the ones of its set bits.  No closed form, so no case split on
// complex, real or repeated poles.  They live in LDS (4 doubles a lane and section), as do the carried states and, in the
// backward, every lane's five coefficient sums per section.
//
// Backward: biquad_fwd_kernel<true> runs the forward again and stores every section's w in fp64 (work: B S N doubles);
// biquad_bwd_kernel walks the tiles from the last to the first, the sections from the last to the first, reads w, adds
// g w into the lane's gb, runs the section down in time, adds lam w into the lane's ga.  The lanes' sums are joined by one
// butterfly at the end: fixed order, the same bits from the same inputs.
//
// No workgroup waits for another; every trip count and every index is a function of (B, N, S) and the thread's position,
// none of the data: coefficients of any value (unstable, inf, NaN) give inf or NaN in the outputs and nothing else.
#include <cstdint>

#include "ds_common.h"
#include "osc_scan.h"

namespace {

using osc_scan::from_prev;
using osc_scan::RUN;
using osc_scan::TILE;

constexpr int MAXS = DS_BIQUAD_MAX_SECTIONS;
static_assert((RUN & (RUN - 1)) == 0, "A^RUN comes from squarings alone");

struct vec2 {
    double a, b;
};
struct mat2 {
    double m00, m01, m10, m11;
};

__device__ __forceinline__ mat2 mmul(const mat2& x, const mat2& y) {
    return {x.m00 * y.m00 + x.m01 * y.m10, x.m00 * y.m01 + x.m01 * y.m11, x.m10 * y.m00 + x.m11 * y.m10,
            x.m10 * y.m01 + x.m11 * y.m11};
}
__device__ __forceinline__ vec2 mvec(const mat2& x, vec2 v) { return {x.m00 * v.a + x.m01 * v.b, x.m10 * v.a + x.m11 * v.b}; }

// what a clip's wavefront keeps in LDS
struct shared_t {
    double co[MAXS][5];      // b0 b1 b2 a1 a2
    double pw[MAXS][4][64];  // A^(RUN q) of lane position q (row-major entries)
    double pt[MAXS][4];      // A^(64 RUN)
    double carry[MAXS][2];   // the state entering the next tile
};

// coefficients and powers of every section of clip b; q = this lane's position in time order
__device__ __forceinline__ void setup(shared_t& sh, const double* __restrict__ sos, int per_clip, int b, int S, int q) {
    const double* base = sos + (per_clip ? (int64_t)b * S * 5 : 0);
    for (int s = 0; s < S; ++s) {
        double c[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) c[k] = base[s * 5 + k];
        mat2 M = {-c[3], -c[4], 1.0, 0.0};
#pragma unroll
        for (int r = 1; r < RUN; r <<= 1) M = mmul(M, M);  // A^RUN
        mat2 P = {1.0, 0.0, 0.0, 1.0};
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            if ((q >> k) & 1) P = mmul(M, P);
            M = mmul(M, M);
        }
#pragma unroll
        for (int k = 0; k < 5; ++k) sh.co[s][k] = c[k];
        sh.pw[s][0][q] = P.m00, sh.pw[s][1][q] = P.m01, sh.pw[s][2][q] = P.m10, sh.pw[s][3][q] = P.m11;
        sh.pt[s][0] = M.m00, sh.pt[s][1] = M.m01, sh.pt[s][2] = M.m10, sh.pt[s][3] = M.m11;
        sh.carry[s][0] = 0.0, sh.carry[s][1] = 0.0;
    }
    __syncthreads();
}

__device__ __forceinline__ mat2 power_of(const shared_t& sh, int s, int q) {
    return {sh.pw[s][0][q], sh.pw[s][1][q], sh.pw[s][2][q], sh.pw[s][3][q]};
}

// One section on one tile, in place: u[0..RUN) of this lane in, v out; wout (or nullptr) receives the lane's w.  REV: time
// runs down, the lanes and a lane's samples in reverse order.  The four steps of the head comment.
template <bool REV>
__device__ __forceinline__ void section_tile(shared_t& sh, int s, int lane, double* u, double* wout) {
    const int q = REV ? 63 - lane : lane;
    const double b0 = sh.co[s][0], b1 = sh.co[s][1], b2 = sh.co[s][2], a1 = sh.co[s][3], a2 = sh.co[s][4];
    // 1. from the zero state
    vec2 e = {0.0, 0.0};
#pragma unroll
    for (int ii = 0; ii < RUN; ++ii) {
        const int i = REV ? RUN - 1 - ii : ii;
        const double w = u[i] - a1 * e.a - a2 * e.b;
        e.b = e.a;
        e.a = w;
    }
    // 2. the scan over the lanes
    vec2 v = e;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const mat2 P = power_of(sh, s, o);
        const vec2 p = {from_prev<REV>(v.a, o), from_prev<REV>(v.b, o)};
        if (q >= o) {
            const vec2 t = mvec(P, p);
            v.a += t.a;
            v.b += t.b;
        }
    }
    // 3. the state entering this lane, and the one leaving the tile
    const vec2 c = {sh.carry[s][0], sh.carry[s][1]};
    vec2 x = {from_prev<REV>(v.a, 1), from_prev<REV>(v.b, 1)};
    if (q == 0) x = {0.0, 0.0};
    const vec2 cq = mvec(power_of(sh, s, q), c);
    x.a += cq.a;
    x.b += cq.b;
    const mat2 PT = {sh.pt[s][0], sh.pt[s][1], sh.pt[s][2], sh.pt[s][3]};
    const vec2 ct = mvec(PT, c);
    const int last = REV ? 0 : 63;
    sh.carry[s][0] = __shfl(v.a, last, 64) + ct.a;  // (every lane stores the same bits)
    sh.carry[s][1] = __shfl(v.b, last, 64) + ct.b;
    // 4. again, from the entering state
#pragma unroll
    for (int ii = 0; ii < RUN; ++ii) {
        const int i = REV ? RUN - 1 - ii : ii;
        const double w = u[i] - a1 * x.a - a2 * x.b;
        u[i] = b0 * w + b1 * x.a + b2 * x.b;
        if (wout) wout[i] = w;
        x.b = x.a;
        x.a = w;
    }
}

// One wavefront a clip.  SAVE = false: y.  SAVE = true: every section's w into wsave (B x S x N fp64), no y.
template <bool SAVE>
__global__ void __launch_bounds__(64)
    biquad_fwd_kernel(const float* __restrict__ x, const double* __restrict__ sos, int per_clip, int N, int S,
                      float* __restrict__ y, double* __restrict__ wsave) {
    __shared__ shared_t sh;
    const int b = blockIdx.x, lane = threadIdx.x;
    setup(sh, sos, per_clip, b, S, lane);
    const float* xrow = x + (int64_t)b * N;
    const int ntiles = (int)(((int64_t)N + TILE - 1) / TILE);
    for (int tile = 0; tile < ntiles; ++tile) {
        const int64_t t0 = (int64_t)tile * TILE + lane * RUN;
        double u[RUN], w[RUN];
#pragma unroll
        for (int i = 0; i < RUN; ++i) u[i] = t0 + i < N ? (double)xrow[t0 + i] : 0.0;
        for (int s = 0; s < S; ++s) {
            section_tile<false>(sh, s, lane, u, SAVE ? w : nullptr);
            if (SAVE) {
                double* wrow = wsave + ((int64_t)b * S + s) * N;
#pragma unroll
                for (int i = 0; i < RUN; ++i)
                    if (t0 + i < N) wrow[t0 + i] = w[i];
            }
        }
        if (!SAVE) {
            float* yrow = y + (int64_t)b * N;
#pragma unroll
            for (int i = 0; i < RUN; ++i)
                if (t0 + i < N) yrow[t0 + i] = (float)u[i];
        }
    }
}

// One wavefront a clip, down in time: gx (B x N) and gsos (B x S x 5) from gy and the stored w.
__global__ void __launch_bounds__(64)
    biquad_bwd_kernel(const float* __restrict__ gy, const double* __restrict__ sos, int per_clip, int N, int S,
                      const double* __restrict__ wsave, float* __restrict__ gx, double* __restrict__ gsos) {
    __shared__ shared_t sh;
    __shared__ double acc[MAXS][5][64];  // a lane's sums: gb0 gb1 gb2 ga1 ga2
    const int b = blockIdx.x, lane = threadIdx.x;
    setup(sh, sos, per_clip, b, S, 63 - lane);
    for (int s = 0; s < S; ++s)
#pragma unroll
        for (int k = 0; k < 5; ++k) acc[s][k][lane] = 0.0;
    const float* grow = gy + (int64_t)b * N;
    float* gxrow = gx + (int64_t)b * N;
    const int ntiles = (int)(((int64_t)N + TILE - 1) / TILE);
    for (int tile = ntiles - 1; tile >= 0; --tile) {
        const int64_t t0 = (int64_t)tile * TILE + lane * RUN;
        double g[RUN];
#pragma unroll
        for (int i = 0; i < RUN; ++i) g[i] = t0 + i < N ? (double)grow[t0 + i] : 0.0;
        for (int s = S - 1; s >= 0; --s) {
            const double* wrow = wsave + ((int64_t)b * S + s) * N;
            double w[RUN + 2];  // w[n-2], w[n-1], then the lane's own samples; 0 outside [0, N)
#pragma unroll
            for (int i = 0; i < RUN + 2; ++i) {
                const int64_t t = t0 + i - 2;
                w[i] = (t >= 0 && t < N) ? wrow[t] : 0.0;
            }
            double s0 = acc[s][0][lane], s1 = acc[s][1][lane], s2 = acc[s][2][lane];
#pragma unroll
            for (int i = RUN - 1; i >= 0; --i) {
                s0 += g[i] * w[i + 2];
                s1 += g[i] * w[i + 1];
                s2 += g[i] * w[i];
            }
            acc[s][0][lane] = s0, acc[s][1][lane] = s1, acc[s][2][lane] = s2;
            section_tile<true>(sh, s, lane, g, nullptr);  // g is lam now
            double r1 = acc[s][3][lane], r2 = acc[s][4][lane];
#pragma unroll
            for (int i = RUN - 1; i >= 0; --i) {
                r1 -= g[i] * w[i + 1];
                r2 -= g[i] * w[i];
            }
            acc[s][3][lane] = r1, acc[s][4][lane] = r2;
        }
#pragma unroll
        for (int i = 0; i < RUN; ++i)
            if (t0 + i < N) gxrow[t0 + i] = (float)g[i];
    }
    for (int s = 0; s < S; ++s)
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const double v = ds::wave_sum(acc[s][k][lane]);
            if (lane == 0) gsos[((int64_t)b * S + s) * 5 + k] = v;
        }
}

using ds::aligned;

int check_args(const char* fn, bool pointers, int per_clip, int B, int N, int S) {
    DS_REQUIRE(pointers, "%s: null pointer", fn);
    DS_REQUIRE(B > 0 && N > 0 && S > 0, "%s: empty problem (B %d, N %d, S %d)", fn, B, N, S);
    DS_REQUIRE(B <= DS_BIQUAD_MAX_ROWS, "%s: B = %d above %d", fn, B, DS_BIQUAD_MAX_ROWS);
    DS_REQUIRE(S <= DS_BIQUAD_MAX_SECTIONS, "%s: S = %d sections above %d", fn, S, DS_BIQUAD_MAX_SECTIONS);
    DS_REQUIRE(per_clip == 0 || per_clip == 1, "%s: per_clip = %d is neither 0 nor 1", fn, per_clip);
    return DS_OK;
}

}  // namespace

extern "C" int64_t ds_biquad_workspace_bytes(int B, int N, int S) {
    if (B <= 0 || B > DS_BIQUAD_MAX_ROWS || N <= 0 || S <= 0 || S > DS_BIQUAD_MAX_SECTIONS) return 0;
    return (int64_t)sizeof(double) * B * S * N;
}

extern "C" int ds_biquad_fwd(const float* x, const double* sos, int per_clip, int B, int N, int S, float* y,
                             ds_stream_t stream) {
    if (int rc = check_args("ds_biquad_fwd", x && sos && y, per_clip, B, N, S)) return rc;
    DS_REQUIRE(aligned(x, 4) && aligned(sos, 8) && aligned(y, 4), "ds_biquad_fwd: misaligned operand");
    biquad_fwd_kernel<false><<<dim3((unsigned)B), 64, 0, ds::as_stream(stream)>>>(x, sos, per_clip, N, S, y, nullptr);
    DS_LAUNCH_CHECK("biquad_fwd_kernel");
    return DS_OK;
}

extern "C" int ds_biquad_bwd(const float* gy, const float* x, const double* sos, int per_clip, int B, int N, int S, void* work,
                             int64_t work_bytes, float* gx, double* gsos, ds_stream_t stream) {
    if (int rc = check_args("ds_biquad_bwd", gy && x && sos && work && gx && gsos, per_clip, B, N, S)) return rc;
    DS_REQUIRE(aligned(gy, 4) && aligned(x, 4) && aligned(sos, 8) && aligned(gx, 4) && aligned(gsos, 8),
               "ds_biquad_bwd: misaligned operand");
    DS_REQUIRE(aligned(work, 16), "ds_biquad_bwd: work not 16-byte aligned");
    DS_REQUIRE(work_bytes >= ds_biquad_workspace_bytes(B, N, S), "ds_biquad_bwd: workspace of %lld bytes, %lld needed",
               (long long)work_bytes, (long long)ds_biquad_workspace_bytes(B, N, S));
    hipStream_t st = ds::as_stream(stream);
    double* w = static_cast<double*>(work);
    biquad_fwd_kernel<true><<<dim3((unsigned)B), 64, 0, st>>>(x, sos, per_clip, N, S, nullptr, w);
    DS_LAUNCH_CHECK("biquad_fwd_kernel");
    biquad_bwd_kernel<<<dim3((unsigned)B), 64, 0, st>>>(gy, sos, per_clip, N, S, w, gx, gsos);
    DS_LAUNCH_CHECK("biquad_bwd_kernel");
    return DS_OK;
}
