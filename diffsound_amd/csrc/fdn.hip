// Late reverberation: a feedback delay network over rendered rows, with gradients to the signal and to every coefficient - gfx950.
//
// Row b of B uses set r = b mod H of H; n delay lines with fixed integer delays m_j >= DS_FDN_MIN_DELAY, everything from rest:
//     q_j[t] = (1 - p_j) s_j[t - m_j] + p_j s_j[t - m_j - 1]          line j's output: its delay and a two-tap absorption low-pass
//     s_i[t] = b_i x[t] + sum_j A_ij q_j[t]                           what enters line i (kept in `state` for the backward)
//     y[t]   = d x[t]   + sum_j c_j q_j[t]
// and, with r the gradient at q and l the gradient at s (both zero from N on),
//     l_i[t] = (1 - p_i) r_i[t + m_i] + p_i r_i[t + m_i + 1]          r_j[t] = c_j gy[t] + sum_i A_ij l_i[t]
//     gx[t] = d gy[t] + sum_i b_i l_i[t]      gb_i = sum_t l_i[t] x[t]      gA_ij = sum_t l_i[t] q_j[t]
//     gc_j  = sum_t gy[t] q_j[t]              gd   = sum_t gy[t] x[t]       gp_j  = sum_t r_j[t] (s_j[t-m_j-1] - s_j[t-m_j])
//
// THE BLOCK LOOP.  Every delay is at least T = min(min_j m_j, FDN_THREADS) and the damping tap only reaches further back, so
// the T samples of block [k T, (k + 1) T) read only state written by earlier blocks.  One workgroup owns a row and walks its
// blocks in order; inside a block one lane owns a sample: it reads the 2 n delayed values (coalesced along t), forms q, and the
// n x n product runs in its registers against the set's coefficients in LDS (uniform addresses: broadcasts).  The history is
// far too large for LDS and lives in `state`; the workgroup that wrote it is the only one that reads it back, so the
// workgroup barrier at the end of a block is the whole hand-off.  No workgroup waits for another.  The backward is the same
// loop in reverse time with A read transposed: its history is r (l_i[t] reads r_i at a different time for every i, so r is
// what has to be kept), in the first B n N doubles of the workspace, and l is two reads of it, as q is two reads of s.
// Sums over j start from the x (gy) term and add j ascending, so no result depends on the block length.
//
// THE PARAMETER SUMS.  Every one is a dot product over t of two of the 4 n + 2 rows l_i, q_j, r_j, s_j[t-m_j-1] - s_j[t-m_j],
// x, gy.  fdn_sums_kernel: workgroup (row b, chunk c of FDN_CHUNK samples - a compile-time constant, never a function of the
// device) stages RED_TILE samples of the rows in LDS (row stride 65 doubles: the 32 rows a wavefront touches on 32 bank pairs)
// and thread o owns output o of the n^2 + 3 n + 1 (and o + 256): one accumulator or two, t ascending.  Partials go to
// work[B n N + (b nchunk + c) NOUT + o]; fdn_join_kernel, a second launch, adds per (r, o) the chunks in ascending order within a
// row and then the rows in ascending order.  No atomics, no read-modify-write in memory: the same bits on any device.  An
// output that is NULL is not accumulated and not stored.
//
// Every trip count is a function of (B, H, N, n) and the delays; no index depends on x, gy or a coefficient.  A delay below
// DS_FDN_MIN_DELAY is the caller's error (the delays are device memory and are never read on the host); the kernels clamp
// it to the minimum, so that no index leaves the row whatever the array holds.
#include <cstdint>

#include "ds_common.h"

namespace {

constexpr int FDN_THREADS = 256;  // lanes of a row's workgroup: the longest block of samples
constexpr int FDN_CHUNK = 1024;   // samples of one partial of the parameter sums
constexpr int RED_TILE = 64;      // samples of the rows staged at a time
constexpr int RED_THREADS = 256;
constexpr int MAXN = DS_FDN_MAX_LINES;
static_assert(FDN_CHUNK % RED_TILE == 0 && MAXN * MAXN <= RED_THREADS && MAXN * MAXN + 3 * MAXN + 1 <= 2 * RED_THREADS,
              "a chunk is whole tiles; a thread owns at most two outputs");

template <int NL>
struct set_t {
    double A[NL * NL];  // A[i NL + j]
    double b[NL], c[NL], p[NL], omp[NL], d;
    int m[NL];
};

// the set of this row into LDS; returns the block length T.  Ends with a barrier.
template <int NL>
__device__ __forceinline__ int load_set(set_t<NL>& sh, int set, int n, const int32_t* __restrict__ delays,
                                        const double* __restrict__ A, const double* __restrict__ b, const double* __restrict__ c,
                                        const double* __restrict__ d, const double* __restrict__ p) {
    const int tid = threadIdx.x;
    for (int e = tid; e < n * n; e += blockDim.x) sh.A[(e / n) * NL + e % n] = A[(int64_t)set * n * n + e];
    if (tid < n) {
        const int64_t e = (int64_t)set * n + tid;
        const double pv = p ? p[e] : 0.0;
        sh.b[tid] = b[e], sh.c[tid] = c[e], sh.p[tid] = pv, sh.omp[tid] = 1.0 - pv;
        const int m = delays[e];
        sh.m[tid] = m < DS_FDN_MIN_DELAY ? DS_FDN_MIN_DELAY : m;
    }
    if (tid == 0) sh.d = d[set];
    __syncthreads();
    int T = FDN_THREADS;
    for (int j = 0; j < n; ++j) T = sh.m[j] < T ? sh.m[j] : T;
    return T;
}

template <int NL>
__global__ void __launch_bounds__(FDN_THREADS)
    fdn_fwd_kernel(const float* __restrict__ x, const int32_t* __restrict__ delays, const double* __restrict__ A,
                   const double* __restrict__ b, const double* __restrict__ c, const double* __restrict__ d,
                   const double* __restrict__ p, int H, int N, int n, double* state, float* __restrict__ y) {
    __shared__ set_t<NL> sh;
    const int row = blockIdx.x, tid = threadIdx.x;
    const int T = load_set(sh, row % H, n, delays, A, b, c, d, p);
    const float* xr = x + (int64_t)row * N;
    float* yr = y + (int64_t)row * N;
    double* st = state + (int64_t)row * n * N;
    for (int64_t t0 = 0; t0 < N; t0 += T) {
        const int64_t t = t0 + tid;
        if (tid < T && t < N) {
            double q[NL];
#pragma unroll
            for (int j = 0; j < NL; ++j)
                if (j < n) {
                    const int64_t u = t - sh.m[j];  // u < t0: written by an earlier block
                    const double* sj = st + (int64_t)j * N;
                    const double s0 = u >= 0 ? sj[u] : 0.0, s1 = u >= 1 ? sj[u - 1] : 0.0;
                    q[j] = __builtin_fma(sh.p[j], s1, sh.omp[j] * s0);
                }
            const double xv = (double)xr[t];
            double acc = sh.d * xv;
#pragma unroll
            for (int j = 0; j < NL; ++j)
                if (j < n) acc = __builtin_fma(sh.c[j], q[j], acc);
            yr[t] = (float)acc;
#pragma unroll
            for (int i = 0; i < NL; ++i)
                if (i < n) {
                    double s = sh.b[i] * xv;
#pragma unroll
                    for (int j = 0; j < NL; ++j)
                        if (j < n) s = __builtin_fma(sh.A[i * NL + j], q[j], s);
                    st[(int64_t)i * N + t] = s;
                }
        }
        __syncthreads();  // the block's state is written before the next block reads it
    }
}

// r (the workspace's first B n N doubles) and gx, blocks in descending order
template <int NL>
__global__ void __launch_bounds__(FDN_THREADS)
    fdn_bwd_kernel(const float* __restrict__ gy, const int32_t* __restrict__ delays, const double* __restrict__ A,
                   const double* __restrict__ b, const double* __restrict__ c, const double* __restrict__ d,
                   const double* __restrict__ p, int H, int N, int n, double* rh, float* __restrict__ gx) {
    __shared__ set_t<NL> sh;
    const int row = blockIdx.x, tid = threadIdx.x;
    const int T = load_set(sh, row % H, n, delays, A, b, c, d, p);
    const float* gr = gy + (int64_t)row * N;
    double* rr = rh + (int64_t)row * n * N;
    for (int64_t t0 = (((int64_t)N - 1) / T) * T; t0 >= 0; t0 -= T) {
        const int64_t t = t0 + tid;
        if (tid < T && t < N) {
            double l[NL];
#pragma unroll
            for (int i = 0; i < NL; ++i)
                if (i < n) {
                    const int64_t v = t + sh.m[i];  // v >= t0 + T: written by a block already done
                    const double* ri = rr + (int64_t)i * N;
                    const double r0 = v < N ? ri[v] : 0.0, r1 = v + 1 < N ? ri[v + 1] : 0.0;
                    l[i] = __builtin_fma(sh.p[i], r1, sh.omp[i] * r0);
                }
            const double g = (double)gr[t];
            if (gx) {
                double acc = sh.d * g;
#pragma unroll
                for (int i = 0; i < NL; ++i)
                    if (i < n) acc = __builtin_fma(sh.b[i], l[i], acc);
                gx[(int64_t)row * N + t] = (float)acc;
            }
#pragma unroll
            for (int j = 0; j < NL; ++j)
                if (j < n) {
                    double r = sh.c[j] * g;
#pragma unroll
                    for (int i = 0; i < NL; ++i)
                        if (i < n) r = __builtin_fma(sh.A[i * NL + j], l[i], r);
                    rr[(int64_t)j * N + t] = r;
                }
        }
        __syncthreads();
    }
}

// the outputs of the parameter sums, in the partials' order: gA (n^2), gb (n), gc (n), gd (1), gp (n)
enum { WANT_A = 1, WANT_B = 2, WANT_C = 4, WANT_D = 8, WANT_P = 16 };
__host__ __device__ inline int nout(int n) { return n * n + 3 * n + 1; }

constexpr int RED_STRIDE = RED_TILE + 1;
struct rows_t {
    double v[(4 * MAXN + 2) * RED_STRIDE];  // rows l_i (i), q_j (n + j), r_j (2 n + j), s_j[t-m_j-1] - s_j[t-m_j] (3 n + j), x (4 n), gy (4 n + 1)
    double p[MAXN], omp[MAXN];
    int m[MAXN];
};

// the two rows of output o, or false where nobody asked for it
__device__ __forceinline__ bool rows_of(int o, int n, int want, int& u, int& v) {
    if (o < n * n) return u = o / n, v = n + o % n, (want & WANT_A) != 0;
    o -= n * n;
    if (o < n) return u = o, v = 4 * n, (want & WANT_B) != 0;
    o -= n;
    if (o < n) return u = 4 * n + 1, v = n + o, (want & WANT_C) != 0;
    o -= n;
    if (o < 1) return u = 4 * n + 1, v = 4 * n, (want & WANT_D) != 0;
    o -= 1;
    if (o < n) return u = 2 * n + o, v = 3 * n + o, (want & WANT_P) != 0;
    return u = v = 0, false;
}

__global__ void __launch_bounds__(RED_THREADS)
    fdn_sums_kernel(const float* __restrict__ gy, const float* __restrict__ x, const int32_t* __restrict__ delays,
                    const double* __restrict__ p, int H, int N, int n, int nchunk, int want, const double* __restrict__ state,
                    const double* __restrict__ rh, double* __restrict__ part) {
    __shared__ rows_t sh;
    const int row = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x;
    if (tid < n) {
        const int64_t e = (int64_t)(row % H) * n + tid;
        const double pv = p ? p[e] : 0.0;
        sh.p[tid] = pv, sh.omp[tid] = 1.0 - pv;
        const int m = delays[e];
        sh.m[tid] = m < DS_FDN_MIN_DELAY ? DS_FDN_MIN_DELAY : m;
    }
    int u0, v0, u1, v1;
    const bool on0 = rows_of(tid, n, want, u0, v0), on1 = rows_of(tid + RED_THREADS, n, want, u1, v1);
    double acc0 = 0.0, acc1 = 0.0;
    const float* xr = x + (int64_t)row * N;
    const float* gr = gy + (int64_t)row * N;
    const double* st = state + (int64_t)row * n * N;
    const double* rr = rh + (int64_t)row * n * N;
    const int64_t c0 = (int64_t)chunk * FDN_CHUNK, c1 = c0 + FDN_CHUNK < N ? c0 + FDN_CHUNK : N;
    const int k = tid % RED_TILE;
    for (int64_t t0 = c0; t0 < c1; t0 += RED_TILE) {
        __syncthreads();  // the tile before has been read (and, the first time, the set is in LDS)
        const int64_t t = t0 + k;
        const bool in = t < c1;
        for (int j = tid / RED_TILE; j < n; j += RED_THREADS / RED_TILE) {
            const int64_t u = t - sh.m[j], w = t + sh.m[j];
            const double* sj = st + (int64_t)j * N;
            const double* rj = rr + (int64_t)j * N;
            const double s0 = in && u >= 0 ? sj[u] : 0.0, s1 = in && u >= 1 ? sj[u - 1] : 0.0;
            const double r0 = in && w < N ? rj[w] : 0.0, r1 = in && w + 1 < N ? rj[w + 1] : 0.0;
            sh.v[j * RED_STRIDE + k] = __builtin_fma(sh.p[j], r1, sh.omp[j] * r0);
            sh.v[(n + j) * RED_STRIDE + k] = __builtin_fma(sh.p[j], s1, sh.omp[j] * s0);
            sh.v[(2 * n + j) * RED_STRIDE + k] = in ? rj[t] : 0.0;
            sh.v[(3 * n + j) * RED_STRIDE + k] = s1 - s0;
        }
        if (tid < RED_TILE) {
            sh.v[4 * n * RED_STRIDE + k] = in ? (double)xr[t] : 0.0;
            sh.v[(4 * n + 1) * RED_STRIDE + k] = in ? (double)gr[t] : 0.0;
        }
        __syncthreads();
        const int cnt = (int)(c1 - t0 < RED_TILE ? c1 - t0 : RED_TILE);
        if (on0)
            for (int e = 0; e < cnt; ++e) acc0 = __builtin_fma(sh.v[u0 * RED_STRIDE + e], sh.v[v0 * RED_STRIDE + e], acc0);
        if (on1)
            for (int e = 0; e < cnt; ++e) acc1 = __builtin_fma(sh.v[u1 * RED_STRIDE + e], sh.v[v1 * RED_STRIDE + e], acc1);
    }
    double* prow = part + ((int64_t)row * nchunk + chunk) * nout(n);
    if (on0) prow[tid] = acc0;
    if (on1) prow[tid + RED_THREADS] = acc1;
}

// per (set r, output o): the chunks in ascending order within a row, then the rows in ascending order
__global__ void __launch_bounds__(256)
    fdn_join_kernel(const double* __restrict__ part, int B, int H, int n, int nchunk, double* __restrict__ gA,
                    double* __restrict__ gb, double* __restrict__ gc, double* __restrict__ gd, double* __restrict__ gp) {
    const int no = nout(n);
    const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= (int64_t)H * no) return;
    const int r = (int)(id / no);
    int o = (int)(id % no);
    double* out;
    if (o < n * n) out = gA ? gA + (int64_t)r * n * n + o : nullptr;
    else if ((o -= n * n) < n) out = gb ? gb + (int64_t)r * n + o : nullptr;
    else if ((o -= n) < n) out = gc ? gc + (int64_t)r * n + o : nullptr;
    else if ((o -= n) < 1) out = gd ? gd + r : nullptr;
    else out = gp ? gp + (int64_t)r * n + (o - 1) : nullptr;
    if (!out) return;
    o = (int)(id % no);
    double total = 0.0;
    for (int b = r; b < B; b += H) {
        double s = 0.0;
        for (int c = 0; c < nchunk; ++c) s += part[((int64_t)b * nchunk + c) * no + o];
        total += s;
    }
    *out = total;
}

using ds::aligned;

int check_args(const char* fn, bool pointers, int B, int H, int N, int n) {
    DS_REQUIRE(pointers, "%s: null pointer", fn);
    DS_REQUIRE(B > 0 && H > 0 && N > 0 && n > 0, "%s: empty problem (B %d, H %d, N %d, n %d)", fn, B, H, N, n);
    DS_REQUIRE(B <= DS_FDN_MAX_ROWS, "%s: B = %d above %d", fn, B, DS_FDN_MAX_ROWS);
    DS_REQUIRE(n <= DS_FDN_MAX_LINES, "%s: n = %d lines above %d", fn, n, DS_FDN_MAX_LINES);
    DS_REQUIRE(H <= B && B % H == 0, "%s: B = %d is not a multiple of H = %d", fn, B, H);
    return DS_OK;
}

inline int nchunks(int N) { return (int)(((int64_t)N + FDN_CHUNK - 1) / FDN_CHUNK); }

// f.template operator()<NL>() at the smallest instantiated NL >= n
template <class F>
void with_lines(int n, F f) {
    if (n <= 4) f.template operator()<4>();
    else if (n <= 8) f.template operator()<8>();
    else f.template operator()<16>();
}

struct fwd_launch {
    const float* x; const int32_t* delays; const double *A, *b, *c, *d, *p; int B, H, N, n; double* state; float* y; hipStream_t st;
    template <int NL>
    void operator()() const {
        fdn_fwd_kernel<NL><<<dim3((unsigned)B), FDN_THREADS, 0, st>>>(x, delays, A, b, c, d, p, H, N, n, state, y);
    }
};

struct bwd_launch {
    const float* gy; const int32_t* delays; const double *A, *b, *c, *d, *p; int B, H, N, n; double* rh; float* gx; hipStream_t st;
    template <int NL>
    void operator()() const {
        fdn_bwd_kernel<NL><<<dim3((unsigned)B), FDN_THREADS, 0, st>>>(gy, delays, A, b, c, d, p, H, N, n, rh, gx);
    }
};

}  // namespace

extern "C" int64_t ds_fdn_workspace_bytes(int B, int H, int N, int n) {
    if (B <= 0 || H <= 0 || N <= 0 || n <= 0 || B > DS_FDN_MAX_ROWS || n > DS_FDN_MAX_LINES || H > B || B % H) return 0;
    return (int64_t)sizeof(double) * B * ((int64_t)n * N + (int64_t)nchunks(N) * nout(n));
}

extern "C" int ds_fdn_fwd(const float* x, const int32_t* delays, const double* A, const double* b, const double* c, const double* d,
                          const double* p, int B, int H, int N, int n, double* state, float* y, ds_stream_t stream) {
    if (int rc = check_args("ds_fdn_fwd", x && delays && A && b && c && d && state && y, B, H, N, n)) return rc;
    DS_REQUIRE(aligned(x, 4) && aligned(delays, 4) && aligned(A, 8) && aligned(b, 8) && aligned(c, 8) && aligned(d, 8) &&
                   aligned(p, 8) && aligned(state, 8) && aligned(y, 4),
               "ds_fdn_fwd: misaligned operand");
    with_lines(n, fwd_launch{x, delays, A, b, c, d, p, B, H, N, n, state, y, ds::as_stream(stream)});
    return DS_LAUNCHED("fdn_fwd_kernel");
}

extern "C" int ds_fdn_bwd(const float* gy, const float* x, const int32_t* delays, const double* A, const double* b, const double* c,
                          const double* d, const double* p, int B, int H, int N, int n, const double* state, void* work,
                          int64_t work_bytes, float* gx, double* gA, double* gb, double* gc, double* gd, double* gp,
                          ds_stream_t stream) {
    if (int rc = check_args("ds_fdn_bwd", gy && x && delays && A && b && c && d && state && work, B, H, N, n)) return rc;
    DS_REQUIRE(aligned(gy, 4) && aligned(x, 4) && aligned(delays, 4) && aligned(A, 8) && aligned(b, 8) && aligned(c, 8) &&
                   aligned(d, 8) && aligned(p, 8) && aligned(state, 8) && aligned(gx, 4) && aligned(gA, 8) && aligned(gb, 8) &&
                   aligned(gc, 8) && aligned(gd, 8) && aligned(gp, 8),
               "ds_fdn_bwd: misaligned operand");
    DS_REQUIRE(gx || gA || gb || gc || gd || gp, "ds_fdn_bwd: every output is NULL");
    DS_REQUIRE(aligned(work, 16), "ds_fdn_bwd: work not 16-byte aligned");
    DS_REQUIRE(work_bytes >= ds_fdn_workspace_bytes(B, H, N, n), "ds_fdn_bwd: workspace of %lld bytes, %lld needed",
               (long long)work_bytes, (long long)ds_fdn_workspace_bytes(B, H, N, n));
    hipStream_t st = ds::as_stream(stream);
    double* rh = static_cast<double*>(work);
    with_lines(n, bwd_launch{gy, delays, A, b, c, d, p, B, H, N, n, rh, gx, st});
    DS_LAUNCH_CHECK("fdn_bwd_kernel");
    const int want = (gA ? WANT_A : 0) | (gb ? WANT_B : 0) | (gc ? WANT_C : 0) | (gd ? WANT_D : 0) | (gp ? WANT_P : 0);
    if (want) {
        double* part = rh + (int64_t)B * n * N;
        const int nchunk = nchunks(N);
        fdn_sums_kernel<<<dim3((unsigned)nchunk, (unsigned)B), RED_THREADS, 0, st>>>(gy, x, delays, p, H, N, n, nchunk, want, state,
                                                                                     rh, part);
        DS_LAUNCH_CHECK("fdn_sums_kernel");
        const int64_t total = (int64_t)H * nout(n);
        fdn_join_kernel<<<dim3((unsigned)((total + 255) / 256)), 256, 0, st>>>(part, B, H, n, nchunk, gA, gb, gc, gd, gp);
        DS_LAUNCH_CHECK("fdn_join_kernel");
    }
    return DS_OK;
}
