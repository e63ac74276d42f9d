// Room response: a long causal FIR over rendered rows, with gradients to the signal and to every tap - gfx950.
//
// Row b of B uses response r = b mod H of H, L taps each, zero initial state, the output cut at N:
//     y[b,t]  = sum_{j=0..min(t, L-1)}      h[r,j] x[b,t-j]
//     gx[b,s] = sum_{j=0..min(L-1, N-1-s)}  h[r,j] gy[b,s+j]
//     gh[r,j] = sum_{b = r, r+H, ...} sum_{t=j..N-1} gy[b,t] x[b,t-j]                  (an empty sum, exactly 0, for j >= N)
// Direct form, products and sums in fp64, y and gx rounded to fp32 once on the store, gh kept in fp64.  No FFT: the chain's
// kernels are exact to a derived bound and give the same bits from the same inputs, and an fp32 FFT gives neither.
//
// The three sums are ONE correlation  out[p] = sum_q a[q] w[p+q]  (a and w zero outside their ranges):
//     gx:  p = s,  a = h[r,:],  w = gy[b,:]
//     y :  the same on the row read backwards: with x'[u] = x[N-1-u], y'[u] = y[N-1-u] the first line is y'[u] = sum_j h[j] x'[u+j]
//     gh:  p = j (the lag),  q = s = t - j,  a = x[b,:],  w = gy[b,:]
// and correlate() below is the one loop that runs them.  A workgroup is one wavefront and owns TILE = 64 R consecutive p,
// lane l the R of them from l R on, their sums in registers.  The q range is walked in passes of TAPS: both operands of a pass
// are staged in LDS already converted to fp64 - a[q0 .. q0+TAPS) and w[p0+q0 .. p0+q0+TILE+TAPS) - and per step q a lane reads
// one broadcast a[q] and ONE new window value w[p+R-1+q+1]; the R window values live in registers, rotated by unrolling R steps.
// R = 8 multiply-adds per two 8-byte LDS reads: bound by the fp64 FMA rate, not by LDS.  The window is read at a stride of R
// doubles from lane to lane, an 8-way bank conflict for 8-byte reads; the staged window is therefore padded by one double
// after every R (element e at e + e / R): stride 9 doubles = 18 banks, gcd(18, 64) = 2, the 32 lanes of a group on 32
// different bank pairs.  LDS: 8 (TAPS + (TILE + TAPS) 9 / 8 + 1) = 8968 bytes a workgroup, 16 registers of sums and 16 of window.
//
// The causal triangle: tile p0 of y' / gx has min(L, N - p0) taps, so the tiles with the smallest p0 are the heaviest and get
// the smallest block indices - launched first; the row index varies fastest, so all rows' heavy tiles go first.
//
// gh: the samples s are split into chunks of GH_CHUNK - a compile-time constant, never a function of the device - and the
// workgroup of (row b, chunk c, lag tile) writes its partial sums to work[(b nchunk + c) Lc + j], Lc = min(L, N); pairs with
// c GH_CHUNK + j0 >= N are empty and skipped.  fir_gh_join_kernel, a second launch, adds for every (r, j) the chunks in
// ascending order within a row and then the rows in ascending order, reading only partials that were written.  No workgroup
// waits for another and nothing is added in memory by two of them: the same inputs give the same bits on any device.
//
// Every trip count and every index is a function of (B, H, N, L) and the thread's position, none of the data: non-finite
// inputs give inf or NaN in the outputs and nothing else.
#include <cstdint>

#include "ds_common.h"

namespace {

constexpr int R = 8;            // consecutive outputs (or lags) a lane owns
constexpr int TILE = 64 * R;    // outputs (y, gx) or lags (gh) a workgroup owns
constexpr int TAPS = 256;       // steps q of one staged pass
constexpr int GH_CHUNK = 2048;  // samples s of one gh partial
static_assert(TAPS % R == 0 && GH_CHUNK % TAPS == 0, "a pass is whole rotations of the window, a chunk whole passes");

constexpr int WIN = TILE + TAPS;  // staged window values of a pass
__device__ __forceinline__ int pad(int e) { return e + e / R; }

struct shared_t {
    double a[TAPS];
    double w[WIN + WIN / R + 1];
};

// acc[i] += sum_{q in [q_lo, q_hi)} a(q) w(p0 + l R + i + q),  l the lane.  a(q) is asked only for q in [q_lo, q_hi); w(e) for
// any e >= 0 and answers 0 outside its row.  The passes are whole: past q_hi the staged a is 0.
template <class A, class W>
__device__ __forceinline__ void correlate(shared_t& sh, int lane, int64_t p0, int64_t q_lo, int64_t q_hi, A a, W w,
                                          double (&acc)[R]) {
    for (int64_t q0 = q_lo; q0 < q_hi; q0 += TAPS) {
        __syncthreads();  // the pass before has been read
        for (int k = lane; k < TAPS; k += 64) sh.a[k] = q0 + k < q_hi ? a(q0 + k) : 0.0;
        for (int e = lane; e < WIN; e += 64) sh.w[pad(e)] = w(p0 + q0 + e);
        __syncthreads();
        double win[R];
#pragma unroll
        for (int i = 0; i < R; ++i) win[i] = sh.w[pad(lane * R + i)];
        for (int k = 0; k < TAPS; k += R) {
#pragma unroll
            for (int u = 0; u < R; ++u) {
                const double av = sh.a[k + u];
#pragma unroll
                for (int i = 0; i < R; ++i) acc[i] += av * win[(i + u) % R];
                win[u] = sh.w[pad(lane * R + R + k + u)];  // k + u + R <= TAPS + R - 1: inside the staged window
            }
        }
    }
}

// y (REV = true: the row backwards) or gx (REV = false) of row b = blockIdx.x, tiles blockIdx.y, + gridDim.y, ...
template <bool REV>
__global__ void __launch_bounds__(64)
    fir_conv_kernel(const float* __restrict__ in, const double* __restrict__ h, int H, int N, int L, float* __restrict__ out) {
    __shared__ shared_t sh;
    const int b = blockIdx.x, lane = threadIdx.x;
    const float* row = in + (int64_t)b * N;
    const double* hr = h + (int64_t)(b % H) * L;
    float* orow = out + (int64_t)b * N;
    const int ntiles = (int)(((int64_t)N + TILE - 1) / TILE);
    for (int tile = blockIdx.y; tile < ntiles; tile += gridDim.y) {
        const int64_t p0 = (int64_t)tile * TILE;
        const int64_t q_hi = (int64_t)L < N - p0 ? (int64_t)L : N - p0;
        double acc[R];
#pragma unroll
        for (int i = 0; i < R; ++i) acc[i] = 0.0;
        correlate(
            sh, lane, p0, 0, q_hi, [&](int64_t q) { return hr[q]; },
            [&](int64_t e) { return e < N ? (double)row[REV ? N - 1 - e : e] : 0.0; }, acc);
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const int64_t p = p0 + lane * R + i;
            if (p < N) orow[REV ? N - 1 - p : p] = (float)acc[i];
        }
    }
}

// gh partials of row b = blockIdx.x: task = chunk * nlt + lag tile, tasks blockIdx.y, + gridDim.y, ...
__global__ void __launch_bounds__(64)
    fir_gh_kernel(const float* __restrict__ gy, const float* __restrict__ x, int N, int Lc, int nchunk, int nlt,
                  double* __restrict__ part) {
    __shared__ shared_t sh;
    const int b = blockIdx.x, lane = threadIdx.x;
    const float* xrow = x + (int64_t)b * N;
    const float* grow = gy + (int64_t)b * N;
    const int64_t ntask = (int64_t)nchunk * nlt;
    for (int64_t task = blockIdx.y; task < ntask; task += gridDim.y) {
        const int c = (int)(task / nlt);
        const int64_t j0 = (task % nlt) * TILE, s0 = (int64_t)c * GH_CHUNK;
        if (s0 + j0 >= N) continue;  // empty: s + j >= N for every pair of them (a function of N alone)
        const int64_t s_hi = s0 + GH_CHUNK < N - j0 ? s0 + GH_CHUNK : N - j0;
        double acc[R];
#pragma unroll
        for (int i = 0; i < R; ++i) acc[i] = 0.0;
        correlate(
            sh, lane, j0, s0, s_hi, [&](int64_t q) { return (double)xrow[q]; },
            [&](int64_t e) { return e < N ? (double)grow[e] : 0.0; }, acc);
        double* prow = part + ((int64_t)b * nchunk + c) * Lc;
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const int64_t j = j0 + lane * R + i;
            if (j < Lc) prow[j] = acc[i];
        }
    }
}

// gh[r,j]: per row the chunks in ascending order, then the rows in ascending order; 0 for j >= N
__global__ void __launch_bounds__(256)
    fir_gh_join_kernel(const double* __restrict__ part, int B, int H, int N, int L, int Lc, int nchunk, double* __restrict__ gh) {
    const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= (int64_t)H * L) return;
    const int r = (int)(id / L);
    const int64_t j = id % L;
    double total = 0.0;
    if (j < N) {
        const int nc = (int)((N - j + GH_CHUNK - 1) / GH_CHUNK);  // the chunks with an s below N - j
        for (int b = r; b < B; b += H) {
            double s = 0.0;
            for (int c = 0; c < nc; ++c) s += part[((int64_t)b * nchunk + c) * Lc + j];
            total += s;
        }
    }
    gh[id] = total;
}

using ds::aligned;

int check_args(const char* fn, bool pointers, int B, int H, int N, int L) {
    DS_REQUIRE(pointers, "%s: null pointer", fn);
    DS_REQUIRE(B > 0 && H > 0 && N > 0 && L > 0, "%s: empty problem (B %d, H %d, N %d, L %d)", fn, B, H, N, L);
    DS_REQUIRE(B <= DS_FIR_MAX_ROWS, "%s: B = %d above %d", fn, B, DS_FIR_MAX_ROWS);
    DS_REQUIRE(L <= DS_FIR_MAX_TAPS, "%s: L = %d taps above %d", fn, L, DS_FIR_MAX_TAPS);
    DS_REQUIRE(H <= B && B % H == 0, "%s: B = %d is not a multiple of H = %d", fn, B, H);
    return DS_OK;
}

inline int nchunks(int N) { return (int)(((int64_t)N + GH_CHUNK - 1) / GH_CHUNK); }

template <bool REV>
int launch_conv(const float* in, const double* h, int B, int H, int N, int L, float* out, hipStream_t st) {
    const int64_t ntiles = ((int64_t)N + TILE - 1) / TILE;
    fir_conv_kernel<REV><<<dim3((unsigned)B, (unsigned)(ntiles < 65535 ? ntiles : 65535)), 64, 0, st>>>(in, h, H, N, L, out);
    return DS_LAUNCHED("fir_conv_kernel");
}

}  // namespace

extern "C" int64_t ds_fir_workspace_bytes(int B, int H, int N, int L) {
    if (B <= 0 || H <= 0 || N <= 0 || L <= 0 || B > DS_FIR_MAX_ROWS || L > DS_FIR_MAX_TAPS || H > B || B % H) return 0;
    return (int64_t)sizeof(double) * B * nchunks(N) * (L < N ? L : N);
}

extern "C" int ds_fir_fwd(const float* x, const double* h, int B, int H, int N, int L, float* y, ds_stream_t stream) {
    if (int rc = check_args("ds_fir_fwd", x && h && y, B, H, N, L)) return rc;
    DS_REQUIRE(aligned(x, 4) && aligned(h, 8) && aligned(y, 4), "ds_fir_fwd: misaligned operand");
    return launch_conv<true>(x, h, B, H, N, L, y, ds::as_stream(stream));
}

extern "C" int ds_fir_bwd(const float* gy, const float* x, const double* h, int B, int H, int N, int L, void* work,
                          int64_t work_bytes, float* gx, double* gh, ds_stream_t stream) {
    if (int rc = check_args("ds_fir_bwd", gy && x && h && (work || !gh), B, H, N, L)) return rc;
    DS_REQUIRE(aligned(gy, 4) && aligned(x, 4) && aligned(h, 8) && aligned(gx, 4) && aligned(gh, 8),
               "ds_fir_bwd: misaligned operand");
    DS_REQUIRE(gx || gh, "ds_fir_bwd: gx and gh are both NULL");
    hipStream_t st = ds::as_stream(stream);
    if (gh) {
        DS_REQUIRE(aligned(work, 16), "ds_fir_bwd: work not 16-byte aligned");
        DS_REQUIRE(work_bytes >= ds_fir_workspace_bytes(B, H, N, L), "ds_fir_bwd: workspace of %lld bytes, %lld needed",
                   (long long)work_bytes, (long long)ds_fir_workspace_bytes(B, H, N, L));
    }
    if (gx)
        if (int rc = launch_conv<false>(gy, h, B, H, N, L, gx, st)) return rc;
    if (gh) {
        double* part = static_cast<double*>(work);
        const int Lc = L < N ? L : N, nchunk = nchunks(N), nlt = (Lc + TILE - 1) / TILE;
        const int64_t ntask = (int64_t)nchunk * nlt;
        fir_gh_kernel<<<dim3((unsigned)B, (unsigned)(ntask < 65535 ? ntask : 65535)), 64, 0, st>>>(gy, x, N, Lc, nchunk, nlt, part);
        DS_LAUNCH_CHECK("fir_gh_kernel");
        const int64_t nout = (int64_t)H * L;
        fir_gh_join_kernel<<<dim3((unsigned)((nout + 255) / 256)), 256, 0, st>>>(part, B, H, N, L, Lc, nchunk, gh);
        DS_LAUNCH_CHECK("fir_gh_join_kernel");
    }
    return DS_OK;
}
