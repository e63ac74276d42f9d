// Debiased Sinkhorn divergence between point clouds - gfx950.  Replaces geomloss.SamplesLoss("sinkhorn", p=2,
// blur, scaling=0.5, debias=True) (geomloss==0.2.6, tensorized backend), which the reference's spectral loss calls
// (src/ddsp/mss_loss.py:104-117).  DESIGN.md section 12 has the scheme.
//
// Cost C(x, y) = |x - y|^2 / 2, computed on the fly from the coordinates (direct (x - y)^2 form): no N x M matrix.
// softmin_eps(C, h)_i = -eps * LSE_j(h_j - C_ij / eps), the LSE by max shift in two passes over j (the max, then the
// sum of exp), as torch.logsumexp does.
//
//   ds_sinkhorn_bbox      per coordinate, the min and max over every point of x and y of every batch, the least
//                         weights and a count of non-finite values: the one record the host reads.
//   ds_sinkhorn_loop      log weights, the initialisation at eps_list[0], then one launch per eps with the four
//                         softmins and the averaging fused.  Ping-pong over two potential slots, arranged so that the
//                         loop ends in slot A.
//   ds_sinkhorn_final     the last extrapolation (slot A -> slot B, no averaging) with each row's LSE kept for the
//                         backward, then the per-batch loss in fp64.
//   ds_sinkhorn_backward  dS/dx, dS/dy from the kept LSEs: P_ij = exp(h_j - C_ij / eps - lse_i).
//
// One wavefront owns ROWS rows of one potential of one batch; its 64 lanes walk the columns j = lane, lane + 64, ...
// and combine their partial max / sum / gradient with an xor butterfly (commutative operations: every lane ends
// with the same bits).  A row's arithmetic therefore depends on nothing but its own row, column cloud and column
// potentials: not on B, not on the batch index, not on the rows it shares a wavefront with.  The four potentials of
// one row i of identical clouds are the same operations on the same values, so their differences are exactly 0.
// No atomics, no LDS, no barriers.
#include <cmath>

#include "ds_common.h"

#pragma clang fp contract(off)  // every fused multiply-add below is written out

namespace {

constexpr int WAVE = 64;
constexpr int WAVES = 4;  // wavefronts per workgroup
constexpr int MAX_D = 32;

template <int DM>
constexpr int rows_for() {
    return DM <= 8 ? 4 : 1;  // rows per wavefront: x_i and the gradient accumulators stay in registers
}

// Potential slot layout inside one buffer of PT = B (2N + 2M) floats: k = 0 f_ba (B x N), 1 g_ab (B x M),
// 2 f_aa (B x N), 3 g_bb (B x M).
struct Geo {
    int64_t B, N, M;
    int D;
    __device__ __forceinline__ int64_t slot(int k) const {
        return k == 0 ? 0 : k == 1 ? B * N : k == 2 ? B * (N + M) : B * (2 * N + M);
    }
};

// What potential k of batch b reads: rows from `rx` (n_r points), columns from `cx` (n_c points) with log weights
// `lw` and column potentials `cp` (the other side's potential for k = 0, 1; its own for k = 2, 3).
struct Role {
    const float* rx;
    const float* cx;
    const float* lw;
    int64_t n_r, n_c;
    int64_t self_off;  // offset of this row block's potentials in a slot buffer
    int64_t col_off;   // offset of the column potentials
};

__device__ __forceinline__ Role role(const Geo& g, int k, int64_t b, const float* x, const float* y, const float* loga,
                                     const float* logb) {
    const int64_t N = g.N, M = g.M, D = g.D;
    const float* xb = x + b * N * D;
    const float* yb = y + b * M * D;
    Role r;
    switch (k) {
        case 0: r = {xb, yb, logb + b * M, N, M, g.slot(0) + b * N, g.slot(1) + b * M}; break;
        case 1: r = {yb, xb, loga + b * N, M, N, g.slot(1) + b * M, g.slot(0) + b * N}; break;
        case 2: r = {xb, xb, loga + b * N, N, N, g.slot(2) + b * N, g.slot(2) + b * N}; break;
        default: r = {yb, yb, logb + b * M, M, M, g.slot(3) + b * M, g.slot(3) + b * M}; break;
    }
    return r;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) v = fmaxf(v, __shfl_xor(v, o, WAVE));
    return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) v += __shfl_xor(v, o, WAVE);
    return v;
}

template <int DM>
__device__ __forceinline__ void load_point(const float* p, int D, float (&v)[DM]) {
#pragma unroll
    for (int k = 0; k < DM; ++k) v[k] = k < D ? p[k] : 0.f;  // padding coordinates add exactly 0 to |x - y|^2
}

template <int DM>
__device__ __forceinline__ float half_d2(const float (&a)[DM], const float (&c)[DM]) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < DM; ++k) {
        const float t = a[k] - c[k];
        s = fmaf(t, t, s);
    }
    return 0.5f * s;
}

// Wave -> (batch, potential, row block), potentials in the order k = 0 .. nk-1 inside a batch.
struct Task {
    int64_t b, row0;
    int k;
};
__device__ __forceinline__ bool decode(int64_t w, const Geo& g, int nk, int rows, Task& t) {
    const int64_t gN = (g.N + rows - 1) / rows, gM = (g.M + rows - 1) / rows;
    const int64_t per = nk == 4 ? 2 * (gN + gM) : gN + gM;
    if (w >= g.B * per) return false;
    t.b = w / per;
    int64_t r = w - t.b * per;
    int k = 0;
    if (r >= gN) {
        r -= gN;
        k = 1;
        if (r >= gM) {
            r -= gM;
            k = 2;
            if (r >= gN) {
                r -= gN;
                k = 3;
            }
        }
    }
    t.k = k;
    t.row0 = r * rows;
    return true;
}

// mode 0: initialisation (h = log w), out = softmin.  mode 1: out = (old + softmin) / 2 with h = log w + old / eps.
// mode 2: the last extrapolation, out = softmin with h = log w + old / eps, and each row's LSE to `lse`.
template <int DM>
__global__ __launch_bounds__(WAVE* WAVES) void sinkhorn_step_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                                    const float* __restrict__ loga,
                                                                    const float* __restrict__ logb, Geo g, int nk,
                                                                    int mode, float eps, float inv_eps,
                                                                    const float* __restrict__ pin,
                                                                    float* __restrict__ pout, float* __restrict__ lse) {
    constexpr int R = rows_for<DM>();
    const int lane = threadIdx.x % WAVE;
    const int64_t w = (int64_t)blockIdx.x * WAVES + threadIdx.x / WAVE;
    Task t;
    if (!decode(w, g, nk, R, t)) return;  // whole wavefronts leave together
    const Role ro = role(g, t.k, t.b, x, y, loga, logb);
    const int D = g.D;
    float xi[R][DM];
#pragma unroll
    for (int q = 0; q < R; ++q) load_point<DM>(ro.rx + min(t.row0 + q, ro.n_r - 1) * D, D, xi[q]);
    const float* cp = mode == 0 ? nullptr : pin + ro.col_off;
    float m[R];
#pragma unroll
    for (int q = 0; q < R; ++q) m[q] = -INFINITY;
    for (int64_t j = lane; j < ro.n_c; j += WAVE) {
        float yj[DM];
        load_point<DM>(ro.cx + j * D, D, yj);
        const float h = mode == 0 ? ro.lw[j] : ro.lw[j] + cp[j] / eps;
#pragma unroll
        for (int q = 0; q < R; ++q) m[q] = fmaxf(m[q], h - half_d2<DM>(xi[q], yj) * inv_eps);
    }
    float s[R];
#pragma unroll
    for (int q = 0; q < R; ++q) {
        m[q] = wave_max(m[q]);
        s[q] = 0.f;
    }
    for (int64_t j = lane; j < ro.n_c; j += WAVE) {
        float yj[DM];
        load_point<DM>(ro.cx + j * D, D, yj);
        const float h = mode == 0 ? ro.lw[j] : ro.lw[j] + cp[j] / eps;
#pragma unroll
        for (int q = 0; q < R; ++q) s[q] += expf((h - half_d2<DM>(xi[q], yj) * inv_eps) - m[q]);
    }
#pragma unroll
    for (int q = 0; q < R; ++q) {
        const float tot = wave_sum(s[q]);
        const int64_t i = t.row0 + q;
        if (lane == q && i < ro.n_r) {
            const float l = logf(tot) + m[q];
            const float ft = -eps * l;
            const int64_t o = ro.self_off + i;
            pout[o] = mode == 1 ? 0.5f * (pin[o] + ft) : ft;
            if (mode == 2) lse[o] = l;
        }
    }
}

// dS/dx_i = g_b a_i (sum_j P_ij (x_i - y_j) - sum_k Q_ik (x_i - x_k)), and the mirror image for y.  k = 0: the x rows
// (P from the f_ba softmin, Q from f_aa), k = 1: the y rows (g_ab, g_bb).
template <int DM>
__global__ __launch_bounds__(WAVE* WAVES) void sinkhorn_backward_kernel(
    const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ a, const float* __restrict__ bw,
    const float* __restrict__ loga, const float* __restrict__ logb, Geo g, int debias, float eps, float inv_eps,
    const float* __restrict__ pin, const float* __restrict__ lse, const float* __restrict__ gloss, int want_x,
    int want_y, float* __restrict__ gx, float* __restrict__ gy) {
    constexpr int R = rows_for<DM>();
    const int lane = threadIdx.x % WAVE;
    const int64_t w = (int64_t)blockIdx.x * WAVES + threadIdx.x / WAVE;
    Task t;
    if (!decode(w, g, 2, R, t)) return;
    if ((t.k == 0 && !want_x) || (t.k == 1 && !want_y)) return;
    const int D = g.D;
    float res[DM];  // lane q keeps row q's first-pass sum
#pragma unroll
    for (int k = 0; k < DM; ++k) res[k] = 0.f;
    const int npass = debias ? 2 : 1;
    for (int pass = 0; pass < npass; ++pass) {
        const int kk = t.k + 2 * pass;  // 0 / 1: the cross potential, 2 / 3: the symmetric one
        const Role ro = role(g, kk, t.b, x, y, loga, logb);
        float xi[R][DM], acc[R][DM], li[R];
#pragma unroll
        for (int q = 0; q < R; ++q) {
            const int64_t i = min(t.row0 + q, ro.n_r - 1);
            load_point<DM>(ro.rx + i * D, D, xi[q]);
            li[q] = lse[ro.self_off + i];
#pragma unroll
            for (int k = 0; k < DM; ++k) acc[q][k] = 0.f;
        }
        const float* cp = pin + ro.col_off;
        for (int64_t j = lane; j < ro.n_c; j += WAVE) {
            float yj[DM];
            load_point<DM>(ro.cx + j * D, D, yj);
            const float h = ro.lw[j] + cp[j] / eps;
#pragma unroll
            for (int q = 0; q < R; ++q) {
                const float p = expf((h - half_d2<DM>(xi[q], yj) * inv_eps) - li[q]);
#pragma unroll
                for (int k = 0; k < DM; ++k) acc[q][k] = fmaf(p, xi[q][k] - yj[k], acc[q][k]);
            }
        }
#pragma unroll
        for (int q = 0; q < R; ++q)
#pragma unroll
            for (int k = 0; k < DM; ++k) {
                const float v = wave_sum(acc[q][k]);
                if (lane == q) res[k] = pass == 0 ? v : res[k] - v;
            }
    }
    const int64_t n = t.k == 0 ? g.N : g.M;
    const int64_t i = t.row0 + lane;
    if (lane < R && i < n) {
        const float* wt = t.k == 0 ? a : bw;
        float* out = t.k == 0 ? gx : gy;
        const int64_t r = t.b * n + i;
        const float c = gloss[t.b] * wt[r];
        for (int k = 0; k < D; ++k) out[r * D + k] = c * res[k];
    }
}

__global__ __launch_bounds__(256) void log_weights_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                          int64_t na, int64_t nb, float* __restrict__ loga,
                                                          float* __restrict__ logb) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < na) loga[i] = logf(a[i]);
    else if (i < na + nb) logb[i - na] = logf(b[i - na]);
}

// Workgroup k < D: min / max of coordinate k over x and y, and its non-finite count; workgroup D: the least weights
// and their non-finite count.  out = [min (D) | max (D) | min a | min b | bad (D + 1)].
__global__ __launch_bounds__(256) void bbox_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                   const float* __restrict__ a, const float* __restrict__ b, int64_t nx,
                                                   int64_t ny, int D, float* __restrict__ out) {
    __shared__ float s0[256], s1[256], s2[256];
    const int k = blockIdx.x, tid = threadIdx.x;
    float lo = INFINITY, hi = -INFINITY, bad = 0.f;
    if (k < D) {
        for (int64_t i = tid; i < nx + ny; i += 256) {
            const float v = i < nx ? x[i * D + k] : y[(i - nx) * D + k];
            if (!isfinite(v)) bad += 1.f;
            lo = fminf(lo, v);
            hi = fmaxf(hi, v);
        }
    } else {  // lo = least a, hi = least b
        hi = INFINITY;
        for (int64_t i = tid; i < nx + ny; i += 256) {
            const float v = i < nx ? a[i] : b[i - nx];
            if (!isfinite(v)) bad += 1.f;
            if (i < nx) lo = fminf(lo, v);
            else hi = fminf(hi, v);
        }
    }
    s0[tid] = lo;
    s1[tid] = hi;
    s2[tid] = bad;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) {
            s0[tid] = fminf(s0[tid], s0[tid + o]);
            s1[tid] = k < D ? fmaxf(s1[tid], s1[tid + o]) : fminf(s1[tid], s1[tid + o]);
            s2[tid] += s2[tid + o];
        }
        __syncthreads();
    }
    if (tid == 0) {
        if (k < D) {
            out[k] = s0[0];
            out[D + k] = s1[0];
        } else {
            out[2 * D] = s0[0];
            out[2 * D + 1] = s1[0];
        }
        out[2 * D + 2 + k] = s2[0];
    }
}

// Per batch: S = <a, f_ba - f_aa> + <b, g_ab - g_bb> (debias) or <a, f_ba> + <b, g_ab>, in fp64, fixed order.
__global__ __launch_bounds__(256) void loss_kernel(const float* __restrict__ a, const float* __restrict__ bw, Geo g,
                                                   int debias, const float* __restrict__ pot, double* __restrict__ loss) {
    __shared__ double sh[256];
    const int64_t b = blockIdx.x;
    const int tid = threadIdx.x;
    const int64_t N = g.N, M = g.M;
    const float* f_ba = pot + g.slot(0) + b * N;
    const float* g_ab = pot + g.slot(1) + b * M;
    const float* f_aa = pot + g.slot(2) + b * N;
    const float* g_bb = pot + g.slot(3) + b * M;
    double s = 0.0;
    for (int64_t i = tid; i < N; i += 256) {
        const double f = debias ? (double)f_ba[i] - (double)f_aa[i] : (double)f_ba[i];
        s += (double)a[b * N + i] * f;
    }
    for (int64_t j = tid; j < M; j += 256) {
        const double f = debias ? (double)g_ab[j] - (double)g_bb[j] : (double)g_ab[j];
        s += (double)bw[b * M + j] * f;
    }
    sh[tid] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) sh[tid] += sh[tid + o];
        __syncthreads();
    }
    if (tid == 0) loss[b] = sh[0];
}

constexpr int64_t MAX_POINTS = (int64_t)1 << 30;

int check_sizes(const char* what, const float* x, const float* y, const float* a, const float* b, int64_t B, int64_t N,
                int64_t M, int64_t D) {
    DS_REQUIRE(x && y && a && b, "%s: null pointer", what);
    DS_REQUIRE(B >= 1 && N >= 1 && M >= 1 && D >= 1 && D <= MAX_D && B * (N + M) <= MAX_POINTS,
               "%s: bad sizes B=%lld N=%lld M=%lld D=%lld (1 <= D <= %d)", what, (long long)B, (long long)N, (long long)M,
               (long long)D, MAX_D);
    return DS_OK;
}

int64_t waves_for(const Geo& g, int nk, int rows) {
    const int64_t gN = ds::ceil_div(g.N, rows), gM = ds::ceil_div(g.M, rows);
    return g.B * (nk == 4 ? 2 * (gN + gM) : gN + gM);
}

template <int DM>
void launch_step(const float* x, const float* y, const float* loga, const float* logb, const Geo& g, int nk, int mode,
                 float eps, const float* pin, float* pout, float* lse, hipStream_t st) {
    const int64_t waves = waves_for(g, nk, rows_for<DM>());
    sinkhorn_step_kernel<DM><<<dim3((unsigned)ds::ceil_div(waves, WAVES)), dim3(WAVE * WAVES), 0, st>>>(
        x, y, loga, logb, g, nk, mode, eps, (float)(1.0 / (double)eps), pin, pout, lse);
}

void step(const float* x, const float* y, const float* loga, const float* logb, const Geo& g, int nk, int mode,
          float eps, const float* pin, float* pout, float* lse, hipStream_t st) {
    if (g.D <= 4) launch_step<4>(x, y, loga, logb, g, nk, mode, eps, pin, pout, lse, st);
    else if (g.D <= 8) launch_step<8>(x, y, loga, logb, g, nk, mode, eps, pin, pout, lse, st);
    else if (g.D <= 16) launch_step<16>(x, y, loga, logb, g, nk, mode, eps, pin, pout, lse, st);
    else launch_step<32>(x, y, loga, logb, g, nk, mode, eps, pin, pout, lse, st);
}

template <int DM>
void launch_backward(const float* x, const float* y, const float* a, const float* b, const float* loga,
                     const float* logb, const Geo& g, int debias, float eps, const float* pin, const float* lse,
                     const float* gloss, float* gx, float* gy, hipStream_t st) {
    const int64_t waves = waves_for(g, 2, rows_for<DM>());
    sinkhorn_backward_kernel<DM><<<dim3((unsigned)ds::ceil_div(waves, WAVES)), dim3(WAVE * WAVES), 0, st>>>(
        x, y, a, b, loga, logb, g, debias, eps, (float)(1.0 / (double)eps), pin, lse, gloss, gx != nullptr,
        gy != nullptr, gx, gy);
}

// Workspace (floats): log a (B N) | log b (B M) | slot A (PT) | slot B (PT) | lse (PT), PT = B (2N + 2M).
struct Work {
    float *loga, *logb, *potA, *potB, *lse;
};
Work carve(float* w, const Geo& g) {
    const int64_t PT = g.B * (2 * g.N + 2 * g.M);
    Work r;
    r.loga = w;
    r.logb = r.loga + g.B * g.N;
    r.potA = r.logb + g.B * g.M;
    r.potB = r.potA + PT;
    r.lse = r.potB + PT;
    return r;
}

bool good_eps(float e) { return std::isfinite(e) && e > 0.f; }

}  // namespace

extern "C" int64_t ds_sinkhorn_workspace_floats(int64_t B, int64_t N, int64_t M) {
    if (B < 1 || N < 1 || M < 1 || B * (N + M) > MAX_POINTS) return -1;
    return B * (N + M) + 3 * B * (2 * N + 2 * M);
}

extern "C" int ds_sinkhorn_bbox(const float* x, const float* y, const float* a, const float* b, int64_t B, int64_t N,
                                int64_t M, int64_t D, float* out, ds_stream_t stream) {
    int rc = check_sizes("ds_sinkhorn_bbox", x, y, a, b, B, N, M, D);
    if (rc != DS_OK) return rc;
    DS_REQUIRE(out, "ds_sinkhorn_bbox: null pointer");
    bbox_kernel<<<dim3((unsigned)D + 1), dim3(256), 0, ds::as_stream(stream)>>>(x, y, a, b, B * N, B * M, (int)D, out);
    DS_LAUNCH_CHECK("ds_sinkhorn_bbox");
    return DS_OK;
}

extern "C" int ds_sinkhorn_loop(const float* x, const float* y, const float* a, const float* b, int64_t B, int64_t N,
                                int64_t M, int64_t D, const float* eps_list, int n_eps, int debias, float* work,
                                ds_stream_t stream) {
    int rc = check_sizes("ds_sinkhorn_loop", x, y, a, b, B, N, M, D);
    if (rc != DS_OK) return rc;
    DS_REQUIRE(eps_list && work, "ds_sinkhorn_loop: null pointer");
    DS_REQUIRE(n_eps >= 1, "ds_sinkhorn_loop: empty schedule");
    for (int e = 0; e < n_eps; ++e)
        DS_REQUIRE(good_eps(eps_list[e]), "ds_sinkhorn_loop: eps_list[%d] = %g is not a positive finite number", e,
                   (double)eps_list[e]);
    DS_REQUIRE((reinterpret_cast<uintptr_t>(work) & 3) == 0, "ds_sinkhorn_loop: workspace not 4-byte aligned");
    const Geo g = {B, N, M, (int)D};
    const int nk = debias ? 4 : 2;
    const Work w = carve(work, g);
    hipStream_t st = ds::as_stream(stream);
    log_weights_kernel<<<dim3((unsigned)ds::ceil_div(B * (N + M), 256)), dim3(256), 0, st>>>(a, b, B * N, B * M, w.loga,
                                                                                           w.logb);
    DS_LAUNCH_CHECK("ds_sinkhorn_loop (log weights)");
    // 1 + n_eps writes that end in slot A
    float* cur = (n_eps % 2 == 0) ? w.potA : w.potB;
    float* nxt = cur == w.potA ? w.potB : w.potA;
    step(x, y, w.loga, w.logb, g, nk, 0, eps_list[0], nullptr, cur, nullptr, st);
    DS_LAUNCH_CHECK("ds_sinkhorn_loop (init)");
    for (int e = 0; e < n_eps; ++e) {
        step(x, y, w.loga, w.logb, g, nk, 1, eps_list[e], cur, nxt, nullptr, st);
        DS_LAUNCH_CHECK("ds_sinkhorn_loop (step)");
        float* t = cur;
        cur = nxt;
        nxt = t;
    }
    return DS_OK;
}

extern "C" int ds_sinkhorn_final(const float* x, const float* y, const float* a, const float* b, int64_t B, int64_t N,
                                 int64_t M, int64_t D, float eps, int debias, float* work, double* loss,
                                 ds_stream_t stream) {
    int rc = check_sizes("ds_sinkhorn_final", x, y, a, b, B, N, M, D);
    if (rc != DS_OK) return rc;
    DS_REQUIRE(work && loss, "ds_sinkhorn_final: null pointer");
    DS_REQUIRE(good_eps(eps), "ds_sinkhorn_final: eps = %g is not a positive finite number", (double)eps);
    const Geo g = {B, N, M, (int)D};
    const Work w = carve(work, g);
    hipStream_t st = ds::as_stream(stream);
    step(x, y, w.loga, w.logb, g, debias ? 4 : 2, 2, eps, w.potA, w.potB, w.lse, st);
    DS_LAUNCH_CHECK("ds_sinkhorn_final (extrapolation)");
    loss_kernel<<<dim3((unsigned)B), dim3(256), 0, st>>>(a, b, g, debias, w.potB, loss);
    DS_LAUNCH_CHECK("ds_sinkhorn_final (loss)");
    return DS_OK;
}

extern "C" int ds_sinkhorn_backward(const float* x, const float* y, const float* a, const float* b, int64_t B,
                                    int64_t N, int64_t M, int64_t D, float eps, int debias, const float* work,
                                    const float* grad_loss, float* grad_x, float* grad_y, ds_stream_t stream) {
    int rc = check_sizes("ds_sinkhorn_backward", x, y, a, b, B, N, M, D);
    if (rc != DS_OK) return rc;
    DS_REQUIRE(work && grad_loss, "ds_sinkhorn_backward: null pointer");
    DS_REQUIRE(good_eps(eps), "ds_sinkhorn_backward: eps = %g is not a positive finite number", (double)eps);
    if (!grad_x && !grad_y) return DS_OK;
    const Geo g = {B, N, M, (int)D};
    const Work w = carve(const_cast<float*>(work), g);
    hipStream_t st = ds::as_stream(stream);
    if (D <= 4) launch_backward<4>(x, y, a, b, w.loga, w.logb, g, debias, eps, w.potA, w.lse, grad_loss, grad_x, grad_y, st);
    else if (D <= 8) launch_backward<8>(x, y, a, b, w.loga, w.logb, g, debias, eps, w.potA, w.lse, grad_loss, grad_x, grad_y, st);
    else if (D <= 16) launch_backward<16>(x, y, a, b, w.loga, w.logb, g, debias, eps, w.potA, w.lse, grad_loss, grad_x, grad_y, st);
    else launch_backward<32>(x, y, a, b, w.loga, w.logb, g, debias, eps, w.potA, w.lse, grad_loss, grad_x, grad_y, st);
    DS_LAUNCH_CHECK("ds_sinkhorn_backward");
    return DS_OK;
}
