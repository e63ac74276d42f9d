// Driven oscillator bank: the damped-oscillator bank under a force signal of ANY length, with a force gradient - gfx950.
//
// Reference: the grouped conv1d(signal, forces) of src/ddsp/oscillator.py:113-141, 282-310, whose autograd reaches the
// force tensor, fed with a recorded force (utils.load_audio returns the Force channel of every clip).  oscillator.hip
// runs that convolution as a causal FIR out of LDS (at most 512 taps, no force gradient).  Here each mode is the
// recursive resonator it is,
//     x[t] = z (x[t-1] + f[t]),  z = exp((-d + i w) / sr),  x[-1] = 0,  f[t] = 0 for t >= F,   y[t] = sum_m amp Im x_m[t],
// which equals the closed form  y[t] = sum_{j <= t} f[j] sum_m amp Im z_m^(t-j+1)  at a cost independent of F.  The
// adjoint runs the same recurrence down in time, l[t] = z (l[t+1] + gy[t]), l[S] = 0:
//     gforce[j] = sum_m amp Im l_m[j],   gamp = sum_t gy[t] Im x[t],
//     G = amp sum_t (x[t-1] + f[t]) l[t]  (complex, no conjugate; x[t-1] + f[t] = x[t] / z),  gd = -Im G / sr,  gw = Re G / sr.
//
// The scan over time: a wavefront lane owns RUN consecutive samples, a tile is the 64 RUN samples of one wavefront.
//   1. boundary pass  one wavefront per (clip, mode) walks the tiles in order: every lane runs its samples from a zero
//                     state, a 6-step shuffle scan with the closed-form powers z^(RUN 2^k) joins the lanes, and the state
//                     entering every tile goes to the workspace (A m ceil(S / TILE) complex doubles).
//   2. tile pass      workgroup = (clip, tile), 4 waves, each looping over its modes: the same lane scan plus the tile's
//                     entering state gives each lane its entering state; the lane then runs its samples again, for real,
//                     and adds amp Im x to an fp64 register per sample.  The waves merge through LDS in a fixed order;
//                     one fp32 rounding per output sample.
//   3. mode pass      (backward) one wavefront per (clip, mode) walks the tiles upwards carrying x, takes l's entering
//                     states from the downward boundary pass, and reduces gamp and G; a last kernel adds G over clips.
// Every power z^n of a jump over n samples is exp / sincos of n d / sr and n w / sr, never a product of rounded powers; a
// mode whose z^TILE underflows to 0 carries nothing across tiles and nothing else happens.  fp64 states, no atomics,
// nothing of size (A, m, S) in memory.
#include <algorithm>
#include <cstdint>

#include "ds_common.h"
#include "osc_scan.h"

namespace {

// the lane-scan helpers (cplx, cmul, zpow, from_prev, load_run, run_from_zero, scan_lanes, lane_entry, tile_exit): osc_scan.h
using namespace osc_scan;

constexpr int RUN = 16;          // samples per lane
constexpr int TILE = 64 * RUN;   // samples per wavefront pass (tests/_osc_driven_ref.py mirrors both)
static_assert(RUN == osc_scan::RUN && TILE == osc_scan::TILE, "osc_scan.h scans RUN samples per lane");

// 1. one wavefront per (clip, mode): bnd[(a m + mm) ntiles + k] = the state entering tile k.  in: (A x ldin), zero from nin on.
template <bool REV>
__global__ void __launch_bounds__(64)
    osc_drv_boundary_kernel(const double* __restrict__ dd, const double* __restrict__ ww, const float* __restrict__ in,
                            int ldin, int nin, int m, int ntiles, double inv_sr, double2* __restrict__ bnd) {
    const int mm = blockIdx.x, a = blockIdx.y, lane = threadIdx.x;
    const int q = REV ? 63 - lane : lane;
    const double d = dd[mm], w = ww[mm];
    const cplx z1 = zpow(d, w, inv_sr, 1), zq = zpow(d, w, inv_sr, RUN * q), zT = zpow(d, w, inv_sr, TILE);
    const float* row = in + (int64_t)a * ldin;
    double2* b = bnd + ((int64_t)a * m + mm) * ntiles;
    cplx carry = {0.0, 0.0};
    for (int kk = 0; kk < ntiles; ++kk) {
        const int k = REV ? ntiles - 1 - kk : kk;
        if (lane == 0) b[k] = make_double2(carry.r, carry.i);
        if (kk == ntiles - 1) break;
        const int t0 = k * TILE;
        if (t0 >= nin) {  // (wave-uniform) nothing drives this tile
            carry = cmul(zT, carry);
            continue;
        }
        double v[RUN];
        load_run(row, t0, lane, nin, v);
        const cplx s = scan_lanes<REV>(run_from_zero<REV>(v, z1), zq, lane);
        carry = tile_exit<REV>(s, carry, zT);
    }
}

// 2. workgroup = (tile, clip): out[a, t] = sum_m amp Im state_m[t] for t < nout.  out: (A x ldout).
template <bool REV>
__global__ void __launch_bounds__(256)
    osc_drv_tile_kernel(const double* __restrict__ dd, const double* __restrict__ ww, const float* __restrict__ amp,
                        const float* __restrict__ in, int ldin, int nin, int m, int ntiles, double inv_sr,
                        const double2* __restrict__ bnd, float* __restrict__ out, int ldout, int nout) {
    __shared__ double s_part[4][64 * (RUN + 1)];  // (a lane's RUN sums padded to RUN + 1: no bank conflicts)
    const int k = blockIdx.x, a = blockIdx.y;
    const int t0 = k * TILE;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q = REV ? 63 - lane : lane;
    const bool driven = t0 < nin;
    double v[RUN], acc[RUN];
    load_run(in + (int64_t)a * ldin, t0, lane, nin, v);
#pragma unroll
    for (int i = 0; i < RUN; ++i) acc[i] = 0.0;
    for (int mm = wave; mm < m; mm += 4) {
        const double d = dd[mm], w = ww[mm];
        const double am = amp ? (double)amp[(int64_t)a * m + mm] : 1.0;
        const cplx z1 = zpow(d, w, inv_sr, 1), zq = zpow(d, w, inv_sr, RUN * q);
        const double2 c = bnd[((int64_t)a * m + mm) * ntiles + k];
        cplx e = {0.0, 0.0};
        if (driven) e = run_from_zero<REV>(v, z1);
        cplx x = lane_entry<REV>(scan_lanes<REV>(e, zq, lane), cplx{c.x, c.y}, zq, lane);
#pragma unroll
        for (int ii = 0; ii < RUN; ++ii) {
            const int i = REV ? RUN - 1 - ii : ii;
            x = cmul(z1, cplx{x.r + v[i], x.i});
            acc[i] += am * x.i;
        }
    }
#pragma unroll
    for (int i = 0; i < RUN; ++i) s_part[wave][lane * (RUN + 1) + i] = acc[i];
    __syncthreads();
    const int n = min(TILE, nout - t0);
    for (int j = threadIdx.x; j < n; j += blockDim.x) {
        const int o = (j / RUN) * (RUN + 1) + (j % RUN);
        out[(int64_t)a * ldout + t0 + j] = (float)((s_part[0][o] + s_part[1][o]) + (s_part[2][o] + s_part[3][o]));
    }
}

// 3. one wavefront per (clip, mode): gamp[a, mm] and gpart[a m + mm] = amp sum_t (x[t-1] + f[t]) l[t].  lbnd: the states
// of l entering every tile (from above), written by osc_drv_boundary_kernel<true> on gy.
__global__ void __launch_bounds__(64)
    osc_drv_mode_kernel(const float* __restrict__ gy, const double* __restrict__ dd, const double* __restrict__ ww,
                        const float* __restrict__ amp, const float* __restrict__ force, int F, int m, int S, int ntiles,
                        double inv_sr, const double2* __restrict__ lbnd, float* __restrict__ gamp,
                        double2* __restrict__ gpart) {
    const int mm = blockIdx.x, a = blockIdx.y, lane = threadIdx.x;
    const double d = dd[mm], w = ww[mm];
    const double am = amp ? (double)amp[(int64_t)a * m + mm] : 1.0;
    const cplx z1 = zpow(d, w, inv_sr, 1), zT = zpow(d, w, inv_sr, TILE);
    const cplx zq_up = zpow(d, w, inv_sr, RUN * lane), zq_dn = zpow(d, w, inv_sr, RUN * (63 - lane));
    const int nf = min(F, S);
    const float* frow = force + (int64_t)a * F;
    const float* grow = gy + (int64_t)a * S;
    const double2* lb = lbnd + ((int64_t)a * m + mm) * ntiles;
    cplx cx = {0.0, 0.0}, G = {0.0, 0.0};
    double ga = 0.0;
    for (int k = 0; k < ntiles; ++k) {
        const int t0 = k * TILE;
        double f[RUN], g[RUN];
        load_run(frow, t0, lane, nf, f);
        load_run(grow, t0, lane, S, g);
        cplx ef = {0.0, 0.0};
        if (t0 < nf) ef = run_from_zero<false>(f, z1);
        const cplx sf = scan_lanes<false>(ef, zq_up, lane);
        cplx x = lane_entry<false>(sf, cx, zq_up, lane);
        cx = tile_exit<false>(sf, cx, zT);
        const cplx sl = scan_lanes<true>(run_from_zero<true>(g, z1), zq_dn, lane);
        const double2 c = lb[k];
        cplx l = lane_entry<true>(sl, cplx{c.x, c.y}, zq_dn, lane);
        cplx u[RUN];
#pragma unroll
        for (int i = 0; i < RUN; ++i) {
            u[i] = cplx{x.r + f[i], x.i};
            x = cmul(z1, u[i]);
            ga += g[i] * x.i;
        }
#pragma unroll
        for (int i = RUN - 1; i >= 0; --i) {
            l = cmul(z1, cplx{l.r + g[i], l.i});
            const cplx t = cmul(u[i], l);
            G.r += t.r;
            G.i += t.i;
        }
    }
    ga = ds::wave_sum(ga);
    G.r = ds::wave_sum(G.r);
    G.i = ds::wave_sum(G.i);
    if (lane == 0) {
        if (gamp) gamp[(int64_t)a * m + mm] = (float)ga;
        gpart[(int64_t)a * m + mm] = make_double2(am * G.r, am * G.i);
    }
}

// gd[mm] = -Im sum_a G / sr, gw[mm] = Re sum_a G / sr, the clips added in order
__global__ void osc_drv_reduce_kernel(const double2* __restrict__ gpart, int A, int m, double inv_sr,
                                      double* __restrict__ gd, double* __restrict__ gw) {
    const int mm = blockIdx.x * blockDim.x + threadIdx.x;
    if (mm >= m) return;
    double gr = 0.0, gi = 0.0;
    for (int a = 0; a < A; ++a) {
        const double2 g = gpart[(int64_t)a * m + mm];
        gr += g.x;
        gi += g.y;
    }
    gd[mm] = -gi * inv_sr;
    gw[mm] = gr * inv_sr;
}

// gforce[a, j] = 0 for S <= j < F: taps that no output sample hears
__global__ void osc_drv_zero_tail_kernel(float* __restrict__ gforce, int F, int S) {
    const int j = S + blockIdx.x * blockDim.x + threadIdx.x;
    if (j < F) gforce[(int64_t)blockIdx.y * F + j] = 0.f;
}

inline int64_t ntiles_of(int S) { return ds::ceil_div(S, TILE); }

inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// The checks both entry points make before those of their own operands' alignment, in their order; `fn` names the entry point
int check_args(const char* fn, bool pointers, int A, int m, int F, int S, double sr, const void* work, int64_t work_bytes) {
    DS_REQUIRE(pointers, "%s: null pointer", fn);
    DS_REQUIRE(A > 0 && m > 0 && S > 0 && F > 0 && sr > 0, "%s: empty problem (A %d, m %d, F %d, S %d)", fn, A, m, F, S);
    DS_REQUIRE(A <= 65535, "%s: A = %d above 65535", fn, A);
    DS_REQUIRE(work_bytes >= ds_osc_driven_workspace_bytes(A, m, S), "%s: workspace of %lld bytes, %lld needed", fn,
               (long long)work_bytes, (long long)ds_osc_driven_workspace_bytes(A, m, S));
    DS_REQUIRE(aligned(work, 16), "%s: work not 16-byte aligned", fn);
    return DS_OK;
}

}  // namespace

extern "C" int64_t ds_osc_driven_workspace_bytes(int A, int m, int S) {
    if (A <= 0 || m <= 0 || S <= 0) return 0;
    return (int64_t)sizeof(double2) * ((int64_t)A * m * ntiles_of(S) + (int64_t)A * m);
}

extern "C" int ds_osc_driven_fwd(const double* d, const double* w, const float* amp, const float* force, int A, int m,
                                 int F, int S, double sr, void* work, int64_t work_bytes, float* y, ds_stream_t stream) {
    if (int rc = check_args("ds_osc_driven_fwd", d && w && force && work && y, A, m, F, S, sr, work, work_bytes)) return rc;
    DS_REQUIRE(aligned(d, 8) && aligned(w, 8) && aligned(force, 4) && aligned(y, 4) && aligned(amp, 4),
               "ds_osc_driven_fwd: misaligned operand");
    hipStream_t st = ds::as_stream(stream);
    const int nt = (int)ntiles_of(S);
    const int nin = std::min(F, S);
    double2* bnd = static_cast<double2*>(work);
    const double inv_sr = 1.0 / sr;
    osc_drv_boundary_kernel<false><<<dim3((unsigned)m, (unsigned)A), 64, 0, st>>>(d, w, force, F, nin, m, nt, inv_sr, bnd);
    DS_LAUNCH_CHECK("osc_drv_boundary_kernel");
    osc_drv_tile_kernel<false><<<dim3((unsigned)nt, (unsigned)A), 256, 0, st>>>(d, w, amp, force, F, nin, m, nt, inv_sr, bnd, y,
                                                                               S, S);
    DS_LAUNCH_CHECK("osc_drv_tile_kernel");
    return DS_OK;
}

extern "C" int ds_osc_driven_bwd(const float* gy, const double* d, const double* w, const float* amp, const float* force,
                                 int A, int m, int F, int S, double sr, void* work, int64_t work_bytes, double* gd, double* gw,
                                 float* gamp, float* gforce, ds_stream_t stream) {
    if (int rc = check_args("ds_osc_driven_bwd", gy && d && w && force && work && gd && gw, A, m, F, S, sr, work, work_bytes))
        return rc;
    DS_REQUIRE(aligned(gd, 8) && aligned(gw, 8), "ds_osc_driven_bwd: gd or gw not 8-byte aligned");
    DS_REQUIRE(aligned(d, 8) && aligned(w, 8) && aligned(force, 4) && aligned(gy, 4) && aligned(amp, 4) && aligned(gamp, 4) &&
                   aligned(gforce, 4),
               "ds_osc_driven_bwd: misaligned operand");
    hipStream_t st = ds::as_stream(stream);
    const int nt = (int)ntiles_of(S);
    double2* lbnd = static_cast<double2*>(work);
    double2* gpart = lbnd + (int64_t)A * m * nt;
    const double inv_sr = 1.0 / sr;
    osc_drv_boundary_kernel<true><<<dim3((unsigned)m, (unsigned)A), 64, 0, st>>>(d, w, gy, S, S, m, nt, inv_sr, lbnd);
    DS_LAUNCH_CHECK("osc_drv_boundary_kernel");
    if (gforce) {
        osc_drv_tile_kernel<true><<<dim3((unsigned)nt, (unsigned)A), 256, 0, st>>>(d, w, amp, gy, S, S, m, nt, inv_sr, lbnd,
                                                                                  gforce, F, std::min(F, S));
        DS_LAUNCH_CHECK("osc_drv_tile_kernel");
        if (F > S) {
            osc_drv_zero_tail_kernel<<<dim3((unsigned)ds::ceil_div(F - S, 256), (unsigned)A), 256, 0, st>>>(gforce, F, S);
            DS_LAUNCH_CHECK("osc_drv_zero_tail_kernel");
        }
    }
    osc_drv_mode_kernel<<<dim3((unsigned)m, (unsigned)A), 64, 0, st>>>(gy, d, w, amp, force, F, m, S, nt, inv_sr, lbnd, gamp,
                                                                     gpart);
    DS_LAUNCH_CHECK("osc_drv_mode_kernel");
    osc_drv_reduce_kernel<<<(unsigned)ds::ceil_div(m, 64), 64, 0, st>>>(gpart, A, m, inv_sr, gd, gw);
    DS_LAUNCH_CHECK("osc_drv_reduce_kernel");
    return DS_OK;
}
