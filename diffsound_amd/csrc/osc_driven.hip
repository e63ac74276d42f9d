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

#include "osc_bank.h"
#include "osc_scan.h"

namespace {

// the lane-scan helpers (cplx, cmul, zpow, from_prev, load_run, run_from_zero, scan_lanes, lane_entry, tile_exit), the waves'
// join and the pieces of the mode pass: osc_scan.h
using namespace osc_scan;
using ds::aligned;
using osc_bank::ntiles_of;

// 1. one wavefront per (clip, mode): bnd[(a m + mm) ntiles + k] = the state entering tile k.  in: (A x ldin), zero from nin on.
// The pass of every bank whose drive is a real row (osc_bank::launch_boundary).  The loop stays written out here and in the
// two kernels that copy it (osc_slide.hip, osc_listen.hip): inside a shared function the compiler rounds the other product of
// Im(zT carry) before the fused multiply-add, and the states entering the third tile move by an ulp.
template <bool REV>
__global__ void __launch_bounds__(64)
    osc_boundary_kernel(const double* __restrict__ dd, const double* __restrict__ ww, const float* __restrict__ in,
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
    __shared__ double s_part[WAVES][PART];
    const int k = blockIdx.x, a = blockIdx.y;
    const int t0 = k * TILE;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q = REV ? 63 - lane : lane;
    const bool driven = t0 < nin;
    double v[RUN], acc[RUN];
    load_run(in + (int64_t)a * ldin, t0, lane, nin, v);
#pragma unroll
    for (int i = 0; i < RUN; ++i) acc[i] = 0.0;
    for (int mm = wave; mm < m; mm += WAVES) {
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
    join_waves(s_part, acc, lane, wave, min(TILE, nout - t0), out + (int64_t)a * ldout + t0);
}

// 3. one wavefront per (clip, mode): gamp[a, mm] and gpart[a m + mm] = amp sum_t (x[t-1] + f[t]) l[t].  lbnd: the states
// of l entering every tile (from above), written by osc_boundary_kernel<true> on gy.
__global__ void __launch_bounds__(64)
    osc_drv_mode_kernel(const float* __restrict__ gy, const double* __restrict__ dd, const double* __restrict__ ww,
                        const float* __restrict__ amp, const float* __restrict__ force, int F, int m, int S, int ntiles,
                        double inv_sr, const double2* __restrict__ lbnd, float* __restrict__ gamp,
                        double2* __restrict__ gpart) {
    const int mm = blockIdx.x, a = blockIdx.y, lane = threadIdx.x;
    const int64_t am_at = (int64_t)a * m + mm;
    const mode_powers p = load_mode(dd, ww, amp, am_at, mm, lane, inv_sr);
    const cplx z1 = p.z1;
    const int nf = min(F, S);
    const float* frow = force + (int64_t)a * F;
    const float* grow = gy + (int64_t)a * S;
    const double2* lb = lbnd + am_at * ntiles;
    cplx cx = {0.0, 0.0}, G = {0.0, 0.0};
    double ga = 0.0;
    for (int k = 0; k < ntiles; ++k) {
        const int t0 = k * TILE;
        double f[RUN], g[RUN];
        load_run(frow, t0, lane, nf, f);
        load_run(grow, t0, lane, S, g);
        cplx ef = {0.0, 0.0};
        if (t0 < nf) ef = run_from_zero<false>(f, z1);
        const cplx sf = scan_lanes<false>(ef, p.zq_up, lane);
        cplx x = lane_entry<false>(sf, cx, p.zq_up, lane);
        cx = tile_exit<false>(sf, cx, p.zT);
        const cplx sl = scan_lanes<true>(run_from_zero<true>(g, z1), p.zq_dn, lane);
        const double2 c = lb[k];
        cplx l = lane_entry<true>(sl, cplx{c.x, c.y}, p.zq_dn, lane);
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
    store_mode(ga, G, p.am, lane, am_at, gamp, gpart);
}

// gd[mm] = -Im sum_a G / sr, gw[mm] = Re sum_a G / sr, the clips added in order
__global__ void osc_reduce_kernel(const double2* __restrict__ gpart, int A, int m, double inv_sr, double* __restrict__ gd,
                                  double* __restrict__ gw) {
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
__global__ void osc_zero_tail_kernel(float* __restrict__ gforce, int F, int S) {
    const int j = S + blockIdx.x * blockDim.x + threadIdx.x;
    if (j < F) gforce[(int64_t)blockIdx.y * F + j] = 0.f;
}

// The checks both entry points make before those of their own operands' alignment, in their order; `fn` names the entry point
int check_args(const char* fn, bool pointers, int A, int m, int F, int S, double sr, const void* work, int64_t work_bytes) {
    DS_REQUIRE(pointers, "%s: null pointer", fn);
    DS_REQUIRE(A > 0 && m > 0 && S > 0 && F > 0 && sr > 0, "%s: empty problem (A %d, m %d, F %d, S %d)", fn, A, m, F, S);
    if (int rc = osc_bank::check_clips(fn, A)) return rc;
    return osc_bank::check_work(fn, work, work_bytes, ds_osc_driven_workspace_bytes(A, m, S));
}

}  // namespace

int osc_bank::launch_boundary(hipStream_t st, bool rev, const double* d, const double* w, const float* in, int ldin, int nin,
                              int A, int m, int nt, double inv_sr, double2* bnd) {
    const dim3 grid((unsigned)m, (unsigned)A);
    if (rev)
        osc_boundary_kernel<true><<<grid, 64, 0, st>>>(d, w, in, ldin, nin, m, nt, inv_sr, bnd);
    else
        osc_boundary_kernel<false><<<grid, 64, 0, st>>>(d, w, in, ldin, nin, m, nt, inv_sr, bnd);
    return DS_LAUNCHED("osc_boundary_kernel");
}

int osc_bank::launch_reduce(hipStream_t st, const double2* gpart, int A, int m, double inv_sr, double* gd, double* gw) {
    osc_reduce_kernel<<<(unsigned)ds::ceil_div(m, 64), 64, 0, st>>>(gpart, A, m, inv_sr, gd, gw);
    return DS_LAUNCHED("osc_reduce_kernel");
}

int osc_bank::launch_zero_tail(hipStream_t st, float* gforce, int A, int F, int S) {
    osc_zero_tail_kernel<<<dim3((unsigned)ds::ceil_div(F - S, 256), (unsigned)A), 256, 0, st>>>(gforce, F, S);
    return DS_LAUNCHED("osc_zero_tail_kernel");
}

extern "C" int64_t ds_osc_driven_workspace_bytes(int A, int m, int S) {
    if (A <= 0 || m <= 0 || S <= 0) return 0;
    return osc_bank::workspace_bytes(A, m, S);
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
    if (int rc = osc_bank::launch_boundary(st, false, d, w, force, F, nin, A, m, nt, inv_sr, bnd)) return rc;
    osc_drv_tile_kernel<false><<<dim3((unsigned)nt, (unsigned)A), 256, 0, st>>>(d, w, amp, force, F, nin, m, nt, inv_sr, bnd, y,
                                                                               S, S);
    return DS_LAUNCHED("osc_drv_tile_kernel");
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
    const double inv_sr = 1.0 / sr;
    return osc_bank::backward(
        st, A, m, F, S, inv_sr, work, gd, gw, gforce,
        [&](int nt, double2* lbnd) { return osc_bank::launch_boundary(st, true, d, w, gy, S, S, A, m, nt, inv_sr, lbnd); },
        [&](int nt, const double2* lbnd) {
            osc_drv_tile_kernel<true><<<dim3((unsigned)nt, (unsigned)A), 256, 0, st>>>(d, w, amp, gy, S, S, m, nt, inv_sr, lbnd,
                                                                                      gforce, F, std::min(F, S));
            return DS_LAUNCHED("osc_drv_tile_kernel");
        },
        [&](int nt, const double2* lbnd, double2* gpart) {
            osc_drv_mode_kernel<<<dim3((unsigned)m, (unsigned)A), 64, 0, st>>>(gy, d, w, amp, force, F, m, S, nt, inv_sr, lbnd, gamp,
                                                                             gpart);
            return DS_LAUNCHED("osc_drv_mode_kernel");
        });
}
