// Sliding contact: the driven oscillator bank of osc_driven.hip with an input gain per mode AND per sample - gfx950.
//
// A scrape, a roll or a bow stroke is a force whose contact point moves while it acts: the gain c_i(p(t)) = d . u_i(p(t)) of
// mode i (csrc/modesample.hip) is then a function of time and multiplies the force BEFORE the resonator.  The reference has
// no counterpart (its amp, src/ddsp/oscillator.py:76, is one free number per clip and mode).  With z_m = exp((-d_m + i w_m) / sr):
//     x_m[t] = z_m (x_m[t-1] + g_m[a,t] f[a,t]),  x[-1] = 0,  f[t] = 0 for t >= F,      y[a,t] = sum_m amp[a,m] Im x_m[t],
//     g_m[a,t] = (1 - th) gain[a,m,k] + th gain[a,m,min(k+1, K-1)],  k = min(t / hop, K-1),  th = (t - k hop) / hop,
//                th = 0 where t / hop >= K-1:
// the gains are piecewise linear between K control frames hop samples apart, the last frame is held, th and the
// interpolation are fp64 from the fp32 gains.  The adjoint runs the same recurrence down in time, l_m[t] = z_m (l_m[t+1] +
// gy[t]), l[S] = 0, and with gin_m[j] = amp_m Im l_m[j]:
//     gforce[a,j] = sum_m g_m[a,j] gin_m[j]  for j < min(F, S), exactly 0 for S <= j < F,
//     ggain[a,m,k] = sum_j hat_k(j) f[a,j] gin_m[j],  hat_k the two interpolation weights (the clamped ones land on K-1);
//                   a frame that no driven sample touches gets exactly 0,
//     gamp[a,m] = sum_t gy[t] Im x_m[t],
//     G_m = sum_a amp sum_t (x[t-1] + g f[t]) l[t]  (complex, no conjugate),  gd = -Im G / sr,  gw = Re G / sr.
// K = 1 is a constant input gain; with all gains 1 the result is the driven bank's y.
//
// The scan is that of osc_driven.hip (osc_scan.h): a lane owns RUN samples, a wave a tile of 64 RUN, boundary pass / tile
// pass / mode pass, every power z^n in closed form, fp64 states, one fp32 rounding per stored element.  hop is a multiple
// of RUN, so a lane's run lies inside ONE frame interval and a lane needs two gains per mode (gain, ggain: (A, m, K), the
// frames contiguous).  Against the driven kernels:
//   boundary pass (forward)   the per-mode input is g_m f; a tile past the end of the force is still one product by z^TILE.
//   tile pass (forward)       the lane's v[i] becomes g_i v[i] per mode.
//   boundary pass on gy       osc_driven.hip's own (osc_bank::launch_boundary).
//   tile pass on gy (gforce)  weights the OUTPUT, acc[i] += am g_i Im l, not the input.
//   mode pass                 u = x + g f; and ggain: each lane has two partials per tile, the (1 - th) and th weighted sums
//                             of f Im l over its run; a segmented shuffle scan adds the lanes of a frame in a fixed order,
//                             a frame that straddles a tile boundary is carried in a (wave-uniform) register, and the lane
//                             that ends a frame stores it - every frame once.
// No atomics, nothing of size (A, m, S) in memory, the workspace of the driven bank.
#include <algorithm>

#include "osc_bank.h"
#include "osc_scan.h"

namespace {

using namespace osc_scan;
using ds::aligned;
using osc_bank::ntiles_of;

static_assert(RUN == DS_OSC_SCAN_RUN, "hop is refused unless it is a multiple of the lane's run");

// (lane_gain / load_gain, the two gains of a lane's run and its interpolation weights: osc_scan.h)

// 1. one wavefront per (clip, mode): bnd[(a m + mm) ntiles + k] = the state of x entering tile k, x driven by g_m force
// (force: A x F, zero from nin on).  osc_driven.hip's boundary loop with the gain on its input; the adjoint's pass on gy is
// that kernel itself (osc_bank::launch_boundary).  q and k are spelled as in that loop (REV = false) ON PURPOSE: this shape
// compiles to the instructions the outputs were pinned with, and a tidier one may round Im(zT carry) the other way.
__global__ void __launch_bounds__(64)
    osc_sld_boundary_kernel(const double* __restrict__ dd, const double* __restrict__ ww, const float* __restrict__ in,
                            int ldin, int nin, const float* __restrict__ gain, int K, int hop, int m, int ntiles,
                            double inv_sr, double2* __restrict__ bnd) {
    const int mm = blockIdx.x, a = blockIdx.y, lane = threadIdx.x;
    const int q = lane;
    const double d = dd[mm], w = ww[mm];
    const cplx z1 = zpow(d, w, inv_sr, 1), zq = zpow(d, w, inv_sr, RUN * q), zT = zpow(d, w, inv_sr, TILE);
    const float* row = in + (int64_t)a * ldin;
    const float* grow = gain + ((int64_t)a * m + mm) * K;
    const double inv_hop = 1.0 / (double)hop;
    double2* b = bnd + ((int64_t)a * m + mm) * ntiles;
    cplx carry = {0.0, 0.0};
    for (int kk = 0; kk < ntiles; ++kk) {
        const int k = kk;
        if (lane == 0) b[k] = make_double2(carry.r, carry.i);
        if (kk == ntiles - 1) break;
        const int t0 = k * TILE;
        if (t0 >= nin) {  // (wave-uniform) nothing drives this tile
            carry = cmul(zT, carry);
            continue;
        }
        double v[RUN];
        load_run(row, t0, lane, nin, v);
        const lane_gain g = load_gain(grow, K, hop, inv_hop, t0 + lane * RUN);
#pragma unroll
        for (int i = 0; i < RUN; ++i) v[i] *= g.at(i);
        const cplx s = scan_lanes<false>(run_from_zero<false>(v, z1), zq, lane);
        carry = tile_exit<false>(s, carry, zT);
    }
}

// 2. workgroup = (tile, clip).  REV = false: out[a, t] = sum_m amp Im x_m[t], x driven by g_m in (y).  REV = true:
// out[a, j] = sum_m amp g_m[a, j] Im l_m[j], l driven by in = gy (gforce).  t, j < nout; out: (A x ldout).
template <bool REV>
__global__ void __launch_bounds__(256)
    osc_sld_tile_kernel(const double* __restrict__ dd, const double* __restrict__ ww, const float* __restrict__ amp,
                        const float* __restrict__ in, int ldin, int nin, const float* __restrict__ gain, int K, int hop, int m,
                        int ntiles, double inv_sr, const double2* __restrict__ bnd, float* __restrict__ out, int ldout,
                        int nout) {
    __shared__ double s_part[WAVES][PART];
    const int k = blockIdx.x, a = blockIdx.y;
    const int t0 = k * TILE;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q = REV ? 63 - lane : lane;
    const bool driven = t0 < nin;
    const double inv_hop = 1.0 / (double)hop;
    double v[RUN], acc[RUN];
    load_run(in + (int64_t)a * ldin, t0, lane, nin, v);
#pragma unroll
    for (int i = 0; i < RUN; ++i) acc[i] = 0.0;
    for (int mm = wave; mm < m; mm += WAVES) {
        const double d = dd[mm], w = ww[mm];
        const double am = amp ? (double)amp[(int64_t)a * m + mm] : 1.0;
        const cplx z1 = zpow(d, w, inv_sr, 1), zq = zpow(d, w, inv_sr, RUN * q);
        const double2 c = bnd[((int64_t)a * m + mm) * ntiles + k];
        const lane_gain g = load_gain(gain + ((int64_t)a * m + mm) * K, K, hop, inv_hop, t0 + lane * RUN);
        if (!REV) {
            double u[RUN];
#pragma unroll
            for (int i = 0; i < RUN; ++i) u[i] = g.at(i) * v[i];
            cplx e = {0.0, 0.0};
            if (driven) e = run_from_zero<false>(u, z1);
            cplx x = lane_entry<false>(scan_lanes<false>(e, zq, lane), cplx{c.x, c.y}, zq, lane);
#pragma unroll
            for (int i = 0; i < RUN; ++i) {
                x = cmul(z1, cplx{x.r + u[i], x.i});
                acc[i] += am * x.i;
            }
        } else {
            cplx e = {0.0, 0.0};
            if (driven) e = run_from_zero<true>(v, z1);
            cplx x = lane_entry<true>(scan_lanes<true>(e, zq, lane), cplx{c.x, c.y}, zq, lane);
#pragma unroll
            for (int i = RUN - 1; i >= 0; --i) {
                x = cmul(z1, cplx{x.r + v[i], x.i});
                acc[i] += (am * g.at(i)) * x.i;
            }
        }
    }
    join_waves(s_part, acc, lane, wave, min(TILE, nout - t0), out + (int64_t)a * ldout + t0);
}

// 3. one wavefront per (clip, mode): gamp[a, mm], gpart[a m + mm] = amp sum_t (x[t-1] + g f[t]) l[t] and, where asked for,
// ggain[a, mm, :].  lbnd: the states of l entering every tile (from above), written by the boundary pass on gy.
//
// ggain.  A lane's partials p0 = sum_i (1 - th_i) f_i Im l_i and p1 = sum_i th_i f_i Im l_i belong to the frame kq of its run
// and to kq + 1; frame_scan (osc_scan.h) adds the lanes of a frame, (c0, c1, prev1, last1) carry the frame that is open at the
// tile's end, and the lane after which the frame changes (or the last lane of the last tile) stores am (P0[k] + P1[k-1]).
__global__ void __launch_bounds__(64)
    osc_sld_mode_kernel(const float* __restrict__ gy, const double* __restrict__ dd, const double* __restrict__ ww,
                        const float* __restrict__ amp, const float* __restrict__ force, const float* __restrict__ gain, int F,
                        int m, int S, int K, int hop, int ntiles, double inv_sr, const double2* __restrict__ lbnd,
                        float* __restrict__ gamp, double2* __restrict__ gpart, float* __restrict__ ggain) {
    const int mm = blockIdx.x, a = blockIdx.y, lane = threadIdx.x;
    const int64_t am_at = (int64_t)a * m + mm;
    const mode_powers p = load_mode(dd, ww, amp, am_at, mm, lane, inv_sr);
    const cplx z1 = p.z1;
    const double am = p.am;
    const int nf = min(F, S);
    const int h = hop / RUN;
    const double inv_hop = 1.0 / (double)hop;
    const float* frow = force + (int64_t)a * F;
    const float* grow = gy + (int64_t)a * S;
    const float* gnrow = gain + am_at * K;
    float* ggrow = ggain ? ggain + am_at * K : nullptr;
    const double2* lb = lbnd + am_at * ntiles;
    cplx cx = {0.0, 0.0}, G = {0.0, 0.0};
    double ga = 0.0;
    double c0 = 0.0, c1 = 0.0, prev1 = 0.0, last1 = 0.0;
    for (int k = 0; k < ntiles; ++k) {
        const int t0 = k * TILE;
        double f[RUN], g[RUN];
        load_run(frow, t0, lane, nf, f);
        load_run(grow, t0, lane, S, g);
        const lane_gain gn = load_gain(gnrow, K, hop, inv_hop, t0 + lane * RUN);
        cplx ef = {0.0, 0.0};
        if (t0 < nf) {
#pragma unroll
            for (int i = 0; i < RUN; ++i) ef = cmul(z1, cplx{ef.r + gn.at(i) * f[i], ef.i});
        }
        cplx x = x_entry(ef, p, lane, cx);
        cplx l = l_entry(run_from_zero<true>(g, z1), p, lane, lb[k]);
        cplx u[RUN];
#pragma unroll
        for (int i = 0; i < RUN; ++i) {
            u[i] = cplx{x.r + gn.at(i) * f[i], x.i};
            x = cmul(z1, u[i]);
            ga += g[i] * x.i;
        }
        double p0 = 0.0, p1 = 0.0;
#pragma unroll
        for (int i = RUN - 1; i >= 0; --i) {
            l = cmul(z1, cplx{l.r + g[i], l.i});
            const cplx t = cmul(u[i], l);
            G.r += t.r;
            G.i += t.i;
            const double fl = f[i] * l.i, th = gn.theta(i);
            p0 += (1.0 - th) * fl;
            p1 += th * fl;
        }
        if (ggrow) {  // (wave-uniform)
            const frame_pos fp = frame_of(k, lane, h, K, ntiles);
            const double out = frame_scan(p0, p1, fp, lane, c0, c1, prev1, last1);
            if (fp.ends) ggrow[fp.kq] = (float)(am * out);
        }
    }
    if (ggrow) {  // frames past the last tile: the first one hears the th weights of the last tile's last frame, the others nothing
        const int klast = last_frame(ntiles, h, K);
        if (lane == 0 && klast + 1 < K) ggrow[klast + 1] = (float)(am * last1);
        for (int kz = klast + 2 + lane; kz < K; kz += 64) ggrow[kz] = 0.f;
    }
    store_mode(ga, G, am, lane, am_at, gamp, gpart);
}

// The checks both entry points make before those of their own operands' alignment, in their order; `fn` names the entry point
int check_args(const char* fn, bool pointers, int A, int m, int F, int S, int K, int hop, double sr, const void* work,
               int64_t work_bytes) {
    DS_REQUIRE(pointers, "%s: null pointer", fn);
    DS_REQUIRE(A > 0 && m > 0 && S > 0 && F > 0 && K > 0, "%s: empty problem (A %d, m %d, F %d, S %d, K %d)", fn, A, m, F, S, K);
    if (int rc = osc_bank::check_clips(fn, A)) return rc;
    if (int rc = osc_bank::check_frames(fn, hop, sr)) return rc;
    return osc_bank::check_work(fn, work, work_bytes, ds_osc_slide_workspace_bytes(A, m, S, K, hop));
}

}  // namespace

extern "C" int64_t ds_osc_slide_workspace_bytes(int A, int m, int S, int K, int hop) {
    if (A <= 0 || m <= 0 || S <= 0 || K <= 0 || hop <= 0 || hop % DS_OSC_SCAN_RUN != 0) return 0;
    return osc_bank::workspace_bytes(A, m, S);
}

extern "C" int ds_osc_slide_fwd(const double* d, const double* w, const float* amp, const float* force, const float* gain,
                                int A, int m, int F, int S, int K, int hop, double sr, void* work, int64_t work_bytes,
                                float* y, ds_stream_t stream) {
    if (int rc = check_args("ds_osc_slide_fwd", d && w && force && gain && work && y, A, m, F, S, K, hop, sr, work, work_bytes))
        return rc;
    DS_REQUIRE(aligned(d, 8) && aligned(w, 8) && aligned(force, 4) && aligned(gain, 4) && aligned(y, 4) && aligned(amp, 4),
               "ds_osc_slide_fwd: misaligned operand");
    hipStream_t st = ds::as_stream(stream);
    const int nt = (int)ntiles_of(S);
    const int nin = std::min(F, S);
    double2* bnd = static_cast<double2*>(work);
    const double inv_sr = 1.0 / sr;
    osc_sld_boundary_kernel<<<dim3((unsigned)m, (unsigned)A), 64, 0, st>>>(d, w, force, F, nin, gain, K, hop, m, nt, inv_sr, bnd);
    DS_LAUNCH_CHECK("osc_sld_boundary_kernel");
    osc_sld_tile_kernel<false><<<dim3((unsigned)nt, (unsigned)A), 256, 0, st>>>(d, w, amp, force, F, nin, gain, K, hop, m, nt,
                                                                               inv_sr, bnd, y, S, S);
    return DS_LAUNCHED("osc_sld_tile_kernel");
}

extern "C" int ds_osc_slide_bwd(const float* gy, const double* d, const double* w, const float* amp, const float* force,
                                const float* gain, int A, int m, int F, int S, int K, int hop, double sr, void* work,
                                int64_t work_bytes, double* gd, double* gw, float* gamp, float* gforce, float* ggain,
                                ds_stream_t stream) {
    if (int rc = check_args("ds_osc_slide_bwd", gy && d && w && force && gain && work && gd && gw, A, m, F, S, K, hop, sr, work,
                            work_bytes))
        return rc;
    DS_REQUIRE(aligned(gd, 8) && aligned(gw, 8), "ds_osc_slide_bwd: gd or gw not 8-byte aligned");
    DS_REQUIRE(aligned(d, 8) && aligned(w, 8) && aligned(force, 4) && aligned(gain, 4) && aligned(gy, 4) && aligned(amp, 4) &&
                   aligned(gamp, 4) && aligned(gforce, 4) && aligned(ggain, 4),
               "ds_osc_slide_bwd: misaligned operand");
    hipStream_t st = ds::as_stream(stream);
    const double inv_sr = 1.0 / sr;
    return osc_bank::backward(
        st, A, m, F, S, inv_sr, work, gd, gw, gforce,
        [&](int nt, double2* lbnd) { return osc_bank::launch_boundary(st, true, d, w, gy, S, S, A, m, nt, inv_sr, lbnd); },
        [&](int nt, const double2* lbnd) {
            osc_sld_tile_kernel<true><<<dim3((unsigned)nt, (unsigned)A), 256, 0, st>>>(d, w, amp, gy, S, S, gain, K, hop, m, nt,
                                                                                      inv_sr, lbnd, gforce, F, std::min(F, S));
            return DS_LAUNCHED("osc_sld_tile_kernel");
        },
        [&](int nt, const double2* lbnd, double2* gpart) {
            osc_sld_mode_kernel<<<dim3((unsigned)m, (unsigned)A), 64, 0, st>>>(gy, d, w, amp, force, gain, F, m, S, K, hop, nt,
                                                                             inv_sr, lbnd, gamp, gpart, ggain);
            return DS_LAUNCHED("osc_sld_mode_kernel");
        });
}
