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
//   boundary pass on gy       as in osc_driven.hip (GAIN = false below).
//   tile pass on gy (gforce)  weights the OUTPUT, acc[i] += am g_i Im l, not the input.
//   mode pass                 u = x + g f; and ggain: each lane has two partials per tile, the (1 - th) and th weighted sums
//                             of f Im l over its run; a segmented shuffle scan adds the lanes of a frame in a fixed order,
//                             a frame that straddles a tile boundary is carried in a (wave-uniform) register, and the lane
//                             that ends a frame stores it - every frame once.
// No atomics, nothing of size (A, m, S) in memory, the workspace of the driven bank.
#include <algorithm>
#include <cstdint>

#include "ds_common.h"
#include "osc_scan.h"

namespace {

using namespace osc_scan;

static_assert(RUN == DS_OSC_SCAN_RUN, "hop is refused unless it is a multiple of the lane's run");

// (lane_gain / load_gain, the two gains of a lane's run and its interpolation weights: osc_scan.h)

// 1. one wavefront per (clip, mode): bnd[(a m + mm) ntiles + k] = the state entering tile k.  in: (A x ldin), zero from nin
// on; GAIN: driven by g_m in (the forward), else by in alone (the adjoint on gy: osc_driven.hip's pass).
template <bool REV, bool GAIN>
__global__ void __launch_bounds__(64)
    osc_sld_boundary_kernel(const double* __restrict__ dd, const double* __restrict__ ww, const float* __restrict__ in,
                            int ldin, int nin, const float* __restrict__ gain, int K, int hop, int m, int ntiles,
                            double inv_sr, double2* __restrict__ bnd) {
    const int mm = blockIdx.x, a = blockIdx.y, lane = threadIdx.x;
    const int q = REV ? 63 - lane : lane;
    const double d = dd[mm], w = ww[mm];
    const cplx z1 = zpow(d, w, inv_sr, 1), zq = zpow(d, w, inv_sr, RUN * q), zT = zpow(d, w, inv_sr, TILE);
    const float* row = in + (int64_t)a * ldin;
    const float* grow = GAIN ? gain + ((int64_t)a * m + mm) * K : nullptr;
    const double inv_hop = 1.0 / (double)hop;
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
        if (GAIN) {
            const lane_gain g = load_gain(grow, K, hop, inv_hop, t0 + lane * RUN);
#pragma unroll
            for (int i = 0; i < RUN; ++i) v[i] *= g.at(i);
        }
        const cplx s = scan_lanes<REV>(run_from_zero<REV>(v, z1), zq, lane);
        carry = tile_exit<REV>(s, carry, zT);
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
    __shared__ double s_part[4][64 * (RUN + 1)];  // (a lane's RUN sums padded to RUN + 1: no bank conflicts)
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
    for (int mm = wave; mm < m; mm += 4) {
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
#pragma unroll
    for (int i = 0; i < RUN; ++i) s_part[wave][lane * (RUN + 1) + i] = acc[i];
    __syncthreads();
    const int n = min(TILE, nout - t0);
    for (int j = threadIdx.x; j < n; j += blockDim.x) {
        const int o = (j / RUN) * (RUN + 1) + (j % RUN);
        out[(int64_t)a * ldout + t0 + j] = (float)((s_part[0][o] + s_part[1][o]) + (s_part[2][o] + s_part[3][o]));
    }
}

// 3. one wavefront per (clip, mode): gamp[a, mm], gpart[a m + mm] = amp sum_t (x[t-1] + g f[t]) l[t] and, where asked for,
// ggain[a, mm, :].  lbnd: the states of l entering every tile (from above), written by the boundary pass on gy.
//
// ggain.  Lane q of tile kt holds run kt 64 + q, which lies in frame kq = min(run / h, K - 1), h = hop / RUN runs per frame.
// Its partials p0 = sum_i (1 - th_i) f_i Im l_i and p1 = sum_i th_i f_i Im l_i belong to frames kq and kq + 1 (p1 = 0 where
// the last frame is held).  P0[k], P1[k] = the sums over the runs of frame k: a shuffle scan cut at the frames' first lanes
// adds them inside the tile, (c0, c1) carry the frame that is open at the tile's end, prev1 = P1 of the frame before the open
// one, and the lane after which the frame changes (or the last lane of the last tile) stores am (P0[k] + P1[k-1]).
__global__ void __launch_bounds__(64)
    osc_sld_mode_kernel(const float* __restrict__ gy, const double* __restrict__ dd, const double* __restrict__ ww,
                        const float* __restrict__ amp, const float* __restrict__ force, const float* __restrict__ gain, int F,
                        int m, int S, int K, int hop, int ntiles, double inv_sr, const double2* __restrict__ lbnd,
                        float* __restrict__ gamp, double2* __restrict__ gpart, float* __restrict__ ggain) {
    const int mm = blockIdx.x, a = blockIdx.y, lane = threadIdx.x;
    const double d = dd[mm], w = ww[mm];
    const double am = amp ? (double)amp[(int64_t)a * m + mm] : 1.0;
    const cplx z1 = zpow(d, w, inv_sr, 1), zT = zpow(d, w, inv_sr, TILE);
    const cplx zq_up = zpow(d, w, inv_sr, RUN * lane), zq_dn = zpow(d, w, inv_sr, RUN * (63 - lane));
    const int nf = min(F, S);
    const int h = hop / RUN;
    const double inv_hop = 1.0 / (double)hop;
    const float* frow = force + (int64_t)a * F;
    const float* grow = gy + (int64_t)a * S;
    const float* gnrow = gain + ((int64_t)a * m + mm) * K;
    float* ggrow = ggain ? ggain + ((int64_t)a * m + mm) * K : nullptr;
    const double2* lb = lbnd + ((int64_t)a * m + mm) * ntiles;
    cplx cx = {0.0, 0.0}, G = {0.0, 0.0};
    double ga = 0.0;
    double c0 = 0.0, c1 = 0.0, prev1 = 0.0, last1 = 0.0;  // last1: P1 so far of the frame of the last lane
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
        const cplx sf = scan_lanes<false>(ef, zq_up, lane);
        cplx x = lane_entry<false>(sf, cx, zq_up, lane);
        cx = tile_exit<false>(sf, cx, zT);
        const cplx sl = scan_lanes<true>(run_from_zero<true>(g, z1), zq_dn, lane);
        const double2 c = lb[k];
        cplx l = lane_entry<true>(sl, cplx{c.x, c.y}, zq_dn, lane);
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
            const int run = k * 64 + lane;
            const int kq = min(run / h, K - 1), kn = min((run + 1) / h, K - 1);
            const int s = kq * h - k * 64;  // the lane of this tile at which frame kq starts (<= 0: in an earlier tile)
            const int s0 = max(s, 0);
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const double u0 = __shfl_up(p0, o, 64), u1 = __shfl_up(p1, o, 64);
                if (lane - o >= s0) {
                    p0 += u0;
                    p1 += u1;
                }
            }
            if (s <= 0) {
                p0 += c0;
                p1 += c1;
            }
            const double pl = __shfl(p1, max(s - 1, 0), 64);  // the last lane of frame kq - 1, where it is in this tile
            const double before = s > 0 ? pl : prev1;
            if (kn != kq || (k == ntiles - 1 && lane == 63)) ggrow[kq] = (float)(am * (p0 + before));
            const int k63 = __shfl(kq, 63, 64), kn63 = __shfl(kn, 63, 64);
            const double e0 = __shfl(p0, 63, 64), e1 = __shfl(p1, 63, 64), b63 = __shfl(before, 63, 64);
            last1 = e1;
            if (kn63 == k63) {
                c0 = e0;
                c1 = e1;
                prev1 = b63;
            } else {
                c0 = c1 = 0.0;
                prev1 = e1;
            }
        }
    }
    if (ggrow) {  // frames past the last tile: the first one hears the th weights of the last tile's last frame, the others nothing
        const int klast = min((ntiles * 64 - 1) / h, K - 1);
        if (lane == 0 && klast + 1 < K) ggrow[klast + 1] = (float)(am * last1);
        for (int kz = klast + 2 + lane; kz < K; kz += 64) ggrow[kz] = 0.f;
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
__global__ void osc_sld_reduce_kernel(const double2* __restrict__ gpart, int A, int m, double inv_sr,
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
__global__ void osc_sld_zero_tail_kernel(float* __restrict__ gforce, int F, int S) {
    const int j = S + blockIdx.x * blockDim.x + threadIdx.x;
    if (j < F) gforce[(int64_t)blockIdx.y * F + j] = 0.f;
}

inline int64_t ntiles_of(int S) { return ds::ceil_div(S, TILE); }

inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// The checks both entry points make before those of their own operands' alignment, in their order; `fn` names the entry point
int check_args(const char* fn, bool pointers, int A, int m, int F, int S, int K, int hop, double sr, const void* work,
               int64_t work_bytes) {
    DS_REQUIRE(pointers, "%s: null pointer", fn);
    DS_REQUIRE(A > 0 && m > 0 && S > 0 && F > 0 && K > 0, "%s: empty problem (A %d, m %d, F %d, S %d, K %d)", fn, A, m, F, S, K);
    DS_REQUIRE(A <= 65535, "%s: A = %d above 65535", fn, A);
    DS_REQUIRE(hop > 0 && hop % DS_OSC_SCAN_RUN == 0, "%s: hop = %d is not a positive multiple of %d", fn, hop,
               DS_OSC_SCAN_RUN);
    DS_REQUIRE(sr > 0, "%s: sr = %g is not positive", fn, sr);
    DS_REQUIRE(work_bytes >= ds_osc_slide_workspace_bytes(A, m, S, K, hop), "%s: workspace of %lld bytes, %lld needed", fn,
               (long long)work_bytes, (long long)ds_osc_slide_workspace_bytes(A, m, S, K, hop));
    DS_REQUIRE(aligned(work, 16), "%s: work not 16-byte aligned", fn);
    return DS_OK;
}

}  // namespace

extern "C" int64_t ds_osc_slide_workspace_bytes(int A, int m, int S, int K, int hop) {
    if (A <= 0 || m <= 0 || S <= 0 || K <= 0 || hop <= 0 || hop % DS_OSC_SCAN_RUN != 0) return 0;
    return (int64_t)sizeof(double2) * ((int64_t)A * m * ntiles_of(S) + (int64_t)A * m);
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
    osc_sld_boundary_kernel<false, true><<<dim3((unsigned)m, (unsigned)A), 64, 0, st>>>(d, w, force, F, nin, gain, K, hop, m, nt,
                                                                                      inv_sr, bnd);
    DS_LAUNCH_CHECK("osc_sld_boundary_kernel");
    osc_sld_tile_kernel<false><<<dim3((unsigned)nt, (unsigned)A), 256, 0, st>>>(d, w, amp, force, F, nin, gain, K, hop, m, nt,
                                                                               inv_sr, bnd, y, S, S);
    DS_LAUNCH_CHECK("osc_sld_tile_kernel");
    return DS_OK;
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
    const int nt = (int)ntiles_of(S);
    double2* lbnd = static_cast<double2*>(work);
    double2* gpart = lbnd + (int64_t)A * m * nt;
    const double inv_sr = 1.0 / sr;
    osc_sld_boundary_kernel<true, false><<<dim3((unsigned)m, (unsigned)A), 64, 0, st>>>(d, w, gy, S, S, nullptr, K, hop, m, nt,
                                                                                      inv_sr, lbnd);
    DS_LAUNCH_CHECK("osc_sld_boundary_kernel");
    if (gforce) {
        osc_sld_tile_kernel<true><<<dim3((unsigned)nt, (unsigned)A), 256, 0, st>>>(d, w, amp, gy, S, S, gain, K, hop, m, nt, inv_sr,
                                                                                  lbnd, gforce, F, std::min(F, S));
        DS_LAUNCH_CHECK("osc_sld_tile_kernel");
        if (F > S) {
            osc_sld_zero_tail_kernel<<<dim3((unsigned)ds::ceil_div(F - S, 256), (unsigned)A), 256, 0, st>>>(gforce, F, S);
            DS_LAUNCH_CHECK("osc_sld_zero_tail_kernel");
        }
    }
    osc_sld_mode_kernel<<<dim3((unsigned)m, (unsigned)A), 64, 0, st>>>(gy, d, w, amp, force, gain, F, m, S, K, hop, nt, inv_sr,
                                                                     lbnd, gamp, gpart, ggain);
    DS_LAUNCH_CHECK("osc_sld_mode_kernel");
    osc_sld_reduce_kernel<<<(unsigned)ds::ceil_div(m, 64), 64, 0, st>>>(gpart, A, m, inv_sr, gd, gw);
    DS_LAUNCH_CHECK("osc_sld_reduce_kernel");
    return DS_OK;
}
