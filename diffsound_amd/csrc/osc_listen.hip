// Listener bank: the driven oscillator bank of osc_driven.hip read out through a COMPLEX gain per (channel, mode, frame) -
// gfx950.
//
// A mode that rings as Im x_m is heard at a point as Im(H x_m), H the conjugate of the mode's transfer to that point
// (diffelastic/radiation.py): two ears differ mostly in the phase of H, and along a path H rotates, e^{ikr(t)}, which is
// the Doppler shift.  The recursive banks already hold the complex state; this one reads both of its parts.  With
// z_m = exp((-d_m + i w_m) / sr), x_m[a,-1] = 0, f[t] = 0 for t >= F:
//     x_m[a,t]    = z_m (x_m[a,t-1] + f[a,t]),
//     H[a,c,m](t) = (1 - th) h[a,c,m,k] + th h[a,c,m,min(k+1, K-1)],  k = min(t / hop, K-1),  th = (t - k hop) / hop,
//                   th = 0 where t / hop >= K-1                       (osc_slide.hip's frames; fp64 from the fp32 h),
//     y[a,c,t]    = sum_m amp[a,m] Im(H[a,c,m](t) x_m[a,t])           = sum_m amp (Hr Im x + Hi Re x).
// K = 1 is a listener at rest; C = 1, K = 1, h = 1 + 0i is the driven bank.  The adjoint has the no-conjugate form of the
// driven and the sliding bank - the loss is sum_t Im(wdrive x), linear in x, and Im(p q) is symmetric in p and q:
//     wdrive_m[a,t] = sum_c gy[a,c,t] H[a,c,m](t)                                    (complex),
//     l_m[a,t]    = z_m (l_m[a,t+1] + wdrive_m[a,t]),  l[S] = 0,
//     gforce[a,j] = sum_m amp Im l_m[a,j]  for j < min(F, S),  exactly 0 for S <= j < F,
//     gamp[a,m]   = sum_c sum_t gy[a,c,t] Im(H x_m[a,t]),
//     gh[a,c,m,k] = amp sum_t hat_k(t) gy[a,c,t] (Im x_m[a,t], Re x_m[a,t]),  hat_k the two interpolation weights;
//                   exactly (0, 0) for a frame that no sample t < S touches,
//     G_m = sum_a amp sum_t (x_m[t-1] + f[t]) l_m[t]  (complex, no conjugate),  gd = -Im G / sr,  gw = Re G / sr.
//
// The scan is that of osc_driven.hip (osc_scan.h): a lane owns RUN samples, a wave a tile of 64 RUN, every power z^n in
// closed form, fp64 states, one fp32 rounding per stored element.  hop is a multiple of RUN, so a lane's run lies inside
// ONE frame interval and a lane needs two complex gains per (channel, mode) (h, gh: (A, C, m, K, 2), frames contiguous,
// re / im innermost).
//   forward   boundary pass   the driven bank's: the states entering every tile do not depend on the channel.
//             tile pass       workgroup = (tile, clip, group of NC channels): a wave scans a mode ONCE and adds Im(H x) into
//                             the NC accumulator rows it keeps in registers; the four waves' partial sums are joined
//                             through LDS in the fixed order (0 + 1) + (2 + 3), one channel after the other.
//   backward  boundary pass   on the complex drive wdrive (time runs down).
//             tile pass       gforce: the l scan under wdrive, acc += amp Im l.
//             mode pass       one wavefront per (clip, mode): x up, l down, G, gamp, and gh - per channel the four
//                             partials (1 - th | th) x (Im x | Re x) of a lane's run, added over the lanes of a frame by
//                             osc_sld_mode_kernel's segmented shuffle scan; the frame that is open at a tile's end is
//                             carried in registers (the carries of channel c, wave-uniform, live in lane c).
//             reduce          the clips added in order.
// No atomics, nothing of size (A, m, S) in memory, the workspace of the driven bank.
#include <algorithm>

#include "osc_bank.h"
#include "osc_scan.h"

namespace {

using namespace osc_scan;
using ds::aligned;
using osc_bank::ntiles_of;

static_assert(RUN == DS_OSC_SCAN_RUN, "hop is refused unless it is a multiple of the lane's run");
static_assert(DS_OSC_LISTEN_MAX_CHANNELS <= 64, "the frame carries of channel c live in lane c");

// the K frames of (clip a, channel c, mode mm)
__device__ __forceinline__ const float2* hrow_of(const float* __restrict__ h, int a, int c, int mm, int C, int m, int K) {
    return reinterpret_cast<const float2*>(h) + (((int64_t)a * C + c) * m + mm) * K;
}

// the lane's complex drive of one mode: vr + i vi = sum_c gy[a,c,.] H[a,c,mm](.), the channels added in order
__device__ __forceinline__ void load_drive(const float* __restrict__ gy, const float* __restrict__ h, int a, int mm, int C, int m,
                                           int S, int K, int hop, double inv_hop, int t0, int lane, double* vr, double* vi) {
#pragma unroll
    for (int i = 0; i < RUN; ++i) vr[i] = vi[i] = 0.0;
    for (int c = 0; c < C; ++c) {
        double g[RUN];
        load_run(gy + ((int64_t)a * C + c) * S, t0, lane, S, g);
        const lane_cgain hg = load_cgain(hrow_of(h, a, c, mm, C, m, K), K, hop, inv_hop, t0 + lane * RUN);
#pragma unroll
        for (int i = 0; i < RUN; ++i) {
            const cplx H = hg.at(hg.theta(i));
            vr[i] += g[i] * H.r;
            vi[i] += g[i] * H.i;
        }
    }
}

// 1. one wavefront per (clip, mode): bnd[(a m + mm) ntiles + k] = the state of l entering tile k (from above), l driven by
// wdrive, which no tile below S is without.  (The forward's boundary pass does not depend on the channel: it is
// osc_driven.hip's, osc_bank::launch_boundary.)  q, k and the block around the drive are spelled as in that loop (REV = true)
// ON PURPOSE: a tidier shape may make the compiler round Im(zT carry) the other way, an ulp in the states.
__global__ void __launch_bounds__(64)
    osc_lis_boundary_kernel(const double* __restrict__ dd, const double* __restrict__ ww, const float* __restrict__ gy,
                            const float* __restrict__ h, int C, int K, int hop, int m, int S, int ntiles, double inv_sr,
                            double2* __restrict__ bnd) {
    const int mm = blockIdx.x, a = blockIdx.y, lane = threadIdx.x;
    const int q = 63 - lane;
    const double d = dd[mm], w = ww[mm];
    const cplx z1 = zpow(d, w, inv_sr, 1), zq = zpow(d, w, inv_sr, RUN * q), zT = zpow(d, w, inv_sr, TILE);
    const double inv_hop = 1.0 / (double)hop;
    double2* b = bnd + ((int64_t)a * m + mm) * ntiles;
    cplx carry = {0.0, 0.0};
    for (int kk = 0; kk < ntiles; ++kk) {
        const int k = ntiles - 1 - kk;
        if (lane == 0) b[k] = make_double2(carry.r, carry.i);
        if (kk == ntiles - 1) break;
        const int t0 = k * TILE;
        cplx e;
        {
            double vr[RUN], vi[RUN];
            load_drive(gy, h, a, mm, C, m, S, K, hop, inv_hop, t0, lane, vr, vi);
            e = run_from_zero<true>(vr, vi, z1);
        }
        const cplx s = scan_lanes<true>(e, zq, lane);
        carry = tile_exit<true>(s, carry, zT);
    }
}

// 2. workgroup = (tile, clip, group of NC channels): y[a, c, t] = sum_m amp Im(H[a,c,m](t) x_m[t]).  A channel of the group
// past C - 1 is computed as channel C - 1 and not stored.
template <int NC>
__global__ void __launch_bounds__(256)
    osc_lis_tile_kernel(const double* __restrict__ dd, const double* __restrict__ ww, const float* __restrict__ amp,
                        const float* __restrict__ force, int F, int nin, const float* __restrict__ h, int C, int K, int hop, int m,
                        int ntiles, double inv_sr, const double2* __restrict__ bnd, float* __restrict__ y, int S) {
    __shared__ double s_part[WAVES][PART];
    const int k = blockIdx.x, a = blockIdx.y, c0 = blockIdx.z * NC;
    const int t0 = k * TILE;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool driven = t0 < nin;
    const double inv_hop = 1.0 / (double)hop;
    double v[RUN], acc[NC][RUN];
    load_run(force + (int64_t)a * F, t0, lane, nin, v);
#pragma unroll
    for (int j = 0; j < NC; ++j)
#pragma unroll
        for (int i = 0; i < RUN; ++i) acc[j][i] = 0.0;
    for (int mm = wave; mm < m; mm += WAVES) {
        const double d = dd[mm], w = ww[mm];
        const double am = amp ? (double)amp[(int64_t)a * m + mm] : 1.0;
        const cplx z1 = zpow(d, w, inv_sr, 1), zq = zpow(d, w, inv_sr, RUN * lane);
        const double2 c = bnd[((int64_t)a * m + mm) * ntiles + k];
        lane_cgain hg[NC];
#pragma unroll
        for (int j = 0; j < NC; ++j)
            hg[j] = load_cgain(hrow_of(h, a, min(c0 + j, C - 1), mm, C, m, K), K, hop, inv_hop, t0 + lane * RUN);
        cplx e = {0.0, 0.0};
        if (driven) e = run_from_zero<false>(v, z1);
        cplx x = lane_entry<false>(scan_lanes<false>(e, zq, lane), cplx{c.x, c.y}, zq, lane);
#pragma unroll
        for (int i = 0; i < RUN; ++i) {
            x = cmul(z1, cplx{x.r + v[i], x.i});
            const double th = hg[0].theta(i);  // (the frame interval of a run is that of every channel)
#pragma unroll
            for (int j = 0; j < NC; ++j) {
                const cplx H = hg[j].at(th);
                acc[j][i] += am * (H.r * x.i + H.i * x.r);
            }
        }
    }
    const int n = min(TILE, S - t0);
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        if (c0 + j < C) {  // (uniform over the workgroup)
            if (j) __syncthreads();
            join_waves(s_part, acc[j], lane, wave, n, y + ((int64_t)a * C + c0 + j) * S + t0);
        }
    }
}

// 3. workgroup = (tile, clip): gforce[a, j] = sum_m amp Im l_m[j], l driven by wdrive; j < nout = min(F, S)
__global__ void __launch_bounds__(256)
    osc_lis_gforce_kernel(const double* __restrict__ dd, const double* __restrict__ ww, const float* __restrict__ amp,
                          const float* __restrict__ gy, const float* __restrict__ h, int C, int K, int hop, int m, int S,
                          int ntiles, double inv_sr, const double2* __restrict__ lbnd, float* __restrict__ gforce, int F,
                          int nout) {
    __shared__ double s_part[WAVES][PART];
    const int k = blockIdx.x, a = blockIdx.y;
    const int t0 = k * TILE;
    if (t0 >= nout) return;  // (uniform over the workgroup) a tile of taps that get no gradient here
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double inv_hop = 1.0 / (double)hop;
    double acc[RUN];
#pragma unroll
    for (int i = 0; i < RUN; ++i) acc[i] = 0.0;
    for (int mm = wave; mm < m; mm += WAVES) {
        const double d = dd[mm], w = ww[mm];
        const double am = amp ? (double)amp[(int64_t)a * m + mm] : 1.0;
        const cplx z1 = zpow(d, w, inv_sr, 1), zq = zpow(d, w, inv_sr, RUN * (63 - lane));
        const double2 c = lbnd[((int64_t)a * m + mm) * ntiles + k];
        double vr[RUN], vi[RUN];
        load_drive(gy, h, a, mm, C, m, S, K, hop, inv_hop, t0, lane, vr, vi);
        cplx l = lane_entry<true>(scan_lanes<true>(run_from_zero<true>(vr, vi, z1), zq, lane), cplx{c.x, c.y}, zq, lane);
#pragma unroll
        for (int i = RUN - 1; i >= 0; --i) {
            l = cmul(z1, cplx{l.r + vr[i], l.i + vi[i]});
            acc[i] += am * l.i;
        }
    }
    join_waves(s_part, acc, lane, wave, min(TILE, nout - t0), gforce + (int64_t)a * F + t0);
}

// 4. one wavefront per (clip, mode): gamp[a, mm], gpart[a m + mm] = amp sum_t (x[t-1] + f[t]) l[t] and, where asked for,
// gh[a, :, mm, :].  lbnd: the states of l entering every tile (from above), written by the boundary pass on wdrive.
__global__ void __launch_bounds__(64)
    osc_lis_mode_kernel(const float* __restrict__ gy, const double* __restrict__ dd, const double* __restrict__ ww,
                        const float* __restrict__ amp, const float* __restrict__ force, const float* __restrict__ h, int F,
                        int C, int m, int S, int K, int hop, int ntiles, double inv_sr, const double2* __restrict__ lbnd,
                        float* __restrict__ gamp, double2* __restrict__ gpart, float* __restrict__ gh) {
    const int mm = blockIdx.x, a = blockIdx.y, lane = threadIdx.x;
    const int64_t am_at = (int64_t)a * m + mm;
    const mode_powers p = load_mode(dd, ww, amp, am_at, mm, lane, inv_sr);
    const cplx z1 = p.z1;
    const double am = p.am;
    const int nf = min(F, S);
    const int hr = hop / RUN;  // runs per frame
    const double inv_hop = 1.0 / (double)hop;
    const float* frow = force + (int64_t)a * F;
    const double2* lb = lbnd + am_at * ntiles;
    cplx cx = {0.0, 0.0}, G = {0.0, 0.0};
    double ga = 0.0;
    // the frame carries of channel c, re and im part, in lane c (read with a broadcast, written by that lane alone)
    double c0r = 0.0, c1r = 0.0, prev1r = 0.0, last1r = 0.0, c0i = 0.0, c1i = 0.0, prev1i = 0.0, last1i = 0.0;
    for (int k = 0; k < ntiles; ++k) {
        const int t0 = k * TILE;
        double f[RUN], vr[RUN], vi[RUN];
        load_run(frow, t0, lane, nf, f);
        cplx ef = {0.0, 0.0};
        if (t0 < nf) ef = run_from_zero<false>(f, z1);
        cplx x = x_entry(ef, p, lane, cx);
        load_drive(gy, h, a, mm, C, m, S, K, hop, inv_hop, t0, lane, vr, vi);
        cplx l = l_entry(run_from_zero<true>(vr, vi, z1), p, lane, lb[k]);
        cplx u[RUN], xs[RUN];
#pragma unroll
        for (int i = 0; i < RUN; ++i) {
            u[i] = cplx{x.r + f[i], x.i};
            x = cmul(z1, u[i]);
            xs[i] = x;
        }
#pragma unroll
        for (int i = RUN - 1; i >= 0; --i) {
            l = cmul(z1, cplx{l.r + vr[i], l.i + vi[i]});
            const cplx t = cmul(u[i], l);
            G.r += t.r;
            G.i += t.i;
        }
        const frame_pos fp = frame_of(k, lane, hr, K, ntiles);
        for (int cc = 0; cc < C; ++cc) {
            double g[RUN];
            load_run(gy + ((int64_t)a * C + cc) * S, t0, lane, S, g);
            const lane_cgain hg = load_cgain(hrow_of(h, a, cc, mm, C, m, K), K, hop, inv_hop, t0 + lane * RUN);
            double p0r = 0.0, p1r = 0.0, p0i = 0.0, p1i = 0.0;
#pragma unroll
            for (int i = 0; i < RUN; ++i) {
                const double th = hg.theta(i);
                const cplx H = hg.at(th);
                ga += g[i] * (H.r * xs[i].i + H.i * xs[i].r);
                const double gs = g[i] * xs[i].i, gc = g[i] * xs[i].r;
                p0r += (1.0 - th) * gs;
                p1r += th * gs;
                p0i += (1.0 - th) * gc;
                p1i += th * gc;
            }
            if (gh) {  // (wave-uniform)
                double a0 = __shfl(c0r, cc, 64), a1 = __shfl(c1r, cc, 64), ap = __shfl(prev1r, cc, 64), al = 0.0;
                double b0 = __shfl(c0i, cc, 64), b1 = __shfl(c1i, cc, 64), bp = __shfl(prev1i, cc, 64), bl = 0.0;
                const double outr = frame_scan(p0r, p1r, fp, lane, a0, a1, ap, al);
                const double outi = frame_scan(p0i, p1i, fp, lane, b0, b1, bp, bl);
                if (fp.ends) {
                    float2* ghrow = reinterpret_cast<float2*>(gh) + (((int64_t)a * C + cc) * m + mm) * K;
                    ghrow[fp.kq] = make_float2((float)(am * outr), (float)(am * outi));
                }
                if (lane == cc) {
                    c0r = a0, c1r = a1, prev1r = ap, last1r = al;
                    c0i = b0, c1i = b1, prev1i = bp, last1i = bl;
                }
            }
        }
    }
    if (gh) {  // frames past the last tile: the first one hears the th weights of the last tile's last frame, the others nothing
        const int klast = last_frame(ntiles, hr, K);
        for (int cc = 0; cc < C; ++cc) {
            float2* ghrow = reinterpret_cast<float2*>(gh) + (((int64_t)a * C + cc) * m + mm) * K;
            const double lr = __shfl(last1r, cc, 64), li = __shfl(last1i, cc, 64);
            if (lane == 0 && klast + 1 < K) ghrow[klast + 1] = make_float2((float)(am * lr), (float)(am * li));
            for (int kz = klast + 2 + lane; kz < K; kz += 64) ghrow[kz] = make_float2(0.f, 0.f);
        }
    }
    store_mode(ga, G, am, lane, am_at, gamp, gpart);
}

// The checks both entry points make before those of their own operands' alignment, in osc_slide.hip's order; `fn` names the
// entry point
int check_args(const char* fn, bool pointers, int A, int C, int m, int F, int S, int K, int hop, double sr, const void* work,
               int64_t work_bytes) {
    DS_REQUIRE(pointers, "%s: null pointer", fn);
    DS_REQUIRE(A > 0 && C > 0 && m > 0 && S > 0 && F > 0 && K > 0, "%s: empty problem (A %d, C %d, m %d, F %d, S %d, K %d)", fn, A,
               C, m, F, S, K);
    if (int rc = osc_bank::check_clips(fn, A)) return rc;
    DS_REQUIRE(C <= DS_OSC_LISTEN_MAX_CHANNELS, "%s: C = %d above %d channels", fn, C, DS_OSC_LISTEN_MAX_CHANNELS);
    if (int rc = osc_bank::check_frames(fn, hop, sr)) return rc;
    return osc_bank::check_work(fn, work, work_bytes, ds_osc_listen_workspace_bytes(A, C, m, S, K, hop));
}

template <int NC>
void launch_tile(hipStream_t st, const double* d, const double* w, const float* amp, const float* force, int F, int nin,
                 const float* h, int A, int C, int K, int hop, int m, int nt, double inv_sr, const double2* bnd, float* y, int S) {
    osc_lis_tile_kernel<NC><<<dim3((unsigned)nt, (unsigned)A, (unsigned)ds::ceil_div(C, NC)), 256, 0, st>>>(
        d, w, amp, force, F, nin, h, C, K, hop, m, nt, inv_sr, bnd, y, S);
}

}  // namespace

extern "C" int64_t ds_osc_listen_workspace_bytes(int A, int C, int m, int S, int K, int hop) {
    if (A <= 0 || C <= 0 || C > DS_OSC_LISTEN_MAX_CHANNELS || m <= 0 || S <= 0 || K <= 0 || hop <= 0 ||
        hop % DS_OSC_SCAN_RUN != 0)
        return 0;
    return osc_bank::workspace_bytes(A, m, S);
}

extern "C" int ds_osc_listen_fwd(const double* d, const double* w, const float* amp, const float* force, const float* h, int A,
                                 int C, int m, int F, int S, int K, int hop, double sr, void* work, int64_t work_bytes, float* y,
                                 ds_stream_t stream) {
    if (int rc = check_args("ds_osc_listen_fwd", d && w && force && h && work && y, A, C, m, F, S, K, hop, sr, work, work_bytes))
        return rc;
    DS_REQUIRE(aligned(d, 8) && aligned(w, 8) && aligned(force, 4) && aligned(h, 8) && aligned(y, 4) && aligned(amp, 4),
               "ds_osc_listen_fwd: misaligned operand");
    hipStream_t st = ds::as_stream(stream);
    const int nt = (int)ntiles_of(S);
    const int nin = std::min(F, S);
    double2* bnd = static_cast<double2*>(work);
    const double inv_sr = 1.0 / sr;
    if (int rc = osc_bank::launch_boundary(st, false, d, w, force, F, nin, A, m, nt, inv_sr, bnd)) return rc;
    if (C == 1)
        launch_tile<1>(st, d, w, amp, force, F, nin, h, A, C, K, hop, m, nt, inv_sr, bnd, y, S);
    else if (C == 2)
        launch_tile<2>(st, d, w, amp, force, F, nin, h, A, C, K, hop, m, nt, inv_sr, bnd, y, S);
    else
        launch_tile<4>(st, d, w, amp, force, F, nin, h, A, C, K, hop, m, nt, inv_sr, bnd, y, S);
    return DS_LAUNCHED("osc_lis_tile_kernel");
}

extern "C" int ds_osc_listen_bwd(const float* gy, const double* d, const double* w, const float* amp, const float* force,
                                 const float* h, int A, int C, int m, int F, int S, int K, int hop, double sr, void* work,
                                 int64_t work_bytes, double* gd, double* gw, float* gamp, float* gforce, float* gh,
                                 ds_stream_t stream) {
    if (int rc = check_args("ds_osc_listen_bwd", gy && d && w && force && h && work && gd && gw, A, C, m, F, S, K, hop, sr, work,
                            work_bytes))
        return rc;
    DS_REQUIRE((amp == nullptr) == (gamp == nullptr), "ds_osc_listen_bwd: gamp goes with amp (both or neither)");
    DS_REQUIRE(aligned(gd, 8) && aligned(gw, 8), "ds_osc_listen_bwd: gd or gw not 8-byte aligned");
    DS_REQUIRE(aligned(d, 8) && aligned(w, 8) && aligned(force, 4) && aligned(h, 8) && aligned(gy, 4) && aligned(amp, 4) &&
                   aligned(gamp, 4) && aligned(gforce, 4) && aligned(gh, 8),
               "ds_osc_listen_bwd: misaligned operand");
    hipStream_t st = ds::as_stream(stream);
    const double inv_sr = 1.0 / sr;
    return osc_bank::backward(
        st, A, m, F, S, inv_sr, work, gd, gw, gforce,
        [&](int nt, double2* lbnd) {
            osc_lis_boundary_kernel<<<dim3((unsigned)m, (unsigned)A), 64, 0, st>>>(d, w, gy, h, C, K, hop, m, S, nt, inv_sr, lbnd);
            return DS_LAUNCHED("osc_lis_boundary_kernel");
        },
        [&](int nt, const double2* lbnd) {
            osc_lis_gforce_kernel<<<dim3((unsigned)nt, (unsigned)A), 256, 0, st>>>(d, w, amp, gy, h, C, K, hop, m, S, nt, inv_sr,
                                                                                  lbnd, gforce, F, std::min(F, S));
            return DS_LAUNCHED("osc_lis_gforce_kernel");
        },
        [&](int nt, const double2* lbnd, double2* gpart) {
            osc_lis_mode_kernel<<<dim3((unsigned)m, (unsigned)A), 64, 0, st>>>(gy, d, w, amp, force, h, F, C, m, S, K, hop, nt,
                                                                             inv_sr, lbnd, gamp, gpart, gh);
            return DS_LAUNCHED("osc_lis_mode_kernel");
        });
}
