// The lane scan of the recursive-resonator banks (osc_driven.hip, osc_slide.hip, osc_listen.hip): a wavefront lane owns RUN consecutive
// samples of x[t] = z (x[t-1] + v[t]), a tile is the 64 RUN samples of one wavefront, and a 6-step shuffle scan with the
// closed-form powers z^(RUN 2^k) joins the lanes.  Every power z^n is exp / sincos of n d / sr and n w / sr, never a product
// of rounded powers.  fp64 throughout.
#pragma once

#include "ds_common.h"

namespace osc_scan {

constexpr int RUN = DS_OSC_SCAN_RUN;  // samples per lane (the unit of the sliding bank's hop, include/diffsound_hip.h)
constexpr int TILE = 64 * RUN;        // samples per wavefront pass (tests/_osc_driven_ref.py mirrors both)
constexpr int WAVES = 4;              // waves of a tile-pass workgroup, each looping over its modes
constexpr int PART = 64 * (RUN + 1);  // a wave's partial sums of a tile: a lane's RUN sums padded to RUN + 1 (no bank conflicts)
static_assert(sizeof(double) * WAVES * PART == 34816, "the tile passes' LDS: __shared__ double s_part[WAVES][PART]");

struct cplx {
    double r, i;
};

__device__ __forceinline__ cplx cmul(cplx a, cplx b) { return {a.r * b.r - a.i * b.i, a.r * b.i + a.i * b.r}; }

// z^n in closed form
__device__ __forceinline__ cplx zpow(double d, double w, double inv_sr, int n) {
    const double tau = (double)n * inv_sr;
    double s, c;
    sincos(w * tau, &s, &c);
    const double e = exp(-d * tau);
    return {e * c, e * s};
}

// REV = false: time runs up (x), lane q = lane follows lane q - 1.  REV = true: time runs down (l), the lane order is reversed.
template <bool REV>
__device__ __forceinline__ double from_prev(double v, int o) {
    return REV ? __shfl_down(v, o, 64) : __shfl_up(v, o, 64);
}

// the lane's samples of one row: v[i] = row[t0 + lane RUN + i] where that index is below n, else 0
__device__ __forceinline__ void load_run(const float* __restrict__ row, int t0, int lane, int n, double* v) {
#pragma unroll
    for (int i = 0; i < RUN; ++i) {
        const int t = t0 + lane * RUN + i;
        v[i] = t < n ? (double)row[t] : 0.0;
    }
}

// the state after the lane's samples, started from zero
template <bool REV>
__device__ __forceinline__ cplx run_from_zero(const double* v, cplx z1) {
    cplx x = {0.0, 0.0};
#pragma unroll
    for (int ii = 0; ii < RUN; ++ii) {
        const int i = REV ? RUN - 1 - ii : ii;
        x = cmul(z1, cplx{x.r + v[i], x.i});
    }
    return x;
}

// the same under a complex input vr + i vi (the adjoint of the listener bank, osc_listen.hip)
template <bool REV>
__device__ __forceinline__ cplx run_from_zero(const double* vr, const double* vi, cplx z1) {
    cplx x = {0.0, 0.0};
#pragma unroll
    for (int ii = 0; ii < RUN; ++ii) {
        const int i = REV ? RUN - 1 - ii : ii;
        x = cmul(z1, cplx{x.r + vr[i], x.i + vi[i]});
    }
    return x;
}

// inclusive scan over the lanes of the from-zero end states: v_q = sum_{p <= q} z^(RUN (q - p)) e_p.  zq = z^(RUN q) of
// this lane, so the power of step o is read from the lane with q = o.
template <bool REV>
__device__ __forceinline__ cplx scan_lanes(cplx e, cplx zq, int lane) {
    const int q = REV ? 63 - lane : lane;
    cplx v = e;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int src = REV ? 63 - o : o;
        const cplx p = {__shfl(zq.r, src, 64), __shfl(zq.i, src, 64)};
        const cplx u = {from_prev<REV>(v.r, o), from_prev<REV>(v.i, o)};
        if (q >= o) {
            const cplx t = cmul(p, u);
            v.r += t.r;
            v.i += t.i;
        }
    }
    return v;
}

// the state entering this lane's samples: the scan of the lane before it plus the tile's entering state moved RUN q samples
template <bool REV>
__device__ __forceinline__ cplx lane_entry(cplx v, cplx carry, cplx zq, int lane) {
    const int q = REV ? 63 - lane : lane;
    cplx ex = {from_prev<REV>(v.r, 1), from_prev<REV>(v.i, 1)};
    if (q == 0) ex = {0.0, 0.0};
    const cplx c = cmul(zq, carry);
    return {ex.r + c.r, ex.i + c.i};
}

// the state leaving the tile
template <bool REV>
__device__ __forceinline__ cplx tile_exit(cplx v, cplx carry, cplx zT) {
    const int last = REV ? 0 : 63;
    const cplx c = cmul(zT, carry);
    return {__shfl(v.r, last, 64) + c.r, __shfl(v.i, last, 64) + c.i};
}

// the four waves' partial sums of a tile joined in the order (0 + 1) + (2 + 3) and stored: n samples from out
__device__ __forceinline__ void join_waves(double (*s_part)[PART], const double* acc, int lane, int wave, int n,
                                           float* __restrict__ out) {
#pragma unroll
    for (int i = 0; i < RUN; ++i) s_part[wave][lane * (RUN + 1) + i] = acc[i];
    __syncthreads();
    for (int j = threadIdx.x; j < n; j += blockDim.x) {
        const int o = (j / RUN) * (RUN + 1) + (j % RUN);
        out[j] = (float)((s_part[0][o] + s_part[1][o]) + (s_part[2][o] + s_part[3][o]));
    }
}

// The mode pass (backward), one wavefront per (clip, mode): x up and l down through the tiles, G = sum_t (x[t-1] + in[t]) l[t].
// What every tile needs of the mode: its amplitude and the powers of z.
struct mode_powers {
    double am;
    cplx z1, zT, zq_up, zq_dn;  // z, z^TILE, z^(RUN lane), z^(RUN (63 - lane))
};

__device__ __forceinline__ mode_powers load_mode(const double* __restrict__ dd, const double* __restrict__ ww,
                                                 const float* __restrict__ amp, int64_t am_at, int mm, int lane, double inv_sr) {
    const double d = dd[mm], w = ww[mm];
    mode_powers p;
    p.am = amp ? (double)amp[am_at] : 1.0;
    p.z1 = zpow(d, w, inv_sr, 1);
    p.zT = zpow(d, w, inv_sr, TILE);
    p.zq_up = zpow(d, w, inv_sr, RUN * lane);
    p.zq_dn = zpow(d, w, inv_sr, RUN * (63 - lane));
    return p;
}

// x entering the lane's run of this tile, from the lanes' from-zero end states ef; cx, the state entering the tile, moves on
__device__ __forceinline__ cplx x_entry(cplx ef, const mode_powers& p, int lane, cplx& cx) {
    const cplx sf = scan_lanes<false>(ef, p.zq_up, lane);
    const cplx x = lane_entry<false>(sf, cx, p.zq_up, lane);
    cx = tile_exit<false>(sf, cx, p.zT);
    return x;
}

// l entering the lane's run from above: el as ef, c the tile's entering state as the downward boundary pass left it
__device__ __forceinline__ cplx l_entry(cplx el, const mode_powers& p, int lane, double2 c) {
    return lane_entry<true>(scan_lanes<true>(el, p.zq_dn, lane), cplx{c.x, c.y}, p.zq_dn, lane);
}

// the lanes' sums joined: gamp[at] = sum_t gy Im x (where asked for) and gpart[at] = amp G
__device__ __forceinline__ void store_mode(double ga, cplx G, double am, int lane, int64_t at, float* __restrict__ gamp,
                                           double2* __restrict__ gpart) {
    ga = ds::wave_sum(ga);
    G.r = ds::wave_sum(G.r);
    G.i = ds::wave_sum(G.i);
    if (lane == 0) {
        if (gamp) gamp[at] = (float)ga;
        gpart[at] = make_double2(am * G.r, am * G.i);
    }
}

// Gains at control frames hop samples apart, piecewise linear in between, the last frame held (osc_slide.hip: input gains;
// osc_listen.hip: complex output gains).  hop is a multiple of RUN, so a lane's run lies inside ONE frame interval.
// the two gains of a lane's run (one frame interval) and what turns a sample of the run into its interpolation weight
struct lane_gain {
    double g0, g1;  // gain[k], gain[min(k + 1, K - 1)]
    double sc;      // 1 / hop, 0 where the last frame is held
    int off;        // the run's first sample - k hop

    __device__ __forceinline__ double theta(int i) const { return (double)(off + i) * sc; }
    __device__ __forceinline__ double at(int i) const {
        const double th = theta(i);
        return (1.0 - th) * g0 + th * g1;
    }
};

// tl: the first sample of the lane's run (a multiple of RUN); grow: the K gains of this (clip, mode)
__device__ __forceinline__ lane_gain load_gain(const float* __restrict__ grow, int K, int hop, double inv_hop, int tl) {
    const int kk = tl / hop;
    const bool held = kk >= K - 1;
    const int k = held ? K - 1 : kk;
    lane_gain g;
    g.g0 = (double)grow[k];
    g.g1 = (double)grow[held ? K - 1 : k + 1];
    g.sc = held ? 0.0 : inv_hop;
    g.off = tl - k * hop;
    return g;
}

// the complex form: the K frames of one (clip, channel, mode) as (re, im) pairs
struct lane_cgain {
    double g0r, g0i, g1r, g1i;
    double sc;
    int off;

    __device__ __forceinline__ double theta(int i) const { return (double)(off + i) * sc; }
    __device__ __forceinline__ cplx at(double th) const {
        return {(1.0 - th) * g0r + th * g1r, (1.0 - th) * g0i + th * g1i};
    }
};

__device__ __forceinline__ lane_cgain load_cgain(const float2* __restrict__ hrow, int K, int hop, double inv_hop, int tl) {
    const int kk = tl / hop;
    const bool held = kk >= K - 1;
    const int k = held ? K - 1 : kk;
    const float2 a = hrow[k], b = hrow[held ? K - 1 : k + 1];
    lane_cgain g;
    g.g0r = (double)a.x;
    g.g0i = (double)a.y;
    g.g1r = (double)b.x;
    g.g1i = (double)b.y;
    g.sc = held ? 0.0 : inv_hop;
    g.off = tl - k * hop;
    return g;
}

// where the lanes of a tile stand among the frames: lane q of tile k holds run k 64 + q, which lies in frame
// kq = min(run / h, K - 1), h = hop / RUN runs per frame
struct frame_pos {
    int kq, kn;      // the frame of this lane's run and of the next lane's
    int s, s0;       // the lane of this tile at which frame kq starts (<= 0: in an earlier tile), and max(s, 0)
    int k63, kn63;   // kq, kn of lane 63
    bool ends;       // the frame changes after this lane, or this is the last lane of the last tile: the lane stores frame kq
};

__device__ __forceinline__ frame_pos frame_of(int k, int lane, int h, int K, int ntiles) {
    frame_pos fp;
    const int run = k * 64 + lane;
    fp.kq = min(run / h, K - 1);
    fp.kn = min((run + 1) / h, K - 1);
    fp.s = fp.kq * h - k * 64;
    fp.s0 = max(fp.s, 0);
    fp.k63 = __shfl(fp.kq, 63, 64);
    fp.kn63 = __shfl(fp.kn, 63, 64);
    fp.ends = fp.kn != fp.kq || (k == ntiles - 1 && lane == 63);
    return fp;
}

// The gradient of the frames' gains.  p0, p1 = the (1 - th) and th weighted sums of a lane's run, belonging to frames kq and
// kq + 1 (p1 = 0 where the last frame is held).  P0[k], P1[k] = the sums over the runs of frame k: a shuffle scan cut at the
// frames' first lanes adds them inside the tile in a fixed order.  Returns P0[kq] + P1[kq - 1] as far as this lane sees them -
// the frame's value in the lane after which the frame changes.  (c0, c1): the frame that is open at the tile's end; prev1: P1
// of the frame before the open one; last1: P1 so far of the frame of the last lane.  All four wave-uniform.
__device__ __forceinline__ double frame_scan(double p0, double p1, const frame_pos& fp, int lane, double& c0, double& c1,
                                             double& prev1, double& last1) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double u0 = __shfl_up(p0, o, 64), u1 = __shfl_up(p1, o, 64);
        if (lane - o >= fp.s0) {
            p0 += u0;
            p1 += u1;
        }
    }
    if (fp.s <= 0) {
        p0 += c0;
        p1 += c1;
    }
    const double pl = __shfl(p1, max(fp.s - 1, 0), 64);  // the last lane of frame kq - 1, where it is in this tile
    const double before = fp.s > 0 ? pl : prev1;
    const double e0 = __shfl(p0, 63, 64), e1 = __shfl(p1, 63, 64), b63 = __shfl(before, 63, 64);
    last1 = e1;
    if (fp.kn63 == fp.k63) {
        c0 = e0;
        c1 = e1;
        prev1 = b63;
    } else {
        c0 = c1 = 0.0;
        prev1 = e1;
    }
    return p0 + before;
}

// the frame of the last tile's last run; the frames past it are closed after the walk (klast + 1 gets last1, the others 0)
__device__ __forceinline__ int last_frame(int ntiles, int h, int K) { return min((ntiles * 64 - 1) / h, K - 1); }

}  // namespace osc_scan
