// The lane scan of the recursive-resonator banks (osc_driven.hip, osc_slide.hip, osc_listen.hip): a wavefront lane owns RUN consecutive
// samples of x[t] = z (x[t-1] + v[t]), a tile is the 64 RUN samples of one wavefront, and a 6-step shuffle scan with the
// closed-form powers z^(RUN 2^k) joins the lanes.  Every power z^n is exp / sincos of n d / sr and n w / sr, never a product
// of rounded powers.  fp64 throughout.
#pragma once

#include "ds_common.h"

namespace osc_scan {

constexpr int RUN = DS_OSC_SCAN_RUN;  // samples per lane (the unit of the sliding bank's hop, include/diffsound_hip.h)
constexpr int TILE = 64 * RUN;        // samples per wavefront pass

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

}  // namespace osc_scan
