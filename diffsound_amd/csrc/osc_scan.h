// The lane scan of the recursive-resonator banks (osc_driven.hip, osc_slide.hip): a wavefront lane owns RUN consecutive
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

}  // namespace osc_scan
