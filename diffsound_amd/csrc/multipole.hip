// Radiated sound at a listener: the multipole series of each mode's exterior field, with gradients - gfx950.
//
// Outside a sphere around the object the pressure of mode j (wave number k_j, convention e^{-i w t}, G = e^{ikr} / (4 pi r) as
// in bem.hip) is a series of outgoing waves about the centre x0:
//     p_j(x) = sum_{l=0..L} sum_{n=-l..l} c_j[l^2 + l + n] h_l(k_j r) Y_{l,n}(u),   d = x - x0, r = |d|, u = d / r,
// h_l the spherical Hankel function of the first kind, Y_{l,n} the real orthonormal harmonics (n > 0: sqrt2 (-1)^n Re Y_l^n,
// n < 0: sqrt2 (-1)^n Im Y_l^|n|, Y_l^n with the Condon-Shortley phase, i.e. sqrt2 K_l^|n| P_l^|n|(cos th) cos / sin(|n| ph)
// with the phase-free P).  The reference has no counterpart.
//
// Cartesian evaluation, no angles: the regular solid harmonics R_{l,n}(x, y, z) = r^l Y_{l,n} are polynomials,
//     R_{l,+-m} = Q_l^m(z, r2) {C_m, S_m},   C_m + i S_m = (x + i y)^m,   r2 = x^2 + y^2 + z^2,
//     Q_m^m = D_m = sqrt(1 / 4 pi) prod_{i<=m} sqrt((2 i + 1) / (2 i)) (times sqrt2 for m > 0),
//     Q_l^m = a_l^m (z Q_{l-1}^m - b_l^m r2 Q_{l-2}^m),  a = sqrt((4 l^2 - 1) / (l^2 - m^2)),  b = sqrt(((l-1)^2 - m^2) / (4 (l-1)^2 - 1)),
// and their gradient is the derivative of these recurrences, carried along (dQ/dz, dQ/dr2; d(C_m + i S_m) = m (x + i y)^(m-1)
// (dx + i dy)).  They are evaluated at the unit vector u: R_l(d) = r^l R_l(u) and grad R_l(d) = r^(l-1) (grad R_l)(u) exactly, so
// with d/dr [h_l(kr) r^-l] = -k h_(l+1)(kr) r^-l
//     grad [h_l(kr) Y_{l,n}] = -k h_(l+1)(kr) R_{l,n}(u) u + (h_l(kr) / r) (grad R_{l,n})(u):
// no power of r, nothing that overflows, and a point on the z axis is an ordinary point.
// h_l: upward from h_0 = -i e^{iz} / z, h_1 = h_0 (1 / z - i) with h_(l+1) = (2 l + 1) / z h_l - h_(l-1); its error stays small
// relative to |h_l| on both sides of l = z (the dominant solution for l > z is the one computed).
//
// Layout: coef and gcoef are (N, m) complex, N = (L + 1)^2, interleaved (re, im), the modes contiguous: lane j owns mode j and
// the reads of a row are coalesced.  out, gout: (P, m) complex.  k (m), pts (P, 3), center (3): fp64 on the device.
// Mapping: one wavefront per point.  Lane mu <= L runs the recurrence of order mu over l = mu .. L and leaves Y (and the three
// derivatives) of the point in LDS; after the barrier lane j runs its own h_l(k_j r) recurrence over the columns j, j + 64, ...
// and reads the harmonics as broadcasts.
//   fwd    out[p, j] = sum_l h_l (sum_n c Y)                                                 (inner sums ascending in n, then l)
//   gpts   gpts[p] = sum_j Re(conj(gout) grad p_j): per lane, then ds::wave_sum, lane 0 stores
//   gcoef  gcoef[e, j] = sum_p gout[p, j] conj(h_l(k_j r_p)) Y_e(u_p): G = min(P, DS_MULTIPOLE_GCOEF_BLOCKS) workgroups, workgroup
//          b adds its points b, b + G, ... in ascending order into its own (N, m) slab of the workspace (the first point stores),
//          a closing kernel adds the slabs in ascending order.
// No atomics; every output element and every workspace element has one owner and is written in a fixed order: two calls give
// the same bits.  Multiply-adds are NOT fused in this unit: tests/_multipole_ref.py restates it operation by operation.
#include <cmath>
#include <cstdint>

#include "ds_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int MAXN = (DS_MULTIPOLE_MAX_ORDER + 1) * (DS_MULTIPOLE_MAX_ORDER + 1);

struct Geo {
    double ux, uy, uz, r, inv;
};

__device__ __forceinline__ Geo geometry(const double* __restrict__ pts, const double* __restrict__ center, int64_t p) {
    const double dx = pts[3 * p] - center[0], dy = pts[3 * p + 1] - center[1], dz = pts[3 * p + 2] - center[2];
    Geo g;
    g.r = sqrt(dx * dx + dy * dy + dz * dz);
    g.inv = 1.0 / g.r;
    g.ux = dx * g.inv;
    g.uy = dy * g.inv;
    g.uz = dz * g.inv;
    return g;
}

// Lane mu <= L: R_{l,+-mu}(x, y, z) for l = mu .. L into sY[l^2 + l +- mu], and with DERIV their gradient into sDx, sDy, sDz.
template <bool DERIV>
__device__ __forceinline__ void harmonics(double x, double y, double z, int L, int lane, double* sY, double* sDx, double* sDy,
                                          double* sDz) {
    if (lane > L) return;
    const int m = lane;
    double c = 1.0, s = 0.0, cp = 0.0, sp = 0.0, D = 0.28209479177387814;  // sqrt(1 / (4 pi))
    for (int i = 1; i <= m; ++i) {
        cp = c;
        sp = s;
        c = cp * x - sp * y;
        s = cp * y + sp * x;
        D = D * sqrt((double)(2 * i + 1) / (double)(2 * i));
    }
    if (m > 0) D = D * 1.4142135623730951;
    const double r2 = x * x + y * y + z * z, fm = (double)m;
    double Q1 = 0.0, Q2 = 0.0, Qz1 = 0.0, Qz2 = 0.0, Qr1 = 0.0, Qr2 = 0.0;
    for (int l = m; l <= L; ++l) {
        double Q = D, Qz = 0.0, Qr = 0.0;
        if (l > m) {
            const double a = sqrt((double)(4 * l * l - 1) / (double)(l * l - m * m));
            const double b = sqrt((double)((l - 1) * (l - 1) - m * m) / (double)(4 * (l - 1) * (l - 1) - 1));
            const double br2 = b * r2;
            Q = a * (z * Q1 - br2 * Q2);
            if (DERIV) {
                Qz = a * ((Q1 + z * Qz1) - br2 * Qz2);
                Qr = a * (z * Qr1 - b * (Q2 + r2 * Qr2));
            }
        }
        const int e = l * l + l;
        sY[e + m] = Q * c;
        if (m > 0) sY[e - m] = Q * s;
        if (DERIV) {
            const double t = Qz + (2.0 * z) * Qr, qx = (2.0 * x) * Qr, qy = (2.0 * y) * Qr, mq = fm * Q;
            sDx[e + m] = qx * c + mq * cp;
            sDy[e + m] = qy * c - mq * sp;
            sDz[e + m] = t * c;
            if (m > 0) {
                sDx[e - m] = qx * s + mq * sp;
                sDy[e - m] = qy * s + mq * cp;
                sDz[e - m] = t * s;
            }
        }
        Q2 = Q1;
        Q1 = Q;
        Qz2 = Qz1;
        Qz1 = Qz;
        Qr2 = Qr1;
        Qr1 = Qr;
    }
}

// h_0, h_1 of z = k r and 1 / z
struct Hankel {
    double r0, i0, r1, i1, iz;
};

__device__ __forceinline__ Hankel hankel_start(double k, double r) {
    const double z = k * r;
    double sn, cs;
    sincos(z, &sn, &cs);
    Hankel h;
    h.iz = 1.0 / z;
    h.r0 = sn * h.iz;
    h.i0 = 0.0 - cs * h.iz;
    h.r1 = h.r0 * h.iz + h.i0;
    h.i1 = h.i0 * h.iz - h.r0;
    return h;
}

// (cur, nxt) = (h_l, h_(l+1)) -> (h_(l+1), h_(l+2))
__device__ __forceinline__ void hankel_step(Hankel& h, int l) {
    const double f = (double)(2 * l + 3) * h.iz;
    const double tr = f * h.r1 - h.r0, ti = f * h.i1 - h.i0;
    h.r0 = h.r1;
    h.i0 = h.i1;
    h.r1 = tr;
    h.i1 = ti;
}

__global__ void __launch_bounds__(64)
    multipole_fwd_kernel(const double* __restrict__ pts, const double* __restrict__ center, const double* __restrict__ k,
                         const double2* __restrict__ coef, int m, int L, double2* __restrict__ out) {
    __shared__ double sY[MAXN];
    const int64_t p = blockIdx.x;
    const int lane = threadIdx.x;
    const Geo g = geometry(pts, center, p);
    harmonics<false>(g.ux, g.uy, g.uz, L, lane, sY, nullptr, nullptr, nullptr);
    __syncthreads();
    for (int j = lane; j < m; j += 64) {
        Hankel h = hankel_start(k[j], g.r);
        double pr = 0.0, pi = 0.0;
        for (int l = 0; l <= L; ++l) {
            double sr = 0.0, si = 0.0;
            for (int e = l * l; e <= l * l + 2 * l; ++e) {
                const double2 c = coef[(int64_t)e * m + j];
                const double Y = sY[e];
                sr += c.x * Y;
                si += c.y * Y;
            }
            pr += h.r0 * sr - h.i0 * si;
            pi += h.r0 * si + h.i0 * sr;
            hankel_step(h, l);
        }
        out[p * m + j] = make_double2(pr, pi);
    }
}

__global__ void __launch_bounds__(64)
    multipole_gpts_kernel(const double* __restrict__ pts, const double* __restrict__ center, const double* __restrict__ k,
                          const double2* __restrict__ coef, const double2* __restrict__ gout, int m, int L,
                          double* __restrict__ gpts) {
    __shared__ double sY[MAXN], sDx[MAXN], sDy[MAXN], sDz[MAXN];
    const int64_t p = blockIdx.x;
    const int lane = threadIdx.x;
    const Geo g = geometry(pts, center, p);
    harmonics<true>(g.ux, g.uy, g.uz, L, lane, sY, sDx, sDy, sDz);
    __syncthreads();
    double ax = 0.0, ay = 0.0, az = 0.0;
    for (int j = lane; j < m; j += 64) {
        const double kj = k[j];
        Hankel h = hankel_start(kj, g.r);
        const double2 go = gout[p * m + j];
        double E = 0.0, Fx = 0.0, Fy = 0.0, Fz = 0.0;
        for (int l = 0; l <= L; ++l) {
            double sr = 0.0, si = 0.0, xr = 0.0, xi = 0.0, yr = 0.0, yi = 0.0, zr = 0.0, zi = 0.0;
            for (int e = l * l; e <= l * l + 2 * l; ++e) {
                const double2 c = coef[(int64_t)e * m + j];
                const double Y = sY[e], X1 = sDx[e], Y1 = sDy[e], Z1 = sDz[e];
                sr += c.x * Y;
                si += c.y * Y;
                xr += c.x * X1;
                xi += c.y * X1;
                yr += c.x * Y1;
                yi += c.y * Y1;
                zr += c.x * Z1;
                zi += c.y * Z1;
            }
            // w = conj(gout) h_l, w1 = conj(gout) h_(l+1)
            const double wr = go.x * h.r0 + go.y * h.i0, wi = go.x * h.i0 - go.y * h.r0;
            const double w1r = go.x * h.r1 + go.y * h.i1, w1i = go.x * h.i1 - go.y * h.r1;
            E += w1r * sr - w1i * si;
            Fx += wr * xr - wi * xi;
            Fy += wr * yr - wi * yi;
            Fz += wr * zr - wi * zi;
            hankel_step(h, l);
        }
        const double kE = kj * E;
        ax += g.inv * Fx - g.ux * kE;
        ay += g.inv * Fy - g.uy * kE;
        az += g.inv * Fz - g.uz * kE;
    }
    ax = ds::wave_sum(ax);
    ay = ds::wave_sum(ay);
    az = ds::wave_sum(az);
    if (lane == 0) {
        gpts[3 * p] = ax;
        gpts[3 * p + 1] = ay;
        gpts[3 * p + 2] = az;
    }
}

// slab b of part ((G, N, m) complex) = the sum over the points b, b + G, ... of gout conj(h_l) Y
__global__ void __launch_bounds__(64)
    multipole_gcoef_kernel(const double* __restrict__ pts, const double* __restrict__ center, const double* __restrict__ k,
                           const double2* __restrict__ gout, int64_t P, int m, int L, double2* __restrict__ part) {
    __shared__ double sY[MAXN];
    const int lane = threadIdx.x;
    const int64_t G = gridDim.x;
    double2* slab = part + (int64_t)blockIdx.x * (L + 1) * (L + 1) * m;
    for (int64_t p = blockIdx.x; p < P; p += G) {
        const bool first = p == blockIdx.x;  // (wave-uniform)
        const Geo g = geometry(pts, center, p);
        harmonics<false>(g.ux, g.uy, g.uz, L, lane, sY, nullptr, nullptr, nullptr);
        __syncthreads();
        for (int j = lane; j < m; j += 64) {
            Hankel h = hankel_start(k[j], g.r);
            const double2 go = gout[p * m + j];
            for (int l = 0; l <= L; ++l) {
                // w = gout conj(h_l)
                const double wr = go.x * h.r0 + go.y * h.i0, wi = go.y * h.r0 - go.x * h.i0;
                for (int e = l * l; e <= l * l + 2 * l; ++e) {
                    const double Y = sY[e];
                    double2 v = make_double2(wr * Y, wi * Y);
                    if (!first) {
                        const double2 o = slab[(int64_t)e * m + j];
                        v.x = o.x + v.x;
                        v.y = o.y + v.y;
                    }
                    slab[(int64_t)e * m + j] = v;
                }
                hankel_step(h, l);
            }
        }
        __syncthreads();  // the next point's harmonics overwrite sY
    }
}

__global__ void multipole_reduce_kernel(const double2* __restrict__ part, int G, int64_t n, double2* __restrict__ gcoef) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double sr = 0.0, si = 0.0;
    for (int b = 0; b < G; ++b) {
        const double2 v = part[(int64_t)b * n + i];
        sr += v.x;
        si += v.y;
    }
    gcoef[i] = make_double2(sr, si);
}

inline bool shape_ok(int64_t P, int m, int L) {
    return P >= 1 && P <= DS_MULTIPOLE_MAX_POINTS && m >= 1 && m <= DS_MULTIPOLE_MAX_MODES && L >= 0 && L <= DS_MULTIPOLE_MAX_ORDER;
}

int check_args(const char* fn, bool pointers, int64_t P, int m, int L) {
    DS_REQUIRE(pointers, "%s: null pointer", fn);
    DS_REQUIRE(P >= 1 && P <= DS_MULTIPOLE_MAX_POINTS, "%s: P = %lld outside 1..%d", fn, (long long)P, DS_MULTIPOLE_MAX_POINTS);
    DS_REQUIRE(m >= 1 && m <= DS_MULTIPOLE_MAX_MODES, "%s: m = %d outside 1..%d", fn, m, DS_MULTIPOLE_MAX_MODES);
    DS_REQUIRE(L >= 0 && L <= DS_MULTIPOLE_MAX_ORDER, "%s: L = %d outside 0..%d", fn, L, DS_MULTIPOLE_MAX_ORDER);
    return DS_OK;
}

using ds::aligned;

inline int64_t slabs(int64_t P) { return P < DS_MULTIPOLE_GCOEF_BLOCKS ? P : DS_MULTIPOLE_GCOEF_BLOCKS; }

}  // namespace

extern "C" int64_t ds_multipole_workspace_bytes(int64_t P, int m, int L) {
    if (!shape_ok(P, m, L)) return 0;
    return (int64_t)sizeof(double2) * slabs(P) * (L + 1) * (L + 1) * m;
}

extern "C" int ds_multipole_fwd(const double* pts, const double* center, const double* k, const double* coef, int64_t P, int m,
                                int L, double* out, ds_stream_t stream) {
    if (int rc = check_args("ds_multipole_fwd", pts && center && k && coef && out, P, m, L)) return rc;
    DS_REQUIRE(aligned(pts, 8) && aligned(center, 8) && aligned(k, 8) && aligned(coef, 16) && aligned(out, 16),
               "ds_multipole_fwd: misaligned operand");
    multipole_fwd_kernel<<<(unsigned)P, 64, 0, ds::as_stream(stream)>>>(pts, center, k, reinterpret_cast<const double2*>(coef), m,
                                                                         L, reinterpret_cast<double2*>(out));
    DS_LAUNCH_CHECK("multipole_fwd_kernel");
    return DS_OK;
}

extern "C" int ds_multipole_bwd(const double* gout, const double* pts, const double* center, const double* k, const double* coef,
                                int64_t P, int m, int L, void* work, int64_t work_bytes, double* gpts, double* gcoef,
                                ds_stream_t stream) {
    if (int rc = check_args("ds_multipole_bwd", gout && pts && center && k && coef, P, m, L)) return rc;
    DS_REQUIRE(gpts || gcoef, "ds_multipole_bwd: gpts and gcoef are both null");
    if (gcoef) {
        DS_REQUIRE(work, "ds_multipole_bwd: null pointer (gcoef needs the workspace)");
        DS_REQUIRE(work_bytes >= ds_multipole_workspace_bytes(P, m, L), "ds_multipole_bwd: workspace of %lld bytes, %lld needed",
                   (long long)work_bytes, (long long)ds_multipole_workspace_bytes(P, m, L));
        DS_REQUIRE(aligned(work, 16), "ds_multipole_bwd: work not 16-byte aligned");
    }
    DS_REQUIRE(aligned(gout, 16) && aligned(pts, 8) && aligned(center, 8) && aligned(k, 8) && aligned(coef, 16) &&
                   aligned(gpts, 8) && aligned(gcoef, 16),
               "ds_multipole_bwd: misaligned operand");
    hipStream_t st = ds::as_stream(stream);
    const double2* go = reinterpret_cast<const double2*>(gout);
    if (gpts) {
        multipole_gpts_kernel<<<(unsigned)P, 64, 0, st>>>(pts, center, k, reinterpret_cast<const double2*>(coef), go, m, L, gpts);
        DS_LAUNCH_CHECK("multipole_gpts_kernel");
    }
    if (gcoef) {
        const int G = (int)slabs(P);
        const int64_t n = (int64_t)(L + 1) * (L + 1) * m;
        double2* part = static_cast<double2*>(work);
        multipole_gcoef_kernel<<<(unsigned)G, 64, 0, st>>>(pts, center, k, go, P, m, L, part);
        DS_LAUNCH_CHECK("multipole_gcoef_kernel");
        multipole_reduce_kernel<<<(unsigned)ds::ceil_div(n, 256), 256, 0, st>>>(part, G, n, reinterpret_cast<double2*>(gcoef));
        DS_LAUNCH_CHECK("multipole_reduce_kernel");
    }
    return DS_OK;
}
