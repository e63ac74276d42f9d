// Contact force: a Hertz hammer coupled to the modes of the object it strikes, with the exact discrete adjoint - gfx950.
//
// The force of a strike is decided by the hammer (mass M, approach speed v0, contact stiffness kH, exponent p) and by the
// object's own compliance at the contact point, which is the modal gain c_i = d . u_i(p) of csrc/modesample.hip.  The
// reference has no counterpart (it is given recorded forces).  Per clip a, with the substep h = 1 / (sr R),
// z_i = exp((-d_i + i w_i) h), kap_i = c[a,i]^2 / w_i and the state xh = 0, vh = v0, s_i = 0 at n = 0, for n = 0 .. F R - 1:
//     u     = sum_i kap_i Im s_i                  (the surface's displacement under the hammer)
//     delta = xh - u ;  f = kH delta^p where delta > 0, else 0
//     force[a, n / R] += f / R                    (box average to the audio rate, one fp32 rounding at the store)
//     vh   -= h f / M ;  xh += h vh               (symplectic Euler)
//     s_i   = z_i (s_i + h f)                     (the banks' convention: the input enters before the rotation)
// Explicit, fp64 throughout.  v0 <= 0: the force and every gradient of the clip are exact zeros.
//
// The adjoint runs the recursion down in time.  lx', lv', ls_i' come from step n + 1 (0 behind the last one); with
// lv = lv' + h lx' and a_i = conj(z_i) ls_i':
//     lf = gforce[n / R] / R - (h / M) lv + h sum_i Re a_i
//     ld = lf kH p delta^(p-1) where delta > 0, else 0 ;  lx = lx' + ld ;  ls_i = a_i - i kap_i ld
//     gkH += lf delta^p ;  gM += lv h f / M^2 ;  gv0 = lv at n = 0 ;  gkap_i -= ld Im s_i[n]
//     H_i += conj(s_i[n] + h f) a_i ;  gd_i = -h Re H_i,  gw_i = h Im H_i - (c^2 / w^2) gkap_i ;  gc_i = (2 c / w) gkap_i.
//
// Mapping: one wavefront per clip, lane l owns modes l, l + 64, ... in registers (NM = ceil(m / 64) <= 8 of them, a
// template parameter, so every array is indexed at compile time); a step is one ds::wave_sum and wave-uniform scalar work
// that all lanes repeat.  Lane 0 stores the force.  No LDS, no barrier, no atomics.  The time loop is sequential by nature:
// with A waves on 256 compute units the kernels are latency-bound.
// Backward: the forward is run again and writes (delta, delta^p) and s_i[n] of every substep to the workspace (stored, not
// checkpointed: 16 (1 + m) bytes per substep and clip); the reverse sweep reads them one step ahead of their use.  The
// per-clip gd / gw partials are added over the clips in ascending order by a closing kernel: every output element has one
// owner, two calls give the same bits.
// Multiply-adds are NOT fused in this unit: the kernels restate the scheme operation by operation, so that what separates them
// from a float64 restatement on the host is the order of the modal sum and the device's exp, sincos and pow, nothing else
// (tests/_contact_ref.py measures its bounds from that restatement's own error).  The loop waits on the butterfly, not on these.
#include <cmath>
#include <cstdint>

#include "ds_common.h"

#pragma clang fp contract(off)

namespace {

struct cplx {
    double r, i;
};

__device__ __forceinline__ cplx cmul(cplx a, cplx b) { return {a.r * b.r - a.i * b.i, a.r * b.i + a.i * b.r}; }
// conj(a) b
__device__ __forceinline__ cplx cmulc(cplx a, cplx b) { return {a.r * b.r + a.i * b.i, a.r * b.i - a.i * b.r}; }

// the lane's modes: z, kap and, where asked for, c and w themselves; a slot past m holds zeros and stays zero
template <int NM>
__device__ __forceinline__ void load_modes(const double* __restrict__ dd, const double* __restrict__ ww,
                                           const double* __restrict__ crow, int m, int lane, double h, cplx* z, double* kap,
                                           double* c, double* w) {
#pragma unroll
    for (int j = 0; j < NM; ++j) {
        const int i = lane + 64 * j;
        z[j] = {0.0, 0.0};
        kap[j] = 0.0;
        if (c) c[j] = 0.0;
        if (w) w[j] = 1.0;
        if (i < m) {
            const double wi = ww[i], ci = crow[i];
            double sn, cs;
            sincos(wi * h, &sn, &cs);
            const double e = exp(-dd[i] * h);
            z[j] = {e * cs, e * sn};
            kap[j] = ci * ci / wi;
            if (c) c[j] = ci;
            if (w) w[j] = wi;
        }
    }
}

// The recursion.  RECORD = false: force (A x F) is written.  RECORD = true: traj[a N + n] = (delta, delta^p or 0) and
// st[(a N + n) m + i] = s_i[n] are written, the force is not.
template <int NM, bool RECORD>
__global__ void __launch_bounds__(64)
    contact_fwd_kernel(const double* __restrict__ dd, const double* __restrict__ ww, const double* __restrict__ gain,
                       const double* __restrict__ mass, const double* __restrict__ vel, const double* __restrict__ stiff,
                       int m, int F, int R, double p, double h, float* __restrict__ force, double2* __restrict__ traj,
                       double2* __restrict__ st) {
    const int a = blockIdx.x, lane = threadIdx.x;
    const double M = mass[a], v0 = vel[a], kH = stiff[a];
    if (!(v0 > 0.0)) {  // (wave-uniform) the hammer never arrives
        if (!RECORD)
            for (int t = lane; t < F; t += 64) force[(int64_t)a * F + t] = 0.f;
        return;
    }
    cplx z[NM], s[NM];
    double kap[NM];
    load_modes<NM>(dd, ww, gain + (int64_t)a * m, m, lane, h, z, kap, nullptr, nullptr);
#pragma unroll
    for (int j = 0; j < NM; ++j) s[j] = {0.0, 0.0};
    double xh = 0.0, vh = v0;
    int64_t n = (int64_t)a * F * R;
    for (int t = 0; t < F; ++t) {
        double acc = 0.0;
        for (int r = 0; r < R; ++r, ++n) {
            double part = 0.0;
#pragma unroll
            for (int j = 0; j < NM; ++j) part += kap[j] * s[j].i;
            const double delta = xh - ds::wave_sum(part);
            double pw = 0.0;
            if (delta > 0.0) pw = pow(delta, p);  // (wave-uniform: the butterfly leaves the same bits in every lane)
            const double f = kH * pw;
            acc += f / (double)R;
            if (RECORD) {
                if (lane == 0) traj[n] = make_double2(delta, pw);
#pragma unroll
                for (int j = 0; j < NM; ++j)
                    if (lane + 64 * j < m) st[n * m + lane + 64 * j] = make_double2(s[j].r, s[j].i);
            }
            const double hf = h * f;
            vh -= hf / M;
            xh += h * vh;
#pragma unroll
            for (int j = 0; j < NM; ++j) s[j] = cmul(z[j], cplx{s[j].r + hf, s[j].i});
        }
        if (!RECORD && lane == 0) force[(int64_t)a * F + t] = (float)acc;
    }
}

// The reverse sweep over what the recording run left.  part[a m + i] = (gd, gw) of clip a; part, ggain, ghammer (gmass,
// gvel, gstiff: all three or none) may each be null.
template <int NM>
__global__ void __launch_bounds__(64)
    contact_bwd_kernel(const float* __restrict__ gforce, const double* __restrict__ dd, const double* __restrict__ ww,
                       const double* __restrict__ gain, const double* __restrict__ mass, const double* __restrict__ vel,
                       const double* __restrict__ stiff, int m, int F, int R, double p, double h,
                       const double2* __restrict__ traj, const double2* __restrict__ st, double2* __restrict__ part,
                       double* __restrict__ ggain, double* __restrict__ gmass, double* __restrict__ gvel,
                       double* __restrict__ gstiff) {
    const int a = blockIdx.x, lane = threadIdx.x;
    const double M = mass[a], v0 = vel[a], kH = stiff[a];
    const bool hit = v0 > 0.0;  // (wave-uniform)
    cplx z[NM], ls[NM], H[NM], sn[NM];
    double kap[NM], c[NM], w[NM], gk[NM];
#pragma unroll
    for (int j = 0; j < NM; ++j) {
        ls[j] = H[j] = sn[j] = {0.0, 0.0};
        gk[j] = 0.0;
        c[j] = 0.0;
        w[j] = 1.0;
    }
    double lx = 0.0, lv = 0.0, gM = 0.0, gK = 0.0;
    if (hit) {
        load_modes<NM>(dd, ww, gain + (int64_t)a * m, m, lane, h, z, kap, c, w);
        const double h_M = h / M, MM = M * M;
        const int64_t n0 = (int64_t)a * F * R;
        const float* grow = gforce + (int64_t)a * F;
        // step n's record is loaded while step n + 1 is worked on
        int64_t n = n0 + (int64_t)F * R - 1;
        double2 tn = traj[n];
#pragma unroll
        for (int j = 0; j < NM; ++j)
            if (lane + 64 * j < m) {
                const double2 v = st[n * m + lane + 64 * j];
                sn[j] = {v.x, v.y};
            }
        for (int t = F - 1; t >= 0; --t) {
            const double g = (double)grow[t] / (double)R;
            for (int r = R - 1; r >= 0; --r, --n) {
                const double delta = tn.x, pw = tn.y;
                cplx s[NM];
#pragma unroll
                for (int j = 0; j < NM; ++j) s[j] = sn[j];
                if (n > n0) {
                    tn = traj[n - 1];
#pragma unroll
                    for (int j = 0; j < NM; ++j)
                        if (lane + 64 * j < m) {
                            const double2 v = st[(n - 1) * m + lane + 64 * j];
                            sn[j] = {v.x, v.y};
                        }
                }
                lv += h * lx;
                cplx aj[NM];
                double sum = 0.0;
#pragma unroll
                for (int j = 0; j < NM; ++j) {
                    aj[j] = cmulc(z[j], ls[j]);
                    sum += aj[j].r;
                }
                const double lf = g - h_M * lv + h * ds::wave_sum(sum);
                const double f = kH * pw;
                double ld = 0.0;
                if (delta > 0.0) ld = lf * kH * p * pow(delta, p - 1.0);  // (wave-uniform)
                gK += lf * pw;
                gM += lv * h * f / MM;
                lx += ld;
                const double hf = h * f;
#pragma unroll
                for (int j = 0; j < NM; ++j) {
                    const cplx t2 = cmulc(cplx{s[j].r + hf, s[j].i}, aj[j]);
                    H[j].r += t2.r;
                    H[j].i += t2.i;
                    gk[j] -= ld * s[j].i;
                    ls[j] = {aj[j].r, aj[j].i - kap[j] * ld};
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < NM; ++j) {
        const int i = lane + 64 * j;
        if (i < m) {
            const double cw = c[j] / w[j];
            if (part) part[(int64_t)a * m + i] = make_double2(0.0 - h * H[j].r, h * H[j].i - cw * cw * gk[j]);
            if (ggain) ggain[(int64_t)a * m + i] = 2.0 * cw * gk[j];
        }
    }
    if (gmass && lane == 0) {
        gmass[a] = gM;
        gvel[a] = lv;
        gstiff[a] = gK;
    }
}

// gd[i], gw[i] = the clips' partials added in ascending order
__global__ void contact_reduce_kernel(const double2* __restrict__ part, int A, int m, double* __restrict__ gd,
                                      double* __restrict__ gw) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    double sd = 0.0, sw = 0.0;
    for (int a = 0; a < A; ++a) {
        const double2 v = part[(int64_t)a * m + i];
        sd += v.x;
        sw += v.y;
    }
    gd[i] = sd;
    gw[i] = sw;
}

inline bool shape_ok(int A, int m, int F, int R) {
    return A >= 1 && A <= 65535 && m >= 1 && m <= DS_CONTACT_MAX_MODES && R >= 1 && R <= DS_CONTACT_MAX_OVERSAMPLE && F >= 1 &&
           (int64_t)F * R <= DS_CONTACT_MAX_SUBSTEPS;
}

// The checks both entry points make, in their order; `fn` names the entry point
int check_args(const char* fn, bool pointers, int A, int m, int F, int R, double p, double sr) {
    DS_REQUIRE(pointers, "%s: null pointer", fn);
    DS_REQUIRE(A >= 1 && A <= 65535, "%s: A = %d outside 1..65535", fn, A);
    DS_REQUIRE(m >= 1 && m <= DS_CONTACT_MAX_MODES, "%s: m = %d outside 1..%d", fn, m, DS_CONTACT_MAX_MODES);
    DS_REQUIRE(R >= 1 && R <= DS_CONTACT_MAX_OVERSAMPLE, "%s: R = %d outside 1..%d", fn, R, DS_CONTACT_MAX_OVERSAMPLE);
    DS_REQUIRE(F >= 1, "%s: F = %d below 1", fn, F);
    DS_REQUIRE((int64_t)F * R <= DS_CONTACT_MAX_SUBSTEPS, "%s: F R = %lld substeps above %d", fn, (long long)F * R,
               DS_CONTACT_MAX_SUBSTEPS);
    DS_REQUIRE(std::isfinite(p) && p >= 1.0, "%s: p = %g is not a finite exponent >= 1", fn, p);
    DS_REQUIRE(sr > 0 && std::isfinite(sr), "%s: sr = %g is not positive", fn, sr);
    return DS_OK;
}

using ds::aligned;

}  // namespace

// the kernel of NM = ceil(m / 64) modes per lane
#define CONTACT_DISPATCH(nm, LAUNCH) \
    switch (nm) {                    \
        case 1: LAUNCH(1); break;    \
        case 2: LAUNCH(2); break;    \
        case 3: LAUNCH(3); break;    \
        case 4: LAUNCH(4); break;    \
        case 5: LAUNCH(5); break;    \
        case 6: LAUNCH(6); break;    \
        case 7: LAUNCH(7); break;    \
        default: LAUNCH(8); break;   \
    }

extern "C" int64_t ds_contact_workspace_bytes(int A, int m, int F, int R) {
    if (!shape_ok(A, m, F, R)) return 0;
    const int64_t N = (int64_t)F * R;
    return (int64_t)sizeof(double2) * ((int64_t)A * N * (1 + m) + (int64_t)A * m);
}

extern "C" int ds_contact_fwd(const double* d, const double* w, const double* gain, const double* mass, const double* vel,
                              const double* stiff, int A, int m, int F, int R, double p, double sr, float* force,
                              ds_stream_t stream) {
    if (int rc = check_args("ds_contact_fwd", d && w && gain && mass && vel && stiff && force, A, m, F, R, p, sr)) return rc;
    DS_REQUIRE(aligned(d, 8) && aligned(w, 8) && aligned(gain, 8) && aligned(mass, 8) && aligned(vel, 8) && aligned(stiff, 8) &&
                   aligned(force, 4),
               "ds_contact_fwd: misaligned operand");
    hipStream_t st = ds::as_stream(stream);
    const double h = 1.0 / (sr * (double)R);
#define LAUNCH(NM)                                                                                                        \
    contact_fwd_kernel<NM, false><<<(unsigned)A, 64, 0, st>>>(d, w, gain, mass, vel, stiff, m, F, R, p, h, force, nullptr, \
                                                             nullptr)
    CONTACT_DISPATCH((m + 63) / 64, LAUNCH)
#undef LAUNCH
    DS_LAUNCH_CHECK("contact_fwd_kernel");
    return DS_OK;
}

extern "C" int ds_contact_bwd(const float* gforce, const double* d, const double* w, const double* gain, const double* mass,
                              const double* vel, const double* stiff, int A, int m, int F, int R, double p, double sr,
                              void* work, int64_t work_bytes, double* gd, double* gw, double* ggain, double* gmass,
                              double* gvel, double* gstiff, ds_stream_t stream) {
    if (int rc = check_args("ds_contact_bwd", gforce && d && w && gain && mass && vel && stiff && work, A, m, F, R, p, sr))
        return rc;
    DS_REQUIRE(!gd == !gw, "ds_contact_bwd: gd and gw go together");
    DS_REQUIRE(!gmass == !gvel && !gmass == !gstiff, "ds_contact_bwd: gmass, gvel and gstiff go together");
    DS_REQUIRE(work_bytes >= ds_contact_workspace_bytes(A, m, F, R), "ds_contact_bwd: workspace of %lld bytes, %lld needed",
               (long long)work_bytes, (long long)ds_contact_workspace_bytes(A, m, F, R));
    DS_REQUIRE(aligned(work, 16), "ds_contact_bwd: work not 16-byte aligned");
    DS_REQUIRE(aligned(d, 8) && aligned(w, 8) && aligned(gain, 8) && aligned(mass, 8) && aligned(vel, 8) && aligned(stiff, 8) &&
                   aligned(gforce, 4) && aligned(gd, 8) && aligned(gw, 8) && aligned(ggain, 8) && aligned(gmass, 8) &&
                   aligned(gvel, 8) && aligned(gstiff, 8),
               "ds_contact_bwd: misaligned operand");
    hipStream_t st = ds::as_stream(stream);
    const double h = 1.0 / (sr * (double)R);
    const int64_t N = (int64_t)F * R;
    double2* traj = static_cast<double2*>(work);
    double2* state = traj + (int64_t)A * N;
    double2* part = gd ? state + (int64_t)A * N * m : nullptr;
#define LAUNCH(NM)                                                                                                      \
    contact_fwd_kernel<NM, true><<<(unsigned)A, 64, 0, st>>>(d, w, gain, mass, vel, stiff, m, F, R, p, h, nullptr, traj, \
                                                            state)
    CONTACT_DISPATCH((m + 63) / 64, LAUNCH)
#undef LAUNCH
    DS_LAUNCH_CHECK("contact_fwd_kernel");
#define LAUNCH(NM)                                                                                                          \
    contact_bwd_kernel<NM><<<(unsigned)A, 64, 0, st>>>(gforce, d, w, gain, mass, vel, stiff, m, F, R, p, h, traj, state, part, \
                                                      ggain, gmass, gvel, gstiff)
    CONTACT_DISPATCH((m + 63) / 64, LAUNCH)
#undef LAUNCH
    DS_LAUNCH_CHECK("contact_bwd_kernel");
    if (gd) {
        contact_reduce_kernel<<<(unsigned)ds::ceil_div(m, 64), 64, 0, st>>>(part, A, m, gd, gw);
        DS_LAUNCH_CHECK("contact_reduce_kernel");
    }
    return DS_OK;
}
