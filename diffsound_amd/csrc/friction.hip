// Friction excitation: a bow (or a rubbing finger) coupled to the modes of the object it rubs, with the exact discrete adjoint
// and a checkpointed backward - gfx950.  contact.hip's sibling: there the force comes from a hammer's spring, here from a
// friction law that reads the object's own velocity at the contact point.
//
// Per clip a the gesture is the bow's velocity vb[a,k] and normal force N[a,k] >= 0 per output sample k, and the friction
// curve's peak velocity vs[a] > 0.  With the substep h = 1 / (sr R), z_i = exp((-d_i + i w_i) h), g_i = c[a,i]^2, r_i = d_i / w_i
// and the state s_i = 0 at n = 0, for n = 0 .. F R - 1 and k = n / R:
//     v   = sum_i g_i (Re s_i - r_i Im s_i)       (the surface's velocity under the bow: d/dt of contact.hip's u)
//     vr  = vb[a,k] - v ;  x = vr / vs
//     phi = x exp((1 - x^2) / 2)                  (odd, peak 1 at vr = vs, falling beyond it: the branch that sustains the tone)
//     f   = N[a,k] phi ;  force[a,k] += f / R     (box average to the audio rate, one fp32 rounding at the store)
//     s_i = z_i (s_i + h f)                       (the banks' convention: the input enters before the rotation)
// Explicit, fp64 throughout.  N = 0 for a whole clip: the force and every gradient of the clip but gN are exact zeros.
//
// The adjoint runs the recursion down in time.  ls_i' comes from step n + 1 (0 behind the last one); with a_i = conj(z_i) ls_i':
//     lf  = gforce[k] / R + h sum_i Re a_i
//     lvr = lf N[k] phi',  phi' = (1 - x^2) exp((1 - x^2) / 2) / vs
//     gN[k] += lf phi ;  gvb[k] += lvr ;  gvs -= lvr x ;  ls_i = a_i - lvr g_i (1 - i r_i)
//     gg_i -= lvr (Re s_i[n] - r_i Im s_i[n]) ;  gr_i += lvr g_i Im s_i[n] ;  H_i += conj(s_i[n] + h f) a_i
//     gd_i = -h Re H_i + gr_i / w_i ;  gw_i = h Im H_i - gr_i d_i / w_i^2 ;  gc_i = 2 c_i gg_i.
//
// Mapping: one wavefront per clip, lane l owns modes l, l + 64, ... in registers (NM modes a lane, NM = ceil(m / 64) rounded up
// to 1, 2, 4 or 8, a template parameter, so every array is indexed at compile time); a substep is one ds::wave_sum and
// wave-uniform scalar work that all lanes repeat.  Lane 0 stores the force.  No LDS, no barrier, no atomics.  The gesture of 64
// samples is read in one coalesced load, a sample a lane, and handed out by shuffle.
// Backward, CHECKPOINTED: the forward is run again and writes s_i only where a sample begins (n = k R): 16 A F m bytes, whatever R
// is.  The reverse sweep takes the samples from the last one down: it re-runs the sample's R substeps from its checkpoint - the
// same function, so the same instructions in the same order as the forward - writes each s_i[n] to the clip's segment
// (16 R m bytes) and leaves vr[n] in a register of lane n mod R (R <= 64); then it walks the segment backwards, each lane
// reading only what it wrote itself, vr by shuffle.  The per-clip gd / gw partials are added over the clips in ascending order
// by a closing kernel: every output element has one owner, two calls give the same bits in every output and in the workspace.
// Multiply-adds are NOT fused in this unit, as in contact.hip: what separates the kernels from a float64 restatement on the
// host (tests/_friction_ref.py) is the order of the modal sum and the device's exp and sincos, nothing else.
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

// the lane's modes: z, g = c^2 and r = d / w; a slot past m holds zeros and stays zero
template <int NM>
__device__ __forceinline__ void load_modes(const double* __restrict__ dd, const double* __restrict__ ww,
                                           const double* __restrict__ crow, int m, int lane, double h, cplx* z, double* g,
                                           double* r) {
#pragma unroll
    for (int j = 0; j < NM; ++j) {
        const int i = lane + 64 * j;
        z[j] = {0.0, 0.0};
        g[j] = 0.0;
        r[j] = 0.0;
        if (i < m) {
            const double wi = ww[i], di = dd[i], ci = crow[i];
            double sn, cs;
            sincos(wi * h, &sn, &cs);
            const double e = exp(-di * h);
            z[j] = {e * cs, e * sn};
            g[j] = ci * ci;
            r[j] = di / wi;
        }
    }
}

// the friction characteristic at vr: x = vr / vs, e = exp((1 - x^2) / 2), phi = x e
struct Phi {
    double x, e, phi;
};
__device__ __forceinline__ Phi friction(double vr, double vs) {
    const double x = vr / vs;
    const double e = exp((1.0 - x * x) / 2.0);
    return {x, e, x * e};
}

// One substep, the one copy that the forward, the recording forward and the reverse sweep's re-run all execute: returns the
// wave-uniform vr and f of the substep and advances s.
template <int NM>
__device__ __forceinline__ void substep(const cplx* z, const double* g, const double* r, cplx* s, double vbk, double Nk, double vs,
                                        double h, double& vr, double& f) {
    double part = 0.0;
#pragma unroll
    for (int j = 0; j < NM; ++j) part += g[j] * (s[j].r - r[j] * s[j].i);
    vr = vbk - ds::wave_sum(part);
    f = Nk * friction(vr, vs).phi;
    const double hf = h * f;
#pragma unroll
    for (int j = 0; j < NM; ++j) s[j] = cmul(z[j], cplx{s[j].r + hf, s[j].i});
}

// The recursion.  RECORD = false: force (A x F) is written.  RECORD = true: ckpt[(a F + k) m + i] = s_i[k R], the state that
// enters sample k, is written, the force is not.
template <int NM, bool RECORD>
__global__ void __launch_bounds__(64)
    friction_fwd_kernel(const double* __restrict__ dd, const double* __restrict__ ww, const double* __restrict__ gain,
                        const double* __restrict__ bowv, const double* __restrict__ load, const double* __restrict__ peak, int m,
                        int F, int R, double h, float* __restrict__ force, double2* __restrict__ ckpt) {
    const int a = blockIdx.x, lane = threadIdx.x;
    const double vs = peak[a];
    cplx z[NM], s[NM];
    double g[NM], r[NM];
    load_modes<NM>(dd, ww, gain + (int64_t)a * m, m, lane, h, z, g, r);
#pragma unroll
    for (int j = 0; j < NM; ++j) s[j] = {0.0, 0.0};
    const int64_t row = (int64_t)a * F;
    for (int t0 = 0; t0 < F; t0 += 64) {  // 64 samples of the gesture: one a lane
        const int cnt = min(64, F - t0);
        double vbl = 0.0, Nl = 0.0;
        if (lane < cnt) {
            vbl = bowv[row + t0 + lane];
            Nl = load[row + t0 + lane];
        }
        for (int tt = 0; tt < cnt; ++tt) {
            const double vbk = __shfl(vbl, tt), Nk = __shfl(Nl, tt);
            if (RECORD) {
#pragma unroll
                for (int j = 0; j < NM; ++j)
                    if (lane + 64 * j < m) ckpt[(row + t0 + tt) * m + lane + 64 * j] = make_double2(s[j].r, s[j].i);
            }
            double acc = 0.0;
            for (int q = 0; q < R; ++q) {
                double vr, f;
                substep<NM>(z, g, r, s, vbk, Nk, vs, h, vr, f);
                acc += f / (double)R;
            }
            if (!RECORD && lane == 0) force[row + t0 + tt] = (float)acc;
        }
    }
}

// The reverse sweep over the checkpoints.  seg[(a R + q) m + i]: the clip's segment, written and read back by the lane that
// owns mode i.  part[a m + i] = (gd, gw) of clip a.  The groups (part), (ggain), (gbow, gload), (gpeak) may each be null: a
// group that is null is neither accumulated nor written.
template <int NM>
__global__ void __launch_bounds__(64)
    friction_bwd_kernel(const float* __restrict__ gforce, const double* __restrict__ dd, const double* __restrict__ ww,
                        const double* __restrict__ gain, const double* __restrict__ bowv, const double* __restrict__ load,
                        const double* __restrict__ peak, int m, int F, int R, double h, const double2* __restrict__ ckpt,
                        double2* seg, double2* __restrict__ part, double* __restrict__ ggain, double* __restrict__ gbow,
                        double* __restrict__ gload, double* __restrict__ gpeak) {
    const int a = blockIdx.x, lane = threadIdx.x;
    const double vs = peak[a];
    const bool want_modes = part != nullptr, want_gain = ggain != nullptr;  // (wave-uniform)
    cplx z[NM], ls[NM], H[NM];
    double g[NM], r[NM], gg[NM], gr[NM];
    load_modes<NM>(dd, ww, gain + (int64_t)a * m, m, lane, h, z, g, r);
#pragma unroll
    for (int j = 0; j < NM; ++j) {
        ls[j] = H[j] = {0.0, 0.0};
        gg[j] = gr[j] = 0.0;
    }
    double gvs = 0.0;
    const int64_t row = (int64_t)a * F;
    double2* myseg = seg + (int64_t)a * R * m;
    for (int t0 = ((F - 1) / 64) * 64; t0 >= 0; t0 -= 64) {
        const int cnt = min(64, F - t0);
        double vbl = 0.0, Nl = 0.0, gl = 0.0;
        if (lane < cnt) {
            vbl = bowv[row + t0 + lane];
            Nl = load[row + t0 + lane];
            gl = (double)gforce[row + t0 + lane] / (double)R;
        }
        for (int tt = cnt - 1; tt >= 0; --tt) {
            const double vbk = __shfl(vbl, tt), Nk = __shfl(Nl, tt), gk = __shfl(gl, tt);
            // the sample again from its checkpoint: s_i[n] to the segment, vr[n] to lane n mod R
            cplx s[NM];
#pragma unroll
            for (int j = 0; j < NM; ++j) {
                s[j] = {0.0, 0.0};
                if (lane + 64 * j < m) {
                    const double2 v = ckpt[(row + t0 + tt) * m + lane + 64 * j];
                    s[j] = {v.x, v.y};
                }
            }
            double vrl = 0.0;
            for (int q = 0; q < R; ++q) {
#pragma unroll
                for (int j = 0; j < NM; ++j)
                    if (lane + 64 * j < m) myseg[(int64_t)q * m + lane + 64 * j] = make_double2(s[j].r, s[j].i);
                double vr, f;
                substep<NM>(z, g, r, s, vbk, Nk, vs, h, vr, f);
                if (lane == q) vrl = vr;
            }
            // and down through it
            double sN = 0.0, sV = 0.0;
            for (int q = R - 1; q >= 0; --q) {
#pragma unroll
                for (int j = 0; j < NM; ++j) {
                    s[j] = {0.0, 0.0};
                    if (lane + 64 * j < m) {
                        const double2 v = myseg[(int64_t)q * m + lane + 64 * j];
                        s[j] = {v.x, v.y};
                    }
                }
                const Phi p = friction(__shfl(vrl, q), vs);
                const double f = Nk * p.phi;
                cplx aj[NM];
                double sum = 0.0;
#pragma unroll
                for (int j = 0; j < NM; ++j) {
                    aj[j] = cmulc(z[j], ls[j]);
                    sum += aj[j].r;
                }
                const double lf = gk + h * ds::wave_sum(sum);
                const double dphi = ((1.0 - p.x * p.x) * p.e) / vs;
                const double lvr = (lf * Nk) * dphi;
                sN += lf * p.phi;
                sV += lvr;
                gvs -= lvr * p.x;
                const double hf = h * f;
#pragma unroll
                for (int j = 0; j < NM; ++j) {
                    if (want_modes) {
                        const cplx t2 = cmulc(cplx{s[j].r + hf, s[j].i}, aj[j]);
                        H[j].r += t2.r;
                        H[j].i += t2.i;
                    }
                    const double lg = lvr * g[j];
                    if (want_gain) gg[j] -= lvr * (s[j].r - r[j] * s[j].i);
                    if (want_modes) gr[j] += lg * s[j].i;
                    ls[j] = {aj[j].r - lg, aj[j].i + lg * r[j]};
                }
            }
            if (gbow && lane == 0) {
                gbow[row + t0 + tt] = sV;
                gload[row + t0 + tt] = sN;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < NM; ++j) {
        const int i = lane + 64 * j;
        if (i < m) {
            if (want_modes) {
                const double wi = ww[i], di = dd[i];
                part[(int64_t)a * m + i] = make_double2((0.0 - h * H[j].r) + gr[j] / wi, h * H[j].i - gr[j] * di / (wi * wi));
            }
            if (want_gain) ggain[(int64_t)a * m + i] = 2.0 * gain[(int64_t)a * m + i] * gg[j];
        }
    }
    if (gpeak && lane == 0) gpeak[a] = gvs;
}

// gd[i], gw[i] = the clips' partials added in ascending order
__global__ void friction_reduce_kernel(const double2* __restrict__ part, int A, int m, double* __restrict__ gd,
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
    return A >= 1 && A <= DS_FRICTION_MAX_CLIPS && m >= 1 && m <= DS_FRICTION_MAX_MODES && R >= 1 &&
           R <= DS_FRICTION_MAX_OVERSAMPLE && F >= 1 && (int64_t)F * R <= DS_FRICTION_MAX_SUBSTEPS;
}

// The checks both entry points make, in their order; `fn` names the entry point
int check_args(const char* fn, bool pointers, int A, int m, int F, int R, double sr) {
    DS_REQUIRE(pointers, "%s: null pointer", fn);
    DS_REQUIRE(A >= 1 && A <= DS_FRICTION_MAX_CLIPS, "%s: A = %d outside 1..%d", fn, A, DS_FRICTION_MAX_CLIPS);
    DS_REQUIRE(m >= 1 && m <= DS_FRICTION_MAX_MODES, "%s: m = %d outside 1..%d", fn, m, DS_FRICTION_MAX_MODES);
    DS_REQUIRE(R >= 1 && R <= DS_FRICTION_MAX_OVERSAMPLE, "%s: R = %d outside 1..%d", fn, R, DS_FRICTION_MAX_OVERSAMPLE);
    DS_REQUIRE(F >= 1, "%s: F = %d below 1", fn, F);
    DS_REQUIRE((int64_t)F * R <= DS_FRICTION_MAX_SUBSTEPS, "%s: F R = %lld substeps above %d", fn, (long long)F * R,
               DS_FRICTION_MAX_SUBSTEPS);
    DS_REQUIRE(sr > 0 && std::isfinite(sr), "%s: sr = %g is not positive", fn, sr);
    return DS_OK;
}

using ds::aligned;

}  // namespace

// the kernel of NM modes per lane, NM = the power of two at or above ceil(m / 64)
#define FRICTION_DISPATCH(m, LAUNCH)    \
    do {                                \
        const int nm_ = ((m) + 63) / 64; \
        if (nm_ <= 1) {                 \
            LAUNCH(1);                  \
        } else if (nm_ <= 2) {          \
            LAUNCH(2);                  \
        } else if (nm_ <= 4) {          \
            LAUNCH(4);                  \
        } else {                        \
            LAUNCH(8);                  \
        }                               \
    } while (0)

extern "C" int64_t ds_friction_workspace_bytes(int A, int m, int F, int R) {
    if (!shape_ok(A, m, F, R)) return 0;
    // the checkpoints, one segment a clip, the per-clip (gd, gw) partials
    return (int64_t)sizeof(double2) * ((int64_t)A * F * m + (int64_t)A * R * m + (int64_t)A * m);
}

extern "C" int ds_friction_fwd(const double* d, const double* w, const double* gain, const double* vb, const double* N,
                               const double* vs, int A, int m, int F, int R, double sr, float* force, ds_stream_t stream) {
    if (int rc = check_args("ds_friction_fwd", d && w && gain && vb && N && vs && force, A, m, F, R, sr)) return rc;
    DS_REQUIRE(aligned(d, 8) && aligned(w, 8) && aligned(gain, 8) && aligned(vb, 8) && aligned(N, 8) && aligned(vs, 8) &&
                   aligned(force, 4),
               "ds_friction_fwd: misaligned operand");
    hipStream_t st = ds::as_stream(stream);
    const double h = 1.0 / (sr * (double)R);
#define LAUNCH(NM) friction_fwd_kernel<NM, false><<<(unsigned)A, 64, 0, st>>>(d, w, gain, vb, N, vs, m, F, R, h, force, nullptr)
    FRICTION_DISPATCH(m, LAUNCH);
#undef LAUNCH
    DS_LAUNCH_CHECK("friction_fwd_kernel");
    return DS_OK;
}

extern "C" int ds_friction_bwd(const float* gforce, const double* d, const double* w, const double* gain, const double* vb,
                               const double* N, const double* vs, int A, int m, int F, int R, double sr, void* work,
                               int64_t work_bytes, double* gd, double* gw, double* ggain, double* gvb, double* gN, double* gvs,
                               ds_stream_t stream) {
    if (int rc = check_args("ds_friction_bwd", gforce && d && w && gain && vb && N && vs && work, A, m, F, R, sr)) return rc;
    DS_REQUIRE(!gd == !gw, "ds_friction_bwd: gd and gw go together");
    DS_REQUIRE(!gvb == !gN, "ds_friction_bwd: gvb and gN go together");
    DS_REQUIRE(work_bytes >= ds_friction_workspace_bytes(A, m, F, R), "ds_friction_bwd: workspace of %lld bytes, %lld needed",
               (long long)work_bytes, (long long)ds_friction_workspace_bytes(A, m, F, R));
    DS_REQUIRE(aligned(work, 16), "ds_friction_bwd: work not 16-byte aligned");
    DS_REQUIRE(aligned(d, 8) && aligned(w, 8) && aligned(gain, 8) && aligned(vb, 8) && aligned(N, 8) && aligned(vs, 8) &&
                   aligned(gforce, 4) && aligned(gd, 8) && aligned(gw, 8) && aligned(ggain, 8) && aligned(gvb, 8) &&
                   aligned(gN, 8) && aligned(gvs, 8),
               "ds_friction_bwd: misaligned operand");
    hipStream_t st = ds::as_stream(stream);
    const double h = 1.0 / (sr * (double)R);
    double2* ckpt = static_cast<double2*>(work);
    double2* seg = ckpt + (int64_t)A * F * m;
    double2* part = gd ? seg + (int64_t)A * R * m : nullptr;
#define LAUNCH(NM) friction_fwd_kernel<NM, true><<<(unsigned)A, 64, 0, st>>>(d, w, gain, vb, N, vs, m, F, R, h, nullptr, ckpt)
    FRICTION_DISPATCH(m, LAUNCH);
#undef LAUNCH
    DS_LAUNCH_CHECK("friction_fwd_kernel");
#define LAUNCH(NM)                                                                                                          \
    friction_bwd_kernel<NM><<<(unsigned)A, 64, 0, st>>>(gforce, d, w, gain, vb, N, vs, m, F, R, h, ckpt, seg, part, ggain, gvb, \
                                                       gN, gvs)
    FRICTION_DISPATCH(m, LAUNCH);
#undef LAUNCH
    DS_LAUNCH_CHECK("friction_bwd_kernel");
    if (gd) {
        friction_reduce_kernel<<<(unsigned)ds::ceil_div(m, 64), 64, 0, st>>>(part, A, m, gd, gw);
        DS_LAUNCH_CHECK("friction_reduce_kernel");
    }
    return DS_OK;
}
