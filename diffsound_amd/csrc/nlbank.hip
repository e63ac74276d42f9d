// Tension-modulated modal bank: the modes of a thin object struck hard, stiffened by the stretching of its own mid-surface
// (Kirchhoff-Carrier for strings, Berger for plates), with the exact discrete adjoint and a checkpointed backward - gfx950.
// contact.hip's and friction.hip's sibling: there the nonlinearity makes a force, here it sits inside the bank and the output
// is the sound.
//
// Per clip a, with the substep h = 1 / (sr R), z_i = exp((-d_i + i w_i) h) and the state s_i = 0 at n = 0, for
// n = 0 .. S R - 1 and k = n / R:
//     q_i   = Im s_i / w_i                                 (the modal coordinate: contact.hip's u without the gain)
//     E_r   = sum_i C[r,i] q_i^2 ;  T_r = gamma[a,r] E_r    (r < K: the stretch energies and the tensions they make)
//     kap_i = sum_r C[r,i] T_r                             (ascending r)
//     p_i   = c[a,i] f[a,k] - kap_i q_i                    (f[a,k] = 0 for k >= F)
//     s_i   = z_i (s_i + h p_i)                            (the banks' convention: the input enters before the rotation)
//     if n = k R + R - 1:  y[a,k] = sr sum_i amp[a,i] Im s_i      (one fp32 rounding at the store)
// Explicit, fp64 throughout.  gamma = 0 and R = 1: osc_driven.hip's x = z (x + f) scaled by h, y the driven bank's with the
// amplitudes amp c.  A clip whose gamma is 0 throughout takes the same path; its T, kap and every nonlinear term are exact zeros.
//
// The adjoint runs the recursion down in time.  ls_i' comes from step n + 1 (0 behind the last one), gy is the incoming
// gradient.  At the last substep of a sample ls_i' += i sr amp_i gy[k] and gamp_i += sr gy[k] Im s_i[n+1].  Then, with
// a_i = conj(z_i) ls_i' and lp_i = h Re a_i:
//     gf[k]  += sum_i c_i lp_i ;            gc_i += f[k] lp_i
//     lkap_i  = -q_i lp_i ;                 lq_i  = -kap_i lp_i
//     lT_r    = sum_i C_ri lkap_i ;         gC_ri += T_r lkap_i
//     ggamma_r += lT_r E_r ;  lE_r = gamma_r lT_r ;  gC_ri += lE_r q_i^2 ;  lq_i += 2 lE_r C_ri q_i
//     ls_i    = a_i + i lq_i / w_i ;        gq_i  += lq_i q_i
//     H_i    += conj(s_i[n] + h p_i) a_i
// and at the end gd_i = -h Re H_i, gw_i = h Im H_i - gq_i / w_i.  (tests/test_nlbank_ref_cpu.py holds this sweep, restated in
// numpy, to central differences of the longdouble forward for all seven gradients.)
//
// Mapping: friction.hip's.  One wavefront per clip, lane l owns modes l, l + 64, ... in registers: NM modes a lane (NM =
// ceil(m / 64) rounded up to 1, 2, 4 or 8) and K terms are template parameters, so every array is indexed at compile time.  A
// forward substep is K ds::wave_sums and per-lane work, a sample's read-out one more; a backward substep is K + 1 of them
// (the lT_r and gf's sum).  Lane 0 stores y and gf.  No LDS, no barrier, no atomics.  The force of 64 samples is read in one
// coalesced load, a sample a lane, and handed out by shuffle.
// Backward, CHECKPOINTED: the forward is run again and writes s_i only where a sample begins (n = k R): 16 A S m bytes, whatever R
// is.  The reverse sweep takes the samples from the last one down: it re-runs the sample's R substeps from its checkpoint - the
// same function, so the same instructions in the same order as the forward - writes each s_i[n] to the clip's segment
// (16 R m bytes) and leaves E_r[n] in registers of lane n mod R (R <= 64); then it walks the segment backwards, each lane
// reading only what it wrote itself, the E_r by shuffle.  The per-clip partials of gd / gw and of gC are added over the clips in
// ascending order by a closing kernel: every output element has one owner, two calls give the same bits in every output and in
// the workspace.
// Multiply-adds are NOT fused in this unit, as in contact.hip and friction.hip: what separates the kernels from a float64
// restatement on the host (tests/_nlbank_ref.py) is the order of the modal sums and the device's exp and sincos, nothing else.
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

// What a lane keeps of its modes: z, w, the input gain c and the K stretch coefficients.  A slot past m holds zeros (w = 1, so
// that q = 0 / 1) and stays zero.
template <int NM, int K>
struct Modes {
    cplx z[NM];
    double w[NM], c[NM], C[K][NM], gam[K];
};

template <int NM, int K>
__device__ __forceinline__ void load_modes(const double* __restrict__ dd, const double* __restrict__ ww,
                                           const double* __restrict__ crow, const double* __restrict__ stretch,
                                           const double* __restrict__ grow, int m, int lane, double h, Modes<NM, K>& M) {
#pragma unroll
    for (int j = 0; j < NM; ++j) {
        const int i = lane + 64 * j;
        M.z[j] = {0.0, 0.0};
        M.w[j] = 1.0;
        M.c[j] = 0.0;
#pragma unroll
        for (int r = 0; r < K; ++r) M.C[r][j] = 0.0;
        if (i < m) {
            const double wi = ww[i], di = dd[i];
            double sn, cs;
            sincos(wi * h, &sn, &cs);
            const double e = exp(-di * h);
            M.z[j] = {e * cs, e * sn};
            M.w[j] = wi;
            M.c[j] = crow[i];
#pragma unroll
            for (int r = 0; r < K; ++r) M.C[r][j] = stretch[(int64_t)r * m + i];
        }
    }
#pragma unroll
    for (int r = 0; r < K; ++r) M.gam[r] = grow[r];
}

// q_i and E_r of the states s: the K wave sums of a substep
template <int NM, int K>
__device__ __forceinline__ void energies(const Modes<NM, K>& M, const cplx* s, double* q, double* E) {
    double part[K];
#pragma unroll
    for (int r = 0; r < K; ++r) part[r] = 0.0;
#pragma unroll
    for (int j = 0; j < NM; ++j) {
        q[j] = s[j].i / M.w[j];
        const double q2 = q[j] * q[j];
#pragma unroll
        for (int r = 0; r < K; ++r) part[r] += M.C[r][j] * q2;
    }
#pragma unroll
    for (int r = 0; r < K; ++r) E[r] = ds::wave_sum(part[r]);
}

// kap_i and hp_i = h p_i from q_i and the E_r: the forward's and the reverse sweep's one copy, so both form the same bits
template <int NM, int K>
__device__ __forceinline__ void drive(const Modes<NM, K>& M, const double* q, const double* E, double fk, double h, double* T,
                                      double* kap, double* hp) {
#pragma unroll
    for (int r = 0; r < K; ++r) T[r] = M.gam[r] * E[r];
#pragma unroll
    for (int j = 0; j < NM; ++j) {
        double kj = M.C[0][j] * T[0];
#pragma unroll
        for (int r = 1; r < K; ++r) kj += M.C[r][j] * T[r];
        kap[j] = kj;
        hp[j] = h * (M.c[j] * fk - kj * q[j]);
    }
}

// One substep, the one copy that the forward, the recording forward and the reverse sweep's re-run all execute: advances s and
// returns the wave-uniform E_r of the substep.
template <int NM, int K>
__device__ __forceinline__ void substep(const Modes<NM, K>& M, cplx* s, double fk, double h, double* E) {
    double q[NM], T[K], kap[NM], hp[NM];
    energies<NM, K>(M, s, q, E);
    drive<NM, K>(M, q, E, fk, h, T, kap, hp);
#pragma unroll
    for (int j = 0; j < NM; ++j) s[j] = cmul(M.z[j], cplx{s[j].r + hp[j], s[j].i});
}

// The recursion.  RECORD = false: y (A x S) is written.  RECORD = true: ckpt[(a S + k) m + i] = s_i[k R], the state that
// enters sample k, is written, y is not.
template <int NM, int K, bool RECORD>
__global__ void __launch_bounds__(64)
    nlbank_fwd_kernel(const double* __restrict__ dd, const double* __restrict__ ww, const double* __restrict__ gain,
                      const double* __restrict__ amp, const double* __restrict__ force, const double* __restrict__ stretch,
                      const double* __restrict__ gamma, int m, int F, int S, int R, double h, double sr, float* __restrict__ y,
                      double2* __restrict__ ckpt) {
    const int a = blockIdx.x, lane = threadIdx.x;
    Modes<NM, K> M;
    load_modes<NM, K>(dd, ww, gain + (int64_t)a * m, stretch, gamma + (int64_t)a * K, m, lane, h, M);
    cplx s[NM];
    double am[NM];
#pragma unroll
    for (int j = 0; j < NM; ++j) {
        s[j] = {0.0, 0.0};
        am[j] = (!RECORD && lane + 64 * j < m) ? amp[(int64_t)a * m + lane + 64 * j] : 0.0;
    }
    const int64_t row = (int64_t)a * S, frow = (int64_t)a * F;
    for (int t0 = 0; t0 < S; t0 += 64) {  // 64 samples of the force: one a lane
        const int cnt = min(64, S - t0);
        const double fl = (lane < cnt && t0 + lane < F) ? force[frow + t0 + lane] : 0.0;
        for (int tt = 0; tt < cnt; ++tt) {
            const double fk = __shfl(fl, tt);
            if (RECORD) {
#pragma unroll
                for (int j = 0; j < NM; ++j)
                    if (lane + 64 * j < m) ckpt[(row + t0 + tt) * m + lane + 64 * j] = make_double2(s[j].r, s[j].i);
            }
            for (int q = 0; q < R; ++q) {
                double E[K];
                substep<NM, K>(M, s, fk, h, E);
            }
            if (!RECORD) {
                double part = 0.0;
#pragma unroll
                for (int j = 0; j < NM; ++j) part += am[j] * s[j].i;
                const double out = sr * ds::wave_sum(part);
                if (lane == 0) y[row + t0 + tt] = (float)out;
            }
        }
    }
}

// The reverse sweep over the checkpoints.  seg[(a R + q) m + i]: the clip's segment, written and read back by the lane that
// owns mode i.  part[a m + i] = (gd, gw) of clip a, partC[(a K + r) m + i] = gC of clip a.  The groups (part), (ggain), (gamp),
// (gforce), (partC), (ggamma) may each be null: a group that is null is neither accumulated nor written.
template <int NM, int K>
__global__ void __launch_bounds__(64)
    nlbank_bwd_kernel(const float* __restrict__ gy, const double* __restrict__ dd, const double* __restrict__ ww,
                      const double* __restrict__ gain, const double* __restrict__ amp, const double* __restrict__ force,
                      const double* __restrict__ stretch, const double* __restrict__ gamma, int m, int F, int S, int R, double h,
                      double sr, const double2* __restrict__ ckpt, double2* seg, double2* __restrict__ part,
                      double* __restrict__ partC, double* __restrict__ ggain, double* __restrict__ gamp,
                      double* __restrict__ gforce, double* __restrict__ ggamma) {
    const int a = blockIdx.x, lane = threadIdx.x;
    const bool want_modes = part != nullptr, want_gain = ggain != nullptr, want_amp = gamp != nullptr,  // (wave-uniform)
        want_force = gforce != nullptr, want_C = partC != nullptr;
    Modes<NM, K> M;
    load_modes<NM, K>(dd, ww, gain + (int64_t)a * m, stretch, gamma + (int64_t)a * K, m, lane, h, M);
    cplx ls[NM], H[NM];
    double gc[NM], ga[NM], gq[NM], gC[K][NM], gg[K];
#pragma unroll
    for (int j = 0; j < NM; ++j) {
        ls[j] = H[j] = {0.0, 0.0};
        gc[j] = ga[j] = gq[j] = 0.0;
#pragma unroll
        for (int r = 0; r < K; ++r) gC[r][j] = 0.0;
    }
#pragma unroll
    for (int r = 0; r < K; ++r) gg[r] = 0.0;
    const int64_t row = (int64_t)a * S, frow = (int64_t)a * F;
    if (want_force)  // force samples behind the output are not read: their gradient is an exact zero
        for (int k = S + lane; k < F; k += 64) gforce[frow + k] = 0.0;
    double2* myseg = seg + (int64_t)a * R * m;
    for (int t0 = ((S - 1) / 64) * 64; t0 >= 0; t0 -= 64) {
        const int cnt = min(64, S - t0);
        const double fl = (lane < cnt && t0 + lane < F) ? force[frow + t0 + lane] : 0.0;
        const double gl = lane < cnt ? sr * (double)gy[row + t0 + lane] : 0.0;
        for (int tt = cnt - 1; tt >= 0; --tt) {
            const double fk = __shfl(fl, tt), gk = __shfl(gl, tt);
            // the sample again from its checkpoint: s_i[n] to the segment, E_r[n] to lane n mod R
            cplx s[NM];
#pragma unroll
            for (int j = 0; j < NM; ++j) {
                s[j] = {0.0, 0.0};
                if (lane + 64 * j < m) {
                    const double2 v = ckpt[(row + t0 + tt) * m + lane + 64 * j];
                    s[j] = {v.x, v.y};
                }
            }
            double El[K];
#pragma unroll
            for (int r = 0; r < K; ++r) El[r] = 0.0;
            for (int q = 0; q < R; ++q) {
#pragma unroll
                for (int j = 0; j < NM; ++j)
                    if (lane + 64 * j < m) myseg[(int64_t)q * m + lane + 64 * j] = make_double2(s[j].r, s[j].i);
                double E[K];
                substep<NM, K>(M, s, fk, h, E);
                if (lane == q) {
#pragma unroll
                    for (int r = 0; r < K; ++r) El[r] = E[r];
                }
            }
            // the sample's read-out: s is s[n + 1] of the sample's last substep (amp is read here, once a sample, and not kept:
            // the registers it would take are what NM = 8 with K = 4 is short of)
#pragma unroll
            for (int j = 0; j < NM; ++j) {
                const double am = lane + 64 * j < m ? amp[(int64_t)a * m + lane + 64 * j] : 0.0;
                ls[j].i += am * gk;
                if (want_amp) ga[j] += gk * s[j].i;
            }
            // and down through the segment
            double sF = 0.0;
            for (int q = R - 1; q >= 0; --q) {
#pragma unroll
                for (int j = 0; j < NM; ++j) {
                    s[j] = {0.0, 0.0};
                    if (lane + 64 * j < m) {
                        const double2 v = myseg[(int64_t)q * m + lane + 64 * j];
                        s[j] = {v.x, v.y};
                    }
                }
                double E[K], T[K], qq[NM], kap[NM], hp[NM], lp[NM], lkap[NM], lq[NM];
#pragma unroll
                for (int r = 0; r < K; ++r) E[r] = __shfl(El[r], q);
#pragma unroll
                for (int j = 0; j < NM; ++j) qq[j] = s[j].i / M.w[j];
                drive<NM, K>(M, qq, E, fk, h, T, kap, hp);
                cplx aj[NM];
                double sumF = 0.0, sumT[K];
#pragma unroll
                for (int r = 0; r < K; ++r) sumT[r] = 0.0;
#pragma unroll
                for (int j = 0; j < NM; ++j) {
                    aj[j] = cmulc(M.z[j], ls[j]);
                    lp[j] = h * aj[j].r;
                    sumF += M.c[j] * lp[j];
                    if (want_gain) gc[j] += fk * lp[j];
                    lkap[j] = -(qq[j] * lp[j]);
                    lq[j] = -(kap[j] * lp[j]);
#pragma unroll
                    for (int r = 0; r < K; ++r) sumT[r] += M.C[r][j] * lkap[j];
                }
                if (want_force) sF += ds::wave_sum(sumF);
#pragma unroll
                for (int r = 0; r < K; ++r) {
                    const double lT = ds::wave_sum(sumT[r]);
                    gg[r] += lT * E[r];
                    const double lE = M.gam[r] * lT;
                    const double lE2 = 2.0 * lE;
#pragma unroll
                    for (int j = 0; j < NM; ++j) {
                        if (want_C) {
                            gC[r][j] += T[r] * lkap[j];
                            gC[r][j] += lE * (qq[j] * qq[j]);
                        }
                        lq[j] += lE2 * (M.C[r][j] * qq[j]);
                    }
                }
#pragma unroll
                for (int j = 0; j < NM; ++j) {
                    if (want_modes) {
                        const cplx t2 = cmulc(cplx{s[j].r + hp[j], s[j].i}, aj[j]);
                        H[j].r += t2.r;
                        H[j].i += t2.i;
                        gq[j] += lq[j] * qq[j];
                    }
                    ls[j] = {aj[j].r, aj[j].i + lq[j] / M.w[j]};
                }
            }
            if (want_force && lane == 0 && t0 + tt < F) gforce[frow + t0 + tt] = sF;
        }
    }
#pragma unroll
    for (int j = 0; j < NM; ++j) {
        const int i = lane + 64 * j;
        if (i < m) {
            if (want_modes) part[(int64_t)a * m + i] = make_double2(0.0 - h * H[j].r, h * H[j].i - gq[j] / M.w[j]);
            if (want_gain) ggain[(int64_t)a * m + i] = gc[j];
            if (want_amp) gamp[(int64_t)a * m + i] = ga[j];
            if (want_C) {
#pragma unroll
                for (int r = 0; r < K; ++r) partC[((int64_t)a * K + r) * m + i] = gC[r][j];
            }
        }
    }
    if (ggamma && lane == 0) {
#pragma unroll
        for (int r = 0; r < K; ++r) ggamma[(int64_t)a * K + r] = gg[r];
    }
}

// gd[i], gw[i] and gC[r,i] = the clips' partials added in ascending order; thread t owns gC's element t and, below m, gd[t], gw[t]
__global__ void nlbank_reduce_kernel(const double2* __restrict__ part, const double* __restrict__ partC, int A, int m, int K,
                                     double* __restrict__ gd, double* __restrict__ gw, double* __restrict__ gC) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= m * K) return;
    if (part && t < m) {
        double sd = 0.0, sw = 0.0;
        for (int a = 0; a < A; ++a) {
            const double2 v = part[(int64_t)a * m + t];
            sd += v.x;
            sw += v.y;
        }
        gd[t] = sd;
        gw[t] = sw;
    }
    if (partC) {
        double sc = 0.0;
        for (int a = 0; a < A; ++a) sc += partC[(int64_t)a * K * m + t];
        gC[t] = sc;
    }
}

inline bool shape_ok(int A, int m, int K, int S, int R) {
    return A >= 1 && A <= DS_NLBANK_MAX_CLIPS && m >= 1 && m <= DS_NLBANK_MAX_MODES && K >= 1 && K <= DS_NLBANK_MAX_TERMS &&
           R >= 1 && R <= DS_NLBANK_MAX_OVERSAMPLE && S >= 1 && (int64_t)S * R <= DS_NLBANK_MAX_SUBSTEPS;
}

// The checks both entry points make, in their order; `fn` names the entry point
int check_args(const char* fn, bool pointers, int A, int m, int K, int F, int S, int R, double sr) {
    DS_REQUIRE(pointers, "%s: null pointer", fn);
    DS_REQUIRE(A >= 1 && A <= DS_NLBANK_MAX_CLIPS, "%s: A = %d outside 1..%d", fn, A, DS_NLBANK_MAX_CLIPS);
    DS_REQUIRE(m >= 1 && m <= DS_NLBANK_MAX_MODES, "%s: m = %d outside 1..%d", fn, m, DS_NLBANK_MAX_MODES);
    DS_REQUIRE(K >= 1 && K <= DS_NLBANK_MAX_TERMS, "%s: K = %d outside 1..%d", fn, K, DS_NLBANK_MAX_TERMS);
    DS_REQUIRE(R >= 1 && R <= DS_NLBANK_MAX_OVERSAMPLE, "%s: R = %d outside 1..%d", fn, R, DS_NLBANK_MAX_OVERSAMPLE);
    DS_REQUIRE(F >= 1, "%s: F = %d below 1", fn, F);
    DS_REQUIRE(S >= 1, "%s: S = %d below 1", fn, S);
    DS_REQUIRE((int64_t)S * R <= DS_NLBANK_MAX_SUBSTEPS, "%s: S R = %lld substeps above %d", fn, (long long)S * R,
               DS_NLBANK_MAX_SUBSTEPS);
    DS_REQUIRE(sr > 0 && std::isfinite(sr), "%s: sr = %g is not positive", fn, sr);
    return DS_OK;
}

using ds::aligned;

}  // namespace

// the kernel of NM modes per lane, NM = the power of two at or above ceil(m / 64), and of K terms
#define NLBANK_DISPATCH_K(NM, K, LAUNCH) \
    do {                                 \
        if ((K) == 1) {                  \
            LAUNCH(NM, 1);               \
        } else if ((K) == 2) {           \
            LAUNCH(NM, 2);               \
        } else if ((K) == 3) {           \
            LAUNCH(NM, 3);               \
        } else {                         \
            LAUNCH(NM, 4);               \
        }                                \
    } while (0)
#define NLBANK_DISPATCH(m, K, LAUNCH)            \
    do {                                         \
        const int nm_ = ((m) + 63) / 64;         \
        if (nm_ <= 1) {                          \
            NLBANK_DISPATCH_K(1, K, LAUNCH);     \
        } else if (nm_ <= 2) {                   \
            NLBANK_DISPATCH_K(2, K, LAUNCH);     \
        } else if (nm_ <= 4) {                   \
            NLBANK_DISPATCH_K(4, K, LAUNCH);     \
        } else {                                 \
            NLBANK_DISPATCH_K(8, K, LAUNCH);     \
        }                                        \
    } while (0)

static_assert(DS_NLBANK_MAX_TERMS == 4 && DS_NLBANK_MAX_MODES == 512, "the dispatch above covers K <= 4 and 8 modes a lane");

extern "C" int64_t ds_nlbank_workspace_bytes(int A, int m, int K, int S, int R) {
    if (!shape_ok(A, m, K, S, R)) return 0;
    // the checkpoints, one segment a clip, the per-clip (gd, gw) partials; the per-clip gC partials
    return (int64_t)sizeof(double2) * ((int64_t)A * S * m + (int64_t)A * R * m + (int64_t)A * m) +
           (int64_t)sizeof(double) * (int64_t)A * K * m;
}

extern "C" int ds_nlbank_fwd(const double* d, const double* w, const double* gain, const double* amp, const double* f,
                             const double* C, const double* gamma, int A, int m, int K, int F, int S, int R, double sr, float* y,
                             ds_stream_t stream) {
    if (int rc = check_args("ds_nlbank_fwd", d && w && gain && amp && f && C && gamma && y, A, m, K, F, S, R, sr)) return rc;
    DS_REQUIRE(aligned(d, 8) && aligned(w, 8) && aligned(gain, 8) && aligned(amp, 8) && aligned(f, 8) && aligned(C, 8) &&
                   aligned(gamma, 8) && aligned(y, 4),
               "ds_nlbank_fwd: misaligned operand");
    hipStream_t st = ds::as_stream(stream);
    const double h = 1.0 / (sr * (double)R);
#define LAUNCH(NM, KK) \
    nlbank_fwd_kernel<NM, KK, false><<<(unsigned)A, 64, 0, st>>>(d, w, gain, amp, f, C, gamma, m, F, S, R, h, sr, y, nullptr)
    NLBANK_DISPATCH(m, K, LAUNCH);
#undef LAUNCH
    DS_LAUNCH_CHECK("nlbank_fwd_kernel");
    return DS_OK;
}

extern "C" int ds_nlbank_bwd(const float* gy, const double* d, const double* w, const double* gain, const double* amp,
                             const double* f, const double* C, const double* gamma, int A, int m, int K, int F, int S, int R,
                             double sr, void* work, int64_t work_bytes, double* gd, double* gw, double* ggain, double* gamp,
                             double* gf, double* gC, double* ggamma, ds_stream_t stream) {
    if (int rc = check_args("ds_nlbank_bwd", gy && d && w && gain && amp && f && C && gamma && work, A, m, K, F, S, R, sr))
        return rc;
    DS_REQUIRE(!gd == !gw, "ds_nlbank_bwd: gd and gw go together");
    DS_REQUIRE(work_bytes >= ds_nlbank_workspace_bytes(A, m, K, S, R), "ds_nlbank_bwd: workspace of %lld bytes, %lld needed",
               (long long)work_bytes, (long long)ds_nlbank_workspace_bytes(A, m, K, S, R));
    DS_REQUIRE(aligned(work, 16), "ds_nlbank_bwd: work not 16-byte aligned");
    DS_REQUIRE(aligned(d, 8) && aligned(w, 8) && aligned(gain, 8) && aligned(amp, 8) && aligned(f, 8) && aligned(C, 8) &&
                   aligned(gamma, 8) && aligned(gy, 4) && aligned(gd, 8) && aligned(gw, 8) && aligned(ggain, 8) &&
                   aligned(gamp, 8) && aligned(gf, 8) && aligned(gC, 8) && aligned(ggamma, 8),
               "ds_nlbank_bwd: misaligned operand");
    hipStream_t st = ds::as_stream(stream);
    const double h = 1.0 / (sr * (double)R);
    double2* ckpt = static_cast<double2*>(work);
    double2* seg = ckpt + (int64_t)A * S * m;
    double2* part2 = seg + (int64_t)A * R * m;
    double* partC = gC ? reinterpret_cast<double*>(part2 + (int64_t)A * m) : nullptr;
    double2* part = gd ? part2 : nullptr;
#define LAUNCH(NM, KK) \
    nlbank_fwd_kernel<NM, KK, true><<<(unsigned)A, 64, 0, st>>>(d, w, gain, amp, f, C, gamma, m, F, S, R, h, sr, nullptr, ckpt)
    NLBANK_DISPATCH(m, K, LAUNCH);
#undef LAUNCH
    DS_LAUNCH_CHECK("nlbank_fwd_kernel");
#define LAUNCH(NM, KK)                                                                                                         \
    nlbank_bwd_kernel<NM, KK><<<(unsigned)A, 64, 0, st>>>(gy, d, w, gain, amp, f, C, gamma, m, F, S, R, h, sr, ckpt, seg, part, \
                                                         partC, ggain, gamp, gf, ggamma)
    NLBANK_DISPATCH(m, K, LAUNCH);
#undef LAUNCH
    DS_LAUNCH_CHECK("nlbank_bwd_kernel");
    if (gd || gC) {
        nlbank_reduce_kernel<<<(unsigned)ds::ceil_div((int64_t)m * K, 64), 64, 0, st>>>(part, partC, A, m, K, gd, gw, gC);
        DS_LAUNCH_CHECK("nlbank_reduce_kernel");
    }
    return DS_OK;
}
