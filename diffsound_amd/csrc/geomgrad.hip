// Geometry backward of the modal read-out - gfx950.
//
//   s(x) = sum_i g_i [ u_i^T K(x) u_i - lambda_i u_i^T M(x) u_i ]          (u_i, lambda_i constants)
//   out  = ds/dx   for the node coordinates x
//
// This is the gradient the reference obtains by autograd through get_vals -> sparse K, M -> coalesce ->
// torch.inverse / torch.det of the per-element transform matrices (reference
// src/diffelastic/diff_model.py:390-399, deform.py:35-68,136-147, mesh.py:58-99), which
// retains every per-Gauss-point intermediate (58 GB at 10k ord-2 tets).  Here nothing is retained: one
// wavefront per element, one lane per mode.  With the affine element map, F = sum_k c_k (x) grad L_k with
// c_k(g) = sum_a dN_a/dL_k(g) u_a, the element energy is  J sum_g w_g [ mu (F:F + F:F^T) + lam tr(F)^2 ],
// so d/d(grad L_k) = J sum_g w_g (2 P(F))^T c_k  and  d/dJ = energy/J - lambda_i rho u^T (M^ (x) I) u.
// The lanes' 14 partial numbers are wave-reduced, lane 0 applies  d(A^-1) = -A^-1 dA A^-1,
// d|det A| = |det A| tr(A^-1 dA)  and scatters 12 fp64 atomics to the four corner nodes
// (mid-edge nodes do not enter the element map).
//
// ds_geometry_grad_tangent: the same gradient for ANY constant tangent C = d vec(P) / d vec(F) (row 3i+j, column 3k+l), the
// stiffness ds_combine_tangent forms (csrc/tangent.hip; reference src/diffelastic/diff_model.py:184-220 assembles A^T C A
// and differentiates it through autograd, :371-399).  The element energy becomes  J sum_g w_g vec(F)^T C vec(F)  and
// dW/dvec(F) = (C + C^T) vec(F) - the exact derivative of the quadratic form also for a C that is symmetric only to
// elastic_tangent's tolerance; S = C + C^T is wave-uniform and lives in LDS.  No atomics: stage 1 leaves every element's 12
// numbers in elem_work, stage 2 sums them per node in the order of the corner-incidence list, one thread per (node,
// component), so two calls give the same bits (as tangent.hip promises for its sums).
#include "ds_common.h"

namespace {

template <int N>
__global__ void __launch_bounds__(256)
    geometry_grad_kernel(const int32_t* __restrict__ tets, int64_t T, const double* __restrict__ tetgeo,
                         const float* __restrict__ U, int64_t ldu, int m, const double* __restrict__ gk,
                         const double* __restrict__ gm, double lam, double mu, const double* __restrict__ gtab,
                         const double* __restrict__ gw, int ng, const double* __restrict__ mtab,
                         double* __restrict__ grad) {
    __shared__ double s_gt[4 * N * 4];  // up to 4 quadrature points
    __shared__ double s_m[N * N];
    for (int i = threadIdx.x; i < ng * N * 4; i += blockDim.x) s_gt[i] = gtab[i];
    for (int i = threadIdx.x; i < N * N; i += blockDim.x) s_m[i] = mtab[i];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t e = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (e >= T) return;  // wave-uniform
    const int32_t* tt = tets + e * N;
    const double* geo = tetgeo + e * 13;
    double G[4][3];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int j = 0; j < 3; ++j) G[k][j] = geo[k * 3 + j];
    const double J = geo[12];

    double dG[4][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    double sW = 0.0, sM = 0.0;
    for (int i = lane; i < m; i += 64) {
        double u[N][3];
#pragma unroll
        for (int a = 0; a < N; ++a) {
            const int64_t row = (int64_t)tt[a] * 3;
#pragma unroll
            for (int d = 0; d < 3; ++d) u[a][d] = (double)U[(row + d) * ldu + i];
        }
        const double gi = gk[i];
        double mass = 0.0;
#pragma unroll
        for (int a = 0; a < N; ++a)
#pragma unroll
            for (int b = 0; b < N; ++b)
                mass += s_m[a * N + b] * (u[a][0] * u[b][0] + u[a][1] * u[b][1] + u[a][2] * u[b][2]);
        sM += gm[i] * mass;
        for (int g = 0; g < ng; ++g) {
            const double* gt = s_gt + g * N * 4;
            double c[4][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
#pragma unroll
            for (int a = 0; a < N; ++a)
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const double w = gt[a * 4 + k];
                    c[k][0] = fma(w, u[a][0], c[k][0]);
                    c[k][1] = fma(w, u[a][1], c[k][1]);
                    c[k][2] = fma(w, u[a][2], c[k][2]);
                }
            double F[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int j = 0; j < 3; ++j) F[r][j] = fma(c[k][r], G[k][j], F[r][j]);
            const double tr = F[0][0] + F[1][1] + F[2][2];
            double W = lam * tr * tr;
            double P2[3][3];  // dW/dF = 2 mu (F + F^T) + 2 lam tr I
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    W += mu * (F[r][j] * F[r][j] + F[r][j] * F[j][r]);
                    P2[r][j] = 2.0 * mu * (F[r][j] + F[j][r]) + (r == j ? 2.0 * lam * tr : 0.0);
                }
            const double wg = gw[g] * gi;
            sW = fma(wg, W, sW);
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int j = 0; j < 3; ++j)
                    dG[k][j] += wg * (P2[0][j] * c[k][0] + P2[1][j] * c[k][1] + P2[2][j] * c[k][2]);
        }
    }
    sW = ds::wave_sum(sW);
    sM = ds::wave_sum(sM);
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int j = 0; j < 3; ++j) dG[k][j] = ds::wave_sum(dG[k][j]);
    if (lane != 0) return;
    // s_e = J * sW(G) - J * sM ;  G_3 = -(G_0 + G_1 + G_2) ;  rows of A^-1 are G_0..2
    double B[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int j = 0; j < 3; ++j) B[k][j] = J * (dG[k][j] - dG[3][j]);
    // dS/dA = -Ainv^T B Ainv^T + (sW - sM) J Ainv^T      (Ainv[k][j] = G[k][j])
    double Tm[3][3];  // Tm = B Ainv^T : Tm[k][r] = sum_j B[k][j] Ainv[r][j]
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int r = 0; r < 3; ++r) Tm[k][r] = B[k][0] * G[r][0] + B[k][1] * G[r][1] + B[k][2] * G[r][2];
    const double sj = (sW - sM) * J;
    double dA[3][3];  // dA[r][c] : derivative w.r.t. A[r][c] = p_c[r] - p_3[r]
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            // (Ainv^T Tm)[r][c] = sum_k Ainv[k][r] Tm[k][c]
            const double t = G[0][r] * Tm[0][c] + G[1][r] * Tm[1][c] + G[2][r] * Tm[2][c];
            dA[r][c] = -t + sj * G[c][r];
        }
    const int cs[4] = {0, N == 4 ? 1 : 2, N == 4 ? 2 : 4, N == 4 ? 3 : 9};
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        double s3 = 0.0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            atomicAdd(&grad[(int64_t)tt[cs[c]] * 3 + r], dA[r][c]);
            s3 += dA[r][c];
        }
        atomicAdd(&grad[(int64_t)tt[cs[3]] * 3 + r], -s3);
    }
}

struct SymTangent {
    double s[81];  // C + C^T, row 3i+j, column 3k+l
};

// Stage 1.  geometry_grad_kernel with the energy of a general tangent; the element's dS/d(corner c, component r) goes to
// elem_work[e * 12 + c * 3 + r] with a plain store.
template <int N>
__global__ void __launch_bounds__(256)
    geometry_grad_tangent_kernel(const int32_t* __restrict__ tets, int64_t T, const double* __restrict__ tetgeo,
                                 const float* __restrict__ U, int64_t ldu, int m, const double* __restrict__ gk,
                                 const double* __restrict__ gm, const SymTangent S, const double* __restrict__ gtab,
                                 const double* __restrict__ gw, int ng, const double* __restrict__ mtab,
                                 double* __restrict__ elem_work) {
    __shared__ double s_gt[4 * N * 4];  // up to 4 quadrature points
    __shared__ double s_m[N * N];
    __shared__ double s_c[81];
    for (int i = threadIdx.x; i < ng * N * 4; i += blockDim.x) s_gt[i] = gtab[i];
    for (int i = threadIdx.x; i < N * N; i += blockDim.x) s_m[i] = mtab[i];
    for (int i = threadIdx.x; i < 81; i += blockDim.x) s_c[i] = S.s[i];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t e = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (e >= T) return;  // wave-uniform
    const int32_t* tt = tets + e * N;
    const double* geo = tetgeo + e * 13;
    double G[4][3];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int j = 0; j < 3; ++j) G[k][j] = geo[k * 3 + j];
    const double J = geo[12];

    double dG[4][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    double sW = 0.0, sM = 0.0;
    for (int i = lane; i < m; i += 64) {
        float u[N][3];  // kept in fp32 (half the registers of the ord-2 element) and promoted where it is used
#pragma unroll
        for (int a = 0; a < N; ++a) {
            const int64_t row = (int64_t)tt[a] * 3;
#pragma unroll
            for (int d = 0; d < 3; ++d) u[a][d] = U[(row + d) * ldu + i];
        }
        const double gi = gk[i];
        double mass = 0.0;
#pragma unroll
        for (int a = 0; a < N; ++a)
#pragma unroll
            for (int b = 0; b < N; ++b)
                mass += s_m[a * N + b] * ((double)u[a][0] * (double)u[b][0] + (double)u[a][1] * (double)u[b][1] +
                                          (double)u[a][2] * (double)u[b][2]);
        sM += gm[i] * mass;
        for (int g = 0; g < ng; ++g) {
            // S is read from LDS at every point.  The 81 reads are loop-invariant and the compiler hoists them: 162 VGPRs
            // that spill the ord-2 element to scratch.  The empty statement emits no instruction; its memory clobber only
            // keeps the reads (s_gt's too) inside the loop.  Reading S through a volatile pointer does the same in words of
            // the language alone but serialises the reads and leaves 368 bytes of scratch per lane.  With AMD clang 22.0.0
            // (ROCm 7.2): 222 / 256 VGPRs for N = 4 / 10, no scratch - which tests/test_geomgrad_tangent_build_cpu.py reads
            // off the built library, so a compiler that brings the spills back is noticed.
            asm volatile("" ::: "memory");
            const double* gt = s_gt + g * N * 4;
            double c[4][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
#pragma unroll
            for (int a = 0; a < N; ++a)
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const double w = gt[a * 4 + k];
                    c[k][0] = fma(w, (double)u[a][0], c[k][0]);
                    c[k][1] = fma(w, (double)u[a][1], c[k][1]);
                    c[k][2] = fma(w, (double)u[a][2], c[k][2]);
                }
            double F[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};  // vec(F), entry 3r+j
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int j = 0; j < 3; ++j) F[3 * r + j] = fma(c[k][r], G[k][j], F[3 * r + j]);
            double P2[9];  // dW/dvec(F) = (C + C^T) vec(F) ;  W = vec(F)^T C vec(F) = vec(F) . P2 / 2
            double W = 0.0;
#pragma unroll
            for (int p = 0; p < 9; ++p) {
                double acc = 0.0;
#pragma unroll
                for (int q = 0; q < 9; ++q) acc = fma(s_c[p * 9 + q], F[q], acc);
                P2[p] = acc;
                W = fma(F[p], acc, W);
            }
            const double wg = gw[g] * gi;
            sW = fma(0.5 * wg, W, sW);
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int j = 0; j < 3; ++j)
                    dG[k][j] += wg * (P2[j] * c[k][0] + P2[3 + j] * c[k][1] + P2[6 + j] * c[k][2]);
        }
    }
    sW = ds::wave_sum(sW);
    sM = ds::wave_sum(sM);
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int j = 0; j < 3; ++j) dG[k][j] = ds::wave_sum(dG[k][j]);
    if (lane != 0) return;
    // as geometry_grad_kernel: s_e = J * sW(G) - J * sM ;  G_3 = -(G_0 + G_1 + G_2) ;  rows of A^-1 are G_0..2
    double B[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int j = 0; j < 3; ++j) B[k][j] = J * (dG[k][j] - dG[3][j]);
    double Tm[3][3];  // Tm = B Ainv^T
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int r = 0; r < 3; ++r) Tm[k][r] = B[k][0] * G[r][0] + B[k][1] * G[r][1] + B[k][2] * G[r][2];
    const double sj = (sW - sM) * J;
    double* o = elem_work + e * 12;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        double s3 = 0.0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            // dS/dA[r][c] = -(Ainv^T Tm)[r][c] + sj Ainv[c][r] ,  A[r][c] = p_c[r] - p_3[r]
            const double t = G[0][r] * Tm[0][c] + G[1][r] * Tm[1][c] + G[2][r] * Tm[2][c];
            const double d = -t + sj * G[c][r];
            o[c * 3 + r] = d;
            s3 += d;
        }
        o[9 + r] = -s3;
    }
}

// Stage 2.  grad[node][r] = sum over the node's (element * 4 + corner) incidences, in the order of the list; 0 for a node
// without one (mid-edge nodes, unreferenced nodes).
__global__ void geometry_grad_gather_kernel(const int32_t* __restrict__ cinc_ptr, const int32_t* __restrict__ cinc,
                                            int64_t nv, int64_t T, const double* __restrict__ elem_work,
                                            double* __restrict__ grad) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nv * 3) return;
    const int64_t node = t / 3;
    const int r = (int)(t - node * 3);
    double acc = 0.0;
    // The list is NOT validated against tets, here or on the host: the ranges are clamped to the 4 T entries and T * 12
    // numbers there are, so a list of another topology reads nothing else - and gives wrong sums without an error.
    const int64_t k1 = min<int64_t>(cinc_ptr[node + 1], 4 * T);
    for (int64_t k = max(cinc_ptr[node], 0); k < k1; ++k) {
        const int64_t ec = cinc[k];
        if (ec >= 0 && ec < 4 * T) acc += elem_work[ec * 3 + r];
    }
    grad[t] = acc;
}

}  // namespace

extern "C" int ds_geometry_grad(const int32_t* tets, int64_t T, int N, int64_t nv, const double* tetgeo, const float* U,
                                int64_t ldu, int m, const double* gk, const double* gm, double lam, double mu,
                                const double* gtab, const double* gw, int ng, const double* mtab, double* grad,
                                ds_stream_t stream) {
    DS_REQUIRE(tets && tetgeo && U && gk && gm && gtab && gw && mtab && grad, "ds_geometry_grad: null pointer");
    DS_REQUIRE(N == 4 || N == 10, "ds_geometry_grad: N must be 4 or 10 (got %d)", N);
    DS_REQUIRE(T > 0 && nv > 0 && m > 0 && ldu >= m, "ds_geometry_grad: bad sizes");
    DS_REQUIRE(ng >= 1 && ng <= 4, "ds_geometry_grad: 1..4 quadrature points supported (got %d)", ng);
    hipStream_t st = ds::as_stream(stream);
    const unsigned grid = (unsigned)ds::ceil_div(T, 4);
    if (N == 4)
        geometry_grad_kernel<4><<<grid, 256, 0, st>>>(tets, T, tetgeo, U, ldu, m, gk, gm, lam, mu, gtab, gw, ng, mtab, grad);
    else
        geometry_grad_kernel<10><<<grid, 256, 0, st>>>(tets, T, tetgeo, U, ldu, m, gk, gm, lam, mu, gtab, gw, ng, mtab, grad);
    DS_LAUNCH_CHECK("geometry_grad_kernel");
    return DS_OK;
}

extern "C" int ds_geometry_grad_tangent(const int32_t* tets, int64_t T, int N, int64_t nv, const double* tetgeo,
                                        const float* U, int64_t ldu, int m, const double* gk, const double* gm,
                                        const double* C, const double* gtab, const double* gw, int ng, const double* mtab,
                                        const int32_t* cinc_ptr, const int32_t* cinc, double* elem_work, double* grad,
                                        ds_stream_t stream) {
    DS_REQUIRE(tets && tetgeo && U && gk && gm && C && gtab && gw && mtab && cinc_ptr && cinc && elem_work && grad,
               "ds_geometry_grad_tangent: null pointer");
    DS_REQUIRE(N == 4 || N == 10, "ds_geometry_grad_tangent: N must be 4 or 10 (got %d)", N);
    DS_REQUIRE(ng >= 1 && ng <= 4, "ds_geometry_grad_tangent: 1..4 quadrature points supported (got %d)", ng);
    DS_REQUIRE(T > 0 && nv > 0 && m > 0, "ds_geometry_grad_tangent: bad sizes (T = %lld, nv = %lld, m = %d)", (long long)T,
               (long long)nv, m);
    DS_REQUIRE(4 * T <= (int64_t)0x7FFFFFFF && nv <= (int64_t)0x7FFFFFFF,
               "ds_geometry_grad_tangent: %lld elements, %lld nodes: int32 ids hold 2^31 - 1", (long long)T, (long long)nv);
    DS_REQUIRE(ldu >= m, "ds_geometry_grad_tangent: ldu = %lld is less than m = %d", (long long)ldu, m);
    SymTangent S;
    for (int e = 0; e < 81; ++e) {
        DS_REQUIRE(C[e] == C[e] && C[e] - C[e] == 0.0, "ds_geometry_grad_tangent: C[%d] is not finite", e);
    }
    for (int p = 0; p < 9; ++p)
        for (int q = 0; q < 9; ++q) S.s[p * 9 + q] = C[p * 9 + q] + C[q * 9 + p];
    DS_REQUIRE((uintptr_t)U % 4 == 0, "ds_geometry_grad_tangent: U is not 4-byte aligned");
    DS_REQUIRE((uintptr_t)tetgeo % 8 == 0 && (uintptr_t)gk % 8 == 0 && (uintptr_t)gm % 8 == 0 && (uintptr_t)gtab % 8 == 0 &&
                   (uintptr_t)gw % 8 == 0 && (uintptr_t)mtab % 8 == 0 && (uintptr_t)elem_work % 8 == 0 &&
                   (uintptr_t)grad % 8 == 0,
               "ds_geometry_grad_tangent: tetgeo, gk, gm, gtab, gw, mtab, elem_work and grad must be 8-byte aligned");
    hipStream_t st = ds::as_stream(stream);
    const unsigned grid = (unsigned)ds::ceil_div(T, 4);
    if (N == 4)
        geometry_grad_tangent_kernel<4><<<grid, 256, 0, st>>>(tets, T, tetgeo, U, ldu, m, gk, gm, S, gtab, gw, ng, mtab,
                                                              elem_work);
    else
        geometry_grad_tangent_kernel<10><<<grid, 256, 0, st>>>(tets, T, tetgeo, U, ldu, m, gk, gm, S, gtab, gw, ng, mtab,
                                                               elem_work);
    DS_LAUNCH_CHECK("geometry_grad_tangent_kernel");
    geometry_grad_gather_kernel<<<(unsigned)ds::ceil_div(nv * 3, 256), 256, 0, st>>>(cinc_ptr, cinc, nv, T, elem_work, grad);
    DS_LAUNCH_CHECK("geometry_grad_gather_kernel");
    return DS_OK;
}
