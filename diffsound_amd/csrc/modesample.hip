// Mode shapes sampled at points of the mesh: the modal gains of a strike - gfx950.
//
//   out[p, i] = sum_a N_a(L_p) sum_c dir[p, c] U[3 tets[elem_p, a] + c, i]          c_i = d . u_i(p)
//
// A strike at a point p of the body with direction d excites mode i with the gain d . u_i(p), u_i the mass-orthonormal
// mode shape.  The reference has no such map: its oscillator modules hold ``amp`` as a free parameter
// (src/ddsp/oscillator.py:76) that nothing ties to the mode shapes.  This unit evaluates the finite-element interpolant
// of U at (element, barycentric) pairs, and the gradient of a loss on the gains with respect to the barycentrics and
// the direction.
//
// THERE IS NO GRADIENT TO U: the eigenvectors are constants everywhere in this project (the read-out differentiates
// the eigenvalues with the vectors held fixed), and so they are here.
//
// Element ids (0 <= elem < T) and node ids (0 <= tets < nv) are NOT checked, here or on the host: they are the
// caller's to check, as for ds_deform_gradient and ds_deform_force (diffsound_amd/impact.py does check them).
//
// Shape functions, in fp64 from the fp32 L, in the local node order of fem_tables.py:
//   P1 (N = 4)   N_a = L_a
//   P2 (N = 10)  corners (slots 0, 2, 4, 9 = L_0..3)  N = L (2 L - 1),  dN/dL = 4 L - 1
//                mid-edge (slot: pair) 1: (0,1)  3: (1,2)  5: (2,0)  6: (0,3)  7: (1,3)  8: (2,3)   N = 4 L_p L_q
//
// Mapping.  One wavefront per point, lane l owns the mode columns l, l + 64, ...: the gather is N * 3 rows of U, m
// contiguous doubles each, and a wave instruction reads 64 consecutive doubles of one row.  The point's element, L,
// direction and node ids are wave-uniform.  Forward: every out / vec element is written by the one lane that computed
// it.  Backward: a lane sums its own columns in ascending order, the 64 partial sums meet in an xor butterfly
// (ds::wave_sum) and lane 0 stores; a point belongs to one wave, so there is no second stage and there are no atomics:
// two calls give the same bits (as bem.hip and the tangent form of geomgrad.hip promise for theirs).
#include <cstdint>

#include "ds_common.h"

namespace {

// P2 slot tables (fem_tables._CORNER / _MID)
__device__ constexpr int kCornerSlot[4] = {0, 2, 4, 9};
__device__ constexpr int kMidSlot[6] = {1, 3, 5, 6, 7, 8};
__device__ constexpr int kMidP[6] = {0, 1, 2, 0, 1, 2};
__device__ constexpr int kMidQ[6] = {1, 2, 0, 3, 3, 3};

template <int N>
__device__ __forceinline__ void shape_values(const double (&l)[4], double (&sv)[N]) {
    if constexpr (N == 4) {
#pragma unroll
        for (int a = 0; a < 4; ++a) sv[a] = l[a];
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) sv[kCornerSlot[k]] = l[k] * (2.0 * l[k] - 1.0);
#pragma unroll
        for (int e = 0; e < 6; ++e) sv[kMidSlot[e]] = 4.0 * l[kMidP[e]] * l[kMidQ[e]];
    }
}

// sum_a dN_a/dL_j w_a for j = 0..3
template <int N>
__device__ __forceinline__ void shape_gradient_dot(const double (&l)[4], const double (&w)[N], double (&g)[4]) {
    if constexpr (N == 4) {
#pragma unroll
        for (int j = 0; j < 4; ++j) g[j] = w[j];
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) g[k] = (4.0 * l[k] - 1.0) * w[kCornerSlot[k]];
#pragma unroll
        for (int e = 0; e < 6; ++e) {
            g[kMidP[e]] = fma(4.0 * l[kMidQ[e]], w[kMidSlot[e]], g[kMidP[e]]);
            g[kMidQ[e]] = fma(4.0 * l[kMidP[e]], w[kMidSlot[e]], g[kMidQ[e]]);
        }
    }
}

template <int N>
__global__ void __launch_bounds__(256)
    mode_sample_fwd_kernel(const int32_t* __restrict__ tets, const double* __restrict__ U, int64_t ldu, int m,
                           const int32_t* __restrict__ elem, const float* __restrict__ L, const float* __restrict__ dir,
                           int64_t P, double* __restrict__ out, double* __restrict__ vec) {
    const int lane = threadIdx.x & 63;
    const int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= P) return;  // wave-uniform
    const int32_t* tt = tets + (int64_t)elem[p] * N;
    double l[4], sv[N];
#pragma unroll
    for (int k = 0; k < 4; ++k) l[k] = (double)L[p * 4 + k];
    shape_values<N>(l, sv);
    int64_t row[N];
#pragma unroll
    for (int a = 0; a < N; ++a) row[a] = (int64_t)tt[a] * 3 * ldu;
    double d[3] = {0.0, 0.0, 0.0};
    if (out) {
#pragma unroll
        for (int c = 0; c < 3; ++c) d[c] = (double)dir[p * 3 + c];
    }
    for (int i = lane; i < m; i += 64) {
        double v[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int a = 0; a < N; ++a) {
            const double* u = U + row[a] + i;
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = fma(sv[a], u[c * ldu], v[c]);
        }
        if (out) out[p * m + i] = fma(d[2], v[2], fma(d[1], v[1], d[0] * v[0]));
        if (vec) {
            double* o = vec + (p * m + i) * 3;
            o[0] = v[0];
            o[1] = v[1];
            o[2] = v[2];
        }
    }
}

template <int N>
__global__ void __launch_bounds__(256)
    mode_sample_bwd_kernel(const int32_t* __restrict__ tets, const double* __restrict__ U, int64_t ldu, int m,
                           const int32_t* __restrict__ elem, const float* __restrict__ L, const float* __restrict__ dir,
                           int64_t P, const double* __restrict__ gout, double* __restrict__ gL,
                           double* __restrict__ gdir) {
    const int lane = threadIdx.x & 63;
    const int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= P) return;  // wave-uniform
    const int32_t* tt = tets + (int64_t)elem[p] * N;
    double l[4], sv[N], d[3];
#pragma unroll
    for (int k = 0; k < 4; ++k) l[k] = (double)L[p * 4 + k];
#pragma unroll
    for (int c = 0; c < 3; ++c) d[c] = (double)dir[p * 3 + c];
    shape_values<N>(l, sv);
    int64_t row[N];
#pragma unroll
    for (int a = 0; a < N; ++a) row[a] = (int64_t)tt[a] * 3 * ldu;
    double sl[4] = {0.0, 0.0, 0.0, 0.0}, sd[3] = {0.0, 0.0, 0.0};
    for (int i = lane; i < m; i += 64) {
        const double g = gout[p * m + i];
        double w[N];  // dir . U[node_a, :, i]
        double v[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int a = 0; a < N; ++a) {
            const double* u = U + row[a] + i;
            const double u0 = u[0], u1 = u[ldu], u2 = u[2 * ldu];
            w[a] = fma(d[2], u2, fma(d[1], u1, d[0] * u0));
            v[0] = fma(sv[a], u0, v[0]);
            v[1] = fma(sv[a], u1, v[1]);
            v[2] = fma(sv[a], u2, v[2]);
        }
        double gj[4];
        shape_gradient_dot<N>(l, w, gj);
#pragma unroll
        for (int j = 0; j < 4; ++j) sl[j] = fma(g, gj[j], sl[j]);
#pragma unroll
        for (int c = 0; c < 3; ++c) sd[c] = fma(g, v[c], sd[c]);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) sl[j] = ds::wave_sum(sl[j]);
#pragma unroll
    for (int c = 0; c < 3; ++c) sd[c] = ds::wave_sum(sd[c]);
    if (lane != 0) return;
    if (gL) {
#pragma unroll
        for (int j = 0; j < 4; ++j) gL[p * 4 + j] = sl[j];
    }
    if (gdir) {
#pragma unroll
        for (int c = 0; c < 3; ++c) gdir[p * 3 + c] = sd[c];
    }
}

int check_common(const char* fn, const int32_t* tets, int64_t T, int N, int64_t nv, const double* U, int64_t ldu, int m,
                 const int32_t* elem, const float* L, int64_t P) {
    DS_REQUIRE(tets && U && elem && L, "%s: null pointer", fn);
    DS_REQUIRE(N == 4 || N == 10, "%s: N must be 4 or 10 (got %d)", fn, N);
    DS_REQUIRE(P > 0 && m > 0 && T > 0 && nv > 0, "%s: bad sizes (P = %lld, m = %d, T = %lld, nv = %lld)", fn, (long long)P,
               m, (long long)T, (long long)nv);
    DS_REQUIRE(ldu >= m, "%s: ldu = %lld is less than m = %d", fn, (long long)ldu, m);
    DS_REQUIRE(T <= (int64_t)0x7FFFFFFF && nv <= (int64_t)0x7FFFFFFF && (P + 3) / 4 <= (int64_t)0x7FFFFFFF,
               "%s: %lld elements, %lld nodes, %lld points: int32 ids and the launch grid hold 2^31 - 1", fn, (long long)T,
               (long long)nv, (long long)P);
    DS_REQUIRE((uintptr_t)tets % 4 == 0 && (uintptr_t)elem % 4 == 0 && (uintptr_t)L % 4 == 0,
               "%s: tets, elem and L must be 4-byte aligned", fn);
    return DS_OK;
}

}  // namespace

extern "C" int ds_mode_sample_fwd(const int32_t* tets, int64_t T, int N, int64_t nv, const double* U, int64_t ldu, int m,
                                  const int32_t* elem, const float* L, const float* dir, int64_t P, double* out,
                                  double* vec, ds_stream_t stream) {
    if (int rc = check_common("ds_mode_sample_fwd", tets, T, N, nv, U, ldu, m, elem, L, P)) return rc;
    DS_REQUIRE(out || vec, "ds_mode_sample_fwd: null pointer (out and vec both)");
    DS_REQUIRE(!out || dir, "ds_mode_sample_fwd: null pointer (out needs dir)");
    DS_REQUIRE((uintptr_t)dir % 4 == 0, "ds_mode_sample_fwd: dir must be 4-byte aligned");
    DS_REQUIRE((uintptr_t)U % 8 == 0 && (uintptr_t)out % 8 == 0 && (uintptr_t)vec % 8 == 0,
               "ds_mode_sample_fwd: U, out and vec must be 8-byte aligned");
    const unsigned grid = (unsigned)ds::ceil_div(P, 4);
    hipStream_t st = ds::as_stream(stream);
    if (N == 4)
        mode_sample_fwd_kernel<4><<<grid, 256, 0, st>>>(tets, U, ldu, m, elem, L, dir, P, out, vec);
    else
        mode_sample_fwd_kernel<10><<<grid, 256, 0, st>>>(tets, U, ldu, m, elem, L, dir, P, out, vec);
    DS_LAUNCH_CHECK("mode_sample_fwd_kernel");
    return DS_OK;
}

extern "C" int ds_mode_sample_bwd(const int32_t* tets, int64_t T, int N, int64_t nv, const double* U, int64_t ldu, int m,
                                  const int32_t* elem, const float* L, const float* dir, int64_t P, const double* gout,
                                  double* gL, double* gdir, ds_stream_t stream) {
    if (int rc = check_common("ds_mode_sample_bwd", tets, T, N, nv, U, ldu, m, elem, L, P)) return rc;
    DS_REQUIRE(dir && gout, "ds_mode_sample_bwd: null pointer");
    DS_REQUIRE(gL || gdir, "ds_mode_sample_bwd: null pointer (gL and gdir both)");
    DS_REQUIRE((uintptr_t)dir % 4 == 0, "ds_mode_sample_bwd: dir must be 4-byte aligned");
    DS_REQUIRE((uintptr_t)U % 8 == 0 && (uintptr_t)gout % 8 == 0 && (uintptr_t)gL % 8 == 0 && (uintptr_t)gdir % 8 == 0,
               "ds_mode_sample_bwd: U, gout, gL and gdir must be 8-byte aligned");
    const unsigned grid = (unsigned)ds::ceil_div(P, 4);
    hipStream_t st = ds::as_stream(stream);
    if (N == 4)
        mode_sample_bwd_kernel<4><<<grid, 256, 0, st>>>(tets, U, ldu, m, elem, L, dir, P, gout, gL, gdir);
    else
        mode_sample_bwd_kernel<10><<<grid, 256, 0, st>>>(tets, U, ldu, m, elem, L, dir, P, gout, gL, gdir);
    DS_LAUNCH_CHECK("mode_sample_bwd_kernel");
    return DS_OK;
}
