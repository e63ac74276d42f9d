// A general (anisotropic) elasticity tangent on the assembled geometry tensors - gfx950.
//
// assemble_blocks_kernel (assemble.hip) leaves in klam the full geometry tensor of every block slot,
//   H_ab[j][l] = integral dN_a/dx_j dN_b/dx_l .
// With the reference's convention F_ij = sum_b dN_b/dx_j u_b,i and vec(F) row 3i+j (src/diffelastic/diff_model.py:
// 207-211) the block of ANY constant tangent C = d vec(P) / d vec(F) is
//   K_ab[i][k] = sum_jl C[3i+j][3k+l] H_ab[j][l]                                   (ds_combine_tangent)
// and the strain-energy moment tensor of a displacement field u,
//   Q[3i+j][3k+l] = sum_ab u_a,i H_ab[j][l] u_b,k ,   u^T K(C) u = <C, Q> ,         (ds_tangent_forms)
// makes every quadratic form of K(C) an 81-term dot product.  No atomics; every sum has one fixed order.
#include "ds_common.h"

namespace {

struct Tangent {
    double c[81];  // row 3i+j, column 3k+l
};

// K[3i+k] = sum_j sum_l C[3i+j][3k+l] H[3j+l], j outer, l inner
__device__ __forceinline__ void contract_block(const Tangent& C, const double* H, double* K) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            double acc = 0.0;
#pragma unroll
            for (int j = 0; j < 3; ++j)
#pragma unroll
                for (int l = 0; l < 3; ++l) acc = fma(C.c[(3 * i + j) * 9 + 3 * k + l], H[3 * j + l], acc);
            K[3 * i + k] = acc;
        }
}

// One thread per block slot.  The 9 doubles of a slot are contiguous and the slots of neighbouring lanes 72 (36) bytes
// apart: as in assemble_blocks_kernel the workgroup's 256 x 9 values come in and leave through LDS as whole rows.
__global__ void __launch_bounds__(256) combine_tangent_kernel(const double* __restrict__ klam,
                                                              const double* __restrict__ ms, int64_t nnzb,
                                                              const Tangent C, double* __restrict__ k64,
                                                              float* __restrict__ k32, float* __restrict__ k32t,
                                                              float* __restrict__ ms32) {
    __shared__ double sBuf[256 * 9];
    const int64_t s0 = (int64_t)blockIdx.x * 256;
    const int64_t s = s0 + threadIdx.x;
    const int nval = (int)min<int64_t>(256, nnzb - s0) * 9;
    for (int e = threadIdx.x; e < nval; e += 256) sBuf[e] = klam[s0 * 9 + e];
    __syncthreads();
    double H[9], K[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) H[e] = threadIdx.x * 9 + e < nval ? sBuf[threadIdx.x * 9 + e] : 0.0;
    contract_block(C, H, K);
    if (k64) {
        __syncthreads();  // (every H has been read)
#pragma unroll
        for (int e = 0; e < 9; ++e) sBuf[threadIdx.x * 9 + e] = K[e];
        __syncthreads();
        for (int e = threadIdx.x; e < nval; e += 256) k64[s0 * 9 + e] = sBuf[e];
    }
    float* sF = reinterpret_cast<float*>(sBuf);
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        float* dst = pass == 0 ? k32 : k32t;
        if (!dst) continue;
        __syncthreads();  // (sBuf has been drained)
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int k = 0; k < 3; ++k) sF[threadIdx.x * 9 + 3 * i + k] = (float)(pass == 0 ? K[3 * i + k] : K[3 * k + i]);
        __syncthreads();
        for (int e = threadIdx.x; e < nval; e += 256) dst[s0 * 9 + e] = sF[e];
    }
    if (s < nnzb) ms32[s] = (float)ms[s];
}

// The fp32 inverse of the fp64 diagonal blocks, the arithmetic of diag_inverse_kernel (assemble.hip) on K = C : H.
__global__ void diag_inverse_tangent_kernel(const double* __restrict__ klam, const int32_t* __restrict__ diagidx,
                                            int64_t nv, const Tangent C, float* __restrict__ dinv) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nv) return;
    const int d = diagidx[i];
    float* o = dinv + i * 9;
    if (d < 0) {  // node not referenced by any element: identity keeps the preconditioner defined
        for (int k = 0; k < 9; ++k) o[k] = (k % 4 == 0) ? 1.f : 0.f;
        return;
    }
    double H[9], a[9];
    for (int k = 0; k < 9; ++k) H[k] = klam[(int64_t)d * 9 + k];
    contract_block(C, H, a);
    const double c0 = a[4] * a[8] - a[5] * a[7];
    const double c1 = a[5] * a[6] - a[3] * a[8];
    const double c2 = a[3] * a[7] - a[4] * a[6];
    const double id = 1.0 / (a[0] * c0 + a[1] * c1 + a[2] * c2);
    o[0] = (float)(c0 * id);
    o[1] = (float)((a[2] * a[7] - a[1] * a[8]) * id);
    o[2] = (float)((a[1] * a[5] - a[2] * a[4]) * id);
    o[3] = (float)(c1 * id);
    o[4] = (float)((a[0] * a[8] - a[2] * a[6]) * id);
    o[5] = (float)((a[2] * a[3] - a[0] * a[5]) * id);
    o[6] = (float)(c2 * id);
    o[7] = (float)((a[1] * a[6] - a[0] * a[7]) * id);
    o[8] = (float)((a[0] * a[4] - a[1] * a[3]) * id);
}

constexpr int TF_ROWS = 64;  // rows of the pattern per workgroup of the first stage (= per partial sum)
constexpr int TF_COLS = 9;   // columns of U per workgroup: 9 x 27 = 243 of its 256 threads work

// Stage 1.  Thread (column c, w = (j, l, k)) of workgroup (row range p, column group): for every row a of the range
//   W = sum_{b in row a} H_ab[j][l] u_b,k        (ascending slots)
// and its three entries (i = 0..2) of the partial Q take u_a,i W, rows ascending.  The 27 threads of a column read the
// 9 doubles of one slot and 3 floats of U between them; nothing is shared between threads, so a column's numbers do
// not depend on the other columns of the call.
__global__ void __launch_bounds__(256) tangent_forms_rows_kernel(const int32_t* __restrict__ rowptr,
                                                                 const int32_t* __restrict__ colidx,
                                                                 const double* __restrict__ klam, int64_t nv,
                                                                 const float* __restrict__ U, int64_t ldu, int m,
                                                                 double* __restrict__ part) {
    const int cl = threadIdx.x / 27, w = threadIdx.x - cl * 27;
    const int64_t c = (int64_t)blockIdx.y * TF_COLS + cl;
    if (cl >= TF_COLS || c >= m) return;
    const int j = w / 9, l = (w / 3) % 3, k = w % 3;
    const int64_t a0 = (int64_t)blockIdx.x * TF_ROWS, a1 = min<int64_t>(nv, a0 + TF_ROWS);
    double q0 = 0.0, q1 = 0.0, q2 = 0.0;
    for (int64_t a = a0; a < a1; ++a) {
        double W = 0.0;
        const int e1 = rowptr[a + 1];
        for (int e = rowptr[a]; e < e1; ++e) {
            const int64_t b = colidx[e];
            W = fma(klam[(int64_t)e * 9 + 3 * j + l], (double)U[(3 * b + k) * ldu + c], W);
        }
        const float* ua = U + 3 * a * ldu + c;
        q0 = fma((double)ua[0], W, q0);
        q1 = fma((double)ua[ldu], W, q1);
        q2 = fma((double)ua[2 * ldu], W, q2);
    }
    double* o = part + ((int64_t)blockIdx.x * m + c) * 81 + 3 * k + l;
    o[(0 + j) * 9] = q0;
    o[(3 + j) * 9] = q1;
    o[(6 + j) * 9] = q2;
}

// Stage 2.  Q[c][e] = sum over the row ranges p, ascending.
__global__ void tangent_forms_reduce_kernel(const double* __restrict__ part, int64_t nparts, int64_t total,
                                            double* __restrict__ Q) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    double acc = 0.0;
    for (int64_t p = 0; p < nparts; ++p) acc += part[p * total + t];
    Q[t] = acc;
}

}  // namespace

extern "C" int ds_combine_tangent(const double* klam, const double* ms, int64_t nnzb, const int32_t* diagidx, int64_t nv,
                                  const double* C, double* k64, float* k32, float* k32t, float* ms32, float* dinv32,
                                  ds_stream_t stream) {
    DS_REQUIRE(klam && ms && diagidx && C && k32 && ms32 && dinv32, "ds_combine_tangent: null pointer");
    DS_REQUIRE(nnzb > 0 && nv > 0, "ds_combine_tangent: empty problem");
    DS_REQUIRE(nnzb <= (int64_t)0x7FFFFFFF, "ds_combine_tangent: %lld block slots, int32 slot ids hold 2^31 - 1",
               (long long)nnzb);
    Tangent t;
    for (int e = 0; e < 81; ++e) {
        DS_REQUIRE(C[e] == C[e] && C[e] - C[e] == 0.0, "ds_combine_tangent: C[%d] is not finite", e);
        t.c[e] = C[e];
    }
    hipStream_t st = ds::as_stream(stream);
    combine_tangent_kernel<<<(unsigned)ds::ceil_div(nnzb, 256), 256, 0, st>>>(klam, ms, nnzb, t, k64, k32, k32t, ms32);
    DS_LAUNCH_CHECK("combine_tangent_kernel");
    diag_inverse_tangent_kernel<<<(unsigned)ds::ceil_div(nv, 256), 256, 0, st>>>(klam, diagidx, nv, t, dinv32);
    DS_LAUNCH_CHECK("diag_inverse_tangent_kernel");
    return DS_OK;
}

extern "C" size_t ds_tangent_forms_workspace_bytes(int64_t nv, int m) {
    if (nv <= 0 || m <= 0) return 0;
    return (size_t)ds::ceil_div(nv, TF_ROWS) * (size_t)m * 81 * sizeof(double);
}

extern "C" int ds_tangent_forms(const int32_t* rowptr, const int32_t* colidx, const double* klam, int64_t nv,
                                const float* U, int64_t ldu, int m, double* Q, void* work, size_t work_bytes,
                                ds_stream_t stream) {
    DS_REQUIRE(rowptr && colidx && klam && U && Q && work, "ds_tangent_forms: null pointer");
    DS_REQUIRE(nv > 0, "ds_tangent_forms: empty problem");
    DS_REQUIRE(m > 0 && m <= DS_TANGENT_FORMS_MAX_COLS, "ds_tangent_forms: m = %d columns, 1 .. %d are served", m,
               DS_TANGENT_FORMS_MAX_COLS);
    DS_REQUIRE(ldu >= m, "ds_tangent_forms: ldu = %lld is less than m = %d", (long long)ldu, m);
    DS_REQUIRE((uintptr_t)U % 4 == 0, "ds_tangent_forms: U is not 4-byte aligned");
    DS_REQUIRE((uintptr_t)klam % 8 == 0 && (uintptr_t)Q % 8 == 0 && (uintptr_t)work % 8 == 0,
               "ds_tangent_forms: klam, Q and work must be 8-byte aligned");
    const size_t need = ds_tangent_forms_workspace_bytes(nv, m);
    DS_REQUIRE(work_bytes >= need, "ds_tangent_forms: workspace of %zu bytes, %zu needed", work_bytes, need);
    hipStream_t st = ds::as_stream(stream);
    const int64_t nparts = ds::ceil_div(nv, TF_ROWS);
    DS_REQUIRE(nparts <= (int64_t)0x7FFFFFFF, "ds_tangent_forms: %lld nodes are too many", (long long)nv);
    double* part = static_cast<double*>(work);
    const dim3 grid((unsigned)nparts, (unsigned)ds::ceil_div(m, TF_COLS));
    tangent_forms_rows_kernel<<<grid, 256, 0, st>>>(rowptr, colidx, klam, nv, U, ldu, m, part);
    DS_LAUNCH_CHECK("tangent_forms_rows_kernel");
    const int64_t total = (int64_t)m * 81;
    tangent_forms_reduce_kernel<<<(unsigned)ds::ceil_div(total, 256), 256, 0, st>>>(part, nparts, total, Q);
    DS_LAUNCH_CHECK("tangent_forms_reduce_kernel");
    return DS_OK;
}
