// Deformation gradient at the Gauss points and its adjoint, the stress -> nodal force gather - gfx950.  Replaces the
// reference's Deform (src/diffelastic/deform.py:35-68 tables, :70-102 gradient, :104-125 + :149-180 force), which
// materialises the physical shape gradients B (T*G, N, 3) and an index map (T*G*N*3) and scatters with atomics.
// DESIGN.md section 13 has the scheme.
//
// Nothing per Gauss point is stored.  With A_t the element's edge matrix (columns v1-v4, v2-v4, v3-v4 of the corner
// nodes, fp32 like the reference's transform_matrix) and D[g] = dN/dL[g] @ dL/dx (G, N, 3), a constant table,
//
//   B[t,g] = D[g] inv(A_t)                                     (ds_deform_tables writes it out, for API parity only)
//   F[b,t,g] = (sum_a u[b,tet[t,a],:] (x) D[g,a,:]) inv(A_t)                                     (ds_deform_gradient)
//   fe[b,t,a,i] = sum_g sum_k D[g,a,k] (w[t,g] P[b,t,g] inv(A_t)^T)[i,k]       (ds_deform_force, element pass)
//   f[b,3 n+i] = sum over the incidences (t,a) of node n, in list order, of fe[b,t,a,i]      (.., node pass)
//
// inv(A_t) is the adjugate over the determinant, recomputed per element per launch from the four corner coordinates;
// the 2x2 minors use Kahan's fused difference of products, so a sliver element loses no more than the reference's
// pivoted fp32 LU does.
//
// Launch shape: a workgroup owns E consecutive elements (E*G <= 256 (element, Gauss point) pairs, one per lane) and
// walks up to COLS batch columns; inv(A_t), w and the lane's rows of D are formed once and reused over the columns.
// A column's tile of F (or P) is contiguous in memory (E*G*9 floats): it passes through LDS so that global memory
// sees 16-byte accesses, with the LDS image shifted by (global float index mod 4) so that both sides are aligned.
//
// Order of the arithmetic: every output element is one fixed sequence of fp32 operations on its own column's data -
// over the local nodes a, then k (gradient); over j, then the Gauss points g in index order, then k (element pass);
// over the node's incidence list in (t, a) order (node pass).  No atomics, no dependence on the batch size or on the
// column's position: two calls give the same bits, and so does a column computed alone.
// fp32 throughout, with contraction off: every fused multiply-add below is written out.
#include <cmath>

#include "ds_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int WG = 256;
constexpr int COLS = 8;  // batch columns per workgroup

template <int ORDER>
struct Elem;
template <>
struct Elem<1> {
    static constexpr int N = 4, G = 27, E = 8;
    static constexpr int corner(int c) { return c; }
};
template <>
struct Elem<2> {
    static constexpr int N = 10, G = 64, E = 4;
    static constexpr int corner(int c) { return c == 0 ? 0 : c == 1 ? 2 : c == 2 ? 4 : 9; }
};

// a b - c d with the rounding error of c d recovered (Kahan)
__device__ __forceinline__ float diff_of_products(float a, float b, float c, float d) {
    const float w = c * d;
    const float e = fmaf(-c, d, w);
    const float f = fmaf(a, b, -w);
    return f + e;
}

// inv (row-major 3x3) and det of A = [p0-p3, p1-p3, p2-p3] (columns); p: the four corners
__device__ __forceinline__ float edge_matrix_inverse(const float (&p)[4][3], float (&inv)[9]) {
    float a[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) a[r][c] = p[c][r] - p[3][r];
    float adj[9];
    adj[0] = diff_of_products(a[1][1], a[2][2], a[1][2], a[2][1]);
    adj[1] = diff_of_products(a[0][2], a[2][1], a[0][1], a[2][2]);
    adj[2] = diff_of_products(a[0][1], a[1][2], a[0][2], a[1][1]);
    adj[3] = diff_of_products(a[1][2], a[2][0], a[1][0], a[2][2]);
    adj[4] = diff_of_products(a[0][0], a[2][2], a[0][2], a[2][0]);
    adj[5] = diff_of_products(a[0][2], a[1][0], a[0][0], a[1][2]);
    adj[6] = diff_of_products(a[1][0], a[2][1], a[1][1], a[2][0]);
    adj[7] = diff_of_products(a[0][1], a[2][0], a[0][0], a[2][1]);
    adj[8] = diff_of_products(a[0][0], a[1][1], a[0][1], a[1][0]);
    const float det = fmaf(a[0][2], adj[6], fmaf(a[0][1], adj[3], a[0][0] * adj[0]));
#pragma unroll
    for (int k = 0; k < 9; ++k) inv[k] = adj[k] / det;
    return det;
}

template <int ORDER>
__device__ __forceinline__ float element_geometry(const float* __restrict__ verts, const int32_t* __restrict__ tet,
                                                  float (&inv)[9]) {
    float p[4][3];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int64_t n = tet[Elem<ORDER>::corner(c)];
#pragma unroll
        for (int r = 0; r < 3; ++r) p[c][r] = verts[3 * n + r];
    }
    return edge_matrix_inverse(p, inv);
}

// The part of every hot kernel that does not depend on the column: the table D as float4 rows in LDS, the tile's
// node ids, and per element inv(A) and |det A|.
template <int ORDER>
struct Tile {
    static constexpr int N = Elem<ORDER>::N, G = Elem<ORDER>::G, E = Elem<ORDER>::E;
    float4 d[G * N];   // D[g][a] = (k0, k1, k2, 0)
    float inv[E][12];  // 9 used
    float absdet[E];
    int32_t node[E * N];
};

template <int ORDER>
__device__ __forceinline__ void tile_setup(Tile<ORDER>& s, const float* __restrict__ verts,
                                           const int32_t* __restrict__ tets, int64_t t0, int ne,
                                           const float* __restrict__ dtab) {
    using L = Elem<ORDER>;
    const int tid = threadIdx.x;
    for (int i = tid; i < L::G * L::N; i += WG) s.d[i] = make_float4(dtab[3 * i], dtab[3 * i + 1], dtab[3 * i + 2], 0.f);
    for (int i = tid; i < ne * L::N; i += WG) s.node[i] = tets[t0 * L::N + i];
    if (tid < ne) {
        float inv[9];
        const float det = element_geometry<ORDER>(verts, tets + (t0 + tid) * L::N, inv);
#pragma unroll
        for (int k = 0; k < 9; ++k) s.inv[tid][k] = inv[k];
        s.absdet[tid] = fabsf(det);
    }
}

// A contiguous run of `count` floats of global memory starting at float index `base`, against its LDS image
// `img`, which holds the run from img[base & 3] on: both sides of every whole quad are 16-byte aligned.
template <bool STORE>
__device__ __forceinline__ void move_tile(float* __restrict__ glob, int64_t base, int count, float* img) {
    const int off = (int)(base & 3);
    float* g0 = glob + (base - off);  // 16-byte aligned: the caller's pointer is
    const int quads = (off + count + 3) >> 2;
    for (int q = threadIdx.x; q < quads; q += WG) {
        const int lo = 4 * q, hi = lo + 4;
        if (lo >= off && hi <= off + count) {
            if (STORE)
                *reinterpret_cast<float4*>(g0 + lo) = *reinterpret_cast<const float4*>(img + lo);
            else
                *reinterpret_cast<float4*>(img + lo) = *reinterpret_cast<const float4*>(g0 + lo);
        } else {
            for (int i = max(lo, off); i < min(hi, off + count); ++i) {
                if (STORE)
                    g0[i] = img[i];
                else
                    img[i] = g0[i];
            }
        }
    }
}

template <int ORDER>
__global__ __launch_bounds__(WG) void deform_gradient_kernel(const float* __restrict__ verts,
                                                            const int32_t* __restrict__ tets, int64_t T,
                                                            const float* __restrict__ dtab,
                                                            const float* __restrict__ gw, const float* __restrict__ u,
                                                            int64_t nv, int64_t batch, int weighted,
                                                            float* __restrict__ F) {
    using L = Elem<ORDER>;
    constexpr int N = L::N, G = L::G, E = L::E, TILE = E * G * 9;
    __shared__ Tile<ORDER> s;
    __shared__ float su[E * N * 3];
    __shared__ __attribute__((aligned(16))) float sout[2][TILE + 4];
    const int tid = threadIdx.x;
    const int64_t t0 = (int64_t)blockIdx.x * E;
    const int ne = (int)min((int64_t)E, T - t0);
    tile_setup<ORDER>(s, verts, tets, t0, ne, dtab);
    __syncthreads();
    const bool active = tid < ne * G;
    const int e = active ? tid / G : 0, g = tid - e * G;
    float inv[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) inv[k] = s.inv[e][k];
    const float w = weighted ? gw[active ? g : 0] * s.absdet[e] : 1.f;
    const int64_t b0 = (int64_t)blockIdx.y * COLS, b1 = min(batch, b0 + COLS);
    for (int64_t b = b0; b < b1; ++b) {
        for (int i = tid; i < ne * N * 3; i += WG) su[i] = u[(b * nv + s.node[i / 3]) * 3 + i % 3];
        __syncthreads();
        const int64_t base = (b * T + t0) * (G * 9);
        float* img = sout[b & 1];
        if (active) {
            float h[3][3] = {};
#pragma unroll
            for (int a = 0; a < N; ++a) {
                const float4 d = s.d[g * N + a];
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const float ui = su[(e * N + a) * 3 + i];
                    h[i][0] = fmaf(ui, d.x, h[i][0]);
                    h[i][1] = fmaf(ui, d.y, h[i][1]);
                    h[i][2] = fmaf(ui, d.z, h[i][2]);
                }
            }
            float* o = img + (int)(base & 3) + tid * 9;
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const float f = fmaf(h[i][2], inv[6 + j], fmaf(h[i][1], inv[3 + j], h[i][0] * inv[j]));
                    o[3 * i + j] = weighted ? f * w : f;
                }
        }
        __syncthreads();
        // (the next column writes the other image and refills su, which this column has finished reading)
        move_tile<true>(F, base, ne * G * 9, img);
    }
}

template <int ORDER>
__global__ __launch_bounds__(WG) void deform_element_force_kernel(const float* __restrict__ verts,
                                                                 const int32_t* __restrict__ tets, int64_t T,
                                                                 const float* __restrict__ dtab,
                                                                 const float* __restrict__ gw,
                                                                 const float* __restrict__ P, int64_t batch,
                                                                 int weighted, float* __restrict__ work) {
    using L = Elem<ORDER>;
    constexpr int N = L::N, G = L::G, E = L::E, TILE = E * G * 9;
    __shared__ Tile<ORDER> s;
    __shared__ __attribute__((aligned(16))) float sp[TILE + 4];
    __shared__ float4 sq[E * G * 3];  // (w P inv^T)[e][g][i] = (k0, k1, k2, 0)
    const int tid = threadIdx.x;
    const int64_t t0 = (int64_t)blockIdx.x * E;
    const int ne = (int)min((int64_t)E, T - t0);
    tile_setup<ORDER>(s, verts, tets, t0, ne, dtab);
    __syncthreads();
    const bool active = tid < ne * G;
    const int e = active ? tid / G : 0, g = tid - e * G;
    float inv[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) inv[k] = s.inv[e][k];
    const float w = weighted ? gw[active ? g : 0] * s.absdet[e] : 1.f;
    // the reduction's lanes: one per (element, local node, component)
    const bool reducer = tid < ne * N * 3;
    const int re = reducer ? tid / (N * 3) : 0, ra = reducer ? (tid / 3) % N : 0, ri = tid % 3;
    const int64_t b0 = (int64_t)blockIdx.y * COLS, b1 = min(batch, b0 + COLS);
    for (int64_t b = b0; b < b1; ++b) {
        const int64_t base = (b * T + t0) * (G * 9);
        move_tile<false>(const_cast<float*>(P), base, ne * G * 9, sp);
        __syncthreads();
        if (active) {
            const float* p = sp + (int)(base & 3) + tid * 9;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const float p0 = p[3 * i], p1 = p[3 * i + 1], p2 = p[3 * i + 2];
                float q[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    q[k] = fmaf(p2, inv[3 * k + 2], fmaf(p1, inv[3 * k + 1], p0 * inv[3 * k]));
                    if (weighted) q[k] *= w;
                }
                sq[tid * 3 + i] = make_float4(q[0], q[1], q[2], 0.f);
            }
        }
        __syncthreads();
        // (the next column's tile lands in sp, which every lane has finished reading; sq is rewritten behind the
        // next barrier, which the reducing lanes reach only when they are done with it)
        if (reducer) {
            float acc = 0.f;
            for (int gg = 0; gg < G; ++gg) {
                const float4 d = s.d[gg * N + ra];
                const float4 q = sq[(re * G + gg) * 3 + ri];
                acc = fmaf(d.z, q.z, fmaf(d.y, q.y, fmaf(d.x, q.x, acc)));
            }
            work[(b * T + t0) * (N * 3) + tid] = acc;
        }
    }
}

// f[b, 3 n + i] = the node's incidences summed in list order; work is (batch, T*N, 3).
__global__ __launch_bounds__(WG) void deform_node_gather_kernel(const float* __restrict__ work, int64_t slots,
                                                               const int32_t* __restrict__ inc_ptr,
                                                               const int32_t* __restrict__ inc, int64_t nv,
                                                               float* __restrict__ f) {
    const int64_t n = (int64_t)blockIdx.x * WG + threadIdx.x;
    if (n >= nv) return;
    const int64_t b = blockIdx.y;
    const float* wb = work + b * slots * 3;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    const int32_t e1 = inc_ptr[n + 1];
    for (int32_t e = inc_ptr[n]; e < e1; ++e) {
        const float* c = wb + (int64_t)inc[e] * 3;
        a0 += c[0];
        a1 += c[1];
        a2 += c[2];
    }
    float* o = f + (b * nv + n) * 3;
    o[0] = a0;
    o[1] = a1;
    o[2] = a2;
}

template <int ORDER>
__global__ __launch_bounds__(WG) void deform_tables_kernel(const float* __restrict__ verts,
                                                          const int32_t* __restrict__ tets, int64_t T,
                                                          const float* __restrict__ dtab,
                                                          const float* __restrict__ gw, float* __restrict__ sfd,
                                                          float* __restrict__ intw, float* __restrict__ det_out) {
    using L = Elem<ORDER>;
    constexpr int N = L::N, G = L::G;
    const int64_t q = (int64_t)blockIdx.x * WG + threadIdx.x;  // t * G + g
    if (q >= T * G) return;
    const int64_t t = q / G;
    const int g = (int)(q - t * G);
    float inv[9];
    const float det = element_geometry<ORDER>(verts, tets + t * N, inv);
    if (det_out && g == 0) det_out[t] = det;
    if (intw) intw[q] = gw[g] * fabsf(det);
    if (sfd) {
        float* o = sfd + q * (N * 3);
        for (int a = 0; a < N; ++a) {
            const float* d = dtab + (g * N + a) * 3;
#pragma unroll
            for (int j = 0; j < 3; ++j) o[3 * a + j] = fmaf(d[2], inv[6 + j], fmaf(d[1], inv[3 + j], d[0] * inv[j]));
        }
    }
}

// one limit for both operators, each being the other's backward: the node pass has one grid row per column
constexpr int64_t MAX_BATCH = 65535;

int check_mesh(const char* who, const void* verts, const void* tets, const void* dtab, const void* gw, int64_t nv,
               int64_t T, int order) {
    DS_REQUIRE(verts && tets && dtab && gw, "%s: null pointer", who);
    DS_REQUIRE(order == 1 || order == 2, "%s: order must be 1 or 2 (got %d)", who, order);
    // T * G * 9 and T * N * 3 index LDS tiles and int32 incidence slots
    DS_REQUIRE(nv >= 1 && T >= 1 && nv < (1ll << 31) / 3 && T < (1ll << 31) / 30, "%s: bad sizes nv=%lld T=%lld", who,
               (long long)nv, (long long)T);
    return DS_OK;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" int ds_deform_tables(const float* verts, int64_t nv, const int32_t* tets, int64_t T, int order,
                                const float* dtab, const float* gw, float* sfd, float* intw, float* det,
                                ds_stream_t stream) {
    if (int rc = check_mesh("ds_deform_tables", verts, tets, dtab, gw, nv, T, order)) return rc;
    const int G = order == 1 ? Elem<1>::G : Elem<2>::G;
    const dim3 grid((unsigned)ds::ceil_div(T * G, WG));
    if (order == 1)
        deform_tables_kernel<1><<<grid, dim3(WG), 0, ds::as_stream(stream)>>>(verts, tets, T, dtab, gw, sfd, intw, det);
    else
        deform_tables_kernel<2><<<grid, dim3(WG), 0, ds::as_stream(stream)>>>(verts, tets, T, dtab, gw, sfd, intw, det);
    DS_LAUNCH_CHECK("ds_deform_tables");
    return DS_OK;
}

extern "C" int ds_deform_gradient(const float* verts, int64_t nv, const int32_t* tets, int64_t T, int order,
                                  const float* dtab, const float* gw, const float* u, int64_t batch, int weighted,
                                  float* F, ds_stream_t stream) {
    if (int rc = check_mesh("ds_deform_gradient", verts, tets, dtab, gw, nv, T, order)) return rc;
    DS_REQUIRE(batch >= 0 && batch <= MAX_BATCH, "ds_deform_gradient: bad batch %lld", (long long)batch);
    if (batch == 0) return DS_OK;
    DS_REQUIRE(u && F, "ds_deform_gradient: null pointer");
    DS_REQUIRE(aligned16(F), "ds_deform_gradient: F not 16-byte aligned");
    const int E = order == 1 ? Elem<1>::E : Elem<2>::E;
    const dim3 grid((unsigned)ds::ceil_div(T, E), (unsigned)ds::ceil_div(batch, COLS));
    if (order == 1)
        deform_gradient_kernel<1><<<grid, dim3(WG), 0, ds::as_stream(stream)>>>(verts, tets, T, dtab, gw, u, nv, batch,
                                                                                weighted, F);
    else
        deform_gradient_kernel<2><<<grid, dim3(WG), 0, ds::as_stream(stream)>>>(verts, tets, T, dtab, gw, u, nv, batch,
                                                                                weighted, F);
    DS_LAUNCH_CHECK("ds_deform_gradient");
    return DS_OK;
}

extern "C" int ds_deform_force(const float* verts, int64_t nv, const int32_t* tets, int64_t T, int order,
                               const float* dtab, const float* gw, const int32_t* inc_ptr, const int32_t* inc,
                               const float* P, int64_t batch, int weighted, float* work, float* f,
                               ds_stream_t stream) {
    if (int rc = check_mesh("ds_deform_force", verts, tets, dtab, gw, nv, T, order)) return rc;
    DS_REQUIRE(batch >= 0 && batch <= MAX_BATCH, "ds_deform_force: bad batch %lld", (long long)batch);
    if (batch == 0) return DS_OK;
    DS_REQUIRE(inc_ptr && inc && P && work && f, "ds_deform_force: null pointer");
    DS_REQUIRE(aligned16(P), "ds_deform_force: P not 16-byte aligned");
    const int E = order == 1 ? Elem<1>::E : Elem<2>::E, N = order == 1 ? Elem<1>::N : Elem<2>::N;
    const dim3 grid((unsigned)ds::ceil_div(T, E), (unsigned)ds::ceil_div(batch, COLS));
    hipStream_t st = ds::as_stream(stream);
    if (order == 1)
        deform_element_force_kernel<1><<<grid, dim3(WG), 0, st>>>(verts, tets, T, dtab, gw, P, batch, weighted, work);
    else
        deform_element_force_kernel<2><<<grid, dim3(WG), 0, st>>>(verts, tets, T, dtab, gw, P, batch, weighted, work);
    DS_LAUNCH_CHECK("ds_deform_force (elements)");
    deform_node_gather_kernel<<<dim3((unsigned)ds::ceil_div(nv, WG), (unsigned)batch), dim3(WG), 0, st>>>(
        work, T * N, inc_ptr, inc, nv, f);
    DS_LAUNCH_CHECK("ds_deform_force (nodes)");
    return DS_OK;
}
