// Differentiable marching tetrahedra (DMTet) - gfx950.  Replaces the torch op chain of the reference's
// DMTet.__call__ (src/dmtet/geometry/dmtet_geometry.py:115-272, dmtet_thickness.py:99-200,
// dmtet_interpolate.py:115-205): occupancy, valid tets, the unique crossing edges, the interpolated vertices, the
// split tets, the surface faces and the final torch.unique compaction.  The outputs are the reference's bit for bit
// (vertex numbering, tet order, orientation); DESIGN.md section 10 has the ordering argument.
//
// Per-grid tables (built once per grid by the caller, diffsound_amd/dmtet.py): the distinct edges sorted by (a, b)
// (ds_edge_table), each tet's six edge ids in DMTet's local order [01, 02, 03, 12, 13, 23], and a vertex ->
// incident-edge CSR.  A crossing edge (exactly one end occupied) always lies in a valid tet, so numbering the
// crossing edges in this static order IS the reference's torch.unique(dim=0) numbering of them.
//
// Occupancy: lo < s <= hi with lo = 0; hi = +inf for the plain variant, hi = *thick for the thickness variant,
// which also subtracts t from both ends of a crossing edge whose ends are both > 0 (dmtet_thickness.py:137).
//
//   ds_mt_count    per tet: the class and its counts (1-tet sides, 3-tet sides, inner tets, faces); per edge: the
//                  crossing flag; per vertex: the "used" flag; exclusive scans (rocPRIM); ONE count record back to
//                  the host - the only synchronisation of a forward.
//   ds_mt_emit     compacted vertices (used grid vertices ascending, then edge vertices), tets (int64), faces,
//                  and the two source maps the backward needs.  No host round trip.
//   ds_mt_backward dL/dpos, dL/dsdf by a gather over the CSR; dL/dt by fixed-order partial sums.  No atomics.
#include <cmath>

#include <rocprim/device/device_scan.hpp>

#include "ds_common.h"

namespace {

// The published marching-tets tables of DMTet (Shen et al. 2021, as in kaolin's tetmesh conversion).  Class bit k =
// local vertex k occupied.  Local slots 0-3 are the tet's vertices, 4-9 the points on its edges [01,02,03,12,13,23].
__constant__ int8_t TRI_TABLE[16][6] = {
    {-1, -1, -1, -1, -1, -1}, {1, 0, 2, -1, -1, -1}, {4, 0, 3, -1, -1, -1}, {1, 4, 2, 1, 3, 4},
    {3, 1, 5, -1, -1, -1},    {2, 3, 0, 2, 5, 3},    {1, 4, 0, 1, 5, 4},    {4, 2, 5, -1, -1, -1},
    {4, 5, 2, -1, -1, -1},    {4, 1, 0, 4, 5, 1},    {3, 2, 0, 3, 5, 2},    {1, 3, 5, -1, -1, -1},
    {4, 1, 2, 4, 3, 1},       {3, 0, 4, -1, -1, -1}, {2, 0, 1, -1, -1, -1}, {-1, -1, -1, -1, -1, -1}};
__constant__ int8_t TET_TABLE[16][12] = {
    {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {0, 4, 5, 6, -1, -1, -1, -1, -1, -1, -1, -1},
    {1, 4, 8, 7, -1, -1, -1, -1, -1, -1, -1, -1},     {7, 1, 8, 6, 5, 1, 7, 6, 5, 0, 1, 6},
    {2, 5, 7, 9, -1, -1, -1, -1, -1, -1, -1, -1},     {4, 0, 6, 7, 9, 0, 7, 6, 7, 0, 9, 2},
    {4, 1, 9, 8, 5, 1, 9, 4, 5, 1, 2, 9},             {6, 0, 1, 2, 8, 6, 1, 2, 9, 6, 8, 2},
    {3, 6, 9, 8, -1, -1, -1, -1, -1, -1, -1, -1},     {5, 0, 4, 8, 5, 0, 8, 3, 5, 8, 9, 3},
    {1, 4, 7, 3, 4, 7, 6, 3, 9, 6, 7, 3},             {0, 1, 5, 3, 5, 1, 9, 3, 5, 1, 7, 9},
    {5, 2, 3, 7, 3, 6, 5, 8, 3, 5, 7, 8},             {0, 4, 7, 8, 0, 3, 8, 7, 0, 3, 7, 2},
    {4, 1, 2, 3, 4, 3, 2, 5, 4, 3, 5, 6},             {0, 1, 2, 3, -1, -1, -1, -1, -1, -1, -1, -1}};
// triangles per class: 0 for classes 0 and 15, 2 when two vertices are occupied, else 1
__device__ __forceinline__ int n_tri(int c) { return (c == 0 || c == 15) ? 0 : (__popc(c) == 2 ? 2 : 1); }

constexpr int BLK = 256;

// per-tet counts, scanned as one record: the output rows each tet writes in every section
struct MtCnt {
    int32_t s1, s3, in, f1, f2;  // 1-tet side rows, 3-tet side rows (3 per tet), inner rows, 1-face rows, 2-face rows
};
struct MtAdd {
    __host__ __device__ MtCnt operator()(const MtCnt& a, const MtCnt& b) const {
        return {a.s1 + b.s1, a.s3 + b.s3, a.in + b.in, a.f1 + b.f1, a.f2 + b.f2};
    }
};

__device__ __forceinline__ bool occ(float s, float hi) { return s > 0.f && s <= hi; }
__device__ __forceinline__ float band_hi(const float* thick) { return thick ? *thick : INFINITY; }

__device__ __forceinline__ int tet_class(const int32_t* tets, int64_t t, const float* sdf, float hi) {
    int c = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) c |= occ(sdf[tets[4 * t + k]], hi) ? (1 << k) : 0;
    return c;
}

__device__ __forceinline__ bool vert_used(const float* sdf, const int32_t* vptr, int64_t v, float hi) {
    return occ(sdf[v], hi) && vptr[v + 1] > vptr[v];
}

// The SDF pair an edge vertex interpolates, after the thickness variant's shift.
__device__ __forceinline__ void edge_sdf(const float* sdf, int32_t a, int32_t b, const float* thick, float hi, float& sa,
                                         float& sb, bool& shifted) {
    sa = sdf[a], sb = sdf[b];
    shifted = thick != nullptr && sa > 0.f && sb > 0.f;
    if (shifted) sa = sa - hi, sb = sb - hi;
}

// The reference's fp32 formula, operation for operation: w_a = (-s_b)/(s_a - s_b), w_b = s_a/(s_a - s_b),
// v = p_a w_a + p_b w_b (flip / divide / multiply / two-term sum), never contracted into an FMA.
__device__ __forceinline__ void interp(const float* pa, const float* pb, float sa, float sb, float* v) {
#pragma clang fp contract(off)
    const float d = sa + (-sb);
    const float wa = -sb / d, wb = sa / d;  // IEEE division (this library keeps the correctly rounded fp32 divide)
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = pa[c] * wa + pb[c] * wb;
}

// Closed-form VJP of one edge vertex: g = dL/dv -> dL/dp_a, dL/dp_b, dL/ds_a, dL/ds_b (s after the shift).
//   dv/dp_a = w_a, dv/dp_b = w_b, dv/ds_a = (p_a - p_b) s_b / d^2, dv/ds_b = -(p_a - p_b) s_a / d^2
__device__ __forceinline__ void edge_vjp(const float* pa, const float* pb, float sa, float sb, const float* g, float* gpa,
                                         float* gpb, float& gsa, float& gsb) {
    const float d = sa - sb;
    const float wa = -sb / d, wb = sa / d;
    float q = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        gpa[c] = g[c] * wa;
        gpb[c] = g[c] * wb;
        q += g[c] * (pa[c] - pb[c]);
    }
    const float r = q / d / d;
    gsa = r * sb;
    gsb = -(r * sa);
}

// ------------------------------------------------------------------ count
__global__ void __launch_bounds__(BLK) mt_flags_kernel(const float* __restrict__ sdf, int64_t n,
                                                       const int32_t* __restrict__ tets, int64_t T,
                                                       const int32_t* __restrict__ ea, const int32_t* __restrict__ eb,
                                                       int64_t E, const int32_t* __restrict__ vptr,
                                                       const float* __restrict__ thick, MtCnt* __restrict__ tcnt,
                                                       int32_t* __restrict__ eflag, int32_t* __restrict__ vflag) {
    const int64_t i = (int64_t)blockIdx.x * BLK + threadIdx.x;
    const float hi = band_hi(thick);
    if (i < T) {
        const int c = tet_class(tets, i, sdf, hi);
        const bool valid = c != 0 && c != 15;
        const int nt = n_tri(c);
        const bool one = c == 1 || c == 2 || c == 4 || c == 8;
        tcnt[i] = {valid && one ? 1 : 0, valid && !one ? 3 : 0, c == 15 ? 1 : 0, nt == 1 ? 1 : 0, nt == 2 ? 2 : 0};
    }
    if (i < E) eflag[i] = occ(sdf[ea[i]], hi) != occ(sdf[eb[i]], hi) ? 1 : 0;
    if (i < n) vflag[i] = vert_used(sdf, vptr, i, hi) ? 1 : 0;
}

__global__ void mt_record_kernel(const MtCnt* tcnt, const MtCnt* toff, int64_t T, const int32_t* eflag,
                                 const int32_t* eid, int64_t E, const int32_t* vflag, const int32_t* vid, int64_t n,
                                 ds_mt_counts_t* rec) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const MtCnt c = MtAdd()(tcnt[T - 1], toff[T - 1]);
    ds_mt_counts_t r;
    r.n_used = vflag[n - 1] + vid[n - 1];
    r.n_cross = eflag[E - 1] + eid[E - 1];
    r.n_side1 = c.s1;
    r.n_side3 = c.s3;
    r.n_inner = c.in;
    r.n_face1 = c.f1;
    r.n_face2 = c.f2;
    r.reserved = 0;
    *rec = r;
}

// ------------------------------------------------------------------ emit
__global__ void __launch_bounds__(BLK) mt_emit_kernel(
    const float* __restrict__ pos, const float* __restrict__ sdf, int64_t n, const int32_t* __restrict__ tets, int64_t T,
    const int32_t* __restrict__ tet_edge, const int32_t* __restrict__ ea, const int32_t* __restrict__ eb, int64_t E,
    const int32_t* __restrict__ vptr, const float* __restrict__ thick, const MtCnt* __restrict__ toff,
    const int32_t* __restrict__ eid, const int32_t* __restrict__ vid, int64_t n_used, int64_t n_side1, int64_t n_side3,
    int64_t n_face1, float* __restrict__ verts, int64_t* __restrict__ out_tets, int64_t* __restrict__ out_faces,
    int32_t* __restrict__ vsrc, int32_t* __restrict__ xedge) {
    const int64_t i = (int64_t)blockIdx.x * BLK + threadIdx.x;
    const float hi = band_hi(thick);
    if (i < n && vert_used(sdf, vptr, i, hi)) {  // kept grid vertex
        const int64_t o = vid[i];
        vsrc[o] = (int32_t)i;
        for (int c = 0; c < 3; ++c) verts[3 * o + c] = pos[3 * i + c];
    }
    if (i < E) {
        const int32_t a = ea[i], b = eb[i];
        if (occ(sdf[a], hi) != occ(sdf[b], hi)) {  // crossing edge -> edge vertex
            const int64_t k = eid[i];
            xedge[k] = (int32_t)i;
            float sa, sb, v[3];
            bool shifted;
            edge_sdf(sdf, a, b, thick, hi, sa, sb, shifted);
            interp(pos + 3 * (int64_t)a, pos + 3 * (int64_t)b, sa, sb, v);
            for (int c = 0; c < 3; ++c) verts[3 * (n_used + k) + c] = v[c];
        }
    }
    if (i < T) {
        const int c = tet_class(tets, i, sdf, hi);
        if (c == 0) return;
        const MtCnt off = toff[i];
        if (c == 15) {
            int64_t* o = out_tets + 4 * (n_side1 + n_side3 + off.in);
            for (int k = 0; k < 4; ++k) o[k] = vid[tets[4 * i + k]];
            return;
        }
        int64_t loc[10];
        for (int k = 0; k < 4; ++k) loc[k] = vid[tets[4 * i + k]];
        for (int k = 0; k < 6; ++k) loc[4 + k] = n_used + eid[tet_edge[6 * i + k]];
        const bool one = c == 1 || c == 2 || c == 4 || c == 8;
        int64_t* o = out_tets + 4 * (one ? off.s1 : n_side1 + off.s3);
        for (int k = 0; k < (one ? 4 : 12); ++k) o[k] = loc[TET_TABLE[c][k]];
        if (out_faces) {
            const int nt = n_tri(c);
            int64_t* f = out_faces + 3 * (nt == 1 ? off.f1 : n_face1 + off.f2);
            for (int k = 0; k < 3 * nt; ++k) f[k] = loc[4 + TRI_TABLE[c][k]] - n_used;
        }
    }
}

// ------------------------------------------------------------------ backward
__global__ void __launch_bounds__(BLK) mt_grad_vertex_kernel(
    const float* __restrict__ gv, const float* __restrict__ pos, const float* __restrict__ sdf, int64_t n,
    const int32_t* __restrict__ ea, const int32_t* __restrict__ eb, const int32_t* __restrict__ vptr,
    const int32_t* __restrict__ vadj, const float* __restrict__ thick, const int32_t* __restrict__ eid,
    const int32_t* __restrict__ vid, int64_t n_used, float* __restrict__ dpos, float* __restrict__ dsdf) {
    const int64_t v = (int64_t)blockIdx.x * BLK + threadIdx.x;
    if (v >= n) return;
    const float hi = band_hi(thick);
    float gp[3] = {0.f, 0.f, 0.f}, gs = 0.f;
    if (vert_used(sdf, vptr, v, hi))
        for (int c = 0; c < 3; ++c) gp[c] = gv[3 * (int64_t)vid[v] + c];
    for (int32_t j = vptr[v]; j < vptr[v + 1]; ++j) {  // incident edges in a fixed order
        const int32_t e = vadj[j], a = ea[e], b = eb[e];
        if (occ(sdf[a], hi) == occ(sdf[b], hi)) continue;
        float sa, sb, gpa[3], gpb[3], gsa, gsb;
        bool shifted;
        edge_sdf(sdf, a, b, thick, hi, sa, sb, shifted);
        edge_vjp(pos + 3 * (int64_t)a, pos + 3 * (int64_t)b, sa, sb, gv + 3 * (n_used + eid[e]), gpa, gpb, gsa, gsb);
        const bool is_a = a == v;
        for (int c = 0; c < 3; ++c) gp[c] += is_a ? gpa[c] : gpb[c];
        gs += is_a ? gsa : gsb;
    }
    for (int c = 0; c < 3; ++c) dpos[3 * v + c] = gp[c];
    dsdf[v] = gs;
}

// dL/dt = -sum over shifted edge vertices of (dL/ds_a + dL/ds_b): per-workgroup tree sums, then one workgroup
// sums the partials in index order.
__device__ __forceinline__ float block_sum(float x, float* sh) {
    sh[threadIdx.x] = x;
    __syncthreads();
    for (int s = BLK / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    return sh[0];
}

__global__ void __launch_bounds__(BLK) mt_grad_thick_kernel(const float* __restrict__ gv, const float* __restrict__ pos,
                                                            const float* __restrict__ sdf, const int32_t* __restrict__ ea,
                                                            const int32_t* __restrict__ eb,
                                                            const int32_t* __restrict__ xedge, int64_t n_cross,
                                                            int64_t n_used, const float* __restrict__ thick,
                                                            float* __restrict__ partial) {
    __shared__ float sh[BLK];
    const int64_t k = (int64_t)blockIdx.x * BLK + threadIdx.x;
    float x = 0.f;
    if (k < n_cross) {
        const int32_t e = xedge[k], a = ea[e], b = eb[e];
        float sa, sb, gpa[3], gpb[3], gsa, gsb;
        bool shifted;
        edge_sdf(sdf, a, b, thick, *thick, sa, sb, shifted);
        if (shifted) {
            edge_vjp(pos + 3 * (int64_t)a, pos + 3 * (int64_t)b, sa, sb, gv + 3 * (n_used + k), gpa, gpb, gsa, gsb);
            x = -(gsa + gsb);
        }
    }
    const float s = block_sum(x, sh);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

__global__ void __launch_bounds__(BLK) mt_grad_thick_final_kernel(const float* __restrict__ partial, int64_t np,
                                                                  float* __restrict__ dt) {
    __shared__ float sh[BLK];
    float x = 0.f;
    for (int64_t j = threadIdx.x; j < np; j += BLK) x += partial[j];
    const float s = block_sum(x, sh);
    if (threadIdx.x == 0) *dt = s;
}

inline unsigned blocks_for(int64_t n) { return (unsigned)ds::ceil_div(n > 0 ? n : 1, (int64_t)BLK); }
inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// workspace layout of ds_mt_count: tcnt | eflag | vflag | record | rocPRIM scratch
struct CountWs {
    size_t tcnt, eflag, vflag, rec, tmp, tmp_bytes, total;
};

int count_layout(int64_t n, int64_t T, int64_t E, CountWs& w) {
    size_t b0 = 0, b1 = 0, b2 = 0;
    int rc;
    if ((rc = ds::check_hip(rocprim::exclusive_scan(nullptr, b0, (const MtCnt*)nullptr, (MtCnt*)nullptr, MtCnt{0, 0, 0, 0, 0},
                                                    (size_t)T, MtAdd(), nullptr),
                            "rocprim::exclusive_scan(size)")) != DS_OK)
        return rc;
    if ((rc = ds::check_hip(rocprim::exclusive_scan(nullptr, b1, (const int32_t*)nullptr, (int32_t*)nullptr, 0, (size_t)E,
                                                    rocprim::plus<int32_t>(), nullptr),
                            "rocprim::exclusive_scan(size)")) != DS_OK)
        return rc;
    if ((rc = ds::check_hip(rocprim::exclusive_scan(nullptr, b2, (const int32_t*)nullptr, (int32_t*)nullptr, 0, (size_t)n,
                                                    rocprim::plus<int32_t>(), nullptr),
                            "rocprim::exclusive_scan(size)")) != DS_OK)
        return rc;
    w.tcnt = 0;
    w.eflag = w.tcnt + align256(sizeof(MtCnt) * (size_t)T);
    w.vflag = w.eflag + align256(sizeof(int32_t) * (size_t)E);
    w.rec = w.vflag + align256(sizeof(int32_t) * (size_t)n);
    w.tmp = w.rec + align256(sizeof(ds_mt_counts_t));
    w.tmp_bytes = std::max(b0, std::max(b1, b2));
    w.total = w.tmp + align256(w.tmp_bytes);
    return DS_OK;
}

bool sizes_ok(int64_t n, int64_t T, int64_t E) {
    const int64_t lim = (int64_t)1 << 30;
    return n > 0 && T > 0 && E > 0 && n < lim && E < lim && 12 * T < lim;
}

}  // namespace

extern "C" int64_t ds_mt_count_workspace_bytes(int64_t n, int64_t T, int64_t E) {
    if (!sizes_ok(n, T, E)) return -1;
    CountWs w;
    if (count_layout(n, T, E, w) != DS_OK) return -1;
    return (int64_t)w.total;
}

extern "C" int ds_mt_count(const float* sdf, int64_t n, const int32_t* tets, int64_t T, const int32_t* ea,
                           const int32_t* eb, int64_t E, const int32_t* vptr, const float* thick, int32_t* toff,
                           int32_t* edge_id, int32_t* vert_id, void* work, int64_t work_bytes, ds_mt_counts_t* counts,
                           ds_stream_t stream) {
    DS_REQUIRE(sdf && tets && ea && eb && vptr && toff && edge_id && vert_id && work && counts,
               "ds_mt_count: null argument");
    DS_REQUIRE(sizes_ok(n, T, E), "ds_mt_count: need 0 < n, E < 2^30 and 0 < 12 T < 2^30 (n=%lld T=%lld E=%lld)",
               (long long)n, (long long)T, (long long)E);
    CountWs w;
    int rc = count_layout(n, T, E, w);
    if (rc != DS_OK) return rc;
    DS_REQUIRE(work_bytes >= (int64_t)w.total, "ds_mt_count: workspace of %lld bytes, need %lld", (long long)work_bytes,
               (long long)w.total);
    hipStream_t st = ds::as_stream(stream);
    char* ws = static_cast<char*>(work);
    auto* tcnt = reinterpret_cast<MtCnt*>(ws + w.tcnt);
    auto* eflag = reinterpret_cast<int32_t*>(ws + w.eflag);
    auto* vflag = reinterpret_cast<int32_t*>(ws + w.vflag);
    auto* rec = reinterpret_cast<ds_mt_counts_t*>(ws + w.rec);
    void* tmp = ws + w.tmp;
    auto* to = reinterpret_cast<MtCnt*>(toff);
    mt_flags_kernel<<<blocks_for(std::max(T, std::max(E, n))), BLK, 0, st>>>(sdf, n, tets, T, ea, eb, E, vptr, thick,
                                                                             tcnt, eflag, vflag);
    DS_LAUNCH_CHECK("mt_flags_kernel");
    size_t b = w.tmp_bytes;
    if ((rc = ds::check_hip(rocprim::exclusive_scan(tmp, b, tcnt, to, MtCnt{0, 0, 0, 0, 0}, (size_t)T, MtAdd(), st),
                            "rocprim::exclusive_scan(tets)")) != DS_OK)
        return rc;
    b = w.tmp_bytes;
    if ((rc = ds::check_hip(rocprim::exclusive_scan(tmp, b, eflag, edge_id, 0, (size_t)E, rocprim::plus<int32_t>(), st),
                            "rocprim::exclusive_scan(edges)")) != DS_OK)
        return rc;
    b = w.tmp_bytes;
    if ((rc = ds::check_hip(rocprim::exclusive_scan(tmp, b, vflag, vert_id, 0, (size_t)n, rocprim::plus<int32_t>(), st),
                            "rocprim::exclusive_scan(vertices)")) != DS_OK)
        return rc;
    mt_record_kernel<<<1, 64, 0, st>>>(tcnt, to, T, eflag, edge_id, E, vflag, vert_id, n, rec);
    DS_LAUNCH_CHECK("mt_record_kernel");
    if ((rc = ds::check_hip(hipMemcpyAsync(counts, rec, sizeof(ds_mt_counts_t), hipMemcpyDeviceToHost, st),
                            "ds_mt_count: count record")) != DS_OK)
        return rc;
    return ds::check_hip(hipStreamSynchronize(st), "ds_mt_count: synchronise");
}

extern "C" int ds_mt_emit(const float* pos, const float* sdf, int64_t n, const int32_t* tets, int64_t T,
                          const int32_t* tet_edge, const int32_t* ea, const int32_t* eb, int64_t E, const int32_t* vptr,
                          const float* thick, const int32_t* toff, const int32_t* edge_id, const int32_t* vert_id,
                          const ds_mt_counts_t* counts, float* verts, int64_t* out_tets, int64_t* out_faces,
                          int32_t* vsrc, int32_t* xedge, ds_stream_t stream) {
    DS_REQUIRE(pos && sdf && tets && tet_edge && ea && eb && vptr && toff && edge_id && vert_id && counts,
               "ds_mt_emit: null argument");
    DS_REQUIRE(sizes_ok(n, T, E), "ds_mt_emit: need 0 < n, E < 2^30 and 0 < 12 T < 2^30");
    const ds_mt_counts_t& c = *counts;
    DS_REQUIRE(c.n_used >= 0 && c.n_used <= n && c.n_cross >= 0 && c.n_cross <= E && c.n_side1 >= 0 &&
                   c.n_side3 >= 0 && c.n_inner >= 0 && c.n_side1 + c.n_side3 + c.n_inner <= 3 * T,
               "ds_mt_emit: count record out of range");
    const int64_t nv_out = c.n_used + c.n_cross, nt_out = c.n_side1 + c.n_side3 + c.n_inner;
    DS_REQUIRE((nv_out == 0 || (verts && (c.n_used == 0 || vsrc) && (c.n_cross == 0 || xedge))) &&
                   (nt_out == 0 || out_tets),
               "ds_mt_emit: null output for a non-empty result");
    if (nv_out == 0 && nt_out == 0) return DS_OK;
    hipStream_t st = ds::as_stream(stream);
    mt_emit_kernel<<<blocks_for(std::max(T, std::max(E, n))), BLK, 0, st>>>(
        pos, sdf, n, tets, T, tet_edge, ea, eb, E, vptr, thick, reinterpret_cast<const MtCnt*>(toff), edge_id, vert_id,
        c.n_used, c.n_side1, c.n_side3, c.n_face1, verts, out_tets, out_faces, vsrc, xedge);
    DS_LAUNCH_CHECK("mt_emit_kernel");
    return DS_OK;
}

extern "C" int64_t ds_mt_backward_workspace_floats(int64_t n_cross) { return n_cross > 0 ? ds::ceil_div(n_cross, BLK) : 1; }

extern "C" int ds_mt_backward(const float* grad_verts, const float* pos, const float* sdf, int64_t n, const int32_t* ea,
                              const int32_t* eb, int64_t E, const int32_t* vptr, const int32_t* vadj,
                              const float* thick, const int32_t* edge_id, const int32_t* vert_id, const int32_t* xedge,
                              int64_t n_used, int64_t n_cross, float* dpos, float* dsdf, float* dt, float* work,
                              ds_stream_t stream) {
    DS_REQUIRE(pos && sdf && ea && eb && vptr && vadj && edge_id && vert_id && dpos && dsdf,
               "ds_mt_backward: null argument");
    DS_REQUIRE(n > 0 && n < ((int64_t)1 << 30) && E > 0 && E < ((int64_t)1 << 30), "ds_mt_backward: bad sizes");
    DS_REQUIRE(n_used >= 0 && n_used <= n && n_cross >= 0 && n_cross <= E, "ds_mt_backward: counts out of range");
    DS_REQUIRE(n_used + n_cross == 0 || grad_verts, "ds_mt_backward: null grad_verts for a non-empty result");
    DS_REQUIRE(!dt || (thick && work && (n_cross == 0 || xedge)), "ds_mt_backward: dL/dt needs thick, xedge and work");
    hipStream_t st = ds::as_stream(stream);
    if (n_used + n_cross == 0) {
        int rc = ds::check_hip(hipMemsetAsync(dpos, 0, sizeof(float) * 3 * (size_t)n, st), "ds_mt_backward: memset");
        if (rc == DS_OK) rc = ds::check_hip(hipMemsetAsync(dsdf, 0, sizeof(float) * (size_t)n, st), "ds_mt_backward: memset");
        if (rc == DS_OK && dt) rc = ds::check_hip(hipMemsetAsync(dt, 0, sizeof(float), st), "ds_mt_backward: memset");
        return rc;
    }
    mt_grad_vertex_kernel<<<blocks_for(n), BLK, 0, st>>>(grad_verts, pos, sdf, n, ea, eb, vptr, vadj, thick, edge_id,
                                                         vert_id, n_used, dpos, dsdf);
    DS_LAUNCH_CHECK("mt_grad_vertex_kernel");
    if (dt) {
        const int64_t np = ds_mt_backward_workspace_floats(n_cross);
        if (n_cross > 0) {
            mt_grad_thick_kernel<<<(unsigned)np, BLK, 0, st>>>(grad_verts, pos, sdf, ea, eb, xedge, n_cross, n_used, thick,
                                                               work);
            DS_LAUNCH_CHECK("mt_grad_thick_kernel");
        }
        mt_grad_thick_final_kernel<<<1, BLK, 0, st>>>(work, n_cross > 0 ? np : 0, dt);
        DS_LAUNCH_CHECK("mt_grad_thick_final_kernel");
    }
    return DS_OK;
}
