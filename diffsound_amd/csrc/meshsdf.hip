// Signed distance from a triangle mesh to a set of points - gfx950.  Replaces open3d's
// RaycastingScene.compute_signed_distance in the reference's shape loops (src/dmtet/geometry/dmtet_thickness.py:301-314,
// dmtet_interpolate.py:318-351, experiments/geometry_train.py:170-197).  DESIGN.md section 11 has the scheme.
//
// One pass over all (point, face) pairs gives, per point: the minimum over faces of the exact point-triangle
// distance, the face that attains it (the lowest index on equal squared distances), and the generalised winding
// number, the sum of the faces' signed solid angles (Van Oosterom-Strackee, atan2 form) over 4 pi.  The signed
// distance is negative inside (open3d's convention), inside = winding number > 0.5.
//
//   ds_mesh_sdf_pack   per face, once per mesh: the 16-float record of include/diffsound_hip.h (fp64 arithmetic,
//                      rounded once).
//   ds_mesh_sdf_query  one lane per point; the face records pass through LDS in tiles of TILE faces, every lane
//                      reads the same LDS address (a broadcast, no bank conflict).
//
// Order of the arithmetic (what makes a point's result independent of the other points of the call, and the two
// launch shapes bitwise equal): the faces are cut into CHUNKS of `tiles_per_chunk` tiles, a function of F alone.
// Inside a chunk the solid angles are summed and the minimum is taken face by face in index order, starting from
// (0, +inf); the chunks' results are then combined in chunk order.  The one-launch shape does both in one kernel;
// the split shape, for few points, gives every (point block, chunk) its own workgroup, which writes its chunk result
// to the workspace, and a second kernel combines them in the same order with the same operations.  No atomics.
// fp32 throughout, with contraction off: every fused multiply-add below is written out.
#include <cfloat>
#include <cmath>

#include "ds_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int TILE = 128;       // faces per LDS tile = threads per workgroup
constexpr int MAX_CHUNKS = 32;  // bounds the split shape's workspace: P * MAX_CHUNKS * 12 bytes
constexpr int REC4 = DS_MESH_SDF_FACE_RECORD / 4;
constexpr int64_t SPLIT_BELOW_BLOCKS = 1024;  // point blocks below which the faces are split across workgroups
constexpr float INV_2PI = 0.15915494309189535f;

struct V3 {
    float x, y, z;
};
__device__ __forceinline__ V3 sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ float dot(V3 a, V3 b) { return fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x)); }
__device__ __forceinline__ V3 cross(V3 a, V3 b) {
    return {fmaf(a.y, b.z, -(a.z * b.y)), fmaf(a.z, b.x, -(a.x * b.z)), fmaf(a.x, b.y, -(a.y * b.x))};
}

// squared distance from the origin to the segment u + t d, 0 <= t <= 1 (inv = 1 / |d|^2, or 0 for a point)
__device__ __forceinline__ float seg_d2(V3 u, V3 d, float inv) {
    const float t = fminf(fmaxf(-dot(u, d) * inv, 0.f), 1.f);
    const V3 q = {fmaf(t, d.x, u.x), fmaf(t, d.y, u.y), fmaf(t, d.z, u.z)};
    return dot(q, q);
}

// The running result of one point over a range of faces.
struct Acc {
    float w;   // sum of atan2(det, den) = half the solid angles
    float d2;  // least squared distance
    int face;  // the face that gave it (-1: none yet)
};

// One (point, face) pair.  r: the face's record in LDS; p: the point.
__device__ __forceinline__ void face_eval(const float4* r, V3 p, int face, Acc& acc) {
    const float4 r0 = r[0], r1 = r[1], r2 = r[2], r3 = r[3];
    const V3 a = {r0.x, r0.y, r0.z}, b = {r0.w, r1.x, r1.y}, c = {r1.z, r1.w, r2.x};
    const V3 n = {r3.x, r3.y, r3.z};
    const bool valid = r3.w != 0.f;
    const V3 A = sub(a, p), B = sub(b, p), C = sub(c, p);  // the vertices seen from the point
    const V3 cab = cross(A, B), cbc = cross(B, C), cca = cross(C, A);
    // distance: the plane when the projection falls inside the triangle, else the nearest edge
    float d2;
    if (valid && dot(n, cab) >= 0.f && dot(n, cbc) >= 0.f && dot(n, cca) >= 0.f) {
        const float h = dot(A, n);
        d2 = h * h;
    } else {
        d2 = fminf(fminf(seg_d2(A, sub(b, a), r2.y), seg_d2(B, sub(c, b), r2.z)), seg_d2(C, sub(a, c), r2.w));
    }
    if (d2 < acc.d2) {
        acc.d2 = d2;
        acc.face = face;
    }
    // solid angle / 2 = atan2(A . (B x C), |A||B||C| + (A.B)|C| + (A.C)|B| + (B.C)|A|); none for a zero-area face
    if (valid) {
        const float la = sqrtf(dot(A, A)), lb = sqrtf(dot(B, B)), lc = sqrtf(dot(C, C));
        const float det = dot(A, cbc);
        const float den = fmaf(dot(B, C), la, fmaf(dot(A, C), lb, fmaf(dot(A, B), lc, la * lb * lc)));
        acc.w += atan2f(det, den);
    }
}

__device__ __forceinline__ void combine(Acc& total, const Acc& part) {
    total.w += part.w;
    if (part.d2 < total.d2) {
        total.d2 = part.d2;
        total.face = part.face;
    }
}

__device__ __forceinline__ void finish(const Acc& t, int64_t p, float* out_signed, float* out_unsigned, int32_t* out_face,
                                       float* out_winding) {
    const float d = sqrtf(t.d2);
    const float w = t.w * INV_2PI;
    out_signed[p] = w > 0.5f ? -d : d;
    if (out_unsigned) out_unsigned[p] = d;
    if (out_face) out_face[p] = t.face;
    if (out_winding) out_winding[p] = w;
}

// SPLIT = false: grid (point blocks), every workgroup walks all chunks and writes the outputs.
// SPLIT = true:  grid (point blocks, chunks), a workgroup walks one chunk and writes its result to the workspace
//                (chunk-major: w[chunk * P + p], d2[...], face[...]).
template <bool SPLIT>
__global__ __launch_bounds__(TILE) void mesh_sdf_kernel(const float* __restrict__ pts, int64_t P,
                                                        const float4* __restrict__ rec, int F, int tiles_per_chunk,
                                                        int nchunks, float* __restrict__ out_signed,
                                                        float* __restrict__ out_unsigned, int32_t* __restrict__ out_face,
                                                        float* __restrict__ out_winding, float* __restrict__ work_w,
                                                        float* __restrict__ work_d2, int32_t* __restrict__ work_face) {
    __shared__ float4 tile[TILE * REC4];
    const int tid = threadIdx.x;
    const int64_t p = (int64_t)blockIdx.x * TILE + tid;
    const bool live = p < P;
    V3 x = {0.f, 0.f, 0.f};
    if (live) x = {pts[3 * p], pts[3 * p + 1], pts[3 * p + 2]};
    const int ntiles = (F + TILE - 1) / TILE;
    const int c0 = SPLIT ? (int)blockIdx.y : 0, c1 = SPLIT ? c0 + 1 : nchunks;
    Acc total = {0.f, INFINITY, -1};
    for (int c = c0; c < c1; ++c) {
        Acc part = {0.f, INFINITY, -1};
        const int t1 = min((c + 1) * tiles_per_chunk, ntiles);
        for (int t = c * tiles_per_chunk; t < t1; ++t) {
            const int f0 = t * TILE;
            const int nf = min(TILE, F - f0);
            __syncthreads();  // the previous tile has been read by every lane
#pragma unroll
            for (int k = 0; k < REC4; ++k) {
                const int i = k * TILE + tid;  // float4 index inside the tile: coalesced, conflict-free
                if (i < nf * REC4) tile[i] = rec[(int64_t)f0 * REC4 + i];
            }
            __syncthreads();
            if (live) {
                for (int j = 0; j < nf; ++j) face_eval(tile + j * REC4, x, f0 + j, part);
            }
        }
        if (SPLIT) {
            if (live) {
                const int64_t o = (int64_t)c * P + p;
                work_w[o] = part.w;
                work_d2[o] = part.d2;
                work_face[o] = part.face;
            }
        } else {
            combine(total, part);
        }
    }
    if (!SPLIT && live) finish(total, p, out_signed, out_unsigned, out_face, out_winding);
}

__global__ __launch_bounds__(256) void mesh_sdf_combine_kernel(int64_t P, int nchunks, const float* __restrict__ work_w,
                                                               const float* __restrict__ work_d2,
                                                               const int32_t* __restrict__ work_face,
                                                               float* __restrict__ out_signed,
                                                               float* __restrict__ out_unsigned,
                                                               int32_t* __restrict__ out_face,
                                                               float* __restrict__ out_winding) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    Acc total = {0.f, INFINITY, -1};
    for (int c = 0; c < nchunks; ++c) {
        const int64_t o = (int64_t)c * P + p;
        const Acc part = {work_w[o], work_d2[o], work_face[o]};
        combine(total, part);
    }
    finish(total, p, out_signed, out_unsigned, out_face, out_winding);
}

// Face records in fp64 from the fp32 vertices, rounded once.  A zero-area face (|ab x ac| == 0) gets normal 0 and
// valid 0; a zero-length edge (or one whose 1/|d|^2 leaves fp32) gets inverse 0, which makes it its start point.
__global__ __launch_bounds__(256) void mesh_sdf_pack_kernel(const float* __restrict__ verts,
                                                            const int32_t* __restrict__ faces, int64_t F,
                                                            float* __restrict__ rec) {
    const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    double v[3][3];
    for (int k = 0; k < 3; ++k) {
        const int64_t i = faces[3 * f + k];
        for (int d = 0; d < 3; ++d) v[k][d] = (double)verts[3 * i + d];
    }
    float* r = rec + f * DS_MESH_SDF_FACE_RECORD;
    for (int k = 0; k < 3; ++k)
        for (int d = 0; d < 3; ++d) r[3 * k + d] = (float)v[k][d];
    for (int k = 0; k < 3; ++k) {  // edges a->b, b->c, c->a
        const int k1 = (k + 1) % 3;
        double l2 = 0.0;
        for (int d = 0; d < 3; ++d) {
            // the kernel forms the edge in fp32 from the fp32 vertices: use that vector's length
            const double e = (double)((float)v[k1][d] - (float)v[k][d]);
            l2 += e * e;
        }
        const double inv = l2 > 0.0 ? 1.0 / l2 : 0.0;
        r[9 + k] = inv <= (double)FLT_MAX ? (float)inv : 0.f;
    }
    double ab[3], ac[3];
    for (int d = 0; d < 3; ++d) {
        ab[d] = v[1][d] - v[0][d];
        ac[d] = v[2][d] - v[0][d];
    }
    const double n[3] = {ab[1] * ac[2] - ab[2] * ac[1], ab[2] * ac[0] - ab[0] * ac[2], ab[0] * ac[1] - ab[1] * ac[0]};
    const double nn = n[0] * n[0] + n[1] * n[1] + n[2] * n[2];
    const bool valid = nn > 0.0;
    const double s = valid ? 1.0 / sqrt(nn) : 0.0;
    for (int d = 0; d < 3; ++d) r[12 + d] = (float)(n[d] * s);
    r[15] = valid ? 1.f : 0.f;
}

struct Plan {
    int ntiles, tiles_per_chunk, nchunks;
    int64_t pblocks;
};
Plan plan(int64_t P, int64_t F) {
    Plan pl;
    pl.ntiles = (int)ds::ceil_div(F, TILE);
    pl.tiles_per_chunk = (int)ds::ceil_div(pl.ntiles, MAX_CHUNKS);
    pl.nchunks = (int)ds::ceil_div(pl.ntiles, pl.tiles_per_chunk);
    pl.pblocks = ds::ceil_div(P, TILE);
    return pl;
}
constexpr int64_t MAX_POINTS = (int64_t)TILE * 0x7fffffff;
constexpr int64_t MAX_FACES = 1 << 30;

}  // namespace

extern "C" int ds_mesh_sdf_pack(const float* verts, const int32_t* faces, int64_t V, int64_t F, float* face_records,
                                ds_stream_t stream) {
    DS_REQUIRE(verts && faces && face_records, "ds_mesh_sdf_pack: null pointer");
    DS_REQUIRE(V >= 1 && F >= 1 && F <= MAX_FACES, "ds_mesh_sdf_pack: bad sizes V=%lld F=%lld", (long long)V, (long long)F);
    mesh_sdf_pack_kernel<<<dim3((unsigned)ds::ceil_div(F, 256)), dim3(256), 0, ds::as_stream(stream)>>>(verts, faces, F,
                                                                                                        face_records);
    DS_LAUNCH_CHECK("ds_mesh_sdf_pack");
    return DS_OK;
}

extern "C" int64_t ds_mesh_sdf_workspace_bytes(int64_t P, int64_t F, int force_split) {
    if (P < 0 || P > MAX_POINTS || F < 1 || F > MAX_FACES) return -1;
    const Plan pl = plan(P, F);
    const bool split = force_split || (pl.pblocks < SPLIT_BELOW_BLOCKS && pl.nchunks > 1);
    return split ? P * pl.nchunks * 12 : 0;
}

extern "C" int ds_mesh_sdf_query(const float* points, int64_t P, const float* face_records, int64_t F, float* out_signed,
                                 float* out_unsigned, int32_t* out_face, float* out_winding, void* work,
                                 int64_t work_bytes, ds_stream_t stream) {
    DS_REQUIRE(P >= 0 && P <= MAX_POINTS && F >= 1 && F <= MAX_FACES, "ds_mesh_sdf_query: bad sizes P=%lld F=%lld",
               (long long)P, (long long)F);
    if (P == 0) return DS_OK;
    DS_REQUIRE(points && face_records && out_signed, "ds_mesh_sdf_query: null pointer");
    DS_REQUIRE((reinterpret_cast<uintptr_t>(face_records) & 15) == 0, "ds_mesh_sdf_query: face_records not 16-byte aligned");
    const Plan pl = plan(P, F);
    const float4* rec = reinterpret_cast<const float4*>(face_records);
    hipStream_t st = ds::as_stream(stream);
    if (work == nullptr) {
        mesh_sdf_kernel<false><<<dim3((unsigned)pl.pblocks), dim3(TILE), 0, st>>>(
            points, P, rec, (int)F, pl.tiles_per_chunk, pl.nchunks, out_signed, out_unsigned, out_face, out_winding, nullptr,
            nullptr, nullptr);
        DS_LAUNCH_CHECK("ds_mesh_sdf_query");
        return DS_OK;
    }
    DS_REQUIRE(work_bytes >= P * pl.nchunks * 12, "ds_mesh_sdf_query: workspace of %lld bytes, %lld needed",
               (long long)work_bytes, (long long)(P * pl.nchunks * 12));
    DS_REQUIRE((reinterpret_cast<uintptr_t>(work) & 3) == 0, "ds_mesh_sdf_query: workspace not 4-byte aligned");
    float* work_w = static_cast<float*>(work);
    float* work_d2 = work_w + P * pl.nchunks;
    int32_t* work_face = reinterpret_cast<int32_t*>(work_d2 + P * pl.nchunks);
    mesh_sdf_kernel<true><<<dim3((unsigned)pl.pblocks, (unsigned)pl.nchunks), dim3(TILE), 0, st>>>(
        points, P, rec, (int)F, pl.tiles_per_chunk, pl.nchunks, nullptr, nullptr, nullptr, nullptr, work_w, work_d2, work_face);
    DS_LAUNCH_CHECK("ds_mesh_sdf_query (split)");
    mesh_sdf_combine_kernel<<<dim3((unsigned)ds::ceil_div(P, 256)), dim3(256), 0, st>>>(
        P, pl.nchunks, work_w, work_d2, work_face, out_signed, out_unsigned, out_face, out_winding);
    DS_LAUNCH_CHECK("ds_mesh_sdf_query (combine)");
    return DS_OK;
}
