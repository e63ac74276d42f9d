// Helmholtz boundary elements (exterior Neumann problem, direct form, piecewise-constant "DP0" space) - gfx950.
// Replaces the reference's bempp-cl operators (src/diffelastic/bem.py:36-61): per-face geometry, the Galerkin
// assembly of A = -1/2 M + K together with rhs = V g, the dense complex GEMV of the GMRES, and the potential
// u(p) = -S g + D u at listener points.  DESIGN.md "Sound radiation (BEM)" has the formulation and the quadrature.
//
//   G(x,y)        = e^{ikr} / (4 pi r)
//   dG/dn_y(x,y)  = n_y.(x-y) (1 - ikr) e^{ikr} / (4 pi r^3)
//
// Regular pairs: the 6-point degree-4 rule on both triangles (36 kernel evaluations).  Near pairs (centroid
// distance < BEM_NEAR_RATIO x the larger diameter; this covers every pair that shares a vertex): the test triangle
// is cut into 16 congruent pieces with the 6-point rule on each (96 outer points); at each outer point the static
// part of the inner integral is exact (1/(4 pi r): Wilton/Graglia edge formula; its n_y derivative: the Van
// Oosterom-Strackee solid angle) and the smooth remainder (e^{ikr}-1)/(4 pi r) and its n_y derivative use the inner
// 6-point rule.  A coincident pair has K_ii = 0 exactly (n_y.(x-y) = 0 on a flat face).
//
// e^{ikr} is evaluated from the phase in revolutions: t = fract(kr / 2 pi) with the product in two floats, then the
// hardware sine / cosine, whose argument is in revolutions; up to kr = 100 the entries stay at the level of the same
// algorithm in fp32 with libm (DESIGN.md "Accuracy").  No float atomics: every sum has a fixed
// order, the results are bitwise reproducible.
#include "ds_common.h"

namespace {

using f4 = __attribute__((ext_vector_type(4))) float;

constexpr int REC = DS_BEM_FACE_RECORD;  // floats per face record (layout: include/diffsound_hip.h)
constexpr float NEAR_RATIO = DS_BEM_NEAR_RATIO;
constexpr float INV4PI = 0.0795774715459476679f;
constexpr float INV2PI = 0.159154943091895336f;    // fp32(1 / 2 pi) = 0.15915493667125702
constexpr float INV2PI_LO = 6.42063832e-9f;         // 1 / 2 pi - INV2PI
constexpr int ASM_COLS = 256;  // columns per assembly workgroup (one per thread)
constexpr int ASM_ROWS = 8;    // rows per assembly workgroup

// 6-point degree-4 rule on the reference triangle: barycentric (a, a, 1-2a) and permutations, weights sum to 1
__device__ __forceinline__ void rule6(int q, float& l0, float& l1, float& w) {
    const float a1 = 0.445948490915965f, w1 = 0.223381589678011f;
    const float a2 = 0.091576213509771f, w2 = 0.109951743655322f;
    const float a = q < 3 ? a1 : a2, b = 1.f - 2.f * a;
    w = q < 3 ? w1 : w2;
    const int r = q % 3;
    l0 = r == 0 ? b : a;
    l1 = r == 1 ? b : a;
}

struct V3 {
    float x, y, z;
};
__device__ __forceinline__ V3 sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ V3 ld3(const float* p) { return {p[0], p[1], p[2]}; }

// e^{ikr} from the phase in revolutions.  The product kr / 2 pi is carried in two floats: p, and what p leaves out
// (the rounding of kr * INV2PI, recovered exactly by the fma, and the part of 1 / 2 pi below its fp32 value).  The
// fp32 constant alone is 4.0e-8 low, a phase error of 4.0e-8 kr that is the same in every term of a sum, so it does
// not average out the way the roundings do.  Only the rounding of kr itself is left.
__device__ __forceinline__ void expikr(float k, float r, float& c, float& s) {
    const float kr = k * r;
    const float p = kr * INV2PI;
    const float lo = fmaf(kr, INV2PI_LO, fmaf(kr, INV2PI, -p));
    const float t = __builtin_amdgcn_fractf(p) + lo;
    s = __builtin_amdgcn_sinf(t);
    c = __builtin_amdgcn_cosf(t);
}

// Exact static inner integrals over the flat triangle (y0, y1, y2) with unit normal n, at the point x:
//   *s1 = int 1/|x-y| dy                          (Wilton/Graglia edge formula)
//   *dl = int n.(x-y)/|x-y|^3 dy = -(solid angle)  (Van Oosterom-Strackee)
__device__ void static_integrals(V3 x, V3 y0, V3 y1, V3 y2, V3 n, bool want_dl, float* s1, float* dl) {
    const V3 a = sub(y0, x), b = sub(y1, x), c = sub(y2, x);
    const float la = sqrtf(dot(a, a)), lb = sqrtf(dot(b, b)), lc = sqrtf(dot(c, c));
    const float w = -dot(n, a), aw = fabsf(w);
    float acc = 0.f;
    const V3 ys[3] = {a, b, c};
    const float ls[3] = {la, lb, lc};
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        const V3 pa = ys[e], pb = ys[(e + 1) % 3];
        const float ra = ls[e], rb = ls[(e + 1) % 3];
        const V3 d = sub(pb, pa);
        const float len = sqrtf(dot(d, d));
        const V3 sv = {d.x / len, d.y / len, d.z / len};
        const V3 m = cross(sv, n);  // outward in-plane normal of the edge
        const float t0 = dot(m, pa);
        const float sm = dot(sv, pa), sp = dot(sv, pb);
        if (fabsf(t0) > 1e-30f) {
            const float f = (sp + sm >= 0.f) ? logf((rb + sp) / (ra + sm)) : logf((ra - sm) / (rb - sp));
            acc += t0 * f;
            if (aw > 0.f) {
                const float r02 = t0 * t0 + w * w;
                acc -= aw * (atanf(t0 * sp / (r02 + aw * rb)) - atanf(t0 * sm / (r02 + aw * ra)));
            }
        }
    }
    *s1 = acc;
    if (want_dl) {
        const float det = dot(a, cross(b, c));
        const float den = la * lb * lc + dot(a, b) * lc + dot(a, c) * lb + dot(b, c) * la;
        *dl = -2.f * atan2f(det, den);
    }
}

// Inner integrals over face j (record fj) at the outer point x, for a near pair: static part exact, remainder by the
// 6-point rule.  Returns int G and int dG/dn_y (complex) over face j.
__device__ void near_inner(V3 x, const float* fj, float k, bool coincident, float& vr, float& vi, float& kr_, float& ki) {
    const V3 n = ld3(fj + 24);
    float s1, dl = 0.f;
    static_integrals(x, ld3(fj + 32), ld3(fj + 35), ld3(fj + 38), n, !coincident, &s1, &dl);
    vr = s1 * INV4PI;
    vi = 0.f;
    kr_ = coincident ? 0.f : dl * INV4PI;
    ki = 0.f;
    for (int q = 0; q < 6; ++q) {
        const V3 d = sub(x, ld3(fj + 3 * q));
        const float wq = fj[18 + q];
        const float r2 = fmaxf(dot(d, d), 1e-30f);
        const float ri = __builtin_amdgcn_rsqf(r2), r = r2 * ri;
        float c, s;
        expikr(k, r, c, s);
        const float g = wq * ri * INV4PI;
        vr += g * (c - 1.f);
        vi += g * s;
        if (!coincident) {
            const float kr = k * r;
            const float h = dot(n, d) * g * ri * ri;
            kr_ += h * (c + kr * s - 1.f);
            ki += h * (s - kr * c);
        }
    }
}

// Near pair: 96 outer points (16 sub-triangles x 6) on face i.
__device__ void near_pair(const float* fi, const float* fj, float k, bool coincident, float& Vr, float& Vi, float& Kr,
                          float& Ki) {
    const V3 p0 = ld3(fi + 32), e1 = sub(ld3(fi + 35), p0), e2 = sub(ld3(fi + 38), p0);
    const float sub_area = fi[31] * (1.f / 16.f);
    Vr = Vi = Kr = Ki = 0.f;
    for (int st = 0; st < 16; ++st) {
        // sub-triangle st of the 4x4 split: 10 "up" (i, j) with i + j <= 3, then 6 "down" with i + j <= 2
        int si, sj, up;
        if (st < 10) {
            up = 1;
            si = st < 4 ? 0 : st < 7 ? 1 : st < 9 ? 2 : 3;
            sj = st - (si == 0 ? 0 : si == 1 ? 4 : si == 2 ? 7 : 9);
        } else {
            up = 0;
            const int u = st - 10;
            si = u < 3 ? 0 : u < 5 ? 1 : 2;
            sj = u - (si == 0 ? 0 : si == 1 ? 3 : 5);
        }
        // corners in (l1, l2) barycentrics on the 1/4 grid
        float a0, b0, a1, b1, a2, b2;
        if (up) {
            a0 = si, b0 = sj, a1 = si + 1, b1 = sj, a2 = si, b2 = sj + 1;
        } else {
            a0 = si + 1, b0 = sj, a1 = si + 1, b1 = sj + 1, a2 = si, b2 = sj + 1;
        }
        for (int q = 0; q < 6; ++q) {
            float l0, l1, w;
            rule6(q, l0, l1, w);
            const float l2 = 1.f - l0 - l1;
            const float u = 0.25f * (l0 * a0 + l1 * a1 + l2 * a2), v = 0.25f * (l0 * b0 + l1 * b1 + l2 * b2);
            const V3 x = {p0.x + u * e1.x + v * e2.x, p0.y + u * e1.y + v * e2.y, p0.z + u * e1.z + v * e2.z};
            float vr, vi, kr, ki;
            near_inner(x, fj, k, coincident, vr, vi, kr, ki);
            const float wx = w * sub_area;
            Vr += wx * vr;
            Vi += wx * vi;
            Kr += wx * kr;
            Ki += wx * ki;
        }
    }
}

__device__ __forceinline__ bool is_near(const float* ci, float hi, const float* cj, float hj) {
    const float dx = ci[0] - cj[0], dy = ci[1] - cj[1], dz = ci[2] - cj[2];
    const float h = NEAR_RATIO * fmaxf(hi, hj);
    return dx * dx + dy * dy + dz * dz < h * h;
}

__global__ void __launch_bounds__(256) bem_geometry_kernel(const float* __restrict__ verts, const int32_t* __restrict__ tris,
                                                           int64_t m, float* __restrict__ rec) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= m) return;
    const V3 v0 = ld3(verts + 3 * (int64_t)tris[3 * f]), v1 = ld3(verts + 3 * (int64_t)tris[3 * f + 1]),
             v2 = ld3(verts + 3 * (int64_t)tris[3 * f + 2]);
    const V3 e1 = sub(v1, v0), e2 = sub(v2, v0), e3 = sub(v2, v1);
    const V3 cr = cross(e1, e2);
    const float len = sqrtf(dot(cr, cr));
    const float area = 0.5f * len;
    float* o = rec + f * REC;
    for (int q = 0; q < 6; ++q) {
        float l0, l1, w;
        rule6(q, l0, l1, w);
        const float l2 = 1.f - l0 - l1;
        o[3 * q] = l0 * v0.x + l1 * v1.x + l2 * v2.x;
        o[3 * q + 1] = l0 * v0.y + l1 * v1.y + l2 * v2.y;
        o[3 * q + 2] = l0 * v0.z + l1 * v1.z + l2 * v2.z;
        o[18 + q] = w * area;
    }
    o[24] = cr.x / len, o[25] = cr.y / len, o[26] = cr.z / len;
    o[27] = (v0.x + v1.x + v2.x) * (1.f / 3.f), o[28] = (v0.y + v1.y + v2.y) * (1.f / 3.f), o[29] = (v0.z + v1.z + v2.z) * (1.f / 3.f);
    o[30] = sqrtf(fmaxf(dot(e1, e1), fmaxf(dot(e2, e2), dot(e3, e3))));
    o[31] = area;
    o[32] = v0.x, o[33] = v0.y, o[34] = v0.z, o[35] = v1.x, o[36] = v1.y, o[37] = v1.z, o[38] = v2.x, o[39] = v2.y, o[40] = v2.z;
    for (int q = 41; q < REC; ++q) o[q] = 0.f;
}

// One workgroup: rows [i0, i0 + ASM_ROWS) x columns [j0, j0 + 256), one column per thread.  Writes A (and V), and the
// workgroup's part of (V g)_i into part[i * ntile + tile] (wave butterfly, then the 4 waves in order).
__global__ void __launch_bounds__(256) bem_assemble_kernel(const float* __restrict__ rec, int64_t n, float k,
                                                           const float2* __restrict__ g, float2* __restrict__ A, int64_t lda,
                                                           float2* __restrict__ V, int64_t ldv, float2* __restrict__ part,
                                                           int64_t ntile) {
    __shared__ float2 red[ASM_ROWS][4];
    const int64_t j = (int64_t)blockIdx.x * ASM_COLS + threadIdx.x;
    const int64_t i0 = (int64_t)blockIdx.y * ASM_ROWS;
    const bool valid = j < n;
    const float* fj = rec + (valid ? j : 0) * REC;
    float yq[18], wq[6];
#pragma unroll
    for (int t = 0; t < 18; ++t) yq[t] = fj[t];
#pragma unroll
    for (int t = 0; t < 6; ++t) wq[t] = fj[18 + t];
    const V3 nj = ld3(fj + 24);
    const float hj = fj[30];
    const float2 gj = valid ? g[j] : make_float2(0.f, 0.f);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int r = 0; r < ASM_ROWS; ++r) {
        const int64_t i = i0 + r;
        if (i >= n) break;
        const float* fi = rec + i * REC;
        float Vr = 0.f, Vi = 0.f, Kr = 0.f, Ki = 0.f;
        if (valid) {
            if (is_near(fi + 27, fi[30], fj + 27, hj)) {
                near_pair(fi, fj, k, i == j, Vr, Vi, Kr, Ki);
            } else {
#pragma unroll
                for (int p = 0; p < 6; ++p) {
                    const V3 x = ld3(fi + 3 * p);
                    const float wx = fi[18 + p];
                    float vr = 0.f, vi = 0.f, kr_ = 0.f, ki = 0.f;
#pragma unroll
                    for (int q = 0; q < 6; ++q) {
                        const V3 d = {x.x - yq[3 * q], x.y - yq[3 * q + 1], x.z - yq[3 * q + 2]};
                        const float r2 = dot(d, d);
                        const float ri = __builtin_amdgcn_rsqf(r2), rr = r2 * ri;
                        float c, s;
                        expikr(k, rr, c, s);
                        const float gw = wq[q] * ri;
                        vr += gw * c;
                        vi += gw * s;
                        const float kr = k * rr;
                        const float h = dot(nj, d) * gw * ri * ri;
                        kr_ += h * (c + kr * s);
                        ki += h * (s - kr * c);
                    }
                    Vr += wx * vr, Vi += wx * vi, Kr += wx * kr_, Ki += wx * ki;
                }
                Vr *= INV4PI, Vi *= INV4PI, Kr *= INV4PI, Ki *= INV4PI;
            }
            const float diag = i == j ? 0.5f * fi[31] : 0.f;
            A[i * lda + j] = make_float2(Kr - diag, Ki);
            if (V) V[i * ldv + j] = make_float2(Vr, Vi);
        }
        float pr = Vr * gj.x - Vi * gj.y, pi = Vr * gj.y + Vi * gj.x;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            pr += __shfl_xor(pr, off, 64);
            pi += __shfl_xor(pi, off, 64);
        }
        if (lane == 0) red[r][wave] = make_float2(pr, pi);
    }
    __syncthreads();
    if (threadIdx.x < ASM_ROWS && i0 + threadIdx.x < n) {
        const int r = threadIdx.x;
        float2 s = red[r][0];
        for (int w = 1; w < 4; ++w) s.x += red[r][w].x, s.y += red[r][w].y;
        part[(i0 + r) * ntile + blockIdx.x] = s;
    }
}

__global__ void __launch_bounds__(256) bem_rhs_kernel(const float2* __restrict__ part, int64_t n, int64_t ntile,
                                                      float2* __restrict__ rhs) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float2 s = make_float2(0.f, 0.f);
    for (int64_t t = 0; t < ntile; ++t) {
        const float2 p = part[i * ntile + t];
        s.x += p.x, s.y += p.y;
    }
    rhs[i] = s;
}

// y_i = scale_i * sum_j A_ij x_j: one wave per row, 16-byte loads (two complex entries per lane), four in flight,
// butterfly reduction.  lda even, A and x 16-byte aligned.
__global__ void __launch_bounds__(256) bem_cgemv_kernel(const float2* __restrict__ A, int64_t lda, const float2* __restrict__ x,
                                                        int64_t n, const float* __restrict__ scale, float2* __restrict__ y) {
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= n) return;
    const f4* a4 = reinterpret_cast<const f4*>(A + row * lda);
    const f4* x4 = reinterpret_cast<const f4*>(x);
    const int64_t n2 = n >> 1;
    float sr = 0.f, si = 0.f;
    int64_t p = lane;
    for (; p + 192 < n2; p += 256) {
        f4 av[4], xv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) av[u] = __builtin_nontemporal_load(a4 + p + 64 * u);
#pragma unroll
        for (int u = 0; u < 4; ++u) xv[u] = x4[p + 64 * u];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            sr += av[u].x * xv[u].x - av[u].y * xv[u].y + av[u].z * xv[u].z - av[u].w * xv[u].w;
            si += av[u].x * xv[u].y + av[u].y * xv[u].x + av[u].z * xv[u].w + av[u].w * xv[u].z;
        }
    }
    for (; p < n2; p += 64) {
        const f4 av = __builtin_nontemporal_load(a4 + p), xv = x4[p];
        sr += av.x * xv.x - av.y * xv.y + av.z * xv.z - av.w * xv.w;
        si += av.x * xv.y + av.y * xv.x + av.z * xv.w + av.w * xv.z;
    }
    if ((n & 1) && lane == 0) {
        const float2 av = A[row * lda + n - 1], xv = x[n - 1];
        sr += av.x * xv.x - av.y * xv.y;
        si += av.x * xv.y + av.y * xv.x;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        sr += __shfl_xor(sr, off, 64);
        si += __shfl_xor(si, off, 64);
    }
    if (lane == 0) {
        const float sc = scale ? scale[row] : 1.f;
        y[row] = make_float2(sc * sr, sc * si);
    }
}

constexpr int POT_TILE = 64;  // faces staged in LDS per step

// One thread per point; faces staged through LDS 64 at a time; each thread sums its faces in index order.
__global__ void __launch_bounds__(256) bem_potential_kernel(const float* __restrict__ rec, int64_t n, float k,
                                                            const float2* __restrict__ gco, const float2* __restrict__ uco,
                                                            const float* __restrict__ pts, int64_t np, float2* __restrict__ out) {
    __shared__ float sf[POT_TILE * REC];
    __shared__ float2 sg[POT_TILE], su[POT_TILE];
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool valid = p < np;
    const V3 x = valid ? ld3(pts + 3 * p) : V3{0.f, 0.f, 0.f};
    float ar = 0.f, ai = 0.f;
    for (int64_t f0 = 0; f0 < n; f0 += POT_TILE) {
        const int cnt = (int)((n - f0) < POT_TILE ? (n - f0) : POT_TILE);
        __syncthreads();
        for (int t = threadIdx.x; t < cnt * REC; t += 256) sf[t] = rec[f0 * REC + t];
        if (threadIdx.x < cnt) {
            sg[threadIdx.x] = gco[f0 + threadIdx.x];
            su[threadIdx.x] = uco[f0 + threadIdx.x];
        }
        __syncthreads();
        if (!valid) continue;
        for (int f = 0; f < cnt; ++f) {
            const float* fj = sf + f * REC;
            float vr, vi, kr_, ki;
            const float dx = x.x - fj[27], dy = x.y - fj[28], dz = x.z - fj[29], h = NEAR_RATIO * fj[30];
            if (dx * dx + dy * dy + dz * dz < h * h) {
                near_inner(x, fj, k, false, vr, vi, kr_, ki);
            } else {
                const V3 nj = ld3(fj + 24);
                vr = vi = kr_ = ki = 0.f;
                for (int q = 0; q < 6; ++q) {
                    const V3 d = sub(x, ld3(fj + 3 * q));
                    const float r2 = dot(d, d);
                    const float ri = __builtin_amdgcn_rsqf(r2), rr = r2 * ri;
                    float c, s;
                    expikr(k, rr, c, s);
                    const float gw = fj[18 + q] * ri;
                    vr += gw * c;
                    vi += gw * s;
                    const float kr = k * rr;
                    const float hh = dot(nj, d) * gw * ri * ri;
                    kr_ += hh * (c + kr * s);
                    ki += hh * (s - kr * c);
                }
                vr *= INV4PI, vi *= INV4PI, kr_ *= INV4PI, ki *= INV4PI;
            }
            const float2 gg = sg[f], uu = su[f];
            ar += -(vr * gg.x - vi * gg.y) + (kr_ * uu.x - ki * uu.y);
            ai += -(vr * gg.y + vi * gg.x) + (kr_ * uu.y + ki * uu.x);
        }
    }
    if (valid) out[p] = make_float2(ar, ai);
}

}  // namespace

extern "C" int64_t ds_bem_assemble_workspace_bytes(int64_t n) {
    if (n <= 0) return 0;
    return n * ds::ceil_div(n, (int64_t)ASM_COLS) * (int64_t)sizeof(float2);
}

extern "C" int ds_bem_geometry(const float* verts, int64_t nv, const int32_t* tris, int64_t m, float* rec, ds_stream_t stream) {
    DS_REQUIRE(verts && tris && rec, "ds_bem_geometry: null pointer");
    DS_REQUIRE(nv > 0 && m > 0, "ds_bem_geometry: empty mesh");
    const int64_t blocks = ds::ceil_div(m, (int64_t)256);
    DS_REQUIRE(blocks < ((int64_t)1 << 31), "ds_bem_geometry: too many faces");
    bem_geometry_kernel<<<(unsigned)blocks, 256, 0, ds::as_stream(stream)>>>(verts, tris, m, rec);
    DS_LAUNCH_CHECK("bem_geometry_kernel");
    return DS_OK;
}

extern "C" int ds_bem_assemble(const float* rec, int64_t n, float k, const float* g, float* A, int64_t lda, float* V, int64_t ldv,
                               float* rhs, void* work, ds_stream_t stream) {
    DS_REQUIRE(rec && g && A && rhs && work, "ds_bem_assemble: null pointer");
    DS_REQUIRE(n > 0 && lda >= n && (!V || ldv >= n), "ds_bem_assemble: bad sizes");
    DS_REQUIRE(k >= 0.f, "ds_bem_assemble: wave number must be >= 0");
    const int64_t ntile = ds::ceil_div(n, (int64_t)ASM_COLS);
    const int64_t rblocks = ds::ceil_div(n, (int64_t)ASM_ROWS);
    DS_REQUIRE(rblocks < 65536 * 1024LL && ntile < ((int64_t)1 << 31), "ds_bem_assemble: n too large");
    float2* part = reinterpret_cast<float2*>(work);
    bem_assemble_kernel<<<dim3((unsigned)ntile, (unsigned)rblocks), 256, 0, ds::as_stream(stream)>>>(
        rec, n, k, reinterpret_cast<const float2*>(g), reinterpret_cast<float2*>(A), lda, reinterpret_cast<float2*>(V), ldv,
        part, ntile);
    DS_LAUNCH_CHECK("bem_assemble_kernel");
    bem_rhs_kernel<<<(unsigned)ds::ceil_div(n, (int64_t)256), 256, 0, ds::as_stream(stream)>>>(part, n, ntile,
                                                                                                reinterpret_cast<float2*>(rhs));
    DS_LAUNCH_CHECK("bem_rhs_kernel");
    return DS_OK;
}

extern "C" int ds_bem_cgemv(const float* A, int64_t lda, const float* x, int64_t n, const float* scale, float* y, ds_stream_t stream) {
    DS_REQUIRE(A && x && y, "ds_bem_cgemv: null pointer");
    DS_REQUIRE(n > 0 && lda >= n && lda % 2 == 0, "ds_bem_cgemv: need n > 0 and an even lda >= n");
    const uintptr_t al = reinterpret_cast<uintptr_t>(A) | reinterpret_cast<uintptr_t>(x);
    DS_REQUIRE((al & 15) == 0, "ds_bem_cgemv: A and x must be 16-byte aligned");
    const int64_t blocks = ds::ceil_div(n, (int64_t)4);
    DS_REQUIRE(blocks < ((int64_t)1 << 31), "ds_bem_cgemv: n too large");
    bem_cgemv_kernel<<<(unsigned)blocks, 256, 0, ds::as_stream(stream)>>>(reinterpret_cast<const float2*>(A), lda,
                                                                           reinterpret_cast<const float2*>(x), n, scale,
                                                                           reinterpret_cast<float2*>(y));
    DS_LAUNCH_CHECK("bem_cgemv_kernel");
    return DS_OK;
}

extern "C" int ds_bem_potential(const float* rec, int64_t n, float k, const float* g, const float* u, const float* pts, int64_t np,
                                float* out, ds_stream_t stream) {
    DS_REQUIRE(rec && g && u && pts && out, "ds_bem_potential: null pointer");
    DS_REQUIRE(n > 0 && np > 0, "ds_bem_potential: empty input");
    DS_REQUIRE(k >= 0.f, "ds_bem_potential: wave number must be >= 0");
    const int64_t blocks = ds::ceil_div(np, (int64_t)256);
    DS_REQUIRE(blocks < ((int64_t)1 << 31), "ds_bem_potential: too many points");
    bem_potential_kernel<<<(unsigned)blocks, 256, 0, ds::as_stream(stream)>>>(
        rec, n, k, reinterpret_cast<const float2*>(g), reinterpret_cast<const float2*>(u), pts, np, reinterpret_cast<float2*>(out));
    DS_LAUNCH_CHECK("bem_potential_kernel");
    return DS_OK;
}
