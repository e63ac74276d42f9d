/* diffsound_hip.h - C ABI of libdiffsound_hip.so (MI355X / gfx950 only).
 *
 * Drop-in boundary for DiffSound's modal-sound hot path.  The reference's only native-op
 * precedent on this path is
 *     void assemble_mass_matrix(const Tensor& vertices, const Tensor& tets, Tensor& values,
 *                               Tensor& rows, Tensor& cols, Tensor& element_mm,
 *                               const double density, const int order)
 *     (reference src/cuda/massMatrixDouble.h:14-15, bound in src/cuda/bind.cu:9-12),
 * whose conventions are kept: the CALLER allocates every input and output buffer, the op fills
 * outputs in place and owns nothing; errors surface to Python as RuntimeError.  Differences, on
 * purpose: plain pointers + sizes instead of torch types, an explicit hipStream_t instead of the
 * legacy default stream (reference src/include/macro.h:146-152), an int status + ds_last_error()
 * instead of C++ exceptions, and no global mutable state besides the opaque host-side pattern
 * handle.  Every function is asynchronous on `stream` unless stated otherwise; none allocates or
 * synchronises, so all of them can be captured into a hipGraph.
 *
 * Layout conventions
 *   - DOF ordering: global DOF 3*node + c (reference src/diffelastic/deform.py:118-125).
 *   - K, K_lambda, K_mu: BSR with 3x3 blocks on the node-adjacency pattern (rowptr[nv+1],
 *     colidx[nnzb], ascending per row), values [nnzb][3][3] row-major.
 *   - M = M_s (x) I3 is stored as the node-level scalar CSR M_s on the same pattern: values [nnzb].
 *   - dense blocks X are row-major (n x ncols) with an explicit leading dimension `ld` (elements)
 *     so that column slices of a wider buffer can be passed without copies.
 *   - dtype codes: DS_F32 = 0, DS_F64 = 1.
 */
#ifndef DIFFSOUND_HIP_H
#define DIFFSOUND_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* ds_stream_t; /* hipStream_t */

enum { DS_F32 = 0, DS_F64 = 1 };
enum { DS_OK = 0, DS_ERR_ARG = 1, DS_ERR_HIP = 2, DS_ERR_NOMEM = 3 };

/* Thread-local text of the last error returned on this thread ("" if none). */
const char* ds_last_error(void);
/* Library ABI version (bumped on any signature change); ds_abi_version() returns the value the library was built with. */
#define DS_ABI_VERSION 45
int ds_abi_version(void);

/* ------------------------------------------------------------------------------------------------
 * Symbolic phase (HOST, CPU only): node-adjacency BSR pattern + per-block contribution lists.
 * Replaces the reference's COO triplet emission + coalesce() (src/diffelastic/diff_model.py:
 * 214-220, 299-312; src/cuda/massMatrixDouble.cu:70-77).  Once per mesh topology.
 *   tets   : (T x N) int32 host array, N = 4 (ord-1) or 10 (ord-2), reference local node order
 *            (src/diffelastic/mesh.py:139-154).
 * Contribution id of element t, local pair (a,b):  t*N*N + a*N + b.
 * ---------------------------------------------------------------------------------------------- */
typedef struct ds_pattern ds_pattern_t;
int ds_pattern_build(const int32_t* tets, int64_t T, int N, int64_t nv, int nthreads, ds_pattern_t** out);
int ds_pattern_sizes(const ds_pattern_t* p, int64_t* nv, int64_t* nnzb, int64_t* ncontrib);
/* Copies into caller-allocated HOST arrays: rowptr[nv+1], colidx[nnzb], diagidx[nv] (slot of block
 * (i,i)), cptr[nnzb+1], clist[ncontrib] (contribution ids grouped by block slot, ascending). */
int ds_pattern_export(const ds_pattern_t* p, int32_t* rowptr, int32_t* colidx, int32_t* diagidx,
                      int32_t* cptr, int32_t* clist);
void ds_pattern_free(ds_pattern_t* p);

/* Node groups of the neighbour-union SpMM (HOST): 4 consecutive nodes share one wave and walk the union of
 * their column lists.  Exports gptr[ngroups+1], gent[ne] (column id | presence mask << 28), goff[ne+1] (block
 * offsets into the group-ordered value copy) and kperm[nnzb] (group-ordered position -> BSR slot). */
typedef struct ds_groups ds_groups_t;
int ds_groups_build(const int32_t* rowptr, const int32_t* colidx, int64_t nv, ds_groups_t** out);
int ds_groups_sizes(const ds_groups_t* g, int64_t* ngroups, int64_t* ne);
int ds_groups_export(const ds_groups_t* g, int32_t* gptr, int32_t* gent, int32_t* goff, int32_t* kperm);
void ds_groups_free(ds_groups_t* g);

/* The same symbolic phase ON THE DEVICE (csrc/dpattern.hip): pattern, contribution lists, neighbour-union tables and
 * the chunk tables (every group of 4 rows cut into chunks of whole entries with at most cap_blocks entries / blocks;
 * almost always one chunk per group) from device connectivity, entry for entry what ds_pattern_build +
 * ds_groups_build and the host cutting rule produce.  The handle owns device arrays; ds_dpattern_build synchronises
 * `stream` (the table sizes come back to the host); ds_dpattern_export copies into caller-allocated DEVICE arrays (any
 * pointer may be NULL): rowptr[nv+1], colidx[nnzb], diagidx[nv], cptr[nnzb+1], clist[ncontrib], gptr[ngroups+1],
 * gent[ne], goff[ne+1], kperm[nnzb], utab[ngroups x 2] (chunk range of each group), ctab[nchunks x 4] (e0, e1, b0, b1).
 * (reference: COO triplets + coalesce() on every assembly, src/diffelastic/diff_model.py:214-220, 299-312, for a mesh
 * that the geometry experiments rebuild every iteration, src/dmtet/geometry/dmtet_thickness.py:251) */
typedef struct ds_dpattern ds_dpattern_t;
int ds_dpattern_build(const int32_t* tets, int64_t T, int N, int64_t nv, int cap_blocks, ds_stream_t stream,
                      ds_dpattern_t** out);
int ds_dpattern_sizes(const ds_dpattern_t* p, int64_t* nnzb, int64_t* ncontrib, int64_t* ne, int64_t* ngroups,
                      int64_t* nchunks);
int ds_dpattern_export(const ds_dpattern_t* p, int32_t* rowptr, int32_t* colidx, int32_t* diagidx, int32_t* cptr,
                       int32_t* clist, int32_t* gptr, int32_t* gent, int32_t* goff, int32_t* kperm, int32_t* utab,
                       int32_t* ctab, ds_stream_t stream);
void ds_dpattern_free(ds_dpattern_t* p);

/* Mesh front end ON THE DEVICE (csrc/dpattern.hip), replacing the float-`unique` of the reference's ord-2 lifting and
 * duplicate merge (src/diffelastic/mesh.py:101-179), which the geometry experiments run on a new mesh every iteration
 * (src/dmtet/geometry/dmtet_thickness.py:251-285).  Both synchronise `stream` (a count comes back to the host).
 *  ds_edge_table  : tets (T x 4) int64 DEVICE (torch long) -> the distinct undirected edges, ea[i] < eb[i], sorted by
 *                   (ea, eb) (arrays of capacity 6 T), and tet_edge (T x 6): the edge id of each local edge in the
 *                   reference's order (0,1) (1,2) (0,2) (0,3) (1,3) (2,3); *n_edges on the HOST.
 *  ds_unique_rows3: xyz (n x 3) fp32 DEVICE -> inv[n] (id of every row among the distinct rows in lexicographic
 *                   (x, y, z) order; -0.0 == +0.0 as in torch.unique) and first[id] = lowest row index with that
 *                   coordinate (capacity n); *n_unique on the HOST. */
int ds_edge_table(const int64_t* tets, int64_t T, int64_t nv, int64_t* ea, int64_t* eb, int64_t* tet_edge,
                  int64_t* n_edges, ds_stream_t stream);
int ds_unique_rows3(const float* xyz, int64_t n, int64_t* inv, int64_t* first, int64_t* n_unique, ds_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Numeric assembly (DEVICE).  K_lambda, K_mu (geometry-only parts of K = lam*K_lambda + mu*K_mu,
 * SURVEY.md 0.6) and M_s in one pass, fp64, deterministic (no atomics): one thread per block slot
 * sums its contribution list in fixed order.  Restates update_stiff_matrix / update_mass_matrix
 * (reference src/diffelastic/diff_model.py:184-312) with the element integrals in closed form over
 * the reference's own Gauss rule (tables built by the host from src/diffelastic/gauss.py:17-38).
 *   verts  : (nv x 3) f32 device          tets : (T x N) i32 device
 *   dtab   : (N x 4 x N x 4) f64 device,  dtab[a][k][b][l] = sum_g w_g dN_a/dL_k dN_b/dL_l
 *   mtab   : (N x N) f64 device,          mtab[a][b]       = sum_g w_g N_a N_b   (already * density
 *            in fp32 where the reference does so, diff_model.py:301-303)
 *   tetgeo : workspace (T x 13) f64 device (barycentric gradients 4x3 + |det|)
 *   out    : klam, kmu (nnzb x 9) f64 ; ms (nnzb) f64
 * ---------------------------------------------------------------------------------------------- */
int ds_assemble_kml(const float* verts, const int32_t* tets, int64_t T, int N, int64_t nv,
                    const int32_t* cptr, const int32_t* clist, int64_t nnzb,
                    const double* dtab, const double* mtab, double* tetgeo,
                    double* klam, double* kmu, double* ms, ds_stream_t stream);

/* K32 = (float)(lam*K_lambda + mu*K_mu) (k32t: the same with every 3x3 block transposed, may be NULL),
 * Ms32 = (float)M_s, and the fp32 inverse of the 3x3 diagonal blocks of K (block-Jacobi preconditioner).
 * Per material hypothesis. */
int ds_combine_material(const double* klam, const double* kmu, const double* ms, int64_t nnzb,
                        const int32_t* diagidx, int64_t nv, double lam, double mu,
                        float* k32, float* k32t, float* ms32, float* dinv32, ds_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Block SpMM  Y = A X  on the BSR-3 pattern (the HBM-roofline kernel; csrc/spmm.hip).  Replaces torch.sparse.mm
 * in the reference's LOBPCG (src/lobpcg/_linalg_utils.py:36-37) and in get_vals
 * (src/diffelastic/diff_model.py:395-397).
 *   kind 0: A = K,   vals (nnzb x 9) f32           X, Y f32
 *   kind 1: A = M,   vals (nnzb)     f32 (M_s)     X, Y f32
 *   kind 2: A = K_*, vals (nnzb x 9) f64           X f32, Y f64   (polish / read-out)
 *   kind 3: A = M,   vals (nnzb)     f64 (M_s)     X f32, Y f64
 *   kind 4: A = K_*, vals (nnzb x 9) f64           X f64, Y f64   (fp64 refinement; ncols % 4 == 0, <= 84,
 *   kind 5: A = M,   vals (nnzb)     f64 (M_s)     X f64, Y f64    32-byte aligned rows)
 * vals_t (kind 0 only, may be NULL): the same blocks stored transposed, vals_t[k][r][i] = K_k[i][r]
 *   (ds_combine_material writes it); enables the one-load-per-block path for ncols <= 84.
 * X: (3nv x ncols) ld = ldx ; Y: (3nv x ncols) ld = ldy ; X and Y must not overlap.
 * ---------------------------------------------------------------------------------------------- */
int ds_spmm_bsr3(int kind, const int32_t* rowptr, const int32_t* colidx, const void* vals,
                 const void* vals_t, int64_t nv, const void* X, int64_t ldx, void* Y, int64_t ldy, int ncols,
                 ds_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Tall-skinny Gram  G = A^T B  (p x q, fp64, row-major, ld = q) with MFMA.
 * Replaces the dense (k x n)(n x k) products of Rayleigh-Ritz / svqb / ortho in the reference
 * (src/lobpcg/_linalg_utils.py:64-73 via torch.matmul).
 *   A: (n x p) f32 or f64 (a_dtype; an f64 A needs an f64 B), lda ;  B: (n x q) f32 or f64 (b_dtype), ldb
 *   flags: DS_GRAM_SYMMETRIC (needs p == q): the caller asserts G is symmetric (e.g. S^T (K S)); only the
 *     block-upper part is computed and mirrored.
 *     DS_GRAM_EXACT: exact products, fp64 accumulation throughout (fp64 MFMA).  Without it an f32 x f32 product
 *     runs on the fp32 MFMA with the accumulators folded into fp64 every 48 rows (error ~1e-9 |A_i||B_j|, far
 *     below the operands' own fp32 rounding) at twice the rate; an f64 B always takes the exact path.
 *   work: device scratch of ds_gram_workspace_bytes(n, p, q) bytes.
 * ---------------------------------------------------------------------------------------------- */
int64_t ds_gram_workspace_bytes(int64_t n, int p, int q);
#define DS_GRAM_SYMMETRIC 1
#define DS_GRAM_EXACT 2
int ds_gram(const void* A, int a_dtype, int64_t lda, int p, const void* B, int b_dtype, int64_t ldb, int q,
            int64_t n, int flags, double* G, void* work, int64_t work_bytes, ds_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Fused block-vector updates of the eigensolver (all (n x ncols) f32 with leading dimensions).
 * ---------------------------------------------------------------------------------------------- */
/* R <- KX - MX * diag(lam) ;  rn2[j] = ||R_j||^2, xn2[j] = ||X_j||^2 (f64, zeroed by this call).  KX may be R (in place).
 * (reference update_residual + the norms of update_converged_count, _lobpcg.py:301-333) */
int ds_residual(const float* KX, int64_t ldk, float* R, int64_t ldr, const float* MX, int64_t ldm, const float* X,
                int64_t ldx, const double* lam, int64_t n, int ncols, double* rn2, double* xn2, ds_stream_t stream);
/* D <- c * T R ; W <- D      (T = block-Jacobi, dinv (nv x 9) f32) */
int ds_cheb_init(const float* R, int64_t ldr, float* D, int64_t ldd, float* W, int64_t ldw,
                 const float* dinv, int64_t nv, int ncols, float c, ds_stream_t stream);
/* R <- R - AD ; D <- c1 D + c2 T R ; W <- W + D */
int ds_cheb_step(const float* AD, int64_t lda, float* R, int64_t ldr, float* D, int64_t ldd,
                 float* W, int64_t ldw, const float* dinv, int64_t nv, int ncols, float c1, float c2,
                 ds_stream_t stream);
/* One fused term of the Chebyshev block-Jacobi polynomial preconditioner (three-term form):
 *   W_next <- W + c1 (W - W_prev) + c2 T (R0 - K W),   written over W_prev ;  first != 0: W_prev = 0, not read.
 * K: (rowptr, colidx, vals f32 (nnzb x 9)); ncols a multiple of 4, <= 84; W and W_prev distinct buffers. */
int ds_cheb_spmm(const int32_t* rowptr, const int32_t* colidx, const float* vals, int64_t nv,
                 const float* W, int64_t ldw, float* Wprev, int64_t ldp, const float* R0, int64_t ldr,
                 const float* dinv, int ncols, float c1, float c2, int first, ds_stream_t stream);
/* Y <- R0 - K X on a block of <= 84 columns (X, Y distinct): the fine-level residual that the two-level
 * preconditioner restricts to the corner-node level; K X itself is never written. */
int ds_spmm_residual(const int32_t* rowptr, const int32_t* colidx, const float* vals, int64_t nv,
                     const float* X, int64_t ldx, const float* R0, int64_t ldr, float* Y, int64_t ldy,
                     int ncols, ds_stream_t stream);
/* Y_i <- beta Y_i + sum_k w[k] X_{colidx[k]}, k in [rowptr[i], rowptr[i+1]), on 3 x ncols node panels
 * (nrows output nodes; X may have a different node count): prolongation / restriction between an ord-2
 * mesh and its corner-node ord-1 sub-mesh (the P1 space written in the P2 nodal basis; node layout of
 * reference src/diffelastic/mesh.py:139-154).  ncols a multiple of 4, 16-byte aligned rows. */
int ds_scalar_csr_spmm(const int32_t* rowptr, const int32_t* colidx, const float* w, int64_t nrows,
                       const float* X, int64_t ldx, float* Y, int64_t ldy, int ncols, float beta,
                       ds_stream_t stream);
/* kgrp: (nnzb x 9) f32 = the TRANSPOSED blocks in group order, kgrp[p] = vals_t[kperm[p]] (tables of ds_groups_build). */
/* The three fp64-value products of the read-out in one walk of the pattern (the panels of X are gathered once instead of
 * three times): Ya = A X, Yb = B X with (nnzb x 9) fp64 blocks (K_lambda, K_mu), Ym = (m (x) I3) X with nnzb fp64 node
 * scalars (M_s); X fp32, results fp64, ncols a multiple of 4 <= 84, 16-byte aligned rows.  Bit-identical to ds_spmm_bsr3
 * kinds 2, 2, 3.  csrc/spmm_f64.hip.  (reference: the autograd read-out of get_undamped_freqs, src/diffelastic/diff_model.py:371-388) */
int ds_spmm_f64_polish(const int32_t* rowptr, const int32_t* colidx, const double* a, const double* b, const double* m,
                       int64_t nv, const float* X, int64_t ldx, double* Ya, double* Yb, double* Ym, int64_t ldy, int ncols,
                       ds_stream_t stream);
/* fp64 values with fp64 (x_f64 != 0) or fp32 vectors on the neighbour-union tables of ds_spmm_union (ABI 28): Y (fp64) = A X for a
 * block of <= 84 columns, one wave per group of 4 nodes walking the union of their neighbours - the fp64 refinement's K W / M W
 * (ds_spmm_bsr3 kinds 4 / 5 gather every neighbour's panel once per ROW: 2.2 x the panels).  vals: kind 0 = the 3x3 blocks in
 * the tables' group order, TRANSPOSED (vals[p][g][i] = A_block[i][g], 9 doubles per block, i.e. ds_pack_groups' layout in fp64);
 * kind 1 = node scalars in that order (A = a (x) I3).  Equal to ds_spmm_bsr3's results to fp64 rounding (another summation order).
 * csrc/spmm_f64.hip, kernel in spmm_f64_union.inc.  (reference: torch.sparse.mm of src/lobpcg/_linalg_utils.py:36-37 in fp64) */
int ds_spmm_f64_union(int kind, int x_f64, const int32_t* utab, const int32_t* ctab, int64_t ngroups, int cap_blocks,
                      const int32_t* gent, const double* vals, int64_t nnzb, int64_t nv, const void* X, int64_t ldx, double* Y,
                      int64_t ldy, int ncols, ds_stream_t stream);
/* The same three products stored as fp32 blocks (ABI 28): the sums are formed in fp64 and rounded once.  Halves what the
 * kernel writes and the Gram product behind it reads; an OPTION of the eigensolver's polish (off by default: the polish then
 * carries ~3e-8 of relative noise instead of being accurate to second order in the iteration error). */
int ds_spmm_f64_polish_f32out(const int32_t* rowptr, const int32_t* colidx, const double* a, const double* b,
                              const double* m, int64_t nv, const float* X, int64_t ldx, float* Ya, float* Yb, float* Ym,
                              int64_t ldy, int ncols, ds_stream_t stream);
int ds_pack_groups(const float* vals_t, const int32_t* kperm, int64_t nnzb, float* kgrp, ds_stream_t stream);
/* Neighbour-union form of ds_spmm_bsr3 / ds_cheb_spmm / ds_spmm_residual for ncols <= 84 (the eigensolver's
 * b-column products and every preconditioner term): one wavefront per group of 4 consecutive nodes walks the UNION
 * of their neighbours, so a neighbour panel shared inside the group is gathered once (Morton order: 0.58 x the
 * panel loads of one wavefront per node).  Tables from ds_groups_build - gent (union entries col | mask << 28),
 * kgrp (TRANSPOSED 3x3 blocks in group order, ds_pack_groups) - cut into chunks of whole entries with at most
 * cap_blocks (<= DS_UNION_CAP = 140) blocks: ctab (nchunks x 4) = (e0, e1, b0, b1), utab (ngroups x 2) = chunk range of each
 * group, ngroups = ceil(nv / 4); utab may be NULL when every group is exactly one chunk (ctab has ngroups rows).
 * epilogue 0: Y <- A X ; 1: Y (= W_prev) <- X + c1 (X - Y) + c2 T (R0 - A X) (first != 0: Y not read) ;
 * (Wprev != NULL, epilogue 1 only: W_prev is read from there and Y is only written - out-of-place form) ;
 * 2: Y <- R0 - A X ; 3: Y <- (A_s (x) I3) X with kgrp = the node-SCALAR values in group order (nnzb floats: the mass
 * matrix).  X and Y distinct, 16-byte aligned rows; operand blocks of 2 GB and more (3 nv ld 4 >= 0x7f000000 bytes)
 * take a variant that builds one buffer descriptor per panel load.
 * level_tag (0 fine, 1 corner-node level) selects instantiations of epilogues 0 and 3 whose kernel symbols differ - nothing else.
 * This and the other fp32 / bf16 walks of these tables: csrc/spmm_union.hip, kernels in spmm_union.inc and spmm_narrow.inc.
 * (reference: torch.sparse.mm in src/lobpcg/_linalg_utils.py:36-37 and the iK callable of _lobpcg.py:441) */
#define DS_UNION_CAP 140
int ds_spmm_union(int epilogue, int level_tag, const int32_t* utab, const int32_t* ctab, int64_t ngroups, int cap_blocks,
                  const int32_t* gent, const float* kgrp, int64_t nnzb, int64_t nv, const float* X, int64_t ldx,
                  float* Y, int64_t ldy, const float* R0, int64_t ldr, const float* dinv, int ncols, float c1, float c2,
                  int first, const float* Wprev, int64_t ldp, ds_stream_t stream);
/* The eigensolver's residual in ONE walk of the neighbour unions (ABI 26): R <- K X - (M_s (x) I3) X diag(lam) on a block of
 * <= 84 columns, and rn2[j] = ||R_j||^2, xn2[j] = ||X_j||^2 (fp64) - what ds_spmm_union (epilogue 0), ds_spmm_union
 * (epilogue 3) and ds_residual compute in three launches and five passes over (n x ncols) blocks (reference:
 * update_residual / update_converged_count, src/lobpcg/_lobpcg.py:301-333).  kgrp / mgrp: the transposed 3x3 blocks and the
 * node-scalar mass values in group order, as for ds_spmm_union; lam: ncols Ritz values on the device (fp64, rounded to fp32 as
 * ds_residual does).  R equals the three-launch result bit for bit; the norms are summed over the groups in a fixed order (no
 * atomics: reproducible, which ds_residual's are not).  work: ds_union_residual_workspace_bytes(ngroups, ncols) bytes. */
int64_t ds_union_residual_workspace_bytes(int64_t ngroups, int ncols);
int ds_union_residual(int level_tag, const int32_t* utab, const int32_t* ctab, int64_t ngroups, int cap_blocks,
                      const int32_t* gent, const float* kgrp, const float* mgrp, int64_t nnzb, int64_t nv, const float* X,
                      int64_t ldx, const double* lam, float* R, int64_t ldr, int ncols, void* work, int64_t work_bytes,
                      double* rn2, double* xn2, ds_stream_t stream);
/* The same walk when the preconditioner that follows is the bf16 two-level cycle (ABI 41; epilogue 6 of the kernel, fine level
 * only: level_tag 0).  Instead of the fp32 R it writes what the cycle's first launch (ds_cheb_init16 on R) would write: R16, the
 * bf16 copy of R, and W1 = c T R, the first Chebyshev iterate of the fine smoother (bf16; T = dinv, the (nv x 9) node blocks,
 * c = 2 / (lmax + lmin)) - both bit for bit what ds_union_residual followed by ds_cheb_init16 produce; rn2 / xn2 as above.
 * ds_twolevel_apply with DS_TL_PREPARED in its storage flags then starts at its first term.  R16 / W1: bf16 blocks, leading dimensions in elements,
 * 8-byte aligned rows. */
int ds_union_residual_pre(int level_tag, const int32_t* utab, const int32_t* ctab, int64_t ngroups, int cap_blocks,
                          const int32_t* gent, const float* kgrp, const float* mgrp, int64_t nnzb, int64_t nv, const float* X,
                          int64_t ldx, const double* lam, const float* dinv, float c, void* R16, int64_t ldr16, void* W1,
                          int64_t ldw1, int ncols, void* work, int64_t work_bytes, double* rn2, double* xn2, ds_stream_t stream);
/* Narrow blocks (ABI 28): Y = K X (kind 0, vals = kgrp) or Y = (M_s (x) I3) X (kind 3, vals = mgrp) on <= 16 columns with the
 * lanes of a wave dealt over the union's ENTRIES instead of over the columns (ds_spmm_union keeps 6 of 64 lanes busy on an
 * 8-column block and takes as long as on 80 columns): the block power iteration of the Chebyshev interval and the operator-norm
 * estimates of the eigensolver.  Same tables as ds_spmm_union; sums in another order: equal to it to fp32 rounding, not bit for
 * bit.  (reference: the operator-norm estimates of src/lobpcg/_lobpcg.py:280-285) */
int ds_spmm_union_narrow(int kind, int level_tag, const int32_t* utab, const int32_t* ctab, int64_t ngroups, const int32_t* gent,
                         const float* vals, int64_t nnzb, int64_t nv, const float* X, int64_t ldx, float* Y, int64_t ldy,
                         int ncols, ds_stream_t stream);
/* Y = K X and Y2 = (M_s (x) I3) X of ONE block (<= 84 columns) in one walk of the neighbour unions (ABI 28; epilogue 5 of the
 * kernel): X is gathered once instead of twice; each product is formed exactly as ds_spmm_union's epilogues 0 and 3 form it
 * (bit-identical results).  The eigensolver's K W and M W of the raw preconditioned residuals (ds_lobpcg_t.raw_rr).
 * (reference: the two torch.sparse.mm of _lobpcg.py:441-459 on the same block) */
int ds_spmm_union_km(int level_tag, const int32_t* utab, const int32_t* ctab, int64_t ngroups, int cap_blocks,
                     const int32_t* gent, const float* kgrp, const float* mgrp, int64_t nnzb, int64_t nv, const float* X,
                     int64_t ldx, float* KX, int64_t ldk, float* MX, int64_t ldm, int ncols, ds_stream_t stream);
/* ------------------------------------------------------------------------------------------------
 * Two-level V-cycle preconditioner in one call (host-side driver, csrc/vcycle.cpp): issues on `stream` the launch
 * sequence  W1 = S R ; W2 = W1 + P C P^T (R - K W1) ; W = W2 + S (R - K W2)  out of ds_cheb_init, ds_spmm_union and
 * ds_scalar_csr_spmm - S: degree-`fine.degree` Chebyshev block-Jacobi smoother for the interval [lmin, lmax] of T K
 * on the fine level, C: the same on the corner-node level, P / P^T the transfer operators.  The preconditioner of
 * the reference's LOBPCG is an opaque callable (src/lobpcg/_lobpcg.py:441); this is the one diffsound_amd supplies.
 * All blocks (rows x ncols) f32 with leading dimensions, 16-byte aligned rows, ncols a multiple of 4 <= 84; R is only
 * read; Wc, D, AD (one common leading dimension), Rr (fine) and Rc, Ec, Dc, ADc (corner-node level, common leading
 * dimension ldc) are scratch.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    const int32_t* utab;   /* neighbour-union tables and values of the level, as for ds_spmm_union */
    const int32_t* ctab;
    int64_t ngroups;
    int32_t cap_blocks;
    int32_t degree;        /* polynomial degree of the level's Chebyshev block-Jacobi operator */
    const int32_t* gent;
    const float* kgrp;
    int64_t nnzb;
    int64_t nv;
    const float* dinv;     /* (nv x 9) inverse diagonal blocks */
    double lmax, lmin;     /* the polynomial targets [lmin, lmax] of T K */
    /* bf16 cycles only: mf_group_nodes = 8 sends the level's bf16 terms to ds_spmm_union16m (tables and the packed
     * blocks as described there); 0: ds_spmm_union16 */
    int32_t mf_group_nodes;
    int32_t mf_max_entries;
    int32_t mf_max_batch_blocks;
    int32_t level_tag;     /* 0: fine level, 1: corner-node level - selects kernel instantiations whose SYMBOLS differ, so
                              that a rocprofv3 kernel table separates the two levels' launches (same code otherwise) */
    const int32_t *mf_gptr, *mf_gcol, *mf_gmeta, *mf_gbase, *mf_ghead;
    const void* mf_kc;
    /* fp32 matrix-core form of the level's own products K X / M X (ds_spmm_union32m): m32_gptr != NULL enables it in
     * ds_lobpcg_iterate; tables for groups of 4 nodes, m32_k / m32_m the values in the tables' order (with 16 bytes of
     * slack behind the last block), m32_m may be NULL (mass matrix not node-scalar) */
    int32_t m32_max_entries;
    int32_t m32_max_batch_blocks;
    const int32_t *m32_gptr, *m32_gcol, *m32_gmeta, *m32_gbase;
    const float* m32_k;
    const float* m32_m;
    /* ABI 33, bf16 cycles on the matrix-core tables only: GROUP-block Jacobi.  tgrp != NULL: (ceil(nv / 8) x 24 x 24) f32, the
     * inverses T_g of the 24 x 24 diagonal blocks of the level's groups of 8 nodes (ds_group_inverse).  The level's polynomial is
     * then p(T_g K) T_g: its right-hand side goes through ds_group_apply16 first, mf_kc holds the blocks of T_g K (ds_group_pack_kc:
     * DENSE over node x entry, mf_gmeta / mf_gbase / mf_ghead with every presence bit set, mf_nblocks = 8 x the number of union
     * entries of the level) and dinv an identity per node.  NULL / 0: the node blocks (dinv) as before. */
    const float* tgrp;
    int64_t mf_nblocks;
} ds_level_t;
typedef struct {
    ds_level_t fine, coarse;
    const int32_t *rptr, *rcol;  /* restriction (corner node <- fine nodes) */
    const float* rw;
    const int32_t *pptr, *pcol;  /* prolongation (fine node <- corner nodes) */
    const float* pw;
    const float* R;
    int64_t ldr;
    float* W;
    int64_t ldw;
    float* D;
    int64_t ldd;
    float* AD;
    int64_t lda;
    float* Rr;
    int64_t ldrr;
    float *Rc, *Ec, *Dc, *ADc;
    int64_t ldc;
    int32_t ncols;
    float* Wc;       /* fine scratch: the cycle's iterate (compact), W itself is written once at the end */
    int64_t ldwc;    /* = ldd = lda */
    int32_t storage; /* flags (ABI 41; until then the values 0 and 1 only).  Bit 0: 0: every scratch block fp32 ; 1: every scratch block bf16 (same fields, 2-byte elements; R and W
                        stay fp32): the preconditioner's iterates need no more mantissa, and its terms are bound by
                        the bytes of their vector streams.
                        DS_TL_PREPARED (with bit 0 only): the cycle's inputs are already written (ds_union_residual_pre) - R16,
                        and the first iterate W1 of the fine smoother in the block the polynomial's first term reads (D; Wc when
                        fine.degree == 1) - so the cycle skips ds_cheb_init16 and R is not read at all.
                        DS_TL_OWN_INIT: read by ds_lobpcg_iterate only - its residual walk does NOT prepare this cycle's inputs
                        (the two launches, for comparison); without it the iteration hands them over whenever it can */
    void* R16;       /* storage 1: fine bf16 scratch for the copy of R (rows x ncols, leading dimension ldr16) */
    int64_t ldr16;
} ds_twolevel_t;
#define DS_TL_BF16 1
#define DS_TL_PREPARED 2
#define DS_TL_OWN_INIT 4
int ds_twolevel_apply(const ds_twolevel_t* p, ds_stream_t stream);
/* One-level form: W <- p(T K) T R with the level's degree / [lmin, lmax] (Chebyshev block-Jacobi polynomial, every term
 * one fused ds_spmm_union launch); a, b: compact scratch blocks (rows x ncols, leading dimension lds). */
int ds_chebyshev_apply(const ds_level_t* level, const float* R, int64_t ldr, float* W, int64_t ldw, float* a, float* b,
                       int64_t lds, int ncols, ds_stream_t stream);
/* ... with bf16 scratch blocks a, b, r16 (rows x ncols bf16, leading dimension lds); degree >= 2. */
int ds_chebyshev_apply16(const ds_level_t* level, const float* R, int64_t ldr, float* W, int64_t ldw, void* a, void* b,
                         void* r16, int64_t lds, int ncols, ds_stream_t stream);
/* bf16-block forms used by the bf16 V-cycle: the fused terms (X, R0, W_prev bf16; Y bf16, or fp32 when y_f32), the
 * first Chebyshev iterate W1 = c T R (R fp32 - then Rcopy, if not NULL, receives its bf16 copy - or bf16) and the level
 * transfer.  Leading dimensions in elements; bf16 rows 8-byte aligned. */
int ds_spmm_union16(int epilogue, const int32_t* utab, const int32_t* ctab, int64_t ngroups, int cap_blocks,
                    const int32_t* gent, const float* kgrp, int64_t nnzb, int64_t nv, const void* X, int64_t ldx,
                    void* Y, int64_t ldy, int y_f32, const void* R0, int64_t ldr, const float* dinv, int ncols,
                    float c1, float c2, int first, const void* Wprev, int64_t ldp, ds_stream_t stream);
/* MFMA form of ds_spmm_union16 (csrc/spmm_mfma.hip, kernels in spmm_mfma.inc): the same two epilogues on the same bf16 blocks, the block
 * products on the matrix cores (v_mfma_f32_16x16x16_bf16; the 3x3 blocks rounded to bf16, fp32 accumulation), one
 * wavefront per group of group_nodes = 8 consecutive nodes.  Topology tables (device): gptr (ngroups + 1) / gcol =
 * the sorted union of the column ids of each group's rows; gmeta per entry = presence mask of the group's nodes |
 * (index of the entry's first block inside the group) << 8; gbase (ngroups) = first block of each group; kperm = the
 * BSR block of every position of the group / entry / node order.  ds_pack_kc writes kc (nnzb x 3 x 4 bf16: the rows of
 * the blocks in that order, padded to 8 bytes) from the BSR values k32 - once per material.  max_entries = the largest
 * group's entry count (<= 256); max_batch_blocks = the largest number of blocks in DS_MF_BATCH = 16 consecutive entries
 * of a group (batches counted from the group's first entry; it sizes the wavefront's LDS) - when max_entries <= 128 the LAST
 * batch of a group also takes up to DS_MF_TAIL entries beyond the 16 (a group of 65 entries is four batches, not five), and
 * max_batch_blocks counts the blocks of the batches so formed.  ghead (ngroups x 128): per group
 * a record of FIXED stride with the first 64 entries of gcol (words 0..63) and of gmeta (words 64..127), zero behind the
 * group's last entry - a wavefront asks for it before it knows where the group's entries start (ABI 29). */
#define DS_MF_BATCH 16
#define DS_MF_TAIL 2
int ds_pack_kc(const float* k32, const int32_t* kperm, int64_t nnzb, void* kc, ds_stream_t stream);
/* ABI 33: the group-block Jacobi of the bf16 polynomial (ds_level_t.tgrp; reference: the preconditioner is the caller's opaque
 * callable, src/lobpcg/_lobpcg.py:441).  Groups of group_nodes = 8 consecutive nodes, ng = ceil(nv / 8).
 * ds_group_inverse: T (ng x 24 x 24 f32) = the inverses of the diagonal blocks K_gg of the BSR-3 matrix (rowptr, colidx, k32:
 *   nnzb x 9 f32), nodes behind the last one as identity rows; once per material.
 * ds_group_pack_kc: kc (8 x entries x 3 x 4 bf16) = the blocks of T_g K, dense: position (gptr[g] + e) * 8 + s' = sum_s
 *   T_g[s', s] K(s, e); gptr / gmeta / gbase / kperm are the COMPACT tables of ds_spmm_union16m on the same topology.
 * ds_group_apply16: Y = T_g X on (3 nv x ncols) blocks, ncols <= 256, X and Y each f32 (x_f32 / y_f32) or bf16; Y may be X when
 *   both have one element type. */
int ds_group_inverse(const int32_t* rowptr, const int32_t* colidx, const float* k32, int64_t nv, int group_nodes, float* T,
                     ds_stream_t stream);
int ds_group_pack_kc(const float* k32, const float* T, const int32_t* gptr, const int32_t* gmeta, const int32_t* gbase,
                     const int32_t* kperm, int group_nodes, int64_t nv, void* kc, ds_stream_t stream);
int ds_group_apply16(const float* T, int group_nodes, const void* X, int x_f32, int64_t ldx, void* Y, int y_f32, int64_t ldy,
                     int64_t nv, int ncols, ds_stream_t stream);
int ds_spmm_union16m(int epilogue, int group_nodes, int level_tag, const int32_t* gptr, const int32_t* gcol,
                     const int32_t* gmeta, const int32_t* gbase, const int32_t* ghead, const void* kc, int64_t nnzb, int64_t ngroups, int max_entries,
                     int max_batch_blocks, int64_t nv, const void* X, int64_t ldx, void* Y, int64_t ldy, int y_f32,
                     const void* R0, int64_t ldr,
                     const float* dinv, int ncols, float c1, float c2, int first, const void* Wprev, int64_t ldp,
                     ds_stream_t stream);
/* fp32 matrix-core form of ds_spmm_union epilogues 0 and 3 (csrc/spmm_mfma32.hip, kernel in spmm_mfma32.inc) - the eigensolver's own products
 * K W, M W, M X on fp32 blocks of <= 84 columns (reference: torch.sparse.mm in src/lobpcg/_linalg_utils.py:36-37):
 * one wavefront per group of 4 consecutive nodes, the gathered panels of a batch of DS_MF32_BATCH union entries staged
 * in LDS as the B operand of v_mfma_f32_16x16x4_f32 (exact fp32: one rounding per product), the 3x3 blocks (epilogue 0:
 * `vals` = nblocks x 9 floats, row-major blocks) or node-scalar values (epilogue 3: nblocks floats) of the batch staged
 * beside them and spread over the 16 x 4 A tile.  Tables as for ds_spmm_union16m but for groups of 4 nodes (gmeta = 4-bit
 * presence mask | first block inside the group << 8), values in the tables' (group, entry, node) order with at least 16
 * bytes of slack behind the last block (vals_bytes = the readable size); max_batch_blocks = the largest number of blocks
 * in DS_MF32_BATCH consecutive entries of a group (batches counted from the group's first entry).  Per output element
 * the products are summed in ONE chain in entry order - the same precision as ds_spmm_union, whose three chains (one per
 * panel row) are added at the end: results agree to fp32 rounding, not bit for bit.  level_tag as in ds_level_t. */
#define DS_MF32_BATCH 8
int ds_spmm_union32m(int epilogue, int level_tag, const int32_t* gptr, const int32_t* gcol, const int32_t* gmeta,
                     const int32_t* gbase, const float* vals, int64_t vals_bytes, int64_t nblocks, int64_t ngroups,
                     int max_entries, int max_batch_blocks, int64_t nv, const float* X, int64_t ldx, float* Y, int64_t ldy,
                     int ncols, ds_stream_t stream);
int ds_cheb_init16(const void* R, int r_f32, int64_t ldr, void* W, int64_t ldw, void* Rcopy, int64_t ldc,
                   const float* dinv, int64_t nv, int ncols, float c, ds_stream_t stream);
int ds_scalar_csr_spmm16(const int32_t* rowptr, const int32_t* colidx, const float* w, int64_t nrows, const void* X,
                         int64_t ldx, void* Y, int64_t ldy, int ncols, float beta, ds_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * The eigensolver's iteration as ONE native call (csrc/lobpcg.cpp; its dense steps: csrc/host_dense.cpp): the loop of the reference's LOBPCG.run /
 * _update_ortho (src/lobpcg/_lobpcg.py:344-376, 433-477) in the re-designed form of lobpcg/modal_solver.py - residual
 * test, hard locking, preconditioner, single-sweep projected Cholesky-QR, Rayleigh-Ritz by recurrence, basis update -
 * issued on `stream`; the <= 3b x 3b dense steps run on the calling thread with the LAPACK / BLAS routines of
 * ds_lapack_t (Fortran calling convention, e.g. SciPy's cython_lapack / cython_blas function pointers).  Synchronises
 * the stream a few times per iteration (residual norms, Gram blocks).
 * On entry: S = [Y (ny rigid columns, 0 or a multiple of 4) | X (b Ritz vectors, M-orthonormal) | - | -], KS[:, :b] = K X,
 * lam = the b Ritz values, S2[:, :ny] = Y.  On exit: the basis buffer holding X (S2 if result_in_s2), lam, rerr (per
 * column: ||K x - lam M x|| / (||x|| (A_norm + |lam| B_norm))), iterations.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    void (*dsyevd)(char* jobz, char* uplo, int* n, double* a, int* lda, double* w, double* work, int* lwork, int* iwork,
                   int* liwork, int* info);
    void (*dgemm)(char* ta, char* tb, int* m, int* n, int* k, double* alpha, double* a, int* lda, double* b, int* ldb,
                  double* beta, double* c, int* ldc);
    /* ABI 31, optional (all three or none; NULL = the Ritz step calls dsyevd): the stages of dsyevd one by one, so that only the
     * wanted third of the eigenvectors of the 3 na x 3 na Ritz problem is back-transformed */
    void (*dsytrd)(char* uplo, int* n, double* a, int* lda, double* d, double* e, double* tau, double* work, int* lwork, int* info);
    void (*dstedc)(char* compz, int* n, double* d, double* e, double* z, int* ldz, double* work, int* lwork, int* iwork,
                   int* liwork, int* info);
    void (*dormtr)(char* side, char* uplo, char* trans, int* m, int* n, double* a, int* lda, double* tau, double* c, int* ldc,
                   double* work, int* lwork, int* info);
} ds_lapack_t;
typedef struct {
    int64_t n, nv;            /* n = 3 nv rows */
    int32_t b, k, ny;         /* block width (multiple of 4, <= 160: products of more than 84 columns run in column slices),
                                 wanted pairs, rigid columns */
    int32_t maxit, lock, ortho_passes, rr_refresh, gram_exact;
    int32_t kx_fresh;         /* != 0: K X' of the new Ritz block by ONE product K X' (b columns) instead of the update
                                 [K X' | K P'] = K [X P W] [Z1 Zp] (3b -> 2b columns) - K P is then never formed: the Gram
                                 blocks among X and P come from the small Ritz algebra, only the residual needs K X */
    int32_t raw_rr;           /* != 0 (needs kx_fresh and res_work): Rayleigh-Ritz on the RAW basis [Y X P W], W = the preconditioned
                                 residuals as they come - K W and M W in one walk (ds_spmm_union_km), ONE Gram launch
                                 [Y X P W]^T [K W | M W], the orthonormalisation of W against [Y X P] folded into the small dense
                                 algebra and into the coefficients of ONE update [X' P'] = [Y X P W] Z; an iteration whose W is
                                 too ill-conditioned for that (eps x amplification >= ortho_tol) takes the explicit route */
    double tol, ortho_tol, A_norm, B_norm;
    float *S, *S2;            /* (n x (ny + 3 b)), leading dimension lds */
    float *KS, *KS2;          /* (n x 3 b), leading dimension ldks */
    float *R, *MX, *MW;       /* (n x b), leading dimension ldr */
    int64_t lds, ldks, ldr;
    ds_level_t level;         /* K of this level: neighbour-union tables + block-Jacobi blocks; degree / lmin / lmax of
                                 the one-level polynomial when twolevel == NULL */
    const float* mgrp;        /* node-scalar mass values in group order (ds_spmm_union epilogue 3) */
    const int32_t *rowptr, *colidx;   /* BSR pattern and values for the wide products of the periodic full refresh */
    const float *k32, *k32t;
    const ds_twolevel_t* twolevel;    /* two-level preconditioner (scratch blocks with >= b columns), or NULL */
    float *pa, *pb;           /* one-level preconditioner scratch (n x b), leading dimension ldp */
    int64_t ldp;
    void* pr16;               /* not NULL: pa, pb, pr16 are bf16 blocks and the polynomial runs on bf16 iterates */
    double* gbuf;             /* device, (ny + 3 b) x 3 b doubles: Gram results */
    float* cbuf;              /* device, 8 x (ny + 3 b) x 2 b floats: update coefficients (a ring of 8 slots) */
    double* nrm;              /* device, 2 x 1024 doubles */
    double* lam_dev;          /* device, b doubles */
    void* res_work;           /* not NULL (and kx_fresh != 0): the residual of every iteration by ds_union_residual - K X' and
                                 M X' of the new Ritz block are then never written; ds_union_residual_workspace_bytes bytes */
    int64_t res_work_bytes;
    void* gram_work;
    int64_t gram_work_bytes;
    double* lam;              /* host, b: in / out */
    double* rerr;             /* host, b: out */
    double* history;          /* host, history_cap entries or NULL: max backward error of the wanted pairs per iteration */
    int32_t history_cap;
    int32_t iterations;       /* out */
    int32_t result_in_s2;     /* out */
    int32_t wait_mode;        /* ABI 31: how THIS solve's host thread waits for its stream - 0: hipStreamSynchronize, 1: a 20 us poll,
                                 then a sleep on a blocking event, -1: the process default (ds_host_wait_mode).  Per solve, so that
                                 the hypothesis lanes of one pipeline, another pipeline of the process and a single solve beside
                                 them each keep their own setting */
    double ritz_tol;          /* ABI 32: > 0: a pair counts as converged (and is locked) only when, besides rel < tol, its Ritz value
                                 moved by less than ritz_tol (relative) in the last step.  The backward error rel is relative to
                                 ||K|| + lambda ||M||: a SMOOTH vector passes a loose tol (the corner-level phase of a nested start:
                                 3e-3) whatever its Rayleigh quotient is - a start block that went through the preconditioner was
                                 locked with Ritz values 2 x off (profiles/r06_start_sweeps.txt).  0: the reference's test alone */
    /* ABI 41, no new field: with res_work, a bf16 two-level cycle on node blocks (twolevel->storage without DS_TL_OWN_INIT),
       level_tag 0 and <= 84 active columns, the residual walk writes the cycle's bf16 inputs instead of the fp32 R
       (ds_union_residual_pre) and the cycle starts at its first term - same iterates bit for bit, one launch and one pass over
       the residual block less per iteration */
} ds_lobpcg_t;
int ds_lobpcg_iterate(ds_lobpcg_t* p, const ds_lapack_t* lapack, ds_stream_t stream);
/* ABI 31.  Self-check of the loop's host-side dense steps with the given LAPACK table - no device involved (the CPU test suite
 * calls it): on a seeded random symmetric positive definite n x n matrix, errs[0] / errs[1] = eigenvalue / residual error of the
 * lowest m pairs from the staged eigensolver (dsytrd + dstedc + dormtr on m columns) against dsyevd, errs[2] / errs[3] = the
 * Cholesky factor and its inverse, errs[4] = orthogonality of the twice-applied Cholesky-QR on n x m columns, errs[5] = 1 when the
 * staged path ran.  errs: 6 doubles. */
int ds_selftest_dense(const ds_lapack_t* lapack, int n, int m, unsigned seed, double* errs);
/* ABI 31.  The two small dense steps that frame the iteration, on the HOST with the caller's LAPACK table (no device; reference: the
 * first Rayleigh-Ritz step of _update_ortho, src/lobpcg/_lobpcg.py:443-448, and the read-out's quadratic forms, diff_model.py:371-399).
 * ds_host_start_block: G = [Y X0]^T [K X0 | M X0] ((ny + b) x 2 b doubles, row-major) of a start block X0 -> its projection against the
 *   M-orthonormal Y, its M-orthonormalisation and its first Ritz step in coefficients: lam (b), coef ((ny + b) x b: X = [Y X0] coef),
 *   cx (b x b: K X = (K X0) cx), *amp (the rounding amplification of the one-sweep orthonormalisation); *route = 1 (nothing else written)
 *   when eps x amp >= ortho_tol or the projected Gram matrix broke down: the caller orthonormalises explicitly.
 * ds_host_polish: GK = nterms (b x b) matrices X^T K_i X one after the other, coefs their weights, GM = X^T M X -> E (k lowest values of
 *   (sum c_i GK_i) z = e GM z), C (b x b, C^T GM C = I), qs ((nterms + 1) x k: c_j^T GK_i c_j, then c_j^T GM c_j). */
int ds_host_start_block(const ds_lapack_t* lapack, const double* G, int ny, int b, double ortho_tol, double eps, double* lam,
                        double* coef, double* cx, double* amp, int* route);
int ds_host_polish(const ds_lapack_t* lapack, int nterms, const double* GK, const double* coefs, const double* GM, int b, int k,
                   double* E, double* C, double* qs);
/* ABI 42.  Two dense steps of the iteration itself, on the HOST with the caller's LAPACK table (no device), exported so that they can be
 * checked against their Python twins of lobpcg/dense.py (_raw_basis_transform, _rr_step); row-major doubles.
 * ds_host_raw_basis: GG = [Y X P W]^T [K W | M W] ((w0 + na) x 2 na, w0 = ny + ncl + nxp), Gxp = [X_a P]^T K [X_a P] (nxp x nxp), lam_locked
 *   (ncl Ritz values) -> *route = 0: G ((nxp + na) x (nxp + na)) = S_a^T K S_a for S_a = [X_a P W_o], Qw ((w0 + na) x na) = W_o in the raw
 *   basis; *route = 1 (nothing else written): eps x amp >= ortho_tol or a breakdown - the caller orthonormalises explicitly.
 * ds_host_rr_step: G (sz x sz, sz >= 2 na) -> E (its na lowest eigenvalues), Z1 (sz x na, their vectors), Zp (sz x na, an orthonormal
 *   basis of (I - Z1 Z1[:na]^T) E_x). */
int ds_host_raw_basis(const ds_lapack_t* lapack, const double* GG, const double* Gxp, const double* lam_locked, int ny, int ncl, int nxp,
                      int na, double ortho_tol, double eps, double* G, double* Qw, int* route);
int ds_host_rr_step(const ds_lapack_t* lapack, const double* G, int sz, int na, double* E, double* Z1, double* Zp);
/* How the host thread of ds_lobpcg_iterate waits for its stream when its descriptor says wait_mode = -1 (ABI 30; process-wide default 0).  0: hipStreamSynchronize (the
 * runtime spins when the host has more cores than devices); 1: a 20 us poll, then a sleep on an event created with
 * hipEventBlockingSync - for callers that run several solves on several streams and threads at once (the hypothesis lanes of
 * diffsound_amd/pipeline.py): waiting lanes then leave their cores to the lanes that are computing. */
int ds_host_wait_mode(int mode);

/* Out <- alpha * A C + beta * Out,  A (n x p) f32, C (p x q) f32 row-major device, Out (n x q) f32.
 * Out may overlap A (e.g. be a column range of it) when q <= 160: every row tile is read completely before it is
 * written.  (reference: X <- S Z etc., _lobpcg.py:463-466) */
int ds_mix(const float* A, int64_t lda, int p, const float* C, int q, float* Out, int64_t ldo,
           int64_t n, float alpha, float beta, ds_stream_t stream);

/* Element-wise passes of the fp64 refinement fused (ABI 28, csrc/refine64.hip; reference: update_residual /
 * update_converged_count of src/lobpcg/_lobpcg.py:301-333 in fp64).  KX, MX, X: (n x b) fp64 blocks, b even <= 512, rows 16-byte
 * aligned; lam: b Ritz values on the device.
 *   ds_residual64_norms   rn2[j] = ||K x_j - lam_j M x_j||^2, xn2[j] = ||x_j||^2 in ONE pass over the three blocks (no residual
 *                         block is written); work: ds_residual64_workspace_doubles(b) doubles; fixed-order sums
 *   ds_residual64_scaled  R (n x nact fp32, nact a multiple of 4) = the residual columns cols[0 .. nact) (ascending or not),
 *                         each multiplied by scale[col] (e.g. 1 / its norm): the input of the fp32 preconditioner */
int64_t ds_residual64_workspace_doubles(int b);
int ds_residual64_norms(const double* KX, int64_t ldk, const double* MX, int64_t ldm, const double* X, int64_t ldx,
                        const double* lam, int64_t n, int b, double* work, int64_t work_doubles, double* rn2, double* xn2,
                        ds_stream_t stream);
int ds_residual64_scaled(const double* KX, int64_t ldk, const double* MX, int64_t ldm, const double* lam, const double* scale,
                         const int32_t* cols, int nact, float* R, int64_t ldr, int64_t n, ds_stream_t stream);

/* A basis held as a list of fp64 blocks (ds_gram64_blocks, ds_mix64). */
#define DS_MIX64_MAX_BLOCKS 4
typedef struct {
    const double* a;  /* device, n x p, row-major */
    int64_t lda;
    int32_t p;
    int32_t offset;   /* ds_mix64: first row of this block's coefficients in C; ds_gram64_blocks: the block's first row
                         (a block of A) or column (a block of B) of G */
} ds_block64_t;

/* G[oa_i + r][ob_j + c] = (A_i^T B_j)[r][c] for every pair of a block of A and a block of B (fp64 operands, fp64 MFMA,
 * fixed-order reduction over the row splits): the Gram blocks of a basis held as a LIST of arrays, [S]^T [K W | M W] of the
 * fp64 refinement in ONE pass over the rows instead of one ds_gram call per pair of blocks.  G is dense row-major,
 * P = sum p_i rows by Q = sum q_j columns: the blocks tile G in the order given (offset_k = the sum of the widths
 * before block k; checked).
 * flags: DS_GRAM_SYMMETRIC - G is symmetric (B = K A with symmetric K, same offsets on both sides): only the tiles on
 * and above the diagonal are computed, the rest mirrored.  At most DS_MIX64_MAX_BLOCKS blocks per side.
 * work: ds_gram_workspace_bytes(n, P, Q) bytes.  (reference: the Gram products of _lobpcg.py:516-525 on the concatenated
 * basis) */
int ds_gram64_blocks(int na, const ds_block64_t* A, int nb, const ds_block64_t* B, int64_t n, int flags, double* G,
                     void* work, int64_t work_bytes, ds_stream_t stream);

/* Out <- alpha * sum_b A_b C[offset_b : offset_b + p_b, :q] + beta * Out, all fp64: the dense n x b updates of the fp64
 * refinement over a basis given as a LIST of blocks (the rigid modes, X, P, W: separate arrays of different widths) and
 * one stacked coefficient matrix C (row-major device, leading dimension ldc) - every block is read once, the result
 * written once.  Out must not overlap any block.  (reference: X <- S Z, src/lobpcg/_lobpcg.py:457-477, there as
 * torch.matmul on the concatenated basis) */
int ds_mix64(int nblocks, const ds_block64_t* blocks, const double* C, int64_t ldc, int q, double* Out,
             int64_t ldo, int64_t n, double alpha, double beta, ds_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Geometry backward of the modal read-out (reference: autograd through get_vals -> K, M -> vertices,
 * src/diffelastic/diff_model.py:390-399 with deform.py:35-68,136-147, mesh.py:58-99):
 *   grad += d/dx sum_i gk[i] u_i^T K(x) u_i - gm[i] u_i^T M(x) u_i      (gm[i] = gk[i] * lambda_i)
 * tetgeo: the (T x 13) geometry workspace filled by ds_assemble_kml for the SAME coordinates;
 * U: (3nv x m) f32 modes; gtab (ng x N x 4) f64 = dN_a/dL_k at ng <= 4 quadrature points, gw (ng) weights
 * (a rule exact for degree 2(order-1)); mtab as in ds_assemble_kml; grad: (nv x 3) f64, ACCUMULATED with fp64
 * atomics (the caller zeroes it). */
int ds_geometry_grad(const int32_t* tets, int64_t T, int N, int64_t nv, const double* tetgeo, const float* U,
                     int64_t ldu, int m, const double* gk, const double* gm, double lam, double mu,
                     const double* gtab, const double* gw, int ng, const double* mtab, double* grad,
                     ds_stream_t stream);
/* The same gradient for a general constant tangent (ABI 40; the stiffness of ds_combine_tangent, reference
 * src/diffelastic/diff_model.py:184-220, :371-399):
 *   grad = d/dx sum_i gk[i] u_i^T K(C, x) u_i - gm[i] u_i^T M(x) u_i ,   element energy J sum_g w_g vec(F)^T C vec(F),
 * differentiated with dW/dvec(F) = (C + C^T) vec(F).  C: 81 doubles on the HOST, row 3i+j, column 3k+l, finite (passed to
 * the kernel by value).  cinc_ptr (nv + 1), cinc (4 T) int32: per node its (element * 4 + corner) incidences in CSR form,
 * ascending - the order of a node's sum; elem_work: T * 12 doubles of scratch.  grad (nv x 3) f64 is WRITTEN, not
 * accumulated: no atomics, two calls give the same bits, nodes without a corner incidence (mid-edge nodes) get 0.
 * 4 T < 2^31; the fp64 buffers 8-byte aligned, U 4-byte aligned.  The incidence list is the caller's statement about tets and
 * is not validated: out-of-range entries are skipped, a list of another topology gives wrong sums without an error. */
int ds_geometry_grad_tangent(const int32_t* tets, int64_t T, int N, int64_t nv, const double* tetgeo, const float* U,
                             int64_t ldu, int m, const double* gk, const double* gm, const double* C, const double* gtab,
                             const double* gw, int ng, const double* mtab, const int32_t* cinc_ptr, const int32_t* cinc,
                             double* elem_work, double* grad, ds_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Damped-oscillator bank (reference src/ddsp/oscillator.py:113-141, 282-310):
 *   s[a,t] = sum_m amp[a,m] exp(-d_m tau_t) sin(w_m tau_t),  tau_t = (t+1)/sr
 *   y[a,t] = sum_{j<F} force[a,j] s[a,t-j]                   (causal FIR, cropped to S samples)
 * d, w: (m) f64 (decay rate and damped angular frequency) ; amp: (A x m) f32 or NULL (= 1) ;
 * force: (A x F) f32 ; y: (A x S) f32.
 * Backward: gy (A x S) f32 -> gd, gw (m) f64, gamp (A x m) f32 (may be NULL) ; gs is scratch (A x S) f32.
 * 1 <= F <= 512 and A <= 65535 (A is a grid dimension); anything else is refused with DS_ERR_ARG.
 * ---------------------------------------------------------------------------------------------- */
int ds_osc_bank_fwd(const double* d, const double* w, const float* amp, const float* force,
                    int A, int m, int F, int S, double sr, float* y, ds_stream_t stream);
int ds_osc_bank_bwd(const float* gy, const double* d, const double* w, const float* amp,
                    const float* force, int A, int m, int F, int S, double sr, float* gs,
                    double* gd, double* gw, float* gamp, ds_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Read-out + render + loss + backward of a pass in one call: steps 3-6 of the reference's training-loop body, the part it
 * runs EVERY epoch (the eigendecomposition only every EIGEN_DECOMPOSE_CYCLE-th: experiments/material_sync_train.py:135-167):
 *   pred_i = ev_i + (lam a_i + mu b_i) - ev_i m_i        get_undamped_freqs, src/diffelastic/diff_model.py:371-388
 *   f_i = float(sqrt(pred_i) / 2 / pi);  w0sq = (2 pi f)^2, d = (alpha + beta w0sq) / 2, w = sqrt(w0sq - d^2)
 *   audio = oscillator bank of (d, w), unit amplitudes, A = 1          TraditionalDampedOscillator, src/ddsp/oscillator.py:282-310
 *   loss = mean((audio - target)^2)   (target NULL: mean(audio^2))
 *   backward != 0: dloss/dE, dloss/dnu through the bank, the damping model and lam(E, nu), mu(E, nu), whose partial
 *   derivatives the caller passes (dlam_dE, dlam_dnu, dmu_dE, dmu_dnu).
 * ev, a_lam, b_mu, m_diag: (m) f64 - eigenvalues and the quadratic forms u^T K_lambda u, u^T K_mu u, u^T M u of the kept
 * eigenvectors; force (F) f32; target (S) f32 or NULL; audio (S) f32 out; freqs (m) f32 out; work: 6 m doubles, fwork: 2 S
 * floats (scratch); out: 3 doubles on the device (loss, dloss/dE, dloss/dnu; the last two only with backward).
 * ---------------------------------------------------------------------------------------------- */
int ds_readout_pass(const double* ev, const double* a_lam, const double* b_mu, const double* m_diag, int m,
                    double lam, double mu, double dlam_dE, double dlam_dnu, double dmu_dE, double dmu_dnu,
                    double alpha, double beta, const float* force, int F, int S, double sr, const float* target,
                    int backward, float* audio, float* freqs, double* work, float* fwork, double* out,
                    ds_stream_t stream);

/* Time-varying bank (reference GTDampedOscillator.forward with non_linear_rate != 0, oscillator.py:217-243):
 *   s[a,t] = sum_m amp[a,m] exp(-D[a,m,t]) sin(2 pi P[a,m,t]),  D = cumsum_t(dmp / sr),  P = cumsum_t(frq / sr)
 *   y = causal FIR of s with force, as above.
 * dmp, frq: (A x m x S) f32 per-sample damping rate [1/s] and damped frequency [Hz]; running sums in fp64.
 * work: scratch of ds_osc_tv_workspace_floats(A, m, S) floats.  Backward: g_dmp, g_frq (A x m x S) f32, gamp (A x m)
 * f32 or NULL; gs scratch (A x S) f32.  Deterministic. */
int64_t ds_osc_tv_workspace_floats(int A, int m, int S);
int ds_osc_tv_fwd(const float* dmp, const float* frq, const float* amp, const float* force, int A, int m, int F,
                  int S, double sr, float* work, float* y, ds_stream_t stream);
int ds_osc_tv_bwd(const float* gy, const float* dmp, const float* frq, const float* amp, const float* force, int A,
                  int m, int F, int S, double sr, float* gs, float* g_dmp, float* g_frq, float* gamp,
                  ds_stream_t stream);

/* Driven bank (ABI 43): the closed-form bank above under a force of ANY length F >= 1 (F > S included), with a force
 * gradient.  Replaces the grouped conv1d(signal, forces) of src/ddsp/oscillator.py:113-141, 282-310 where the force is a
 * recorded one (utils.load_audio returns the Force channel of every clip) or is itself being fitted: conv1d's autograd
 * reaches the force tensor.  Per mode the recursive resonator
 *   x[t] = z (x[t-1] + force[t]),  z = exp((-d + i w) / sr),  x[-1] = 0,  force[t] = 0 for t >= F ;  y[a,t] = sum_m amp[a,m] Im x_m[a,t]
 * which is  y[a,t] = sum_{j < F, j <= t} force[a,j] sum_m amp[a,m] Im z_m^(t-j+1), the y of ds_osc_bank_fwd.  Backward with
 * l[t] = z (l[t+1] + gy[t]), l[S] = 0:  gforce[a,j] = sum_m amp Im l_m[a,j] for j < min(F, S) and exactly 0 for j >= S ;
 * gamp[a,m] = sum_t gy Im x ;  G_m = sum_a amp sum_t x l / z (complex product),  gd = -Im G / sr,  gw = Re G / sr.
 * d, w, amp (NULL = 1), force, y, gy, gd, gw, gamp (may be NULL): dtypes and meaning of ds_osc_bank_fwd / _bwd ; gforce
 * (A x F) f32 or NULL.  A <= 65535.  work: ds_osc_driven_workspace_bytes(A, m, S) bytes, 16-byte aligned, scratch: the
 * state entering every tile of 1024 samples per (clip, mode) - A m ceil(S / 1024) complex doubles, written by both calls -
 * and A m complex doubles that only the backward writes; each call fills it itself, nothing is kept between calls.
 * gd, gw 8-byte aligned.  fp64 states, every power z^n from exp / sincos of n d / sr, n w / sr; one fp32 rounding per
 * sample of y, gforce, gamp.  No atomics: the same inputs give the same bits in every output and in the workspace.
 * Asynchronous on the stream, no allocation, no synchronisation.  Refused (DS_ERR_ARG, message in ds_last_error()): a
 * null required pointer, A, m, S or F <= 0, sr <= 0, A > 65535, work_bytes below the query, a misaligned pointer. */
int64_t ds_osc_driven_workspace_bytes(int A, int m, int S);
int ds_osc_driven_fwd(const double* d, const double* w, const float* amp, const float* force, int A, int m, int F, int S,
                      double sr, void* work, int64_t work_bytes, float* y, ds_stream_t stream);
int ds_osc_driven_bwd(const float* gy, const double* d, const double* w, const float* amp, const float* force, int A, int m,
                      int F, int S, double sr, void* work, int64_t work_bytes, double* gd, double* gw, float* gamp /*or NULL*/,
                      float* gforce /*or NULL, A x F*/, ds_stream_t stream);

/* Sliding contact (still ABI 45, three added symbols): the driven bank above with an input gain per mode AND per sample - a
 * scrape, a roll or a bow stroke, whose contact point moves while the force acts, so that the gain c_i(p(t)) of mode i
 * multiplies the force BEFORE the resonator.  The reference has no counterpart (its amp, src/ddsp/oscillator.py:76, is one
 * free number per clip and mode).
 *   x_m[t] = z_m (x_m[t-1] + g_m[a,t] force[a,t]),  x[-1] = 0,  force[t] = 0 for t >= F ;  y[a,t] = sum_m amp[a,m] Im x_m[t]
 *   g_m[a,t] = (1 - th) gain[a,m,k] + th gain[a,m,min(k+1, K-1)],  k = min(t / hop, K-1),  th = (t - k hop) / hop, and th = 0
 *   where t / hop >= K-1: piecewise linear between K control frames hop samples apart, the last frame held; th and the
 *   interpolation in fp64 from the fp32 gains.  K = 1 is a constant input gain; unit gains give ds_osc_driven_fwd's y.
 * Backward with l[t] = z (l[t+1] + gy[t]), l[S] = 0 and gin_m[j] = amp_m Im l_m[j]:
 *   gforce[a,j] = sum_m g_m[a,j] gin_m[j] for j < min(F, S), exactly 0 for S <= j < F ;
 *   ggain[a,m,k] = sum_j hat_k(j) force[a,j] gin_m[j], hat_k the two interpolation weights (the clamped ones land on K-1),
 *   exactly 0 for a frame that no driven sample touches ;  gamp[a,m] = sum_t gy Im x ;
 *   G_m = sum_a amp sum_t (x[t-1] + g force[t]) l[t] (complex product),  gd = -Im G / sr,  gw = Re G / sr.
 * gain, ggain: (A x m x K) f32, the frames contiguous.  hop: a positive multiple of DS_OSC_SCAN_RUN (a lane's run of samples
 * then lies inside one frame interval).  Everything else as ds_osc_driven_fwd / _bwd: dtypes, NULL amp / gamp / gforce (and
 * ggain), A <= 65535, work of ds_osc_slide_workspace_bytes(A, m, S, K, hop) bytes (0 for arguments that would be refused),
 * 16-byte aligned, fp64 states, closed-form powers, one fp32 rounding per stored element, no atomics, the same bits from the
 * same inputs, asynchronous, no allocation.  Refused (DS_ERR_ARG, message in ds_last_error()): a null required pointer;
 * A, m, F, S or K <= 0; A > 65535; hop <= 0 or no multiple of DS_OSC_SCAN_RUN; sr <= 0; work_bytes below the query; a
 * misaligned workspace or operand. */
#define DS_OSC_SCAN_RUN 16 /* samples per wavefront lane of the recursive-resonator kernels: the unit of hop */
int64_t ds_osc_slide_workspace_bytes(int A, int m, int S, int K, int hop);
int ds_osc_slide_fwd(const double* d, const double* w, const float* amp, const float* force, const float* gain, int A, int m,
                     int F, int S, int K, int hop, double sr, void* work, int64_t work_bytes, float* y, ds_stream_t stream);
int ds_osc_slide_bwd(const float* gy, const double* d, const double* w, const float* amp, const float* force, const float* gain,
                     int A, int m, int F, int S, int K, int hop, double sr, void* work, int64_t work_bytes, double* gd, double* gw,
                     float* gamp /*or NULL*/, float* gforce /*or NULL, A x F*/, float* ggain /*or NULL, A x m x K*/,
                     ds_stream_t stream);

/* Listener bank (still ABI 45, three added symbols): the driven bank above read out through a COMPLEX gain per (channel,
 * mode, frame) - the listener's half of the chain: a mode that rings as Im x is heard at a point as Im(H x), H the conjugate
 * of the mode's transfer to that point; channels (two ears) differ in the phase of H, and a listener that moves hears H
 * rotate (the Doppler shift).  One scan of the modes serves every channel.  The reference has no counterpart.
 *   x_m[a,t] = z_m (x_m[a,t-1] + force[a,t]),  z_m = exp((-d_m + i w_m) / sr),  x[-1] = 0,  force[t] = 0 for t >= F ;
 *   H[a,c,m](t) = (1 - th) h[a,c,m,k] + th h[a,c,m,min(k+1, K-1)],  k, th as in ds_osc_slide_fwd (last frame held; th and the
 *   interpolation in fp64 from the fp32 h) ;
 *   y[a,c,t] = sum_m amp[a,m] Im(H[a,c,m](t) x_m[a,t]) = sum_m amp (Hr Im x + Hi Re x).
 * K = 1 is a listener at rest; C = 1, K = 1, h = 1 + 0i gives ds_osc_driven_fwd's y.  Backward, with the complex drive
 * wdrive_m[a,t] = sum_c gy[a,c,t] H[a,c,m](t) and l[t] = z (l[t+1] + wdrive[t]), l[S] = 0 (no conjugate anywhere):
 *   gforce[a,j] = sum_m amp Im l_m[a,j] for j < min(F, S), exactly 0 for S <= j < F ;
 *   gamp[a,m] = sum_c sum_t gy[a,c,t] Im(H x_m[a,t]) ;
 *   gh[a,c,m,k] = amp sum_t hat_k(t) gy[a,c,t] (Im x_m[a,t], Re x_m[a,t]), hat_k the two interpolation weights (the clamped
 *   ones land on K-1), exactly (0, 0) for a frame that no sample t < S touches ;
 *   G_m = sum_a amp sum_t (x_m[t-1] + force[t]) l_m[t] (complex product),  gd = -Im G / sr,  gw = Re G / sr.
 * h, gh: (A x C x m x K x 2) f32, the frames contiguous, (re, im) innermost, 8-byte aligned.  y, gy: (A x C x S) f32.
 * 1 <= C <= DS_OSC_LISTEN_MAX_CHANNELS.  hop: a positive multiple of DS_OSC_SCAN_RUN.  amp NULL = 1; gamp is NULL exactly when
 * amp is; gforce and gh may each be NULL: what is NULL is not computed and does not change the bits of the rest.  Everything
 * else as ds_osc_driven_fwd / _bwd: dtypes, A <= 65535, work of ds_osc_listen_workspace_bytes(A, C, m, S, K, hop) bytes (0 for
 * arguments that would be refused), 16-byte aligned, fp64 states, closed-form powers, one fp32 rounding per stored element,
 * no atomics, the same bits from the same inputs, asynchronous, no allocation.  Refused (DS_ERR_ARG, message in
 * ds_last_error()), in this order: a null required pointer; A, C, m, F, S or K <= 0; A > 65535; C above
 * DS_OSC_LISTEN_MAX_CHANNELS; hop <= 0 or no multiple of DS_OSC_SCAN_RUN; sr <= 0; work_bytes below the query; a misaligned
 * workspace; (backward) gamp without amp or amp without gamp; gd or gw misaligned; a misaligned operand. */
#define DS_OSC_LISTEN_MAX_CHANNELS 16 /* C: the frame carries of channel c live in lane c; a workgroup carries up to 4 */
int64_t ds_osc_listen_workspace_bytes(int A, int C, int m, int S, int K, int hop);
int ds_osc_listen_fwd(const double* d, const double* w, const float* amp, const float* force, const float* h, int A, int C,
                      int m, int F, int S, int K, int hop, double sr, void* work, int64_t work_bytes, float* y,
                      ds_stream_t stream);
int ds_osc_listen_bwd(const float* gy, const double* d, const double* w, const float* amp, const float* force, const float* h,
                      int A, int C, int m, int F, int S, int K, int hop, double sr, void* work, int64_t work_bytes, double* gd,
                      double* gw, float* gamp /*NULL with amp*/, float* gforce /*or NULL, A x F*/,
                      float* gh /*or NULL, A x C x m x K x 2*/, ds_stream_t stream);

/* Propagation delay (still ABI 45, three added symbols): a time-varying fractional delay line - what a receiver on a path
 * hears of a source at rest is s(t - r(t) / c): the onset time, the delayed envelope and the Doppler shift at once.  The
 * listener bank above puts r into the phase of each mode only; this family delays the rendered rows themselves.  The
 * reference has no counterpart.  Per row b (B rows: clip x channel), all index arithmetic in fp64:
 *   tau(t) = tau[b,k] + th (tau[b,min(k+1, K-1)] - tau[b,k]),  k, th as in ds_osc_slide_fwd (k = min(t / hop, K-1),
 *   th = (t - k hop) / hop, th = 0 where t / hop >= K-1: piecewise linear between K frames hop samples apart, the last frame
 *   held; this is (1 - th) tau_k + th tau_k+1 in the form that returns equal frames exactly) ;
 *   p(t) = t - tau(t),  n = floor(p),  f = p - n ;
 *   h(u) = sinc(u) cos^2(pi u / (2 R)) for |u| < R, 0 outside,  R = DS_DELAY_HALF_TAPS,  sinc(u) = sin(pi u) / (pi u) ;
 *   y[b,t] = sum_{i = -R+1 .. R} h(f - i) s[b, n + i],  s = 0 outside [0, S).
 * h is not normalised: h(-i) = delta_i, so an integer delay (f = 0) copies s[b,n], bit for bit, and gives exactly 0 where n
 * lies outside [0, S).  h is C1 everywhere (value and slope vanish at +-R): the derivative to the delay is continuous
 * where p crosses an integer.  Backward, no conjugate and no approximation:
 *   gs[b,j] = sum_t gy[b,t] h(p(t) - j) ;
 *   gtau[b,k] = - sum_t hat_k(t) gy[b,t] sum_j s[b,j] h'(p(t) - j), hat_k the two interpolation weights (the clamped ones
 *   land on K-1), exactly 0 for a frame that no sample t < S touches.
 * PRECONDITION (the caller's: tau lives on the device and cannot be checked here): two consecutive frames of a row differ
 * by at most hop DS_DELAY_MAX_SLOPE - a receiver below Mach 0.5.  Then p rises by 0.5 .. 1.5 per sample, the samples that
 * reach an input j are one run of at most 4 R + 1, and gs is a gather: no atomics, the same bits from the same inputs.
 * SAFE FOR EVERY tau: no address is formed from an unchecked p - the range test is made in fp64 before any conversion to
 * an integer.  A position outside [-R, S + R) yields y = 0; a non-finite tau(t) yields y = NaN and contributes nothing to gs
 * and gtau, without a memory access; where the slope precondition is violated gs is unspecified (y and gtau are still what
 * the formulas say) but every search and every index stays inside [0, S).
 * s, y, gy, gs: (B x S) f32, 4-byte aligned.  tau, gtau: (B x K) f64, in samples, 8-byte aligned.  hop: any positive number of
 * samples.  1 <= B <= DS_DELAY_MAX_ROWS.  fp32 signal, fp64 weights and accumulation, one fp32 rounding per stored element of
 * y and gs.  The forward needs no workspace; the backward takes ds_delay_workspace_bytes(B, S, K, hop) bytes (0 for arguments
 * that would be refused), 16-byte aligned.  gs and gtau may each be NULL: what is NULL is not computed and does not change
 * the bits of the rest.  Asynchronous on the stream, no allocation.  Refused (DS_ERR_ARG, message in ds_last_error()), in
 * this order: a null required pointer; B, S or K <= 0; B above DS_DELAY_MAX_ROWS; hop <= 0; (backward) work_bytes below the
 * query; a misaligned workspace; a misaligned operand. */
#define DS_DELAY_HALF_TAPS 8    /* R: 2 R = 16 taps per output */
#define DS_DELAY_MAX_SLOPE 0.5  /* |tau[b,k+1] - tau[b,k]| <= hop DS_DELAY_MAX_SLOPE */
#define DS_DELAY_MAX_ROWS 65535 /* B: the rows are the launch grid's second axis */
int64_t ds_delay_workspace_bytes(int B, int S, int K, int hop);
int ds_delay_fwd(const float* s, const double* tau, int B, int S, int K, int hop, float* y, ds_stream_t stream);
int ds_delay_bwd(const float* gy, const float* s, const double* tau, int B, int S, int K, int hop, void* work,
                 int64_t work_bytes, float* gs /*or NULL*/, double* gtau /*or NULL*/, ds_stream_t stream);

/* Recording chain (still ABI 45, three added symbols): a cascade of S second-order sections (biquads) over B rows of N
 * samples - the receiver's half of a recorded clip (a microphone, a room, a parametric EQ) and the high-pass that prepares
 * one.  Per section, zero initial state, a row of sos = (b0 b1 b2 a1 a2) with a0 = 1:
 *   w[n] = u[n] - a1 w[n-1] - a2 w[n-2] ;   v[n] = b0 w[n] + b1 w[n-1] + b2 w[n-2] ;   section s + 1 reads the v of section s ;
 *   u of section 0 is x, y is the v of section S - 1.
 * Backward, the sections in reverse order, g the gradient at a section's output (gy for the last):
 *   lam[n] = sum_k b_k g[n+k] - a1 lam[n+1] - a2 lam[n+2] (g, lam = 0 from N on): the gradient at the section's input, gx for
 *   section 0 ;   gb_k = sum_n g[n] w[n-k] ;   ga_k = - sum_n lam[n] w[n-k] ;   gsos row = (gb0 gb1 gb2 ga1 ga2).
 * x, y, gy, gx: (B x N) f32, 4-byte aligned.  sos: (S x 5) f64 shared by the rows when per_clip = 0, (B x S x 5) when
 * per_clip = 1; gsos: ALWAYS (B x S x 5) f64 (the caller adds the rows up for shared coefficients); 8-byte aligned.
 * 1 <= B <= DS_BIQUAD_MAX_ROWS, 1 <= S <= DS_BIQUAD_MAX_SECTIONS.  All arithmetic in fp64; only y and gx are rounded to fp32,
 * once.  One wavefront a row walks it in tiles of 64 DS_OSC_SCAN_RUN samples, all sections on a tile before the next is
 * loaded, the lanes joined by a shuffle scan with powers of the companion matrix [[-a1, -a2], [1, 0]] formed by repeated
 * squaring (no case split on the kind of poles).  The forward needs no workspace.  The backward runs the forward again and
 * keeps every section's w: ds_biquad_workspace_bytes(B, N, S) = 8 B S N bytes (0 for arguments that would be refused),
 * 16-byte aligned.  The coefficient sums are added lane by lane over the tiles and joined by one butterfly: no atomics, the
 * same bits from the same inputs.  No workgroup waits for another.  Asynchronous on the stream, no allocation.
 * SAFE FOR EVERY sos: no index and no trip count depends on the data.  Unstable or non-finite coefficients yield inf or
 * NaN in the outputs and nothing else (stability - |a2| < 1 and |a1| < 1 + a2 - is the caller's to check).
 * Refused (DS_ERR_ARG, message in ds_last_error()), before any device work, in this order: a null pointer (every pointer is
 * required); B, N or S <= 0; B above DS_BIQUAD_MAX_ROWS; S above DS_BIQUAD_MAX_SECTIONS; per_clip neither 0 nor 1; a misaligned
 * operand; (backward) a misaligned workspace; work_bytes below the query. */
#define DS_BIQUAD_MAX_SECTIONS 16 /* S: powers, carried states and coefficient sums of every section live in LDS */
#define DS_BIQUAD_MAX_ROWS 65535  /* B */
int64_t ds_biquad_workspace_bytes(int B, int N, int S);
int ds_biquad_fwd(const float* x, const double* sos, int per_clip, int B, int N, int S, float* y, ds_stream_t stream);
int ds_biquad_bwd(const float* gy, const float* x, const double* sos, int per_clip, int B, int N, int S, void* work,
                  int64_t work_bytes, float* gx, double* gsos, ds_stream_t stream);

/* Room response (still ABI 45, three added symbols): a long causal FIR over B rows of N samples - the room of the
 * receiver's half of a recorded clip (a microphone, a room, a parametric EQ): early reflections and a decaying tail of
 * thousands of taps, with gradients to the signal and to every tap.  H responses of L taps; B is a multiple of H and row b
 * uses response b mod H (H = 1: one room for all rows; H = C: one per channel, the channel varying fastest; H = B: one per
 * row).  Zero initial state, the output cut at N; no sum is approximated and no index is conjugated:
 *   y[b,t]  = sum_{j=0..min(t, L-1)}      h[b mod H, j] x[b, t-j] ;
 *   gx[b,s] = sum_{j=0..min(L-1, N-1-s)}  h[b mod H, j] gy[b, s+j] ;
 *   gh[r,j] = sum_{b = r, r+H, ...} sum_{t=j..N-1} gy[b,t] x[b, t-j], exactly 0 for j >= N (an empty sum).
 * x, y, gy, gx: (B x N) f32, 4-byte aligned.  h, gh: (H x L) f64, 8-byte aligned.  1 <= H <= B <= DS_FIR_MAX_ROWS,
 * 1 <= L <= DS_FIR_MAX_TAPS (2 s at 32 kHz; L may exceed N).  Direct form, N L - L^2 / 2 multiply-adds a row, and no FFT: products
 * and sums are in fp64, y and gx are rounded to fp32 once, on the store, gh stays fp64.  BIT FOR BIT: a response that is a
 * unit tap at lag k copies x shifted by k bit for bit, with exact zeros in front, as long as the inputs are finite, and the
 * same holds for gx from gy (a sum of exact zeros and one exact product; a negative zero is the number zero and comes out
 * as +0).  The three sums are one loop: a lane owns 8 consecutive outputs (y, gx) or lags (gh), keeps a sliding window of
 * the other operand in registers and reads one broadcast value and one new window value a step from LDS, where both
 * operands are staged in fp64; a workgroup owns 512 outputs or lags, the heaviest tiles of the causal triangle are launched
 * first.  The forward needs no workspace.  gh sums N - j samples and B / H rows: the samples are split into chunks of 2048 (a
 * constant, never a function of the device), the chunks' partial sums go to the workspace and a second launch adds them,
 * chunks ascending and then rows ascending: ds_fir_workspace_bytes(B, H, N, L) = 8 B ceil(N / 2048) min(L, N) bytes (0 for
 * arguments that would be refused), 16-byte aligned, needed only where gh is asked for.  No read-modify-write in memory, no
 * workgroup waits for another: the same inputs give the same bits on any device.  gx and gh may each be NULL: what is NULL
 * is not computed and does not change the bits of the other.  Asynchronous on the stream, no allocation.
 * SAFE FOR EVERY x, gy AND h: no index and no trip count depends on the data.  Non-finite inputs yield inf or NaN in the
 * outputs and nothing else (in the rows and responses they belong to).
 * Refused (DS_ERR_ARG, message in ds_last_error()), before any device work, in this order: a null required pointer (x, h, y;
 * gy, x, h, and work where gh is given); B, H, N or L <= 0; B above DS_FIR_MAX_ROWS; L above DS_FIR_MAX_TAPS; H > B or B not a
 * multiple of H; a misaligned operand; (backward) gx and gh both NULL; a misaligned workspace; work_bytes below the query. */
#define DS_FIR_MAX_TAPS 65536 /* L */
#define DS_FIR_MAX_ROWS 65535 /* B: the rows are the launch grid's first axis */
int64_t ds_fir_workspace_bytes(int B, int H, int N, int L);
int ds_fir_fwd(const float* x, const double* h, int B, int H, int N, int L, float* y, ds_stream_t stream);
int ds_fir_bwd(const float* gy, const float* x, const double* h, int B, int H, int N, int L, void* work, int64_t work_bytes,
               float* gx /*or NULL*/, double* gh /*or NULL*/, ds_stream_t stream);

/* Late reverberation (still ABI 45, three added symbols): a feedback delay network (FDN) over B rows of N samples - the
 * late field of a room in a few dozen coefficients where ds_fir_* spends one per tap, at a cost per sample that does not
 * depend on the tail's length.  n delay lines, H coefficient sets; B is a multiple of H and row b uses set b mod H, as in
 * ds_fir_*.  Everything starts from rest, s[t < 0] = 0:
 *   q_j[t] = (1 - p_j) s_j[t - m_j] + p_j s_j[t - m_j - 1]      line j's output: its delay and a two-tap absorption low-pass ;
 *   s_i[t] = b_i x[t] + sum_j A_ij q_j[t]                       what enters line i ;
 *   y[t]   = d x[t]   + sum_j c_j q_j[t].
 * Backward, r the gradient at q and l the gradient at s, both 0 from N on:
 *   l_i[t] = (1 - p_i) r_i[t + m_i] + p_i r_i[t + m_i + 1] ;   r_j[t] = c_j gy[t] + sum_i A_ij l_i[t] ;
 *   gx[t] = d gy[t] + sum_i b_i l_i[t] ;   gb_i = sum_t l_i[t] x[t] ;   gA_ij = sum_t l_i[t] q_j[t] ;   gc_j = sum_t gy[t] q_j[t] ;
 *   gd = sum_t gy[t] x[t] ;   gp_j = sum_t r_j[t] (s_j[t-m_j-1] - s_j[t-m_j]) ;   the parameter sums also run over the rows b = r, r + H, ...
 *   of a set.
 * x, y, gy, gx: (B x N) f32, 4-byte aligned.  delays: (H x n) int32, DEVICE memory, every one at least DS_FDN_MIN_DELAY (a delay
 * may exceed N: a line that never returns).  A, gA: (H x n x n) f64, row i what enters line i; b, c, p, gb, gc, gp: (H x n) f64;
 * d, gd: (H) f64; p NULL = 0 (the same bits as an array of zeros), else 0 <= p_j <= 0.5 for a low-pass; 8-byte aligned.  state:
 * (B x n x N) f64, s, written by the forward and read by the backward.  1 <= H <= B <= DS_FDN_MAX_ROWS, 1 <= n <= DS_FDN_MAX_LINES.
 * All arithmetic in fp64; y and gx are rounded to fp32 once, on the store.  Sums over j start from the x (gy) term and add j
 * ascending.  BIT FOR BIT, for finite inputs: c = 0, d = 1 returns x (a negative zero is the number zero and comes out as +0);
 * A = 0, b_j = c_j = 1, d = 0, p = 0 returns the sum over j of x shifted by m_j, with exact zeros in front.
 * One workgroup a row walks the row in blocks of T = min(min_j m_j, 256) samples, one lane a sample, the n x n product in
 * registers against the set's coefficients in LDS: every delay reaches back at least T, so a block reads only state that
 * earlier blocks wrote, and the workgroup barrier between two blocks is the whole hand-off.  The backward is the same loop
 * in reverse time with A transposed; its history r takes the first 8 B n N bytes of the workspace.  The parameter sums are
 * split into chunks of 1024 samples (a constant, never a function of the device), the chunks' partial sums go to the
 * workspace and a second launch adds them, chunks ascending and then rows ascending:
 * ds_fdn_workspace_bytes(B, H, N, n) = 8 B (n N + ceil(N / 1024) (n^2 + 3 n + 1)) bytes (0 for arguments that would be refused),
 * 16-byte aligned.  No atomics, no read-modify-write in memory, no workgroup waits for another: the same inputs give the
 * same bits on any device.  gx, gA, gb, gc, gd, gp may each be NULL: what is NULL is not computed and does not change the
 * bits of the rest.  Asynchronous on the stream, no allocation.
 * SAFE FOR EVERY x, gy AND COEFFICIENT: no index and no trip count depends on them.  Non-finite inputs and unstable A yield
 * inf or NaN in the outputs of their rows and nothing else.  THE DELAYS ARE NEVER READ ON THE HOST: a delay below
 * DS_FDN_MIN_DELAY is the caller's to refuse (diffsound_amd.ddsp.fdn does); the kernels read such a delay as DS_FDN_MIN_DELAY, so no
 * index leaves the row whatever the array holds.
 * Refused (DS_ERR_ARG, message in ds_last_error()), before any device work, in this order: a null required pointer (every
 * pointer but p and the backward's six outputs); B, H, N or n <= 0; B above DS_FDN_MAX_ROWS; n above DS_FDN_MAX_LINES; H > B or B
 * not a multiple of H; a misaligned operand; (backward) every output NULL; a misaligned workspace; work_bytes below the
 * query. */
#define DS_FDN_MAX_LINES 16   /* n: a lane holds the n line outputs of its sample in registers */
#define DS_FDN_MIN_DELAY 64   /* m_j: a block of the recursion is at least one wavefront */
#define DS_FDN_MAX_ROWS 65535 /* B */
int64_t ds_fdn_workspace_bytes(int B, int H, int N, int n);
int ds_fdn_fwd(const float* x, const int32_t* delays, const double* A, const double* b, const double* c, const double* d,
               const double* p /*or NULL*/, int B, int H, int N, int n, double* state, float* y, ds_stream_t stream);
int ds_fdn_bwd(const float* gy, const float* x, const int32_t* delays, const double* A, const double* b, const double* c,
               const double* d, const double* p /*or NULL*/, int B, int H, int N, int n, const double* state, void* work,
               int64_t work_bytes, float* gx /*or NULL*/, double* gA /*or NULL*/, double* gb /*or NULL*/, double* gc /*or NULL*/,
               double* gd /*or NULL*/, double* gp /*or NULL*/, ds_stream_t stream);

/* Contact force (still ABI 45, three added symbols): a Hertz hammer - mass[a] > 0, approach speed vel[a], contact stiffness
 * stiff[a] > 0, exponent p >= 1 (1.5 for Hertz) - coupled to the m modes (d [1/s], w [rad/s, damped]: the banks' pair) of the
 * object it strikes through the modal gains gain[a,i] at the contact point (ds_mode_sample_fwd).  The reference has no
 * counterpart.  With h = 1 / (sr R), z_i = exp((-d_i + i w_i) h), kap_i = gain[a,i]^2 / w_i, and xh = 0, vh = vel[a], s_i = 0 at
 * n = 0, for n = 0 .. F R - 1:
 *   u = sum_i kap_i Im s_i ;  delta = xh - u ;  f = stiff delta^p where delta > 0, else 0 ;  force[a, n / R] += f / R ;
 *   vh -= h f / mass ;  xh += h vh ;  s_i = z_i (s_i + h f).
 * fp64 throughout, force (A x F) stored as f32 (one rounding), as the banks take it.  vel[a] <= 0: the clip's force and all its
 * gradients are exact zeros.  Explicit: stable while h sqrt(p stiff delta_max^(p-1) (1 / mass + sum_i kap_i w_i)) << 2; a
 * non-finite result is not detected.  Rigid-body motion of the object is not in the model.
 * ds_contact_bwd is the exact adjoint of that recursion: from gforce (A x F) f32, gd, gw (m) summed over the clips in ascending
 * order, ggain (A x m), gmass, gvel, gstiff (A), all f64; gd and gw are both given or both NULL, so are gmass / gvel / gstiff,
 * ggain may be NULL: what is NULL is not computed into memory.  It runs the forward again and keeps (delta, delta^p) and s_i[n]
 * of every substep in work: ds_contact_workspace_bytes(A, m, F, R) = 16 (A F R (1 + m) + A m) bytes (0 for arguments that would
 * be refused), 16-byte aligned.  One wavefront per clip, no atomics, the same bits from the same inputs; asynchronous on the
 * stream, no allocation, no synchronisation.  Refused (DS_ERR_ARG, message in ds_last_error()): a null required pointer; A
 * outside 1..65535; m outside 1..DS_CONTACT_MAX_MODES; R outside 1..DS_CONTACT_MAX_OVERSAMPLE; F < 1; F R above
 * DS_CONTACT_MAX_SUBSTEPS; p < 1 or not finite; sr <= 0; half a gradient pair; work_bytes below the query; a misaligned
 * workspace or operand. */
#define DS_CONTACT_MAX_MODES 512       /* 8 modes per wavefront lane, in registers */
#define DS_CONTACT_MAX_OVERSAMPLE 64   /* R */
#define DS_CONTACT_MAX_SUBSTEPS 1048576 /* F R */
int64_t ds_contact_workspace_bytes(int A, int m, int F, int R);
int ds_contact_fwd(const double* d, const double* w, const double* gain, const double* mass, const double* vel,
                   const double* stiff, int A, int m, int F, int R, double p, double sr, float* force, ds_stream_t stream);
int ds_contact_bwd(const float* gforce, const double* d, const double* w, const double* gain, const double* mass,
                   const double* vel, const double* stiff, int A, int m, int F, int R, double p, double sr, void* work,
                   int64_t work_bytes, double* gd /*or NULL*/, double* gw /*or NULL*/, double* ggain /*or NULL*/,
                   double* gmass /*or NULL*/, double* gvel /*or NULL*/, double* gstiff /*or NULL*/, ds_stream_t stream);

/* Friction excitation (still ABI 45, three added symbols): a bow, a rubbing finger or a wet rim - velocity vb[a,k] and normal
 * force N[a,k] >= 0 per clip and output sample (A x F, the gesture), the friction curve's peak velocity vs[a] > 0 - coupled to the
 * m modes (d > 0 [1/s], w > 0 [rad/s, damped]: the banks' pair) of the object it rubs through the modal gains gain[a,i] at the
 * contact point (ds_mode_sample_fwd).  The force is no input: it follows from the object's own velocity under the bow.  The
 * reference has no counterpart.  With h = 1 / (sr R), z_i = exp((-d_i + i w_i) h), g_i = gain[a,i]^2, r_i = d_i / w_i, and s_i = 0
 * at n = 0, for n = 0 .. F R - 1 and k = n / R:
 *   v = sum_i g_i (Re s_i - r_i Im s_i) ;  vr = vb[a,k] - v ;  phi = (vr / vs) exp((1 - (vr / vs)^2) / 2) ;  f = N[a,k] phi ;
 *   force[a,k] += f / R ;  s_i = z_i (s_i + h f).
 * phi is odd, peaks at 1 where vr = vs and falls beyond: the steep branch around 0 is sticking, the falling one sustains the
 * oscillation.  fp64 throughout, force (A x F) stored as f32 (one rounding, after the sample's R contributions are summed in
 * ascending n), as the banks take it.  N = 0 for a whole clip: the clip's force and all its gradients but gN are exact zeros.
 * Explicit: stable while h max(N) (sqrt(e) / vs) sum_i g_i << 2, R is the remedy; a non-finite result is not detected.
 * ds_friction_bwd is the exact adjoint of that recursion: from gforce (A x F) f32, gd, gw (m) summed over the clips in ascending
 * order, ggain (A x m), gvb, gN (A x F), gvs (A), all f64.  The groups gd with gw; ggain; gvb with gN; gvs may each be NULL: what
 * is NULL is neither accumulated nor written, and the rest keeps its bits.  CHECKPOINTED: it runs the forward again and keeps
 * s_i only where a sample begins, then re-runs each sample's R substeps from its checkpoint into one segment per clip before
 * it walks them backwards - the same instructions in the same order as the forward, so the adjoint is exact for the forward
 * that ran.  work: ds_friction_workspace_bytes(A, m, F, R) = 16 (A F m + A R m + A m) bytes (checkpoints, segments, the per-clip
 * (gd, gw) partials; 0 for arguments that would be refused), 16-byte aligned.  One wavefront per clip, no atomics, the same bits
 * from the same inputs in every output and in the workspace; asynchronous on the stream, no allocation, no synchronisation.
 * Refused (DS_ERR_ARG, message in ds_last_error()), in this order: a null required pointer; A outside
 * 1..DS_FRICTION_MAX_CLIPS; m outside 1..DS_FRICTION_MAX_MODES; R outside 1..DS_FRICTION_MAX_OVERSAMPLE; F < 1; F R above
 * DS_FRICTION_MAX_SUBSTEPS; sr <= 0; half a gradient pair; work_bytes below the query; a misaligned workspace or operand. */
#define DS_FRICTION_MAX_MODES 512         /* 8 modes per wavefront lane, in registers */
#define DS_FRICTION_MAX_OVERSAMPLE 64     /* R: a lane per substep of a sample holds its vr */
#define DS_FRICTION_MAX_CLIPS 65535       /* A */
#define DS_FRICTION_MAX_SUBSTEPS 16777216 /* F R */
int64_t ds_friction_workspace_bytes(int A, int m, int F, int R);
int ds_friction_fwd(const double* d, const double* w, const double* gain, const double* vb, const double* N, const double* vs,
                    int A, int m, int F, int R, double sr, float* force, ds_stream_t stream);
int ds_friction_bwd(const float* gforce, const double* d, const double* w, const double* gain, const double* vb, const double* N,
                    const double* vs, int A, int m, int F, int R, double sr, void* work, int64_t work_bytes,
                    double* gd /*or NULL*/, double* gw /*or NULL*/, double* ggain /*or NULL*/, double* gvb /*or NULL*/,
                    double* gN /*or NULL*/, double* gvs /*or NULL*/, ds_stream_t stream);

/* Tension-modulated modal bank (still ABI 45, three added symbols): the m modes (d [1/s], w > 0 [rad/s, damped]: the banks' pair)
 * of a thin object struck hard, stiffened by the stretching of its own mid-surface - the quartic energy
 * V = 1/4 sum_r gamma_r (sum_i C_ri q_i^2)^2 of Kirchhoff-Carrier (strings) and Berger (plates) on top of the modal quadratic
 * one.  The nonlinearity sits inside the bank: the input is a force f (A x F) f64, the output the sound y (A x S) f32.  gain
 * (A x m): the mode shapes at the contact, amp (A x m): the output gains, C (K x m) >= 0: the stretch coefficients, shared by the
 * clips, gamma (A x K) >= 0: the coupling strengths.  The reference has no counterpart.  With h = 1 / (sr R),
 * z_i = exp((-d_i + i w_i) h) and s_i = 0 at n = 0, for n = 0 .. S R - 1 and k = n / R:
 *   q_i = Im s_i / w_i ;  E_r = sum_i C[r,i] q_i^2 ;  T_r = gamma[a,r] E_r ;  kap_i = sum_r C[r,i] T_r ;
 *   p_i = gain[a,i] f[a,k] - kap_i q_i  (f[a,k] = 0 for k >= F) ;  s_i = z_i (s_i + h p_i) ;
 *   if n = k R + R - 1:  y[a,k] = sr sum_i amp[a,i] Im s_i.
 * fp64 throughout, y stored as f32 (one rounding).  gamma = 0 and R = 1: y is ds_osc_driven_fwd's with the amplitudes amp gain.
 * Force samples at k >= S are not read.  A clip whose gamma is 0 throughout takes the same path: its nonlinear terms are exact
 * zeros.  Explicit: stable while h sqrt(max_i kap_i) << 2 at the largest amplitude reached, R is the remedy; a non-finite result
 * is not detected.
 * ds_nlbank_bwd is the exact adjoint of that recursion: from gy (A x S) f32, gd, gw (m) and gC (K x m) summed over the clips in
 * ascending order, ggain, gamp (A x m), gf (A x F; exact zeros at k >= S), ggamma (A x K), all f64.  The groups gd with gw; ggain;
 * gamp; gf; gC; ggamma may each be NULL: what is NULL is neither accumulated nor written, and the rest keeps its bits.
 * CHECKPOINTED like ds_friction_bwd: s_i is kept only where a sample begins, each sample's R substeps are re-run from its
 * checkpoint into one segment per clip - the same instructions in the same order as the forward - and walked backwards.
 * work: ds_nlbank_workspace_bytes(A, m, K, S, R) = 16 (A S m + A R m + A m) + 8 A K m bytes (checkpoints, segments, the per-clip
 * (gd, gw) partials, the per-clip gC partials; 0 for arguments that would be refused), 16-byte aligned.  One wavefront per clip,
 * no atomics, the same bits from the same inputs in every output and in the workspace; asynchronous on the stream, no
 * allocation, no synchronisation.
 * Refused (DS_ERR_ARG, message in ds_last_error()), in this order: a null required pointer; A outside 1..DS_NLBANK_MAX_CLIPS; m
 * outside 1..DS_NLBANK_MAX_MODES; K outside 1..DS_NLBANK_MAX_TERMS; R outside 1..DS_NLBANK_MAX_OVERSAMPLE; F < 1; S < 1; S R above
 * DS_NLBANK_MAX_SUBSTEPS; sr <= 0; half of (gd, gw); work_bytes below the query; a misaligned workspace or operand. */
#define DS_NLBANK_MAX_MODES 512         /* 8 modes per wavefront lane, in registers */
#define DS_NLBANK_MAX_TERMS 4           /* K: stretch terms, each one wave sum a substep */
#define DS_NLBANK_MAX_OVERSAMPLE 64     /* R: a lane per substep of a sample holds its E_r */
#define DS_NLBANK_MAX_CLIPS 65535       /* A */
#define DS_NLBANK_MAX_SUBSTEPS 16777216 /* S R */
int64_t ds_nlbank_workspace_bytes(int A, int m, int K, int S, int R);
int ds_nlbank_fwd(const double* d, const double* w, const double* gain, const double* amp, const double* f, const double* C,
                  const double* gamma, int A, int m, int K, int F, int S, int R, double sr, float* y, ds_stream_t stream);
int ds_nlbank_bwd(const float* gy, const double* d, const double* w, const double* gain, const double* amp, const double* f,
                  const double* C, const double* gamma, int A, int m, int K, int F, int S, int R, double sr, void* work,
                  int64_t work_bytes, double* gd /*or NULL*/, double* gw /*or NULL*/, double* ggain /*or NULL*/,
                  double* gamp /*or NULL*/, double* gf /*or NULL*/, double* gC /*or NULL*/, double* ggamma /*or NULL*/,
                  ds_stream_t stream);

/* Filtered-noise branch (ABI 44; reference src/ddsp/filtered_noise.py:20-67, FilteredNoise.forward and its autograd): per
 * frame of F samples, L logits -> magnitudes -> a Hann-windowed linear-phase FIR of T = 2 L - 1 taps, applied to a white-noise
 * frame and overlap-added at stride F.  nf = S / F + 1 frames.
 *   mag[k] = 2 sigmoid(c[k])^2.3 + 1e-6 ;  z[n] = (mag[0] + 2 sum_{k>=1} mag[k] cos(2 pi ((k n) mod T) / T)) / T ;
 *   h[j] = z[(j - (L - 1)) mod T] (0.5 - 0.5 cos(2 pi j / T)) ;  out[b, f F + s] += gain sum_t noise[b, f, t] h_{b,f}[s - t],
 *   s < T + F - 1, cut at S.
 * c (B x nf x L) f32 logits (the module's coefficient_bank), noise (B x nf x F) f32, out, gy (B x S) f32, gc (B x nf x L) f32 =
 * d / dc of sum gy out.  One launch each; gather forms, no atomics, every output element written exactly once: the same inputs
 * give the same bits.  The backward reads c, noise and gy only; a frame that starts at or after S gets gc = 0 exactly.
 * fp32 storage and fp32 convolution sums, fp64 cosine sums and transcendentals (csrc/filtered_noise.hip).  Asynchronous on the
 * stream, no allocation, no synchronisation.  Refused (DS_ERR_ARG, the message in ds_last_error() names the argument): a null
 * pointer, L outside [2, 129], F outside [1, 256], S < 1, B outside [1, 65535]. */
int ds_filtered_noise_fwd(const float* c, const float* noise, int B, int S, int L, int F, double gain, float* out,
                          ds_stream_t stream);
int ds_filtered_noise_bwd(const float* gy, const float* c, const float* noise, int B, int S, int L, int F, double gain, float* gc,
                          ds_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Multi-scale spectral loss head (reference src/ddsp/mss_loss.py:50-62, 70-122: SSSLoss types 'l1_loss' and
 * 'rmse_loss' on torchaudio.transforms.Spectrogram(n_fft, hop_length = n_fft / 4) = |torch.stft(center=True,
 * pad_mode="reflect", periodic Hann window, onesided)|^2).
 *   x: (B x S) f32 clips ; n_fft a power of two in [8, 2048], n_fft / 2 < S ; T = 1 + S / hop frames, F = n_fft/2 + 1 bins
 *   ds_stft_power      P (B x F x T) f32 power spectrogram ; re, im (B x F x T) f32 or both NULL (kept for the backward)
 *   ds_spec_loss       kind 0: sums (B x F x 2) f64 = per-row sums of |w_t dlog2| and |w_t dlin| over bins f >= 1
 *                        (loss = (alpha * sum0 + sum1) / (B (F-1) T), w_t = 2 t / (T - 1): the reference's time weights)
 *                      kind 1: sums[..][0] = per-row sums of (log2(Pp+eps) - log2(Pt+eps))^2 over bins f < fclip
 *                        (loss = sqrt(sum / (B fclip T)))
 *                      gP (B x F x T) f32 or NULL: d loss / d Pp (kind 1: to be divided by the loss value)
 *   ds_stft_power_bwd  gx (B x S) f32 = gscale * d/dx sum gP P(x), through re, im of the forward;
 *                      gframes: scratch (B x T x n_fft) f32.  Deterministic (gather form, no atomics).
 * ---------------------------------------------------------------------------------------------- */
int ds_stft_power(const float* x, int B, int S, int n_fft, int hop, float* P, float* re, float* im,
                  ds_stream_t stream);
int ds_spec_loss(int kind, const float* Pp, const float* Pt, int B, int F, int T, float alpha, float eps, int fclip,
                 double* sums, float* gP, ds_stream_t stream);
int ds_stft_power_bwd(const float* gP, const float* re, const float* im, int B, int S, int n_fft, int hop,
                      float gscale, float* gframes, float* gx, ds_stream_t stream);

/* Point clouds of the early-phase spectral loss (ABI 45; reference src/ddsp/mss_loss.py:19-48, 104-117: spec2point on the
 * 'geomloss' path).  From one power spectrogram P (B x F x T) f32, as ds_stft_power leaves it, both clouds of a scale:
 * lin (B x F x 4) and log (B x fclip x 4), 1 <= fclip <= F.  Columns 0..2: F.interpolate(row, size=3, mode='linear',
 * align_corners=False) of P (lin) or of (log2(P + eps) - log2(eps)) / 40 (log; the logarithm before the interpolation, no log
 * spectrogram is written).  Column 3: row / bins, bins = the cloud's rows (F or fclip); with freq (E entries, f32, Hz) the
 * reference's writes on top, in its order - rounds w = 2, 1, 0, cur = pos - w then cur = pos + w, pos = bins /
 * (sample_rate // 2) * freq[e], cur / bins into row trunc(cur) of every batch when 0 <= trunc(cur) < bins; a later write
 * overrides an earlier one, inside one write the highest e wins (a sequential index_put), non-finite entries write nothing.
 * The position arithmetic is the fp32 operations torch performs on device tensors, correctly rounded, uncontracted; "/ bins" is
 * the product with 1.0f / bins, torch's device form of a division by a scalar (csrc/specpoints.hip).
 *   ds_spec_points_fwd  freq, win both NULL (target clouds: column 3 = row / bins) or both given; win: F + fclip 64-bit words
 *                       (lin rows, then log rows), written here: 0 or (write + 1) << 56 | e of the row's winner.
 *   ds_spec_points_bwd  g_freq[e] = gscale * sum over both clouds of (bins / (sample_rate // 2)) / bins * sum over the writes q of
 *                       e whose row belongs to write q (of this or of another entry: autograd's rule for index_put_) of
 *                       sum_b g[b, row, 3]; g_lin (B x F x 4), g_log (B x fclip x 4), either may be NULL (zero); gscale: the
 *                       number of equal copies one entry stands for (1 for a dense list).
 *                       freq, win: those of the forward.  A gather, batches ascending, fp64 sums: the same bits on every call.
 *                       Nothing flows to P (the reference detaches it).
 * Asynchronous on the stream, no allocation, no synchronisation.  Refused (DS_ERR_ARG, message in ds_last_error()): a null
 * required pointer, B, F or T < 1, fclip outside [1, F], eps <= 0, E outside [1, 2^56), sample_rate < 2, clouds not 16-byte
 * aligned. */
int ds_spec_points_fwd(const float* P, int B, int F, int T, float eps, int fclip, const float* freq /*or NULL*/, int64_t E,
                       int sample_rate, unsigned long long* win /*or NULL*/, float* lin, float* log, ds_stream_t stream);
int ds_spec_points_bwd(const float* g_lin /*or NULL*/, const float* g_log /*or NULL*/, int B, int F, int fclip, const float* freq,
                       int64_t E, int sample_rate, const unsigned long long* win, double gscale, float* g_freq, ds_stream_t stream);

/* Launch timing hook for the benchmark's live roofline figure: while `stream` is registered (capacity > 0; 0 or a
 * NULL stream un-registers), every fused Chebyshev-term launch (ds_spmm_union epilogue 1) issued on it - from Python or
 * from the native drivers - is bracketed by HIP events.  ds_profile_collect un-registers, waits for the events and
 * returns the number of records copied: duration [ms], nv, nnzb, ncols and `first` | element bytes of the vector
 * blocks << 8 (4: fp32 term, 2: bf16 term of ds_spmm_union16) of each launch - the algorithmic bytes follow from those.
 * One stream at a time. */
int ds_profile_stream(ds_stream_t stream, int64_t capacity);
/* Which launches the hook records (bit k = kind k; 0 restores the default, the fused term only).  The kind of a record
 * comes back in bits 16.. of ds_profile_collect's `first` word; its shape in (nv, nnzb, ncols):
 *   DS_PROF_TERM   fused Chebyshev term (ds_spmm_union / 16 / 16m epilogue 1)   nv, nnzb, ncols
 *   DS_PROF_KX     Y = K X   (ds_spmm_union epilogue 0)                        nv, nnzb, ncols
 *   DS_PROF_MX     Y = M_s X (ds_spmm_union epilogue 3)                        nv, nnzb, ncols
 *   DS_PROF_RESID  the walk of ds_union_residual (without its two reductions)  nv, nnzb, ncols
 *   DS_PROF_GRAM   ds_gram (partial products + reduction)                      p, n, q ; first = symmetric | fast << 1
 *   DS_PROF_MIX    ds_mix                                                      p, n, q */
#define DS_PROF_TERM 0
#define DS_PROF_KX 1
#define DS_PROF_MX 2
#define DS_PROF_RESID 3
#define DS_PROF_GRAM 4
#define DS_PROF_MIX 5
#define DS_PROF_KM 6 /* ds_spmm_union_km: nv, nnzb, ncols */
int ds_profile_kinds(unsigned mask);
int64_t ds_profile_collect(float* ms, int64_t* nv, int64_t* nnzb, int32_t* ncols, int32_t* first, int64_t cap);

/* ------------------------------------------------------------------------------------------------
 * STREAM triad  a = b + s c  (n f32 elements, n % 4 == 0, 16-byte aligned): the measured HBM bandwidth
 * (3 n 4 bytes per call) that bench.py quotes the SpMM against.  Not part of the modal path.
 * ---------------------------------------------------------------------------------------------- */
int ds_stream_triad(float* a, const float* b, const float* c, int64_t n, float s, ds_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Helmholtz boundary elements (csrc/bem.hip): exterior Neumann problem in direct form, piecewise-constant
 * ("DP0") space, one coefficient per triangle.  Replaces the bempp-cl operators of the reference's
 * src/diffelastic/bem.py (the Python side: diffsound_amd/diffelastic/bem.py).  Complex data is interleaved
 * fp32 (re, im) pairs, torch.complex64-compatible; matrices are row-major with an explicit leading dimension
 * in complex elements.  G(x,y) = e^{ikr}/(4 pi r); the quadrature and the near-pair rule: DESIGN.md.
 *
 * Face record (DS_BEM_FACE_RECORD floats per face): [0,18) the 6 quadrature points (x, y, z), [18,24) their
 * weights times the area, [24,27) unit normal (right-hand rule on the vertex order), [27,30) centroid,
 * [30] diameter (longest edge), [31] area, [32,41) the three vertices, the rest 0.
 * A pair (i, j) is NEAR when |c_i - c_j| < DS_BEM_NEAR_RATIO * max(h_i, h_j) (every pair that shares a vertex
 * is near: a centroid lies within 2/3 h of each vertex); a point p is near face j when |p - c_j| <
 * DS_BEM_NEAR_RATIO * h_j.
 * ---------------------------------------------------------------------------------------------- */
#define DS_BEM_FACE_RECORD 48
#define DS_BEM_NEAR_RATIO 1.75f
/* Per-face geometry, once per mesh (replaces the bempp grid + DP0 space, bem.py:7-13 and :25): verts (nv x 3)
 * f32, tris (m x 3) int32 (indices checked by the caller), rec (m x DS_BEM_FACE_RECORD) f32. */
int ds_bem_geometry(const float* verts, int64_t nv, const int32_t* tris, int64_t m, float* rec, ds_stream_t stream);
/* Bytes of the workspace ds_bem_assemble needs for n faces (the per-workgroup parts of V g). */
int64_t ds_bem_assemble_workspace_bytes(int64_t n);
/* Galerkin assembly (replaces bem.py:36-43 and the V g product of :44): A = -1/2 M + K (n x n complex, lda),
 * rhs = V g (n complex) from g (n complex), both in one pass; V itself (n x n, ldv) only when V != NULL.
 * k >= 0.  work: ds_bem_assemble_workspace_bytes(n) bytes.  Bitwise reproducible (no atomics). */
int ds_bem_assemble(const float* rec, int64_t n, float k, const float* g, float* A, int64_t lda, float* V, int64_t ldv,
                    float* rhs, void* work, ds_stream_t stream);
/* y = diag(scale) A x for the complex n x n matrix A (the matvec of the GMRES that replaces bem.py:45-46); scale
 * (n real) may be NULL (= 1).  lda even, A and x 16-byte aligned.  Fixed reduction order. */
int ds_bem_cgemv(const float* A, int64_t lda, const float* x, int64_t n, const float* scale, float* y, ds_stream_t stream);
/* Potential at np points pts (np x 3 f32): out_p = -sum_j g_j int_Tj G(p,y) dy + sum_j u_j int_Tj dG/dn_y(p,y) dy
 * (replaces bem.py:50-61).  g, u: n complex face coefficients; out: np complex. */
int ds_bem_potential(const float* rec, int64_t n, float k, const float* g, const float* u, const float* pts, int64_t np,
                     float* out, ds_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Differentiable marching tetrahedra (csrc/dmtet.hip): one engine for the reference's three DMTet variants
 * (src/dmtet/geometry/dmtet_geometry.py:115-272 plain, dmtet_thickness.py:99-200 thickness band,
 * dmtet_interpolate.py:115-205 interpolated SDF, which is formed by the caller).  Occupancy is 0 < s <= hi with
 * hi = +inf (thick == NULL) or hi = *thick (DEVICE pointer, one f32: the thickness variant; a crossing edge whose
 * ends are both > 0 then has t subtracted from both values).  Outputs equal the reference's bit for bit.
 *
 * Per-grid tables (DEVICE int32, built once per grid by the caller): tets (T x 4); the distinct edges ea[e] < eb[e]
 * sorted by (a, b) (ds_edge_table); tet_edge (T x 6) = the edge id of local edges [01,02,03,12,13,23]; the vertex
 * -> incident-edge CSR vptr (n + 1) / vadj (2 E).  Indices are the caller's to check (ds_edge_table does).
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    int64_t n_used;  /* kept grid vertices (occupied and in some tet): output vertices [0, n_used) */
    int64_t n_cross; /* crossing edges: output vertices [n_used, n_used + n_cross) */
    int64_t n_side1; /* output tets of the 1-tet classes (1, 2, 4, 8) */
    int64_t n_side3; /* output tets of the 3-tet classes (3 per source tet) */
    int64_t n_inner; /* output tets of class 15 */
    int64_t n_face1; /* surface faces of the 1-triangle classes */
    int64_t n_face2; /* surface faces of the 2-triangle classes (2 per source tet) */
    int64_t reserved;
} ds_mt_counts_t;
/* Bytes of the workspace ds_mt_count needs (-1 if the sizes are out of range). */
int64_t ds_mt_count_workspace_bytes(int64_t n, int64_t T, int64_t E);
/* Replaces the occupancy / valid-tet / torch.unique(dim=0) / mask.sum() part of DMTet.__call__ (dmtet_geometry.py:
 * 122-154, dmtet_thickness.py:107-131, dmtet_interpolate.py:124-145).  sdf (n) f32.  Writes toff (T x 5 int32: each
 * tet's first row in the 1-tet, 3-tet, inner, 1-face and 2-face sections), edge_id (E: number of each crossing edge
 * among the crossing edges) and vert_id (n: number of each kept vertex), then copies ONE ds_mt_counts_t to the HOST
 * `counts` and synchronises `stream` - the only synchronisation of a forward. */
int ds_mt_count(const float* sdf, int64_t n, const int32_t* tets, int64_t T, const int32_t* ea, const int32_t* eb,
                int64_t E, const int32_t* vptr, const float* thick, int32_t* toff, int32_t* edge_id, int32_t* vert_id,
                void* work, int64_t work_bytes, ds_mt_counts_t* counts, ds_stream_t stream);
/* Replaces the interpolation, the gathers of the split tets and faces, the inner tets and the final torch.unique
 * compaction (dmtet_geometry.py:155-272, dmtet_thickness.py:133-200, dmtet_interpolate.py:146-205).  pos (n x 3) f32;
 * counts = the record ds_mt_count returned (HOST).  verts ((n_used + n_cross) x 3) f32: kept grid vertices ascending,
 * then the edge vertices p_a (-s_b)/(s_a - s_b) + p_b s_a/(s_a - s_b) in fp32 without contraction; out_tets
 * ((n_side1 + n_side3 + n_inner) x 4) int64; out_faces ((n_face1 + n_face2) x 3) int64 indices of edge vertices
 * (may be NULL); vsrc (n_used) the grid vertex of each kept vertex; xedge (n_cross) the edge of each edge vertex. */
int ds_mt_emit(const float* pos, const float* sdf, int64_t n, const int32_t* tets, int64_t T, const int32_t* tet_edge,
               const int32_t* ea, const int32_t* eb, int64_t E, const int32_t* vptr, const float* thick,
               const int32_t* toff, const int32_t* edge_id, const int32_t* vert_id, const ds_mt_counts_t* counts,
               float* verts, int64_t* out_tets, int64_t* out_faces, int32_t* vsrc, int32_t* xedge, ds_stream_t stream);
/* Floats of the workspace ds_mt_backward needs for dL/dt. */
int64_t ds_mt_backward_workspace_floats(int64_t n_cross);
/* Autograd of the above (the reference relies on torch autograd through dmtet_geometry.py:155-173 and the final
 * gather all_verts[all_unique_tets]): grad_verts ((n_used + n_cross) x 3) -> dpos (n x 3), dsdf (n) by a gather
 * over the CSR (kept vertices pass their gradient through; edge vertices add the closed-form derivatives), and,
 * when dt != NULL, dL/dt (one f32) by fixed-order partial sums in work (ds_mt_backward_workspace_floats).  No
 * atomics: bitwise reproducible. */
int ds_mt_backward(const float* grad_verts, const float* pos, const float* sdf, int64_t n, const int32_t* ea,
                   const int32_t* eb, int64_t E, const int32_t* vptr, const int32_t* vadj, const float* thick,
                   const int32_t* edge_id, const int32_t* vert_id, const int32_t* xedge, int64_t n_used,
                   int64_t n_cross, float* dpos, float* dsdf, float* dt, float* work, ds_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Signed distance from a triangle mesh to points (csrc/meshsdf.hip, ABI 36).  Replaces open3d's
 * RaycastingScene.compute_signed_distance of the reference's shape loops (src/dmtet/geometry/dmtet_thickness.py:
 * 301-314, dmtet_interpolate.py:318-351, experiments/geometry_train.py:170-197).  Brute force over all (point, face)
 * pairs in fp32; per point the exact point-triangle distance to the nearest face, that face (the lowest index on
 * equal squared distances), and the generalised winding number (sum of the signed solid angles / 4 pi).  Signed
 * distance: negative inside, inside = winding number > 0.5, so faces must be wound counter-clockwise seen from
 * outside.  No atomics; a point's result does not depend on the other points of the call.
 *
 * Face record (DS_MESH_SDF_FACE_RECORD floats per face, 16-byte aligned): [0,9) the vertices a, b, c;
 * [9,12) 1/|b-a|^2, 1/|c-b|^2, 1/|a-c|^2 (0 for a zero-length edge); [12,15) the unit normal (b-a) x (c-a);
 * [15] 1 when the face has area, else 0 (such a face gives the distance to its segment or point and no solid angle).
 * ---------------------------------------------------------------------------------------------- */
#define DS_MESH_SDF_FACE_RECORD 16
/* Once per mesh: verts (V x 3) f32, faces (F x 3) int32 (indices checked by the caller) -> face_records
 * (F x DS_MESH_SDF_FACE_RECORD) f32. */
int ds_mesh_sdf_pack(const float* verts, const int32_t* faces, int64_t V, int64_t F, float* face_records,
                     ds_stream_t stream);
/* Bytes of the workspace for the launch shape that splits the faces across workgroups: what ds_mesh_sdf_query
 * should be given for P points and F faces.  0 when the one-launch shape is the better one (many points, or one
 * chunk of faces) and force_split == 0; -1 when the sizes are out of range. */
int64_t ds_mesh_sdf_workspace_bytes(int64_t P, int64_t F, int force_split);
/* Per query: points (P x 3) f32 -> out_signed (P) f32 and, where not NULL, out_unsigned (P) f32, out_face (P) int32,
 * out_winding (P) f32.  work == NULL: one launch.  work != NULL (work_bytes >= ds_mesh_sdf_workspace_bytes(P, F, 1)):
 * the faces are split across workgroups and a second kernel combines the parts in fixed order; both shapes give the
 * same bits.  A non-finite coordinate gives a non-finite result (the Python side rejects such input). */
int ds_mesh_sdf_query(const float* points, int64_t P, const float* face_records, int64_t F, float* out_signed,
                      float* out_unsigned, int32_t* out_face, float* out_winding, void* work, int64_t work_bytes,
                      ds_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Debiased Sinkhorn divergence between point clouds (csrc/sinkhorn.hip, ABI 37).  Replaces geomloss==0.2.6
 * SamplesLoss("sinkhorn", p=2, blur, scaling, debias, reach=None) on its tensorized backend, which the reference's
 * spectral loss calls (src/ddsp/mss_loss.py:104-117).  Cost C(x, y) = |x - y|^2 / 2 from the coordinates on the fly;
 * softmin_eps(C, h)_i = -eps LSE_j(h_j - C_ij / eps).  Memory O(B (N + M) D): no N x M matrix.  No atomics; a
 * batch's result does not depend on B or on its index, and two runs give the same bits.
 *
 * x (B x N x D) f32, y (B x M x D) f32, a (B x N) f32, b (B x M) f32 weights (> 0; the caller passes 1/N, 1/M for
 * uniform ones), 1 <= D <= 32.  The caller fetches the bbox record, checks it and derives the eps schedule (the one
 * synchronisation of a call); nothing else here synchronises.
 * ---------------------------------------------------------------------------------------------- */
/* Floats of the workspace of one call: log a, log b, two potential slots and the last step's LSEs (B (N + M) +
 * 3 B (2N + 2M)); -1 when the sizes are out of range.  The backward reads what ds_sinkhorn_final left there. */
int64_t ds_sinkhorn_workspace_floats(int64_t B, int64_t N, int64_t M);
/* out (3 D + 3) f32: [0, D) per-coordinate minimum over every point of x and y of every batch, [D, 2D) maximum,
 * [2D] least a, [2D + 1] least b, [2D + 2, 3D + 3) counts of non-finite values (one per coordinate, then the
 * weights).  The diameter is the norm of max - min. */
int ds_sinkhorn_bbox(const float* x, const float* y, const float* a, const float* b, int64_t B, int64_t N, int64_t M,
                     int64_t D, float* out, ds_stream_t stream);
/* The whole eps loop: f_ba, g_ab (and with debias f_aa, g_bb) initialised at eps_list[0] (HOST array of n_eps
 * positive values), then for every eps of the list the four softmins and the averaging (f + ft) / 2, one launch per
 * eps.  The potentials end in the workspace. */
int ds_sinkhorn_loop(const float* x, const float* y, const float* a, const float* b, int64_t B, int64_t N, int64_t M,
                     int64_t D, const float* eps_list, int n_eps, int debias, float* work, ds_stream_t stream);
/* The last extrapolation at eps (= blur^2) without averaging, keeping each row's LSE, then per batch
 * loss[b] = <a, f_ba - f_aa> + <b, g_ab - g_bb> (debias) or <a, f_ba> + <b, g_ab>, summed in fp64. */
int ds_sinkhorn_final(const float* x, const float* y, const float* a, const float* b, int64_t B, int64_t N, int64_t M,
                      int64_t D, float eps, int debias, float* work, double* loss, ds_stream_t stream);
/* dS/dx_i = g_b a_i (sum_j P_ij (x_i - y_j) - sum_k Q_ik (x_i - x_k)) with P, Q the row-softmax weights of the last
 * f_ba, f_aa softmins (what autograd gives through geomloss's last step), and the mirror image for y; grad_loss (B)
 * f32 on the device.  grad_x / grad_y may be NULL. */
int ds_sinkhorn_backward(const float* x, const float* y, const float* a, const float* b, int64_t B, int64_t N,
                         int64_t M, int64_t D, float eps, int debias, const float* work, const float* grad_loss,
                         float* grad_x, float* grad_y, ds_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Deformation gradient at the Gauss points and the stress -> nodal force gather (csrc/deform.hip, ABI 38).  Replaces
 * the reference's Deform (src/diffelastic/deform.py:8-180) without its materialised tables: the physical shape
 * gradients B[t,g] = D[g] inv(A_t) are recomputed per element from the four corner coordinates (A_t = the columns
 * v1-v4, v2-v4, v3-v4, src/diffelastic/mesh.py:58-99; adjugate over determinant in fp32).  No atomics; a column's
 * result does not depend on the other columns of the call, and two runs give the same bits.
 *
 * Common arguments: verts (nv x 3) f32; tets (T x N) int32, N = 4 (order 1) or 10 (order 2), indices checked by the
 * caller; dtab (G x N x 3) f32 = dN/dL at the Gauss points times dL/dx, gw (G) f32 the Gauss weights, G =
 * (order + 2)^3 (deform.py:12-17, 47-56).  Gauss-point tensors are indexed t * G + g like the reference's.
 * ---------------------------------------------------------------------------------------------- */
/* Any of: sfd (T*G x N x 3) f32 = B (deform.py:35-68), intw (T*G) f32 = gw[g] |det A_t| (deform.py:136-147), det (T)
 * f32 = det A_t (the caller's degenerate-element check).  NULL outputs are skipped.  For API parity and tests: the two
 * functions below do not read these tables. */
int ds_deform_tables(const float* verts, int64_t nv, const int32_t* tets, int64_t T, int order, const float* dtab,
                     const float* gw, float* sfd, float* intw, float* det, ds_stream_t stream);
/* F[b, t*G+g, i, j] = sum_a u[b, tet[t,a], i] B[t,g,a,j] (deform.py:70-102), times intw[t*G+g] when weighted != 0.
 * u (batch x nv x 3) f32 -> F (batch x T*G x 3 x 3) f32, 16-byte aligned. */
int ds_deform_gradient(const float* verts, int64_t nv, const int32_t* tets, int64_t T, int order, const float* dtab,
                       const float* gw, const float* u, int64_t batch, int weighted, float* F, ds_stream_t stream);
/* f[b, 3 n + i] = sum over (t, a) with tet[t,a] == n, over g and j, of intw[t*G+g] P[b,t*G+g,i,j] B[t,g,a,j]
 * (deform.py:104-125, 149-180; the reference scatters with atomics), without the intw factor when weighted == 0.
 * P (batch x T*G x 3 x 3) f32, 16-byte aligned -> f (batch x 3 nv) f32.  inc_ptr (nv + 1), inc (T*N) int32: the
 * node -> t*N + a incidence list in CSR form, the order of a node's entries is the order of its sum.  work: batch *
 * T * N * 3 floats (the per-element forces between the two passes). */
int ds_deform_force(const float* verts, int64_t nv, const int32_t* tets, int64_t T, int order, const float* dtab,
                    const float* gw, const int32_t* inc_ptr, const int32_t* inc, const float* P, int64_t batch,
                    int weighted, float* work, float* f, ds_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * A general constant tangent on the assembled geometry tensors (csrc/tangent.hip, ABI 39).  The reference assembles
 * A^T B A for any 9 x 9 B = jacobian_F() (src/diffelastic/diff_model.py:184-220); here klam of ds_assemble_kml already
 * holds H_ab[j][l] = integral dN_a/dx_j dN_b/dx_l of every block slot, and with vec(F) row 3i+j (:207-211)
 *   K_ab[i][k] = sum_jl C[3i+j][3k+l] H_ab[j][l].
 * ---------------------------------------------------------------------------------------------- */
/* The per-material step for a tangent C (81 doubles on the HOST, row 3i+j, column 3k+l; passed to the kernels by value):
 * k64 (nnzb x 9, may be NULL) = C : H in fp64, one fixed summation order; k32 = its fp32 rounding; k32t (may be NULL) =
 * k32 with every 3x3 block transposed; ms32 = (float)ms; dinv32 (nv x 9) = the fp32 inverse of the fp64 diagonal blocks
 * (identity for a node no element references), as the isotropic combine step computes it.  nnzb < 2^31. */
int ds_combine_tangent(const double* klam, const double* ms, int64_t nnzb, const int32_t* diagidx, int64_t nv,
                       const double* C, double* k64, float* k32, float* k32t, float* ms32, float* dinv32,
                       ds_stream_t stream);
/* Strain-energy moment tensors of the columns of U (3 nv x m fp32, row-major, leading dimension ldu >= m, 4-byte aligned):
 *   Q[c][3i+j][3k+l] = sum_a sum_{b in row a} u_a,i H_ab[j][l] u_b,k     (m x 81 fp64),
 * so that u_c^T K(C) u_c = sum of C .* Q[c] for every tangent C.  fp64 arithmetic on the BSR pattern (rowptr, colidx,
 * klam); two stages in a fixed order and no atomics: two calls give the same bits, and a column's Q does not depend on
 * the other columns of the call.  1 <= m <= DS_TANGENT_FORMS_MAX_COLS.  work: scratch of the stated size, 8-byte aligned. */
#define DS_TANGENT_FORMS_MAX_COLS 589815
size_t ds_tangent_forms_workspace_bytes(int64_t nv, int m);
int ds_tangent_forms(const int32_t* rowptr, const int32_t* colidx, const double* klam, int64_t nv, const float* U,
                     int64_t ldu, int m, double* Q, void* work, size_t work_bytes, ds_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Mode shapes sampled at points of the mesh: the modal gains of a strike (csrc/modesample.hip).  Stands in for the free
 * ``amp`` of the reference's oscillator modules (src/ddsp/oscillator.py:76), which nothing ties to the mode shapes: a
 * strike at point p with direction d excites mode i with the gain d . u_i(p).
 *
 * Common arguments: tets (T x N) int32, N = 4 (order 1) or 10 (order 2), local node order of fem_tables.py; U (3 nv x m)
 * fp64, row 3 * node + c, leading dimension ldu >= m (the layout of DiffSoundObj.U_hat); per point p of P: elem[p]
 * int32 element id, L[p] four fp32 barycentrics of that element, dir[p] three fp32 components.  Element ids and node
 * ids are the caller's to check (as for the Deform operators above).  fp64 buffers 8-byte aligned.  Asynchronous on
 * the stream; nothing is allocated.  One wave owns a point and sums in a fixed order: two calls give the same bits.
 * There is no gradient to U: the eigenvectors are constants.
 * ---------------------------------------------------------------------------------------------- */
/* out[p, i] = sum_a N_a(L_p) sum_c dir[p, c] U[3 tets[elem_p, a] + c, i]   (P x m fp64), the shape functions in fp64
 * from the fp32 L; vec[p, i, c] = sum_a N_a U[3 node_a + c, i] (P x m x 3 fp64), the displacement without the dot
 * product.  Either output may be NULL, not both; dir may be NULL when out is. */
int ds_mode_sample_fwd(const int32_t* tets, int64_t T, int N, int64_t nv, const double* U, int64_t ldu, int m,
                       const int32_t* elem, const float* L, const float* dir, int64_t P, double* out, double* vec,
                       ds_stream_t stream);
/* gout (P x m) fp64 ->  gL[p, j] = sum_i gout[p, i] sum_a dN_a/dL_j dir_p . U[node_a, :, i]   (P x 4 fp64)  and
 * gdir[p, c] = sum_i gout[p, i] sum_a N_a U[3 node_a + c, i]   (P x 3 fp64).  Either may be NULL, not both. */
int ds_mode_sample_bwd(const int32_t* tets, int64_t T, int N, int64_t nv, const double* U, int64_t ldu, int m,
                       const int32_t* elem, const float* L, const float* dir, int64_t P, const double* gout, double* gL,
                       double* gdir, ds_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Radiated sound at a listener (csrc/multipole.hip; still ABI 45, three added symbols): the multipole series of each mode's
 * exterior field about a centre x0, convention e^{-i w t}, G = e^{ikr} / (4 pi r) as in the boundary elements above.  The
 * reference has no counterpart.  For mode j (wave number k[j] > 0), d = x - x0, r = |d|, u = d / r:
 *   out[p, j] = sum_{l=0..L} sum_{n=-l..l} coef[l^2 + l + n, j] h_l(k[j] r_p) Y_{l,n}(u_p),
 * h_l the spherical Hankel function of the first kind (upward recurrence from h_0 = -i e^{iz} / z), Y_{l,n} the real
 * orthonormal spherical harmonics: Y_{l,0} = Y_l^0, Y_{l,n>0} = sqrt2 (-1)^n Re Y_l^n, Y_{l,n<0} = sqrt2 (-1)^n Im Y_l^|n|, Y_l^n
 * with the Condon-Shortley phase; evaluated as solid harmonics by Cartesian recurrences, so a point on the z axis is an
 * ordinary point.  Everything fp64 on the DEVICE, complex data interleaved (re, im): pts (P x 3), center (3), k (m), coef and
 * gcoef (N x m) complex with N = (L + 1)^2 and the MODES contiguous (the transpose of a per-mode coefficient list: lane j of a
 * wavefront owns mode j), out and gout (P x m) complex.  r = 0 and k <= 0 are the caller's to refuse (non-finite results).
 * ds_multipole_bwd: with <a, b> = sum conj(a) b, gpts (P x 3) = d Re<gout, out> / d pts and gcoef = sum_p gout conj(h_l) Y, the
 * gradient of Re<gout, out> to (Re coef, Im coef) as a complex number.  Either may be NULL and is then not computed, not both.
 * gcoef needs work of ds_multipole_workspace_bytes(P, m, L) = 16 min(P, DS_MULTIPOLE_GCOEF_BLOCKS) N m bytes (0 for arguments that
 * would be refused), 16-byte aligned: per-workgroup partial sums over the points, added in ascending order by a closing
 * kernel; work may be NULL when gcoef is.  One wavefront per point, no atomics, every output and workspace element has one
 * owner: the same bits from the same inputs.  Asynchronous on the stream, no allocation, no synchronisation.  Refused
 * (DS_ERR_ARG, message in ds_last_error()): a null required pointer; P outside 1..DS_MULTIPOLE_MAX_POINTS; m outside
 * 1..DS_MULTIPOLE_MAX_MODES; L outside 0..DS_MULTIPOLE_MAX_ORDER; both gradient outputs NULL; work_bytes below the query; a
 * misaligned workspace or operand (complex operands 16 bytes, real ones 8).
 * ---------------------------------------------------------------------------------------------- */
#define DS_MULTIPOLE_MAX_ORDER 32        /* L; a real object at 10 kHz has k a of about 18 and needs L in the twenties */
#define DS_MULTIPOLE_MAX_MODES 512       /* m */
#define DS_MULTIPOLE_MAX_POINTS 16777216 /* P per call */
#define DS_MULTIPOLE_GCOEF_BLOCKS 128    /* workgroups (and workspace slabs) of the gcoef reduction */
int64_t ds_multipole_workspace_bytes(int64_t P, int m, int L);
int ds_multipole_fwd(const double* pts, const double* center, const double* k, const double* coef, int64_t P, int m, int L,
                     double* out, ds_stream_t stream);
int ds_multipole_bwd(const double* gout, const double* pts, const double* center, const double* k, const double* coef, int64_t P,
                     int m, int L, void* work /*or NULL with gcoef*/, int64_t work_bytes, double* gpts /*or NULL*/,
                     double* gcoef /*or NULL*/, ds_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DIFFSOUND_HIP_H */
