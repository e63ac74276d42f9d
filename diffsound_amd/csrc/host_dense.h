// The small (<= 3b x 3b) dense algebra of the eigensolver's native loop (lobpcg.cpp): row-major fp64 on the calling host thread,
// LAPACK / BLAS through the caller's ds_lapack_t.  Pure host code - no device call, no stream.  The named steps are the twins of
// the functions of the same names in lobpcg/dense.py, whose docstrings say what they compute (read the two side by side);
// tests/test_cabi_cpu.py checks one against the other through ds_host_raw_basis / ds_host_rr_step / ds_host_start_block.
#pragma once
#include <chrono>
#include <vector>

#include "diffsound_hip.h"

namespace ds::dense {

struct Mat {
    int r = 0, c = 0;
    std::vector<double> a;
    Mat() = default;
    Mat(int r_, int c_) : r(r_), c(c_), a((size_t)r_ * c_, 0.0) {}
    double& operator()(int i, int j) { return a[(size_t)i * c + j]; }
    double operator()(int i, int j) const { return a[(size_t)i * c + j]; }
    // sub-block copies: values move, nothing is computed
    Mat block(int i0, int j0, int rows, int cols) const;  // this[i0 : i0 + rows, j0 : j0 + cols]
    void set_block(int i0, int j0, const Mat& M);         // this[i0 : i0 + M.r, j0 : j0 + M.c] = M
    void set_block_T(int i0, int j0, const Mat& M);       // this[i0 : i0 + M.c, j0 : j0 + M.r] = M^T
};
Mat hcat(const Mat& A, const Mat& B);  // [A B]

// host time of one solve spent in gemm / the eigensolvers, per thread (the loop resets and reads it: DS_EXP_TIMING=1)
struct Timers {
    double eigh = 0, dense = 0;
    int neigh = 0;
};
extern thread_local Timers g_timers;
inline double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

void symmetrize(Mat& G);
bool all_finite(const Mat& G);
Mat gemm(const ds_lapack_t& la, const Mat& A, bool ta, const Mat& B, bool tb);  // op(A) op(B)
bool cholesky(const Mat& A, Mat& L);  // lower factor, L L^T = A; false on breakdown
Mat lower_inverse(const Mat& L);
// eigenvalues ascending, columns of Z = eigenvectors; false when LAPACK reports failure.  eigh_lowest: Zm = the lowest m vectors
bool eigh(const ds_lapack_t& la, const Mat& Gsym, std::vector<double>& w, Mat& Z);
bool eigh_lowest(const ds_lapack_t& la, const Mat& Gsym, int m, std::vector<double>& w, Mat& Zm);
bool svqb_transform(const ds_lapack_t& la, const Mat& G, Mat& T);
bool orthonormalizer_q(const ds_lapack_t& la, const Mat& G, const std::vector<double>* rem, Mat& T, double& amp);
bool orthonormal_columns(const ds_lapack_t& la, const Mat& Tm, Mat& Q);

// C = V^T M W, G0 = W^T M W (symmetric) -> T, CtC = C^T C, amp.  BrokeDown is the Python form's None; LapackFailed: dsyevd failed
// in the clamped-eigenvalue fallback.  What a caller does with either is its own business.
enum class Projected { Ok, BrokeDown, LapackFailed };
Projected project_in_coefficients(const ds_lapack_t& la, const Mat& C, const Mat& G0, bool cholesky_gate, Mat& T, Mat& CtC,
                                  double& amp);
// true: G (sz x sz, sz = nxp + na) and Qw ((w0 + na) x na, W_o in the raw basis: the Python form's Q is [E | Qw] with E the unit
// columns that pick [X_a P]); false: the caller takes the explicit route.  lam_locked: the ncl locked Ritz values.
bool raw_basis_transform(const ds_lapack_t& la, const Mat& GG, const Mat& Gxp, const double* lam_locked, int ny, int ncl, int nxp,
                         int na, double ortho_tol, double eps, Mat& G, Mat& Qw);
// Symmetrises G in place; E = ALL its eigenvalues ascending.  false (the library's error message set) when LAPACK fails.
bool rr_step(const ds_lapack_t& la, Mat& G, int na, std::vector<double>& E, Mat& Z1, Mat& Zp);
// [Z1 Zp]^T G [Z1 Zp] of the new basis (the next step's Gxp), symmetrised: the half-flop form of _ritz_step's Gxp_
Mat next_projected_K(const ds_lapack_t& la, const Mat& G, const std::vector<double>& E, const Mat& Z1, const Mat& Zp);
// Coefficients of [X' P'] in the raw basis: [E | Qw] ZZ = Qw Z_w + E Z_xp, ZZ = [Z1 Zp] (sz x 2 na)
Mat raw_update_coefficients(const ds_lapack_t& la, const Mat& Qw, const Mat& ZZ, int ny, int ncl, int nxp, int na);

}  // namespace ds::dense
