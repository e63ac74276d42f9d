// The native eigensolver loop's small dense algebra (host_dense.h) and its pure-host entry points.  No device call in this file.
#include "host_dense.h"

#include <algorithm>
#include <cmath>
#include <limits>

#include "ds_common.h"

namespace ds::dense {

thread_local Timers g_timers;

Mat Mat::block(int i0, int j0, int rows, int cols) const {
    Mat B(rows, cols);
    for (int i = 0; i < rows; ++i)
        for (int j = 0; j < cols; ++j) B(i, j) = (*this)(i0 + i, j0 + j);
    return B;
}

void Mat::set_block(int i0, int j0, const Mat& M) {
    for (int i = 0; i < M.r; ++i)
        for (int j = 0; j < M.c; ++j) (*this)(i0 + i, j0 + j) = M(i, j);
}

void Mat::set_block_T(int i0, int j0, const Mat& M) {
    for (int i = 0; i < M.r; ++i)
        for (int j = 0; j < M.c; ++j) (*this)(i0 + j, j0 + i) = M(i, j);
}

Mat hcat(const Mat& A, const Mat& B) {
    Mat AB(A.r, A.c + B.c);
    AB.set_block(0, 0, A);
    AB.set_block(0, A.c, B);
    return AB;
}

void symmetrize(Mat& G) {
    for (int i = 0; i < G.r; ++i)
        for (int j = i + 1; j < G.c; ++j) {
            const double v = 0.5 * (G(i, j) + G(j, i));
            G(i, j) = G(j, i) = v;
        }
}

bool all_finite(const Mat& G) {
    for (double v : G.a)
        if (!std::isfinite(v)) return false;
    return true;
}

// row-major through column-major dgemm: C^T = op(B)^T op(A)^T
Mat gemm(const ds_lapack_t& la, const Mat& A, bool ta, const Mat& B, bool tb) {
    const int m = ta ? A.c : A.r, k = ta ? A.r : A.c, n = tb ? B.r : B.c;
    Mat C(m, n);
    if (m == 0 || n == 0 || k == 0) return C;
    struct T_ { double t0 = now_s(); ~T_() { g_timers.dense += now_s() - t0; } } t_;
    char opb = tb ? 'T' : 'N', opa = ta ? 'T' : 'N';
    int mm = n, nn = m, kk = k, ldb = B.c, lda = A.c, ldc = n;
    double one = 1.0, zero = 0.0;
    la.dgemm(&opb, &opa, &mm, &nn, &kk, &one, const_cast<double*>(B.a.data()), &ldb, const_cast<double*>(A.a.data()), &lda,
             &zero, C.a.data(), &ldc);
    return C;
}

// sum of a[k] * b[k * sb], k < n, on four independent accumulators: the compiler keeps a floating-point reduction in its
// source order, i.e. one dependent chain of 4-cycle multiply-adds - the factorisations below spent 0.07 ms each on an 80 x 80
// block that way, seven of them per iteration: most of the "rest" of profiles/r05_host_time_one_lane.txt (0.4 ms per iteration)
inline double dot4(const double* a, const double* b, int sb, int n) {
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    int k = 0;
    for (; k + 4 <= n; k += 4) {
        s0 += a[k] * b[(size_t)k * sb];
        s1 += a[k + 1] * b[(size_t)(k + 1) * sb];
        s2 += a[k + 2] * b[(size_t)(k + 2) * sb];
        s3 += a[k + 3] * b[(size_t)(k + 3) * sb];
    }
    for (; k < n; ++k) s0 += a[k] * b[(size_t)k * sb];
    return (s0 + s1) + (s2 + s3);
}

bool cholesky(const Mat& A, Mat& L) {
    const int n = A.r;
    L = Mat(n, n);
    double* l = L.a.data();
    for (int j = 0; j < n; ++j) {
        const double d = A(j, j) - dot4(l + (size_t)j * n, l + (size_t)j * n, 1, j);
        if (!(d > 0.0) || !std::isfinite(d)) return false;
        const double ljj = std::sqrt(d);
        L(j, j) = ljj;
        for (int i = j + 1; i < n; ++i) L(i, j) = (A(i, j) - dot4(l + (size_t)i * n, l + (size_t)j * n, 1, j)) / ljj;
    }
    return all_finite(L);
}

Mat lower_inverse(const Mat& L) {
    const int n = L.r;
    Mat X(n, n);
    const double* l = L.a.data();
    double* x = X.a.data();
    for (int j = 0; j < n; ++j) {
        X(j, j) = 1.0 / L(j, j);
        for (int i = j + 1; i < n; ++i)  // (X's column j is walked with stride n: 80 x 80 doubles sit in the L1)
            X(i, j) = -dot4(l + (size_t)i * n + j, x + (size_t)j * n + j, n, i - j) / L(i, i);
    }
    return X;
}

bool eigh(const ds_lapack_t& la, const Mat& Gsym, std::vector<double>& w, Mat& Z) {
    struct T_ { double t0 = now_s(); ~T_() { g_timers.eigh += now_s() - t0; ++g_timers.neigh; } } t_;
    const int n = Gsym.r;
    std::vector<double> A = Gsym.a;  // symmetric: row-major == column-major
    w.assign(n, 0.0);
    char jobz = 'V', uplo = 'L';
    int nn = n, lda = n, info = 0, lwork = -1, liwork = -1, iq = 0;
    double wq = 0.0;
    la.dsyevd(&jobz, &uplo, &nn, A.data(), &lda, w.data(), &wq, &lwork, &iq, &liwork, &info);
    if (info != 0) return false;
    lwork = (int)wq;
    liwork = iq;
    std::vector<double> work((size_t)std::max(1, lwork));
    std::vector<int> iwork((size_t)std::max(1, liwork));
    la.dsyevd(&jobz, &uplo, &nn, A.data(), &lda, w.data(), work.data(), &lwork, iwork.data(), &liwork, &info);
    if (info != 0) return false;
    Z = Mat(n, n);  // column-major eigenvector j = A[j * n + i]  ->  Z(i, j)
    for (int j = 0; j < n; ++j)
        for (int i = 0; i < n; ++i) Z(i, j) = A[(size_t)j * n + i];
    return true;
}

// The LOWEST m eigenpairs of a symmetric matrix: w = all n eigenvalues ascending, Zm (n x m, row-major) = the first m eigenvectors.
// The Ritz step wants a third of the vectors of its 3 na x 3 na problem.  dsyevd is tridiagonalisation + divide and conquer on the
// tridiagonal matrix + back-transformation of ALL n vectors (dormtr, 2 n^3 flops); with the three stages called one by one only
// the wanted m columns are back-transformed: 13 % of the call at n = 240, m = 80 (the divide-and-conquer stage, which has no
// subset form, is half of it).  (dsyevr / dsyevx on the index range and the MRRR tridiagonal solver dstemr are slower in SciPy's
// OpenBLAS: profiles/r05_host_eigh_probe.txt, profiles/r06_host_eigh_stages.txt.)  Falls back to dsyevd when the table has no stages.
bool eigh_lowest(const ds_lapack_t& la, const Mat& Gsym, int m, std::vector<double>& w, Mat& Zm) {
    const int n = Gsym.r;
    if (!la.dsytrd || !la.dstedc || !la.dormtr || m >= n || n < 32) {
        Mat Z;
        if (!eigh(la, Gsym, w, Z)) return false;
        Zm = Z.block(0, 0, n, std::min(m, n));
        return true;
    }
    struct T_ { double t0 = now_s(); ~T_() { g_timers.eigh += now_s() - t0; ++g_timers.neigh; } } t_;
    thread_local std::vector<double> A, e, tau, work, Zt;
    thread_local std::vector<int> iwork;
    A = Gsym.a;  // symmetric: row-major == column-major
    w.assign(n, 0.0);
    e.assign(n, 0.0), tau.assign(n, 0.0);
    int nn = n, lda = n, info = 0;
    int lwork = std::max(64 * n, 1 + 4 * n + n * n), liwork = 3 + 5 * n;
    if ((int)work.size() < lwork) work.resize(lwork);
    if ((int)iwork.size() < liwork) iwork.resize(liwork);
    if (Zt.size() < (size_t)n * n) Zt.resize((size_t)n * n);
    char lo = 'L', compz = 'I', side = 'L', notr = 'N';
    la.dsytrd(&lo, &nn, A.data(), &lda, w.data(), e.data(), tau.data(), work.data(), &lwork, &info);
    if (info != 0) return false;
    la.dstedc(&compz, &nn, w.data(), e.data(), Zt.data(), &lda, work.data(), &lwork, iwork.data(), &liwork, &info);
    if (info != 0) return false;
    int mm = m;
    la.dormtr(&side, &lo, &notr, &nn, &mm, A.data(), &lda, tau.data(), Zt.data(), &lda, work.data(), &lwork, &info);
    if (info != 0) return false;
    Zm = Mat(n, m);
    for (int j = 0; j < m; ++j)
        for (int i = 0; i < n; ++i) Zm(i, j) = Zt[(size_t)j * n + i];
    return true;
}

// T with (W T)^T M (W T) = I given G = W^T M W, clamped-eigenvalue form (dense._svqb_transform)
bool svqb_transform(const ds_lapack_t& la, const Mat& G, Mat& T) {
    const int n = G.r;
    std::vector<double> d(n);
    for (int i = 0; i < n; ++i) d[i] = 1.0 / std::sqrt(std::max(G(i, i), 1e-300));
    Mat Gs = G;
    symmetrize(Gs);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) Gs(i, j) *= d[i] * d[j];
    std::vector<double> E;
    Mat Z;
    if (!eigh(la, Gs, E, Z)) return false;
    double emax = 0.0;
    for (double e : E) emax = std::max(emax, std::fabs(e));
    T = Mat(n, n);
    for (int j = 0; j < n; ++j) {
        const double e = std::max(E[j], 1e-12 * emax);
        const double s = 1.0 / std::sqrt(e);
        for (int i = 0; i < n; ++i) T(i, j) = d[i] * Z(i, j) * s;
    }
    return true;
}

// (T, amp) of dense._orthonormalizer_q; rem: optional squared M-norms removed by the preceding projection
bool orthonormalizer_q(const ds_lapack_t& la, const Mat& Gin, const std::vector<double>* rem, Mat& T, double& amp) {
    Mat G = Gin;
    symmetrize(G);
    const int n = G.r;
    std::vector<double> diag(n), d(n);
    for (int i = 0; i < n; ++i) {
        diag[i] = std::max(G(i, i), 1e-300);
        d[i] = 1.0 / std::sqrt(diag[i]);
    }
    Mat Gs = G;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) Gs(i, j) *= d[i] * d[j];
    Mat L;
    if (!cholesky(Gs, L)) {
        amp = std::numeric_limits<double>::infinity();
        return svqb_transform(la, G, T);
    }
    double lmin = std::numeric_limits<double>::infinity();
    for (int i = 0; i < n; ++i) lmin = std::min(lmin, L(i, i));
    amp = 1.0 / std::max(lmin, 1e-300);
    if (rem)
        for (int i = 0; i < n; ++i) amp = std::max(amp, std::sqrt((*rem)[i] / diag[i]));
    const Mat Li = lower_inverse(L);
    T = Mat(n, n);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) T(i, j) = d[i] * Li(j, i);
    return true;
}

// orthonormal basis (Euclidean) of the columns of Tm: scaled Cholesky-QR twice (dense._orthonormal_columns)
bool orthonormal_columns(const ds_lapack_t& la, const Mat& Tm, Mat& Q) {
    Q = Tm;
    for (int pass = 0; pass < 2; ++pass) {
        Mat G = gemm(la, Q, true, Q, false);
        const int n = G.r;
        std::vector<double> d(n);
        for (int i = 0; i < n; ++i) d[i] = 1.0 / std::sqrt(std::max(G(i, i), 1e-300));
        symmetrize(G);
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j) G(i, j) *= d[i] * d[j];
        Mat L;
        if (!cholesky(G, L)) return false;  // (the Python loop falls back to Householder QR: the caller does, too)
        const Mat Li = lower_inverse(L);
        Mat X(n, n);
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j) X(i, j) = d[i] * Li(j, i);
        Q = gemm(la, Q, false, X, false);
    }
    return true;
}

Projected project_in_coefficients(const ds_lapack_t& la, const Mat& C, const Mat& G0, bool cholesky_gate, Mat& T, Mat& CtC,
                                  double& amp) {
    const int na = G0.r;
    CtC = gemm(la, C, true, C, false);
    Mat Gp(na, na);
    for (int i = 0; i < na; ++i)
        for (int j = 0; j < na; ++j) Gp(i, j) = G0(i, j) - CtC(i, j);
    for (int i = 0; i < na; ++i)
        if (Gp(i, i) <= 1e-9 * std::fabs(G0(i, i))) return Projected::BrokeDown;
    if (!all_finite(Gp)) return Projected::BrokeDown;
    Mat L;
    if (cholesky_gate && !cholesky(Gp, L)) return Projected::BrokeDown;
    std::vector<double> rem(na);
    for (int i = 0; i < na; ++i) rem[i] = CtC(i, i);
    return orthonormalizer_q(la, Gp, &rem, T, amp) ? Projected::Ok : Projected::LapackFailed;
}

bool raw_basis_transform(const ds_lapack_t& la, const Mat& GG, const Mat& Gxp, const double* lam_locked, int ny, int ncl, int nxp,
                         int na, double ortho_tol, double eps, Mat& G, Mat& Qw) {
    const int w0 = ny + ncl + nxp, pr = w0 + na;
    const Mat C = GG.block(0, na, w0, na);
    Mat G0 = GG.block(w0, na, na, na);
    symmetrize(G0);
    Mat T, CtC;
    double amp = 0.0;
    // (no Cholesky gate: the factorisation of the diagonally scaled block inside orthonormalizer_q is the breakdown test - amp = inf,
    // the explicit route; the unscaled Cholesky in front of it that the Python form has was 0.07 ms of every iteration for the
    // same answer.  A dsyevd failure in the fallback is the explicit route, too.)
    if (project_in_coefficients(la, C, G0, false, T, CtC, amp) != Projected::Ok) return false;
    if (!std::isfinite(amp) || (ortho_tol > 0.0 && eps * amp >= ortho_tol)) return false;
    Mat CT = gemm(la, C, false, T, false);
    Mat GKraw(pr, pr);  // [Y X P W]^T K [Y X P W]: known blocks among Y, X, P (K Y = 0, X_l^T K X_l = diag(lam_l)); measured columns of W
    for (int i = 0; i < ncl; ++i) GKraw(ny + i, ny + i) = lam_locked[i];
    GKraw.set_block(ny + ncl, ny + ncl, Gxp);
    const Mat GKv = GG.block(0, 0, w0, na);
    GKraw.set_block(0, w0, GKv);
    GKraw.set_block_T(w0, 0, GKv);
    for (int i = 0; i < na; ++i)
        for (int j = 0; j < na; ++j) GKraw(w0 + i, w0 + j) = 0.5 * (GG(w0 + i, j) + GG(w0 + j, i));
    // Q = [E | Qw]: E picks the rows of [X_a P] (unit columns), Qw = [-C T; T] are W_o's coordinates.  G = Q^T GKraw Q block by
    // block - the unit columns cost nothing: a third of the flops of the two full products of the Python form (one lane alone is
    // bound by this host algebra, not by the kernels)
    for (double& v : CT.a) v = -v;
    Qw = Mat(pr, na);
    Qw.set_block(0, 0, CT);
    Qw.set_block(w0, 0, T);
    const Mat H = gemm(la, GKraw, false, Qw, false);  // (pr x na) = GKraw Qw
    const Mat Gww = gemm(la, Qw, true, H, false);     // (na x na) = Qw^T GKraw Qw
    const Mat Hxp = H.block(ny + ncl, 0, nxp, na);
    G = Mat(nxp + na, nxp + na);
    G.set_block(0, 0, Gxp);
    G.set_block(0, nxp, Hxp);
    G.set_block_T(nxp, 0, Hxp);
    G.set_block(nxp, nxp, Gww);
    return true;
}

bool rr_step(const ds_lapack_t& la, Mat& G, int na, std::vector<double>& E, Mat& Z1, Mat& Zp) {
    symmetrize(G);
    // (only the wanted third of the vectors is back-transformed: eigh_lowest.  dsyevr on the index range 1..na - the same
    // tridiagonalisation, a third of the vectors - was measured: 3.3 ms per 240 x 240 problem with SciPy's OpenBLAS against
    // 1.45 ms for the full dsyevd; not used)
    if (!eigh_lowest(la, G, na, E, Z1)) {
        ds::set_error("rr_step: dsyevd failed in the Rayleigh-Ritz step");
        return false;
    }
    Mat Tm = gemm(la, Z1, false, Z1.block(0, 0, na, na), true);  // Z1 Z1[:na]^T
    for (double& v : Tm.a) v = -v;
    for (int i = 0; i < na; ++i) Tm(i, i) += 1.0;
    if (!orthonormal_columns(la, Tm, Zp)) {  // rank-deficient P block: clamped-eigenvalue basis instead
        Mat GT = gemm(la, Tm, true, Tm, false), Tq;
        if (!svqb_transform(la, GT, Tq)) {
            ds::set_error("rr_step: dsyevd failed on the P block");
            return false;
        }
        Zp = gemm(la, Tm, false, Tq, false);
    }
    return true;
}

Mat next_projected_K(const ds_lapack_t& la, const Mat& G, const std::vector<double>& E, const Mat& Z1, const Mat& Zp) {
    const int na = Z1.c;
    const Mat GZp = gemm(la, G, false, Zp, false);
    const Mat Gxz = gemm(la, Z1, true, GZp, false), Gpp = gemm(la, Zp, true, GZp, false);
    Mat Gxp(2 * na, 2 * na);
    for (int i = 0; i < na; ++i) Gxp(i, i) = E[i];
    Gxp.set_block(0, na, Gxz);
    Gxp.set_block_T(na, 0, Gxz);
    Gxp.set_block(na, na, Gpp);
    symmetrize(Gxp);
    return Gxp;
}

Mat raw_update_coefficients(const ds_lapack_t& la, const Mat& Qw, const Mat& ZZ, int ny, int ncl, int nxp, int na) {
    Mat Zr = gemm(la, Qw, false, ZZ.block(nxp, 0, na, 2 * na), false);  // Qw Z_w ...
    for (int i = 0; i < nxp; ++i)                                        // ... + E Z_xp
        for (int j = 0; j < 2 * na; ++j) Zr(ny + ncl + i, j) += ZZ(i, j);
    return Zr;
}

}  // namespace ds::dense

using namespace ds::dense;

namespace {
Mat from_rows(const double* src, int rows, int cols) {
    Mat M(rows, cols);
    std::copy(src, src + M.a.size(), M.a.begin());
    return M;
}
void to_rows(const Mat& M, double* dst) { std::copy(M.a.begin(), M.a.end(), dst); }
}  // namespace

// Self-check of the leaf routines on a seeded random symmetric positive definite matrix (errs: include/diffsound_hip.h)
extern "C" int ds_selftest_dense(const ds_lapack_t* lapack, int n, int m, unsigned seed, double* errs) {
    DS_REQUIRE(lapack && lapack->dsyevd && lapack->dgemm && errs && n >= 2 && m >= 1 && m <= n, "ds_selftest_dense: bad arguments");
    unsigned long long st = seed * 2654435761ull + 12345ull;
    auto rnd = [&]() {
        st = st * 6364136223846793005ull + 1442695040888963407ull;
        return ((st >> 11) & ((1ull << 53) - 1)) / double(1ull << 53) - 0.5;
    };
    Mat B(n, n);
    for (double& v : B.a) v = rnd();
    Mat G = gemm(*lapack, B, false, B, true);
    for (int i = 0; i < n; ++i) G(i, i) += 0.05 * (i + 1);
    symmetrize(G);
    double gmax = 0.0;
    for (double v : G.a) gmax = std::max(gmax, std::fabs(v));
    std::vector<double> w, wf;
    Mat Zm, Zf;
    if (!eigh_lowest(*lapack, G, m, w, Zm) || !eigh(*lapack, G, wf, Zf)) {
        ds::set_error("ds_selftest_dense: LAPACK reported failure");
        return DS_ERR_ARG;
    }
    errs[0] = errs[1] = errs[2] = errs[3] = errs[4] = 0.0;
    for (int j = 0; j < n; ++j) errs[0] = std::max(errs[0], std::fabs(w[j] - wf[j]) / std::fabs(wf[n - 1]));
    const Mat GZ = gemm(*lapack, G, false, Zm, false);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < m; ++j) errs[1] = std::max(errs[1], std::fabs(GZ(i, j) - Zm(i, j) * w[j]) / gmax);
    Mat L;
    if (!cholesky(G, L)) {
        ds::set_error("ds_selftest_dense: Cholesky broke down on a positive definite matrix");
        return DS_ERR_ARG;
    }
    const Mat LLt = gemm(*lapack, L, false, L, true);
    for (size_t i = 0; i < G.a.size(); ++i) errs[2] = std::max(errs[2], std::fabs(LLt.a[i] - G.a[i]) / gmax);
    const Mat Li = lower_inverse(L), I1 = gemm(*lapack, Li, false, L, false);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) errs[3] = std::max(errs[3], std::fabs(I1(i, j) - (i == j ? 1.0 : 0.0)));
    Mat Tm(n, m), Q;
    for (double& v : Tm.a) v = rnd();
    if (!orthonormal_columns(*lapack, Tm, Q)) {
        ds::set_error("ds_selftest_dense: orthonormal_columns broke down");
        return DS_ERR_ARG;
    }
    const Mat QtQ = gemm(*lapack, Q, true, Q, false);
    for (int i = 0; i < m; ++i)
        for (int j = 0; j < m; ++j) errs[4] = std::max(errs[4], std::fabs(QtQ(i, j) - (i == j ? 1.0 : 0.0)));
    errs[5] = (lapack->dsytrd && lapack->dstedc && lapack->dormtr && m < n && n >= 32) ? 1.0 : 0.0;
    return DS_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Dense steps as pure host entry points with the caller's LAPACK table (arguments: include/diffsound_hip.h); the CPU test suite
// checks them against the Python forms (modal_solver.py: `_start_block_transform`, `small` in ModalSolver._polish; dense.py:
// `_raw_basis_transform`, `_rr_step`).  The first two frame the native loop - the Python solver calls them, one call instead of
// ~30 torch calls on tiny CPU tensors each; the last two are the loop's own steps, exported to be tested.
extern "C" int ds_host_start_block(const ds_lapack_t* lapack, const double* Gin, int ny, int b, double ortho_tol, double eps,
                                   double* lam, double* coef, double* cx, double* amp_out, int* route) {
    DS_REQUIRE(lapack && lapack->dsyevd && lapack->dgemm && Gin && lam && coef && cx && amp_out && route && ny >= 0 && b > 0,
               "ds_host_start_block: bad arguments");
    const ds_lapack_t& la = *lapack;
    *route = 1;
    const Mat G = from_rows(Gin, ny + b, 2 * b);
    const Mat Gyk = G.block(0, 0, ny, b), Cy = G.block(0, b, ny, b);
    Mat A = G.block(ny, 0, b, b), B0 = G.block(ny, b, b, b);
    symmetrize(A), symmetrize(B0);
    Mat T, CtC;
    double amp = 0.0;
    switch (project_in_coefficients(la, Cy, B0, false, T, CtC, amp)) {
        case Projected::BrokeDown: return DS_OK;
        case Projected::LapackFailed:
            ds::set_error("ds_host_start_block: dsyevd failed in the orthonormalisation");
            return DS_ERR_ARG;
        case Projected::Ok: break;
    }
    if (!(ortho_tol > 0.0 && eps * amp < ortho_tol)) return DS_OK;  // (one sweep would leave eps * amp: the explicit route repairs it)
    Mat A1 = A;
    if (ny) {
        const Mat CtG = gemm(la, Cy, true, Gyk, false);
        for (int i = 0; i < b; ++i)
            for (int j = 0; j < b; ++j) A1(i, j) -= CtG(i, j) + CtG(j, i);
    }
    Mat H = gemm(la, gemm(la, T, true, A1, false), false, T, false);
    symmetrize(H);
    std::vector<double> E;
    Mat Z;
    if (!eigh(la, H, E, Z)) {
        ds::set_error("ds_host_start_block: dsyevd failed in the first Ritz step");
        return DS_ERR_ARG;
    }
    const Mat Cx = gemm(la, T, false, Z, false);
    Mat CyCx = ny ? gemm(la, Cy, false, Cx, false) : Mat(0, b);
    for (double& v : CyCx.a) v = -v;
    Mat Coef(ny + b, b);
    Coef.set_block(0, 0, CyCx);
    Coef.set_block(ny, 0, Cx);
    std::copy(E.begin(), E.begin() + b, lam);
    to_rows(Coef, coef);
    to_rows(Cx, cx);
    *amp_out = amp;
    *route = 0;
    return DS_OK;
}

// fp64 polish of a converged block: the generalised Ritz problem (sum c_i GK_i) z = e GM z through the Cholesky factor of GM and
// the quadratic forms of the k wanted vectors.  DS_ERR_ARG with a message when GM is not positive definite.
extern "C" int ds_host_polish(const ds_lapack_t* lapack, int nterms, const double* GK, const double* coefs, const double* GMin, int b, int k,
                              double* Eout, double* Cout, double* qs) {
    DS_REQUIRE(lapack && lapack->dsyevd && lapack->dgemm && GK && coefs && GMin && Eout && Cout && qs && nterms >= 1 && b > 0 && k > 0 && k <= b,
               "ds_host_polish: bad arguments");
    const ds_lapack_t& la = *lapack;
    Mat GA(b, b), GB = from_rows(GMin, b, b);
    for (int t = 0; t < nterms; ++t)
        for (size_t i = 0; i < GA.a.size(); ++i) GA.a[i] += coefs[t] * GK[(size_t)t * b * b + i];
    symmetrize(GA), symmetrize(GB);
    Mat L;
    if (!cholesky(GB, L)) {
        ds::set_error("ds_host_polish: X^T M X of the converged block is not positive definite");
        return DS_ERR_ARG;
    }
    const Mat Li = lower_inverse(L);
    Mat H = gemm(la, gemm(la, Li, false, GA, false), false, Li, true);
    symmetrize(H);
    std::vector<double> E;
    Mat Zt;
    if (!eigh(la, H, E, Zt)) {
        ds::set_error("ds_host_polish: dsyevd failed");
        return DS_ERR_ARG;
    }
    const Mat C = gemm(la, Li, true, Zt, false);
    std::copy(E.begin(), E.begin() + k, Eout);
    to_rows(C, Cout);
    const Mat Ck = C.block(0, 0, b, k);
    for (int t = 0; t <= nterms; ++t) {
        Mat Gt = GB;
        if (t < nterms) {
            Gt = from_rows(GK + (size_t)t * b * b, b, b);
            symmetrize(Gt);
        }
        const Mat GC = gemm(la, Gt, false, Ck, false);
        for (int j = 0; j < k; ++j) {
            double sacc = 0.0;
            for (int i = 0; i < b; ++i) sacc += Ck(i, j) * GC(i, j);
            qs[(size_t)t * k + j] = sacc;
        }
    }
    return DS_OK;
}

extern "C" int ds_host_raw_basis(const ds_lapack_t* lapack, const double* GG, const double* Gxp, const double* lam_locked, int ny,
                                 int ncl, int nxp, int na, double ortho_tol, double eps, double* G_out, double* Qw_out, int* route) {
    DS_REQUIRE(lapack && lapack->dsyevd && lapack->dgemm && GG && Gxp && (lam_locked || ncl == 0) && G_out && Qw_out && route &&
                   ny >= 0 && ncl >= 0 && na > 0 && nxp >= na,
               "ds_host_raw_basis: bad arguments");
    Mat G, Qw;
    *route = 1;
    if (!raw_basis_transform(*lapack, from_rows(GG, ny + ncl + nxp + na, 2 * na), from_rows(Gxp, nxp, nxp), lam_locked, ny, ncl, nxp,
                             na, ortho_tol, eps, G, Qw))
        return DS_OK;
    to_rows(G, G_out);
    to_rows(Qw, Qw_out);
    *route = 0;
    return DS_OK;
}

extern "C" int ds_host_rr_step(const ds_lapack_t* lapack, const double* Gin, int sz, int na, double* E_out, double* Z1_out,
                               double* Zp_out) {
    DS_REQUIRE(lapack && lapack->dsyevd && lapack->dgemm && Gin && E_out && Z1_out && Zp_out && na > 0 && sz >= 2 * na,
               "ds_host_rr_step: bad arguments");
    DS_REQUIRE((!lapack->dsytrd) == (!lapack->dstedc) && (!lapack->dsytrd) == (!lapack->dormtr),
               "ds_host_rr_step: the staged eigensolver needs dsytrd, dstedc and dormtr together (or none of them)");
    Mat G = from_rows(Gin, sz, sz), Z1, Zp;
    std::vector<double> E;
    if (!rr_step(*lapack, G, na, E, Z1, Zp)) return DS_ERR_ARG;
    std::copy(E.begin(), E.begin() + na, E_out);
    to_rows(Z1, Z1_out);
    to_rows(Zp, Zp_out);
    return DS_OK;
}
