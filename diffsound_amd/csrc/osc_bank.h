// Host side of the recursive-resonator banks (osc_driven.hip, osc_slide.hip, osc_listen.hip): the workspace they share, the
// argument checks they have in common, the passes that do not depend on the bank, and the order of the backward's launches.
#pragma once

#include <cstdint>

#include "ds_common.h"
#include "osc_scan.h"

namespace osc_bank {

inline int64_t ntiles_of(int S) { return ds::ceil_div(S, osc_scan::TILE); }

// the state entering every tile of every (clip, mode), then one partial of G per (clip, mode)
inline int64_t workspace_bytes(int A, int m, int S) {
    return (int64_t)sizeof(double2) * ((int64_t)A * m * ntiles_of(S) + (int64_t)A * m);
}

// The checks the entry points have in common behind "null pointer" and "empty problem"; `fn` names the entry point.  Their
// order: clips, (the listener's channels,) frames where the bank has them, workspace.
inline int check_clips(const char* fn, int A) {
    DS_REQUIRE(A <= 65535, "%s: A = %d above 65535", fn, A);
    return DS_OK;
}

inline int check_frames(const char* fn, int hop, double sr) {
    DS_REQUIRE(hop > 0 && hop % DS_OSC_SCAN_RUN == 0, "%s: hop = %d is not a positive multiple of %d", fn, hop,
               DS_OSC_SCAN_RUN);
    DS_REQUIRE(sr > 0, "%s: sr = %g is not positive", fn, sr);
    return DS_OK;
}

// `need`: the entry point's ds_osc_*_workspace_bytes
inline int check_work(const char* fn, const void* work, int64_t work_bytes, int64_t need) {
    DS_REQUIRE(work_bytes >= need, "%s: workspace of %lld bytes, %lld needed", fn, (long long)work_bytes, (long long)need);
    DS_REQUIRE(ds::aligned(work, 16), "%s: work not 16-byte aligned", fn);
    return DS_OK;
}

// The passes that are the same kernel in every bank (osc_driven.hip).  Each returns DS_OK or the launch's error.
// the boundary pass under a real row: in (A x ldin), zero from nin on; rev: time runs down (the adjoint on gy)
int launch_boundary(hipStream_t st, bool rev, const double* d, const double* w, const float* in, int ldin, int nin, int A, int m,
                    int nt, double inv_sr, double2* bnd);
// gd[mm] = -Im sum_a gpart / sr, gw[mm] = Re sum_a gpart / sr, the clips added in order
int launch_reduce(hipStream_t st, const double2* gpart, int A, int m, double inv_sr, double* gd, double* gw);
// gforce[a, j] = 0 for S <= j < F: taps that no output sample hears
int launch_zero_tail(hipStream_t st, float* gforce, int A, int F, int S);

// The backward's launches in their order: boundary(nt, lbnd) scans the adjoint's drive downwards, tile(nt, lbnd) writes gforce
// below min(F, S), mode(nt, lbnd, gpart) leaves the per-clip partials that the reduce adds.  Each returns DS_OK or an error.
template <class Boundary, class Tile, class Mode>
int backward(hipStream_t st, int A, int m, int F, int S, double inv_sr, void* work, double* gd, double* gw, float* gforce,
             Boundary boundary, Tile tile, Mode mode) {
    const int nt = (int)ntiles_of(S);
    double2* lbnd = static_cast<double2*>(work);
    double2* gpart = lbnd + (int64_t)A * m * nt;
    if (int rc = boundary(nt, lbnd)) return rc;
    if (gforce) {
        if (int rc = tile(nt, lbnd)) return rc;
        if (F > S)
            if (int rc = launch_zero_tail(st, gforce, A, F, S)) return rc;
    }
    if (int rc = mode(nt, lbnd, gpart)) return rc;
    return launch_reduce(st, gpart, A, m, inv_sr, gd, gw);
}

}  // namespace osc_bank
