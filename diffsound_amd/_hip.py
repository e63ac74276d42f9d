"""ctypes binding of libdiffsound_hip.so (the C ABI declared in include/diffsound_hip.h).

There is NO fallback: if the library is missing or a call fails, a RuntimeError is raised
(the reference's native op surfaces errors the same way, as RuntimeError through pybind:
reference src/include/macro.h:75-83).  Tensors are passed as raw ``data_ptr()`` values and the
kernels are enqueued on torch's current HIP stream.
"""
import ctypes
import threading
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DS_EXP_LIB") or os.path.join(_HERE, "csrc", "libdiffsound_hip.so")  # (DS_EXP_LIB: A/B builds, experiments)
ABI_VERSION = 45  # DS_ABI_VERSION of include/diffsound_hip.h

c_i32p = ctypes.POINTER(ctypes.c_int32)
_P = ctypes.c_void_p
_I64 = ctypes.c_int64
_I = ctypes.c_int
_D = ctypes.c_double
_F = ctypes.c_float


class MtCounts(ctypes.Structure):
    """ds_mt_counts_t of include/diffsound_hip.h."""
    _fields_ = [("n_used", _I64), ("n_cross", _I64), ("n_side1", _I64), ("n_side3", _I64), ("n_inner", _I64),
                ("n_face1", _I64), ("n_face2", _I64), ("reserved", _I64)]


class Block64(ctypes.Structure):
    """ds_block64_t of include/diffsound_hip.h."""
    _fields_ = [("a", _P), ("lda", _I64), ("p", ctypes.c_int32), ("offset", ctypes.c_int32)]


class LevelDesc(ctypes.Structure):
    """ds_level_t of include/diffsound_hip.h."""
    _fields_ = [("utab", _P), ("ctab", _P), ("ngroups", _I64), ("cap_blocks", ctypes.c_int32),
                ("degree", ctypes.c_int32), ("gent", _P), ("kgrp", _P), ("nnzb", _I64), ("nv", _I64), ("dinv", _P),
                ("lmax", _D), ("lmin", _D), ("mf_group_nodes", ctypes.c_int32), ("mf_max_entries", ctypes.c_int32),
                ("mf_max_batch_blocks", ctypes.c_int32), ("level_tag", ctypes.c_int32),
                ("mf_gptr", _P), ("mf_gcol", _P), ("mf_gmeta", _P), ("mf_gbase", _P), ("mf_ghead", _P), ("mf_kc", _P),
                ("m32_max_entries", ctypes.c_int32), ("m32_max_batch_blocks", ctypes.c_int32),
                ("m32_gptr", _P), ("m32_gcol", _P), ("m32_gmeta", _P), ("m32_gbase", _P), ("m32_k", _P), ("m32_m", _P),
                ("tgrp", _P), ("mf_nblocks", _I64)]


class TwoLevelDesc(ctypes.Structure):
    """ds_twolevel_t of include/diffsound_hip.h."""
    _fields_ = [("fine", LevelDesc), ("coarse", LevelDesc), ("rptr", _P), ("rcol", _P), ("rw", _P), ("pptr", _P),
                ("pcol", _P), ("pw", _P), ("R", _P), ("ldr", _I64), ("W", _P), ("ldw", _I64), ("D", _P), ("ldd", _I64),
                ("AD", _P), ("lda", _I64), ("Rr", _P), ("ldrr", _I64), ("Rc", _P), ("Ec", _P), ("Dc", _P), ("ADc", _P),
                ("ldc", _I64), ("ncols", ctypes.c_int32), ("Wc", _P), ("ldwc", _I64), ("storage", ctypes.c_int32),
                ("R16", _P), ("ldr16", _I64)]


TL_BF16, TL_PREPARED, TL_OWN_INIT = 1, 2, 4  # DS_TL_* of include/diffsound_hip.h: the flags of ds_twolevel_t.storage


class LapackTable(ctypes.Structure):
    """ds_lapack_t: Fortran-convention dsyevd / dgemm entry points, and (ABI 31, optional) the stages of dsyevd."""
    _fields_ = [("dsyevd", _P), ("dgemm", _P), ("dsytrd", _P), ("dstedc", _P), ("dormtr", _P)]


class LobpcgDesc(ctypes.Structure):
    """ds_lobpcg_t of include/diffsound_hip.h."""
    _i32 = ctypes.c_int32
    _fields_ = [("n", _I64), ("nv", _I64), ("b", _i32), ("k", _i32), ("ny", _i32), ("maxit", _i32), ("lock", _i32),
                ("ortho_passes", _i32), ("rr_refresh", _i32), ("gram_exact", _i32), ("kx_fresh", _i32), ("raw_rr", _i32),
                ("tol", _D), ("ortho_tol", _D),
                ("A_norm", _D), ("B_norm", _D), ("S", _P), ("S2", _P), ("KS", _P), ("KS2", _P), ("R", _P), ("MX", _P),
                ("MW", _P), ("lds", _I64), ("ldks", _I64), ("ldr", _I64), ("level", LevelDesc), ("mgrp", _P),
                ("rowptr", _P), ("colidx", _P), ("k32", _P), ("k32t", _P), ("twolevel", ctypes.POINTER(TwoLevelDesc)),
                ("pa", _P), ("pb", _P), ("ldp", _I64), ("pr16", _P), ("gbuf", _P), ("cbuf", _P), ("nrm", _P), ("lam_dev", _P),
                ("res_work", _P), ("res_work_bytes", _I64), ("gram_work", _P), ("gram_work_bytes", _I64), ("lam", ctypes.POINTER(_D)), ("rerr", ctypes.POINTER(_D)),
                ("history", ctypes.POINTER(_D)), ("history_cap", _i32), ("iterations", _i32), ("result_in_s2", _i32),
                ("wait_mode", _i32), ("ritz_tol", ctypes.c_double)]


_LEVEL, _TWOLEVEL, _LOBPCG, _LAPACK = (ctypes.POINTER(t) for t in (LevelDesc, TwoLevelDesc, LobpcgDesc, LapackTable))

# Every entry point of the header, by translation unit in the header's order: (result, arguments).  A new one goes HERE.
_SIGNATURES = {
    "ds_last_error": (ctypes.c_char_p, []),
    "ds_abi_version": (_I, []),
    # symbolic phase: pattern.cpp (host), dpattern.hip (device)
    "ds_pattern_build": (_I, [_P, _I64, _I, _I64, _I, ctypes.POINTER(_P)]),
    "ds_pattern_sizes": (_I, [_P, ctypes.POINTER(_I64), ctypes.POINTER(_I64), ctypes.POINTER(_I64)]),
    "ds_pattern_export": (_I, [_P, _P, _P, _P, _P, _P]),
    "ds_pattern_free": (None, [_P]),
    "ds_groups_build": (_I, [_P, _P, _I64, ctypes.POINTER(_P)]),
    "ds_groups_sizes": (_I, [_P, ctypes.POINTER(_I64), ctypes.POINTER(_I64)]),
    "ds_groups_export": (_I, [_P, _P, _P, _P, _P]),
    "ds_groups_free": (None, [_P]),
    "ds_dpattern_build": (_I, [_P, _I64, _I, _I64, _I, _P, ctypes.POINTER(_P)]),
    "ds_dpattern_sizes": (_I, [_P, ctypes.POINTER(_I64), ctypes.POINTER(_I64), ctypes.POINTER(_I64), ctypes.POINTER(_I64),
                               ctypes.POINTER(_I64)]),
    "ds_dpattern_export": (_I, [_P] * 13),
    "ds_dpattern_free": (None, [_P]),
    "ds_edge_table": (_I, [_P, _I64, _I64, _P, _P, _P, ctypes.POINTER(_I64), _P]),
    "ds_unique_rows3": (_I, [_P, _I64, _P, _P, ctypes.POINTER(_I64), _P]),
    # numeric assembly: assemble.hip
    "ds_assemble_kml": (_I, [_P, _P, _I64, _I, _I64, _P, _P, _I64, _P, _P, _P, _P, _P, _P, _P]),
    "ds_combine_material": (_I, [_P, _P, _P, _I64, _P, _I64, _D, _D, _P, _P, _P, _P, _P]),
    # block SpMM: spmm.hip
    "ds_spmm_bsr3": (_I, [_I, _P, _P, _P, _P, _I64, _P, _I64, _P, _I64, _I, _P]),
    # tall-skinny Gram: gram.hip
    "ds_gram_workspace_bytes": (_I64, [_I64, _I, _I]),
    "ds_gram": (_I, [_P, _I, _I64, _I, _P, _I, _I64, _I, _I64, _I, _P, _P, _I64, _P]),
    # fused block-vector updates: blockops.hip, spmm.hip, transfer.hip, spmm_f64.hip, spmm_union.hip
    "ds_residual": (_I, [_P, _I64, _P, _I64, _P, _I64, _P, _I64, _P, _I64, _I, _P, _P, _P]),
    "ds_cheb_init": (_I, [_P, _I64, _P, _I64, _P, _I64, _P, _I64, _I, _F, _P]),
    "ds_cheb_step": (_I, [_P, _I64, _P, _I64, _P, _I64, _P, _I64, _P, _I64, _I, _F, _F, _P]),
    "ds_cheb_spmm": (_I, [_P, _P, _P, _I64, _P, _I64, _P, _I64, _P, _I64, _P, _I, _F, _F, _I, _P]),
    "ds_spmm_residual": (_I, [_P, _P, _P, _I64, _P, _I64, _P, _I64, _P, _I64, _I, _P]),
    "ds_scalar_csr_spmm": (_I, [_P, _P, _P, _I64, _P, _I64, _P, _I64, _I, _F, _P]),
    "ds_spmm_f64_polish": (_I, [_P, _P, _P, _P, _P, _I64, _P, _I64, _P, _P, _P, _I64, _I, _P]),
    "ds_spmm_f64_union": (_I, [_I, _I, _P, _P, _I64, _I, _P, _P, _I64, _I64, _P, _I64, _P, _I64, _I, _P]),
    "ds_spmm_f64_polish_f32out": (_I, [_P, _P, _P, _P, _P, _I64, _P, _I64, _P, _P, _P, _I64, _I, _P]),
    "ds_pack_groups": (_I, [_P, _P, _I64, _P, _P]),
    "ds_spmm_union": (_I, [_I, _I, _P, _P, _I64, _I, _P, _P, _I64, _I64, _P, _I64, _P, _I64, _P, _I64, _P, _I, _F, _F, _I, _P,
                          _I64, _P]),
    "ds_union_residual_workspace_bytes": (_I64, [_I64, _I]),
    "ds_union_residual": (_I, [_I, _P, _P, _I64, _I, _P, _P, _P, _I64, _I64, _P, _I64, _P, _P, _I64, _I, _P, _I64, _P, _P, _P]),
    "ds_union_residual_pre": (_I, [_I, _P, _P, _I64, _I, _P, _P, _P, _I64, _I64, _P, _I64, _P, _P, _F, _P, _I64, _P, _I64, _I, _P,
                                   _I64, _P, _P, _P]),
    "ds_spmm_union_narrow": (_I, [_I, _I, _P, _P, _I64, _P, _P, _I64, _I64, _P, _I64, _P, _I64, _I, _P]),
    "ds_spmm_union_km": (_I, [_I, _P, _P, _I64, _I, _P, _P, _P, _I64, _I64, _P, _I64, _P, _I64, _P, _I64, _I, _P]),
    # two-level cycle and its bf16 kernels: vcycle.cpp, spmm_union.hip, spmm_mfma.hip, spmm_mfma32.hip, precond16.hip
    "ds_twolevel_apply": (_I, [_TWOLEVEL, _P]),
    "ds_chebyshev_apply": (_I, [_LEVEL, _P, _I64, _P, _I64, _P, _P, _I64, _I, _P]),
    "ds_chebyshev_apply16": (_I, [_LEVEL, _P, _I64, _P, _I64, _P, _P, _P, _I64, _I, _P]),
    "ds_spmm_union16": (_I, [_I, _P, _P, _I64, _I, _P, _P, _I64, _I64, _P, _I64, _P, _I64, _I, _P, _I64, _P, _I, _F,
                            _F, _I, _P, _I64, _P]),
    "ds_pack_kc": (_I, [_P, _P, _I64, _P, _P]),
    "ds_group_inverse": (_I, [_P, _P, _P, _I64, _I, _P, _P]),
    "ds_group_pack_kc": (_I, [_P, _P, _P, _P, _P, _P, _I, _I64, _P, _P]),
    "ds_group_apply16": (_I, [_P, _I, _P, _I, _I64, _P, _I, _I64, _I64, _I, _P]),
    "ds_spmm_union16m": (_I, [_I, _I, _I, _P, _P, _P, _P, _P, _P, _I64, _I64, _I, _I, _I64, _P, _I64, _P, _I64, _I, _P, _I64, _P, _I, _F,
                              _F, _I, _P, _I64, _P]),
    "ds_spmm_union32m": (_I, [_I, _I, _P, _P, _P, _P, _P, _I64, _I64, _I64, _I, _I, _I64, _P, _I64, _P, _I64, _I, _P]),
    "ds_cheb_init16": (_I, [_P, _I, _I64, _P, _I64, _P, _I64, _P, _I64, _I, _F, _P]),
    "ds_scalar_csr_spmm16": (_I, [_P, _P, _P, _I64, _P, _I64, _P, _I64, _I, _F, _P]),
    # the native iteration and its steps: lobpcg.cpp, host_dense.cpp, blockops.hip, refine64.hip, gram.hip, mix64.hip
    "ds_lobpcg_iterate": (_I, [_LOBPCG, _LAPACK, _P]),
    "ds_selftest_dense": (_I, [_LAPACK, _I, _I, ctypes.c_uint, ctypes.POINTER(_D)]),
    "ds_host_start_block": (_I, [_LAPACK, _P, _I, _I, _D, _D, _P, _P, _P, ctypes.POINTER(_D), ctypes.POINTER(_I)]),
    "ds_host_polish": (_I, [_LAPACK, _I, _P, _P, _P, _I, _I, _P, _P, _P]),
    "ds_host_raw_basis": (_I, [_LAPACK, _P, _P, _P, _I, _I, _I, _I, _D, _D, _P, _P, ctypes.POINTER(_I)]),
    "ds_host_rr_step": (_I, [_LAPACK, _P, _I, _I, _P, _P, _P]),
    "ds_host_wait_mode": (_I, [_I]),
    "ds_mix": (_I, [_P, _I64, _I, _P, _I, _P, _I64, _I64, _F, _F, _P]),
    "ds_residual64_workspace_doubles": (_I64, [_I]),
    "ds_residual64_norms": (_I, [_P, _I64, _P, _I64, _P, _I64, _P, _I64, _I, _P, _I64, _P, _P, _P]),
    "ds_residual64_scaled": (_I, [_P, _I64, _P, _I64, _P, _P, _P, _I, _P, _I64, _I64, _P]),
    "ds_gram64_blocks": (_I, [_I, _P, _I, _P, _I64, _I, _P, _P, _I64, _P]),
    "ds_mix64": (_I, [_I, _P, _P, _I64, _I, _P, _I64, _I64, _D, _D, _P]),
    # geometry backward: geomgrad.hip
    "ds_geometry_grad": (_I, [_P, _I64, _I, _I64, _P, _P, _I64, _I, _P, _P, _D, _D, _P, _P, _I, _P, _P, _P]),
    "ds_geometry_grad_tangent": (_I, [_P, _I64, _I, _I64, _P, _P, _I64, _I, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P, _P]),
    # oscillator family and the pass's read-out: oscillator.hip, readout.hip, osc_driven.hip
    "ds_osc_bank_fwd": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _D, _P, _P]),
    "ds_osc_bank_bwd": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _D, _P, _P, _P, _P, _P]),
    "ds_readout_pass": (_I, [_P, _P, _P, _P, _I, _D, _D, _D, _D, _D, _D, _D, _D, _P, _I, _I, _D, _P, _I, _P, _P, _P, _P, _P, _P]),
    "ds_osc_tv_workspace_floats": (_I64, [_I, _I, _I]),
    "ds_osc_tv_fwd": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _D, _P, _P, _P]),
    "ds_osc_tv_bwd": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _D, _P, _P, _P, _P, _P]),
    "ds_osc_driven_workspace_bytes": (_I64, [_I, _I, _I]),
    "ds_osc_driven_fwd": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _D, _P, _I64, _P, _P]),
    "ds_osc_driven_bwd": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _D, _P, _I64, _P, _P, _P, _P, _P]),
    # sliding contact: osc_slide.hip
    "ds_osc_slide_workspace_bytes": (_I64, [_I, _I, _I, _I, _I]),
    "ds_osc_slide_fwd": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _D, _P, _I64, _P, _P]),
    "ds_osc_slide_bwd": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _D, _P, _I64, _P, _P, _P, _P, _P, _P]),
    # listener bank: osc_listen.hip
    "ds_osc_listen_workspace_bytes": (_I64, [_I, _I, _I, _I, _I, _I]),
    "ds_osc_listen_fwd": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _D, _P, _I64, _P, _P]),
    "ds_osc_listen_bwd": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _D, _P, _I64, _P, _P, _P, _P, _P, _P]),
    # propagation delay: delay.hip
    "ds_delay_workspace_bytes": (_I64, [_I, _I, _I, _I]),
    "ds_delay_fwd": (_I, [_P, _P, _I, _I, _I, _I, _P, _P]),
    "ds_delay_bwd": (_I, [_P, _P, _P, _I, _I, _I, _I, _P, _I64, _P, _P, _P]),
    # recording chain: biquad.hip
    "ds_biquad_workspace_bytes": (_I64, [_I, _I, _I]),
    "ds_biquad_fwd": (_I, [_P, _P, _I, _I, _I, _I, _P, _P]),
    "ds_biquad_bwd": (_I, [_P, _P, _P, _I, _I, _I, _I, _P, _I64, _P, _P, _P]),
    # room response: fir.hip
    "ds_fir_workspace_bytes": (_I64, [_I, _I, _I, _I]),
    "ds_fir_fwd": (_I, [_P, _P, _I, _I, _I, _I, _P, _P]),
    "ds_fir_bwd": (_I, [_P, _P, _P, _I, _I, _I, _I, _P, _I64, _P, _P, _P]),
    # late reverberation: fdn.hip
    "ds_fdn_workspace_bytes": (_I64, [_I, _I, _I, _I]),
    "ds_fdn_fwd": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _P]),
    "ds_fdn_bwd": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _I64, _P, _P, _P, _P, _P, _P, _P]),
    # Hertz hammer coupled to the modes: contact.hip
    "ds_contact_workspace_bytes": (_I64, [_I, _I, _I, _I]),
    "ds_contact_fwd": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _D, _D, _P, _P]),
    "ds_contact_bwd": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _D, _D, _P, _I64, _P, _P, _P, _P, _P, _P, _P]),
    # friction exciter coupled to the modes: friction.hip
    "ds_friction_workspace_bytes": (_I64, [_I, _I, _I, _I]),
    "ds_friction_fwd": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _D, _P, _P]),
    "ds_friction_bwd": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _D, _P, _I64, _P, _P, _P, _P, _P, _P, _P]),
    # tension-modulated modal bank: nlbank.hip
    "ds_nlbank_workspace_bytes": (_I64, [_I, _I, _I, _I, _I]),
    "ds_nlbank_fwd": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _D, _P, _P]),
    "ds_nlbank_bwd": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _D, _P, _I64, _P, _P, _P, _P, _P, _P, _P, _P]),
    # filtered noise: filtered_noise.hip
    "ds_filtered_noise_fwd": (_I, [_P, _P, _I, _I, _I, _I, _D, _P, _P]),
    "ds_filtered_noise_bwd": (_I, [_P, _P, _P, _I, _I, _I, _I, _D, _P, _P]),
    # spectral loss head: stft.hip, specpoints.hip
    "ds_stft_power": (_I, [_P, _I, _I, _I, _I, _P, _P, _P, _P]),
    "ds_spec_loss": (_I, [_I, _P, _P, _I, _I, _I, _F, _F, _I, _P, _P, _P]),
    "ds_stft_power_bwd": (_I, [_P, _P, _P, _I, _I, _I, _I, _F, _P, _P, _P]),
    "ds_spec_points_fwd": (_I, [_P, _I, _I, _I, _F, _I, _P, _I64, _I, _P, _P, _P, _P]),
    "ds_spec_points_bwd": (_I, [_P, _P, _I, _I, _I, _P, _I64, _I, _P, _D, _P, _P]),
    # kernel timing and the bandwidth probe: profile.cpp, stream.hip
    "ds_profile_stream": (_I, [_P, _I64]),
    "ds_profile_kinds": (_I, [ctypes.c_uint]),
    "ds_profile_collect": (_I64, [_P, _P, _P, _P, _P, _I64]),
    "ds_stream_triad": (_I, [_P, _P, _P, _I64, _F, _P]),
    # boundary elements: bem.hip
    "ds_bem_geometry": (_I, [_P, _I64, _P, _I64, _P, _P]),
    "ds_bem_assemble_workspace_bytes": (_I64, [_I64]),
    "ds_bem_assemble": (_I, [_P, _I64, _F, _P, _P, _I64, _P, _I64, _P, _P, _P]),
    "ds_bem_cgemv": (_I, [_P, _I64, _P, _I64, _P, _P, _P]),
    "ds_bem_potential": (_I, [_P, _I64, _F, _P, _P, _P, _I64, _P, _P]),
    # marching tetrahedra: dmtet.hip
    "ds_mt_count_workspace_bytes": (_I64, [_I64, _I64, _I64]),
    "ds_mt_count": (_I, [_P, _I64, _P, _I64, _P, _P, _I64, _P, _P, _P, _P, _P, _P, _I64, _P, _P]),
    "ds_mt_emit": (_I, [_P, _P, _I64, _P, _I64, _P, _P, _P, _I64, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "ds_mt_backward_workspace_floats": (_I64, [_I64]),
    "ds_mt_backward": (_I, [_P, _P, _P, _I64, _P, _P, _I64, _P, _P, _P, _P, _P, _P, _I64, _I64, _P, _P, _P, _P, _P]),
    # mesh signed distance: meshsdf.hip
    "ds_mesh_sdf_pack": (_I, [_P, _P, _I64, _I64, _P, _P]),
    "ds_mesh_sdf_workspace_bytes": (_I64, [_I64, _I64, _I]),
    "ds_mesh_sdf_query": (_I, [_P, _I64, _P, _I64, _P, _P, _P, _P, _P, _I64, _P]),
    # Sinkhorn divergence: sinkhorn.hip
    "ds_sinkhorn_workspace_floats": (_I64, [_I64, _I64, _I64]),
    "ds_sinkhorn_bbox": (_I, [_P, _P, _P, _P, _I64, _I64, _I64, _I64, _P, _P]),
    "ds_sinkhorn_loop": (_I, [_P, _P, _P, _P, _I64, _I64, _I64, _I64, _P, _I, _I, _P, _P]),
    "ds_sinkhorn_final": (_I, [_P, _P, _P, _P, _I64, _I64, _I64, _I64, _F, _I, _P, _P, _P]),
    "ds_sinkhorn_backward": (_I, [_P, _P, _P, _P, _I64, _I64, _I64, _I64, _F, _I, _P, _P, _P, _P, _P]),
    # deformation gradient and force gather: deform.hip
    "ds_deform_tables": (_I, [_P, _I64, _P, _I64, _I, _P, _P, _P, _P, _P, _P]),
    "ds_deform_gradient": (_I, [_P, _I64, _P, _I64, _I, _P, _P, _P, _I64, _I, _P, _P]),
    "ds_deform_force": (_I, [_P, _I64, _P, _I64, _I, _P, _P, _P, _P, _P, _I64, _I, _P, _P, _P]),
    # general tangents: tangent.hip
    "ds_combine_tangent": (_I, [_P, _P, _I64, _P, _I64, _P, _P, _P, _P, _P, _P, _P]),
    "ds_tangent_forms_workspace_bytes": (ctypes.c_size_t, [_I64, _I]),
    "ds_tangent_forms": (_I, [_P, _P, _P, _I64, _P, _I64, _I, _P, _P, ctypes.c_size_t, _P]),
    # mode shapes at points: modesample.hip
    "ds_mode_sample_fwd": (_I, [_P, _I64, _I, _I64, _P, _I64, _I, _P, _P, _P, _I64, _P, _P, _P]),
    "ds_mode_sample_bwd": (_I, [_P, _I64, _I, _I64, _P, _I64, _I, _P, _P, _P, _I64, _P, _P, _P, _P]),
    # multipole series of the modes' exterior fields at listener points: multipole.hip
    "ds_multipole_workspace_bytes": (_I64, [_I64, _I, _I]),
    "ds_multipole_fwd": (_I, [_P, _P, _P, _P, _I64, _I, _I, _P, _P]),
    "ds_multipole_bwd": (_I, [_P, _P, _P, _P, _P, _I64, _I, _I, _P, _I64, _P, _P, _P]),
}
EXPORTED_SYMBOLS = tuple(_SIGNATURES)

_lib = None


def lib():
    """Load (once) and return the ctypes handle; RuntimeError if the HIP extension is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"diffsound_amd: HIP extension {LIB_PATH} is missing - build it with "
                "`python -c 'import __graft_entry__ as g; g.build()'` or `make -C diffsound_amd/csrc`. "
                "There is no CPU fallback.")
        handle = ctypes.CDLL(LIB_PATH)
        handle.ds_abi_version.restype = _I
        got = handle.ds_abi_version()
        if got != ABI_VERSION:  # a stale build resolves every symbol and would be called with shifted arguments
            raise RuntimeError(f"diffsound_amd: {LIB_PATH} has ABI version {got}, this package needs {ABI_VERSION} - "
                               "rebuild it with `make -C diffsound_amd/csrc`")
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(handle, name)
            fn.restype = res
            fn.argtypes = args
        _lib = handle
    return _lib


def check(status, what):
    if status != 0:
        msg = lib().ds_last_error()
        raise RuntimeError(f"{what} failed (status {status}): {msg.decode() if msg else ''}")


def call(name, *args):
    """The entry point ``name`` with ``args`` as they stand (one that takes no stream); RuntimeError on a non-zero status."""
    check(getattr(lib(), name)(*args), name)


def launch(name, *args, device=None):
    """The entry point ``name`` with ``args`` and, last, the current stream.  ``device``: the launch runs with that device
    current and on its stream - every caller outside the operator layer passes its operands' device.  None: the calling
    thread's device as it is (the operator layer: its lane thread has set the device, and a guard per launch would cost
    what ``stream_ptr`` saves)."""
    if device is not None:
        with torch.cuda.device(device):  # (the stream below is then that device's)
            return launch(name, *args)
    status = getattr(lib(), name)(*args, stream_ptr())
    if status != 0:  # (tested here: the operator layer's success path does without one more Python call)
        check(status, name)


def workspace(name, *dims, device, dtype=torch.uint8):
    """(uninitialised tensor, count) for the query ``name`` (a ds_*_workspace_{bytes,floats,doubles}) of ``dims``: ``count``
    elements of ``dtype`` on ``device``."""
    count = getattr(lib(), name)(*dims)
    return torch.empty(count, dtype=dtype, device=device), count


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def stream_ptr():
    """The calling thread's current HIP stream as a pointer-sized int (ctypes converts it for the c_void_p slot).
    The raw-stream query is the one compiled-kernel launchers use: ~0.3 us against ~9 us for building a
    torch.cuda.Stream object on every launch (a pass makes ~1000 launches per lane, under the interpreter lock)."""
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    return None if t is None else t.data_ptr()


def require_gpu(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("diffsound_amd: tensors must live on the HIP device (no CPU fallback)")


_lapack = None


def lapack_table(source=None):
    """ds_lapack_t for ds_lobpcg_iterate: Fortran-convention dsyevd / dgemm entry points and, where the library has them, the
    stages dsytrd / dstedc / dormtr.  Sources, in order of preference (``source`` or the environment variable DS_LAPACK names
    one: "scipy" | "torch"):
      scipy  scipy.linalg.cython_lapack / cython_blas export every routine as a PyCapsule (OpenBLAS: dsyevd 240 x 240 in
             2.35 ms on the GPU box's host, and the stages, so the Ritz step back-transforms only the wanted third);
      torch  the MKL inside libtorch_cpu.so exports dsyevd_ / dgemm_ as plain symbols (2.9 ms; no stages) - so the product does
             not DEPEND on SciPy's private capsule table: without SciPy, or with a SciPy whose capsules have moved,
             the solve still runs, 20 % slower on the host side.
    The table changes nothing in the process: the BLAS thread count is the caller's business (``blas_one_thread`` below is what
    the native solve is wrapped in)."""
    global _lapack
    want = source or os.environ.get("DS_LAPACK") or None
    if want not in (None, "scipy", "torch"):
        raise ValueError(f"lapack_table: unknown source {want!r} (scipy | torch)")
    if _lapack is not None and (want is None or _lapack_source == want):
        return _lapack
    errors = []
    for name in ((want,) if want else ("scipy", "torch")):
        try:
            table = _lapack_from_scipy() if name == "scipy" else _lapack_from_torch()
        except Exception as ex:  # (ImportError, KeyError on a capsule, OSError / AttributeError on a symbol)
            errors.append(f"{name}: {type(ex).__name__}: {ex}")
            continue
        if want is None or _lapack is None:
            _set_lapack(table, name)
        return table
    raise RuntimeError("diffsound_amd: no LAPACK for the eigensolver's dense steps (" + "; ".join(errors) + ")")


_lapack_source = None


def _set_lapack(table, name):
    global _lapack, _lapack_source
    _lapack, _lapack_source = table, name


def lapack_source():
    """Which library the process-wide table came from ("scipy" | "torch"), None before the first call of lapack_table()."""
    return _lapack_source


def _lapack_from_scipy():
    import scipy.linalg.cython_blas as cb
    import scipy.linalg.cython_lapack as cl

    get = ctypes.pythonapi.PyCapsule_GetPointer
    name = ctypes.pythonapi.PyCapsule_GetName
    get.restype, get.argtypes = ctypes.c_void_p, [ctypes.py_object, ctypes.c_char_p]
    name.restype, name.argtypes = ctypes.c_char_p, [ctypes.py_object]
    addr = lambda cap: get(cap, name(cap))
    stages = [addr(cl.__pyx_capi__[nm]) if nm in cl.__pyx_capi__ else None for nm in ("dsytrd", "dstedc", "dormtr")]
    if not all(stages):
        stages = [None, None, None]
    return LapackTable(addr(cl.__pyx_capi__["dsyevd"]), addr(cb.__pyx_capi__["dgemm"]), *stages)


def _lapack_from_torch():
    lib = ctypes.CDLL(os.path.join(os.path.dirname(torch.__file__), "lib", "libtorch_cpu.so"))
    addr = lambda nm: ctypes.cast(getattr(lib, nm), ctypes.c_void_p).value
    stages = [None, None, None]
    try:
        stages = [addr(nm) for nm in ("dsytrd_", "dstedc_", "dormtr_")]
    except AttributeError:
        pass
    return LapackTable(addr("dsyevd_"), addr("dgemm_"), *stages)


class blas_one_thread:
    """The <= 3b x 3b problems of the native eigensolver loop are fastest on one BLAS thread and are solved by several
    hypothesis lanes at once.  Context manager, re-entrant across threads: the first solve that enters limits the BLAS
    behind SciPy to one thread (threadpoolctl), the last one that leaves restores what was there - nothing stays changed
    in the host process (round 2 left the limit in place for good, which also skewed the CPU baseline)."""

    _lock = threading.Lock()
    _depth = 0
    _ctl = None
    _controller = False  # threadpoolctl's view of the loaded BLAS libraries, built once (a scan of every loaded library:
                         # ~1 ms, too much to pay on every solve)

    def __enter__(self):
        cls = blas_one_thread
        with cls._lock:
            if cls._depth == 0:
                if cls._controller is False:
                    lapack_table()  # (loads SciPy's BLAS: the controller only knows the libraries loaded when it is built)
                    try:
                        from threadpoolctl import ThreadpoolController

                        cls._controller = ThreadpoolController()
                    except Exception:  # threadpoolctl missing: the BLAS keeps its own thread count
                        cls._controller = None
                cls._ctl = None if cls._controller is None else cls._controller.limit(limits=1, user_api="blas")
            cls._depth += 1

    def __exit__(self, *a):
        cls = blas_one_thread
        with cls._lock:
            cls._depth -= 1
            if cls._depth == 0 and cls._ctl is not None:
                cls._ctl.restore_original_limits()
                cls._ctl = None


def host_start_block(G, ny, b, ortho_tol, eps):
    """ds_host_start_block on a host fp64 tensor G ((ny + b) x 2 b): (lam, coef, cx, amp) as host tensors, or None when the caller
    has to take the explicit route."""
    G = G.contiguous()
    lam = torch.empty(b, dtype=torch.float64)
    coef = torch.empty((ny + b, b), dtype=torch.float64)
    cx = torch.empty((b, b), dtype=torch.float64)
    amp, route = _D(0.0), _I(0)
    with blas_one_thread():
        call("ds_host_start_block", ctypes.byref(lapack_table()), G.data_ptr(), ny, b, float(ortho_tol), float(eps), lam.data_ptr(),
             coef.data_ptr(), cx.data_ptr(), ctypes.byref(amp), ctypes.byref(route))
    return None if route.value else (lam, coef, cx, amp.value)


def host_polish(GK, coefs, GM, k):
    """ds_host_polish on host fp64 tensors: GK a list of (b x b) matrices, coefs their weights, GM (b x b): (E (k), C (b x b),
    qs ((len(GK) + 1) x k))."""
    b = GM.shape[0]
    gk = torch.stack([g_.contiguous() for g_ in GK]).contiguous()
    cf = torch.tensor([float(c) for c in coefs], dtype=torch.float64)
    GM = GM.contiguous()
    E = torch.empty(k, dtype=torch.float64)
    C = torch.empty((b, b), dtype=torch.float64)
    qs = torch.empty((len(GK) + 1, k), dtype=torch.float64)
    with blas_one_thread():
        call("ds_host_polish", ctypes.byref(lapack_table()), len(GK), gk.data_ptr(), cf.data_ptr(), GM.data_ptr(), b, k, E.data_ptr(),
             C.data_ptr(), qs.data_ptr())
    return E, C, qs


def host_raw_basis(GG, Gxp, lam_locked, ny, ncl, nxp, na, ortho_tol, eps):
    """ds_host_raw_basis on host fp64 tensors (the arguments of dense._raw_basis_transform): (G, Qw) - Qw the last na columns of
    the Python form's Q - or None for the explicit route.  The solver does not call it: it is the native loop's own step, here to be tested."""
    GG, Gxp, lam_locked = GG.contiguous(), Gxp.contiguous(), lam_locked.contiguous()
    G = torch.empty((nxp + na, nxp + na), dtype=torch.float64)
    Qw = torch.empty((ny + ncl + nxp + na, na), dtype=torch.float64)
    route = _I(0)
    with blas_one_thread():
        call("ds_host_raw_basis", ctypes.byref(lapack_table()), GG.data_ptr(), Gxp.data_ptr(), lam_locked.data_ptr(), ny, ncl, nxp, na,
             float(ortho_tol), float(eps), G.data_ptr(), Qw.data_ptr(), ctypes.byref(route))
    return None if route.value else (G, Qw)


def host_rr_step(G, na):
    """ds_host_rr_step on a host fp64 tensor G (sz x sz): (E (na), Z1 (sz x na), Zp (sz x na)) as dense._rr_step returns them."""
    G = G.contiguous()
    sz = G.shape[0]
    E = torch.empty(na, dtype=torch.float64)
    Z1, Zp = torch.empty((sz, na), dtype=torch.float64), torch.empty((sz, na), dtype=torch.float64)
    with blas_one_thread():
        call("ds_host_rr_step", ctypes.byref(lapack_table()), G.data_ptr(), sz, na, E.data_ptr(), Z1.data_ptr(), Zp.data_ptr())
    return E, Z1, Zp


class Pattern:
    """Host-side symbolic BSR-3 pattern (see ds_pattern_build in include/diffsound_hip.h)."""

    def __init__(self, tets_cpu_i32, nv, nthreads=0):
        t = tets_cpu_i32
        if t.device.type != "cpu" or t.dtype != torch.int32 or not t.is_contiguous() or t.dim() != 2:
            raise ValueError("Pattern: tets must be a contiguous (T, N) int32 CPU tensor")
        handle = ctypes.c_void_p()
        call("ds_pattern_build", ptr(t), t.shape[0], t.shape[1], nv, nthreads, ctypes.byref(handle))
        try:
            a, b, c = _I64(), _I64(), _I64()
            call("ds_pattern_sizes", handle, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c))
            self.nv, self.nnzb, self.ncontrib = a.value, b.value, c.value
            self.rowptr = torch.empty(self.nv + 1, dtype=torch.int32)
            self.colidx = torch.empty(self.nnzb, dtype=torch.int32)
            self.diagidx = torch.empty(self.nv, dtype=torch.int32)
            self.cptr = torch.empty(self.nnzb + 1, dtype=torch.int32)
            self.clist = torch.empty(self.ncontrib, dtype=torch.int32)
            call("ds_pattern_export", handle, ptr(self.rowptr), ptr(self.colidx), ptr(self.diagidx), ptr(self.cptr), ptr(self.clist))
        finally:
            lib().ds_pattern_free(handle)


class DevicePattern:
    """Symbolic phase on the device (ds_dpattern_build): every table as an int32 tensor on ``tets``' device.
    ``utab`` (ngroups, 2) = chunk range of each group, ``ctab`` (nchunks, 4) = (e0, e1, b0, b1) per chunk."""

    def __init__(self, tets_i32, nv, cap):
        t = tets_i32
        if not t.is_cuda or t.dtype != torch.int32 or not t.is_contiguous() or t.dim() != 2:
            raise ValueError("DevicePattern: tets must be a contiguous (T, N) int32 HIP tensor")
        handle = ctypes.c_void_p()
        call("ds_dpattern_build", ptr(t), t.shape[0], t.shape[1], nv, cap, stream_ptr(), ctypes.byref(handle))  # (stream not last)
        try:
            a, b, c, d, e = _I64(), _I64(), _I64(), _I64(), _I64()
            call("ds_dpattern_sizes", handle, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(d), ctypes.byref(e))
            self.nv, self.nnzb, self.ncontrib, self.ne, self.ngroups, self.nchunks = nv, a.value, b.value, c.value, d.value, e.value
            self.single = self.nchunks == self.ngroups  # every group is one chunk
            mk = lambda n: torch.empty(n, dtype=torch.int32, device=t.device)
            self.rowptr, self.colidx, self.diagidx = mk(nv + 1), mk(self.nnzb), mk(nv)
            self.cptr, self.clist = mk(self.nnzb + 1), mk(self.ncontrib)
            self.gptr, self.gent, self.goff, self.kperm = mk(self.ngroups + 1), mk(self.ne), mk(self.ne + 1), mk(self.nnzb)
            self.utab = torch.empty((self.ngroups, 2), dtype=torch.int32, device=t.device)
            self.ctab = torch.empty((self.nchunks, 4), dtype=torch.int32, device=t.device)
            launch("ds_dpattern_export", handle, ptr(self.rowptr), ptr(self.colidx), ptr(self.diagidx), ptr(self.cptr),
                   ptr(self.clist), ptr(self.gptr), ptr(self.gent), ptr(self.goff), ptr(self.kperm), ptr(self.utab), ptr(self.ctab))
            torch.cuda.current_stream(t.device).synchronize()  # the handle's arrays are freed below
        finally:
            lib().ds_dpattern_free(handle)


def edge_table(tets4, nv):
    """ds_edge_table: (T, 4) long HIP tensor -> (ea, eb, tet_edge): the distinct undirected edges (ea < eb, sorted)
    and the (T, 6) edge ids of every element's local edges, all long tensors on the same device."""
    t = tets4
    if not t.is_cuda or t.dtype != torch.int64 or t.dim() != 2 or t.shape[1] != 4:
        raise ValueError("edge_table: tets must be a (T, 4) int64 HIP tensor")
    t = t.contiguous()
    T = t.shape[0]
    ea = torch.empty(6 * T, dtype=torch.int64, device=t.device)
    eb = torch.empty(6 * T, dtype=torch.int64, device=t.device)
    te = torch.empty((T, 6), dtype=torch.int64, device=t.device)
    ne = _I64()
    launch("ds_edge_table", ptr(t), T, nv, ptr(ea), ptr(eb), ptr(te), ctypes.byref(ne), device=t.device)
    return ea[:ne.value], eb[:ne.value], te


def unique_rows3(xyz):
    """ds_unique_rows3: (n, 3) fp32 HIP tensor -> (inv (n,), first (n_unique,)) as torch.unique(dim=0,
    return_inverse=True) numbers the rows; first[i] = lowest row index holding the i-th distinct coordinate."""
    x = xyz
    if not x.is_cuda or x.dtype != torch.float32 or x.dim() != 2 or x.shape[1] != 3:
        raise ValueError("unique_rows3: need an (n, 3) float32 HIP tensor")
    x = x.contiguous()
    n = x.shape[0]
    inv = torch.empty(n, dtype=torch.int64, device=x.device)
    first = torch.empty(n, dtype=torch.int64, device=x.device)
    nu = _I64()
    launch("ds_unique_rows3", ptr(x), n, ptr(inv), ptr(first), ctypes.byref(nu), device=x.device)
    return inv, first[:nu.value]


class Groups:
    """Node groups of the neighbour-union SpMM (ds_groups_build): host arrays gptr, gent, goff, kperm (int32)."""

    def __init__(self, rowptr_cpu, colidx_cpu, nv):
        handle = ctypes.c_void_p()
        call("ds_groups_build", ptr(rowptr_cpu), ptr(colidx_cpu), nv, ctypes.byref(handle))
        try:
            a, b = _I64(), _I64()
            call("ds_groups_sizes", handle, ctypes.byref(a), ctypes.byref(b))
            self.ngroups, self.ne = a.value, b.value
            self.gptr = torch.empty(self.ngroups + 1, dtype=torch.int32)
            self.gent = torch.empty(self.ne, dtype=torch.int32)
            self.goff = torch.empty(self.ne + 1, dtype=torch.int32)
            self.kperm = torch.empty(colidx_cpu.numel(), dtype=torch.int32)
            call("ds_groups_export", handle, ptr(self.gptr), ptr(self.gent), ptr(self.goff), ptr(self.kperm))
        finally:
            lib().ds_groups_free(handle)


def union_chunks(gptr_cpu, goff_cpu, cap):
    """Chunk tables of the neighbour-union SpMM (ds_spmm_union): every group of 4 nodes (entries gptr[g]..gptr[g+1],
    blocks goff[e]..) is cut into chunks of whole entries with at most ``cap`` entries and ``cap`` blocks.  Returns
    (utab (ngroups, 2) int32 = chunk range of each group, ctab (nchunks, 4) int32 = (e0, e1, b0, b1)) as CPU tensors,
    or (None, None) if a single entry does not fit."""
    import numpy as np

    gp, go = gptr_cpu.numpy().astype(np.int64), goff_cpu.numpy().astype(np.int64)
    ng = gp.shape[0] - 1
    e0, e1 = gp[:-1], gp[1:]
    single = ((e1 - e0) <= cap) & ((go[e1] - go[e0]) <= cap)
    per_group = [None] * ng if not single.all() else None
    counts = np.ones(ng, dtype=np.int64)
    for gi in np.nonzero(~single)[0]:  # rare: a group whose union or block count exceeds the image
        e, rows = int(e0[gi]), []
        while e < e1[gi]:
            lim = min(int(e1[gi]), e + cap)  # furthest entry end with <= cap blocks and <= cap entries
            nxt = max(int(np.searchsorted(go[e:lim + 1], go[e] + cap, side="right")) - 1 + e, e + 1)
            rows.append((e, nxt, go[e], go[nxt]))
            e = nxt
        per_group[gi] = rows
        counts[gi] = len(rows)
    start = np.concatenate([[0], np.cumsum(counts)])
    ctab = np.empty((int(start[-1]), 4), dtype=np.int64)
    s_idx = start[:-1][single]
    ctab[s_idx] = np.stack([e0[single], e1[single], go[e0[single]], go[e1[single]]], 1)
    for gi in np.nonzero(~single)[0]:
        ctab[start[gi]:start[gi + 1]] = np.asarray(per_group[gi], dtype=np.int64)
    if ctab.shape[0] == 0 or int((ctab[:, 3] - ctab[:, 2]).max()) > cap:
        return None, None
    utab = np.stack([start[:-1], start[1:]], 1)
    return torch.from_numpy(utab.astype(np.int32)), torch.from_numpy(ctab.astype(np.int32))
