"""Every argument refusal of the neighbour-union SpMM entry points (csrc/spmm_union.hip), pinned by its return code and its full
ds_last_error() text.  A refusal returns before the first HIP call, so none of this needs a GPU: the pointers are small aligned
host integers that are never dereferenced.

One case per DS_REQUIRE of ds_pack_groups, ds_spmm_union, ds_spmm_union_narrow, ds_union_residual, ds_union_residual_pre,
ds_spmm_union_km and ds_spmm_union16 (the eighth entry point, ds_union_residual_workspace_bytes, refuses nothing; its value is
pinned through the workspace refusals).  A case starts from arguments the entry point accepts and changes only what violates
ITS condition, so every earlier condition holds - the table pins the ORDER of the checks as well as their wording.

Left out, because they sit behind a launch and need a device: the DS_LAUNCH_CHECK of every kernel launch (pack_groups_kernel,
spmm_union_kernel, spmm_union_narrow_kernel, union_norm_partial_kernel, union_norm_final_kernel) and the return code of the
walk that ds_union_residual / ds_union_residual_pre hand on before their two norm reductions."""
import os

import pytest

DS_ERR_ARG = 1
PIPE_OOB = 0x7F000000  # the descriptor range of spmm_device.h

# aligned, distinct, never dereferenced
UTAB, CTAB, GENT, KGRP, MGRP, X, Y, R0, DINV, WPREV, LAM, WORK, RN2, XN2, W1, VALS_T, KPERM = (0x1000 * (i + 1) for i in range(17))

# nv = 8 nodes in 2 groups of 4, 8 columns: what every entry point accepts.  Values are listed in the order of the C signature.
UNION = dict(epilogue=1, level_tag=0, utab=UTAB, ctab=CTAB, ngroups=2, cap_blocks=140, gent=GENT, kgrp=KGRP, nnzb=16, nv=8, X=X, ldx=8,
             Y=Y, ldy=8, R0=R0, ldr=8, dinv=DINV, ncols=8, c1=0.5, c2=0.5, first=0, Wprev=None, ldp=0, stream=None)
NARROW = dict(kind=0, level_tag=0, utab=UTAB, ctab=CTAB, ngroups=2, gent=GENT, vals=KGRP, nnzb=16, nv=8, X=X, ldx=8, Y=Y, ldy=8,
              ncols=8, stream=None)
RESID = dict(level_tag=0, utab=UTAB, ctab=CTAB, ngroups=2, cap_blocks=140, gent=GENT, kgrp=KGRP, mgrp=MGRP, nnzb=16, nv=8, X=X, ldx=8,
             lam=LAM, R=Y, ldr=8, ncols=8, work=WORK, work_bytes=1 << 20, rn2=RN2, xn2=XN2, stream=None)
PRE = dict(level_tag=0, utab=UTAB, ctab=CTAB, ngroups=2, cap_blocks=140, gent=GENT, kgrp=KGRP, mgrp=MGRP, nnzb=16, nv=8, X=X, ldx=8,
           lam=LAM, dinv=DINV, c=0.5, R16=Y, ldr16=8, W1=W1, ldw1=8, ncols=8, work=WORK, work_bytes=1 << 20, rn2=RN2, xn2=XN2,
           stream=None)
KM = dict(level_tag=0, utab=UTAB, ctab=CTAB, ngroups=2, cap_blocks=140, gent=GENT, kgrp=KGRP, mgrp=MGRP, nnzb=16, nv=8, X=X, ldx=8,
          KX=Y, ldk=8, MX=R0, ldm=8, ncols=8, stream=None)
UNION16 = dict(epilogue=1, utab=UTAB, ctab=CTAB, ngroups=2, cap_blocks=140, gent=GENT, kgrp=KGRP, nnzb=16, nv=8, X=X, ldx=8, Y=Y, ldy=8,
               y_f32=0, R0=R0, ldr=8, dinv=DINV, ncols=8, c1=0.5, c2=0.5, first=0, Wprev=None, ldp=0, stream=None)
PACK = dict(vals_t=VALS_T, kperm=KPERM, nnzb=16, kgrp=KGRP, stream=None)
GOOD = {"ds_pack_groups": PACK, "ds_spmm_union": UNION, "ds_spmm_union_narrow": NARROW, "ds_union_residual": RESID,
        "ds_union_residual_pre": PRE, "ds_spmm_union_km": KM, "ds_spmm_union16": UNION16}

LD_OOB = (PIPE_OOB // 12 // 4 + 1) * 4  # the first leading dimension (a multiple of 4) whose 3-row fp32 panel leaves the range
LD16_OOB = (PIPE_OOB // 48 // 4 + 1) * 4  # the same for a bf16 block of nv = 8 nodes (3 nv ld 2 bytes)
NNZB_OOB = (1 << 32) // 36 + 1  # the first block count whose 36-byte blocks leave a 32-bit offset
WORK_BYTES = 2 * 2 * 8 * 4 + 256 * 2 * 8 * 8  # ds_union_residual_workspace_bytes(ngroups = 2, ncols = 8)
SHAPE = "ncols must be a multiple of 4 <= 84 and ngroups = ceil(nv / 4)"
LEVEL = "level_tag must be 0 (fine) or 1 (corner-node level)"

# (entry point, what the case violates, the changed arguments, the message behind "<entry point>: ")
CASES = [
    ("ds_pack_groups", "null", dict(vals_t=None), "bad argument"),
    ("ds_pack_groups", "empty", dict(nnzb=0), "bad argument"),

    ("ds_spmm_union", "null", dict(ctab=None), "null pointer"),
    ("ds_spmm_union", "epilogue", dict(epilogue=4), "bad epilogue 4"),
    ("ds_spmm_union", "level", dict(level_tag=2), LEVEL),
    ("ds_spmm_union", "r0", dict(R0=None), "the epilogue needs R0"),
    ("ds_spmm_union", "dinv", dict(dinv=None), "the Chebyshev epilogue needs dinv"),
    ("ds_spmm_union", "ncols", dict(ncols=88, ldx=88, ldy=88, ldr=88), SHAPE),
    ("ds_spmm_union", "ncols-mod4", dict(ncols=6), SHAPE),
    ("ds_spmm_union", "ngroups", dict(ngroups=3), SHAPE),
    ("ds_spmm_union", "cap", dict(cap_blocks=141), "a chunk of 141 blocks exceeds the LDS image (DS_UNION_CAP = 140)"),
    ("ds_spmm_union", "cap-zero", dict(cap_blocks=0), "a chunk of 0 blocks exceeds the LDS image (DS_UNION_CAP = 140)"),
    ("ds_spmm_union", "ld", dict(ldy=4), "leading dimension smaller than ncols"),
    ("ds_spmm_union", "ldr", dict(ldr=4), "leading dimension smaller than ncols"),
    ("ds_spmm_union", "alias", dict(Y=X), "X and Y must be different buffers"),
    ("ds_spmm_union", "panel-range", dict(ldx=LD_OOB), f"a 3-row panel of {LD_OOB * 12} bytes exceeds the descriptor range"),
    ("ds_spmm_union", "value-range", dict(nnzb=NNZB_OOB), "value array exceeds the descriptor range"),
    ("ds_spmm_union", "align", dict(X=X + 8), "rows, kgrp and ctab must be 16-byte aligned"),
    ("ds_spmm_union", "align-r0", dict(R0=R0 + 8), "rows, kgrp and ctab must be 16-byte aligned"),
    ("ds_spmm_union", "wprev", dict(Wprev=WPREV, ldp=4), "bad W_prev block"),

    ("ds_spmm_union_narrow", "null", dict(vals=None), "null pointer"),
    ("ds_spmm_union_narrow", "kind", dict(kind=1), "kind must be 0 (3x3 blocks) or 3 (node-scalar values)"),
    ("ds_spmm_union_narrow", "level", dict(level_tag=2), LEVEL),
    ("ds_spmm_union_narrow", "ncols", dict(ncols=20, ldx=20, ldy=20), "ncols must be a multiple of 4 <= 16 and ngroups = ceil(nv / 4)"),
    ("ds_spmm_union_narrow", "ngroups", dict(ngroups=3), "ncols must be a multiple of 4 <= 16 and ngroups = ceil(nv / 4)"),
    ("ds_spmm_union_narrow", "ld", dict(ldx=4), "leading dimension smaller than ncols"),
    ("ds_spmm_union_narrow", "alias", dict(Y=X), "X and Y must be different buffers"),
    ("ds_spmm_union_narrow", "align", dict(ctab=CTAB + 8), "rows and ctab must be 16-byte aligned"),

    ("ds_union_residual", "null", dict(R=None), "null pointer"),
    ("ds_union_residual", "level", dict(level_tag=2), LEVEL),
    ("ds_union_residual", "ncols", dict(ncols=88, ldx=88, ldr=88), SHAPE),
    ("ds_union_residual", "ngroups", dict(ngroups=3), SHAPE),
    ("ds_union_residual", "cap", dict(cap_blocks=141), "a chunk of 141 blocks exceeds the LDS image"),
    ("ds_union_residual", "ld", dict(ldr=4), "leading dimension smaller than ncols"),
    ("ds_union_residual", "alias", dict(R=X), "X and R must be different buffers"),
    ("ds_union_residual", "range", dict(ldr=LD_OOB), "operand beyond the descriptor range"),
    ("ds_union_residual", "align", dict(work=WORK + 8), "rows, kgrp, ctab and the workspace must be 16-byte aligned"),
    ("ds_union_residual", "align-r", dict(R=Y + 8), "rows, kgrp, ctab and the workspace must be 16-byte aligned"),
    ("ds_union_residual", "workspace", dict(work_bytes=WORK_BYTES - 1), f"workspace of {WORK_BYTES} bytes needed"),

    ("ds_union_residual_pre", "null-r16", dict(R16=None), "null pointer"),
    ("ds_union_residual_pre", "null", dict(W1=None), "null pointer"),
    ("ds_union_residual_pre", "null-dinv", dict(dinv=None), "null pointer"),
    ("ds_union_residual_pre", "level", dict(level_tag=1), "level_tag must be 0 (fine)"),
    ("ds_union_residual_pre", "ncols", dict(ncols=6), SHAPE),
    ("ds_union_residual_pre", "cap", dict(cap_blocks=141), "a chunk of 141 blocks exceeds the LDS image"),
    ("ds_union_residual_pre", "ld", dict(ldw1=4), "leading dimension smaller than ncols"),
    ("ds_union_residual_pre", "alias", dict(W1=Y), "X, R16 and W1 must be different buffers"),
    ("ds_union_residual_pre", "range", dict(nnzb=NNZB_OOB), "operand beyond the descriptor range"),
    ("ds_union_residual_pre", "align-bf16", dict(R16=Y + 4), "bf16 rows must be 8-byte aligned"),
    ("ds_union_residual_pre", "align-dinv", dict(dinv=DINV + 2), "bf16 rows must be 8-byte aligned"),
    ("ds_union_residual_pre", "align", dict(X=X + 8), "rows, kgrp, ctab and the workspace must be 16-byte aligned"),
    ("ds_union_residual_pre", "workspace", dict(work_bytes=0), f"workspace of {WORK_BYTES} bytes needed"),

    ("ds_spmm_union_km", "null", dict(mgrp=None), "null pointer"),
    ("ds_spmm_union_km", "level", dict(level_tag=-1), LEVEL),
    ("ds_spmm_union_km", "ncols", dict(ncols=0), SHAPE),
    ("ds_spmm_union_km", "cap", dict(cap_blocks=141), "a chunk of 141 blocks exceeds the LDS image"),
    ("ds_spmm_union_km", "ld", dict(ldm=4), "leading dimension smaller than ncols"),
    ("ds_spmm_union_km", "alias", dict(MX=Y), "X, KX and MX must be different buffers"),
    ("ds_spmm_union_km", "range", dict(ldx=LD_OOB), "operand beyond the descriptor range"),
    ("ds_spmm_union_km", "align", dict(ldk=10), "rows, kgrp and ctab must be 16-byte aligned"),

    ("ds_spmm_union16", "null", dict(R0=None), "null pointer"),
    ("ds_spmm_union16", "epilogue", dict(epilogue=0), "epilogue must be 1 (Chebyshev term) or 2 (residual)"),
    ("ds_spmm_union16", "dinv", dict(dinv=None), "the Chebyshev epilogue needs dinv"),
    ("ds_spmm_union16", "ngroups", dict(ngroups=1), SHAPE),
    ("ds_spmm_union16", "cap", dict(cap_blocks=141), "a chunk of 141 blocks exceeds the LDS image"),
    ("ds_spmm_union16", "ld", dict(ldr=4), "leading dimension smaller than ncols"),
    ("ds_spmm_union16", "alias", dict(Y=X), "X and Y must be different buffers"),
    ("ds_spmm_union16", "block-range", dict(ldx=LD16_OOB), f"a bf16 operand block of {LD16_OOB * 48} bytes exceeds the descriptor range"),
    ("ds_spmm_union16", "value-range", dict(nnzb=NNZB_OOB), "value array exceeds the descriptor range"),
    ("ds_spmm_union16", "align", dict(X=X + 4), "bf16 rows must be 8-byte aligned (fp32 output rows, kgrp and ctab 16-byte)"),
    ("ds_spmm_union16", "align-f32out", dict(y_f32=1, Y=Y + 8), "bf16 rows must be 8-byte aligned (fp32 output rows, kgrp and ctab 16-byte)"),
    ("ds_spmm_union16", "wprev", dict(Wprev=WPREV, ldp=4), "bad W_prev block"),
    ("ds_spmm_union16", "f32out", dict(epilogue=2, y_f32=1), "an fp32 result is the Chebyshev term's only"),
]


def _lib():
    from diffsound_amd import _hip

    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return _hip.lib()


def test_table_names_every_entry_point_and_no_argument_twice():
    from diffsound_amd import _hip

    assert {c[0] for c in CASES} == set(GOOD)
    assert len({c[:2] for c in CASES}) == len(CASES)
    for entry, _, change, _ in CASES:
        assert set(change) <= set(GOOD[entry]), (entry, change)
    for entry, good in GOOD.items():
        assert len(good) == len(_hip._SIGNATURES[entry][1]), entry


@pytest.mark.parametrize("entry,what,change,message", CASES, ids=[f"{c[0]}-{c[1]}" for c in CASES])
def test_refusal(entry, what, change, message):
    lib = _lib()
    args = dict(GOOD[entry], **change)
    rc = getattr(lib, entry)(*args.values())
    assert rc == DS_ERR_ARG
    assert lib.ds_last_error().decode() == f"{entry}: {message}"


def test_workspace_bytes():
    assert _lib().ds_union_residual_workspace_bytes(2, 8) == WORK_BYTES
