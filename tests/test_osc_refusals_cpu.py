"""Every argument refusal of the six oscillator-bank entry points (csrc/oscillator.hip, csrc/osc_driven.hip), pinned by its
return code and its full ds_last_error() text.  A refusal returns before the first HIP call, so none of this needs a GPU: the
pointers are small aligned host integers that are never dereferenced.

A case starts from arguments the entry point accepts and changes only what violates ITS condition, so every earlier condition
holds - the table pins the ORDER of the checks as well as their wording.  The texts are those of the library before the checks
were gathered into one checker per file; the two ``A = 65536`` cases of ds_osc_bank_fwd / _bwd came with that change (the
launch error they replace needed a device).  The time-varying pair has always reported A > 65535 as an empty problem.

Left out, because they sit behind a launch and need a device: the DS_LAUNCH_CHECK of every kernel launch."""
import os

import pytest

DS_ERR_ARG = 1

# distinct, 16-byte aligned, never dereferenced
D, W, AMP, FORCE, GY, Y, GS, GD, GW, GAMP, GFORCE, DMP, FRQ, G_DMP, G_FRQ, WORK = (0x1000 * (i + 1) for i in range(16))

DIMS = dict(A=2, m=3, F=5, S=7, sr=44100.0)
WORK_BYTES = 16 * (2 * 3 * 1 + 2 * 3)  # ds_osc_driven_workspace_bytes(A = 2, m = 3, S = 7): one tile of 1024 samples

# what every entry point accepts.  Values are listed in the order of the C signature.
GOOD = {
    "ds_osc_bank_fwd": dict(d=D, w=W, amp=AMP, force=FORCE, **DIMS, y=Y, stream=None),
    "ds_osc_bank_bwd": dict(gy=GY, d=D, w=W, amp=AMP, force=FORCE, **DIMS, gs=GS, gd=GD, gw=GW, gamp=GAMP, stream=None),
    "ds_osc_tv_fwd": dict(dmp=DMP, frq=FRQ, amp=AMP, force=FORCE, **DIMS, work=WORK, y=Y, stream=None),
    "ds_osc_tv_bwd": dict(gy=GY, dmp=DMP, frq=FRQ, amp=AMP, force=FORCE, **DIMS, gs=GS, g_dmp=G_DMP, g_frq=G_FRQ, gamp=GAMP,
                          stream=None),
    "ds_osc_driven_fwd": dict(d=D, w=W, amp=AMP, force=FORCE, **DIMS, work=WORK, work_bytes=WORK_BYTES, y=Y, stream=None),
    "ds_osc_driven_bwd": dict(gy=GY, d=D, w=W, amp=AMP, force=FORCE, **DIMS, work=WORK, work_bytes=WORK_BYTES, gd=GD, gw=GW,
                              gamp=GAMP, gforce=GFORCE, stream=None),
}

FORCE_LEN = "force length {} not in 1..512"
EMPTY_DRV = "empty problem (A {}, m {}, F {}, S {})"
TOO_MANY = "A = 65536 above 65535"

# (entry point, what the case violates, the changed arguments, the message behind "<entry point>: ")
CASES = [
    ("ds_osc_bank_fwd", "null", dict(force=None), "null pointer"),
    ("ds_osc_bank_fwd", "null-out", dict(y=None), "null pointer"),
    ("ds_osc_bank_fwd", "empty", dict(m=0), "empty problem"),
    ("ds_osc_bank_fwd", "sr", dict(sr=0.0), "empty problem"),
    ("ds_osc_bank_fwd", "F=0", dict(F=0), FORCE_LEN.format(0)),
    ("ds_osc_bank_fwd", "F=513", dict(F=513), FORCE_LEN.format(513)),
    ("ds_osc_bank_fwd", "A=65536", dict(A=65536), TOO_MANY),

    ("ds_osc_bank_bwd", "null", dict(gy=None), "null pointer"),
    ("ds_osc_bank_bwd", "null-out", dict(gw=None), "null pointer"),
    ("ds_osc_bank_bwd", "empty", dict(S=0), "empty problem"),
    ("ds_osc_bank_bwd", "F=0", dict(F=0), FORCE_LEN.format(0)),
    ("ds_osc_bank_bwd", "F=513", dict(F=513), FORCE_LEN.format(513)),
    ("ds_osc_bank_bwd", "A=65536", dict(A=65536), TOO_MANY),

    ("ds_osc_tv_fwd", "null", dict(frq=None), "null pointer"),
    ("ds_osc_tv_fwd", "null-work", dict(work=None), "null pointer"),
    ("ds_osc_tv_fwd", "empty", dict(A=0), "empty problem"),
    ("ds_osc_tv_fwd", "F=0", dict(F=0), FORCE_LEN.format(0)),
    ("ds_osc_tv_fwd", "F=513", dict(F=513), FORCE_LEN.format(513)),
    ("ds_osc_tv_fwd", "A=65536", dict(A=65536), "empty problem"),

    ("ds_osc_tv_bwd", "null", dict(dmp=None), "null pointer"),
    ("ds_osc_tv_bwd", "null-out", dict(g_frq=None), "null pointer"),
    ("ds_osc_tv_bwd", "empty", dict(m=-1), "empty problem"),
    ("ds_osc_tv_bwd", "F=0", dict(F=0), FORCE_LEN.format(0)),
    ("ds_osc_tv_bwd", "F=513", dict(F=513), FORCE_LEN.format(513)),
    ("ds_osc_tv_bwd", "A=65536", dict(A=65536), "empty problem"),

    ("ds_osc_driven_fwd", "null", dict(w=None), "null pointer"),
    ("ds_osc_driven_fwd", "null-work", dict(work=None), "null pointer"),
    ("ds_osc_driven_fwd", "empty", dict(S=0), EMPTY_DRV.format(2, 3, 5, 0)),
    ("ds_osc_driven_fwd", "F=0", dict(F=0), EMPTY_DRV.format(2, 3, 0, 7)),
    ("ds_osc_driven_fwd", "A=65536", dict(A=65536), TOO_MANY),
    ("ds_osc_driven_fwd", "work-short", dict(work_bytes=WORK_BYTES - 1), f"workspace of {WORK_BYTES - 1} bytes, {WORK_BYTES} needed"),
    ("ds_osc_driven_fwd", "work-misaligned", dict(work=WORK + 8), "work not 16-byte aligned"),
    ("ds_osc_driven_fwd", "operand-misaligned", dict(d=D + 4), "misaligned operand"),
    ("ds_osc_driven_fwd", "amp-misaligned", dict(amp=AMP + 2), "misaligned operand"),

    ("ds_osc_driven_bwd", "null", dict(gy=None), "null pointer"),
    ("ds_osc_driven_bwd", "null-out", dict(gd=None), "null pointer"),
    ("ds_osc_driven_bwd", "empty", dict(m=0), EMPTY_DRV.format(2, 0, 5, 7)),
    ("ds_osc_driven_bwd", "sr", dict(sr=-1.0), EMPTY_DRV.format(2, 3, 5, 7)),
    ("ds_osc_driven_bwd", "A=65536", dict(A=65536), TOO_MANY),
    ("ds_osc_driven_bwd", "work-short", dict(work_bytes=0), f"workspace of 0 bytes, {WORK_BYTES} needed"),
    ("ds_osc_driven_bwd", "work-misaligned", dict(work=WORK + 8), "work not 16-byte aligned"),
    ("ds_osc_driven_bwd", "gd-misaligned", dict(gd=GD + 4), "gd or gw not 8-byte aligned"),
    ("ds_osc_driven_bwd", "gw-misaligned", dict(gw=GW + 4), "gd or gw not 8-byte aligned"),
    ("ds_osc_driven_bwd", "operand-misaligned", dict(gforce=GFORCE + 2), "misaligned operand"),
    ("ds_osc_driven_bwd", "gy-misaligned", dict(gy=GY + 1), "misaligned operand"),
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
    import test_osc_listen_cabi_cpu
    import test_osc_slide_cabi_cpu

    tabled = set(GOOD) | set(test_osc_slide_cabi_cpu.NAMES) | set(test_osc_listen_cabi_cpu.NAMES)  # (theirs: the other two banks)
    assert {n for n in tabled if "workspace" not in n} == {n for n in _hip._SIGNATURES
                                                           if n.startswith("ds_osc_") and "workspace" not in n}
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


def test_driven_workspace_bytes():
    assert _lib().ds_osc_driven_workspace_bytes(2, 3, 7) == WORK_BYTES
