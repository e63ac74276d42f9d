"""The FIR entry points resolve on a CPU-only box, are declared in the header, bound in _hip and built by the Makefile, and
refuse bad arguments before any device work, the earlier reason first."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _fir_ref as F  # noqa: E402
from _cabi import assert_refused, hip_built as _hip_built, refusal_calls, symbols_declared  # noqa: E402

NAMES = ("ds_fir_workspace_bytes", "ds_fir_fwd", "ds_fir_bwd")


def test_fir_symbols():
    header, src = symbols_declared(NAMES, "fir.hip")
    _hip = _hip_built()
    assert re.search(r"#define DS_FIR_MAX_TAPS 65536\b", header) and re.search(r"#define DS_FIR_MAX_ROWS 65535\b", header)
    assert _hip.lib().ds_abi_version() == 45 == _hip.ABI_VERSION  # three added symbols, no bump
    assert "atomic" not in src
    assert len(re.findall(r"\bacc\[i\] \+= av \* ", src)) == 1   # one inner loop for the three sums, not three copies
    # the promises are said where the caller reads them, and the workspace formula with them
    flat = re.sub(r"\s*\n \*\s*", " ", header)   # (the comment's line breaks)
    for text in ("copies x shifted by k bit for bit, with exact zeros in front, as long as the inputs are finite",
                 "the same holds for gx from gy", "no index and no trip count depends on the data",
                 "yield inf or NaN in the outputs and nothing else", "Asynchronous on the stream, no allocation",
                 "ds_fir_workspace_bytes(B, H, N, L) = 8 B ceil(N / 2048) min(L, N) bytes"):
        assert text in flat, text


def test_the_cases_were_built_from_the_kernels_constants():
    src = open(os.path.join(ROOT, "diffsound_amd", "csrc", "fir.hip")).read()
    const = lambda name: re.search(r"constexpr int %s = ([^;]+);" % name, src).group(1)
    assert int(const("R")) == F.R and const("TILE") == "64 * R" and 64 * F.R == F.TILE
    assert int(const("TAPS")) == F.TAPS and int(const("GH_CHUNK")) == F.GH_CHUNK
    header = open(os.path.join(ROOT, "include", "diffsound_hip.h")).read()
    assert f"#define DS_FIR_MAX_TAPS {F.MAX_TAPS}" in header and f"#define DS_FIR_MAX_ROWS {F.MAX_ROWS}" in header


OK = 1 << 20  # never dereferenced: the checks come first
GOOD = dict(gy=OK, x=OK, h=OK, B=6, H=3, N=5000, L=300, work=OK, bytes=1 << 20, y=OK, gx=OK, gh=OK)
NEED = 8 * 6 * 3 * 300   # ceil(5000 / 2048) = 3 chunks
FWD = ("x", "h", "B", "H", "N", "L", "y")
BWD = ("gy", "x", "h", "B", "H", "N", "L", "work", "bytes", "gx", "gh")
BAD = [(dict(x=None), "null pointer"), (dict(h=None), "null pointer"),
       (dict(B=0), "empty problem"), (dict(B=-6), "empty problem"), (dict(H=0), "empty problem"), (dict(H=-1), "empty problem"),
       (dict(N=0), "empty problem"), (dict(N=-3), "empty problem"), (dict(L=0), "empty problem"), (dict(L=-2), "empty problem"),
       (dict(B=65536, H=1), "B = 65536 above 65535"), (dict(L=65537), "L = 65537 taps above 65536"),
       (dict(H=7), "B = 6 is not a multiple of H = 7"), (dict(H=4), "B = 6 is not a multiple of H = 4"),
       (dict(x=OK + 2), "misaligned operand"), (dict(h=OK + 4), "misaligned operand")]
BAD_FWD = [(dict(y=None), "null pointer"), (dict(y=OK + 2), "misaligned operand")]
BAD_BWD = [(dict(gy=None), "null pointer"), (dict(work=None), "null pointer"), (dict(gy=OK + 2), "misaligned operand"),
           (dict(gx=OK + 2), "misaligned operand"), (dict(gh=OK + 4), "misaligned operand"),
           (dict(gx=None, gh=None), "gx and gh are both NULL"), (dict(gx=None, gh=None, work=None), "gx and gh are both NULL"),
           (dict(work=OK + 8), "work not 16-byte aligned"), (dict(bytes=NEED - 1), f"bytes, {NEED} needed"),
           (dict(gx=None, bytes=0), f"bytes, {NEED} needed")]
# the order of the refusals: the earlier reason wins where two are wrong
ORDER = [(dict(x=None, B=0), "null pointer"), (dict(N=0, B=65536), "empty problem"), (dict(B=65536, L=65537), "above 65535"),
         (dict(L=65537, H=4), "taps above 65536"), (dict(H=4, x=OK + 2), "not a multiple")]
ORDER_BWD = [(dict(gy=OK + 2, gx=None, gh=None), "misaligned operand"), (dict(gx=None, gh=None, bytes=0), "both NULL"),
             (dict(work=OK + 8, bytes=1), "work not 16-byte aligned"), (dict(H=4, work=OK + 8), "not a multiple")]
CALLS, IDS = refusal_calls(("ds_fir_fwd", FWD), ("ds_fir_bwd", BWD), BAD, BAD_FWD, BAD_BWD, ORDER, ORDER_BWD)


@pytest.mark.parametrize("fn,order,change,text", CALLS, ids=IDS)
def test_fir_arguments_are_checked_first(fn, order, change, text):
    """Every host-side refusal: DS_ERR_ARG and a message that names the entry point and the reason, in front of any launch."""
    assert_refused(fn, order, GOOD, change, text, status=1)


def test_fir_workspace_query_needs_no_device():
    lib = _hip_built().lib()
    for B, H, N, L in [(6, 3, 5000, 300), (2, 1, 37, 100), (4, 2, 4097, 4096), (2, 2, 2048, 1), (2, 2, 2049, 65536),
                       (65535, 1, 1 << 20, 65536)]:
        assert lib.ds_fir_workspace_bytes(B, H, N, L) == 8 * B * -(-N // F.GH_CHUNK) * min(L, N)      # the header's formula
    for a in [(0, 1, 7, 3), (-1, 1, 7, 3), (65536, 1, 7, 3), (2, 0, 7, 3), (2, 3, 7, 3), (6, 4, 7, 3), (2, 1, 0, 3), (2, 1, -7, 3),
              (2, 1, 7, 0), (2, 1, 7, 65537)]:
        assert lib.ds_fir_workspace_bytes(*a) == 0
