"""The biquad entry points resolve on a CPU-only box, are declared in the header, bound in _hip and built by the Makefile,
and refuse bad arguments before any device work, the earlier reason first."""
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _cabi import assert_refused, hip_built as _hip_built, refusal_calls, symbols_declared  # noqa: E402

NAMES = ("ds_biquad_workspace_bytes", "ds_biquad_fwd", "ds_biquad_bwd")


def test_biquad_symbols():
    header, src = symbols_declared(NAMES, "biquad.hip")
    _hip = _hip_built()
    assert re.search(r"#define DS_BIQUAD_MAX_SECTIONS 16\b", header) and re.search(r"#define DS_BIQUAD_MAX_ROWS 65535\b", header)
    assert _hip.lib().ds_abi_version() == 45 == _hip.ABI_VERSION  # three added symbols, no bump
    assert "atomic" not in src
    assert "osc_scan::RUN" in src and not re.search(r"constexpr\s+int\s+RUN\b", src)   # the scan's constant, no second one
    # the two promises are said where the caller reads them, and the workspace formula with them
    flat = re.sub(r"\s*\n \*\s*", " ", header)   # (the comment's line breaks)
    for text in ("no index and no trip count depends on the data", "yield inf or NaN in the outputs and nothing else",
                 "ds_biquad_workspace_bytes(B, N, S) = 8 B S N bytes"):
        assert text in flat, text


OK = 1 << 20  # never dereferenced: the checks come first
GOOD = dict(gy=OK, x=OK, sos=OK, per_clip=0, B=2, N=7, S=3, work=OK, bytes=1 << 16, y=OK, gx=OK, gsos=OK)
FWD = ("x", "sos", "per_clip", "B", "N", "S", "y")
BWD = ("gy", "x", "sos", "per_clip", "B", "N", "S", "work", "bytes", "gx", "gsos")
BAD = [(dict(x=None), "null pointer"), (dict(sos=None), "null pointer"),
       (dict(B=0), "empty problem"), (dict(B=-1), "empty problem"), (dict(N=0), "empty problem"), (dict(N=-3), "empty problem"),
       (dict(S=0), "empty problem"), (dict(S=-2), "empty problem"), (dict(B=65536), "B = 65536 above 65535"),
       (dict(S=17), "S = 17 sections above 16"), (dict(per_clip=2), "per_clip = 2 is neither 0 nor 1"),
       (dict(per_clip=-1), "per_clip = -1 is neither 0 nor 1"),
       (dict(x=OK + 2), "misaligned operand"), (dict(sos=OK + 4), "misaligned operand")]
BAD_FWD = [(dict(y=None), "null pointer"), (dict(y=OK + 2), "misaligned operand")]
BAD_BWD = [(dict(gy=None), "null pointer"), (dict(work=None), "null pointer"), (dict(gx=None), "null pointer"),
           (dict(gsos=None), "null pointer"), (dict(gy=OK + 2), "misaligned operand"), (dict(gx=OK + 2), "misaligned operand"),
           (dict(gsos=OK + 4), "misaligned operand"), (dict(work=OK + 8), "work not 16-byte aligned"),
           (dict(bytes=8 * 2 * 7 * 3 - 1), "bytes, 336 needed")]
# the order of the refusals: the earlier reason wins where two are wrong
ORDER = [(dict(x=None, B=0), "null pointer"), (dict(B=0, S=17), "empty problem"), (dict(B=65536, S=17), "above 65535"),
         (dict(S=17, per_clip=2), "sections above 16"), (dict(per_clip=2, x=OK + 2), "neither 0 nor 1")]
ORDER_BWD = [(dict(per_clip=2, work=OK + 8), "neither 0 nor 1"), (dict(gx=OK + 2, work=OK + 8), "misaligned operand"),
             (dict(gsos=OK + 4, bytes=1), "misaligned operand"), (dict(work=OK + 8, bytes=1), "work not 16-byte aligned")]
CALLS, IDS = refusal_calls(("ds_biquad_fwd", FWD), ("ds_biquad_bwd", BWD), BAD, BAD_FWD, BAD_BWD, ORDER, ORDER_BWD)


@pytest.mark.parametrize("fn,order,change,text", CALLS, ids=IDS)
def test_biquad_arguments_are_checked_first(fn, order, change, text):
    """Every host-side refusal: a non-zero status and a message that names the entry point and the reason, in front of any
    launch."""
    assert_refused(fn, order, GOOD, change, text)


def test_biquad_workspace_query_needs_no_device():
    lib = _hip_built().lib()
    for B, N, S in [(2, 7, 3), (3, 1025, 16), (65535, 1 << 20, 4)]:
        assert lib.ds_biquad_workspace_bytes(B, N, S) == 8 * B * S * N      # the header's formula
    for a in [(0, 7, 3), (-1, 7, 3), (65536, 7, 3), (2, 0, 3), (2, -7, 3), (2, 7, 0), (2, 7, 17)]:
        assert lib.ds_biquad_workspace_bytes(*a) == 0
