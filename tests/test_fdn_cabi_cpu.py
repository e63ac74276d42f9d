"""The FDN entry points resolve on a CPU-only box, are declared in the header, bound in _hip and built by the Makefile, and
refuse bad arguments before any device work, the earlier reason first."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _fdn_ref as F  # noqa: E402
from _cabi import assert_refused, hip_built as _hip_built, refusal_calls, symbols_declared  # noqa: E402

NAMES = ("ds_fdn_workspace_bytes", "ds_fdn_fwd", "ds_fdn_bwd")


def test_fdn_symbols():
    header, src = symbols_declared(NAMES, "fdn.hip")
    _hip = _hip_built()
    assert _hip.lib().ds_abi_version() == 45 == _hip.ABI_VERSION  # three added symbols, no bump
    code = re.sub(r"//[^\n]*", "", src)
    assert "atomic" not in code and "__shfl" not in code
    # the hand-off is the workgroup barrier and nothing else: no fence, no flag, no spinning
    assert "__threadfence" not in code and "volatile" not in code and "while" not in code
    flat = re.sub(r"\s*\n \*\s*", " ", header)   # (the comment's line breaks)
    for text in ("c = 0, d = 1 returns x (a negative zero is the number zero and comes out as +0)",
                 "THE DELAYS ARE NEVER READ ON THE HOST", "the kernels read such a delay as DS_FDN_MIN_DELAY",
                 "no index and no trip count depends on them", "Asynchronous on the stream, no allocation",
                 "what is NULL is not computed and does not change the bits of the rest",
                 "ds_fdn_workspace_bytes(B, H, N, n) = 8 B (n N + ceil(N / 1024) (n^2 + 3 n + 1)) bytes"):
        assert text in flat, text


def test_the_cases_were_built_from_the_kernels_constants():
    src = open(os.path.join(ROOT, "diffsound_amd", "csrc", "fdn.hip")).read()
    const = lambda name: re.search(r"constexpr int %s = ([^;]+);" % name, src).group(1)
    assert int(const("FDN_THREADS")) == F.THREADS and int(const("FDN_CHUNK")) == F.CHUNK and int(const("RED_TILE")) == F.RED_TILE
    assert const("MAXN") == "DS_FDN_MAX_LINES"
    header = open(os.path.join(ROOT, "include", "diffsound_hip.h")).read()
    for name, value in (("MAX_LINES", F.MAX_LINES), ("MIN_DELAY", F.MIN_DELAY), ("MAX_ROWS", F.MAX_ROWS)):
        assert re.search(r"#define DS_FDN_%s %d\b" % (name, value), header), name
    from diffsound_amd.ddsp import fdn

    assert (fdn.MAX_LINES, fdn.MIN_DELAY, fdn.MAX_ROWS) == (16, 64, 65535) == (F.MAX_LINES, F.MIN_DELAY, F.MAX_ROWS)


OK = 1 << 20  # never dereferenced: the checks come first
GOOD = dict(gy=OK, x=OK, delays=OK, A=OK, b=OK, c=OK, d=OK, p=OK, B=6, H=3, N=5000, n=5, state=OK, work=OK, bytes=1 << 24, y=OK,
            gx=OK, gA=OK, gb=OK, gc=OK, gd=OK, gp=OK)
NEED = 8 * 6 * (5 * 5000 + 5 * 41)   # ceil(5000 / 1024) = 5 chunks of 25 + 15 + 1 sums
SETS = ("delays", "A", "b", "c", "d", "p", "B", "H", "N", "n")
FWD = ("x",) + SETS + ("state", "y")
BWD = ("gy", "x") + SETS + ("state", "work", "bytes", "gx", "gA", "gb", "gc", "gd", "gp")
NONE = dict(gx=None, gA=None, gb=None, gc=None, gd=None, gp=None)
BAD = [(dict([(k, None)]), "null pointer") for k in ("x", "delays", "A", "b", "c", "d", "state")]
BAD += [(dict([(k, v)]), "empty problem") for k in ("B", "H", "N", "n") for v in (0, -2)]
BAD += [(dict(B=65536, H=1), "B = 65536 above 65535"), (dict(n=17), "n = 17 lines above 16"),
        (dict(H=7), "B = 6 is not a multiple of H = 7"), (dict(H=4), "B = 6 is not a multiple of H = 4"),
        (dict(x=OK + 2), "misaligned operand"), (dict(delays=OK + 2), "misaligned operand")]
BAD += [(dict([(k, OK + 4)]), "misaligned operand") for k in ("A", "b", "c", "d", "p", "state")]
BAD_FWD = [(dict(y=None), "null pointer"), (dict(y=OK + 2), "misaligned operand")]
BAD_BWD = [(dict(gy=None), "null pointer"), (dict(work=None), "null pointer"), (dict(gy=OK + 2), "misaligned operand"),
           (dict(gx=OK + 2), "misaligned operand")]
BAD_BWD += [(dict([(k, OK + 4)]), "misaligned operand") for k in ("gA", "gb", "gc", "gd", "gp")]
BAD_BWD += [(NONE, "every output is NULL"), (dict(work=OK + 8), "work not 16-byte aligned"),
            (dict(bytes=NEED - 1), f"bytes, {NEED} needed"), (dict(gA=None, gb=None, gc=None, gd=None, gp=None, bytes=0), f"bytes, {NEED} needed")]
# the order of the refusals: the earlier reason wins where two are wrong
ORDER = [(dict(x=None, B=0), "null pointer"), (dict(N=0, B=65536), "empty problem"), (dict(B=65536, n=17), "above 65535"),
         (dict(n=17, H=4), "lines above 16"), (dict(H=4, x=OK + 2), "not a multiple")]
ORDER_BWD = [(dict(NONE, gy=OK + 2), "misaligned operand"), (dict(NONE, work=OK + 8), "every output is NULL"),
             (dict(work=OK + 8, bytes=1), "work not 16-byte aligned"), (dict(H=4, work=OK + 8), "not a multiple")]
CALLS, IDS = refusal_calls(("ds_fdn_fwd", FWD), ("ds_fdn_bwd", BWD), BAD, BAD_FWD, BAD_BWD, ORDER, ORDER_BWD)


@pytest.mark.parametrize("fn,order,change,text", CALLS, ids=IDS)
def test_fdn_arguments_are_checked_first(fn, order, change, text):
    """Every host-side refusal: DS_ERR_ARG and a message that names the entry point and the reason, in front of any launch."""
    assert_refused(fn, order, GOOD, change, text, status=1)


def test_a_null_damping_is_no_refusal_but_the_delays_are_not_read():
    """p may be NULL, and the delays are device memory: a host call with a fake pointer gets as far as the next refusal."""
    assert_refused("ds_fdn_fwd", FWD, GOOD, dict(p=None, y=OK + 2), "misaligned operand", status=1)
    assert_refused("ds_fdn_bwd", BWD, GOOD, dict(p=None, bytes=0), "needed", status=1)


def test_fdn_workspace_query_needs_no_device():
    lib = _hip_built().lib()
    assert lib.ds_fdn_workspace_bytes(6, 3, 5000, 5) == NEED
    for B, H, N, n in [(2, 1, 37, 1), (4, 2, 1024, 16), (2, 2, 1025, 3), (65535, 1, 1 << 20, 16), (8, 1, 32000, 16)]:
        assert lib.ds_fdn_workspace_bytes(B, H, N, n) == 8 * B * (n * N + -(-N // F.CHUNK) * (n * n + 3 * n + 1))   # the header's formula
    for a in [(0, 1, 7, 3), (-1, 1, 7, 3), (65536, 1, 7, 3), (2, 0, 7, 3), (2, 3, 7, 3), (6, 4, 7, 3), (2, 1, 0, 3), (2, 1, -7, 3),
              (2, 1, 7, 0), (2, 1, 7, 17)]:
        assert lib.ds_fdn_workspace_bytes(*a) == 0
