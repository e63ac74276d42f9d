"""The multipole entry points resolve on a CPU-only box, are declared in the header, bound in _hip and built by the
Makefile, and refuse bad arguments before any device work; so does the Python layer."""
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _cabi import assert_refused, hip_built as _hip_built, refusal_calls, symbols_declared  # noqa: E402

NAMES = ("ds_multipole_workspace_bytes", "ds_multipole_fwd", "ds_multipole_bwd")


def test_multipole_symbols():
    header, src = symbols_declared(NAMES, "multipole.hip")
    _hip = _hip_built()
    assert re.search(r"#define DS_MULTIPOLE_MAX_ORDER 32\b", header)
    assert re.search(r"#define DS_MULTIPOLE_MAX_MODES 512\b", header)
    assert _hip.lib().ds_abi_version() == 45 == _hip.ABI_VERSION  # three added symbols, no bump
    assert "atomic" not in src.replace("No atomics", "")
    assert "#pragma clang fp contract(off)" in src


OK = 1 << 20  # never dereferenced: the checks come first
GOOD = dict(gout=OK, pts=OK, center=OK, k=OK, coef=OK, P=3, m=5, L=2, out=OK, work=OK, bytes=1 << 16, gpts=OK, gcoef=OK)
FWD = ("pts", "center", "k", "coef", "P", "m", "L", "out")
BWD = ("gout", "pts", "center", "k", "coef", "P", "m", "L", "work", "bytes", "gpts", "gcoef")
NEED = 16 * 3 * 9 * 5  # 16 min(P, 128) (L + 1)^2 m
BAD = [(dict(pts=None), "null pointer"), (dict(center=None), "null pointer"), (dict(k=None), "null pointer"),
       (dict(coef=None), "null pointer"),
       (dict(P=0), "P = 0 outside 1..16777216"), (dict(P=-2), "outside 1..16777216"), (dict(P=(1 << 24) + 1), "outside 1..16777216"),
       (dict(m=0), "m = 0 outside 1..512"), (dict(m=513), "m = 513 outside 1..512"), (dict(m=-1), "outside 1..512"),
       (dict(L=-1), "L = -1 outside 0..32"), (dict(L=33), "L = 33 outside 0..32"),
       (dict(pts=OK + 4), "misaligned operand"), (dict(center=OK + 2), "misaligned operand"), (dict(k=OK + 4), "misaligned operand"),
       (dict(coef=OK + 8), "misaligned operand")]
BAD_FWD = [(dict(out=None), "null pointer"), (dict(out=OK + 8), "misaligned operand")]
BAD_BWD = [(dict(gout=None), "null pointer"), (dict(gout=OK + 8), "misaligned operand"),
           (dict(gpts=None, gcoef=None), "gpts and gcoef are both null"),
           (dict(work=None), "null pointer"), (dict(bytes=NEED - 1), "bytes, %d needed" % NEED), (dict(bytes=0), "needed"),
           (dict(work=OK + 8), "work not 16-byte aligned"),
           (dict(gpts=OK + 4), "misaligned operand"), (dict(gcoef=OK + 8), "misaligned operand")]
CALLS, IDS = refusal_calls(("ds_multipole_fwd", FWD), ("ds_multipole_bwd", BWD), BAD, BAD_FWD, BAD_BWD, id_from=13, id_sep="-")


@pytest.mark.parametrize("fn,order,change,text", CALLS, ids=IDS)
def test_multipole_arguments_are_checked_first(fn, order, change, text):
    """Every host-side refusal: DS_ERR_ARG and a message that names the entry point and the reason, in front of any launch."""
    assert_refused(fn, order, GOOD, change, text, status=1)


def test_multipole_workspace_query_needs_no_device():
    lib = _hip_built().lib()
    assert lib.ds_multipole_workspace_bytes(3, 5, 2) == NEED
    assert lib.ds_multipole_workspace_bytes(1, 1, 0) == 16
    assert lib.ds_multipole_workspace_bytes(128, 64, 32) == 16 * 128 * 1089 * 64
    assert lib.ds_multipole_workspace_bytes(1 << 24, 512, 32) == 16 * 128 * 1089 * 512  # the slabs stop at 128; beyond 2^30
    for a in [(0, 5, 2), (-1, 5, 2), ((1 << 24) + 1, 5, 2), (3, 0, 2), (3, 513, 2), (3, 5, -1), (3, 5, 33)]:
        assert lib.ds_multipole_workspace_bytes(*a) == 0


def test_python_layer_refuses_before_device_work():
    """The checks of ``multipole_eval`` and ``fit_multipoles`` need no device: ValueError on a CPU-only box, and RuntimeError
    for CPU tensors that pass them."""
    import torch

    from diffsound_amd.diffelastic.radiation import fit_multipoles, multipole_eval
    from src.diffelastic.radiation import ModalRadiator, multipole_eval as alias  # noqa: F401

    assert alias is multipole_eval
    f64 = lambda *v: torch.tensor(v, dtype=torch.float64)  # noqa: E731
    nan = float("nan")
    good = dict(points=torch.tensor([[1.0, 0.0, 0.0], [0.0, 2.0, 1.0]], dtype=torch.float64), center=f64(0.0, 0.0, 0.5),
                k=f64(1.0, 2.0), coef=torch.ones(2, 4, dtype=torch.complex128), order=1)
    bad = [(dict(points=torch.ones(2, 2, dtype=torch.float64)), r"points must be \(P, 3\)"),
           (dict(points=torch.ones(3, dtype=torch.float64)), r"points must be \(P, 3\)"),
           (dict(points=torch.ones(0, 3, dtype=torch.float64)), r"points must be \(P, 3\)"),
           (dict(points=torch.ones(2, 3, dtype=torch.long)), "points must be a floating-point tensor"),
           (dict(center=f64(0.0, 0.0)), r"center must be \(3,\)"), (dict(k=torch.ones(2, 1, dtype=torch.float64)), r"k must be \(m,\)"),
           (dict(k=torch.ones(513, dtype=torch.float64), coef=torch.ones(513, 4, dtype=torch.complex128)), "m <= 512"),
           (dict(coef=torch.ones(2, 9, dtype=torch.complex128)), r"coef must be \(2, 4\)"),
           (dict(coef=torch.ones(4, 2, dtype=torch.complex128)), r"coef must be \(2, 4\)"),
           (dict(coef=torch.ones(2, 4, dtype=torch.float64)), "coef must be a complex tensor"),
           (dict(order=-1), "order = -1 outside 0..32"), (dict(order=33, coef=torch.ones(2, 34 * 34, dtype=torch.complex128)), "order = 33"),
           (dict(order=1.0), "order"),
           (dict(points=torch.tensor([[1.0, nan, 0.0], [0.0, 2.0, 1.0]], dtype=torch.float64)), "points is not finite"),
           (dict(center=f64(0.0, float("inf"), 0.0)), "center is not finite"), (dict(k=f64(1.0, nan)), "k is not finite"),
           (dict(coef=torch.full((2, 4), complex(nan, 0.0), dtype=torch.complex128)), "coef is not finite"),
           (dict(k=f64(1.0, 0.0)), "k must be positive"), (dict(k=f64(-1.0, 2.0)), "k must be positive"),
           (dict(points=torch.tensor([[1.0, 0.0, 0.0], [0.0, 0.0, 0.5]], dtype=torch.float64)), "lies at the center")]
    for change, text in bad:
        with pytest.raises(ValueError, match=text):
            multipole_eval(**dict(good, **change))
    with pytest.raises(RuntimeError, match="HIP device"):
        multipole_eval(**good)
    pts = torch.ones(7, 3, dtype=torch.float64)
    vals = torch.ones(7, 2, dtype=torch.complex128)
    with pytest.raises(ValueError, match=r"7 samples, at least 2 \(order \+ 1\)\^2 = 8 needed"):
        fit_multipoles(pts, vals, good["k"], good["center"], 1)
    with pytest.raises(ValueError, match="order = 40"):
        fit_multipoles(pts, vals, good["k"], good["center"], 40)
    with pytest.raises(ValueError, match=r"values must be complex \(7, 2\)"):
        fit_multipoles(pts, vals[:, :1], good["k"], good["center"], 0)
    with pytest.raises(ValueError, match="values is not finite"):
        fit_multipoles(pts, vals * nan, good["k"], good["center"], 0)
    with pytest.raises(RuntimeError, match="HIP device"):
        fit_multipoles(pts, vals, good["k"], good["center"], 0)
