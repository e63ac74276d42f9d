"""The contact-force entry points resolve on a CPU-only box, are declared in the header, bound in _hip and built by the
Makefile, and refuse bad arguments before any device work."""
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _cabi import assert_refused, hip_built as _hip_built, refusal_calls, symbols_declared  # noqa: E402

NAMES = ("ds_contact_workspace_bytes", "ds_contact_fwd", "ds_contact_bwd")


def test_contact_symbols():
    header, src = symbols_declared(NAMES, "contact.hip")
    _hip = _hip_built()
    assert re.search(r"#define DS_CONTACT_MAX_MODES 512\b", header)
    assert _hip.lib().ds_abi_version() == 45 == _hip.ABI_VERSION  # three added symbols, no bump
    assert "__shared__" not in src and "__syncthreads" not in src
    assert "atomic" not in src.replace("no atomics", "")


OK = 1 << 20  # never dereferenced: the checks come first
GOOD = dict(gforce=OK, d=OK, w=OK, gain=OK, mass=OK, vel=OK, stiff=OK, A=2, m=3, F=5, R=4, p=1.5, sr=44100.0, work=OK,
            bytes=1 << 16, force=OK, gd=OK, gw=OK, ggain=OK, gmass=OK, gvel=OK, gstiff=OK)
FWD = ("d", "w", "gain", "mass", "vel", "stiff", "A", "m", "F", "R", "p", "sr", "force")
BWD = ("gforce", "d", "w", "gain", "mass", "vel", "stiff", "A", "m", "F", "R", "p", "sr", "work", "bytes", "gd", "gw", "ggain",
       "gmass", "gvel", "gstiff")
NEED = 16 * (2 * 20 * 4 + 2 * 3)  # 16 (A F R (1 + m) + A m)
BAD = [(dict(d=None), "null pointer"), (dict(w=None), "null pointer"), (dict(gain=None), "null pointer"),
       (dict(mass=None), "null pointer"), (dict(vel=None), "null pointer"), (dict(stiff=None), "null pointer"),
       (dict(A=0), "A = 0 outside 1..65535"), (dict(A=-1), "outside 1..65535"), (dict(A=65536), "outside 1..65535"),
       (dict(m=0), "m = 0 outside 1..512"), (dict(m=513), "m = 513 outside 1..512"),
       (dict(R=0), "R = 0 outside 1..64"), (dict(R=65), "R = 65 outside 1..64"),
       (dict(F=0), "F = 0 below 1"), (dict(F=-3), "below 1"),
       (dict(F=(1 << 20) // 4 + 1), "substeps above 1048576"), (dict(F=1 << 30, R=64), "substeps above 1048576"),
       (dict(p=0.99), "exponent >= 1"), (dict(p=float("nan")), "exponent >= 1"), (dict(p=float("inf")), "exponent >= 1"),
       (dict(sr=0.0), "not positive"), (dict(sr=-1.0), "not positive"),
       (dict(d=OK + 4), "misaligned operand"), (dict(gain=OK + 4), "misaligned operand"), (dict(stiff=OK + 2), "misaligned operand")]
BAD_FWD = [(dict(force=None), "null pointer"), (dict(force=OK + 2), "misaligned operand")]
BAD_BWD = [(dict(gforce=None), "null pointer"), (dict(work=None), "null pointer"),
           (dict(bytes=NEED - 1), "bytes, %d needed" % NEED), (dict(bytes=0), "needed"), (dict(work=OK + 8), "work not 16-byte aligned"),
           (dict(gd=None), "gd and gw go together"), (dict(gw=None), "gd and gw go together"),
           (dict(gvel=None), "go together"), (dict(gmass=None, gstiff=None), "go together"),
           (dict(gforce=OK + 2), "misaligned operand"), (dict(ggain=OK + 4), "misaligned operand")]
CALLS, IDS = refusal_calls(("ds_contact_fwd", FWD), ("ds_contact_bwd", BWD), BAD, BAD_FWD, BAD_BWD, id_from=11, id_sep="-")


@pytest.mark.parametrize("fn,order,change,text", CALLS, ids=IDS)
def test_contact_arguments_are_checked_first(fn, order, change, text):
    """Every host-side refusal: DS_ERR_ARG and a message that names the entry point and the reason, in front of any launch."""
    assert_refused(fn, order, GOOD, change, text, status=1)


def test_contact_workspace_query_needs_no_device():
    lib = _hip_built().lib()
    assert lib.ds_contact_workspace_bytes(2, 3, 5, 4) == NEED
    assert lib.ds_contact_workspace_bytes(64, 64, 512, 8) == 16 * (64 * 4096 * 65 + 64 * 64)
    assert lib.ds_contact_workspace_bytes(65535, 512, 1 << 20, 1) == 16 * (65535 * (1 << 20) * 513 + 65535 * 512)  # beyond 2^32
    for a in [(0, 3, 5, 4), (65536, 3, 5, 4), (2, 0, 5, 4), (2, 513, 5, 4), (2, 3, 0, 4), (2, 3, 5, 0), (2, 3, 5, 65),
              (2, 3, (1 << 20) // 4 + 1, 4), (2, 3, 1 << 30, 64), (-1, 3, 5, 4)]:
        assert lib.ds_contact_workspace_bytes(*a) == 0


def test_python_layer_refuses_before_device_work():
    """The checks of ``contact_force`` need no device: ValueError on a CPU-only box, and RuntimeError for CPU tensors that
    pass them."""
    import torch

    from diffsound_amd.ddsp import HertzHammer, contact_force

    f64 = lambda *v: torch.tensor(v, dtype=torch.float64)  # noqa: E731
    good = dict(d=f64(3.0, 4.0), w=f64(3e3, 9e3), gain=torch.ones(2, 2, dtype=torch.float64), mass=f64(0.01, 0.01),
                velocity=f64(1.0, -1.0), stiffness=f64(1e7, 1e7), force_len=8, sr=44100.0)
    bad = [(dict(w=f64(3e3, 0.0)), "w must be positive"), (dict(w=f64(-3e3, 9e3)), "w must be positive"),
           (dict(mass=f64(0.01, 0.0)), "mass and stiffness"), (dict(stiffness=f64(-1e7, 1e7)), "mass and stiffness"),
           (dict(d=f64(3.0, float("nan"))), "d is not finite"), (dict(velocity=f64(float("inf"), 1.0)), "velocity is not finite"),
           (dict(gain=torch.full((2, 2), float("nan"), dtype=torch.float64)), "gain is not finite"),
           (dict(w=f64(3e3, 9e3, 1e4)), r"d and w must be \(m,\)"), (dict(gain=torch.ones(2, 3, dtype=torch.float64)), r"gain must be \(A, 2\)"),
           (dict(gain=torch.ones(2, dtype=torch.float64)), r"gain must be \(A, 2\)"), (dict(mass=f64(0.01)), r"mass must be \(2,\)"),
           (dict(velocity=f64(1.0, 1.0, 1.0)), r"velocity must be \(2,\)"), (dict(stiffness=torch.ones(2, 1, dtype=torch.float64)), r"stiffness must be \(2,\)"),
           (dict(d=torch.ones(513, dtype=torch.float64), w=torch.ones(513, dtype=torch.float64), gain=torch.ones(2, 513, dtype=torch.float64)),
            "outside 1..512"),
           (dict(oversample=0), "oversample = 0"), (dict(oversample=65), "oversample = 65"), (dict(force_len=0), "below 1"),
           (dict(force_len=(1 << 20) // 8 + 1), "substeps"), (dict(exponent=0.5), "exponent"), (dict(exponent=float("nan")), "exponent"),
           (dict(sr=0.0), "sr")]
    for change, text in bad:
        with pytest.raises(ValueError, match=text):
            contact_force(**dict(good, **change))
    with pytest.raises(RuntimeError, match="HIP device"):
        contact_force(**good)
    hammer = HertzHammer(2, 0.01, 1.0, 1e7)
    with pytest.raises(RuntimeError, match="HIP device"):
        hammer(good["d"], good["w"], good["gain"], 8, 44100.0)
    with pytest.raises(ValueError, match="must be positive"):
        HertzHammer(2, 0.0, 1.0, 1e7)
