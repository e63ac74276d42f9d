"""The sliding-contact entry points resolve on a CPU-only box, are declared in the header, bound in _hip and built by the
Makefile, and refuse bad arguments before any device work."""
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _cabi import CSRC, assert_refused, hip_built as _hip_built, refusal_calls, symbols_declared  # noqa: E402

NAMES = ("ds_osc_slide_workspace_bytes", "ds_osc_slide_fwd", "ds_osc_slide_bwd")


def test_osc_slide_symbols():
    header, slide = symbols_declared(NAMES, "osc_slide.hip")
    _hip = _hip_built()
    assert re.search(r"#define DS_OSC_SCAN_RUN 16\b", header)
    assert _hip.lib().ds_abi_version() == 45 == _hip.ABI_VERSION  # three added symbols, no bump
    driven, scan = (open(os.path.join(CSRC, n)).read() for n in ("osc_driven.hip", "osc_scan.h"))
    assert '#include "osc_scan.h"' in slide and '#include "osc_scan.h"' in driven
    for helper in ("struct cplx", "cplx cmul(", "cplx zpow(", "double from_prev(", "void load_run(", "cplx run_from_zero(",
                   "cplx scan_lanes(", "cplx lane_entry(", "cplx tile_exit(", "void join_waves(", "double frame_scan(",
                   "struct frame_pos"):
        assert helper in scan and helper not in driven and helper not in slide, helper
    sources = [n for n in sorted(os.listdir(CSRC)) if n.endswith((".hip", ".h", ".inc", ".cpp"))]
    assert [n for n in sources if "bool aligned(" in open(os.path.join(CSRC, n)).read()] == ["ds_common.h"]  # ds::aligned
    assert "atomic" not in slide.replace("No atomics", "").replace("no atomics", "")


OK = 1 << 20  # never dereferenced: the checks come first
GOOD = dict(gy=OK, d=OK, w=OK, amp=OK, force=OK, gain=OK, A=2, m=3, F=5, S=7, K=2, hop=16, sr=32000.0, work=OK, bytes=1 << 16,
            y=OK, gd=OK, gw=OK, gamp=OK, gforce=OK, ggain=OK)
FWD = ("d", "w", "amp", "force", "gain", "A", "m", "F", "S", "K", "hop", "sr", "work", "bytes", "y")
BWD = ("gy", "d", "w", "amp", "force", "gain", "A", "m", "F", "S", "K", "hop", "sr", "work", "bytes", "gd", "gw", "gamp", "gforce",
       "ggain")
BAD = [(dict(d=None), "null pointer"), (dict(w=None), "null pointer"), (dict(force=None), "null pointer"),
       (dict(gain=None), "null pointer"), (dict(work=None), "null pointer"),
       (dict(A=0), "empty problem"), (dict(A=-1), "empty problem"), (dict(m=0), "empty problem"), (dict(F=0), "empty problem"),
       (dict(S=0), "empty problem"), (dict(S=-3), "empty problem"), (dict(K=0), "empty problem"), (dict(K=-2), "empty problem"),
       (dict(A=65536), "above 65535"),
       (dict(hop=0), "not a positive multiple of 16"), (dict(hop=-16), "not a positive multiple of 16"),
       (dict(hop=24), "not a positive multiple of 16"), (dict(hop=17), "not a positive multiple of 16"),
       (dict(sr=0.0), "sr = 0"), (dict(sr=-1.0), "not positive"),
       (dict(bytes=16 * (2 * 3 + 2 * 3) - 1), "bytes, 192 needed"), (dict(work=OK + 8), "work not 16-byte aligned"),
       (dict(d=OK + 4), "misaligned operand"), (dict(w=OK + 4), "misaligned operand"), (dict(force=OK + 2), "misaligned operand"),
       (dict(gain=OK + 2), "misaligned operand"), (dict(amp=OK + 1), "misaligned operand")]
BAD_FWD = [(dict(y=None), "null pointer"), (dict(y=OK + 2), "misaligned operand")]
BAD_BWD = [(dict(gy=None), "null pointer"), (dict(gd=None), "null pointer"), (dict(gw=None), "null pointer"),
           (dict(gd=OK + 4), "gd or gw not 8-byte aligned"), (dict(gw=OK + 4), "gd or gw not 8-byte aligned"),
           (dict(gy=OK + 2), "misaligned operand"), (dict(gamp=OK + 2), "misaligned operand"),
           (dict(gforce=OK + 2), "misaligned operand"), (dict(ggain=OK + 2), "misaligned operand")]
CALLS, IDS = refusal_calls(("ds_osc_slide_fwd", FWD), ("ds_osc_slide_bwd", BWD), BAD, BAD_FWD, BAD_BWD, id_from=7)


@pytest.mark.parametrize("fn,order,change,text", CALLS, ids=IDS)
def test_osc_slide_arguments_are_checked_first(fn, order, change, text):
    """Every host-side refusal: a non-zero status and a message that names the entry point and the reason, in front of any
    launch."""
    assert_refused(fn, order, GOOD, change, text)


def test_osc_slide_workspace_query_needs_no_device():
    lib = _hip_built().lib()
    assert lib.ds_osc_slide_workspace_bytes(2, 3, 7, 2, 16) == 192
    assert lib.ds_osc_slide_workspace_bytes(8, 64, 8000, 125, 64) == 16 * (8 * 64 * 8 + 8 * 64)
    for a in [(0, 3, 7, 2, 16), (2, 0, 7, 2, 16), (2, 3, 0, 2, 16), (2, 3, 7, 0, 16), (2, 3, 7, 2, 0), (2, 3, 7, 2, 8), (2, 3, 7, 2, -16)]:
        assert lib.ds_osc_slide_workspace_bytes(*a) == 0


def test_python_layer_refuses_before_device_work():
    """The module-level checks of a 3-D mode_gain need no device: they raise ValueError on a CPU-only box."""
    import torch

    from diffsound_amd.ddsp.oscillator import DampedOscillator, GTDampedOscillator, TraditionalDampedOscillator
    from diffsound_amd.diffelastic.material_model import Material, MatSet

    mat = Material(MatSet.Ceramic)
    force = torch.zeros(2, 8)
    force[:, 0] = 1
    f_range = [100.0 * (i + 1) for i in range(8)]
    freq = torch.linspace(300.0, 900.0, 3).reshape(3, 1)
    gain3 = torch.ones(2, 4, 3)
    mods = [(TraditionalDampedOscillator(force, 2, 3, 64, 32000, mat), (freq,)),
            (DampedOscillator(force, 2, 3, 64, 32000, f_range, mat), (freq,)),
            (GTDampedOscillator(force, 2, 3, 64, 32000, f_range, mat), ())]
    for mod, args in mods:
        with pytest.raises(ValueError, match="needs gain_hop"):
            mod(*args, mode_gain=gain3)
        for hop in (24, 0, -16, 8):
            with pytest.raises(ValueError, match="multiple of 16"):
                mod(*args, mode_gain=gain3, gain_hop=hop)
        with pytest.raises(ValueError, match=r"must be \(2, K, 3\)"):
            mod(*args, mode_gain=torch.ones(2, 4, 5), gain_hop=16)
        with pytest.raises(ValueError, match="gain_hop goes with a 3-D"):
            mod(*args, mode_gain=torch.ones(2, 3), gain_hop=16)
    with pytest.raises(ValueError, match="non_linear_rate must be 0"):
        mods[2][0](non_linear_rate=0.5, mode_gain=gain3, gain_hop=16)
