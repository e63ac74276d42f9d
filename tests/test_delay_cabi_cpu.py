"""The delay-line entry points resolve on a CPU-only box, are declared in the header, bound in _hip and built by the
Makefile, and refuse bad arguments before any device work."""
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _cabi import assert_refused, hip_built as _hip_built, refusal_calls, symbols_declared  # noqa: E402

NAMES = ("ds_delay_workspace_bytes", "ds_delay_fwd", "ds_delay_bwd")


def test_delay_symbols():
    header, src = symbols_declared(NAMES, "delay.hip")
    _hip = _hip_built()
    assert re.search(r"#define DS_DELAY_HALF_TAPS 8\b", header) and re.search(r"#define DS_DELAY_MAX_SLOPE 0\.5\b", header)
    assert re.search(r"#define DS_DELAY_MAX_ROWS 65535\b", header)
    assert _hip.lib().ds_abi_version() == 45 == _hip.ABI_VERSION  # three added symbols, no bump
    assert "atomic" not in src.replace("No atomics", "").replace("no atomics", "")
    # what the header promises for every tau is said where the caller reads it
    for text in ("before any conversion to", "outside [-R, S + R) yields y = 0", "non-finite tau(t) yields y = NaN", "stays inside [0, S)"):
        assert text in header, text


OK = 1 << 20  # never dereferenced: the checks come first
GOOD = dict(gy=OK, s=OK, tau=OK, B=2, S=7, K=2, hop=16, work=OK, bytes=1 << 16, y=OK, gs=OK, gtau=OK)
FWD = ("s", "tau", "B", "S", "K", "hop", "y")
BWD = ("gy", "s", "tau", "B", "S", "K", "hop", "work", "bytes", "gs", "gtau")
BAD = [(dict(s=None), "null pointer"), (dict(tau=None), "null pointer"),
       (dict(B=0), "empty problem"), (dict(B=-1), "empty problem"), (dict(S=0), "empty problem"), (dict(S=-3), "empty problem"),
       (dict(K=0), "empty problem"), (dict(K=-2), "empty problem"), (dict(B=65536), "B = 65536 above 65535"),
       (dict(hop=0), "hop = 0 is not positive"), (dict(hop=-16), "hop = -16 is not positive"),
       (dict(s=OK + 2), "misaligned operand"), (dict(tau=OK + 4), "misaligned operand")]
BAD_FWD = [(dict(y=None), "null pointer"), (dict(y=OK + 2), "misaligned operand")]
BAD_BWD = [(dict(gy=None), "null pointer"), (dict(work=None), "null pointer"),
           (dict(bytes=8 * 2 * 7 - 1), "bytes, 112 needed"), (dict(work=OK + 8), "work not 16-byte aligned"),
           (dict(gy=OK + 2), "misaligned operand"), (dict(gs=OK + 2), "misaligned operand"), (dict(gtau=OK + 4), "misaligned operand")]
# the order of the refusals: the earlier reason wins where two are wrong
ORDER = [(dict(s=None, B=0), "null pointer"), (dict(B=0, hop=0), "empty problem"), (dict(B=65536, hop=0), "above 65535"),
         (dict(hop=0, s=OK + 2), "is not positive")]
ORDER_BWD = [(dict(hop=0, bytes=1), "is not positive"), (dict(bytes=1, work=OK + 8), "112 needed"),
             (dict(work=OK + 8, gs=OK + 2), "work not 16-byte aligned")]
CALLS, IDS = refusal_calls(("ds_delay_fwd", FWD), ("ds_delay_bwd", BWD), BAD, BAD_FWD, BAD_BWD, ORDER, ORDER_BWD)


@pytest.mark.parametrize("fn,order,change,text", CALLS, ids=IDS)
def test_delay_arguments_are_checked_first(fn, order, change, text):
    """Every host-side refusal: a non-zero status and a message that names the entry point and the reason, in front of any
    launch."""
    assert_refused(fn, order, GOOD, change, text)


def test_delay_workspace_query_needs_no_device():
    lib = _hip_built().lib()
    assert lib.ds_delay_workspace_bytes(2, 7, 2, 16) == 112
    assert lib.ds_delay_workspace_bytes(65535, 1 << 20, 3, 48) == 8 * 65535 * (1 << 20)
    for a in [(0, 7, 2, 16), (-1, 7, 2, 16), (65536, 7, 2, 16), (2, 0, 2, 16), (2, 7, 0, 16), (2, 7, 2, 0), (2, 7, 2, -16)]:
        assert lib.ds_delay_workspace_bytes(*a) == 0


def test_python_layer_refuses_before_device_work():
    """The checks of ``propagate`` and of ``listener_delay`` that need no device raise ValueError on a CPU-only box."""
    import torch

    from diffsound_amd.ddsp.delay import propagate
    from diffsound_amd.ddsp.oscillator import DampedOscillator, GTDampedOscillator, TraditionalDampedOscillator
    from diffsound_amd.diffelastic.material_model import Material, MatSet

    s, tau = torch.zeros(2, 3, 40), torch.zeros(3, 4)
    for hop in (0, -16, 16.0, "16", True, None):
        with pytest.raises(ValueError, match="not a positive int"):
            propagate(s, tau, hop)
    with pytest.raises(ValueError, match="signal must be a floating-point tensor"):
        propagate(torch.zeros(2, 40, dtype=torch.int32), tau, 16)
    with pytest.raises(ValueError, match="delay must be a floating-point tensor"):
        propagate(s, [[0.0]], 16)
    with pytest.raises(ValueError, match="does not broadcast"):
        propagate(s, torch.zeros(2, 4), 16)
    with pytest.raises(ValueError, match="does not broadcast"):
        propagate(s, torch.zeros(5, 2, 3, 4), 16)
    with pytest.raises(ValueError, match=r"signal must be \(\.\.\., S\)"):
        propagate(torch.zeros(2, 0), torch.zeros(2, 1), 16)
    with pytest.raises(ValueError, match=r"delay must be \(\.\.\., K\)"):
        propagate(s, torch.zeros(3, 0), 16)
    with pytest.raises(ValueError, match="at most 65535"):
        propagate(torch.zeros(65536, 1), torch.zeros(1), 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        propagate(s, tau, 16)

    mat = Material(MatSet.Ceramic)
    force = torch.zeros(2, 8)
    force[:, 0] = 1
    f_range = [100.0 * (i + 1) for i in range(8)]
    freq = torch.linspace(300.0, 900.0, 3).reshape(3, 1)
    rest, moving = torch.ones(2, 3, dtype=torch.complex64), torch.ones(2, 3, 4, dtype=torch.complex64)
    mods = [(TraditionalDampedOscillator(force, 2, 3, 64, 32000, mat), (freq,)),
            (DampedOscillator(force, 2, 3, 64, 32000, f_range, mat), (freq,)),
            (GTDampedOscillator(force, 2, 3, 64, 32000, f_range, mat), ())]
    for mod, args in mods:
        with pytest.raises(ValueError, match="listener_delay goes with a listener_gain"):
            mod(*args, listener_delay=torch.zeros(2, 1))
        with pytest.raises(ValueError, match="4 frames, listener_gain has K = 1"):
            mod(*args, listener_gain=rest, listener_delay=torch.zeros(2, 4))
        with pytest.raises(ValueError, match="3 frames, listener_gain has K = 4"):
            mod(*args, listener_gain=moving, listener_hop=16, listener_delay=torch.zeros(2, 3))
        for bad in (torch.zeros(3, 4), torch.zeros(4), torch.zeros(3, 2, 4), torch.zeros(2, 2, 2, 4), [[0.0] * 4] * 2,
                    torch.zeros(2, 4, dtype=torch.int64)):
            with pytest.raises(ValueError, match=r"\(C, K\) or \(2, C, K\) tensor with C = 2"):
                mod(*args, listener_gain=moving, listener_hop=16, listener_delay=bad)
