"""The mode-sampling entry points resolve on a CPU-only box, are declared in the header, bound in _hip and built by the
Makefile, and refuse bad arguments before any device work."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _mode_sample_ref as R  # noqa: E402
from _cabi import hip_built as _hip_built, symbols_declared  # noqa: E402


def test_mode_sample_symbols():
    header, text = symbols_declared(("ds_mode_sample_fwd", "ds_mode_sample_bwd"), "modesample.hip")
    assert "src/ddsp/oscillator.py:76" in header  # what the entry points stand in for
    assert "NO GRADIENT TO U" in text and "the\n// caller's to check" in text
    assert "atomic" not in text.replace("no atomics", "").replace("No atomics", "")


def test_mode_sample_arguments_are_checked_first():
    assert R.check_refusals(_hip_built().lib()) >= 30


def test_impact_module_and_its_alias_import_without_a_device():
    import diffsound_amd.impact as a
    import src.diffelastic.impact as b

    assert a.ContactSurface is b.ContactSurface
