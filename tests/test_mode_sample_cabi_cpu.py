"""The mode-sampling entry points resolve on a CPU-only box, are declared in the header, bound in _hip and built by the
Makefile, and refuse bad arguments before any device work."""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _mode_sample_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hip_built():
    from diffsound_amd import _hip

    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return _hip


def test_mode_sample_symbols():
    _hip = _hip_built()
    lib = _hip.lib()
    header = open(os.path.join(ROOT, "include", "diffsound_hip.h")).read()
    for name in ("ds_mode_sample_fwd", "ds_mode_sample_bwd"):
        assert name in _hip.EXPORTED_SYMBOLS and hasattr(lib, name)
        assert re.search(r"\b%s\s*\(" % name, header)
    assert "src/ddsp/oscillator.py:76" in header  # what the entry points stand in for
    assert "modesample.hip" in open(os.path.join(ROOT, "diffsound_amd", "csrc", "Makefile")).read()
    text = open(os.path.join(ROOT, "diffsound_amd", "csrc", "modesample.hip")).read()
    assert "NO GRADIENT TO U" in text and "the\n// caller's to check" in text
    assert "atomic" not in text.replace("no atomics", "").replace("No atomics", "")


def test_mode_sample_arguments_are_checked_first():
    assert R.check_refusals(_hip_built().lib()) >= 30


def test_impact_module_and_its_alias_import_without_a_device():
    import diffsound_amd.impact as a
    import src.diffelastic.impact as b

    assert a.ContactSurface is b.ContactSurface
