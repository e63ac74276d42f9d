"""The point-cloud entry points of ABI 45 resolve on a CPU-only box, are declared in the header and bound in _hip, and
refuse bad arguments before any device work."""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _cabi import hip_built as _hip_built, symbols_declared  # noqa: E402


def test_spec_points_symbols_and_abi():
    header, _ = symbols_declared(("ds_spec_points_fwd", "ds_spec_points_bwd"), "specpoints.hip")
    _hip = _hip_built()
    assert re.search(r"#define DS_ABI_VERSION 45\b", header)
    assert _hip.ABI_VERSION == 45 and _hip.lib().ds_abi_version() == 45
    assert "src/ddsp/mss_loss.py:19-48, 104-117" in header


def test_spec_points_arguments_are_checked_first():
    """Every refusal happens in front of the first launch: null pointers, shapes, a frequency list without its table."""
    _hip = _hip_built()
    lib = _hip.lib()
    fake = 1 << 20  # never dereferenced: the checks come first
    assert lib.ds_spec_points_fwd(None, 1, 33, 3, 1e-7, 33, None, 0, 0, None, fake, fake, None) == 1
    assert b"null pointer" in lib.ds_last_error()
    assert lib.ds_spec_points_fwd(fake, 1, 33, 3, 1e-7, 34, None, 0, 0, None, fake, fake, None) == 1
    assert b"fclip" in lib.ds_last_error()
    assert lib.ds_spec_points_fwd(fake, 1, 33, 0, 1e-7, 33, None, 0, 0, None, fake, fake, None) == 1
    assert b"T = 0" in lib.ds_last_error()
    assert lib.ds_spec_points_fwd(fake, 1, 33, 3, 0.0, 33, None, 0, 0, None, fake, fake, None) == 1
    assert b"eps" in lib.ds_last_error()
    assert lib.ds_spec_points_fwd(fake, 1, 33, 3, 1e-7, 33, fake, 4, 32000, None, fake, fake, None) == 1
    assert b"winner table" in lib.ds_last_error()
    assert lib.ds_spec_points_fwd(fake, 1, 33, 3, 1e-7, 33, None, 0, 0, None, fake + 4, fake, None) == 1
    assert b"aligned" in lib.ds_last_error()
    assert lib.ds_spec_points_fwd(fake, 1, 33, 3, 1e-7, 33, fake, 0, 32000, fake, fake, fake, None) == 1
    assert b"E = 0" in lib.ds_last_error()
    assert lib.ds_spec_points_fwd(fake, 1, 33, 3, 1e-7, 33, fake, 4, 1, fake, fake, fake, None) == 1
    assert b"sample_rate" in lib.ds_last_error()
    assert lib.ds_spec_points_bwd(fake, fake, 1, 33, 33, None, 4, 32000, fake, 1.0, fake, None) == 1
    assert b"null pointer" in lib.ds_last_error()
    assert lib.ds_spec_points_bwd(fake, fake, 1, 33, 0, fake, 4, 32000, fake, 1.0, fake, None) == 1
    assert b"fclip" in lib.ds_last_error()
