"""The built ds_geometry_grad_tangent kernels use no scratch memory.  The ord-2 instantiation sits at the 256-VGPR ceiling:
it stays out of scratch only because the 81 entries of C + C^T are LDS operands of every quadrature point and not a
register-resident table (a compiler-level barrier in csrc/geomgrad.hip keeps the reads inside the loop).  A compiler that
schedules differently would bring the spills back without any wrong number, so the shipped binary's metadata is checked."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

from test_cabi_cpu import _gfx950_code_objects  # noqa: E402


def test_tangent_kernels_use_no_scratch(tmp_path):
    readelf = shutil.which("llvm-readelf") or "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not os.path.exists(readelf):
        pytest.skip("llvm-readelf not found")
    from diffsound_amd import _hip

    objs = [b for b in _gfx950_code_objects(_hip.LIB_PATH) if b"geometry_grad_tangent_kernel" in b]
    assert len(objs) == 1  # csrc/geomgrad.hip
    path = tmp_path / "geomgrad.o"
    path.write_bytes(objs[0])
    notes = subprocess.run([readelf, "--notes", str(path)], capture_output=True, text=True, check=True).stdout
    seen = {}
    for entry in notes.split(".agpr_count:")[1:]:  # one metadata record per kernel, its keys in alphabetical order
        name = re.search(r"\.name:\s+(\S+)", entry).group(1)
        if "geometry_grad_tangent_kernel" in name or "geometry_grad_gather_kernel" in name:
            seen[name] = {k: int(re.search(rf"\.{k}:\s+(\d+)", entry).group(1))
                          for k in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count", "vgpr_count")}
    print(seen)
    assert len(seen) == 3  # the ord-1 and the ord-2 element kernel, the per-node sum
    for name, r in seen.items():
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (name, r)
