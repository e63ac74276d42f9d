"""Record tests/golden/ops_call_traces.json (tests/test_ops_calls_cpu.py::test_call_traces_equal_the_recorded_ones):
python tests/golden/make_ops_call_traces.py  from the repository root, with the library built.

The committed record was taken at commit 41a941e ("Split ModalSolver.solve into named phases shared with solve_basic"), the
parent of the change that split diffsound_amd/modal_ops.py into modal_ops.py and block_ops.py: the test holds the reorganised
operator layer to the launches of the layer before it.  Record it again only for a change that is meant to alter a launch."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import test_ops_calls_cpu as T  # noqa: E402


def main():
    mp = pytest.MonkeyPatch()
    try:
        traces = T.call_traces(mp)
    finally:
        mp.undo()
    with open(T.GOLDEN, "w") as f:
        json.dump(traces, f, separators=(",", ":"))
        f.write("\n")
    print({case: len(tr) for case, tr in traces.items()})


if __name__ == "__main__":
    main()
