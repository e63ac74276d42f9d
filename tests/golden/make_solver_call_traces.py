"""Record tests/golden/solver_call_traces.json (tests/test_solver_cpu.py::test_call_traces_equal_the_recorded_ones) from the
solver as it stands:  python tests/golden/make_solver_call_traces.py  from the repository root.

A trace is the same on every machine only when no branch of the solves is decided by a near-tie, so the script also prints, for
every solver that ran (the nested start's corner-node solver included), eps * amp of every orthonormalisation sweep against
SolverConfig.ortho_tol and every tested backward error against the tolerance.  It refuses to write when an eps * amp is within
a factor 2 of ortho_tol, or a backward error within 5 % of its tolerance (the corner-node solve of a nested start runs until
its pairs have passed the tolerance; machines differ in the last digits of these numbers, not in their first).
As recorded: eps * amp / ortho_tol <= 0.05 in the one-level cases (a factor 20 away); in the nested cases the corner-node
phase's swept start block gives 0.35 and the sweeps after it <= 0.17 - a block that went through two preconditioner sweeps is
that ill-conditioned whatever the seed (seeds 0 ... 15: 0.21 ... 0.51), so another seed does not buy a wider margin there."""
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from diffsound_amd.lobpcg import modal_solver as ms  # noqa: E402
from tests import test_solver_cpu as T  # noqa: E402


def main():
    torch.set_num_threads(1)
    cube = getattr(T.cube, "__wrapped__", None) or T.cube.__pytest_wrapped__.obj  # (the fixture's function)
    cube = cube()
    mp = pytest.MonkeyPatch()
    margins = []

    def watch(method):
        inner = getattr(ms.ModalSolver, method)

        def run(self, k, *a, **kw):
            user, rels = kw.get("tracker"), []

            def tracker(state):
                rels.append(state.tvars["rerr"].clone())
                if user is not None:
                    user(state)

            kw["tracker"] = tracker
            res = inner(self, k, *a, **kw)
            eps = 6e-8 if self.ops.dtype == torch.float32 else 1.1e-16
            tol = self.cfg.tol or (2e-6 if self.ops.dtype == torch.float32 else 1e-10)
            margins.extend(("ortho", eps * amp / self.cfg.ortho_tol) for amp in self.ortho_log)
            margins.extend(("rerr", float(r) / tol) for rel in rels for r in rel)
            print(f"  {method} on {getattr(self.ops, 'level', '') or 'fine'}: iterations {res.iterations}, eps * amp / ortho_tol",
                  [f"{eps * amp / self.cfg.ortho_tol:.3g}" for amp in self.ortho_log])
            print("    rerr / tol per tested step:", [[f"{float(r) / tol:.3g}" for r in rel] for rel in rels])
            return res

        mp.setattr(ms.ModalSolver, method, run)

    watch("solve")
    watch("solve_basic")
    traces = T._call_traces(cube, mp, report=lambda case, solver: print(case))
    mp.undo()
    close = [(what, ratio) for what, ratio in margins if (0.5 < ratio < 2.0 if what == "ortho" else 1 / 1.05 < ratio < 1.05)]
    if close:
        raise SystemExit(f"too close to a threshold: {close}")
    with open(os.path.join(ROOT, "tests", "golden", "solver_call_traces.json"), "w") as f:
        json.dump(traces, f, separators=(",", ":"))
        f.write("\n")
    print({case: len(tr) for case, tr in traces.items()})


if __name__ == "__main__":
    main()
