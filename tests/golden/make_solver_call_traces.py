"""Record tests/golden/solver_call_traces.json (tests/test_solver_cpu.py::test_call_traces_equal_the_recorded_ones) from the
solver as it stands:  python tests/golden/make_solver_call_traces.py  from the repository root.

A trace is the same on every machine only when no branch of the solves is decided by a near-tie, so the script also prints, for
every solver that ran (the nested start's corner-node solver included), eps * amp of every orthonormalisation sweep against
SolverConfig.ortho_tol and every tested backward error against the tolerance.  It refuses to write when an eps * amp is within
a factor 2 of ortho_tol, or a backward error within 5 % of its tolerance (the corner-node solve of a nested start runs until
its pairs have passed the tolerance; machines differ in the last digits of these numbers, not in their first).
As recorded: eps * amp / ortho_tol <= 0.05 in the one-level cases (a factor 20 away); in the nested cases the corner-node
phase's swept start block gives 0.35 and the sweeps after it <= 0.17 - a block that went through two preconditioner sweeps is
that ill-conditioned whatever the seed (seeds 0 ... 15: 0.21 ... 0.51), so another seed does not buy a wider margin there.

The two refinement cases (solve_refine, solve_refine_fused) were recorded at commit de106a6 ("Split ddsp/oscillator.py; say the
oscillator-bank plumbing once"), the parent of the change that moved ModalSolver.refine64 into lobpcg/refine.py: the test holds
the phases there to the calls of the one method before it.  Their fp32 phase runs to convergence, so the 5 % rule above covers
it; for the fp64 steps the script prints rel / (0.3 * refine_tol) of every column at every step that chooses an active set (the
soft locking's threshold) and refuses within a factor 2 of 1.  It forms these backward errors itself, from the blocks X, K X,
M X that the solver's mix64 calls return and the Rayleigh quotients of their columns - a margin needs no more digits than that,
and no hook into the refinement's code.
The two cases run with seed 4, not the default 0: with seed 0 the fp32 phase tests a backward error at 0.967 and one at 1.04
times its tolerance, inside the 5 % rule; of the seeds 1 ... 8 only 2, 4 and 8 keep every tested value further away (1.063, 1.084,
1.055 as the closest factor), seed 2 has an eps * amp / ortho_tol of 0.51, and 4 has the widest margin of the rest (0.29 there).
As recorded: 15 fp32 iterations; fp64 history 1.45e-6, 2.65e-7, 1.05e-7, 2.72e-8; rel / (0.3 refine_tol) between 32 and 1.9e6
(a converged fp32 block sits orders of magnitude above the fp64 tolerance), so all 24 columns are active in all three steps;
step 0 forms the pencil from the vectors, steps 1 and 2 by recurrence."""
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

    def watch_refinement(solver):
        """Backward errors of the fp64 blocks as they appear: outside the P updates (whose blocks name their rows) the mix64
        calls return X, K X, M X in turn."""
        ops, held, steps, norms = solver.ops, [], [], []
        inner = ops.mix64

        def mix64(blocks, C, out=None, **kw):
            got = inner(blocks, C, out=out, **kw)
            if not any(isinstance(blk, tuple) for blk in blocks):
                held.append(got)
            if len(held) == 3:
                X, KX, MX = held
                del held[:]
                lam = (X * KX).sum(0) / (X * MX).sum(0)
                R = KX - MX * lam[None, :]
                An, Bn = norms
                steps.append(torch.linalg.vector_norm(R, dim=0) / (torch.linalg.vector_norm(X, dim=0) * (An + lam.abs() * Bn)))
            return got

        ops.mix64 = mix64
        inner64 = solver.refine64

        def refine64(res, k_, A_norm, B_norm):
            norms[:] = A_norm, B_norm
            out = inner64(res, k_, A_norm, B_norm)
            ratios = [[float(r) / (0.3 * solver.cfg.refine_tol) for r in rel] for rel in steps[:-1]]  # (the last step chooses nothing)
            print("    fp64 steps", out.refine_iterations, "history", [f"{h:.3g}" for h in out.refine_history])
            for it, row in enumerate(ratios):
                print(f"    step {it}: rel / (0.3 refine_tol) min {min(row):.3g} max {max(row):.3g}", [f"{r:.3g}" for r in row])
            margins.extend(("refine", r) for row in ratios for r in row)
            return out

        solver.refine64 = refine64

    def watch(method):
        inner = getattr(ms.ModalSolver, method)

        def run(self, k, *a, **kw):
            user, rels = kw.get("tracker"), []

            def tracker(state):
                rels.append(state.tvars["rerr"].clone())
                if user is not None:
                    user(state)

            kw["tracker"] = tracker
            if method == "solve" and self.cfg.refine_tol > 0.0:
                watch_refinement(self)
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
    close = [(what, ratio) for what, ratio in margins if (1 / 1.05 < ratio < 1.05 if what == "rerr" else 0.5 < ratio < 2.0)]
    if close:
        raise SystemExit(f"too close to a threshold: {close}")
    with open(os.path.join(ROOT, "tests", "golden", "solver_call_traces.json"), "w") as f:
        json.dump(traces, f, separators=(",", ":"))
        f.write("\n")
    print({case: len(tr) for case, tr in traces.items()})


if __name__ == "__main__":
    main()
