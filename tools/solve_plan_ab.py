"""What single solves enqueue and return, one line per instance: the rows and the Phase-I instances of tests/test_gpu_solve_plan.py and
the fixtures lp_M, lp_C2 and EQ600.  A refactor of the engine's host code must print the same listing as its parent, field by field
(profiles/solve_plan_ab.log): run it once on each build and diff the two outputs."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.append(ROOT)   # (appended: a gomilp_amd earlier on the path — another build — wins)
sys.path.append(os.path.dirname(os.path.abspath(__file__)))

from gomilp_amd import lp, synth   # noqa: E402
import tests.test_gpu_solve_plan as T   # noqa: E402
from gen_golden import eqlp_problem   # noqa: E402

FIELDS = ["pivots_phase1", "pivots_phase2", "bland_steps", "art_exchanges", "kernel_launches", "cond_fallbacks"]


def line(name, problem, knobs):
    c, A, b = problem
    cx = lp.Context(**knobs)
    try:
        g = cx.upload(c, A, b).solve(0.0)
    finally:
        cx.close()
    x = "-" if g.x is None else hashlib.sha256(np.ascontiguousarray(g.x).tobytes()).hexdigest()[:16]
    print("%-44s status %s pipeline %s %s x %s" % (name, lp.STATUS_NAMES.get(g.status, g.status), g.stats["pipeline"],
                                                  " ".join("%s %d" % (f, g.stats[f]) for f in FIELDS), x), flush=True)


def main():
    for r in T.ROWS:
        line(T.row_id(r), T.problem(*r[:4]), T.run_knobs(r))
    for name in sorted(T.PHASE1):
        line("phase1-" + name, T.problem(*T.phase1_key(name)), T.PHASE1[name][3])
    line("lp_C2", synth.dense_lp_standard_form(1024, 1), {})
    line("lp_M", synth.dense_lp_standard_form(2048, 2), {})
    line("EQ600", eqlp_problem(5, 420, 300), {})


if __name__ == "__main__":
    main()
