"""Times general starts beyond the tableau's LDS row (n - m > 8191): the guarded three-kernel revised loop.
Per shape: ms per solve (median of the timed runs, after one warm-up), pivots of both phases, exact steps (stats cond_fallbacks),
ms per pivot.  Equality-form LPs of tests/test_gpu_wide_general.py eqlp: 160 x 9060 and 1000 x 12000.

    python tools/wide_general_time.py [--runs 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gomilp_amd import lp  # noqa: E402
from oracle import oracle as O  # noqa: E402

SHAPES = [("160x9060", 1, 9000, 100, 60), ("1000x12000", 2, 11500, 500, 500)]


def eqlp(seed, N, E, I):
    """E Gaussian equality rows, I inequality rows over N variables (tools/gen_golden.py eqlp_problem with separate row counts)"""
    rng = np.random.default_rng(seed)
    x0 = np.abs(rng.standard_normal(N))
    A = rng.standard_normal((E, N)); b = A @ x0
    G = rng.standard_normal((I, N)); h = G @ x0 + np.abs(rng.standard_normal(I))
    c = np.abs(rng.standard_normal(N))
    return O.convert_to_equalities(c, A, b, G, h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    args = ap.parse_args()
    for name, seed, N, E, I in SHAPES:
        c, A, b = eqlp(seed, N, E, I)
        cx = lp.Context()
        try:
            p = cx.upload(c, A, b)
            g = p.solve(0.0)   # warm-up: allocations, first launches
            ms = []
            for _ in range(args.runs):
                t0 = time.perf_counter()
                g = p.solve(0.0)
                ms.append(1e3 * (time.perf_counter() - t0))
        finally:
            cx.close()
        pivots = g.stats["pivots_phase1"] + g.stats["pivots_phase2"]
        med = float(np.median(ms))
        print(json.dumps({"shape": name, "m": A.shape[0], "n": A.shape[1], "status": lp.STATUS_NAMES.get(g.status, g.status),
                          "pipeline": g.stats["pipeline"], "ms_per_solve": round(med, 2), "ms_runs": [round(v, 2) for v in ms],
                          "pivots": [g.stats["pivots_phase1"], g.stats["pivots_phase2"]], "exact_steps": g.stats["cond_fallbacks"],
                          "ms_per_pivot": round(med / max(1, pivots), 4), "z": g.z}), flush=True)


if __name__ == "__main__":
    main()
