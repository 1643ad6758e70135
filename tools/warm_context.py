"""Developer tool: per-node cold and warm time of the single-context warm start (gomilp_lp_solve_warm) on the two
branch children of a kept root — setup (child B^-1, x_B, y from the parent's state), dual loop, finish (Phase-II confirmation + the
final solve), against the cold solve of the same child.
usage: warm_context.py [m,nv ...]   (default: 2048,2048 and 8200,16400 — the 2048 x 4096 and 8200 x 24600 slack roots)"""
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from gomilp_amd import lp  # noqa: E402
from tests.test_gpu_large_rows import _gen  # noqa: E402

shapes = [tuple(int(v) for v in a.split(",")) for a in sys.argv[1:]] or [(2048, 2048), (8200, 16400)]
for m, nv in shapes:
    c, A, b = _gen(m, nv, 0)
    cx = lp.Context()
    try:
        root = cx.upload(c, A, b)
        r0 = root.solve(keep=True)
        print("%d x %d root: status %d, %d pivots, %.3f s, state kept %d (%.0f MB)" % (
            m, nv + m, r0.status, r0.stats["pivots_phase1"] + r0.stats["pivots_phase2"], r0.stats["seconds_total"],
            r0.stats["warm"]["kept"], r0.stats["warm"]["keep_bytes"] / 1e6), flush=True)
        f = np.abs(r0.x[:nv] - np.round(r0.x[:nv]))
        j = int(np.argmax(f))
        fl = math.floor(r0.x[j])
        for row in ((j, 1.0, float(fl)), (j, -1.0, -float(fl + 1))):
            ch = root.child([row])
            cold = ch.solve()
            w = ch.solve(parent=root)
            ws, st = w.stats["warm"], w.stats
            finish = st["seconds_total"] - ws["seconds_setup"] - ws["seconds_dual"]
            print("  child x_%d %s %g: cold %d pivots %.2f ms | warm %d dual + %d primal pivots, setup %.2f ms, dual %.2f ms (%.1f us / pivot), "
                  "finish %.2f ms (final solve %.2f ms), total %.2f ms | status %d / %d, |dz| %.1e" % (
                      j, "<=" if row[1] > 0 else ">=", row[2] * row[1], cold.stats["pivots_phase1"] + cold.stats["pivots_phase2"],
                      1e3 * cold.stats["seconds_total"], ws["pivots_dual"], st["pivots_phase2"], 1e3 * ws["seconds_setup"], 1e3 * ws["seconds_dual"],
                      1e6 * ws["seconds_dual"] / max(1, ws["pivots_dual"]), 1e3 * finish, 1e3 * st["seconds_final_solve"], 1e3 * st["seconds_total"],
                      w.status, cold.status, abs(w.z - cold.z) if w.status == 0 else 0.0), flush=True)
            ch.free()
    finally:
        cx.close()
