"""Developer tool (not run by the tests): waves of 2, 4 and 8 one-row children of an 8200 x 24648 slack-basis root through a frontier
pool with large_rows = 1 (the batched revised simplex in its chunked kernels), against the same children one after the other on a
single context, cold and warm.  Both paths run under the same pivot budget (the cold solves of these children take ~9500 pivots of
~0.6 ms each; the budget keeps the run short and the work equal: the two paths take the same pivots).

usage: large_pool_timing.py [pivot budget, default 2000] [log file, default profiles/large_pool_timing.log] [wave sizes, default 2,4,8]"""
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from gomilp_amd import lp  # noqa: E402

BUDGET = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
LOG = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "large_pool_timing.log")
COUNTS = [int(v) for v in sys.argv[3].split(",")] if len(sys.argv) > 3 else [2, 4, 8]
M0, NV, NCOST, DUAL = 8200, 16448, 48, 256
_log = open(LOG, "w")


def say(s):
    print(s, flush=True)
    _log.write(s + "\n")
    _log.flush()


def gen(m, nv):
    """min c^T x, G x <= h, x >= 0 as [G | I]: G small non-negative integers, h = 2 * rowsum + 1, c non-zero on NCOST columns"""
    rng = np.random.default_rng(91000 + 31 * m)
    G = rng.integers(0, 3, (m, nv), dtype=np.int8)
    h = 2.0 * G.sum(axis=1, dtype=np.int64) + 1.0
    c = np.zeros(nv + m)
    c[rng.choice(nv, NCOST, replace=False)] = -rng.integers(1, 10, NCOST).astype(float)
    A = np.zeros((m, nv + m))
    A[:, :nv] = G
    A[np.arange(m), nv + np.arange(m)] = 1.0
    return c, A, h


say("large_pool_timing: root %d x %d, pivot budget %d, dual budget %d" % (M0, NV + M0, BUDGET, DUAL))
c, A, b = gen(M0, NV)

pool = lp.FrontierPool(workers=1, large_rows=1, warm_revised=1)
pool.set_root(c, A, b)
t0 = time.perf_counter()
r0 = pool.solve_warm([[]], tags=[0], keep=[1])
say("pool: root solved and kept in %.2f s: status %s, pivots %d, warm_kept %d, batched %d" % (
    time.perf_counter() - t0, lp.STATUS_NAMES.get(int(r0.status[0])), r0.stats["pivots_phase2"], r0.stats["warm_kept"], r0.stats["batched_relaxations"]))
xs = r0.x[0][:NV]
top = [int(j) for j in np.argsort(-xs)[:4]]
pairs = []
for j in top:   # a bound that cuts the root's point off, and its complement
    fl = float(math.floor(xs[j] / 2))
    pairs += [[(j, 1.0, fl)], [(j, -1.0, -(fl + 1.0))]]
pool.set("max_pivots", BUDGET)

cx = lp.Context(max_pivots=0)
root = cx.upload(c, A, b)
t0 = time.perf_counter()
g0 = root.solve(0.0, keep=True)
say("context: root solved and kept in %.2f s: status %s, pivots %d" % (time.perf_counter() - t0, lp.STATUS_NAMES.get(g0.status), g0.stats["pivots_phase2"]))
cx.set("max_pivots", BUDGET)

for count in COUNTS:
    wave = pairs[:count]
    for mode in ("cold", "warm"):
        t0 = time.perf_counter()
        if mode == "cold":
            r = pool.solve(wave)
        else:
            r = pool.solve_warm(wave, parents=[0] * count, tags=list(range(1, 1 + count)), keep=[0] * count, dual_budget=DUAL)
        tp = time.perf_counter() - t0
        s = r.stats
        t0 = time.perf_counter()
        piv = pivd = 0
        same = True
        for i, rows in enumerate(wave):
            ch = root.child(rows)
            g = ch.solve(0.0, parent=root, dual_budget=DUAL) if mode == "warm" else ch.solve(0.0)
            ch.free()
            piv += g.stats["pivots_phase1"] + g.stats["pivots_phase2"]
            pivd += g.stats["warm"]["pivots_dual"] if mode == "warm" and "pivots_dual" in g.stats.get("warm", {}) else 0
            same = same and g.status == r.status[i] and (mode == "warm" or np.float64(g.z).tobytes() == np.float64(r.z[i]).tobytes())
        tc = time.perf_counter() - t0
        say("%d children %s: pool %.3f s (batched %d, host_fallbacks %d, supersteps %d, pivots %d + %d, dual %d, warm_started %d, warm_fallbacks %d, "
            "schedule %.3f s) | context, one after the other %.3f s (pivots %d, dual %d) | pool / context %.2f | statuses%s equal: %s" % (
                count, mode, tp, s["batched_relaxations"], s["host_fallbacks"], s["supersteps"], s["pivots_phase1"], s["pivots_phase2"], s["pivots_dual"],
                s["warm_started"], s["warm_fallbacks"], s["seconds_batch"], tc, piv, pivd, tp / tc, "" if mode == "warm" else " and z bits", same))
pool.close()
cx.close()
_log.close()
