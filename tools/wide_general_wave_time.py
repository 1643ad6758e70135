#!/usr/bin/env python3
"""Wide waves of equality-form roots (no slack basis) on the batched revised simplex (pool knob rev_general, DESIGN.md section 2.5e
"Equality-form roots"; 2: every size up to 300 rows) against the same calls with the knob at 0 (the workers), same process, same pool, the variants taken in turn:
median of five calls after one warm-up.

    python tools/wide_general_wave_time.py [--log FILE]      (default FILE: profiles/wide_general_wave_time.log; the lines go to stdout too)

Waves: the 24 children (12 down, 12 up branches on the first 12 nonzero structural variables of the root optimum) of the two 80 x 316
roots of tests/test_gpu_wide_general_frontier.py, and up to 24 children of a 160 x 600 and of a 299 x 1139 root (variables with a root value
above 1, so that no branch row has a zero right-hand side: those children are degenerate, take thousands of Bland steps on a worker on
either path and would be the whole timing).  Seconds are host-clock around calls that return results, i.e. end in a device synchronise."""
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOG = os.path.join(ROOT, "profiles", "wide_general_wave_time.log")
if "--log" in sys.argv:
    i = sys.argv.index("--log")
    LOG = os.path.abspath(sys.argv[i + 1])
    del sys.argv[i:i + 2]
sys.path.insert(0, ROOT)

from gomilp_amd import lp
from tests.test_gpu_wide_general import eqlp

_log = None


def say(line):
    print(line, flush=True)
    if _log:
        _log.write(line + "\n")
        _log.flush()


def branches(x, picks):
    return [[(j, 1, float(math.floor(x[j])))] for j in picks] + [[(j, -1, -float(math.ceil(x[j])))] for j in picks]


WAVES = [
    ("80 x 316, Phase I", (1, 260, 24, 56, False), lambda x: [j for j in range(260) if x[j] != 0][:12]),
    ("80 x 316, feasible start", (2, 260, 24, 56, True), lambda x: [j for j in range(260) if x[j] != 0][:12]),
    ("160 x 600, Phase I", (5, 480, 40, 120, False), lambda x: [j for j in range(440) if x[j] > 1 and x[j] != math.floor(x[j])][:12]),
    ("299 x 1139, Phase I", (4, 900, 60, 239, False), lambda x: [j for j in range(840) if x[j] > 1 and x[j] != math.floor(x[j])][:12]),
]


def main():
    global _log
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    _log = open(LOG, "w")
    say("wide_general_wave_time: rev_general = 2 against 0, median of five")
    say("| root | children | rev_general | s / wave | relaxations / s | supersteps | launches | batched | host_fallbacks | share handed over | pivots |  # calls")
    say("|---|---|---|---|---|---|---|---|---|---|---|")
    for name, args, pick in WAVES:
        pool = lp.FrontierPool(workers=8)
        c, A, b = eqlp(*args)
        pool.set_root(c, A, b)
        r = pool.solve_root(0.0)
        assert r.status == lp.OK, r.status
        wave = branches(r.x, pick(r.x))
        n = len(wave)
        ts, last = {2: [], 0: []}, {}
        for knob in (2, 0):
            pool.set("rev_general", knob)
            pool.solve(wave)   # warm-up
        for _ in range(5):
            for knob in (2, 0):
                pool.set("rev_general", knob)
                t0 = time.perf_counter()
                last[knob] = pool.solve(wave)
                ts[knob].append(time.perf_counter() - t0)
        same = all((last[2].status == last[0].status).tolist()) and last[2].z.tobytes() == last[0].z.tobytes() and last[2].x.tobytes() == last[0].x.tobytes()
        for knob in (2, 0):
            t, s = statistics.median(ts[knob]), last[knob].stats
            say("| %s | %d | %d | %.4f | %.0f | %d | %d | %d | %d | %.2f | %d |  # calls: %s%s" % (
                name, n, knob, t, n / t, s["supersteps"], s["kernel_launches"], s["batched_relaxations"], s["host_fallbacks"], s["host_fallbacks"] / n,
                s["pivots_phase1"] + s["pivots_phase2"], " ".join("%.4f" % v for v in ts[knob]), "" if same else "  RESULTS DIFFER"))
        pool.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
