#!/usr/bin/env python3
"""Warm starts of wide frontier waves on the batched revised simplex (pool knob warm_revised) against the same calls
with the knob at 0 and against the cold calls, same process, same pool, the variants taken in turn: median of five calls after one warm-up.

    python tools/wide_warm_timing.py [--log FILE]        (default FILE: profiles/wide_warm_timing.log; the lines go to stdout too)
    python tools/wide_warm_timing.py --checkout DIR      the warm calls only, on the built package of another checkout (the parent commit,
                                                         which has no such knob): the yardstick that warm_revised = 0 must reproduce —
                                                         compare launches, supersteps and pivots

Tree: bnb.solve_milp on the 260 x 1040 MILP (63 nodes), cold (pool.solve per wave) and warm=True with the knob at 0 and at 1.
Waves: D (one down branch per fractional integer variable, J = 1) and P (64 children, J = 6) of the 300 x 1500 root from the kept root:
pool.solve (cold, batched), solve_warm with the knob at 0 (the workers, cold) and at 1.  Seconds are host-clock around calls that return
results, i.e. end in a device synchronise."""
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OTHER = None
LOG = os.path.join(ROOT, "profiles", "wide_warm_timing.log")
if "--checkout" in sys.argv:
    i = sys.argv.index("--checkout")
    OTHER = os.path.abspath(sys.argv[i + 1])
    del sys.argv[i:i + 2]
if "--log" in sys.argv:
    i = sys.argv.index("--log")
    LOG = os.path.abspath(sys.argv[i + 1])
    del sys.argv[i:i + 2]
sys.path.insert(0, OTHER or ROOT)

from gomilp_amd import bnb, lp, synth

_log = None


def say(line):
    print(line, flush=True)
    if _log:
        _log.write(line + "\n")
        _log.flush()


def timed(variants, reps=5):
    """variants: name -> callable returning what the row reports.  One warm-up each, then `reps` rounds that take the variants in turn."""
    last, ts = {}, {k: [] for k in variants}
    for k, f in variants.items():
        f()
    for _ in range(reps):
        for k, f in variants.items():
            t0 = time.perf_counter()
            last[k] = f()
            ts[k].append(time.perf_counter() - t0)
    return {k: (statistics.median(ts[k]), ts[k], last[k]) for k in variants}


def tree_rows(pool):
    m, nv, seed = 260, 780, 1
    c, A, b = synth.dense_lp_standard_form(m, seed, nv)
    mask = list(synth.integrality_mask(nv, m))

    def run(warm, knob):
        def f():
            if knob is not None and not OTHER:
                pool.set("warm_revised", knob)
            return bnb.solve_milp(c, A, b, None, None, mask, max_nodes=63, pool=pool, warm=warm)
        return f

    variants = {"warm=True, other checkout": run(True, None)} if OTHER else \
        {"cold (pool.solve)": run(False, 0), "warm=True, warm_revised 0": run(True, 0), "warm=True, warm_revised 1": run(True, 1)}
    say("tree: 260 x 1040 MILP, 63 nodes")
    say("| variant | s / tree | relaxations / s | relaxations | pivots | pivots / node | dual pivots | warm_started | warm_fallbacks | error |")
    say("|---|---|---|---|---|---|---|---|---|---|")
    for k, (t, ts, res) in timed(variants).items():
        say("| %s | %.4f | %.0f | %d | %d | %.1f | %d | %d | %d | %s |  # calls: %s" % (
            k, t, res.relaxations / t, res.relaxations, res.pivots, res.pivots / res.relaxations, res.pivots_dual, res.warm_started, res.warm_fallbacks,
            res.error, " ".join("%.4f" % v for v in ts)))


def wave_rows(pool):
    m, nv, seed = 300, 1200, 2
    c, A, b = synth.dense_lp_standard_form(m, seed, nv)
    mask = synth.integrality_mask(nv, m)
    pool.set_root(c, A, b)
    r = pool.solve_root(0.0)
    waves = {"D": [[(j, 1, float(math.floor(r.x[j])))] for j in range(len(mask) - 1, -1, -1) if mask[j] and r.x[j] != math.floor(r.x[j])],
             "P": synth.frontier_children(r.x, mask, 6)}
    say("waves of the 300 x 1500 root from the kept root")
    say("| wave | children | variant | s / wave | relaxations / s | supersteps | launches | batched | host_fallbacks | pivots | dual pivots | warm_started | warm_fallbacks |")
    say("|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for name, wave in waves.items():
        n = len(wave)

        def warm(knob):
            def f():
                if knob is not None and not OTHER:
                    pool.set("warm_revised", knob)
                pool.release_warm(-1)
                pool.solve_warm([[]], tags=[0], keep=[1])   # (the kept root: part of neither timing)
                t0 = time.perf_counter()
                q = pool.solve_warm(wave, parents=[0] * n, tags=list(range(1, n + 1)), keep=[0] * n)
                return q, time.perf_counter() - t0
            return f

        def cold():
            t0 = time.perf_counter()
            q = pool.solve(wave)
            return q, time.perf_counter() - t0

        variants = {"solve_warm, other checkout": warm(None)} if OTHER else \
            {"solve (cold)": cold, "solve_warm, warm_revised 0": warm(0), "solve_warm, warm_revised 1": warm(1)}
        rows = {k: [] for k in variants}   # (the call itself is timed, not the kept root in front of it)
        lastq = {}
        for k, f in variants.items():
            f()   # warm-up
        for _ in range(5):
            for k, f in variants.items():
                q, t = f()
                rows[k].append(t)
                lastq[k] = q
        for k in variants:
            t, s = statistics.median(rows[k]), lastq[k].stats
            say("| %s | %d | %s | %.4f | %.0f | %d | %d | %d | %d | %d | %d | %d | %d |  # calls: %s" % (
                name, n, k, t, n / t, s["supersteps"], s["kernel_launches"], s["batched_relaxations"], s["host_fallbacks"],
                s["pivots_phase1"] + s["pivots_phase2"], s["pivots_dual"], s["warm_started"], s["warm_fallbacks"],
                " ".join("%.4f" % v for v in rows[k])))
    pool.release_warm(-1)


def main():
    global _log
    if not OTHER:
        os.makedirs(os.path.dirname(LOG), exist_ok=True)
        _log = open(LOG, "w")
    say("wide_warm_timing: %s" % ("the package of another checkout (--checkout)" if OTHER else "this checkout's package"))
    pool = lp.FrontierPool(workers=8)
    tree_rows(pool)
    wave_rows(pool)
    pool.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
