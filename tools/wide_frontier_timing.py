#!/usr/bin/env python3
"""Seconds per wide frontier wave with the pool knob batch_revised at 0 (every relaxation on a worker's single-relaxation engine) and at 1
(the device-batched revised simplex), there with the pool knob rev_exchange at 0 (a zero-level artificial exchange goes
to a worker's whole solve) and at 1 (it is done on the device), same process, same pool: median of five pool calls after one warm-up.

    python tools/wide_frontier_timing.py [m nv seed]        (default 300 1200 2)
    python tools/wide_frontier_timing.py --checkout DIR     wave P only, on the built package of another checkout (the parent commit,
                                                            which has no such knob): the yardstick that batch_revised = 0 must reproduce

Waves on the root optimum the pool computes: P (64 children, 6 branch rows), D (one down branch per fractional integer variable),
P8 (256 children, 8 branch rows).  One line per (wave, knobs): seconds, the spread of the five calls (max - min), relaxations / s,
supersteps, launches, host_fallbacks, art_exchanges, pivots."""
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OTHER = None
if "--checkout" in sys.argv:
    i = sys.argv.index("--checkout")
    OTHER = os.path.abspath(sys.argv[i + 1])
    del sys.argv[i:i + 2]
sys.path.insert(0, OTHER or ROOT)

from gomilp_amd import lp, synth


def main(argv):
    m, nv, seed = (int(a) for a in argv[:3]) if len(argv) >= 3 else (300, 1200, 2)
    c, A, b = synth.dense_lp_standard_form(m, seed, nv)
    mask = synth.integrality_mask(nv, m)
    pool = lp.FrontierPool(workers=8)
    pool.set_root(c, A, b)
    r = pool.solve_root(0.0)
    waves = {"P": synth.frontier_children(r.x, mask, 6),
             "D": [[(j, 1, float(math.floor(r.x[j])))] for j in range(len(mask) - 1, -1, -1) if mask[j] and r.x[j] != math.floor(r.x[j])],
             "P8": synth.frontier_children(r.x, mask, 8)}
    if OTHER:
        waves = {"P": waves["P"]}
    print("root %d x %d seed %d, %s" % (m, nv + m, seed, "the package of another checkout (--checkout)" if OTHER else "this checkout's package"))
    print("| wave | children | batch_revised | rev_exchange | s / wave | spread | relaxations / s | supersteps | launches | host_fallbacks | art_exchanges | pivots | bland |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for name, wave in waves.items():
        for knob, exch in (((-1, -1),) if OTHER else ((0, 0), (1, 0), (1, 1))):
            if knob >= 0:
                pool.set("batch_revised", knob)
                pool.set("rev_exchange", exch)
            pool.solve(wave)   # warm-up
            ts = []
            for _ in range(5):
                t0 = time.perf_counter()
                q = pool.solve(wave)
                ts.append(time.perf_counter() - t0)
            s, t = q.stats, statistics.median(ts)
            print("| %s | %d | %s | %s | %.4f | %.4f | %.0f | %d | %d | %d | %d | %d | %d |" % (
                name, len(wave), knob if knob >= 0 else "other checkout", exch if knob > 0 else "-", t, max(ts) - min(ts), len(wave) / t, s["supersteps"],
                s["kernel_launches"], s["host_fallbacks"], s.get("art_exchanges", 0), s["pivots_phase1"] + s["pivots_phase2"], s["bland_steps"]),
                  "  # calls: " + " ".join("%.4f" % v for v in ts), flush=True)
    pool.close()
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
