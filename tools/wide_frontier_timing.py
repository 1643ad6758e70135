#!/usr/bin/env python3
"""Seconds per wide frontier wave with the pool knob batch_revised at 0 (every relaxation on a worker's single-relaxation engine) and at 1
(the device-batched revised simplex), there with the pool knob rev_exchange at 0 (a zero-level artificial exchange goes
to a worker's whole solve) and at 1 (it is done on the device), same process, same pool: median of five pool calls after one warm-up.

    python tools/wide_frontier_timing.py [m nv seed]        (default 300 1200 2)
    python tools/wide_frontier_timing.py --checkout DIR     wave P only, on the built package of another checkout (the parent commit,
                                                            which has no such knob): the yardstick that batch_revised = 0 must reproduce
    python tools/wide_frontier_timing.py --roots            waves of several roots, pool knob rev_roots at 0 (the wave on the workers,
                                                            whole) and at 1 (one schedule on the batched revised simplex); with
                                                            --checkout DIR: the same waves on the other checkout's package, no knob set

Waves on the root optimum the pool computes: P (64 children, 6 branch rows), D (one down branch per fractional integer variable),
P8 (256 children, 8 branch rows).  One line per (wave, knobs): seconds, the spread of the five calls (max - min), relaxations / s,
supersteps, launches, host_fallbacks, art_exchanges, pivots.

The roots leg: IND64 — three wide roots of 300 x 1500 (seeds 2, 3, 4) in one pool, 64 independent LPs spread over them: per root the 8
children of a 3-row P wave, and K = 0 children of the roots in turn up to 64; M — the mixed wave of tests/test_gpu_wide_roots.py on a
pool with the 260 x 1040 root (seed 1) and the 300 x 1500 root (seed 2): the K = 0 child of each, both D waves, both 6-row P waves,
neighbours of different roots."""
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
ROOTS_LEG = "--roots" in sys.argv
if ROOTS_LEG:
    sys.argv.remove("--roots")
sys.path.insert(0, OTHER or ROOT)

from gomilp_amd import lp, synth


def down_branches(x, mask):
    return [[(j, 1, float(math.floor(x[j])))] for j in range(len(mask) - 1, -1, -1) if mask[j] and x[j] != math.floor(x[j])]


def roots_pool(shapes):
    """a pool with these (m, nv, seed) roots and each root's optimum (from its K = 0 child)"""
    pool = lp.FrontierPool(workers=8)
    for t, (m, nv, seed) in enumerate(shapes):
        (pool.add_root if t else pool.set_root)(*synth.dense_lp_standard_form(m, seed, nv))
    r = pool.solve([[] for _ in shapes], roots=list(range(len(shapes))))
    return pool, [r.x[t][: nv + m] for t, (m, nv, _) in enumerate(shapes)]


def interleave(lists):
    out = []
    for t in range(max(len(q) for q in lists)):
        out += [q[t] for q in lists if t < len(q)]
    return out


def main_roots():
    def measure(pool, name, wave, roots):
        for knob in ((-1,) if OTHER else (0, 1)):
            if knob >= 0:
                pool.set("rev_roots", knob)
            pool.solve(wave, roots=roots)   # warm-up
            ts = []
            for _ in range(5):
                t0 = time.perf_counter()
                q = pool.solve(wave, roots=roots)
                ts.append(time.perf_counter() - t0)
            s, t = q.stats, statistics.median(ts)
            print("| %s | %d | %s | %.4f | %.4f | %.0f | %d | %d | %d | %d | %d | %d | %d |" % (
                name, len(wave), knob if knob >= 0 else "other checkout", t, max(ts) - min(ts), len(wave) / t, s["batched_relaxations"], s["supersteps"],
                s["kernel_launches"], s["host_fallbacks"], s.get("art_exchanges", 0), s["pivots_phase1"] + s["pivots_phase2"], s["bland_steps"]),
                  "  # calls: " + " ".join("%.4f" % v for v in ts), flush=True)

    print("waves of several roots, %s" % ("the package of another checkout (--checkout)" if OTHER else "this checkout's package"))
    print("| wave | relaxations | rev_roots | s / wave | spread | relaxations / s | batched | supersteps | launches | host_fallbacks | art_exchanges | pivots | bland |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    shapes = [(300, 1200, 2), (300, 1200, 3), (300, 1200, 4)]
    pool, xs = roots_pool(shapes)
    per = [[(t, c) for c in synth.frontier_children(xs[t], synth.integrality_mask(nv, m), 3)] for t, (m, nv, _) in enumerate(shapes)]
    ind = interleave(per)
    ind += [(t % 3, []) for t in range(64 - len(ind))]
    measure(pool, "IND64", [c for _, c in ind], [t for t, _ in ind])
    pool.close()
    shapes = [(260, 780, 1), (300, 1200, 2)]
    pool, xs = roots_pool(shapes)
    per = []
    for t, (m, nv, _) in enumerate(shapes):
        mask = synth.integrality_mask(nv, m)
        per.append([(t, [])] + [(t, c) for c in down_branches(xs[t], mask)] + [(t, c) for c in synth.frontier_children(xs[t], mask, 6)])
    mixed = interleave(per[::-1])
    measure(pool, "M", [c for _, c in mixed], [t for t, _ in mixed])
    pool.close()
    return 0


def main(argv):
    if ROOTS_LEG:
        return main_roots()
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
