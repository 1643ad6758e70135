#!/usr/bin/env python3
"""Seconds per wide frontier wave on the batched revised simplex with the pool knob rev_inplace at 0 (a transposed copy
of the child's matrix per relaxation, k_rv_assemble) and at 1 (the root's resident A^T read in place), same process, same pool, the two
values alternating call by call: median of five pool calls per value after one warm-up each.

    python tools/wide_inplace_timing.py [--first 1] [m nv seed]        (default 300 1200 2; --first 1: every pair of calls takes
                                                                        rev_inplace = 1 first — the order must not matter)

Waves on the root optimum the pool computes, as tools/wide_frontier_timing.py: P (64 children, 6 branch rows), D (one down branch per
fractional integer variable), P8 (256 children, 8 branch rows), and W2048: 2048 children of 6 branch rows — the 64 sign patterns on each
of 32 windows of 6 consecutive entries of the list of integer variables (fractional ones first, as synth.frontier_children picks them).
One line per (wave, knob): wall clock around the pool call (median, spread = max - min, all five values), the schedule's own seconds
(seconds_batch of the last of the five calls), supersteps, launches, the counts that must not differ, and the two arenas of
the wave from gomilp_debug_rev_footprint in MiB.  Below the table: the computed footprint of one 8200 x 24648 child, which needs no run."""
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gomilp_amd import lp, synth

MIB = float(1 << 20)


def windows_wave(x, mask, nwin, K=6):
    """nwin windows of K consecutive picks (fractional integer variables from the highest index down, then integer-valued ones), every
    sign pattern of each"""
    picks = [j for j in range(len(mask) - 1, -1, -1) if mask[j] and x[j] != math.floor(x[j])]
    picks += [j for j in range(len(mask) - 1, -1, -1) if mask[j] and j not in picks]
    wave = []
    for w in range(nwin):
        sel = picks[w:w + K]
        for pattern in range(1 << K):
            cons = []
            for k, j in enumerate(sel):
                fl = float(math.floor(x[j]))
                cons.append((j, -1, -(fl + 1.0)) if (pattern >> k) & 1 else (j, 1, fl))
            wave.append(cons)
    return wave


def main(argv):
    order = (0, 1)
    if "--first" in argv:
        i = argv.index("--first")
        order = (1, 0) if int(argv[i + 1]) else (0, 1)
        del argv[i:i + 2]
    m, nv, seed = (int(a) for a in argv[:3]) if len(argv) >= 3 else (300, 1200, 2)
    c, A, b = synth.dense_lp_standard_form(m, seed, nv)
    mask = synth.integrality_mask(nv, m)
    pool = lp.FrontierPool(workers=8)
    pool.set_root(c, A, b)
    r = pool.solve_root(0.0)
    waves = {"P": synth.frontier_children(r.x, mask, 6),
             "D": [[(j, 1, float(math.floor(r.x[j])))] for j in range(len(mask) - 1, -1, -1) if mask[j] and r.x[j] != math.floor(r.x[j])],
             "P8": synth.frontier_children(r.x, mask, 8),
             "W2048": windows_wave(r.x, mask, 32)}
    print("root %d x %d seed %d, batch_revised = 1, rev_exchange = 1, rev_inplace %d and %d alternating on one pool" % (m, nv + m, seed, order[0], order[1]))
    print("| wave | children | rev_inplace | s / wave | spread | relaxations / s | schedule s | supersteps | launches | batched | host_fallbacks | "
          "art_exchanges | pivots | bland | At MiB | work MiB |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for name, wave in waves.items():
        ts, last = {0: [], 1: []}, {}
        for knob in order:   # warm-up: the buffers of either mode grow here
            pool.set("rev_inplace", knob)
            pool.solve(wave)
        for _ in range(5):
            for knob in order:
                pool.set("rev_inplace", knob)
                t0 = time.perf_counter()
                q = pool.solve(wave)
                ts[knob].append(time.perf_counter() - t0)
                last[knob] = q
        same = bool((last[0].status == last[1].status).all() and (last[0].z.view("u8") == last[1].z.view("u8")).all()
                    and (last[0].x.view("u8") == last[1].x.view("u8")).all())
        for knob in (0, 1):
            s, t = last[knob].stats, statistics.median(ts[knob])
            at, wk = lp.debug_rev_footprint([(m, nv + m)], wave, inplace=bool(knob))
            print("| %s | %d | %d | %.4f | %.4f | %.0f | %.4f | %d | %d | %d | %d | %d | %d | %d | %.1f | %.1f |" % (
                name, len(wave), knob, t, max(ts[knob]) - min(ts[knob]), len(wave) / t, s["seconds_batch"], s["supersteps"], s["kernel_launches"],
                s["batched_relaxations"], s["host_fallbacks"], s["art_exchanges"], s["pivots_phase1"] + s["pivots_phase2"], s["bland_steps"],
                8 * at / MIB, 8 * wk / MIB), "  # calls: " + " ".join("%.4f" % v for v in ts[knob]), flush=True)
        print("  # wave %s: status, z and x of the two modes %s" % (name, "equal by bits" if same else "DIFFER"), flush=True)
    pool.close()
    for shape, K in (((8200, 24648), 1), ((300, 1500), 6)):
        for knob in (0, 1):
            at, wk = lp.debug_rev_footprint([shape], [K], inplace=bool(knob))
            print("one K = %d child of a %d x %d root, rev_inplace %d: At %.1f MiB, work %.1f MiB" % (K, shape[0], shape[1], knob, 8 * at / MIB, 8 * wk / MIB))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
