"""Wide waves on the root's matrix in place (pool knob rev_inplace, DESIGN.md §2.5e "Root in place"): the batched revised simplex reads a
child's column from its root's resident A^T through ChildCol (gomilp_amd/csrc/rev_child_col.h) instead of an assembled copy per child.
The in-place kernels run the arithmetic of the assembled ones on synthesised values, term for term, so every comparison here is
rev_inplace = 1 against rev_inplace = 0 on the same pool, by bits: status, has_x, z and x as uint64, and the pivot, Bland, Phase-I,
superstep, hand-over and batched counts equal.

Shapes: the smallest the schedule takes with both parities of m0 (66 and 67 rows) for the index edges of the accessor — the double2 that
straddles m0, ld - m0 of either parity, several branch rows on one variable, the artificial row — and the roots and waves of the
existing wide tests for the degenerate wave, the artificial exchange, the chunked forms, warm starts and several roots."""
import functools
import math

import numpy as np
import pytest

from gomilp_amd import lp, synth
from tests.test_gpu_pool_large_rows import _root2
from tests.test_gpu_wide_exchange import _root as _exch_root, _wave as _exch_wave
from tests.test_gpu_wide_frontier import _root as _wide_root, _wave as _wide_wave, bits
from tests.test_gpu_wide_roots import SMALL

pytestmark = pytest.mark.gpu

EXACT = ("pivots_phase1", "pivots_phase2", "bland_steps", "phase1_runs", "supersteps", "host_fallbacks", "batched_relaxations")
DEFAULTS = dict(batch_revised=1, rev_roots=1, rev_exchange=1, warm_revised=0, exact_degenerate=1, max_pivots=0, large_rows=0, row_chunk=0,
                rev_inplace=0, rev_mem_limit=0)

_pools = {}


def _pool(key, root=None, workers=4, **knobs):
    """one pool per root for the whole module; every knob a run depends on is set per run (large_rows in front of row_chunk)"""
    if key not in _pools:
        p = lp.FrontierPool(workers=workers)
        p.set_root(*root)
        _pools[key] = p
    p = _pools[key]
    for k, v in {**DEFAULTS, **knobs}.items():
        p.set(k, v)
    return p


@pytest.fixture(scope="module", autouse=True)
def _close_pools():
    yield
    for p in _pools.values():
        p.close()
    _pools.clear()


def _show(label, r):
    s = r.stats
    print("%s: %d children, batched %d, host_fallbacks %d, supersteps %d, pivots %d + %d, bland %d, phase1 %d, art_exchanges %d, warm_started %d, "
          "warm_kept %d, pivots_dual %d, launches %d, %.4f s" % (
              label, len(r.status), s["batched_relaxations"], s["host_fallbacks"], s["supersteps"], s["pivots_phase1"], s["pivots_phase2"],
              s["bland_steps"], s["phase1_runs"], s["art_exchanges"], s["warm_started"], s["warm_kept"], s["pivots_dual"], s["kernel_launches"],
              s["seconds_total"]))
    return r


def _same(a, b, keys=EXACT):
    assert np.array_equal(a.status, b.status), (a.status, b.status)
    assert np.array_equal(a.has_x, b.has_x)
    assert np.array_equal(bits(a.z), bits(b.z)), np.flatnonzero(bits(a.z) != bits(b.z))
    assert np.array_equal(bits(a.x), bits(b.x)), np.flatnonzero((bits(a.x) != bits(b.x)).any(axis=1))
    for k in keys:
        assert a.stats[k] == b.stats[k], (k, a.stats[k], b.stats[k])


def _both(key, label, wave, roots=None, **knobs):
    """the wave at rev_inplace 0 and 1 on one pool; the in-place run assembles nothing: one launch less"""
    a = _show("%s, rev_inplace 0" % label, _pool(key, **knobs, rev_inplace=0).solve(wave, roots=roots))
    b = _show("%s, rev_inplace 1" % label, _pool(key, **knobs, rev_inplace=1).solve(wave, roots=roots))
    _pool(key)
    _same(a, b)
    assert b.stats["batched_relaxations"] > 0 and b.stats["supersteps"] > 0
    assert b.stats["art_exchanges"] == a.stats["art_exchanges"]
    return a, b


# ---- 1. index edges -----------------------------------------------------------------------------------------------------------------

EDGE = {66: (66, 200, 1), 67: (67, 210, 1)}   # even / odd m0; 66: the small root of tests/test_gpu_wide_roots.py


def _edge_wave(x, nv):
    """on the root optimum x: the K = 0 child; down branches on K = 1..4 fractional variables (ld - m0 = 0 / 2 / 2 / 4 at even m0,
    1 / 1 / 3 / 3 at odd m0: the straddling pair with one, two and no branch entry beside the root's last element); two children with
    two rows on ONE variable — fl <= x_j <= fl + 1, and x_j <= fl with x_j >= fl + 1, which is infeasible —; up branches x_j >= fl + 1,
    a negative right-hand side: Phase I and its artificial row; one child that mixes the two kinds"""
    fr = [j for j in range(nv) if x[j] != math.floor(x[j])]
    assert len(fr) >= 4
    fl = lambda j: float(math.floor(x[j]))   # noqa: E731
    w = [[]]
    for K in range(1, 5):
        w.append([(j, 1, fl(j)) for j in fr[:K]])
    j = fr[0]
    w.append([(j, 1, fl(j) + 1.0), (j, -1, -fl(j))])
    w.append([(j, 1, fl(j)), (j, -1, -(fl(j) + 1.0))])
    for j in fr[:4]:
        w.append([(j, -1, -(fl(j) + 1.0))])
    w.append([(fr[0], -1, -(fl(fr[0]) + 1.0)), (fr[1], 1, fl(fr[1])), (fr[2], -1, -(fl(fr[2]) + 1.0))])
    return w


@pytest.mark.parametrize("m", [66, 67])
def test_index_edges(m):
    """(the oracle on the CPU gives, for both roots: children 0-5 GOMILP_OK without Phase I, child 6 and child 11 infeasible, the up
    branches 7-10 GOMILP_OK after Phase I)"""
    mm, nv, seed = EDGE[m]
    key = "edge%d" % m
    knobs = dict(exact_degenerate=0)
    r0 = _pool(key, synth.dense_lp_standard_form(mm, seed, nv), **knobs).solve([[]])
    assert r0.status[0] == lp.OK
    wave = _edge_wave(r0.x[0], nv)
    a, b = _both(key, "%d rows, index edges" % m, wave, **knobs)
    assert b.stats["batched_relaxations"] + b.stats["host_fallbacks"] == len(wave)
    assert b.stats["phase1_runs"] >= 6
    assert list(b.status[:6]) == [lp.OK] * 6
    assert b.status[6] == lp.ERR_INFEASIBLE and b.status[11] == lp.ERR_INFEASIBLE
    assert lp.OK in list(b.status[7:11])   # (GOMILP_OK after Phase I)
    workers = _show("%d rows, index edges, batch_revised 0" % m, _pool(key, **knobs, batch_revised=0).solve(wave))
    _pool(key)
    assert workers.stats["batched_relaxations"] == 0
    _same(workers, b, EXACT[:4])


# ---- 2. the degenerate wave ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["P", "D"])
def test_r300_waves(name):
    """R300 (300 x 1500, seed 2): wave P — 64 children, most pivots Bland steps — and wave D, at the default exact_degenerate"""
    wave = _wide_wave(300, name)
    a, b = _both(300, "R300 wave %s" % name, wave, root=_wide_root(300))
    if name == "P":
        assert len(wave) == 64 and b.stats["bland_steps"] > 0
    assert a.stats["kernel_launches"] > 0


# ---- 3. the zero-level artificial exchange -------------------------------------------------------------------------------------------

def test_artificial_exchange():
    a, b = _both("x300", "exchange root, wave P3", _exch_wave(300, "P3"), root=_exch_root(300))
    assert a.stats["art_exchanges"] > 0 and b.stats["art_exchanges"] > 0


# ---- 4. the chunked forms ------------------------------------------------------------------------------------------------------------

def test_one_chunk_with_a_tail():
    _both(300, "R300 wave D, row_chunk 512", _wide_wave(300, "D"), root=_wide_root(300), large_rows=1, row_chunk=512)


def test_chunked_exchange_scan():
    a, b = _both("x300", "exchange root, wave P3, row_chunk 512", _exch_wave(300, "P3"), root=_exch_root(300), large_rows=1, row_chunk=512)
    assert b.stats["art_exchanges"] > 0


@functools.lru_cache(maxsize=None)
def _wave2():
    """the wave of tests/test_gpu_pool_large_rows.py on its 1100-row root: the up and down one-row children of the three highest-index
    fractional structural variables of the root optimum (1101 rows, ld2 = 551: three chunks of 256 double2)"""
    nv = _root2()[1].shape[1] - _root2()[1].shape[0]
    r = _pool(1100, _root2()).solve_root(0.0)
    assert r.status == lp.OK
    picks = [j for j in range(nv - 1, -1, -1) if r.x[j] != math.floor(r.x[j])][:3]
    wave = []
    for j in picks:
        fl = float(math.floor(r.x[j]))
        wave += [[(j, 1, fl)], [(j, -1, -(fl + 1.0))]]
    return wave


def test_three_chunks():
    a, b = _both(1100, "1100 rows, row_chunk 512", _wave2(), root=_root2(), large_rows=1, row_chunk=512, max_pivots=400)
    assert b.stats["phase1_runs"] == 3


# ---- 5. warm starts -------------------------------------------------------------------------------------------------------------------

def _two_generations(pool):
    """R260: the root kept; wave D warm from it, kept (one new row each); every D child with one more row from its kept parent, and the
    same two-row children from the kept root (two new rows)"""
    D = _wide_wave(260, "D")
    n = len(D)
    pool.release_warm(-1)
    r0 = pool.solve_warm([[]], tags=[0], keep=[1])
    assert r0.status[0] == lp.OK and r0.stats["warm_kept"] == 1
    g1 = pool.solve_warm(D, parents=[0] * n, tags=list(range(1, 1 + n)), keep=[1] * n, dual_budget=4096)
    wave2 = [D[i] + D[(i + 1) % n] for i in range(n)]
    g2 = pool.solve_warm(wave2 + wave2, parents=list(range(1, 1 + n)) + [0] * n, tags=[-1] * (2 * n), keep=[0] * (2 * n), dual_budget=4096)
    pool.release_warm(-1)
    return r0, g1, g2


@pytest.mark.parametrize("chunk", [0, 512])
def test_warm_starts(chunk):
    """warm_revised = 1 at 260 rows; chunk 512: the chunked dual pricing kernel (large_rows = 1, row_chunk = 512)"""
    knobs = dict(warm_revised=1, large_rows=1 if chunk else 0, row_chunk=chunk)
    runs = {}
    for ip in (0, 1):
        runs[ip] = _two_generations(_pool(260, _wide_root(260), workers=8, **knobs, rev_inplace=ip))
    _pool(260)
    for gen, (a, b) in enumerate(zip(runs[0], runs[1])):
        _show("R260 generation %d, row_chunk %d, rev_inplace 0" % (gen, chunk), a)
        _show("R260 generation %d, row_chunk %d, rev_inplace 1" % (gen, chunk), b)
        _same(a, b, EXACT + ("pivots_dual", "warm_kept", "warm_started", "warm_fallbacks"))
    assert runs[1][1].stats["warm_started"] == len(runs[1][1].status) and runs[1][1].stats["pivots_dual"] > 0
    assert runs[1][2].stats["warm_started"] == len(runs[1][2].status)


# ---- 6. two roots and more: ld0 differs per relaxation -------------------------------------------------------------------------------

def test_several_roots():
    """the small mixed wave of tests/test_gpu_wide_roots.py (66 / 80 / 70 rows): per root its K = 0 child and the 8 sign patterns of 3
    branch rows on the optimum the pool computes, neighbours of different roots"""
    order = tuple(SMALL)
    key = "small"
    knobs = dict(exact_degenerate=0)
    if key not in _pools:
        p = lp.FrontierPool(workers=4)
        p.set_root(*synth.dense_lp_standard_form(SMALL[order[0]][0], SMALL[order[0]][2], SMALL[order[0]][1]))
        for m in order[1:]:
            p.add_root(*synth.dense_lp_standard_form(SMALL[m][0], SMALL[m][2], SMALL[m][1]))
        _pools[key] = p
    r0 = _pool(key, **knobs).solve([[], [], []], roots=[0, 1, 2])
    assert list(r0.status) == [lp.OK] * 3
    per = []
    for t, m in enumerate(order):
        mm, nv, _ = SMALL[m]
        kids = synth.frontier_children(r0.x[t][: nv + mm], synth.integrality_mask(nv, mm), 3)
        assert len(kids) == 8
        per.append([(t, [])] + [(t, c) for c in kids])
    W = [per[t][k] for k in range(9) for t in range(3)]
    a, b = _both(key, "three small roots", [e[1] for e in W], roots=[e[0] for e in W], **knobs)
    assert b.stats["batched_relaxations"] + b.stats["host_fallbacks"] == len(W)


# ---- 7. the capability: a wave that does not fit with copies runs batched in place ----------------------------------------------------

def test_wave_fits_in_place_only():
    """R300 wave P on a fresh pool under rev_mem_limit halfway between what the wave needs in place and what it needs with copies
    (RevBatchEngine::run's own inequality on the probe's byte counts): with copies it goes to the workers, whole; in place it runs
    batched; the same bits either way"""
    c, A, b = _wide_root(300)
    wave = _wide_wave(300, "P")
    assert len(wave) == 64
    shape = [(A.shape[0], A.shape[1])]
    need = {}
    for ip in (0, 1):
        at, wk = lp.debug_rev_footprint(shape, wave, inplace=bool(ip))
        nbytes = 8 * (at + wk)
        need[ip] = nbytes * 17 // 16 + (256 << 20)
    limit = (need[0] + need[1]) // 2 >> 20
    print("need with copies %.1f MiB, in place %.1f MiB, rev_mem_limit %d MiB" % (need[0] / 2 ** 20, need[1] / 2 ** 20, limit))
    assert need[1] + (8 << 20) < limit << 20 < need[0] - (8 << 20)
    pool = lp.FrontierPool(workers=8, rev_mem_limit=limit)
    try:
        pool.set_root(c, A, b)
        copies = _show("R300 wave P under the limit, rev_inplace 0", pool.solve(wave))
        pool.set("rev_inplace", 1)
        inplace = _show("R300 wave P under the limit, rev_inplace 1", pool.solve(wave))
        pool.set("rev_mem_limit", 0)
        pool.set("rev_inplace", 0)
        free = _show("R300 wave P without a limit, rev_inplace 0", pool.solve(wave))
    finally:
        pool.close()
    assert copies.stats["batched_relaxations"] == 0 and copies.stats["supersteps"] == 0
    assert inplace.stats["batched_relaxations"] + inplace.stats["host_fallbacks"] == 64
    assert inplace.stats["batched_relaxations"] == 64
    _same(copies, inplace, EXACT[:4])
    _same(free, inplace)
