"""Frontier pools beyond the 64 KB LDS window (pool knob large_rows, DESIGN.md §2.5e "Chunked forms"): the batched revised simplex in its
chunked kernels (batch_revised.hip: the CK = true instances of k_rv_*), the staged m-long vectors streamed through LDS row_chunk doubles at a time.

The chunked kernels run the helpers of the one-pass kernels on dot products accumulated in the same order (kernels_common.h: dot_group), so
every comparison between chunk sizes, and with the worker path, is by bits: status and has_x equal, z and x equal as uint64, the pivot,
Bland and Phase-I totals equal (_assert_same_bits of tests/test_gpu_wide_frontier.py).

Tests 1-5 force chunks (large_rows = 1, row_chunk = 512 / 1536 doubles) at the smallest shapes that have one chunk with a ragged tail
(300 rows: 152 double2 in a chunk of 256) and several chunks with one (1100 rows: 551 double2 = 256 + 256 + 39).  Tests 6 and 7 run the
real sizes: an 8200-row root (children with ld = 8202, automatic chunks of 4096 doubles) and a 4100-row root whose children start warm
only with the knob (the dual pricing kernel stages two vectors: one pass up to 4096 rows)."""
import functools
import math
import time

import numpy as np
import pytest

from gomilp_amd import lp, synth
from tests.test_gpu_large_rows import BUDGET, _gen
from tests.test_gpu_wide_exchange import _root as _exch_root, _wave as _exch_wave
from tests.test_gpu_wide_frontier import _against_reference, _assert_same_bits, _root as _wide_root, _wave as _wide_wave, bits

pytestmark = pytest.mark.gpu

WORKERS = 4
DEFAULTS = dict(batch_revised=1, rev_exchange=1, warm_revised=0, exact_degenerate=1, max_pivots=0, large_rows=0, row_chunk=0)

_pools = {}


def _pool(key, root=None, workers=WORKERS, **knobs):
    """one pool per root for the whole module; every knob a run depends on is set per run (large_rows in front of row_chunk)"""
    if key not in _pools:
        p = lp.FrontierPool(workers=workers, large_rows=knobs.get("large_rows", 0))
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
          "warm_fallbacks %d, warm_kept %d, pivots_dual %d, launches %d, %.3f s" % (
              label, len(r.status), s["batched_relaxations"], s["host_fallbacks"], s["supersteps"], s["pivots_phase1"], s["pivots_phase2"],
              s["bland_steps"], s["phase1_runs"], s["art_exchanges"], s["warm_started"], s["warm_fallbacks"], s["warm_kept"], s["pivots_dual"],
              s["kernel_launches"], s["seconds_total"]))
    return r


# ---- 1. one chunk with a tail ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["P", "D"])
def test_one_chunk_with_a_tail(name):
    """waves P and D of the 300 x 1200 root (children of 301 / 306 rows): one chunk of 256 double2 holds the vector and its tail"""
    wave = _wide_wave(300, name)
    a = _show("300 rows, wave %s, large_rows 0" % name, _pool(300, _wide_root(300)).solve(wave))
    b = _show("300 rows, wave %s, row_chunk 512" % name, _pool(300, large_rows=1, row_chunk=512).solve(wave))
    _pool(300)
    _assert_same_bits(a, b)
    assert b.stats["batched_relaxations"] + b.stats["host_fallbacks"] == len(wave) and b.stats["supersteps"] > 0
    assert a.stats["supersteps"] == b.stats["supersteps"]
    _against_reference(300, name, b)


# ---- 2. several chunks --------------------------------------------------------------------------------------------------------------

M2, NV2, SEED2 = 1100, 2300, 1


@functools.lru_cache(maxsize=None)
def _root2():
    return synth.dense_lp_standard_form(M2, SEED2, NV2)


@functools.lru_cache(maxsize=None)
def _wave2():
    """the up and down one-row children of the three highest-index fractional structural variables of the root optimum"""
    r = _pool(M2, _root2()).solve_root(0.0)
    assert r.status == lp.OK
    picks = [j for j in range(NV2 - 1, -1, -1) if r.x[j] != math.floor(r.x[j])][:3]
    assert len(picks) == 3
    wave = []
    for j in picks:
        fl = float(math.floor(r.x[j]))
        wave += [[(j, 1, fl)], [(j, -1, -(fl + 1.0))]]
    return wave


@functools.lru_cache(maxsize=None)
def _run2(batch_revised, large_rows, row_chunk):
    wave = _wave2()
    r = _pool(M2, _root2(), batch_revised=batch_revised, large_rows=large_rows, row_chunk=row_chunk, max_pivots=400).solve(wave)
    _pool(M2)
    return _show("1100 rows, batch_revised %d large_rows %d row_chunk %d" % (batch_revised, large_rows, row_chunk), r)


@pytest.mark.parametrize("chunk", [512, 1536])
def test_multi_chunk(chunk):
    """1101 rows, ld2 = 551: row_chunk 512 gives three chunks (256 + 256 + 39 double2), 1536 one; three of the six children start in
    Phase I (the forced pivot and the refresh through the chunked k_rv_ftran / k_rv_update / k_rv_matvec)"""
    ref, workers, g = _run2(1, 1, 0), _run2(0, 0, 0), _run2(1, 1, chunk)
    assert len(g.status) == 6
    assert g.stats["phase1_runs"] == 3
    assert g.stats["batched_relaxations"] + g.stats["host_fallbacks"] == 6
    assert workers.stats["batched_relaxations"] == 0
    _assert_same_bits(ref, g)
    _assert_same_bits(workers, g)
    assert ref.stats["supersteps"] == g.stats["supersteps"]


# ---- 3. Bland steps -----------------------------------------------------------------------------------------------------------------

def test_bland_steps():
    """synth.wide_degenerate_lp(1000, 0) under a budget of 400 pivots: the root itself and two one-row children; the Bland rule inside the
    loop (k_rv_bland, the candidate's FTRAN in the chunked k_rv_ftran, replaceBland's leaving row in the chunked k_rv_update)"""
    root = synth.wide_degenerate_lp(1000, 0)
    wave = [[], [(0, 1, 1.0)], [(1, 1, 0.0)]]
    a = _show("degenerate 1000 rows, row_chunk 0", _pool("deg", root, large_rows=1, max_pivots=BUDGET).solve(wave))
    b = _show("degenerate 1000 rows, row_chunk 512", _pool("deg", large_rows=1, row_chunk=512, max_pivots=BUDGET).solve(wave))
    _pool("deg")
    assert b.stats["batched_relaxations"] + b.stats["host_fallbacks"] == 3
    _assert_same_bits(a, b)
    assert b.stats["bland_steps"] > 0


# ---- 4. the zero-level artificial exchange ------------------------------------------------------------------------------------------

def test_artificial_exchange():
    """No construction of tests/test_gpu_wide_exchange.py has more than 512 rows, so its largest: wave P3 of the 300 x 1200 root (8
    children of 303 rows, children 1 and 2 exchange) — the candidate scan in the chunked k_rv_exch, one chunk with a tail"""
    wave = _exch_wave(300, "P3")
    a = _show("exchange, row_chunk 0", _pool("x300", _exch_root(300), large_rows=1).solve(wave))
    b = _show("exchange, row_chunk 512", _pool("x300", large_rows=1, row_chunk=512).solve(wave))
    _pool("x300")
    _assert_same_bits(a, b)
    assert b.stats["art_exchanges"] == a.stats["art_exchanges"] > 0
    assert b.stats["host_fallbacks"] == a.stats["host_fallbacks"]


# ---- 5. warm starts -----------------------------------------------------------------------------------------------------------------

def _warm2(row_chunk):
    pool = _pool(M2, _root2(), warm_revised=1, large_rows=1, row_chunk=row_chunk)
    pool.release_warm(-1)
    r0 = pool.solve_warm([[]], tags=[0], keep=[1])
    assert r0.status[0] == lp.OK and r0.stats["warm_kept"] == 1
    wave = _wave2()
    r = pool.solve_warm(wave, parents=[0] * len(wave), tags=list(range(1, 1 + len(wave))), keep=[0] * len(wave))
    pool.release_warm(-1)
    _pool(M2)
    return _show("1100 rows warm, row_chunk %d" % row_chunk, r)


def test_warm_start():
    """the six children of test 2 from the kept root: the chunked k_rv_dual_price (two vectors, 256 double2 each at a time) in front of
    the chunked k_rv_ftran<RR_DUAL> / k_rv_update<RR_DUAL>; against the cold wave under the contract of the warm mode"""
    a, b = _warm2(0), _warm2(512)
    _assert_same_bits(a, b)
    for k in ("pivots_dual", "warm_started", "warm_fallbacks"):
        assert a.stats[k] == b.stats[k], (k, a.stats[k], b.stats[k])
    assert b.stats["pivots_dual"] > 0 and b.stats["warm_started"] == 6
    cold = _show("1100 rows cold", _pool(M2, _root2(), large_rows=1, row_chunk=512).solve(_wave2()))
    _pool(M2)
    assert np.array_equal(b.status, cold.status), (b.status, cold.status)
    for i in range(6):
        if cold.status[i] == lp.OK:
            assert abs(b.z[i] - cold.z[i]) <= 1e-9 * max(1.0, abs(cold.z[i])), (i, b.z[i], cold.z[i])


# ---- 6. beyond 8192 rows ------------------------------------------------------------------------------------------------------------

def _cost_children(c, nv):
    j = int(np.flatnonzero(c[:nv])[0])
    return [[(j, 1, 1.0)], [(j, -1, -1.0)]]


def test_beyond_8192_rows():
    """8200 x 24648 root, two one-row children (8201 rows, ld = 8202; the second starts in Phase I) under a budget of 16 pivots: both run
    on the batched schedule in automatic chunks of 4096 doubles and equal a context's solve of the same child, bit for bit.  A pool that
    holds such a root keeps the knob."""
    t0 = time.time()
    m0, nv = 8200, 16448
    c, A, b = _gen(m0, nv, 0)
    n0 = nv + m0
    wave = _cost_children(c, nv)
    pool = lp.FrontierPool(workers=1, large_rows=1, max_pivots=16)
    try:
        pool.set_root(c, A, b)
        r = _show("8200 rows", pool.solve(wave))
        assert r.stats["batched_relaxations"] == 2 and r.stats["host_fallbacks"] == 0
        with pytest.raises(ValueError):
            pool.set("large_rows", 0)
        r2 = pool.solve(wave)   # (the refused call left the pool as it was)
        assert np.array_equal(r.status, r2.status) and np.array_equal(bits(r.z), bits(r2.z))
    finally:
        pool.close()
    cx = lp.Context(max_pivots=16)
    try:
        root = cx.upload(c, A, b)
        for i, rows in enumerate(wave):
            ch = root.child(rows)
            g = ch.solve(0.0)
            ch.free()
            print("child %d: status %s pivots %d + %d z %.17g" % (i, lp.STATUS_NAMES.get(g.status, g.status), g.stats["pivots_phase1"],
                                                                 g.stats["pivots_phase2"], g.z))
            assert g.status == r.status[i], (i, g.status, r.status[i])
            assert bits(np.float64(g.z)) == bits(r.z[i]), (i, g.z, r.z[i])
            assert (g.x is not None) == bool(r.has_x[i]), i
            if g.x is not None:
                assert np.array_equal(bits(g.x[:n0]), bits(r.x[i][:n0])), i
        root.free()
    finally:
        cx.close()
    print("test_beyond_8192_rows: %.1f s" % (time.time() - t0))


# ---- 7. warm beyond 4096 rows -------------------------------------------------------------------------------------------------------

def test_warm_beyond_4096_rows():
    """4100 x 12400 root kept, its two one-row children (ld = 4102) with parents: with large_rows = 1 both start warm (chunked dual
    pricing); with the knob at 0 the wave runs cold with keeping, as before"""
    t0 = time.time()
    m0, nv = 4100, 8300
    c, A, b = _gen(m0, nv, 0)
    wave = _cost_children(c, nv)
    pool = lp.FrontierPool(workers=1, warm_revised=1)
    runs = {}
    try:
        pool.set_root(c, A, b)
        for knob in (1, 0):
            pool.set("large_rows", knob)
            pool.release_warm(-1)
            r0 = pool.solve_warm([[]], tags=[0], keep=[1])
            assert r0.status[0] == lp.OK and r0.stats["warm_kept"] == 1 and r0.stats["batched_relaxations"] == 1, (knob, r0.status, r0.stats)
            runs[knob] = _show("4100 rows, large_rows %d" % knob, pool.solve_warm(wave, parents=[0, 0], tags=[1, 2], keep=[0, 0]))
        pool.release_warm(-1)
    finally:
        pool.close()
    on, off = runs[1], runs[0]
    assert on.stats["warm_started"] == 2
    assert off.stats["warm_started"] == 0
    assert on.stats["batched_relaxations"] + on.stats["host_fallbacks"] == 2 and off.stats["batched_relaxations"] + off.stats["host_fallbacks"] == 2
    assert np.array_equal(on.status, off.status), (on.status, off.status)
    for i in range(2):
        if off.status[i] == lp.OK:
            assert abs(on.z[i] - off.z[i]) <= 1e-9 * max(1.0, abs(off.z[i])), (i, on.z[i], off.z[i])
    print("test_warm_beyond_4096_rows: %.1f s" % (time.time() - t0))
