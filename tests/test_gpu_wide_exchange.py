"""The zero-level artificial exchange on the device-batched revised simplex (pool knob rev_exchange): a wide relaxation
whose Phase I ends with the artificial basic at level zero (simplex.go:581-606) exchanges it inside the schedule — every nonbasic column
tried at once by the worker's acceptance rule, the smallest passing id taken (batch_revised.hip: k_rv_exch) — instead of going to a
worker's whole solve.  The column is the worker's, so the same pool call at rev_exchange = 1, at rev_exchange = 0 (the hand-over) and at
batch_revised = 0 (every relaxation on a worker) must agree bit for bit.

Roots, waves and fixtures as in tests/test_gpu_wide_frontier.py.  Wave P3: the 8 sign patterns of 3 branch rows
(synth.frontier_children(root_x, mask, 3)); its children 1 and 2 exchange.  Wave P (6 rows, 64 children): children 1, 2, 4, 8, 16.
The D waves have no such child.  The scan tries every candidate in one launch: there are no windows to test."""
import functools
import math
import os

import numpy as np
import pytest

from gomilp_amd import lp, synth

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROOTS = {260: (260, 780, 1), 300: (300, 1200, 2)}
WORKERS = 8


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def _fixture(m):
    return dict(np.load(os.path.join(GOLD, "wide_frontier_%d_%d_%d.npz" % ROOTS[m])))


@functools.lru_cache(maxsize=None)
def _root(m):
    mm, nv, seed = ROOTS[m]
    return synth.dense_lp_standard_form(mm, seed, nv)


def down_branches(root_x, mask):
    return [[(j, 1, float(math.floor(root_x[j])))] for j in range(len(mask) - 1, -1, -1) if mask[j] and root_x[j] != math.floor(root_x[j])]


@functools.lru_cache(maxsize=None)
def _wave(m, name):
    mm, nv, _ = ROOTS[m]
    mask = synth.integrality_mask(nv, mm)
    root_x = _fixture(m)["root_x"]
    if name == "D":
        return down_branches(root_x, mask)
    return synth.frontier_children(root_x, mask, {"P3": 3, "P": 6}[name])


_pools = {}


def _pool(m, **knobs):
    """one pool per root for the whole module; every knob a call depends on is set here"""
    if m not in _pools:
        p = lp.FrontierPool(workers=WORKERS)
        p.set_root(*_root(m))
        _pools[m] = p
    p = _pools[m]
    for k, v in {**dict(batch_revised=1, rev_exchange=1, warm_revised=0, exact_degenerate=1, max_pivots=0), **knobs}.items():
        p.set(k, v)
    return p


@pytest.fixture(scope="module", autouse=True)
def _close_pools():
    yield
    for p in _pools.values():
        p.close()
    _pools.clear()


@functools.lru_cache(maxsize=None)
def _run(m, name, batch_revised, rev_exchange):
    r = _pool(m, batch_revised=batch_revised, rev_exchange=rev_exchange).solve(_wave(m, name))
    s = r.stats
    print("wave %s of the %d-row root, batch_revised = %d, rev_exchange = %d: %d children, batched %d, host_fallbacks %d, art_exchanges %d, "
          "supersteps %d, pivots %d + %d, bland %d, phase1 %d, launches %d, %.4f s" % (
              name, m, batch_revised, rev_exchange, len(r.status), s["batched_relaxations"], s["host_fallbacks"], s["art_exchanges"],
              s["supersteps"], s["pivots_phase1"], s["pivots_phase2"], s["bland_steps"], s["phase1_runs"], s["kernel_launches"], s["seconds_total"]))
    return r


def _assert_same_bits(a, b):
    assert np.array_equal(a.status, b.status), (a.status, b.status)
    assert np.array_equal(a.has_x, b.has_x)
    assert np.array_equal(bits(a.z), bits(b.z)), np.flatnonzero(bits(a.z) != bits(b.z))
    assert np.array_equal(bits(a.x), bits(b.x)), np.flatnonzero((bits(a.x) != bits(b.x)).any(axis=1))
    for k in ("pivots_phase1", "pivots_phase2", "bland_steps", "phase1_runs"):
        assert a.stats[k] == b.stats[k], (k, a.stats[k], b.stats[k])


@pytest.mark.parametrize("m", [260, 300])
def test_eight_child_wave_exchanges_on_the_device(m):
    """Children 1 and 2 of the 3-row wave end Phase I with the artificial basic at level zero (the accepted column is about the 448th of
    780 nonbasic ones on the 260-row root, the 840th of 1200 on the 300-row root).  With the knob they stay in the schedule; the results
    are those of the hand-over and of the worker path, bit for bit."""
    on, off, workers = _run(m, "P3", 1, 1), _run(m, "P3", 1, 0), _run(m, "P3", 0, 1)
    assert len(on.status) == 8
    assert on.stats["host_fallbacks"] == 0
    assert on.stats["batched_relaxations"] == 8
    assert on.stats["art_exchanges"] == 2
    assert off.stats["host_fallbacks"] == 2 and off.stats["art_exchanges"] == 0 and off.stats["batched_relaxations"] == 6
    assert workers.stats["batched_relaxations"] == 0 and workers.stats["art_exchanges"] == 0
    _assert_same_bits(on, off)
    _assert_same_bits(on, workers)


@pytest.mark.parametrize("m", [260, 300])
def test_wave_p(m):
    """64 children, five of them exchange; against the hand-over by bits, against the oracle's recorded results under the contract of the
    unguarded revised pipelines: same status, |z - z_ref| <= 1e-9 max(1, |z_ref|)."""
    on, off = _run(m, "P", 1, 1), _run(m, "P", 1, 0)
    assert len(on.status) == 64
    assert on.stats["art_exchanges"] == 5
    assert on.stats["host_fallbacks"] == 0 and on.stats["batched_relaxations"] == 64
    assert off.stats["art_exchanges"] == 0
    _assert_same_bits(on, off)
    fx = _fixture(m)
    st, z, hx = fx["P_status"], fx["P_z"], fx["P_has_x"]
    for i in range(64):
        assert on.status[i] == st[i], (i, int(on.status[i]), int(st[i]))
        assert bool(on.has_x[i]) == bool(hx[i]), i
        if hx[i]:
            assert abs(on.z[i] - z[i]) <= 1e-9 * max(1.0, abs(z[i])), (i, on.z[i], z[i])


def test_warm_child_of_an_exchanged_relaxation():
    """warm_revised = 1: child 1 of the 3-row wave is solved cold with keep and takes the exchange; B^-1 and the basis list it leaves are
    consistent, so its one-row child starts warm from its tag and reaches the cold solve's status and z."""
    m = 260
    mm, nv, _ = ROOTS[m]
    mask = synth.integrality_mask(nv, mm)
    cons = list(_wave(m, "P3")[1])
    pool = _pool(m, warm_revised=1)
    pool.release_warm(-1)
    r = pool.solve_warm([cons], tags=[7], keep=[1])
    print("child 1, cold with keep: status %d z %.17g art_exchanges %d host_fallbacks %d warm_kept %d" % (
        r.status[0], r.z[0], r.stats["art_exchanges"], r.stats["host_fallbacks"], r.stats["warm_kept"]))
    assert r.stats["art_exchanges"] == 1 and r.stats["host_fallbacks"] == 0
    assert r.status[0] == lp.OK and r.stats["warm_kept"] == 1
    used = {t[0] for t in cons}
    more = [t for t in down_branches(r.x[0], mask) if t[0][0] not in used]
    assert more
    child = cons + more[0]
    w = pool.solve_warm([child], parents=[7], tags=[8], keep=[0])
    pool.release_warm(-1)
    cold = _pool(m).solve([child])
    print("its child: warm_started %d warm_fallbacks %d pivots_dual %d status %d z %.17g | cold status %d z %.17g" % (
        w.stats["warm_started"], w.stats["warm_fallbacks"], w.stats["pivots_dual"], w.status[0], w.z[0], cold.status[0], cold.z[0]))
    assert w.stats["warm_started"] == 1
    assert w.status[0] == cold.status[0]
    if cold.status[0] == lp.OK:
        assert abs(w.z[0] - cold.z[0]) <= 1e-9 * max(1.0, abs(cold.z[0])), (w.z[0], cold.z[0])


@pytest.mark.parametrize("m", [260, 300])
def test_d_wave_costs_nothing(m):
    """no child of a D wave exchanges: no scan is launched, the launches are those of rev_exchange = 0"""
    on, off = _run(m, "D", 1, 1), _run(m, "D", 1, 0)
    assert on.stats["art_exchanges"] == 0 and off.stats["art_exchanges"] == 0
    assert on.stats["host_fallbacks"] == off.stats["host_fallbacks"]
    assert on.stats["kernel_launches"] == off.stats["kernel_launches"], (on.stats["kernel_launches"], off.stats["kernel_launches"])
    assert on.stats["supersteps"] == off.stats["supersteps"]
    _assert_same_bits(on, off)
