"""Wide frontier waves (n - m >= 2m, more than 256 rows, slack starts) on the device-batched revised simplex (pool knob batch_revised,
DESIGN.md §2.5e): the same pool call with the knob at 0 (every relaxation on a worker's Engine::solve, the path this schedule replaces)
and at 1 must agree bit for bit; both against the reference under the documented contract of the unguarded revised pipelines
(same status, z to 1e-9, a primal-feasible x); the routing takes exactly the waves a worker runs on those pipelines.

Roots are synth.dense_lp_standard_form(m, seed, nv).  Wave P: the 2^K sign patterns of K branch rows (synth.frontier_children) on the
oracle's root optimum; wave D: one down branch per fractional integer variable of that optimum, highest index first.  The oracle's
results (tools/gen_golden.py wide / wide_tree) are fixtures: tests/golden/wide_frontier_*.npz, milp_wide260.npz.

Tree (test_tree_*): bnb.solve_milp on the 260 x 1040 MILP with a budget of 63 nodes, through a pool, with the knob at 1 and at 0."""
import functools
import math
import os
import sys

import numpy as np
import pytest

from gomilp_amd import bnb, lp, synth

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# 507: the children of the 507 x 1014 root are narrow (n - m = 1014 < 2 (507 + K)): the tableau schedule takes them at either knob value.
# 5071: 507 x 1100, whose children are wide; with 5 branch rows they have ld = 512, the fused pipeline's shape on a worker.
ROOTS = {260: (260, 780, 1), 300: (300, 1200, 2), 507: (507, 1014, 5), 5071: (507, 1100, 5)}
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
    """name: 'P' (6 rows), 'P5' (5 rows), 'D'"""
    mm, nv, _ = ROOTS[m]
    mask = synth.integrality_mask(nv, mm)
    root_x = _fixture(m)["root_x"]
    if name == "D":
        return down_branches(root_x, mask)
    return synth.frontier_children(root_x, mask, 5 if name == "P5" else 6)


_pools = {}


def _pool(key, root, **knobs):
    """one pool per root for the whole module (first-touch allocations once); knobs are set per call"""
    if key not in _pools:
        p = lp.FrontierPool(workers=WORKERS)
        p.set_root(*root)
        _pools[key] = p
    p = _pools[key]
    for k, v in {**dict(batch_revised=1, exact_degenerate=1, max_pivots=0), **knobs}.items():
        p.set(k, v)
    return p


@pytest.fixture(scope="module", autouse=True)
def _close_pools():
    yield
    for p in _pools.values():
        p.close()
    _pools.clear()


@functools.lru_cache(maxsize=None)
def _run(m, name, knob):
    r = _pool(m, _root(m), batch_revised=knob).solve(_wave(m, name))
    s = r.stats
    print("wave %s of the %d-row root, batch_revised = %d: %d children, batched %d, host_fallbacks %d, supersteps %d, pivots %d + %d, "
          "bland %d, phase1 %d, launches %d, %.3f s" % (name, m, knob, len(r.status), s["batched_relaxations"], s["host_fallbacks"], s["supersteps"],
                                                        s["pivots_phase1"], s["pivots_phase2"], s["bland_steps"], s["phase1_runs"],
                                                        s["kernel_launches"], s["seconds_total"]))
    return r


WAVES = [(260, "P"), (260, "D"), (300, "P"), (300, "D")]


@pytest.mark.parametrize("m,name", WAVES)
def test_wide_wave_runs_batched(m, name):
    """Every relaxation of the wave runs on the batched schedule or is one of its two Phase-I hand-overs (the |x_art| band, the
    zero-level artificial exchange), and those are at most one in eight."""
    r = _run(m, name, 1)
    s, count = r.stats, len(r.status)
    print("batched_relaxations %d host_fallbacks %d of %d" % (s["batched_relaxations"], s["host_fallbacks"], count))
    assert s["batched_relaxations"] + s["host_fallbacks"] == count
    assert s["host_fallbacks"] <= count // 8
    assert s["supersteps"] > 0


def _assert_same_bits(a, b):
    assert np.array_equal(a.status, b.status), (a.status, b.status)
    assert np.array_equal(a.has_x, b.has_x)
    assert np.array_equal(bits(a.z), bits(b.z)), np.flatnonzero(bits(a.z) != bits(b.z))
    assert np.array_equal(bits(a.x), bits(b.x)), np.flatnonzero((bits(a.x) != bits(b.x)).any(axis=1))
    for k in ("pivots_phase1", "pivots_phase2", "bland_steps", "phase1_runs"):
        assert a.stats[k] == b.stats[k], (k, a.stats[k], b.stats[k])


@pytest.mark.parametrize("m,name", WAVES + [(507, "P5"), (507, "D"), (5071, "P5"), (5071, "D")])
def test_bit_equal_to_worker_path(m, name):
    """batch_revised = 1 against = 0 on the same pool: status, has_x, z and x as bits, pivot / Bland / Phase-I totals.  The P5 children of
    the 507 x 1100 root have ld = 512: a worker runs them on the fused pipeline, the batched schedule on the three-kernel form.  (The
    children of the 507 x 1014 root are narrow, 1014 < 2 * 512: the tableau schedule takes them whatever the knob says.)"""
    a, b = _run(m, name, 0), _run(m, name, 1)
    _assert_same_bits(a, b)
    if m == 507:
        assert a.stats["batched_relaxations"] == b.stats["batched_relaxations"] == len(a.status)
    else:
        assert a.stats["batched_relaxations"] == 0 and b.stats["batched_relaxations"] + b.stats["host_fallbacks"] == len(b.status)


@pytest.mark.parametrize("name", ["P", "D"])
def test_context_solves_equal_the_wave(name):
    """Every child of the 260-row waves on an lp.Context: status, z and the root's part of x by bits, pivots and Bland steps as totals."""
    m = 260
    c, A, b = _root(m)
    n0 = A.shape[1]
    wave, r = _wave(m, name), _run(m, name, 1)
    cx = lp.Context()
    piv = bland = 0
    try:
        root = cx.upload(c, A, b)
        for i, cons in enumerate(wave):
            ch = root.child(list(cons))
            g = ch.solve(0.0)
            ch.free()
            piv += g.stats["pivots_phase1"] + g.stats["pivots_phase2"]
            bland += g.stats["bland_steps"]
            assert g.status == r.status[i], (i, g.status, r.status[i])
            assert bits(np.float64(g.z)) == bits(r.z[i]), (i, g.z, r.z[i])
            assert (g.x is not None) == bool(r.has_x[i])
            if g.x is not None:
                assert np.array_equal(bits(g.x[:n0]), bits(r.x[i][:n0])), i
    finally:
        cx.close()
    assert piv == r.stats["pivots_phase1"] + r.stats["pivots_phase2"], (piv, r.stats)
    assert bland == r.stats["bland_steps"], (bland, r.stats)


def _against_reference(m, name, r):
    """the contract of tests/test_gpu_wide.py _check(..., guarded=False) per child; returns how many children equal the oracle's bits"""
    fx = _fixture(m)
    c, A, b = _root(m)
    n0 = A.shape[1]
    wave = _wave(m, name)
    st, z, hx, x = fx[name + "_status"], fx[name + "_z"], fx[name + "_has_x"], fx[name + "_x"]
    assert len(wave) == len(st)
    equal = 0
    for i, cons in enumerate(wave):
        assert r.status[i] == st[i], (i, lp.STATUS_NAMES.get(int(r.status[i])), int(st[i]))
        if hx[i]:
            assert r.has_x[i]
            assert abs(r.z[i] - z[i]) <= 1e-9 * max(1.0, abs(z[i])), (i, r.z[i], z[i])
            xi = r.x[i][:n0]
            assert xi.min() >= -1e-9 and np.abs(A @ xi - b).max() <= 1e-9 * max(1.0, np.abs(b).max()), i
            for (j, sign, rhs) in cons:   # the branch rows (their slacks are beyond the root's width)
                assert sign * xi[j] <= rhs + 1e-9 * max(1.0, abs(rhs)), (i, j)
            equal += int(bits(np.float64(r.z[i])) == bits(np.float64(z[i])) and np.array_equal(bits(xi), bits(x[i])))
        else:
            assert not r.has_x[i]
            equal += 1
    return equal


@pytest.mark.parametrize("m,name", WAVES)
def test_against_reference(m, name):
    e1 = _against_reference(m, name, _run(m, name, 1))
    e0 = _against_reference(m, name, _run(m, name, 0))
    print("wave %s of the %d-row root: %d of %d children equal the oracle bit for bit (batch_revised = 0: %d)" % (name, m, e1, len(_wave(m, name)), e0))
    assert e1 == e0


@pytest.mark.parametrize("name,budget", [("D", 100), ("P", 2)])
def test_pivot_budget_equal_to_worker_path(name, budget):
    """pool knob max_pivots: the loop stops on the device (ST_MAX_PIVOTS) — GOMILP_ERR_UNSUPPORTED with the point of the basis reached in
    Phase II (wave D, 100 pivots), ERR_PHASE1_WRAPPED in Phase I (wave P, 2 pivots) — as a worker's solve reports it, bit for bit"""
    wave = _wave(260, name)
    a = _pool(260, _root(260), batch_revised=0, max_pivots=budget).solve(wave)
    b = _pool(260, _root(260), batch_revised=1, max_pivots=budget).solve(wave)
    _pool(260, _root(260))   # (the knobs back to their defaults)
    print("wave %s, max_pivots = %d: statuses %s" % (name, budget, dict(zip(*np.unique(b.status, return_counts=True)))))
    _assert_same_bits(a, b)
    assert b.stats["batched_relaxations"] + b.stats["host_fallbacks"] == len(wave) and a.stats["batched_relaxations"] == 0
    assert (lp.ERR_UNSUPPORTED if name == "D" else lp.ERR_PHASE1_WRAPPED) in b.status


# ---- routing ----

def _gpu_wave(pool, m, nv, K):
    """P wave with K rows on the root optimum the pool itself computes (routing tests: no oracle needed)"""
    r = pool.solve_root(0.0)
    assert r.status == lp.OK
    return synth.frontier_children(r.x, synth.integrality_mask(nv, m), K)


def test_guarded_wide_wave_stays_on_the_workers():
    """200 rows: the exact-step guard is on, a worker runs the blocked tableau with exact steps"""
    pool = _pool("r200", synth.dense_lp_standard_form(200, 1, 600))
    r = pool.solve(_gpu_wave(pool, 200, 600, 6))
    assert r.stats["batched_relaxations"] == 0 and r.stats["host_fallbacks"] == 0


def test_exact_mode_2_stays_on_the_workers():
    pool = _pool(260, _root(260), exact_degenerate=2)
    r = pool.solve(_wave(260, "P"))
    pool.set("exact_degenerate", 1)
    assert r.stats["batched_relaxations"] == 0 and r.stats["host_fallbacks"] == 0


def test_knob_off_stays_on_the_workers():
    r = _run(260, "P", 0)
    assert r.stats["batched_relaxations"] == 0 and r.stats["host_fallbacks"] == 0 and r.stats["supersteps"] == 0


def test_narrow_wave_is_untouched():
    """the C5 shape (512 x 1024, n - m < 2m): the tableau schedule takes it whatever the knob says"""
    m, seed = synth.CONFIGS["C5"]
    pool = _pool("c5", synth.dense_lp_standard_form(m, seed))
    wave = _gpu_wave(pool, m, m, 4)
    a = _pool("c5", None, batch_revised=0).solve(wave)
    b = _pool("c5", None, batch_revised=1).solve(wave)
    assert a.stats["batched_relaxations"] > 0
    assert (a.stats["batched_relaxations"], a.stats["host_fallbacks"]) == (b.stats["batched_relaxations"], b.stats["host_fallbacks"])
    assert np.array_equal(bits(a.z), bits(b.z)) and np.array_equal(a.status, b.status)


@pytest.mark.parametrize("m,taken", [(252, True), (250, False)])
def test_edge_of_the_guard(m, taken):
    """6-row children of a 252-row root have 258 rows: taken; of a 250-row root 256 rows (guard on): not"""
    pool = _pool("e%d" % m, synth.dense_lp_standard_form(m, 1, 780))
    wave = _gpu_wave(pool, m, 780, 6)
    r = pool.solve(wave)
    print("%d-row root: batched %d host_fallbacks %d of %d" % (m, r.stats["batched_relaxations"], r.stats["host_fallbacks"], len(wave)))
    if taken:
        assert r.stats["batched_relaxations"] > 0 and r.stats["batched_relaxations"] + r.stats["host_fallbacks"] == len(wave)
        _assert_same_bits(_pool("e%d" % m, None, batch_revised=0).solve(wave), r)
    else:
        assert r.stats["batched_relaxations"] == 0 and r.stats["host_fallbacks"] == 0


# ---- a tree ----

class _Recording:
    """a FrontierPool whose waves' stats are kept"""

    def __init__(self, pool):
        self._pool, self.waves = pool, []

    def __getattr__(self, k):
        return getattr(self._pool, k)

    def solve(self, children, *a, **kw):
        r = self._pool.solve(children, *a, **kw)
        self.waves.append(r.stats)
        return r


@functools.lru_cache(maxsize=None)
def _tree(knob):
    mm, nv, seed = ROOTS[260]
    c, A, b = _root(260)
    rec = _Recording(_pool(260, _root(260), batch_revised=knob))
    res = bnb.solve_milp(c, A, b, None, None, list(synth.integrality_mask(nv, mm)), max_nodes=63, pool=rec)
    return res, rec.waves


def test_tree_equal_with_and_without_the_schedule():
    (t0, _), (t1, w1) = _tree(0), _tree(1)
    assert t0.error == t1.error
    assert len(t0.nodes) == len(t1.nodes)
    for a, b in zip(t0.nodes, t1.nodes):
        assert (a.id, a.parent, a.constraints, a.status, a.decision) == (b.id, b.parent, b.constraints, b.status, b.decision), a.id
        assert bits(np.float64(a.z)) == bits(np.float64(b.z)), a.id
        assert (a.x is None) == (b.x is None), a.id
        if a.x is not None:
            assert np.array_equal(bits(a.x), bits(b.x)), a.id
    print("tree: %d nodes, %d waves, batched relaxations per wave %s" % (len(t1.nodes), len(w1), [s["batched_relaxations"] for s in w1]))
    assert any(s["batched_relaxations"] > 0 for s in w1)


def _first_difference(nodes, fx):
    """index of the first solved node whose status, branching decision or z (1e-9 rule) differs from the oracle tree's; len(nodes): none"""
    sys.path.insert(0, os.path.join(os.path.dirname(GOLD), os.pardir, "tools"))
    from gen_golden import DECISIONS
    for i, nd in enumerate(nodes):
        if i >= len(fx["ids"]) or nd.id != fx["ids"][i] or nd.parent != fx["parent"][i]:
            return i
        if [tuple(map(float, t)) for t in nd.constraints] != [tuple(t) for t in fx["constraints"][i][: fx["ncons"][i]]]:
            return i
        if nd.status != fx["status"][i] or nd.decision != DECISIONS[fx["decision"][i]]:
            return i
        if nd.status == lp.OK and not abs(nd.z - fx["z"][i]) <= 1e-9 * max(1.0, abs(fx["z"][i])):
            return i
    return len(nodes)


@pytest.mark.parametrize("knob", [0, 1])
def test_tree_against_reference(knob):
    """Every solved node's id, parent, constraints, status and branching decision equal the oracle tree's (fixture milp_wide260.npz: 64
    solved nodes, DeadlineExceeded), and z to 1e-9 — for the tree of the worker path (batch_revised = 0) and of the new schedule alike."""
    fx = np.load(os.path.join(GOLD, "milp_wide260.npz"))
    res = _tree(knob)[0]
    nodes = [nd for nd in res.nodes if nd.status != -1]
    d = _first_difference(nodes, fx)
    print("oracle tree: %d solved nodes; batch_revised = %d: %d solved nodes, first node that differs: %s" % (
        len(fx["ids"]), knob, len(nodes), "none" if d == len(nodes) else nodes[d].id))
    assert d == len(nodes), nodes[d].id
    assert len(nodes) == len(fx["ids"]) and (res.error or "") == str(fx["error"])
