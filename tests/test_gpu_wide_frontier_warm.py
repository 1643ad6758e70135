"""Warm starts of wide frontier waves on the device-batched revised simplex (pool knob warm_revised): a
gomilp_frontier_solve_warm call whose wave passes the wide routing test runs on RevBatchEngine; a relaxation whose parent's kept state is
of that schedule and whose branch rows extend the parent's by J >= 1 starts from B^-1 = [[B_p^-1, 0], [R, I_J]] with the dual loop, every
other relaxation of the wave starts cold in the same run.

Roots and waves as in tests/test_gpu_wide_frontier.py (synth.dense_lp_standard_form, synth.integrality_mask, down branches,
synth.frontier_children); the expected values of the 260- and 300-row waves and of the tree are that file's fixtures.  The contract of the
warm mode (include/gomilp_lp.h): status, branching decision, |z - z_ref| <= 1e-9 max(1, |z_ref|), a primal-feasible x."""
import functools
import math
import os
import sys

import numpy as np
import pytest

from gomilp_amd import bnb, lp, synth

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROOTS = {66: (66, 200, 1), 260: (260, 780, 1), 300: (300, 1200, 2), 507: (507, 1014, 5)}
WORKERS = 8
BIG_BUDGET = 4096


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
    return down_branches(root_x, mask) if name == "D" else synth.frontier_children(root_x, mask, 6)


_pools = {}


def _pool(m, **knobs):
    """one pool per root for the whole module; the knobs of every call are set here (the small root runs at exact_degenerate = 0: with
    the guard of mode 1 off only beyond 256 rows, 65 rows is the smallest size the batched revised simplex takes)"""
    if m not in _pools:
        p = lp.FrontierPool(workers=WORKERS)
        p.set_root(*_root(m))
        _pools[m] = p
    p = _pools[m]
    for k, v in {**dict(batch_revised=1, warm_revised=1, exact_degenerate=0 if m == 66 else 1, max_pivots=0), **knobs}.items():
        p.set(k, v)
    return p


@pytest.fixture(scope="module", autouse=True)
def _close_pools():
    yield
    for p in _pools.values():
        p.close()
    _pools.clear()


def _keep_root(pool):
    """the root through the batched schedule, kept under tag 0 (as bnb.solve_milp(warm=True) does)"""
    pool.release_warm(-1)
    r = pool.solve_warm([[]], tags=[0], keep=[1])
    assert r.status[0] == lp.OK
    return r


def _warm_wave(pool, wave, parents, budget=BIG_BUDGET, tag0=1, keep=1):
    return pool.solve_warm(wave, parents=parents, tags=list(range(tag0, tag0 + len(wave))), keep=[keep] * len(wave), dual_budget=budget)


def _say(label, r):
    s = r.stats
    print("%s: %d children, warm_started %d, warm_fallbacks %d, warm_kept %d, pivots_dual %d, pivots %d + %d, batched %d, host_fallbacks %d, "
          "supersteps %d, launches %d" % (label, len(r.status), s["warm_started"], s["warm_fallbacks"], s["warm_kept"], s["pivots_dual"],
                                          s["pivots_phase1"], s["pivots_phase2"], s["batched_relaxations"], s["host_fallbacks"], s["supersteps"],
                                          s["kernel_launches"]))


def _check_contract(root, wave, r, st, z, label):
    """status, z (1e-9 rule) and a primal-feasible x per child; infeasible children come out ERR_INFEASIBLE without x"""
    c, A, b = root
    n0 = A.shape[1]
    assert len(wave) == len(st) == len(r.status)
    for i, cons in enumerate(wave):
        print("%s child %d: status %d / %d, z %.17g / %.17g" % (label, i, r.status[i], st[i], r.z[i], z[i]))
        assert r.status[i] == st[i], (label, i, lp.STATUS_NAMES.get(int(r.status[i])), int(st[i]))
        if st[i] == lp.OK:
            assert r.has_x[i]
            assert abs(r.z[i] - z[i]) <= 1e-9 * max(1.0, abs(z[i])), (label, i, r.z[i], z[i])
            xi = r.x[i][:n0]
            assert xi.min() >= -1e-9 and np.abs(A @ xi - b).max() <= 1e-9 * max(1.0, np.abs(b).max()), (label, i)
            for (j, sign, rhs) in cons:
                assert sign * xi[j] <= rhs + 1e-9 * max(1.0, abs(rhs)), (label, i, j)
        else:
            assert not r.has_x[i], (label, i)


# ---- 1. small shapes against the live oracle ----

@functools.lru_cache(maxsize=None)
def _small():
    """The 66 x 266 root and three waves on the oracle's optima.  A: one-row children of the root — its down branches (variables basic
    in the root), an up and a down branch on a variable that is nonbasic there (a zero row of R), and an up branch beyond the variable's
    bound min_i b_i / A_ij (infeasible); B: one more down branch on every A child that the oracle solves; C: the rows of B's children,
    both new against the root (J = 2)."""
    from oracle import oracle as O
    O.set_threads(8)
    mm, nv, _ = ROOTS[66]
    c, A, b = _root(66)
    mask = synth.integrality_mask(nv, mm)

    def solve(cons):
        return O.simplex(*O.child_standard_form(c, A, b, list(cons)), 0.0, None, fast_initial_basis=True) if cons else \
            O.simplex(c, A, b, 0.0, None, fast_initial_basis=True)

    root = solve([])
    assert root.status == lp.OK and np.count_nonzero(root.x) == mm   # nondegenerate: x_j = 0 means nonbasic
    wave_a = down_branches(root.x, mask)
    assert len(wave_a) >= 2 and all(root.x[cons[0][0]] > 0 for cons in wave_a)   # basic in the parent
    j0 = max(j for j in range(nv) if mask[j] and root.x[j] == 0.0)                 # nonbasic in the parent
    wave_a += [[(j0, -1, -1.0)], [(j0, 1, 0.0)]]
    jb = wave_a[0][0][0]
    bound = min(b[i] / A[i, jb] for i in range(mm) if A[i, jb] > 0)
    wave_a.append([(jb, -1, -(math.floor(bound) + 1.0))])
    ref_a = [solve(cons) for cons in wave_a]
    assert ref_a[-1].status == lp.ERR_INFEASIBLE
    wave_b, par_b = [], []
    for i, (cons, o) in enumerate(zip(wave_a, ref_a)):
        if o.status != lp.OK:
            continue
        more = [t for t in down_branches(o.x[: nv + mm], mask) if t[0][0] != cons[0][0]]
        if more:
            wave_b.append(cons + more[0])
            par_b.append(i)
    assert len(wave_b) >= 2
    ref_b = [solve(cons) for cons in wave_b]
    return dict(root=root, A=wave_a, refA=ref_a, B=wave_b, parB=par_b, refB=ref_b)


def _ref_arrays(refs):
    return np.array([o.status for o in refs]), np.array([o.z for o in refs])


def test_small_shapes_against_the_oracle():
    """ldp != ld (children of the 66-row root: ld 68 against 66), ldp == ld (their children: 68 rows), J = 2 from the root; a branch
    variable basic in its parent and one nonbasic; an infeasible child.  warm_started = the children whose parent was kept."""
    S = _small()
    root = _root(66)
    pool = _pool(66)
    r0 = _keep_root(pool)
    _say("root 66 x 266", r0)
    assert r0.stats["warm_kept"] == 1 and r0.stats["batched_relaxations"] == 1
    assert abs(r0.z[0] - S["root"].z) <= 1e-9 * max(1.0, abs(S["root"].z))
    # A: every child starts from the kept root
    ra = _warm_wave(pool, S["A"], [0] * len(S["A"]), tag0=1)
    _say("wave A (m = 67, ld = 68, parent ld = 66)", ra)
    st_a, z_a = _ref_arrays(S["refA"])
    _check_contract(root, S["A"], ra, st_a, z_a, "A")
    assert ra.stats["warm_started"] == len(S["A"])
    assert ra.stats["batched_relaxations"] == len(S["A"]) and ra.stats["host_fallbacks"] == 0
    assert ra.stats["warm_kept"] == int((st_a == lp.OK).sum())
    assert (st_a == lp.ERR_INFEASIBLE).any() and ra.stats["pivots_dual"] > 0
    # B: children of A's children (all of them kept: their status is OK)
    rb = _warm_wave(pool, S["B"], [1 + i for i in S["parB"]], tag0=100)
    _say("wave B (m = 68, ld = 68 as the parent's)", rb)
    st_b, z_b = _ref_arrays(S["refB"])
    _check_contract(root, S["B"], rb, st_b, z_b, "B")
    assert rb.stats["warm_started"] == len(S["B"])
    # C: the same relaxations, two new rows against the root
    rc = _warm_wave(pool, S["B"], [0] * len(S["B"]), tag0=200, keep=0)
    _say("wave C (J = 2 from the root)", rc)
    _check_contract(root, S["B"], rc, st_b, z_b, "C")
    assert rc.stats["warm_started"] == len(S["B"]) and rc.stats["warm_kept"] == 0
    # a parent that was never kept, one that is no prefix, no parent at all: cold in the same run
    mixed = [S["B"][0], [S["B"][1][1], S["B"][1][0]], S["B"][0]]
    rm = _warm_wave(pool, mixed, [9999, 1 + S["parB"][1], -1], tag0=300, keep=0)
    _say("unknown tag / not a prefix / no parent", rm)
    assert rm.stats["warm_started"] == 0 and rm.stats["batched_relaxations"] == 3
    cold = pool.solve(mixed)
    assert np.array_equal(rm.status, cold.status) and np.array_equal(bits(rm.z), bits(cold.z)) and np.array_equal(bits(rm.x), bits(cold.x))
    pool.release_warm(-1)


# ---- 2. bit equality with the single-context warm start ----

@pytest.mark.parametrize("m", [260, 300])
def test_bit_equal_to_the_context_warm_start(m):
    """The D wave from the kept root on the pool against lp.Context (fused = 0: the three-kernel loop) with the root solved with keep and
    every child by solve(parent=root): status, has_x, z and x as bits, dual and Phase-II pivot totals — both run the helpers of
    simplex_helpers.h on the same B^-1."""
    c, A, b = _root(m)
    n0 = A.shape[1]
    wave = _wave(m, "D")
    pool = _pool(m)
    _keep_root(pool)
    r = _warm_wave(pool, wave, [0] * len(wave), keep=0)
    _say("wave D of the %d-row root" % m, r)
    assert r.stats["warm_started"] == len(wave) and r.stats["warm_fallbacks"] == 0
    cx = lp.Context(fused=0, exact_degenerate=1)
    pivd = piv2 = 0
    try:
        root = cx.upload(c, A, b)
        g0 = root.solve(keep=True)
        assert g0.status == lp.OK and g0.stats["warm"]["kept"] == 1
        for i, cons in enumerate(wave):
            ch = root.child(list(cons))
            g = ch.solve(parent=root, keep=False, dual_budget=BIG_BUDGET)
            ch.free()
            w = g.stats["warm"]
            print("child %d: context status %d z %.17g dual %d phase II %d | pool status %d z %.17g" % (
                i, g.status, g.z, w["pivots_dual"], g.stats["pivots_phase2"], r.status[i], r.z[i]))
            assert w["warm_started"] == 1 and w["fallback"] == 0, (i, w)
            pivd += w["pivots_dual"]
            piv2 += g.stats["pivots_phase2"]
            assert g.status == r.status[i], (i, g.status, r.status[i])
            assert (g.x is not None) == bool(r.has_x[i]), i
            assert bits(np.float64(g.z)) == bits(r.z[i]), (i, g.z, r.z[i])
            if g.x is not None:
                assert np.array_equal(bits(g.x[:n0]), bits(r.x[i][:n0])), i
    finally:
        cx.close()
    print("dual pivots: context %d pool %d; Phase-II pivots: context %d pool %d" % (pivd, r.stats["pivots_dual"], piv2, r.stats["pivots_phase2"]))
    assert pivd == r.stats["pivots_dual"] and piv2 == r.stats["pivots_phase2"]
    pool.release_warm(-1)


# ---- 3. against the reference ----

@pytest.mark.parametrize("m,name", [(260, "D"), (300, "D"), (260, "P"), (300, "P")])
def test_against_reference(m, name):
    """D (J = 1) and P (J = 6, 64 sign patterns, most of them infeasible) from the kept root against the oracle's fixture"""
    fx = _fixture(m)
    wave = _wave(m, name)
    pool = _pool(m)
    _keep_root(pool)
    r = _warm_wave(pool, wave, [0] * len(wave), keep=0)
    _say("wave %s of the %d-row root" % (name, m), r)
    print("warm_fallbacks %d pivots_dual %d" % (r.stats["warm_fallbacks"], r.stats["pivots_dual"]))
    _check_contract(_root(m), wave, r, fx[name + "_status"], fx[name + "_z"], "%s%d" % (name, m))
    assert r.stats["warm_started"] == len(wave)
    assert r.stats["batched_relaxations"] + r.stats["host_fallbacks"] == len(wave)
    pool.release_warm(-1)


# ---- 4. the tree ----

class _Recording:
    """a FrontierPool whose warm waves' stats are kept"""

    def __init__(self, pool):
        self._pool, self.waves = pool, []

    def __getattr__(self, k):
        return getattr(self._pool, k)

    def solve_warm(self, children, *a, **kw):
        r = self._pool.solve_warm(children, *a, **kw)
        self.waves.append(r.stats)
        return r


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


def test_tree_warm_on_the_batched_revised_simplex():
    """bnb.solve_milp(warm=True) on the 260 x 1040 MILP, 63 nodes: every solved node as in the oracle's tree; every node whose parent
    ended OK (and so was kept) starts warm.  Without the knob this tree runs cold on the workers: warm_started == 0.

    warm_started counts a handed-back relaxation too (as on the tableau schedule, and as the budget test below requires), so the nodes
    that stayed warm are warm_started - warm_fallbacks: those plus the fallbacks are the nodes with an OK parent.  (Measured at the
    default budget of 64 dual pivots: 63 such nodes, warm_started 63, warm_fallbacks 1.)"""
    mm, nv, seed = ROOTS[260]
    c, A, b = _root(260)
    rec = _Recording(_pool(260))
    res = bnb.solve_milp(c, A, b, None, None, list(synth.integrality_mask(nv, mm)), max_nodes=63, pool=rec, warm=True)
    fx = np.load(os.path.join(GOLD, "milp_wide260.npz"))
    nodes = [nd for nd in res.nodes if nd.status != -1]
    d = _first_difference(nodes, fx)
    started = sum(s["warm_started"] for s in rec.waves)
    fallbacks = sum(s["warm_fallbacks"] for s in rec.waves)
    by_id = {nd.id: nd for nd in nodes}
    want = sum(1 for nd in nodes if nd.id != 0 and by_id[nd.parent].status == lp.OK)
    print("tree: %d solved nodes (oracle %d), first node that differs: %s; warm_started %d, warm_fallbacks %d, nodes with an OK parent %d, "
          "dual pivots %d, pivots %d, batched per wave %s" % (len(nodes), len(fx["ids"]), "none" if d == len(nodes) else nodes[d].id, started,
                                                              fallbacks, want, res.pivots_dual, res.pivots,
                                                              [s["batched_relaxations"] for s in rec.waves]))
    assert d == len(nodes), nodes[d].id
    assert len(nodes) == len(fx["ids"]) and (res.error or "") == str(fx["error"])
    assert started > 0
    stayed = started - fallbacks
    assert stayed >= 0 and stayed + fallbacks == want
    assert any(s["batched_relaxations"] > 0 for s in rec.waves)


# ---- 5. the dual-pivot budget ----

def test_budget_hand_back_equals_the_cold_call():
    """dual_budget = 1 on the D wave of the 260-row root: a child that needs a second dual pivot is handed back, re-initialised in place and
    solved cold by the same run — bit for bit what pool.solve returns for it; a child that stayed warm keeps the contract of the
    reference.  The stats of a call are totals, so every child also runs as a call of its own: that tells which ones fell back."""
    fx = _fixture(260)
    wave = _wave(260, "D")
    pool = _pool(260)
    cold = pool.solve(wave)
    # one child per call: the stats of the call are the child's
    _keep_root(pool)
    nfb = 0
    for i, cons in enumerate(wave):
        r = pool.solve_warm([cons], parents=[0], tags=[1 + i], keep=[0], dual_budget=1)
        s = r.stats
        print("child %d: warm_started %d warm_fallbacks %d pivots_dual %d status %d z %.17g (cold %.17g)" % (
            i, s["warm_started"], s["warm_fallbacks"], s["pivots_dual"], r.status[0], r.z[0], cold.z[i]))
        assert s["warm_started"] == 1 and s["warm_fallbacks"] in (0, 1) and s["pivots_dual"] <= 1
        if s["warm_fallbacks"]:
            nfb += 1
            assert r.status[0] == cold.status[i] and r.has_x[0] == cold.has_x[i]
            assert bits(r.z[0]) == bits(cold.z[i]) and np.array_equal(bits(r.x[0]), bits(cold.x[i])), i
        else:
            _check_contract(_root(260), [cons], r, fx["D_status"][i:i + 1], fx["D_z"][i:i + 1], "D260[%d]" % i)
    # the whole wave in one run: the same counts, the handed-back children again equal to the cold call
    r = _warm_wave(pool, wave, [0] * len(wave), budget=1, keep=0)
    _say("wave D of the 260-row root, dual_budget = 1", r)
    assert r.stats["warm_started"] == len(wave) and r.stats["warm_fallbacks"] == nfb
    assert nfb > 0
    _check_contract(_root(260), wave, r, fx["D_status"], fx["D_z"], "D260")
    if nfb == len(wave):
        _same(r, cold)
    pool.release_warm(-1)


# ---- 6. nothing else moves ----

def _same(a, b):
    assert np.array_equal(a.status, b.status) and np.array_equal(a.has_x, b.has_x)
    assert np.array_equal(bits(a.z), bits(b.z)) and np.array_equal(bits(a.x), bits(b.x))


def test_knob_off_is_the_cold_worker_path():
    wave = _wave(260, "D")
    pool = _pool(260, warm_revised=0)
    _keep_root(pool)   # (a K = 0 relaxation of a wide root: on the workers too, nothing kept)
    r = _warm_wave(pool, wave, [0] * len(wave))
    _say("wave D, warm_revised = 0", r)
    assert r.stats["warm_started"] == 0 and r.stats["warm_kept"] == 0 and r.stats["batched_relaxations"] == 0
    _same(r, pool.solve(wave))


def test_cold_calls_do_not_look_at_the_knob():
    wave = _wave(260, "P")
    a = _pool(260, warm_revised=0).solve(wave)
    b = _pool(260, warm_revised=1).solve(wave)
    _same(a, b)
    for k in ("kernel_launches", "supersteps", "batched_relaxations", "host_fallbacks", "pivots_phase1", "pivots_phase2", "warm_started"):
        assert a.stats[k] == b.stats[k], (k, a.stats[k], b.stats[k])


def test_narrow_warm_wave_is_untouched():
    """the children of the 507 x 1014 root are narrow: the tableau schedule keeps them and starts their children warm, alike at either
    knob value"""
    mm, nv, _ = ROOTS[507]
    mask = synth.integrality_mask(nv, mm)
    out = []
    for knob in (0, 1):
        pool = _pool(507, warm_revised=knob)
        pool.release_warm(-1)
        r0 = pool.solve_root(0.0)
        assert r0.status == lp.OK
        first = down_branches(r0.x, mask)[:4]
        r1 = pool.solve_warm(first, tags=list(range(1, 1 + len(first))), keep=[1] * len(first))
        second, parents = [], []
        for i, cons in enumerate(first):
            more = [t for t in down_branches(r1.x[i], mask) if t[0][0] != cons[0][0]] if r1.status[i] == lp.OK else []
            if more:
                second.append(cons + more[0])
                parents.append(1 + i)
        assert second
        r2 = pool.solve_warm(second, parents=parents, tags=list(range(100, 100 + len(second))), keep=[0] * len(second))
        _say("narrow waves, warm_revised = %d: kept" % knob, r1)
        _say("narrow waves, warm_revised = %d: warm" % knob, r2)
        out.append((r1, r2))
        pool.release_warm(-1)
    for a, b in zip(*out):
        _same(a, b)
        for k in ("warm_started", "warm_fallbacks", "warm_kept", "pivots_dual", "batched_relaxations", "host_fallbacks", "pivots_phase1",
                  "pivots_phase2", "kernel_launches", "supersteps"):
            assert a.stats[k] == b.stats[k], (k, a.stats[k], b.stats[k])


def test_release_and_set_root_drop_the_entries():
    wave = _wave(260, "D")[:4]
    pool = _pool(260)
    _keep_root(pool)
    pool.release_warm(0)
    r = _warm_wave(pool, wave, [0] * len(wave), keep=0)
    assert r.stats["warm_started"] == 0 and r.stats["batched_relaxations"] + r.stats["host_fallbacks"] == len(wave)
    _same(r, pool.solve(wave))
    _keep_root(pool)
    assert _warm_wave(pool, wave, [0] * len(wave), keep=0).stats["warm_started"] == len(wave)
    pool.set_root(*_root(260))
    r = _warm_wave(pool, wave, [0] * len(wave), keep=0)
    assert r.stats["warm_started"] == 0
    _same(r, pool.solve(wave))
