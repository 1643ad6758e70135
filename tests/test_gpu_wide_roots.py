"""Wide frontier waves of SEVERAL roots on the device-batched revised simplex (pool knobs batch_revised / rev_roots):
FrontierPool.solve(children, roots=...) with wide roots runs as one schedule when every root the wave uses passes that schedule's test.
The results must be, bit for bit, those of the worker path (batch_revised = 0, rev_roots = 0), those of each relaxation in a wave of its
own root alone, and independent of which root the pool holds as root 0; against the reference they keep the contract of
tests/test_gpu_wide_frontier.py.

Roots and waves as in that file: R260 = dense_lp_standard_form(260, 1, 780), R300 = (300, 2, 1200); wave P: the 64 sign patterns of 6
branch rows, wave D: one down branch per fractional integer variable, both on the oracle's root optimum (fixtures
tests/golden/wide_frontier_*.npz).  The mixed wave M: the K = 0 child of each root, both D waves (8 + 14), both P waves (64 + 64) — 152
relaxations, 73 of R260 and 79 of R300.  Inside each root they are spread by a fixed stride, then the two lists alternate, R300 first:
list neighbours belong to different roots, except for the six relaxations R300 has more than R260, which close the list."""
import functools
import math
import os

import numpy as np
import pytest

from gomilp_amd import lp, synth

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROOTS = {260: (260, 780, 1), 300: (300, 1200, 2)}
SMALL = {66: (66, 200, 1), 80: (80, 330, 2), 70: (70, 560, 3)}
WORKERS = 8
TOTALS = ("pivots_phase1", "pivots_phase2", "bland_steps", "phase1_runs")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def _fixture(m):
    return dict(np.load(os.path.join(GOLD, "wide_frontier_%d_%d_%d.npz" % ROOTS[m])))


@functools.lru_cache(maxsize=None)
def _root(m):
    mm, nv, seed = {**ROOTS, **SMALL}[m]
    return synth.dense_lp_standard_form(mm, seed, nv)


def _width(m):
    mm, nv, _ = {**ROOTS, **SMALL}[m]
    return nv + mm


def down_branches(root_x, mask):
    return [[(j, 1, float(math.floor(root_x[j])))] for j in range(len(mask) - 1, -1, -1) if mask[j] and root_x[j] != math.floor(root_x[j])]


@functools.lru_cache(maxsize=None)
def _wave(m, name):
    mm, nv, _ = ROOTS[m]
    mask = synth.integrality_mask(nv, mm)
    root_x = _fixture(m)["root_x"]
    return down_branches(root_x, mask) if name == "D" else synth.frontier_children(root_x, mask, 6)


def _spread(items, stride):
    """a fixed permutation: position t takes item t * stride mod len (stride coprime to len)"""
    n = len(items)
    assert math.gcd(stride, n) == 1
    return [items[(t * stride) % n] for t in range(n)]


def _interleave(a, b):
    """b first, then alternating; what one list has more closes the list"""
    out = []
    for t in range(max(len(a), len(b))):
        if t < len(b):
            out.append(b[t])
        if t < len(a):
            out.append(a[t])
    return out


@functools.lru_cache(maxsize=None)
def _mixed():
    """M as a list of (root, wave name, index in that wave, constraints)"""
    per = {}
    for m in (260, 300):
        per[m] = [(m, "K0", 0, [])] + [(m, "D", i, c) for i, c in enumerate(_wave(m, "D"))] + [(m, "P", i, c) for i, c in enumerate(_wave(m, "P"))]
    assert (len(per[260]), len(per[300])) == (73, 79)
    M = _interleave(_spread(per[260], 31), _spread(per[300], 34))
    assert len(M) == 152 and sum(M[t][0] == M[t + 1][0] for t in range(len(M) - 1)) == 5   # (the six surplus relaxations of R300)
    return M


_pools = {}


def _pool(key, roots, workers=WORKERS, **knobs):
    """one pool per list of roots for the whole module (roots[0] is the set_root problem); the knobs of every call are set here"""
    if key not in _pools:
        p = lp.FrontierPool(workers=workers)
        p.set_root(*_root(roots[0]))
        for m in roots[1:]:
            p.add_root(*_root(m))
        _pools[key] = p
    p = _pools[key]
    for k, v in {**dict(batch_revised=1, rev_roots=1, rev_exchange=1, warm_revised=0, exact_degenerate=1, max_pivots=0), **knobs}.items():
        p.set(k, v)
    return p


@pytest.fixture(scope="module", autouse=True)
def _close_pools():
    yield
    for p in _pools.values():
        p.close()
    _pools.clear()


def _say(label, r):
    s = r.stats
    print("%s: %d relaxations, batched %d, host_fallbacks %d, supersteps %d, pivots %d + %d, bland %d, phase1 %d, launches %d, %.3f s" % (
        label, len(r.status), s["batched_relaxations"], s["host_fallbacks"], s["supersteps"], s["pivots_phase1"], s["pivots_phase2"],
        s["bland_steps"], s["phase1_runs"], s["kernel_launches"], s["seconds_total"]))


@functools.lru_cache(maxsize=None)
def _run_mixed(first, batch_revised, rev_roots):
    """M on the pool whose root 0 is `first` (260: set_root(R260) + add_root(R300); 300: the other way round)"""
    order = (260, 300) if first == 260 else (300, 260)
    M = _mixed()
    r = _pool("two-%d" % first, order, batch_revised=batch_revised, rev_roots=rev_roots).solve(
        [e[3] for e in M], roots=[order.index(e[0]) for e in M])
    _say("M, root 0 = R%d, batch_revised = %d, rev_roots = %d" % (first, batch_revised, rev_roots), r)
    return r


@functools.lru_cache(maxsize=None)
def _run_alone(m):
    """the relaxations of M that belong to root m, in M's order, as a single-root wave on a pool that holds this root only"""
    r = _pool("one-%d" % m, (m,)).solve([e[3] for e in _mixed() if e[0] == m])
    _say("the relaxations of R%d alone" % m, r)
    return r


def _runs_batched(r):
    s, count = r.stats, len(r.status)
    print("batched_relaxations %d host_fallbacks %d supersteps %d of %d" % (s["batched_relaxations"], s["host_fallbacks"], s["supersteps"], count))
    assert s["batched_relaxations"] + s["host_fallbacks"] == count
    assert s["host_fallbacks"] <= count // 8
    assert s["supersteps"] > 0


def _same_bits(a, b, widths, totals=True):
    """status, has_x and z by bits, of every row of x its root's part; the pivot / Bland / Phase-I totals"""
    assert np.array_equal(a.status, b.status), np.flatnonzero(a.status != b.status)
    assert np.array_equal(a.has_x, b.has_x)
    assert np.array_equal(bits(a.z), bits(b.z)), np.flatnonzero(bits(a.z) != bits(b.z))
    for i, n in enumerate(widths):
        assert np.array_equal(bits(a.x[i][:n]), bits(b.x[i][:n])), i
    for k in TOTALS if totals else ():
        assert a.stats[k] == b.stats[k], (k, a.stats[k], b.stats[k])


def _same_row(a, i, b, k, n, what):
    assert a.status[i] == b.status[k] and a.has_x[i] == b.has_x[k], (what, a.status[i], b.status[k])
    assert bits(a.z[i]) == bits(b.z[k]), (what, a.z[i], b.z[k])
    assert np.array_equal(bits(a.x[i][:n]), bits(b.x[k][:n])), what


def _mixed_widths():
    return [_width(e[0]) for e in _mixed()]


# ---- 1 ----

def test_mixed_wave_runs_batched():
    """The wave of two wide roots runs on the batched revised simplex (before this routing it went to the workers whole:
    batched_relaxations = 0); the cap on the Phase-I hand-overs is that of test_gpu_wide_frontier.py::test_wide_wave_runs_batched."""
    _runs_batched(_run_mixed(260, 1, 1))


# ---- 2 ----

def test_mixed_wave_bit_equal_to_worker_path():
    a, b = _run_mixed(260, 0, 1), _run_mixed(260, 1, 1)
    assert a.stats["batched_relaxations"] == 0 and a.stats["supersteps"] == 0
    _same_bits(a, b, _mixed_widths())


def test_rev_roots_off_is_the_worker_path():
    a, b = _run_mixed(260, 1, 0), _run_mixed(260, 1, 1)
    assert a.stats["batched_relaxations"] == 0 and a.stats["host_fallbacks"] == 0 and a.stats["supersteps"] == 0
    _same_bits(a, b, _mixed_widths())


# ---- 3 ----

@pytest.mark.parametrize("m", [260, 300])
def test_independent_of_the_neighbours(m):
    """every relaxation of M against the same relaxation in the single-root wave of its own root (a pool that holds that root only)"""
    r, alone = _run_mixed(260, 1, 1), _run_alone(m)
    idx = [i for i, e in enumerate(_mixed()) if e[0] == m]
    assert len(idx) == len(alone.status)
    _runs_batched(alone)
    for k, i in enumerate(idx):
        _same_row(r, i, alone, k, _width(m), _mixed()[i][:3])


# ---- 4 ----

def test_root_zero_is_not_special():
    """set_root(R300) + add_root(R260): the re-indexed wave gives every relaxation the same bits, and the same totals"""
    a, b = _run_mixed(260, 1, 1), _run_mixed(300, 1, 1)
    _runs_batched(b)
    _same_bits(a, b, _mixed_widths())
    _same_bits(_run_mixed(300, 0, 1), b, _mixed_widths())


# ---- 5 ----

def _against_reference(r):
    """the per-child contract of test_gpu_wide_frontier.py::_against_reference; returns how many relaxations equal the oracle's bits"""
    equal = 0
    for i, (m, name, k, cons) in enumerate(_mixed()):
        fx = _fixture(m)
        c, A, b = _root(m)
        n0 = A.shape[1]
        if name == "K0":
            st, z, hx, x = lp.OK, fx["root_z"], 1, fx["root_x"]
        else:
            st, z, hx, x = fx[name + "_status"][k], fx[name + "_z"][k], fx[name + "_has_x"][k], fx[name + "_x"][k]
        assert r.status[i] == st, (i, m, name, k, lp.STATUS_NAMES.get(int(r.status[i])), int(st))
        if hx:
            assert r.has_x[i]
            assert abs(r.z[i] - z) <= 1e-9 * max(1.0, abs(z)), (i, m, name, k, r.z[i], z)
            xi = r.x[i][:n0]
            assert xi.min() >= -1e-9 and np.abs(A @ xi - b).max() <= 1e-9 * max(1.0, np.abs(b).max()), (i, m, name, k)
            for (j, sign, rhs) in cons:
                assert sign * xi[j] <= rhs + 1e-9 * max(1.0, abs(rhs)), (i, m, name, k, j)
            equal += int(bits(np.float64(r.z[i])) == bits(np.float64(z)) and np.array_equal(bits(xi), bits(np.asarray(x)[:n0])))
        else:
            assert not r.has_x[i]
            equal += 1
    return equal


def test_mixed_wave_against_reference():
    e1 = _against_reference(_run_mixed(260, 1, 1))
    e0 = _against_reference(_run_mixed(260, 0, 1))
    print("M: %d of %d relaxations equal the oracle bit for bit (batch_revised = 0: %d)" % (e1, len(_mixed()), e0))
    assert e1 == e0


# ---- 6 ----

@functools.lru_cache(maxsize=None)
def _small_wave():
    """three small wide roots that differ in ld, nn and pricing grid; the K = 0 child of each and a 3-row P wave (8 children) per root on
    the optimum the pool computes (an extra root's optimum comes from its K = 0 child); neighbours of different roots"""
    order = tuple(SMALL)
    pool = _pool("small", order, workers=4, exact_degenerate=0)
    r0 = pool.solve([[], [], []], roots=[0, 1, 2])
    assert list(r0.status) == [lp.OK] * 3
    per = []
    for t, m in enumerate(order):
        mm, nv, _ = SMALL[m]
        kids = synth.frontier_children(r0.x[t][: nv + mm], synth.integrality_mask(nv, mm), 3)
        assert len(kids) == 8
        per.append([(m, [])] + [(m, c) for c in kids])
    return [per[t][k] for k in range(9) for t in range(3)]


@functools.lru_cache(maxsize=None)
def _run_small(batch_revised, rev_roots):
    order = tuple(SMALL)
    W = _small_wave()
    r = _pool("small", order, workers=4, exact_degenerate=0, batch_revised=batch_revised, rev_roots=rev_roots).solve(
        [e[1] for e in W], roots=[order.index(e[0]) for e in W])
    _say("small roots, batch_revised = %d, rev_roots = %d" % (batch_revised, rev_roots), r)
    return r


def test_smallest_shapes():
    """66 rows (one partly filled wave of lanes), 80 and 70 rows with 330 and 560 structural columns, exact_degenerate = 0 and cond_guard
    at its default: runs batched, equals the worker path at either knob, and every relaxation equals its root's own single-root wave"""
    W = _small_wave()
    widths = [_width(e[0]) for e in W]
    b = _run_small(1, 1)
    _runs_batched(b)
    a = _run_small(0, 1)
    assert a.stats["batched_relaxations"] == 0
    _same_bits(a, b, widths)
    a = _run_small(1, 0)
    assert a.stats["batched_relaxations"] == 0 and a.stats["supersteps"] == 0
    _same_bits(a, b, widths)
    for m in SMALL:
        idx = [i for i, e in enumerate(W) if e[0] == m]
        alone = _pool("small-%d" % m, (m,), workers=4, exact_degenerate=0).solve([W[i][1] for i in idx])
        _say("the %d-row root alone" % m, alone)
        _runs_batched(alone)
        for k, i in enumerate(idx):
            _same_row(b, i, alone, k, _width(m), (m, k))


# ---- 7 ----

def test_unused_extra_root_does_not_change_the_routing():
    """(a) the single-root P wave of R260 on the pool that also holds R300: still batched, the bits of the pool without an extra root"""
    wave = _wave(260, "P")
    a = _pool("one-260", (260,)).solve(wave)
    for rev_roots in (1, 0):   # (a wave of root 0 alone is no wave of several roots: the knob does not touch it)
        b = _pool("two-260", (260, 300), rev_roots=rev_roots).solve(wave)
        _say("wave P of R260, R300 held but unused, rev_roots = %d" % rev_roots, b)
        _runs_batched(b)
        _same_bits(a, b, [_width(260)] * len(wave))
        assert b.stats["supersteps"] == a.stats["supersteps"]


def test_wave_with_a_narrow_root_goes_where_it_went_and_set_root_drops_the_extras():
    """(b) R260 plus the narrow C5 root (512 x 1024) in one wave: not taken by the revised schedule, whole — the same relaxation counts
    and bits at batch_revised 0 and 1.  (c) set_root again: the added root is gone (roots=[1] is BAD_SHAPE), a single-root wave runs
    batched."""
    m5, seed5 = synth.CONFIGS["C5"]
    key = "narrow"
    assert key not in _pools
    p = lp.FrontierPool(workers=WORKERS)
    p.set_root(*_root(260))
    p.add_root(*synth.dense_lp_standard_form(m5, seed5))
    _pools[key] = p
    wave = _wave(260, "P")[:6] + [[], [(0, 1, 0.0)]]
    roots = [0] * 6 + [1, 1]
    res = []
    for knob in (0, 1):
        r = _pool(key, None, batch_revised=knob).solve(wave, roots=roots)
        _say("R260 + C5, batch_revised = %d" % knob, r)
        res.append(r)
    a, b = res
    assert (a.stats["batched_relaxations"], a.stats["host_fallbacks"]) == (b.stats["batched_relaxations"], b.stats["host_fallbacks"])
    assert b.stats["batched_relaxations"] == 0 and b.stats["supersteps"] == 0   # (no schedule takes a wave of a wide and a narrow root)
    _same_bits(a, b, [_width(260)] * 6 + [2 * m5] * 2)
    # (c)
    p.set_root(*_root(260))
    _pool(key, None)
    with pytest.raises(RuntimeError):
        p.solve([[]], roots=[1])
    r = p.solve(_wave(260, "D"))
    _say("wave D of R260 after set_root", r)
    _runs_batched(r)
    alone = _run_alone(260)
    idx = {e[2]: k for k, e in enumerate([e for e in _mixed() if e[0] == 260]) if e[1] == "D"}
    for i in range(len(r.status)):
        _same_row(r, i, alone, idx[i], _width(260), ("D", i))


# ---- 8 ----

def _two_generations(pool):
    """R260: the root kept, wave D warm from it (kept), then every D child with one more row — the next down branch of the list"""
    D = _wave(260, "D")
    pool.release_warm(-1)
    r0 = pool.solve_warm([[]], tags=[0], keep=[1])
    assert r0.status[0] == lp.OK
    g1 = pool.solve_warm(D, parents=[0] * len(D), tags=list(range(1, 1 + len(D))), keep=[1] * len(D), dual_budget=4096)
    wave2 = [D[i] + D[(i + 1) % len(D)] for i in range(len(D))]
    g2 = pool.solve_warm(wave2, parents=list(range(1, 1 + len(D))), tags=[-1] * len(D), keep=[0] * len(D), dual_budget=4096)
    pool.release_warm(-1)
    return g1, g2


def test_warm_call_with_an_extra_root_present():
    """gomilp_frontier_solve_warm names no roots: a wave of root 0, on the schedule whatever else the pool holds"""
    with_extra = _two_generations(_pool("two-260", (260, 300), warm_revised=1))
    without = _two_generations(_pool("one-260", (260,), warm_revised=1))
    _pool("two-260", (260, 300))
    _pool("one-260", (260,))
    for gen, (a, b) in enumerate(zip(with_extra, without), 1):
        s = a.stats
        print("generation %d with R300 held: warm_started %d, warm_fallbacks %d, batched %d, host_fallbacks %d (without: warm_started %d)" % (
            gen, s["warm_started"], s["warm_fallbacks"], s["batched_relaxations"], s["host_fallbacks"], b.stats["warm_started"]))
        assert s["warm_started"] > 0
        assert np.array_equal(a.status, b.status), (a.status, b.status)
        assert np.array_equal(a.has_x, b.has_x)
        for i in range(len(a.status)):
            if a.has_x[i]:
                assert abs(a.z[i] - b.z[i]) <= 1e-9 * max(1.0, abs(b.z[i])), (gen, i, a.z[i], b.z[i])


# ---- 9 ----

def test_launch_count_of_a_cold_wave():
    """kernel_launches against the schedule's own definition, where it can be derived by hand: one cold wave of 4 one-row children of the
    66 x 200 root (the first four down branches on its optimum), assembled (rev_inplace = 0) and in place (rev_inplace = 1).

    From the wrapper bodies of batch_revised.hip: the start of a cold wave of slack roots is launch_rv_assemble (k_rv_assemble; none with
    rev_inplace) + launch_rv_init (k_rv_init) = 2 launches, 1 in place.  A superstep s without a dual loop, a searched start or an
    exchange is launch_rv_setup (K2 + K3 of the forced pivot, k_rv_lists, k_rv_matvec, k_rv_y_partial, k_rv_y_reduce, k_rv_check = 7),
    chunk_s times launch_rv_pivot (k_rv_bland, K1, K2, K3 = 4) with chunk_s = 8 for s < 2 and 32 behind, and launch_rv_ctrl (1).  So the
    schedule launches 2 + sum over s < supersteps of (7 + 4 chunk_s + 1) kernels, and one fewer in place.

    The pool reports the schedule's launches and those of the workers' final solves (worker_step) as one sum and exposes neither alone, so
    what is asserted is the part that the two runs pin between them: the same supersteps, and exactly one launch more assembled than in
    place — the assemble term.  (The final solves are the same launches in both runs: the bases are equal bit for bit.)  The closed form
    and what the pool reports beyond it are printed."""
    mm, nv, _ = SMALL[66]

    def pool(inplace):
        return _pool("small-66", (66,), workers=4, exact_degenerate=0, rev_inplace=inplace, large_rows=0)

    try:
        r0 = pool(0).solve([[]])
        assert r0.status[0] == lp.OK
        kids = down_branches(r0.x[0][: nv + mm], synth.integrality_mask(nv, mm))[:4]
        assert len(kids) == 4 and all(len(c) == 1 for c in kids)
        runs = []
        for inplace in (0, 1):
            r = pool(inplace).solve(kids)
            s = r.stats
            _say("4 one-row children of the 66-row root, rev_inplace = %d" % inplace, r)
            closed = (2 - inplace) + sum(7 + 4 * (8 if t < 2 else 32) + 1 for t in range(s["supersteps"]))
            print("  art_exchanges %d, warm_started %d; the schedule's closed form: %d launches, reported beyond it: %d" % (
                s["art_exchanges"], s["warm_started"], closed, s["kernel_launches"] - closed))
            assert (s["batched_relaxations"], s["host_fallbacks"], s["art_exchanges"], s["warm_started"]) == (4, 0, 0, 0)
            runs.append(r)
    finally:
        pool(0)
    a, b = runs
    _same_bits(a, b, [_width(66)] * 4)
    assert a.stats["supersteps"] == b.stats["supersteps"] > 0
    assert a.stats["kernel_launches"] - b.stats["kernel_launches"] == 1
