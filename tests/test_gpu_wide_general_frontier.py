"""Wide frontier waves of roots WITHOUT a slack basis (equality rows, n - m >= 2m) on the device-batched revised simplex (pool knob
rev_general, DESIGN.md section 2.5e "Equality-form roots"): a child starts from its root's searched basis + its branch slacks
(k_rv_gen_start), Phase I takes its artificial column from k_rv_gen_art, the loops are the guarded (G = true) instances of K1-K3, and a
relaxation leaves the schedule for a worker's whole solve where its start or a pivot would be decided on a fresh gonum-order solve.

Against the live oracle per relaxation (status, z and x bits) and against the worker path of the same pool (rev_general = 0: the
same bits and the wave's pivot / Phase-I totals).  Roots: eqlp / deg_eq of tests/test_gpu_wide_general.py."""
import functools
import math

import numpy as np
import pytest

from gomilp_amd import lp, synth
from oracle import oracle as O
from tests.test_gpu_wide import BUDGET
from tests.test_gpu_wide_general import deg_eq, eqlp

pytestmark = pytest.mark.gpu

WORKERS = 4
ROOTS = {
    "phase1": ("eqlp", 1, 260, 24, 56, False),     # 80 x 316, the searched basis is infeasible: every child needs Phase I
    "feasible": ("eqlp", 2, 260, 24, 56, True),    # 80 x 316, the searched basis is feasible
    "large": ("eqlp", 3, 900, 40, 230, False),     # 270 x 1130: 68 workgroups per row kernel, two passes of the artificial column's rows
    "slack66": ("slack", 66, 1, 200),              # 66 x 266, slack basis: guarded on a worker at the default knobs
    "slack260": ("slack", 260, 1, 780),            # 260 x 1040, slack basis, more than 256 rows: the unguarded batched schedule
}
DEG_SEEDS = (0, 1, 2, 3)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def _root(name):
    key = ROOTS[name] if name in ROOTS else name
    if key[0] == "eqlp":
        return eqlp(*key[1:])
    if key[0] == "deg":
        return deg_eq(*key[1:])
    return synth.dense_lp_standard_form(*key[1:])


_pools = {}


def _pool(names, **knobs):
    """one pool per list of roots for the whole module; knobs are set per call"""
    if names not in _pools:
        p = lp.FrontierPool(workers=WORKERS)
        p.set_root(*_root(names[0]))
        for nm in names[1:]:
            p.add_root(*_root(nm))
        _pools[names] = p
    p = _pools[names]
    for k, v in {**dict(rev_general=1, rev_inplace=0, max_pivots=0), **knobs}.items():
        p.set(k, v)
    return p


@pytest.fixture(scope="module", autouse=True)
def _close_pools():
    yield
    for p in _pools.values():
        p.close()
    _pools.clear()


def branches(x, nstruct, nvars):
    """nvars down branches (j, 1, floor x_j), then nvars up branches (j, -1, -ceil x_j), on the first nvars nonzero structural variables"""
    picks = [j for j in range(nstruct) if x[j] != 0][:nvars]
    assert len(picks) == nvars
    return [[(j, 1, float(math.floor(x[j])))] for j in picks] + [[(j, -1, -float(math.ceil(x[j])))] for j in picks]


@functools.lru_cache(maxsize=None)
def _children(name):
    c, A, b = _root(name)
    if name == "large":   # (the root on the pool's first worker: the oracle is not run on this shape)
        r = _pool((name,)).solve_root(0.0)
        assert r.status == lp.OK
        # (variables above 1: a down branch with a zero right-hand side is degenerate here and takes a worker 15 to 25 s on either path)
        x = np.where(r.x > 1, r.x, 0.0)
        return branches(x, 900, 3)
    O.set_threads(8)
    o = O.simplex(c, A, b, 0.0, None, fast_initial_basis=True)
    assert o.status == O.OK
    return branches(o.x, 260, 12)


@functools.lru_cache(maxsize=None)
def _oracle_children(name):
    c, A, b = _root(name)
    O.set_threads(8)
    return [O.simplex(*O.child_standard_form(c, A, b, ch), 0.0, None, fast_initial_basis=True) for ch in _children(name)]


def _report(tag, r):
    s, count = r.stats, len(r.status)
    print("%s: %d relaxations, batched %d, host_fallbacks %d (share %.2f), supersteps %d, pivots %d + %d, bland %d, phase1 %d, launches %d, %.3f s" % (
        tag, count, s["batched_relaxations"], s["host_fallbacks"], s["host_fallbacks"] / max(count, 1), s["supersteps"], s["pivots_phase1"],
        s["pivots_phase2"], s["bland_steps"], s["phase1_runs"], s["kernel_launches"], s["seconds_total"]))


@functools.lru_cache(maxsize=None)
def _run(name, rev_general, rev_inplace=0):
    r = _pool((name,), rev_general=rev_general, rev_inplace=rev_inplace).solve(_children(name))
    _report("%s root, rev_general = %d, rev_inplace = %d" % (name, rev_general, rev_inplace), r)
    return r


def _assert_same_bits(a, b, totals=True):
    assert np.array_equal(a.status, b.status), (a.status, b.status)
    assert np.array_equal(a.has_x, b.has_x)
    assert np.array_equal(bits(a.z), bits(b.z)), np.flatnonzero(bits(a.z) != bits(b.z))
    assert np.array_equal(bits(a.x), bits(b.x)), np.flatnonzero((bits(a.x) != bits(b.x)).any(axis=1))
    for k in ("pivots_phase1", "pivots_phase2", "phase1_runs") if totals else ():
        assert a.stats[k] == b.stats[k], (k, a.stats[k], b.stats[k])


def _assert_oracle(r, name):
    n0 = _root(name)[1].shape[1]
    for i, oc in enumerate(_oracle_children(name)):
        assert r.status[i] == oc.status, (i, r.status[i], oc.status)
        if oc.x is None:
            assert not r.has_x[i], i
            continue
        assert r.has_x[i] and bits(r.z[i]) == bits(oc.z), (i, r.z[i], oc.z)
        assert np.array_equal(bits(r.x[i, :n0]), bits(oc.x[:n0])), i


SMALL = ["phase1", "feasible"]


@pytest.mark.parametrize("name", SMALL)
def test_roots_and_children_end_ok_on_the_oracle(name):
    """(a) 80 x 316: the root and its 24 children (12 down, 12 up branches) all end OK on the CPU oracle."""
    c, A, b = _root(name)
    assert A.shape == (80, 316)
    kids = _children(name)
    assert len(kids) == 24 and all(ch[0][0] < 316 - 80 for ch in kids)
    assert all(oc.status == O.OK for oc in _oracle_children(name))


@pytest.mark.parametrize("name", SMALL)
def test_wave_against_the_oracle_and_the_worker_path(name):
    """(b) the wave with rev_general = 1: per relaxation the oracle's status, z and x bits; against rev_general = 0 on the same pool the
    same bits and the wave's pivot and Phase-I totals."""
    r = _run(name, 1)
    _assert_oracle(r, name)
    _assert_same_bits(_run(name, 0), r)
    assert r.stats["bland_steps"] == 0 or r.stats["host_fallbacks"] > 0   # (a relaxation that stays takes no Bland step)


@pytest.mark.parametrize("name", SMALL)
def test_the_route_was_taken(name):
    """(c) every relaxation ran on the schedule or was handed over by it, and at least one ran; the worker path batches none."""
    r, w = _run(name, 1), _run(name, 0)
    s, count = r.stats, len(r.status)
    print("%s: share handed over %d / %d" % (name, s["host_fallbacks"], count))
    assert s["batched_relaxations"] + s["host_fallbacks"] == count
    assert s["batched_relaxations"] >= 1 and s["supersteps"] > 0
    assert w.stats["batched_relaxations"] == 0 and w.stats["host_fallbacks"] == 0


@pytest.mark.parametrize("name", SMALL)
def test_root_in_place_gives_the_same_bits(name):
    """(d) rev_inplace = 1: the artificial column and every child column through ChildCol — the bits of (b), the same hand-overs."""
    r, p = _run(name, 1), _run(name, 1, 1)
    _assert_oracle(p, name)
    _assert_same_bits(r, p)
    assert p.stats["batched_relaxations"] == r.stats["batched_relaxations"] and p.stats["host_fallbacks"] == r.stats["host_fallbacks"]


@pytest.mark.parametrize("slack", ["slack66", "slack260"])
def test_mixed_wave_of_slack_and_general_roots(slack):
    """(e) the K = 0 relaxations of both 80 x 316 roots and of one slack wide root in one gomilp_frontier_solve_roots wave: each equals its
    own single-root wave bit for bit, and the slack relaxation equals its result at rev_general = 0.  The 66-row slack root is guarded on
    a worker at the default knobs (exact_degenerate = 1, up to 256 rows), so its wave runs where it ran before; the 260-row one passes the
    unguarded test, and the wave is one schedule with both kinds of loop launches."""
    names = ("phase1", "feasible", slack)
    wave, rof = [[], [], []], [0, 1, 2]
    mixed = _pool(names).solve(wave, roots=rof)
    _report("mixed wave with %s" % slack, mixed)
    off = _pool(names, rev_general=0).solve(wave, roots=rof)
    assert mixed.status[2] == off.status[2] and bits(mixed.z[2]) == bits(off.z[2]) and np.array_equal(bits(mixed.x[2]), bits(off.x[2]))
    for i in range(3):
        alone = _pool(names).solve([[]], roots=[i])
        assert mixed.status[i] == alone.status[0] and mixed.has_x[i] == alone.has_x[0], i
        assert bits(mixed.z[i]) == bits(alone.z[0]) and np.array_equal(bits(mixed.x[i]), bits(alone.x[0])), i
    _assert_same_bits(off, mixed)
    if slack == "slack260":
        assert mixed.stats["batched_relaxations"] + mixed.stats["host_fallbacks"] == 3 and mixed.stats["batched_relaxations"] >= 2
        assert off.stats["batched_relaxations"] == 0


def test_larger_shape_against_the_worker_path():
    """(f) 270 x 1130 with six children: ld = 272 > 256, so k_rv_gen_art and k_rv_gen_start take two passes.  Against the worker path only.
    Beyond 96 rows the route is taken with rev_general = 2 only (it is slower than the workers there)."""
    c, A, b = _root("large")
    assert A.shape == (270, 1130)
    assert _run("large", 1).stats["batched_relaxations"] == 0
    r, w = _run("large", 2), _run("large", 0)
    assert len(r.status) == 6
    _assert_same_bits(w, r)
    assert r.stats["batched_relaxations"] + r.stats["host_fallbacks"] == 6 and r.stats["batched_relaxations"] >= 1


def test_hand_over_on_degenerate_integer_data():
    """(g) deg_eq(80, 240, seed), 80 x 300 (n - m = 220 >= 2 * 82), max_pivots = BUDGET: integer data with zero-level rows and ties — the
    start guard and the loop guard hand relaxations to a worker's whole solve, and every relaxation equals the worker path bit for bit."""
    names = tuple(("deg", 80, 240, s) for s in DEG_SEEDS)
    for nm in names:
        A = _root(nm)[1]
        assert A.shape[1] - A.shape[0] >= 2 * (A.shape[0] + 2)
    wave, rof = [], []
    for i in range(len(names)):
        wave += [[], [(0, 1, 1.0)], [(0, -1, -1.0), (1, 1, 0.0)]]
        rof += [i] * 3
    r = _pool(names, max_pivots=BUDGET).solve(wave, roots=rof)
    _report("degenerate wave", r)
    w = _pool(names, max_pivots=BUDGET, rev_general=0).solve(wave, roots=rof)
    _assert_same_bits(w, r)
    assert r.stats["batched_relaxations"] + r.stats["host_fallbacks"] == len(wave)
    assert r.stats["host_fallbacks"] >= 1
    assert w.stats["batched_relaxations"] == 0
