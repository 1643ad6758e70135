"""General starts wider than the tableau: equality rows (no slack basis, the column search of simplex.go:611-637) or a supplied
initial_basic, with n - m > 8191 — the tableau's row no longer fits the 64 KB LDS window, and such a start takes the three-kernel
revised loop with the exact-step guard (LPArgs::guard: degenerate, tied and tiny pivots stop the kernels, ST_NEED_EXACT, and are
decided on fresh gonum-order solves).  The same loop runs the committed EQ fixtures with the knob tableau = 0.
Against the live oracle; integer data through test_gpu_wide's _check: status, the five trace fields of every pivot, pivots per
phase, the positional final basis, x and z bits."""
import functools
import os
import sys

import numpy as np
import pytest

from gomilp_amd import lp, synth
from oracle import oracle as O
from tests.test_gpu_wide import BUDGET, TAB, _check, five

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REVISED = "three-kernel"


def eqlp(seed, N, E, I, feasible=False):
    """tools/gen_golden.py eqlp_problem with separate row counts: E Gaussian equality rows, I inequality rows over N variables.
    feasible: x0 zero but for its last E entries — the searched basis (the I slacks, the last E structural columns) is feasible."""
    rng = np.random.default_rng(seed)
    x0 = np.abs(rng.standard_normal(N))
    if feasible:
        x0 = x0 + 0.1
        x0[:N - E] = 0.0
    A = rng.standard_normal((E, N)); b = A @ x0
    G = rng.standard_normal((I, N)); h = G @ x0 + np.abs(rng.standard_normal(I))
    c = np.abs(rng.standard_normal(N))
    return O.convert_to_equalities(c, A, b, G, h)


def deg_eq(m, nv, seed):
    """Integer data as synth.wide_degenerate_lp, rows 0 .. m // 4 - 1 equalities without a slack (row 0 >= 1: every column
    bounded), b = G x0 for a 0 / 1 / 2 point on m // 2 columns, the inequality rows' b raised by 0 / 0 / 1 / 2, m // 4 duplicates
    among the inequality rows, c = [-(0..4), 0]."""
    rng = np.random.default_rng(9000 + 7919 * m + seed)
    E = m // 4
    G = rng.integers(0, 4, (m, nv)).astype(float)
    G[0] = np.maximum(G[0], 1.0)
    x0 = np.zeros(nv)
    x0[rng.choice(nv, size=m // 2, replace=False)] = rng.integers(0, 3, m // 2)
    b = G @ x0
    b[E:] += rng.choice([0.0, 0.0, 1.0, 2.0], size=m - E)
    ndup = m // 4
    dst = rng.choice(np.arange(E, m), size=ndup, replace=False)
    src = rng.choice(np.setdiff1d(np.arange(E, m), dst), size=ndup)
    G[dst], b[dst] = G[src], b[src]
    c = np.concatenate([-rng.integers(0, 5, nv).astype(float), np.zeros(m - E)])
    A = np.zeros((m, nv + m - E))
    A[:, :nv] = G
    A[np.arange(E, m), nv + np.arange(m - E)] = 1.0
    return c, A, b


@functools.lru_cache(maxsize=None)
def _problem(key):
    kind = key[0]
    if kind == "eqlp":
        return eqlp(*key[1:])
    if kind == "deg":
        return deg_eq(*key[1:])
    raise KeyError(key)


@functools.lru_cache(maxsize=None)
def _oracle(key, initial_basic=None):
    c, A, b = _problem(key)
    O.set_threads(8)
    ib = None if initial_basic is None else np.array(initial_basic, dtype=np.int64)
    return O.simplex(c, A, b, 0.0, ib, fast_initial_basis=True, trace=True, stop_after_pivots=BUDGET if key[0] == "deg" else -1)


@functools.lru_cache(maxsize=None)
def _solve(key, knobs=(), initial_basic=None):
    c, A, b = _problem(key)
    kn = dict(knobs)
    if key[0] == "deg":
        kn.setdefault("max_pivots", BUDGET)
    cx = lp.Context(**kn)
    try:
        ib = None if initial_basic is None else np.array(initial_basic, dtype=np.int64)
        return cx.upload(c, A, b).solve(0.0, trace=True, initial_basic=ib)
    finally:
        cx.close()


def _wide(key):
    c, A, b = _problem(key)
    return A.shape[1] - A.shape[0]


BOUNDARY = {8231: TAB, 8232: (REVISED,)}


@pytest.mark.parametrize("N", sorted(BOUNDARY))
def test_boundary_of_the_tableau_row(N):
    """64 x 8255 (n - m = 8191: the tableau row fits) stays on the blocked tableau; 64 x 8256 (n - m = 8192) takes the guarded
    three-kernel loop.  Host column search (64 rows), Phase I; both bit for bit."""
    key = ("eqlp", 1, N, 40, 24)
    assert _wide(key) == N - 40
    o = _oracle(key)
    g = _solve(key)
    assert g.stats["pipeline"] in BOUNDARY[N], g.stats["pipeline"]
    _check(g, o, "eqlp 64 x %d" % (N + 24))


WIDE = {"phase1": ("eqlp", 1, 9000, 100, 60, False), "feasible": ("eqlp", 1, 9000, 100, 60, True)}


@pytest.mark.parametrize("name", sorted(WIDE))
def test_device_search_both_phases(name):
    """160 x 9060 (n - m = 8900): the device column search (96 rows and more), B^-1 handed over in place, with Phase I (an infeasible
    searched basis: the artificial column by k_gs_art, the forced pivot, the zero-level exchange) and without.  Bit for bit in the
    default mode; mode 0 (guard off: today's kernel instances on the new route) ends at the reference's optimum."""
    key = WIDE[name]
    o = _oracle(key)
    g = _solve(key)
    assert g.stats["pipeline"] == REVISED
    assert g.stats["phase1_used"] == (1 if name == "phase1" else 0)
    _check(g, o, "160 x 9060 %s" % name)
    g0 = _solve(key, (("exact_degenerate", 0),))
    assert g0.stats["pipeline"] == REVISED
    print("mode 0: %d + %d pivots, trace identical: %s" % (g0.stats["pivots_phase1"], g0.stats["pivots_phase2"], five(g0.pivots) == five(o.pivots)))
    assert g0.status == lp.OK and abs(g0.z - o.z) <= 1e-9 * max(1.0, abs(o.z)), (g0.status, g0.z, o.z)


def test_supplied_basis_beyond_the_tableau_row():
    """initial_basic = the oracle's final basis of the feasible 160 x 9060 LP: the new route, no pivot, x and z of the oracle's run
    with the same initial_basic."""
    key = WIDE["feasible"]
    basis = tuple(int(j) for j in _oracle(key).basis)
    o = _oracle(key, basis)
    assert o.status == O.OK
    g = _solve(key, (), basis)
    assert g.stats["pipeline"] == REVISED
    assert g.status == lp.OK and g.stats["pivots_phase1"] + g.stats["pivots_phase2"] == 0
    assert np.array_equal(g.x, o.x) and g.z == o.z


DEG = [(m, m // 4 + 8192, seed) for m in (48, 128) for seed in range(4)]
# (m, seed, mode) -> the first pivot that differs: the 1e-9 guard misses a tie the reference's rounding decides (modes 1 / 2 only)
TIE_MISSED = {(48, 1, 1): 104, (48, 1, 2): 104, (128, 0, 1): 124, (128, 0, 2): 124}


def _feasible_and_dual_feasible(g, problem):
    c, A, b = problem
    assert g.x.min() >= -1e-9 and np.abs(A @ g.x - b).max() <= 1e-9 * max(1.0, np.abs(b).max())
    y = np.linalg.solve(A[:, g.basis].T, c[g.basis])
    assert (c - A.T @ y).min() >= -1e-9


@pytest.mark.parametrize("mode", [3, 1, 2])
@pytest.mark.parametrize("m,nv,seed", DEG)
def test_degenerate_equality_rows(m, nv, seed, mode):
    """Integer data with equality rows, n - m = 8192: ties, zero-level rows, Bland steps, cycles, mat.Condition exits.  Mode 3
    (strict: every decision, the stop test included, on fresh solves) bit for bit everywhere, mat.Condition through the exact steps'
    fresh condition numbers.  Modes 1 / 2 bit for bit where the reference ends OK or cycles; where it leaves with mat.Condition the
    engine may go on (general starts beyond 64 rows have no condition guard but the exact steps' — DESIGN.md §3): OK or
    ERR_CONDITION, an OK point feasible and dual feasible."""
    key = ("deg", m, nv, seed)
    assert _wide(key) == 8192
    o = _oracle(key)
    g = _solve(key, (("exact_degenerate", mode),))
    assert g.stats["pipeline"] == REVISED
    common = next((i for i, (u, v) in enumerate(zip(five(g.pivots), five(o.pivots))) if u != v), min(len(g.pivots), len(o.pivots)))
    print("deg m %d seed %d mode %d: common trace prefix %d of %d / %d, exact steps %d" % (
        m, seed, mode, common, len(g.pivots), len(o.pivots), g.stats["cond_fallbacks"]))
    if mode == 3:
        _check(g, o, "deg m %d seed %d strict" % (m, seed))
        assert g.stats["cond_fallbacks"] >= g.stats["pivots_phase1"] + g.stats["pivots_phase2"]
        return
    if o.status == O.ERR_CONDITION:
        assert g.status in (lp.OK, lp.ERR_CONDITION), lp.STATUS_NAMES.get(g.status)
        if g.status == lp.OK:
            _feasible_and_dual_feasible(g, _problem(key))
        return
    if (m, seed, mode) in TIE_MISSED:
        assert common == TIE_MISSED[(m, seed, mode)]
        if o.truncated:
            # off the path of a reference that cycles: the budget, an optimum, or a basis that is singular (mat.Condition, the status
            # the reference gives one) — the condition guard of general starts beyond 64 rows is the exact steps' alone
            assert g.status in (lp.ERR_UNSUPPORTED, lp.OK, lp.ERR_CONDITION), lp.STATUS_NAMES.get(g.status)
            if g.status == lp.OK:
                _feasible_and_dual_feasible(g, _problem(key))
            return
    _check(g, o, "deg m %d seed %d mode %d" % (m, seed, mode), (m, seed, mode) not in TIE_MISSED, _problem(key))


@pytest.mark.parametrize("rows", [600, 1000])
def test_eq_fixtures_on_the_revised_route(rows):
    """The committed EQ fixtures (tools/gen_golden.py eqlp: the reference's own column search and pivot loop) with tableau = 0: the
    guarded three-kernel loop, the fixture's trace, pivots per phase, basis, x and z bits."""
    sys.path.insert(0, os.path.join(HERE, "..", "tools"))
    from gen_golden import eqlp_problem
    fx = np.load(os.path.join(HERE, "golden", "lp_EQ%d.npz" % rows), allow_pickle=False)
    c0, A0, b0 = eqlp_problem(int(fx["seed"]), int(fx["n"]), int(fx["m"]))
    cx = lp.Context(tableau=0)
    try:
        g = cx.upload(c0, A0, b0).solve(0.0, trace=True)
    finally:
        cx.close()
    assert g.stats["pipeline"] == REVISED
    assert g.status == int(fx["status"]) == lp.OK
    assert (g.stats["pivots_phase1"], g.stats["pivots_phase2"]) == (int(fx["pivots_phase1"]), int(fx["pivots_phase2"]))
    tr = np.array(five(g.pivots), dtype=np.int64).reshape(-1, 5)
    want = fx["trace"][:, [0, 2, 3, 4, 5]]
    assert tr.shape == want.shape and np.array_equal(tr, want), "first differing pivot %d" % int(np.argmax((tr != want).any(axis=1)))
    assert np.array_equal(g.basis, fx["basis"].astype(np.int64))
    assert g.z == float(fx["z"]) and np.array_equal(g.x, fx["x"])


@pytest.mark.parametrize("name", sorted(WIDE))
def test_chunked_staging_is_bit_identical(name):
    """row_chunk = 512: the chunked forms of the guard instances decide from the same values as the one-pass forms."""
    key = WIDE[name]
    g1 = _solve(key)
    g2 = _solve(key, (("row_chunk", 512),))
    assert g2.stats["pipeline"] == REVISED and g2.status == g1.status
    assert five(g2.pivots) == five(g1.pivots)
    assert np.array_equal(g2.x, g1.x) and g2.z == g1.z


ROOT = ("eqlp", 1, 8232, 40, 24)


def _children():
    c, A, b = _problem(ROOT)
    o = _oracle(ROOT)
    assert o.status == O.OK
    integ = [j < 8232 and j % 4 == 0 for j in range(A.shape[1])]
    return synth.frontier_children(o.x, integ, nvars=3)


def test_pool_root_and_children():
    """A FrontierPool on the n - m = 8192 root: solve_root equals the single-context solve; a wave of 8 children (their standard
    forms keep n - m = 8192) runs on the pool's workers, each against the oracle on O.child_standard_form: status, z and x bits."""
    c, A, b = _problem(ROOT)
    o = _oracle(ROOT)
    kids = _children()
    assert len(kids) == 8
    pool = lp.FrontierPool(workers=4)
    try:
        pool.set_root(c, A, b)
        r = pool.solve_root(0.0)
        assert r.status == o.status and r.z == o.z and np.array_equal(r.x, o.x)
        res = pool.solve(kids)
    finally:
        pool.close()
    n0 = A.shape[1]
    for i, ch in enumerate(kids):
        oc = O.simplex(*O.child_standard_form(c, A, b, ch), 0.0, None, fast_initial_basis=True)
        assert res.status[i] == oc.status, (i, res.status[i], oc.status)
        if oc.x is None:
            continue
        assert res.has_x[i] and res.z[i] == oc.z, (i, res.z[i], oc.z)
        assert np.array_equal(res.x[i, :n0], oc.x[:n0]), i


def test_warm_child_of_a_general_start_parent_runs_cold():
    """A general-start parent kept with keep = True holds no B^-1: its child's warm solve falls back (fallback 5) to the cold solve,
    bit for bit."""
    c, A, b = _problem(ROOT)
    ch = _children()[0]
    cx = lp.Context()
    try:
        root = cx.upload(c, A, b)
        pr = root.solve(0.0, parent=None, keep=True)
        assert pr.status == lp.OK and pr.stats["pipeline"] == REVISED
        kid = root.child(ch)
        w = kid.solve(0.0, parent=root)
        assert w.stats["warm"]["fallback"] == 5
        cold = kid.solve(0.0)
    finally:
        cx.close()
    assert w.status == cold.status and w.z == cold.z and np.array_equal(w.x, cold.x)
