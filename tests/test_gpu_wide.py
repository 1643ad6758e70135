"""Wide relaxations (n - m >= 2m, slack-basis start) against the live oracle: the family synth.wide_degenerate_lp — integer data,
duplicated rows, ties in the ratio test, Bland steps, instances on which the reference's rule cycles.  A slack-basis wide LP takes the
revised-simplex pipelines (fused / three-kernel, running B^-1, host-driven Bland branch) unless the exact-step guard of
exact_degenerate is on for its size: then the tableau pipelines, whose exact steps decide degenerate pivots on fresh gonum-order solves
(DESIGN.md §2, §3).  Every case: status, the five trace fields of every pivot, pivots per phase, the positional final basis, x and z bits."""
import functools
import math

import numpy as np
import pytest

from gomilp_amd import lp, synth
from oracle import oracle as O

pytestmark = pytest.mark.gpu

BUDGET = 400      # pivot budget of the cycling instances (the reference's lp.Simplex has no iteration limit)
TAB = ("blocked", "tableau")
KNOBS = {"default": {}, "fused": dict(tableau=0, fused=1), "three-kernel": dict(tableau=0, fused=0), "strict-2": dict(exact_degenerate=2)}


def fused_supported(m):
    """fused_kernels.hip fused_supported(ld), ld = (m + 1) & ~1"""
    ld = (m + 1) & ~1
    return ld % 128 == 0 and ld // 128 in (1, 2, 4, 8, 16, 32)


def guard_on(m, mode=1):
    """the exact-step guard of engine_tableau.cpp make_bt_args for a slack-basis start of integer data"""
    return mode in (2, 3) or (mode == 1 and m <= 256)


def expected_pipeline(knobs, m):
    if knobs.get("tableau", 1) and guard_on(m, knobs.get("exact_degenerate", 1)):
        return TAB
    return ("fused",) if knobs.get("fused", 1) and fused_supported(m) else ("three-kernel",)


def five(tr):
    return [(p[0], p[2], p[3], p[4], p[5]) for p in tr]   # phase, minIdx, replace, entering, leaving


@functools.lru_cache(maxsize=None)
def _oracle(key):
    c, A, b = _problem(key)
    O.set_threads(8)
    return O.simplex(c, A, b, 0.0, None, fast_initial_basis=True, trace=True, stop_after_pivots=BUDGET)


@functools.lru_cache(maxsize=None)
def _problem(key):
    kind = key[0]
    if kind == "root":
        _, m, ratio, seed = key
        return synth.wide_degenerate_lp(m, seed, ratio)
    if kind == "nv":
        _, m, nv, seed = key
        return synth.wide_degenerate_lp(m, seed, nv / m)
    if kind == "child":
        _, m, ratio, seed, cons = key
        return O.child_standard_form(*synth.wide_degenerate_lp(m, seed, ratio), list(cons))
    raise KeyError(key)


def _check(g, o, label, guarded=True, problem=None):
    """g: engine result (trace on), o: oracle result with stop_after_pivots = BUDGET.  guarded: the exact-step guard was on — the
    reference's path bit for bit.  Unguarded (exact_degenerate = 0, tableau = 0 forced, default knobs beyond 256 rows): the revised
    pipelines decide ties and replaceBland's candidates on their running B^-1, without the kappa_1 test of simplex.go:377 — the same
    documented deviation as on the tableau side: same status and optimal value to 1e-9, a feasible point."""
    print("%s: status %s / %s, pivots %d + %d / %d + %d, bland steps engine %d oracle %d, pipeline %s%s" % (
        label, lp.STATUS_NAMES.get(g.status, g.status), O.STATUS_NAMES.get(o.status, o.status), g.stats["pivots_phase1"],
        g.stats["pivots_phase2"], o.pivots_phase1, o.pivots_phase2, g.stats["bland_steps"], o.bland_steps, g.stats["pipeline"],
        "" if guarded else " (unguarded)"))
    if not guarded:
        if o.truncated:
            # the reference never ends; the unguarded engine walks the budget too, or (another path) ends at an optimum — checked here
            # on its own terms: a feasible point whose basis is dual feasible in a plain float64 solve
            assert g.status in (lp.ERR_UNSUPPORTED, lp.OK), lp.STATUS_NAMES.get(g.status)
            if g.status == lp.ERR_UNSUPPORTED:
                assert g.stats["pivots_phase2"] == o.pivots_phase2
            else:
                c, A, b = problem
                assert g.x.min() >= -1e-9 and np.abs(A @ g.x - b).max() <= 1e-9 * max(1.0, np.abs(b).max())
                y = np.linalg.solve(A[:, g.basis].T, c[g.basis])
                assert (c - A.T @ y).min() >= -1e-9
            return
        assert g.status == o.status, (lp.STATUS_NAMES.get(g.status), O.STATUS_NAMES.get(o.status))
        if o.x is not None:
            c, A, b = problem
            assert abs(g.z - o.z) <= 1e-9 * max(1.0, abs(o.z)), (g.z, o.z)
            assert g.x.min() >= -1e-9 and np.abs(A @ g.x - b).max() <= 1e-9 * max(1.0, np.abs(b).max())
        return
    if o.truncated:   # the reference's rule cycles: the engine must walk the same cycle until the budget ends it
        assert g.status == lp.ERR_UNSUPPORTED and len(g.pivots) == len(o.pivots), (g.status, len(g.pivots))   # (the budget counts Phase-II pivots)
        assert five(g.pivots) == five(o.pivots), "pivot sequence differs"
        return
    assert g.status == o.status, (lp.STATUS_NAMES.get(g.status), O.STATUS_NAMES.get(o.status))
    if o.status in (O.OK, O.ERR_BLAND):
        assert five(g.pivots) == five(o.pivots), "first differing pivot %d" % next(
            (i for i, (a, b) in enumerate(zip(five(g.pivots), five(o.pivots))) if a != b), min(len(g.pivots), len(o.pivots)))
        assert (g.stats["pivots_phase1"], g.stats["pivots_phase2"]) == (o.pivots_phase1, o.pivots_phase2)
    if o.x is None:
        assert g.x is None
        assert (math.isnan(g.z) and math.isnan(o.z)) or g.z == o.z
        return
    assert np.array_equal(g.basis, o.basis), "positional final basis"
    assert np.array_equal(g.x, o.x), float(np.max(np.abs(g.x - o.x)))
    assert g.z == o.z


def _solve(key, knobs, child=None):
    """key: the problem (a root when `child` is given: the child is assembled on the device)"""
    c, A, b = _problem(key)
    cx = lp.Context(max_pivots=BUDGET, **knobs)
    try:
        root = cx.upload(c, A, b)
        return (root.child(list(child)) if child else root).solve(0.0, trace=True)
    finally:
        cx.close()


# guarded cases that leave the reference's path (a tie the 1e-9 guard does not see); every other guarded case is asserted bit for bit
TIE_MISSED = {(256, 2.5, 0, "default"), (256, 2.5, 0, "strict-2"), (257, 4, 0, "strict-2"), (257, 4, 1, "strict-2"),
              (300, 2.5, 0, "strict-2"), (300, 4, 0, "strict-2"), (300, 4, 1, "strict-2")}
ROOTS = [(m, ratio, seed) for m in (8, 24, 48, 64, 65, 96, 128, 200, 256, 257, 300) for ratio in (2, 2.5, 4) for seed in (0, 1)]


@pytest.mark.parametrize("pipe", list(KNOBS))
@pytest.mark.parametrize("m,ratio,seed", ROOTS)
def test_wide_degenerate_root_matches_oracle(m, ratio, seed, pipe):
    """Roots of the family on every pipeline a wide LP can take: default knobs, fused forced (where fused_supported(ld)), three-kernel
    forced, exact_degenerate = 2 (the tableau with its exact steps at every size).  64 / 65 rows: the edge of the host replay of the
    condition guards; 256 / 257: the edge of exact_degenerate = 1.  Bit for bit on the guarded pipelines, except the cases of TIE_MISSED:
    there, from 256 rows on, the tableau's exact steps (guard 1e-9 on the winning ratio) do not catch every tie the reference's rounding
    decides (256 x 896 seed 0 leaves the reference's path at pivot 47) — held, like the unguarded cases, to the documented deviation of
    DESIGN.md §3: status, z to 1e-9, a feasible point."""
    key = ("root", m, ratio, seed)
    o = _oracle(key)
    g = _solve(key, KNOBS[pipe])
    want = expected_pipeline(KNOBS[pipe], m)
    assert g.stats["pipeline"] in want, g.stats["pipeline"]
    _check(g, o, "m %d ratio %g seed %d %s" % (m, ratio, seed, pipe), want == TAB and (m, ratio, seed, pipe) not in TIE_MISSED, _problem(key))


CYCLING = [(24, 4, 5), (32, 2.5, 11), (48, 2.5, 3), (48, 4, 4)]


@pytest.mark.parametrize("pipe", ["default", "strict-2"])
@pytest.mark.parametrize("m,ratio,seed", CYCLING)
def test_wide_instances_on_which_the_reference_cycles(m, ratio, seed, pipe):
    """The reference's rule does not terminate on these (oracle truncated at the budget): with max_pivots = budget the engine stops with
    ERR_UNSUPPORTED after exactly that many pivots, its trace equal to the oracle's pivot by pivot (the guarded pipelines: the cycle is
    made of rounding-size steps of the reference's fresh solves)."""
    key = ("root", m, ratio, seed)
    o = _oracle(key)
    assert o.truncated and len(o.pivots) == BUDGET
    g = _solve(key, KNOBS[pipe])
    _check(g, o, "cycling m %d ratio %g seed %d %s" % (m, ratio, seed, pipe))


@pytest.mark.parametrize("m", [96, 200])
@pytest.mark.parametrize("dnv", [-1, 0, 1])
def test_routing_edge(m, dnv):
    """nv = 2m - 1 / 2m / 2m + 1 structural columns: n - m < 2m takes the tableau; from 2m on a slack-basis start takes the revised
    pipelines, unless the exact-step guard is on for its size (default knobs up to 256 rows).  All three match the oracle either way."""
    nv = 2 * m + dnv
    key = ("nv", m, nv, 0)
    o = _oracle(key)
    for knobs in ({}, dict(exact_degenerate=0)):
        g = _solve(key, knobs)
        want = TAB if (dnv < 0 or guard_on(m, knobs.get("exact_degenerate", 1))) else ("fused",) if fused_supported(m) else ("three-kernel",)
        assert g.stats["pipeline"] in want, (knobs, g.stats["pipeline"])
        _check(g, o, "m %d nv %d %s" % (m, nv, knobs), guard_on(m, knobs.get("exact_degenerate", 1)), _problem(key))


@pytest.mark.parametrize("m,seed", [(512, 0), (514, 1)])
def test_default_pipeline_where_fused_support_flips(m, seed):
    """Above 256 rows the default knobs take the revised pipelines: fused where fused_supported(ld) holds (ld = 512), three-kernel one
    row-pair further (ld = 514).  (Seeds on which the reference ends OK: on 511 / 513 / 514-seed-0 it stops with mat.Condition.)"""
    key = ("root", m, 2, seed)
    o = _oracle(key)
    g = _solve(key, {})
    assert g.stats["pipeline"] == ("fused" if fused_supported(m) else "three-kernel")
    _check(g, o, "m %d default" % m, False, _problem(key))


def _branch_var(m, ratio, seed):
    """the structural variable with the largest value at the oracle's root optimum"""
    o = _oracle(("root", m, ratio, seed))
    assert o.status == O.OK
    nv = int(ratio * m)
    j = int(np.argmax(o.x[:nv]))
    assert o.x[j] > 0
    return j, float(o.x[j])


CHILD_ROOTS = [(64, 2.5, 0), (126, 2.5, 0), (200, 2.5, 0)]


def _children(m, ratio, seed):
    j, v = _branch_var(m, ratio, seed)
    up = (j, 1, float(math.floor(v / 2)))          # x_j <= floor(v / 2): the root optimum cut off, slack start feasible
    lo = (j, -1, -float(math.floor(v) + 1))        # x_j >= floor(v) + 1: negative right-hand side, Phase I with the artificial column
    return {"stacked1": (up,), "stacked2": (up,) * 2, "stacked4": (up,) * 4, "phase1": (lo,), "phase1x2": (lo, lo),
            "infeasible": ((0, -1, -50.0),)}       # x_0 >= 50 against row 0 (entries >= 1, right-hand side <= 8)


@pytest.mark.parametrize("pipe", list(KNOBS))
@pytest.mark.parametrize("m,ratio,seed", CHILD_ROOTS)
def test_children_of_wide_roots(m, ratio, seed, pipe):
    """Children built like subproblem.go:141-159: stacked identical branch rows (the maxFunBranchPoint habit of branching on the same
    variable again, branching.go:54-72) — 1, 2 and 4 copies of one (var, sign, value); infeasible-start children (Phase I, artificial
    column); an infeasible child.  Assembled on the device (upload(...).child(...)) on every pipeline."""
    fused_ok = []
    for name, cons in _children(m, ratio, seed).items():
        key = ("child", m, ratio, seed, cons)
        o = _oracle(key)
        g = _solve(("root", m, ratio, seed), KNOBS[pipe], child=cons)
        mm = m + len(cons)
        want = expected_pipeline(KNOBS[pipe], mm)
        assert g.stats["pipeline"] in want or o.x is None and g.x is None, g.stats["pipeline"]
        fused_ok.append(g.stats["pipeline"] == "fused")
        _check(g, o, "child %s of m %d ratio %g seed %d %s" % (name, m, ratio, seed, pipe), want == TAB, _problem(key))
        if name == "infeasible":
            assert g.status == lp.ERR_INFEASIBLE
    if pipe == "fused" and m == 126:
        assert any(fused_ok)   # (126 + 2 rows: ld = 128, the fused pipeline on a child)


@pytest.mark.parametrize("m,ratio,seed", CHILD_ROOTS)
def test_children_of_wide_roots_through_the_flat_call(m, ratio, seed):
    """The same children through the lp.Simplex drop-in (gomilp_lp_simplex: host buffers in / out, default knobs)."""
    for name, cons in _children(m, ratio, seed).items():
        key = ("child", m, ratio, seed, cons)
        o = _oracle(key)
        if o.truncated:
            continue   # (the flat call has no pivot budget, like the reference; the cycle is covered above with max_pivots)
        g = lp.simplex(*_problem(key), 0.0, None)
        assert g.status == o.status, (name, g.status, o.status)
        assert (g.x is None) == (o.x is None)
        if o.x is not None:
            assert np.array_equal(g.basis, o.basis) and np.array_equal(g.x, o.x) and g.z == o.z, name
            assert (g.stats["pivots_phase1"], g.stats["pivots_phase2"]) == (o.pivots_phase1, o.pivots_phase2), name


@pytest.mark.parametrize("pipe", list(KNOBS))
@pytest.mark.parametrize("cost", [-10.0, -0.5])
def test_unbounded_wide_lp(pipe, cost):
    """A column with a negative cost and no positive entry: computeMove finds every ratio +Inf, lp.ErrUnbounded (simplex.go:328) —
    entering at once (cost -10) or after other pivots (cost -0.5)."""
    c, A, b = synth.wide_degenerate_lp(64, 0, 2.5)
    m = A.shape[0]
    col = -(np.arange(m) % 3).astype(float)               # entries 0, -1, -2: not a zero column (that is verifyInputs' ErrUnbounded)
    A = np.hstack([A[:, :160], col[:, None], A[:, 160:]])
    c = np.concatenate([c[:160], [cost], c[160:]])
    o = O.simplex(c, A, b, 0.0, None, fast_initial_basis=True, trace=True, stop_after_pivots=BUDGET)
    assert o.status == O.ERR_UNBOUNDED
    cx = lp.Context(**KNOBS[pipe])
    try:
        g = cx.upload(c, A, b).solve(0.0, trace=True)
    finally:
        cx.close()
    assert g.status == lp.ERR_UNBOUNDED and g.z == -math.inf and g.x is None
    if g.pivots:
        assert five(g.pivots) == five(o.pivots)
    g = lp.simplex(c, A, b, 0.0, None)
    assert g.status == lp.ERR_UNBOUNDED and g.z == -math.inf


@pytest.mark.parametrize("m,ratio,seed", [(64, 4, 0), (200, 2.5, 2)])
def test_exact_degenerate_modes_on_a_wide_root(m, ratio, seed):
    """exact_degenerate 0 / 1 / 2 / 3 on a degenerate wide root.  Modes 1 / 2 / 3 follow the reference bit for bit (on the tableau
    pipelines: the guard needs their exact steps); mode 0 — no exact steps — ends at the reference's vertex value.  Mode 3 decides EVERY
    pivot and the stop test in an exact step: stats cond_fallbacks counts one per step — up to 64 rows it also counts the host replay of
    the condition guards, so there the count is taken once more with cond_guard = 0, where it is the exact steps alone.  Only the block
    kernels of the blocked tableau stop for exact steps: where that pipeline does not run (tableau = 0 or blocked = 0 forced, on this wide
    root and on a narrow one), mode 3 refuses — ERR_UNSUPPORTED, never a silent default-mode solve."""
    key = ("root", m, ratio, seed)
    o = _oracle(key)
    assert o.status == O.OK and o.bland_steps > 0
    for mode in (0, 1, 2, 3):
        g = _solve(key, dict(exact_degenerate=mode))
        if mode == 0:
            print("mode 0: status %d, pivots %d / %d, z %.17g / %.17g" % (g.status, g.stats["pivots_phase2"], o.pivots_phase2, g.z, o.z))
            assert g.status == lp.OK and abs(g.z - o.z) <= 1e-9 * max(1.0, abs(o.z))
            continue
        assert g.stats["pipeline"] in TAB
        _check(g, o, "mode %d m %d" % (mode, m))
        if mode == 3:
            pivots = g.stats["pivots_phase1"] + g.stats["pivots_phase2"]
            if m <= 64:
                assert g.stats["cond_fallbacks"] >= 2 * pivots + 1   # exact steps + about one replay evaluation per pivot
                g = _solve(key, dict(exact_degenerate=3, cond_guard=0))
                _check(g, o, "mode 3 cond_guard 0 m %d" % m)
            print("mode 3: %d exact steps for %d pivots" % (g.stats["cond_fallbacks"], pivots))
            assert g.stats["cond_fallbacks"] == pivots + 1 > 1     # every pivot and the stop test
    narrow = ("nv", m, 2 * m - 1, seed)
    for k, knobs in ((key, dict(tableau=0)), (key, dict(blocked=0)), (narrow, dict(blocked=0)), (narrow, dict(tableau=0))):
        g = _solve(k, dict(exact_degenerate=3, **knobs))
        assert g.status == lp.ERR_UNSUPPORTED and g.x is None, (k, knobs, g.status)
