"""The starts and exits of equality-form wide waves that tests/test_gpu_wide_general_frontier.py does not reach (pool knob rev_general,
DESIGN.md section 2.5e "Equality-form roots"; k_rv_gen_start, k_rv_gen_art and the G = true instances of K1-K3 in batch_revised.hip):
  (A) branches on variables that are BASIC in the root's searched basis — the `pos >= 0` arm of k_rv_gen_start, B^-1 row
      -sign * B0^-1[pos, :] and x_B entry rhs - sign * x_B0[pos] — which WavePlan's branch-variable rule (var < n - m) leaves reachable
      only where the column search skipped a dependent column and took one below n - m: the roots PD and FD;
  (B) children that Phase I finds infeasible, (E) the unbounded exit of the guarded FTRAN;
  (C) waves that hold K = 0 .. 4 together (odd and even K: with and without the padded row of ld = (m + 1) & ~1), in both slot orders;
  (D) all of these read in place; (F) mixed with a slack root; (G) the pivot budget spent in Phase I and in Phase II.
Per relaxation against the live oracle (status, z and x bits) and against the worker path of the same pool (rev_general = 0: the same
bits and the wave's pivot / Phase-I totals).  No tolerance: the route promises bits.

The schedule hands a relaxation to a worker where its start is within 1e-9 of a decision (k_rv_gen_start).  start_model below is that
guard in numpy on the oracle's x_B0 (the engine's host column search returns the same basis list, lp.find_independent): no chosen child
trips it, so a hand-over in these waves comes from the loop guard (ST_NEED_EXACT).

What the classes were seen to catch, on a copy of the tree with k_rv_gen_start changed: with `s = +d->asign[kk]` (the sign of the copied
B^-1 row) both cases of (A), (B) on PD, (C) on FD and their in-place cases fail — (235, 1, 1.0) on FD ends at the unconstrained optimum,
(235, 1, -72.0) on PD ends OK instead of infeasible — and on FD the x_j <= 0 children, whose start x_B is the same, are no longer handed over
(8 of 8 stay): it is the loop guard that hands them over, not the start guard.  With `kk = i` in the B^-1 row branch the K = 1 waves of (A) pass and the first K = 2 wave
on a feasible-start root ((B) on F) never returns: a wave with a wrong B^-1 has no pivot limit at max_pivots = 0.

Not covered: the zero-level exchange (RR_EXCH) of a searched start.  The oracle exchanges an artificial in three (j, 1, 0.0) children
of (A); on the schedule those children stop at a degenerate step and a worker solves them, so art_exchanges is 0 on both paths.
In (C) on P the K = 3 and K = 4 children are handed over too; on F and FD all five run on the schedule."""
import functools
import math

import numpy as np
import pytest

from gomilp_amd import lp, synth
from oracle import oracle as O
from tests.test_gpu_wide_general import eqlp
from tests.test_gpu_wide_general_frontier import _assert_same_bits, _report, bits, branches

pytestmark = pytest.mark.gpu

WORKERS = 4
N, E, I = 260, 24, 56          # 80 x 316
NB = N + I - (E + I)           # n - m = 236: WavePlan takes branch variables below it only


def eqlp_dep(seed, on_basis):
    """eqlp(seed, N, E, I) with two dependent columns among the last E structural ones (column N - 1 = 2 * column N - 2, column N - 5 =
    column N - 6, over the stacked equality and inequality rows) before b and h are computed: the descending column search skips two
    and takes N - 25 and N - 26, both below n - m.  on_basis: x0 has its support on the structural columns of that searched basis
    (|N(0,1)| + 0.1), so the searched basis is feasible."""
    rng = np.random.default_rng(seed)
    x0 = np.abs(rng.standard_normal(N))
    A = rng.standard_normal((E, N))
    G = rng.standard_normal((I, N))
    for M in (A, G):
        M[:, N - 1] = 2.0 * M[:, N - 2]
        M[:, N - 5] = M[:, N - 6]
    if on_basis:
        full = O.convert_to_equalities(np.zeros(N), A, np.zeros(E), G, np.zeros(I))[1]
        keep = [j for j in O.find_linearly_independent(full, fast=True) if j < N]
        x1 = np.zeros(N)
        x1[keep] = x0[keep] + 0.1
        x0 = x1
    b = A @ x0
    h = G @ x0 + np.abs(rng.standard_normal(I))
    c = np.abs(rng.standard_normal(N))
    return O.convert_to_equalities(c, A, b, G, h)


def unbounded(name, ncost):
    c, A, b = _root(name)
    c = c.copy()
    c[:ncost] = -np.abs(c[:ncost]) - 1.0
    return c, A, b


ROOTS = {
    "P": lambda: eqlp(1, N, E, I, False),      # the searched basis is infeasible: every child needs Phase I
    "F": lambda: eqlp(2, N, E, I, True),       # the searched basis is feasible
    "PD": lambda: eqlp_dep(1, False),          # P's recipe with the dependent columns
    "FD": lambda: eqlp_dep(2, True),           # dependent columns, the searched basis feasible: Phase II at once from a sign-flipped row
    "UF": lambda: unbounded("F", 4),           # ERR_UNBOUNDED in Phase II, no Phase I
    "UP": lambda: unbounded("P", 1),           # ERR_UNBOUNDED behind a device Phase I
    "slack260": lambda: synth.dense_lp_standard_form(260, 1, 780),   # 260 x 1040, slack basis: the unguarded batched schedule
}
BASE = {"UF": "F", "UP": "P"}


@functools.lru_cache(maxsize=None)
def _root(name):
    return ROOTS[name]()


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


# ------------------------------------------------------------------------------------------------
# the CPU side: searched basis, optimum, oracle per child, the start guard
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _start(name):
    """(searched basis by position, x of that basis scattered over the columns)"""
    c, A, b = _root(BASE.get(name, name))
    basis = O.find_linearly_independent(A, fast=True)
    assert len(basis) == A.shape[0]
    s = O.basis_solve(c, A, b, basis)
    assert s.status == O.OK
    return tuple(basis), s.x


def _low_basic(name):
    """the searched-basis columns a wave may branch on"""
    return [j for j in _start(name)[0] if j < NB]


@functools.lru_cache(maxsize=None)
def _opt(name):
    """(x of the oracle optimum, nz: branchable structural variables that are nonzero at it, zs: those that are zero)"""
    O.set_threads(8)
    o = O.simplex(*_root(BASE.get(name, name)), 0.0, None, fast_initial_basis=True)
    assert o.status == O.OK
    free = range(4, NB) if name in BASE else range(NB)   # (not the columns whose cost makes a U root unbounded)
    return o.x, [j for j in free if o.x[j] != 0], [j for j in free if o.x[j] == 0]


@functools.lru_cache(maxsize=None)
def _oracle(name, child):
    c, A, b = _root(name)
    O.set_threads(8)
    return O.simplex(*O.child_standard_form(c, A, b, list(child)), 0.0, None, fast_initial_basis=True)


def start_model(name, child):
    """k_rv_gen_start's decisions on the oracle's numbers: (handed over, starts infeasible)"""
    basis, x0 = _start(name)
    v = np.array([rhs - sign * x0[var] for var, sign, rhs in reversed(child)] + [x0[j] for j in basis])
    s = np.sort(v)
    close = bool((np.abs(v + 1e-13) <= 1e-9).any())
    tie = s[1] - s[0] <= 1e-9 * max(1.0, abs(s[0]))
    return close or bool(tie), bool((v < -1e-13).any())


def _kids(*children):
    return tuple(tuple((int(j), int(s), float(r)) for j, s, r in ch) for ch in children)


def down(name, j):
    return (j, 1, float(math.floor(_opt(name)[0][j])))


def up(name, j):
    return (j, -1, -float(math.ceil(_opt(name)[0][j])))


def _first(name, options, what):
    """the first of `options` (children) that the start guard lets through"""
    for ch in options:
        if not start_model(name, ch)[0]:
            return ch
    raise AssertionError("%s: every %s child meets the start guard" % (name, what))


# ------------------------------------------------------------------------------------------------
# the waves, one per class and root: (roots of the pool, children, root index per child)
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def wave_a(name):
    """(A) per searched-basis column j < n - m: x_j <= ceil x0_j, x_j <= floor x0_j, x_j >= ceil x0_j, x_j <= 0"""
    x0 = _start(name)[1]
    out = []
    for j in _low_basic(name):
        out += [[(j, 1, math.ceil(x0[j]))], [(j, 1, math.floor(x0[j]))], [(j, -1, -math.ceil(x0[j]))], [(j, 1, 0.0)]]
    return _kids(*out)


@functools.lru_cache(maxsize=None)
def wave_b(name):
    """(B) x_j <= f and x_j >= f + 1, f = floor x*_j, on four variables that are nonzero at the optimum (and the basic ones of PD);
    a nonbasic variable with f = 0 would start at x_B = 0, within the start guard: the first four that it lets through"""
    x = _opt(name)[0]
    pair = lambda j: _kids([(j, 1, math.floor(x[j])), (j, -1, -(math.floor(x[j]) + 1.0))])[0]
    low = _low_basic(name) if name == "PD" else []
    picks = [pair(j) for j in _opt(name)[1] if j not in low and not start_model(name, pair(j))[0]][:4]
    assert len(picks) == 4
    return tuple(picks) + tuple(pair(j) for j in low)


@functools.lru_cache(maxsize=None)
def wave_c(name):
    """(C) K = 0, 1, 2, 3, 4 in one wave.  nz down branches need floor x*_j >= 1 on a variable that is nonbasic at the start (x_B = 0 is
    within the guard), and the two smallest entries of a start must differ: every stacked child is the first of its kind that the guard
    lets through.  On FD the K = 3 child has a searched-basis variable first."""
    x, nz, zs = _opt(name)
    big = [j for j in nz if x[j] >= 1.0]
    assert len(big) >= 2 and len(nz) >= 6 and len(zs) >= 3
    k1 = (zs[0], -1, -1.0)
    k2 = _first(name, [[down(name, a), up(name, b)] for a in big for b in nz if a != b], "K = 2")
    lead = [(j, 1, float(math.ceil(_start(name)[1][j]))) for j in _low_basic(name)] if name == "FD" else [down(name, a) for a in big]
    k3 = _first(name, [[ld, up(name, b), (zs[1], -1, -2.0)] for ld in lead for b in nz if b != ld[0] and b != k2[1][0]], "K = 3")
    k4 = _first(name, [[up(name, b), (zs[2], -1, -1.0), down(name, a), (zs[1], -1, -2.0)] for a in big[::-1] for b in nz[::-1] if a != b], "K = 4")
    return _kids([], [k1], k2, k3, k4)


@functools.lru_cache(maxsize=None)
def wave_e():
    """(E) K = 0 of both unbounded roots, two up branches on variables that are zero at the base root's optimum of each, two children of P"""
    kids, rof = [], []
    for r, nm in ((1, "UF"), (2, "UP")):
        zs = _opt(nm)[2]
        kids += [[], [(zs[0], -1, -1.0)], [(zs[1], -1, -2.0)]]
        rof += [r] * 3
    p = _p_children()   # (a down branch to 0 on a nonbasic variable starts at x_B = 0, within the guard: the first of each half that is not)
    return ("P", "UF", "UP"), _kids(*kids) + (_first("P", p[:12], "down"), _first("P", p[12:], "up")), tuple(rof) + (0, 0)


@functools.lru_cache(maxsize=None)
def wave_f():
    """(F) K = 0 .. 2 of P, of FD and of the slack root in one wave"""
    names = ("P", "FD", "slack260")
    kids = wave_c("P")[:3] + wave_c("FD")[:3] + _kids([], [(0, 1, 1.0)], [(0, -1, -1.0), (1, 1, 2.0)])
    return names, kids, (0, 0, 0, 1, 1, 1, 2, 2, 2)


@functools.lru_cache(maxsize=None)
def _p_children():
    """the 24 children of the existing file's 'phase1' root: 12 down, then 12 up branches"""
    return _kids(*branches(_opt("P")[0], N, 12))


SINGLE = {"A": wave_a, "B": wave_b, "C": wave_c}
CASES = [("A", "PD"), ("A", "FD"), ("B", "P"), ("B", "F"), ("B", "PD"), ("C", "P"), ("C", "F"), ("C", "FD")]


def _wave(cls, name):
    kids = SINGLE[cls](name)
    return (name,), kids, (0,) * len(kids)


@functools.lru_cache(maxsize=None)
def _run(names, kids, rof, rev_general=1, rev_inplace=0, max_pivots=0):
    r = _pool(names, rev_general=rev_general, rev_inplace=rev_inplace, max_pivots=max_pivots).solve([list(ch) for ch in kids], roots=list(rof))
    _report("%s, K %s, rev_general = %d, rev_inplace = %d, max_pivots = %d" % (
        "+".join(names), "".join(str(len(ch)) for ch in kids), rev_general, rev_inplace, max_pivots), r)
    return r


# ------------------------------------------------------------------------------------------------
# the bar
# ------------------------------------------------------------------------------------------------
def _assert_oracle(r, names, kids, rof):
    """per relaxation the oracle's status, z bits and x bits; returns the oracle's results"""
    out = []
    for i, (ch, ri) in enumerate(zip(kids, rof)):
        oc = _oracle(names[ri], ch)
        out.append(oc)
        assert r.status[i] == oc.status, (i, ch, r.status[i], oc.status)
        if oc.status == O.ERR_UNBOUNDED:
            assert r.z[i] == -math.inf, (i, r.z[i])
        if oc.x is None:
            assert not r.has_x[i], i
            continue
        n0 = _root(names[ri])[1].shape[1]
        assert r.has_x[i] and bits(r.z[i]) == bits(oc.z), (i, ch, r.z[i], oc.z)
        assert np.array_equal(bits(r.x[i, :n0]), bits(oc.x[:n0])), (i, ch)
    return out


def _assert_route(r, w, tag):
    """every relaxation ran on the schedule or was handed over by it, at least one ran; the worker path batches none"""
    s, count = r.stats, len(r.status)
    print("%s: share handed over %d / %d" % (tag, s["host_fallbacks"], count))
    assert s["batched_relaxations"] + s["host_fallbacks"] == count, (s["batched_relaxations"], s["host_fallbacks"], count)
    assert s["batched_relaxations"] >= 1 and s["supersteps"] > 0
    assert w.stats["batched_relaxations"] == 0


def _assert_start_guard(names, kids, rof):
    """no child of the wave is handed over by the start guard; returns per child whether it starts infeasible"""
    out = []
    for ch, ri in zip(kids, rof):
        if names[ri] == "slack260":
            continue
        handed, infeasible = start_model(names[ri], ch)
        assert not handed, (names[ri], ch)
        out.append(infeasible)
    return out


def _full_bar(names, kids, rof, tag):
    _assert_start_guard(names, kids, rof)
    r, w = _run(names, kids, rof, 1), _run(names, kids, rof, 0)
    oc = _assert_oracle(r, names, kids, rof)
    _assert_same_bits(w, r)
    _assert_route(r, w, tag)
    print("%s: oracle statuses %s, pivots %s, art_exchanges %d" % (
        tag, [o.status for o in oc], [(o.pivots_phase1, o.pivots_phase2) for o in oc], sum(o.art_exchanges for o in oc)))
    return r, w, oc


# ------------------------------------------------------------------------------------------------
# tests
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["PD", "FD"])
def test_dependent_roots_take_columns_below_the_slack_rule(name):
    """The roots of (A): 80 x 316, the searched basis holds at least two columns below n - m (the ones WavePlan lets a wave branch on),
    the root ends OK on the oracle; FD's searched basis is feasible with every entry far from the start guard."""
    c, A, b = _root(name)
    assert A.shape == (80, 316) and NB == A.shape[1] - A.shape[0]
    basis, x0 = _start(name)
    assert len(_low_basic(name)) >= 2, sorted(basis)[:4]
    _opt(name)
    if name == "FD":
        assert min(x0[j] for j in basis) >= 0.01, min(x0[j] for j in basis)
        assert start_model(name, ()) == (False, False)
    else:
        assert start_model(name, ()) == (False, True)
    for plain in ("P", "F"):
        assert _low_basic(plain) == []


@pytest.mark.parametrize("name", ["PD", "FD"])
def test_branches_on_basic_variables(name):
    """(A) K = 1 on the searched-basis columns below n - m: k_rv_gen_start copies -sign * B0^-1[pos, :] and starts from
    rhs - sign * x_B0[pos].  On FD the wave holds starts that are feasible (Phase II at once) and starts that need Phase I.
    (j, 1, 0.0) on a basic variable starts at -x0_j and ends Phase I with the artificial basic at level zero on the oracle; on the
    schedule it stops at a degenerate step first (the loop guard) and a worker solves it, so the two exchange counts compared here are
    both 0 and the device's RR_EXCH stays unrun on this route.  On FD floor x0_j = 0, so the second and the fourth child are equal."""
    names, kids, rof = _wave("A", name)
    assert len(kids) == 4 * len(_low_basic(name)) >= 8
    infeasible = _assert_start_guard(names, kids, rof)
    if name == "FD":
        assert any(infeasible) and not all(infeasible)
    r, w, oc = _full_bar(names, kids, rof, "(A) %s" % name)
    print("(A) %s: art_exchanges on the schedule %d, on the worker path %d" % (name, r.stats["art_exchanges"], w.stats["art_exchanges"]))
    assert sum(o.art_exchanges for o in oc) >= 1
    assert r.stats["art_exchanges"] == w.stats["art_exchanges"], (r.stats["art_exchanges"], w.stats["art_exchanges"])


@pytest.mark.parametrize("name", ["P", "F", "PD"])
def test_infeasible_children(name):
    """(B) x_j <= f and x_j >= f + 1: the device's Phase-I verdict |x_art| > 1e-12 against the oracle's ERR_INFEASIBLE."""
    names, kids, rof = _wave("B", name)
    r, w, oc = _full_bar(names, kids, rof, "(B) %s" % name)
    assert all(o.status == O.ERR_INFEASIBLE for o in oc), [o.status for o in oc]
    assert not r.has_x.any()


@pytest.mark.parametrize("name", ["P", "F", "FD"])
def test_stacked_and_mixed_depth(name):
    """(C) K = 0 .. 4 in one wave (the rows i >= m of the shorter relaxations leave k_rv_gen_start's grid; odd K has the padded row):
    the reversed order kk = K - 1 - pos of the branch slacks, the unit entry at m0 + kk, ChildCol over several branch rows.  The same
    children in reverse slot order give the same bits per relaxation."""
    names, kids, rof = _wave("C", name)
    assert [len(ch) for ch in kids] == [0, 1, 2, 3, 4]
    assert all(len({v for v, _, _ in ch}) == len(ch) for ch in kids)
    if name == "FD":
        low = set(_low_basic(name))
        assert any(0 < sum(v in low for v, _, _ in ch) < len(ch) for ch in kids)
    r, w, oc = _full_bar(names, kids, rof, "(C) %s" % name)
    back = _run(names, kids[::-1], rof, 1)
    for i in range(len(kids)):
        k = len(kids) - 1 - i
        assert r.status[i] == back.status[k] and r.has_x[i] == back.has_x[k], i
        assert bits(r.z[i]) == bits(back.z[k]) and np.array_equal(bits(r.x[i]), bits(back.x[k])), i


@pytest.mark.parametrize("cls,name", CASES)
def test_in_place(cls, name):
    """(D) rev_inplace = 1 on the waves of (A), (B), (C): the bits and the hand-overs of rev_inplace = 0."""
    names, kids, rof = _wave(cls, name)
    r, p = _run(names, kids, rof, 1), _run(names, kids, rof, 1, 1)
    _assert_oracle(p, names, kids, rof)
    _assert_same_bits(r, p)
    assert p.stats["batched_relaxations"] == r.stats["batched_relaxations"] and p.stats["host_fallbacks"] == r.stats["host_fallbacks"]


def test_unbounded():
    """(E) the ST_UNBOUNDED exit of the guarded FTRAN: without a Phase I (UF) and behind a device Phase I (UP), beside children of P,
    which keep the bits they have in a wave of their own."""
    names, kids, rof = wave_e()
    r, w, oc = _full_bar(names, kids, rof, "(E)")
    assert (rof[0], rof[3]) == (1, 2) and not kids[0] and not kids[3]
    assert oc[0].status == oc[3].status == O.ERR_UNBOUNDED
    alone = _run(names, kids[-2:], rof[-2:], 1)
    for i in (0, 1):
        k = len(kids) - 2 + i
        assert r.status[k] == alone.status[i] and r.has_x[k] == alone.has_x[i], i
        assert bits(r.z[k]) == bits(alone.z[i]) and np.array_equal(bits(r.x[k]), bits(alone.x[i])), i


def test_mixed_kinds_with_children():
    """(F) K = 0 .. 2 of P, FD and the 260-row slack root in one gomilp_frontier_solve_roots wave: each relaxation equals its result in
    a single-root wave bit for bit, the equality-form ones the oracle, the slack ones rev_general = 0."""
    names, kids, rof = wave_f()
    _assert_start_guard(names, kids, rof)
    r, w = _run(names, kids, rof, 1), _run(names, kids, rof, 0)
    _assert_oracle(r, names[:2], kids[:6], rof[:6])
    _assert_same_bits(w, r)
    _assert_route(r, w, "(F)")
    for root in range(3):
        idx = [i for i, ri in enumerate(rof) if ri == root]
        alone = _run(names, tuple(kids[i] for i in idx), (root,) * len(idx), 1)
        for k, i in enumerate(idx):
            assert r.status[i] == alone.status[k] and r.has_x[i] == alone.has_x[k], i
            assert bits(r.z[i]) == bits(alone.z[k]) and np.array_equal(bits(r.x[i]), bits(alone.x[k])), i


@pytest.mark.parametrize("budget", [40, 200])
def test_pivot_budget(budget):
    """(G) max_pivots on P's 24 children: 40 ends inside every Phase I (each takes more than 40 pivots on the oracle), 200 inside
    Phase II.  Against the worker path."""
    names, kids, rof = ("P",), _p_children(), (0,) * 24
    oc = [_oracle("P", ch) for ch in kids]
    assert all(o.status == O.OK and o.pivots_phase1 > 40 for o in oc)
    assert all(o.pivots_phase1 < 200 < o.pivots_phase1 + o.pivots_phase2 for o in oc), [(o.pivots_phase1, o.pivots_phase2) for o in oc]
    # (these children are the existing file's: a down branch to 0 starts at x_B = 0 and is handed over by the start guard)
    stay = [not start_model("P", ch)[0] for ch in kids]
    print("start guard: %d of 24 stay" % sum(stay))
    assert sum(stay) >= 12
    r, w = _run(names, kids, rof, 1, 0, budget), _run(names, kids, rof, 0, 0, budget)
    _pool(names)   # (max_pivots back to 0)
    _assert_same_bits(w, r)
    _assert_route(r, w, "(G) max_pivots = %d" % budget)
    assert not (r.status == lp.OK).any(), r.status
