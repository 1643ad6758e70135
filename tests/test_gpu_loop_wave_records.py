"""The 16 x 128 instance of the persistent loop kernel with one exchange record per WAVE (btg_kernels.hip xchg_wave; default up to 2048 rows)
against the live oracle and against the single-workgroup kernels (bt_groups = -1) on LPs built to tie the two argmins of a pivot at every
level the exchange decides on: inside a wave, between the two waves of a workgroup, between workgroups.

Context knob bt_groups = 16 puts the instance on LPs of a few hundred rows: thread t of workgroup g owns row and nonbasic position
128 g + t, lanes 0..63 of a workgroup are its wave 0.  LPs in the standard form of synth.dense_lp_standard_form (A = [G | I], slack start:
structural column j starts at nonbasic position j, the slack of row i at basis position m - 1 - i).  Sizes above 256 rows: up to there the engine hands
(nearly) degenerate pivots to the host (knob exact_degenerate) and the kernel's own tie-breaks and Bland steps would not run.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SPACINGS = (1, 64, 128)   # same wave | the two waves of one workgroup | two workgroups


def _standard(c, G, h):
    m, nv = G.shape
    A = np.zeros((m, nv + m))
    A[:, :nv] = G
    A[np.arange(m), nv + np.arange(m)] = 1.0
    return np.concatenate([c, np.zeros(m)]), A, h.copy()


ROW_P = 131   # basis position of the first tied row: lane 3 of wave 0 of workgroup 1 (+ 64: its wave 1, + 128: workgroup 2)


def tied_lp(m, seed, cols=False, rows=None):
    """Dense LP of synth.dense_lp_inequality_form with exact ties.  Column 30 has the lowest cost and enters first.
    cols: it stands four times, at nonbasic positions 30, + 1, + 64, + 128 (one tie inside a wave, between the waves of a workgroup and between
    workgroups at once), and two more columns stand twice, 64 resp. 128 apart, with the next lowest costs.
    rows (1, 64, 128 or "all"): equal rows with equal right-hand sides at basis positions ROW_P and ROW_P + rows (all: + 1, + 64, + 128) whose
    ratio in column 30 lies below every other, so the first ratio test ties and leaves basic variables at level zero.  The slack start
    lists the basis from the last slack down (findLinearlyIndependent): the row at basis position p is row m - 1 - p."""
    from gomilp_amd import synth
    c, G, h = synth.dense_lp_inequality_form(m, seed)
    c[30] = -1.5
    twins = [30]
    if cols:
        twins = [30] + [30 + d for d in SPACINGS]
        for j in twins[1:]:
            G[:, j] = G[:, 30]
            c[j] = c[30]
        G[:, 17 + 64] = G[:, 17]
        c[17] = c[17 + 64] = -1.375
        G[:, 140 + 128] = G[:, 140]
        c[140] = c[140 + 128] = -1.25
    if rows:
        pos = [ROW_P] + [ROW_P + d for d in (SPACINGS if rows == "all" else (rows,))]
        for p in pos:
            G[m - 1 - p] = G[m - 1 - ROW_P]
            G[m - 1 - p, twins] = 0.9375
            h[m - 1 - p] = 0.375
    return _standard(c, G, h)


def unbounded_lp(m, seed):
    """tied_lp (no tied rows: a run without level-zero vertices, whose pivots the rounding noise of the reference's fresh solves would
    decide) with a ray: two equal structural columns, two workgroups apart, without a positive entry, priced in after some sixty pivots."""
    from gomilp_amd import synth
    c, A, b = tied_lp(m, seed)
    u = synth.splitmix64_uniform(seed + 100, m)
    for j in (50, 50 + 128):
        A[:, j] = -u
        c[j] = -0.375
    return c, A, b


def phase1_lp(m, seed):
    """tied_lp (rows tied four ways) with three rows x_j >= 1 / 32: negative right-hand sides, the slack basis is infeasible (Phase I)."""
    c, A, b = tied_lp(m, seed, rows="all")
    nv = A.shape[1] - m
    for i, j in ((60, 7), (60 + 64, 9), (60 + 128, 11)):
        A[i, :nv] = 0.0
        A[i, j] = -1.0
        b[i] = -0.03125
    return c, A, b


def bland_lp(m, seed):
    """Integer data (entries 0..3, right-hand sides 0..8 with zeros among them, costs -(0..4)), duplicate rows and columns at the three
    spacings: zero ratios at the start and along the way, so pivots fall to the Bland rule."""
    rng = np.random.default_rng(9100 + seed)
    G = rng.integers(0, 4, (m, m)).astype(float)
    G[0] = np.maximum(G[0], 1.0)   # every column bounded by row 0
    h = rng.integers(1, 9, m).astype(float)
    h[rng.choice(np.arange(1, m), size=m // 8, replace=False)] = 0.0
    c = -rng.integers(0, 5, m).astype(float)
    for k, d in enumerate(SPACINGS):
        G[:, 10 + 3 * k + d] = G[:, 10 + 3 * k]
        c[10 + 3 * k + d] = c[10 + 3 * k] = -4.0
        G[25 + 3 * k + d] = G[25 + 3 * k]
        h[25 + 3 * k + d] = h[25 + 3 * k] = 0.0
    return _standard(c, G, h)


def _trace(piv):
    """(phase, min_idx, replace, entering, leaving) per pivot."""
    return np.array(piv, dtype=np.int64).reshape(-1, 6)[:, [0, 2, 3, 4, 5]]


def _wave_launches(lp):
    f = lp.lib().gomilp_debug_loop_wave_rec_launches
    f.restype = ctypes.c_longlong
    return int(f())


def _solve(lp, c, A, b, tol=0.0, **knobs):
    cx = lp.Context(**knobs)
    try:
        return cx.upload(c, A, b).solve(tol, trace=True)
    finally:
        cx.close()


def _same(g, o, what):
    """Status, pivot trace, and where there is a solution final basis, x and z bits.  (The engine hands out no trace behind an unbounded
    end: there the pivot counts of _check stand for it.)"""
    assert g.status == o.status, (what, g.status, o.status)
    if len(g.pivots) or o.x is not None:
        got, want = _trace(g.pivots), _trace(o.pivots)
        assert got.shape == want.shape, "%s: %d pivots against %d" % (what, len(got), len(want))
        assert np.array_equal(got, want), "%s: first differing pivot %d" % (what, int(np.argmax((got != want).any(axis=1))))
    if o.x is not None:
        assert np.array_equal(g.basis, o.basis), what
        assert np.array_equal(g.x, o.x) and g.z == o.z, what + ": x / z bits"


def _check(lp, O, c, A, b, tol=0.0):
    """The wave-record instance against the live oracle and against the single-workgroup kernels; returns (result, oracle result)."""
    o = O.simplex(c, A, b, tol, None, fast_initial_basis=True, trace=True)
    before = _wave_launches(lp)
    g = _solve(lp, c, A, b, tol, bt_groups=16)
    assert _wave_launches(lp) > before and g.stats["pipeline"] == "blocked" and g.stats["device_retries"] == 0   # the kernel under test ran, and to its end
    one = _solve(lp, c, A, b, tol, bt_groups=-1)
    assert g.stats["kernel_launches"] < one.stats["kernel_launches"]   # (one launch per 512 pivots against two per block)
    _same(g, o, "oracle")
    _same(g, one, "bt_groups=-1")
    assert (g.stats["pivots_phase1"], g.stats["pivots_phase2"]) == (o.pivots_phase1, o.pivots_phase2)
    assert (g.stats["pivots_phase1"], g.stats["pivots_phase2"]) == (one.stats["pivots_phase1"], one.stats["pivots_phase2"])
    return g, o


@pytest.fixture(scope="module")
def mods():
    from gomilp_amd import lp
    from oracle import oracle as O
    return lp, O


@pytest.mark.parametrize("rows", [1, 64, 128, "all"])
def test_tied_rows_one_lane_one_wave_one_workgroup_apart(mods, rows):
    """Equal rows at basis positions 131 and 131 + 1 / + 64 / + 128 (or all four) tie the first ratio test: the first position leaves, as in
    floats.MinIdx, and the others stay behind at level zero."""
    lp, O = mods
    g, o = _check(lp, O, *tied_lp(300, 11, rows=rows))
    assert o.status == lp.OK
    assert _trace(o.pivots)[0, 1:3].tolist() == [30, ROW_P]


@pytest.mark.parametrize("m,seed,rows", [(300, 11, None), (320, 12, None), (320, 12, "all")])
def test_duplicate_columns_one_lane_one_wave_one_workgroup_apart(mods, m, seed, rows):
    """Column 30 four times (positions 30, 31, 94, 158), columns 17 / 81 and 140 / 268 twice: equal columns keep equal reduced costs, so every
    time one of them is the entering choice it is an exact tie, and the first position must win.  tol = 1e-10: at tol = 0 the reference
    itself re-enters a basic column's twin on its rounding noise (reduced cost -1e-17) and on half of these LPs never ends."""
    lp, O = mods
    g, o = _check(lp, O, *tied_lp(m, seed, cols=True, rows=rows), tol=1e-10)
    assert o.status == lp.OK
    tr = _trace(o.pivots)
    assert tr[0, 1] == 30 and {30, 17, 140} <= set(tr[:, 3].tolist())   # the first of each group entered


def test_unbounded_end(mods):
    lp, O = mods
    g, o = _check(lp, O, *unbounded_lp(300, 11))
    assert o.status == lp.ERR_UNBOUNDED and o.pivots_phase2 > 20 and o.bland_steps == 0


def test_phase_one_start(mods):
    lp, O = mods
    g, o = _check(lp, O, *phase1_lp(300, 11))
    assert o.status == lp.OK and o.phase1_used and o.pivots_phase1 > 0 and g.stats["phase1_used"]


def test_bland_steps_on_integer_data(mods):
    lp, O = mods
    g, o = _check(lp, O, *bland_lp(288, 3))
    assert o.status == lp.OK and o.bland_steps > 20 and g.stats["bland_steps"] > 20


def test_1100_rows_at_default_knobs_equal_the_single_workgroup_kernels(mods):
    """The default path of the 1025..2048-row class (no knob: 16 x 128 threads, wave records) against bt_groups = -1."""
    lp, _ = mods
    from gomilp_amd import synth
    c, A, b = synth.dense_lp_standard_form(1100, 9)
    before = _wave_launches(lp)
    g = _solve(lp, c, A, b)
    assert _wave_launches(lp) > before and g.status == lp.OK and g.stats["device_retries"] == 0
    one = _solve(lp, c, A, b, bt_groups=-1)
    _same(g, one, "bt_groups=-1")
