"""The wave-record instance of the persistent loop kernel (16 x 128 threads, btg_kernels.hip) and its sixteen block terms per row / column:
the shift of the v' terms runs behind the post of the next pivot's first exchange 0 (shift_v), so between two pivots the newest term lives in
a register of its own, the start of a block clears the terms one entry early, and the first exchange 0 of a pivot is one call for ordinary
and set-up pivots alike.  (The cases were laid out for term sums by row broadcast as well — term l fetched by lane l & 15 of every 16-lane
row; that part was measured and not kept, the cases hold for any layout of the terms.)  Against the live oracle, trace and bits, and against
the single-workgroup kernels (bt_groups = -1):
  * row and column counts that leave the last 16-lane row of a wave part padding or a single lane, more and fewer columns than rows;
  * every term count: launches of 32 pivots (a first block without lagging terms, later blocks with eight) and the default chunk, pivot
    counts of at least 40 so that all sixteen terms are live;
  * the winner of both exchanges in lanes 0, 15, 16, 31, 32, 47, 48 and 63 of a wave, at the first pivot and behind the sixteenth;
  * Bland steps with all terms live (several exchanges 0 per pivot, ONE shift), a Phase-I start (the set-up pivot), an unbounded end,
    the default path at 1300 rows.

Pattern, helpers and LP layout of test_gpu_loop_wave_records.py (context knob bt_groups = 16: thread t of workgroup g owns row and nonbasic
position 128 g + t; structural column j starts at nonbasic position j, the slack of row i at basis position m - 1 - i).  Seeds were picked
with the CPU oracle; what they were picked for is asserted."""
import pytest

from tests.test_gpu_loop_wave_records import _check, _same, _solve, _standard, _trace, _wave_launches, bland_lp, phase1_lp, unbounded_lp

pytestmark = pytest.mark.gpu

M = 300
LANES = {0, 15, 16, 31, 32, 47, 48, 63}   # first and last lane of every 16-lane row of a wave
# (entering position, leaving position) of the first pivot: the eight lanes in both waves of workgroups 0 and 1, each lane on both sides
FIRST = ((0, 255), (15, 240), (80, 175), (95, 160), (160, 95), (175, 80), (240, 15), (255, 0))


@pytest.fixture(scope="module")
def mods():
    from gomilp_amd import lp
    from oracle import oracle as O
    return lp, O


def first_pivot_at(e, l, seed=21):
    """Dense LP whose first entering column stands at nonbasic position e (the lowest cost) and whose first leaving row stands at basis
    position l (row m - 1 - l: the lowest ratio in that column, the way tied_lp builds its rows)."""
    from gomilp_amd import synth
    c, G, h = synth.dense_lp_inequality_form(M, seed)
    c[e] = -1.5
    G[M - 1 - l, e] = 0.9375
    h[M - 1 - l] = 0.375
    return _standard(c, G, h)


def _lanes_behind_the_sixteenth(o):
    late = _trace(o.pivots)[16:]
    return set((late[:, 1] & 63).tolist()) & LANES, set((late[:, 2] & 63).tolist()) & LANES


@pytest.mark.parametrize("m,nv,seed", [(257, None, 1), (290, None, 4), (300, None, 4), (300, None, 5), (300, 200, 3), (300, 450, 2)])
def test_row_and_column_counts_off_the_16_lane_row(mods, m, nv, seed):
    """257 = 16 x 16 + 1 rows (the last 16-lane row holds a single real lane), 290 and 300 (part padding); 300 rows with 200 and with 450
    structural columns: row slabs and column slabs differ.  More than 40 pivots each: all sixteen terms live, several blocks."""
    lp, O = mods
    from gomilp_amd import synth
    g, o = _check(lp, O, *synth.dense_lp_standard_form(m, seed, nv))
    assert o.status == lp.OK and not o.phase1_used and o.bland_steps == 0 and o.pivots_phase2 >= 40


def test_winners_in_the_first_and_last_lane_of_every_row_behind_the_sixteenth_pivot(mods):
    """Two dense LPs (seeds 4 and 5 at 300 rows) whose pivots behind the sixteenth — all terms live — put the entering column and the leaving
    row into each of the lanes 0, 15, 16, 31, 32, 47, 48 and 63 of a wave at least once."""
    lp, O = mods
    from gomilp_amd import synth
    ql, pl = set(), set()
    for seed in (4, 5):
        g, o = _check(lp, O, *synth.dense_lp_standard_form(M, seed))
        assert o.status == lp.OK
        q1, p1 = _lanes_behind_the_sixteenth(o)
        ql |= q1
        pl |= p1
    assert ql == LANES and pl == LANES


@pytest.mark.parametrize("e,l", FIRST)
def test_first_pivot_winners_in_the_first_and_last_lane_of_every_row(mods, e, l):
    lp, O = mods
    assert (e & 63) in LANES and (l & 63) in LANES
    g, o = _check(lp, O, *first_pivot_at(e, l))
    assert o.status == lp.OK and _trace(o.pivots)[0, 1:3].tolist() == [e, l] and o.pivots_phase2 >= 32


def test_launches_of_32_pivots_give_the_trace_of_the_default_chunk(mods):
    """loop_chunk = 32: every launch starts with a block without lagging terms (nothing to shift but zeros) and goes on with blocks of eight
    lagging terms; the default chunk runs the same 140 pivots in one launch."""
    lp, O = mods
    from gomilp_amd import synth
    c, A, b = synth.dense_lp_standard_form(M, 4)
    before = _wave_launches(lp)
    whole = _solve(lp, c, A, b, bt_groups=16)
    mid = _wave_launches(lp)
    cut = _solve(lp, c, A, b, bt_groups=16, loop_chunk=32)
    assert mid > before and _wave_launches(lp) - mid > mid - before   # more launches of the instance for the same pivots
    assert whole.stats["device_retries"] == 0 and cut.stats["device_retries"] == 0
    assert whole.status == lp.OK and _trace(whole.pivots).shape[0] >= 40
    _same(cut, whole, "loop_chunk=32")
    o = O.simplex(c, A, b, 0.0, None, fast_initial_basis=True, trace=True)
    _same(cut, o, "oracle")


@pytest.mark.parametrize("m,seed", [(257, 1), (288, 3)])
def test_bland_steps_with_all_terms_live(mods, m, seed):
    """A Bland step runs several exchanges 0 and `column` several times inside one pivot: the terms are shifted once, behind the first.
    53 and 26 pivots, every one a Bland step: from the seventeenth on all sixteen terms are live."""
    lp, O = mods
    g, o = _check(lp, O, *bland_lp(m, seed))
    assert o.status == lp.OK and o.bland_steps > 20 and g.stats["bland_steps"] > 20 and o.pivots_phase2 > 16


def test_phase_one_start(mods):
    """The forced set-up pivot: its exchange 0 is the call of the ordinary pivots, with the candidate list of the forced column."""
    lp, O = mods
    g, o = _check(lp, O, *phase1_lp(290, 12))
    assert o.status == lp.OK and o.phase1_used and o.pivots_phase1 > 0 and g.stats["phase1_used"] and o.pivots_phase2 >= 40


def test_unbounded_end(mods):
    lp, O = mods
    g, o = _check(lp, O, *unbounded_lp(290, 12))
    assert o.status == lp.ERR_UNBOUNDED and o.pivots_phase2 >= 40 and o.bland_steps == 0


def test_1300_rows_at_default_knobs_equal_the_single_workgroup_kernels(mods):
    lp, _ = mods
    from gomilp_amd import synth
    c, A, b = synth.dense_lp_standard_form(1300, 7)
    before = _wave_launches(lp)
    g = _solve(lp, c, A, b)
    assert _wave_launches(lp) > before and g.status == lp.OK and g.stats["device_retries"] == 0
    one = _solve(lp, c, A, b, bt_groups=-1)
    _same(g, one, "bt_groups=-1")
