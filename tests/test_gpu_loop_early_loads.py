"""The wave-record instance of the persistent loop kernel (16 x 128 threads, btg_kernels.hip): a wave's record is posted by the winner's own lane
(four 16-byte stores from one lane), and the row side of the row phase (u, x_B, the shift of the u terms, the basis list) runs under the row
load.  What that can break, against the live oracle and against the single-workgroup kernels (bt_groups = -1): the winner in every lane
position of an exchange, the ends of a launch right behind an exchange (optimum on the first and the second exchange of a block, a degenerate
pivot handed to the host), launch boundaries, the default path.  (The cases were laid out for loads issued inside the exchange as well; that
part was measured and not kept, the cases hold for any form of the exchange.)

Pattern, helpers and LP layout of test_gpu_loop_wave_records.py (context knob bt_groups = 16: thread t of workgroup g owns row and nonbasic
position 128 g + t; structural column j starts at nonbasic position j, the slack of row i at basis position m - 1 - i)."""
import pytest

from tests.test_gpu_loop_wave_records import _check, _same, _solve, _standard, _trace, _wave_launches, tied_lp

pytestmark = pytest.mark.gpu

M = 300
POSITIONS = (0, 63, 64, 127, 128, 299)   # lane 0 and lane 63 of both waves of workgroup 0, workgroup 1, the last real index before the padding


@pytest.fixture(scope="module")
def mods():
    from gomilp_amd import lp
    from oracle import oracle as O
    return lp, O


def entering_at(pos, seed=21):
    """Dense LP whose first entering column stands at nonbasic position pos (the lowest cost)."""
    from gomilp_amd import synth
    c, G, h = synth.dense_lp_inequality_form(M, seed)
    c[pos] = -1.5
    return _standard(c, G, h)


def leaving_at(pos, seed=21):
    """Column 30 enters first; the row at basis position pos (row m - 1 - pos) has the lowest ratio in it, the way tied_lp builds ROW_P."""
    from gomilp_amd import synth
    c, G, h = synth.dense_lp_inequality_form(M, seed)
    c[30] = -1.5
    G[M - 1 - pos, 30] = 0.9375
    h[M - 1 - pos] = 0.375
    return _standard(c, G, h)


@pytest.mark.parametrize("pos", POSITIONS)
def test_first_entering_column_in_every_lane_position(mods, pos):
    lp, O = mods
    g, o = _check(lp, O, *entering_at(pos))
    assert o.status == lp.OK and _trace(o.pivots)[0, 1] == pos


@pytest.mark.parametrize("pos", POSITIONS)
def test_first_leaving_row_in_every_lane_position(mods, pos):
    lp, O = mods
    g, o = _check(lp, O, *leaving_at(pos))
    assert o.status == lp.OK and _trace(o.pivots)[0, 1:3].tolist() == [30, pos]


@pytest.mark.parametrize("seed,rem", [(3, 0), (25, 1)])
def test_optimal_end_on_the_first_and_second_exchange_of_a_block(mods, seed, rem):
    """Blocks of 8 pivots: with a Phase-II pivot count of 8 n the exchange that finds the optimum is the first of a block (no current term yet,
    the tableau buffer of the new block), with 8 n + 1 the second (one current term).  Seeds picked with the oracle: 128 and 153 pivots."""
    lp, O = mods
    from gomilp_amd import synth
    g, o = _check(lp, O, *synth.dense_lp_standard_form(M, seed))
    assert o.status == lp.OK and not o.phase1_used and o.bland_steps == 0
    assert o.pivots_phase2 > 100 and o.pivots_phase2 % 8 == rem


def test_degenerate_pivots_handed_to_the_host_at_256_rows(mods):
    """Up to 256 rows the guards end the launch on a (nearly) degenerate ratio (ST_NEED_EXACT) and the host decides that pivot: the launch
    ends behind the second exchange, with the posted record of a pivot that is not committed.  Rows tied four ways (at 256 rows tied_lp's position 131 + 128 wraps to basis position 3, which leaves first)."""
    lp, O = mods
    g, o = _check(lp, O, *tied_lp(256, 11, rows="all"))
    assert o.status == lp.OK
    assert _trace(o.pivots)[0, 1:3].tolist() == [30, 3]


def test_four_blocks_per_launch_give_the_trace_of_the_default_chunk(mods):
    """loop_chunk = 32: r, x_B and the index lists are stored and loaded again every 32 pivots."""
    lp, O = mods
    from gomilp_amd import synth
    c, A, b = synth.dense_lp_standard_form(M, 25)   # (153 pivots: two launches at the default chunk of 512, five and more at 32)
    before = _wave_launches(lp)
    whole = _solve(lp, c, A, b, bt_groups=16)
    mid = _wave_launches(lp)
    cut = _solve(lp, c, A, b, bt_groups=16, loop_chunk=32)
    assert mid > before and _wave_launches(lp) - mid > mid - before   # more launches of the instance for the same pivots
    assert whole.stats["device_retries"] == 0 and cut.stats["device_retries"] == 0
    assert whole.status == lp.OK and _trace(whole.pivots).shape[0] > 32
    _same(cut, whole, "loop_chunk=32")
    o = O.simplex(c, A, b, 0.0, None, fast_initial_basis=True, trace=True)
    _same(cut, o, "oracle")


def test_1300_rows_at_default_knobs_equal_the_single_workgroup_kernels(mods):
    lp, _ = mods
    from gomilp_amd import synth
    c, A, b = synth.dense_lp_standard_form(1300, 5)
    before = _wave_launches(lp)
    g = _solve(lp, c, A, b)
    assert _wave_launches(lp) > before and g.status == lp.OK and g.stats["device_retries"] == 0
    one = _solve(lp, c, A, b, bt_groups=-1)
    _same(g, one, "bt_groups=-1")
