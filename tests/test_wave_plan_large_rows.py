"""The routing of frontier waves beyond the 64 KB LDS window (children with ld > 8192) under the pool knob large_rows, through the
host-only probe of WavePlan (gomilp_amd/csrc/frontier_pool.hpp).  No device is touched.

With the knob at 0 (default) such waves go to the workers, whole; at 1 the batched revised simplex takes those it would take within the
window (its chunked kernels, batch_revised.hip).  The tableau schedule never sees them: its control kernel's column limit
(n + 2 <= 7700, BatchEngine::eligible) is far below."""
import pytest

U, GEN = 1, 2   # lp.WP_* root flags: unit (slack) basis, searched basis present

FEAS, P1 = [(0, 1, 0.5)], [(0, -1, -0.5)]   # a branch row that keeps the slack start feasible / one that needs Phase I


@pytest.fixture(scope="module")
def lp():
    from gomilp_amd import lp
    return lp


def route(lp, roots, kids, **kw):
    return lp.debug_wave_plan(roots, kids, **kw)["route"]


BIG = (8200, 8200 + 16404, U)    # one-row children: 8201 rows (ld = 8202), n - m = 16404 >= 2 * 8201
EDGE = (8191, 8191 + 16400, U)   # K = 1: 8192 rows, ld = 8192, the last shape inside the window; K = 2: ld = 8194; n - m = 16400 >= 2 * 8193


def test_wave_beyond_the_window_needs_the_knob(lp):
    kids = [FEAS, P1]
    assert route(lp, [BIG], kids) == "WORKERS"
    assert route(lp, [BIG], kids, large_rows=0) == "WORKERS"
    assert route(lp, [BIG], kids, large_rows=1) == "REVISED"
    # a warm call needs warm_revised as within the window
    assert route(lp, [BIG], kids, warm=[1, 1], large_rows=1) == "WORKERS"
    assert route(lp, [BIG], kids, warm=[1, 1], large_rows=1, warm_revised=1) == "REVISED"
    assert route(lp, [BIG], kids, large_rows=1, batch_revised=0) == "WORKERS"


@pytest.mark.parametrize("knob", [0, 1])
def test_edge_of_the_window(lp, knob):
    assert route(lp, [EDGE], [FEAS, P1], large_rows=knob) == "REVISED"                                    # ld = 8192
    assert route(lp, [EDGE], [FEAS * 2, P1 * 2], large_rows=knob) == ("REVISED" if knob else "WORKERS")   # ld = 8194
    # the tallest relaxation of the wave decides
    assert route(lp, [EDGE], [FEAS, P1 * 2], large_rows=knob) == ("REVISED" if knob else "WORKERS")


def test_the_other_conditions_stay(lp):
    kids = [FEAS, P1]
    # narrow (n - m < 2m): the revised formulation does not apply, and the tableau schedule's column limit keeps it off the tableau
    assert route(lp, [(8200, 8200 + 4000, U)], kids, large_rows=1) == "WORKERS"
    assert route(lp, [(8200, 8200 + 4000, U)], kids, large_rows=0) == "WORKERS"
    # no slack basis
    assert route(lp, [(8200, 8200 + 16404, GEN)], kids, large_rows=1) == "WORKERS"
    assert route(lp, [(8200, 8200 + 16404, 0)], kids, large_rows=1) == "WORKERS"
    # the exact-step guard on every pivot
    assert route(lp, [BIG], kids, large_rows=1, exact_degenerate=2) == "WORKERS"
    # a periodic refresh stays on the workers
    assert route(lp, [BIG], kids, large_rows=1, refresh=50) == "WORKERS"
    # a branch row on a slack column: the child has no slack basis
    assert route(lp, [BIG], [FEAS, [(16404, 1, 0.5)]], large_rows=1) == "WORKERS"
    assert route(lp, [BIG], [FEAS, [(16403, 1, 0.5)]], large_rows=1) == "REVISED"


def test_never_the_tableau_schedule(lp):
    """BatchEngine::eligible is as it was: n + 2 <= 7700 keeps every shape beyond the window off the tableau schedule, whatever the knobs"""
    for root in (BIG, EDGE, (8200, 8200 + 4000, U), (8200, 8200 + 64, U), (8200, 8200 + 16404, GEN)):
        for kw in ({}, {"large_rows": 1}, {"large_rows": 1, "exact_degenerate": 0, "cond_guard": 0}, {"large_rows": 1, "batch_revised": 0}):
            assert route(lp, [root], [FEAS * 2, P1 * 2], **kw) != "TABLEAU", (root, kw)


def test_within_the_window_the_knob_changes_nothing(lp):
    for root in ((300, 902, U), (300, 901, U), (255, 255 + 512, U), (96, 160, U), (300, 902, GEN)):
        for kids in ([FEAS] * 4, [FEAS, P1 * 2]):
            assert lp.debug_wave_plan([root], kids, large_rows=1) == lp.debug_wave_plan([root], kids), (root, kids)


def test_row_chunk_is_a_pool_knob_with_the_context_value_checks(lp):
    """the pool remembers row_chunk (the forced chunk of the batched schedule under large_rows = 1); the routing does not depend on it"""
    for v in (0, 512, 1536, 8192):
        assert route(lp, [BIG], [FEAS, P1], large_rows=1, row_chunk=v) == "REVISED"
        assert route(lp, [BIG], [FEAS, P1], row_chunk=v) == "WORKERS"
    for v in (-512, 256, 1000, 8704):
        with pytest.raises(ValueError):
            route(lp, [BIG], [FEAS, P1], large_rows=1, row_chunk=v)
