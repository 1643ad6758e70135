"""The routing of wide waves whose root has no slack basis (equality rows: a searched basis; pool knob rev_general, DESIGN.md sections
2.5e "Equality-form roots" and 2.5f) through the host-only probe of WavePlan.  No device is touched."""
import pytest

U, GEN = 1, 2   # lp.WP_* root flags: unit (slack) basis, searched basis present

EQ = (80, 316, GEN)          # 24 equality + 56 inequality rows over 260 variables: n - m = 236 >= 2 (m + K) up to K = 38
SLACK = (300, 904, U)        # a wide slack root of more than 256 rows: no exact-step guard at the default knobs
DOWN, UP = [(0, 1, 0.5)], [(0, -1, -0.5)]


@pytest.fixture(scope="module")
def lp():
    from gomilp_amd import lp
    return lp


def route(lp, roots, kids, **kw):
    return lp.debug_wave_plan(roots, kids, **kw)["route"]


def test_a_wide_general_root_takes_the_batched_revised_simplex(lp):
    assert route(lp, [EQ], [DOWN, UP] * 12) == "REVISED"
    assert route(lp, [EQ], [[]] * 2) == "REVISED"            # K = 0: independent equality-form LPs


def test_knob_off_is_the_worker_path(lp):
    assert route(lp, [EQ], [DOWN, UP] * 12, rev_general=0) == "WORKERS"
    assert route(lp, [EQ], [DOWN, UP] * 12, batch_revised=0) == "WORKERS"


def test_a_warm_call_stays_on_the_workers(lp):
    assert route(lp, [EQ], [DOWN, UP], warm=[1, 1]) == "WORKERS"
    assert route(lp, [EQ], [DOWN, UP], warm=[1, 1], warm_revised=1) == "WORKERS"
    assert route(lp, [EQ], [DOWN, UP], warm=[0, 0], warm_revised=1) == "WORKERS"


def test_the_condition_guard_keeps_small_bases(lp):
    small = (60, 240, GEN)
    assert route(lp, [small], [[]] * 2, cond_guard=1) == "WORKERS"
    assert route(lp, [small], [[]] * 2, cond_guard=0) == "REVISED"
    assert route(lp, [(64, 256, GEN)], [DOWN] * 2, cond_guard=1) == "REVISED"   # children of 65 rows


def test_mixed_slack_and_general_roots_are_one_schedule(lp):
    kids, rof = [DOWN, UP, DOWN, UP], [0, 0, 1, 1]
    assert route(lp, [SLACK, EQ], kids, root_of=rof, rev_roots=1) == "REVISED"
    assert route(lp, [SLACK, EQ], kids, root_of=rof, rev_roots=0) == "WORKERS"
    assert route(lp, [EQ, SLACK], kids, root_of=rof, rev_roots=1) == "REVISED"
    assert route(lp, [SLACK, EQ], kids, root_of=rof, rev_general=0) == "WORKERS"
    # roots the pool merely holds do not count
    assert route(lp, [SLACK, EQ], [DOWN, UP], root_of=[0, 0], rev_general=0) == "REVISED"


def test_the_guard_modes_and_the_shape_rule(lp):
    # mode 0 (no guard) and strict mode keep the worker path; mode 2 runs the same guarded loop as mode 1
    assert route(lp, [EQ], [DOWN] * 2, exact_degenerate=0) == "WORKERS"
    assert route(lp, [EQ], [DOWN] * 2, exact_degenerate=3) == "WORKERS"
    assert route(lp, [EQ], [DOWN] * 2, exact_degenerate=2) == "REVISED"
    # n - m = 236: children of 118 rows are wide (236 >= 236), of 119 rows they are not — and a narrow general root is the tableau's
    assert route(lp, [EQ], [DOWN * 16]) == "REVISED"            # 96 rows
    assert route(lp, [EQ], [DOWN * 38], rev_general=2) == "REVISED"
    assert route(lp, [EQ], [DOWN * 39], rev_general=2) != "REVISED"
    assert route(lp, [(80, 200, GEN)], [DOWN] * 2) == "TABLEAU"
    # a branch row on a column at or beyond n0 - m0 (the rule of slack roots, kept)
    assert route(lp, [EQ], [[(236, 1, 0.5)]]) == "WORKERS"
    # one-pass staging only: a pool that stages in chunks keeps these waves on the workers
    assert route(lp, [EQ], [DOWN] * 2, large_rows=1) == "REVISED"
    assert route(lp, [EQ], [DOWN] * 2, large_rows=1, row_chunk=512) == "WORKERS"
    # children of up to 96 rows at the default, of up to 300 rows with the knob at 2
    assert route(lp, [(95, 400, GEN)], [DOWN] * 2) == "REVISED"
    assert route(lp, [(96, 400, GEN)], [DOWN] * 2) == "WORKERS"
    assert route(lp, [(96, 400, GEN)], [DOWN] * 2, rev_general=2) == "REVISED"
    assert route(lp, [(299, 1200, GEN)], [DOWN] * 2, rev_general=2) == "REVISED"
    assert route(lp, [(300, 1200, GEN)], [DOWN] * 2, rev_general=2) == "WORKERS"
    with pytest.raises(ValueError):
        route(lp, [EQ], [DOWN], rev_general=3)
