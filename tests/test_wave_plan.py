"""The routing of a frontier wave (WavePlan, gomilp_amd/csrc/frontier_pool.hpp) through its host-only probe: the table of DESIGN.md
section 2.5f, both sides of every edge.  No device is touched."""
import itertools

import pytest

U, GEN, BNEG, BAD = 1, 2, 4, 8   # lp.WP_* root flags: unit (slack) basis, searched basis present, some b < 0, verify verdict not OK


@pytest.fixture(scope="module")
def lp():
    from gomilp_amd import lp
    return lp


NARROW = (96, 160, U)      # n - m = 64 < 2m, above the 64-row guard
WIDE = (300, 904, U)       # n - m = 604 >= 2 (m + K) up to K = 2; more than 256 rows: no exact-step guard
FEAS, P1 = [(0, 1, 0.5)], [(0, -1, -0.5)]   # a branch row that keeps the slack start feasible / one that needs Phase I


def plan(lp, roots, kids, **kw):
    return lp.debug_wave_plan(roots, kids, **kw)


def route(lp, roots, kids, **kw):
    return plan(lp, roots, kids, **kw)["route"]


def test_probe_needs_no_device_and_refuses_bad_input(lp):
    p = plan(lp, [NARROW], [FEAS] * 3)
    assert p == {"route": "TABLEAU", "cut": "ONE", "groups": ["whole"] * 3, "pos": [0, 1, 2]}
    assert plan(lp, [NARROW], []) == {"route": "WORKERS", "cut": "NONE", "groups": [], "pos": []}   # count = 0
    with pytest.raises(ValueError):
        plan(lp, [NARROW], [FEAS], no_such_knob=1)
    with pytest.raises(ValueError):
        plan(lp, [NARROW], [FEAS], root_of=[1])
    with pytest.raises(ValueError):
        plan(lp, [NARROW], [FEAS, FEAS], warm=[1, 0], spent=[1])   # (not a warm start)
    with pytest.raises(ValueError):
        plan(lp, [(0, 10, U)], [FEAS])


def test_formulation_edge_n_minus_m_against_2m(lp):
    # children of 301 rows: n - m = 601 < 602: the tableau; 602: the revised formulation
    assert route(lp, [(300, 901, U)], [FEAS] * 4) == "TABLEAU"
    assert route(lp, [(300, 902, U)], [FEAS] * 4) == "REVISED"
    # ... which needs a slack basis, and more than 256 rows while the exact-step guard is on
    assert route(lp, [(300, 902, GEN)], [FEAS] * 4) == "WORKERS"
    assert route(lp, [(255, 255 + 512, U)], [FEAS] * 4) == "WORKERS"          # 256 rows: guarded
    assert route(lp, [(256, 256 + 514, U)], [FEAS] * 4) == "REVISED"          # 257 rows
    assert route(lp, [(255, 255 + 512, U)], [FEAS] * 4, exact_degenerate=0) == "REVISED"
    assert route(lp, [(300, 902, U, 1e10)], [FEAS] * 4) == "WORKERS"           # scale_span > 1e9: guarded
    assert route(lp, [(300, 902, U)], [FEAS] * 4, exact_degenerate=2) == "WORKERS"
    # the relaxation with the most rows decides: K = 2 and K = 3 on n - m = 604 (2 * 302 = 604, 2 * 303 = 606)
    assert route(lp, [WIDE], [FEAS, FEAS * 2]) == "REVISED"
    assert route(lp, [WIDE], [FEAS, FEAS * 3]) == "TABLEAU"


def test_small_bases_and_the_condition_guard(lp):
    small, above = (63, 100, U), (64, 100, U)      # children of 64 / 65 rows
    assert route(lp, [small], [FEAS] * 4) == "WORKERS"
    assert route(lp, [small], [FEAS] * 4, cond_guard=0) == "TABLEAU"
    assert route(lp, [above], [FEAS] * 4) == "TABLEAU"
    # the widest relaxation of the wave decides for the tableau; the revised schedule looks at the smallest
    assert route(lp, [small], [FEAS, FEAS * 2]) == "TABLEAU"
    wide_small = (63, 63 + 200, U)
    assert route(lp, [wide_small], [FEAS] * 4, exact_degenerate=0) == "WORKERS"
    assert route(lp, [wide_small], [FEAS] * 4, exact_degenerate=0, cond_guard=0) == "REVISED"
    assert route(lp, [wide_small], [FEAS, FEAS * 2], exact_degenerate=0) == "WORKERS"


def test_control_kernel_column_limit(lp):
    # n + 2 > 7700 with n = the child's columns (K = 1)
    assert route(lp, [(3849, 7697, U)], [FEAS] * 2) == "TABLEAU"    # 7698 + 2 = 7700
    assert route(lp, [(3849, 7698, U)], [FEAS] * 2) == "WORKERS"    # 7701


@pytest.mark.parametrize("m,with_large_loop", [(1024, "TABLEAU"), (1025, "WORKERS"), (2048, "WORKERS"), (2049, "TABLEAU")])
def test_large_loop_takes_need_1025_to_2048(lp, m, with_large_loop):
    root = (m, m + 64, U)   # independent LPs (K = 0): need = max(m, batch_ldt(64)) = m
    assert route(lp, [root], [[]] * 2) == "TABLEAU"
    assert route(lp, [root], [[]] * 2, large_loop=1) == with_large_loop


def test_a_negative_b_is_one_tableau_column_more(lp):
    # n - m = 1024 nonbasic columns: ldt 1024, with the Phase-I artificial 1088
    shape = (600, 1624)
    assert route(lp, [shape + (U,)], [[]] * 2, large_loop=1) == "TABLEAU"
    assert route(lp, [shape + (U | BNEG,)], [[]] * 2, large_loop=1) == "WORKERS"
    assert route(lp, [shape + (U,)], [[], P1], large_loop=1) == "WORKERS"        # (a branch row does the same)
    assert route(lp, [shape + (GEN,)], [[]] * 2, large_loop=1) == "WORKERS"      # (and a searched basis: feasibility unknown on the host)
    # the phase split: every child of such a root is a Phase-I start
    kids = [FEAS] * 8 + [P1] * 8
    assert plan(lp, [NARROW], kids)["cut"] == "PHASE_SPLIT"
    assert plan(lp, [(96, 160, U | BNEG)], kids)["cut"] == "ONE"
    p = plan(lp, [(96, 160, GEN)], kids)
    assert (p["route"], p["cut"]) == ("TABLEAU", "ONE")
    assert route(lp, [(96, 160, 0)], kids) == "WORKERS"              # neither a slack basis nor a searched one
    assert route(lp, [(96, 160, U | BAD)], kids) == "WORKERS"        # the verify verdict


def test_halves_need_four_large_relaxations_and_a_cold_call(lp):
    big = (1100, 2200, U)   # need 1100: the 8-workgroup block kernel, 16 pivots per block
    assert plan(lp, [big], [[]] * 3)["cut"] == "ONE"
    p = plan(lp, [big], [[]] * 4)
    assert (p["cut"], p["groups"], p["pos"]) == ("HALVES", ["half0", "half0", "half1", "half1"], [0, 1, 0, 1])
    p = plan(lp, [big], [[]] * 5)
    assert (p["groups"], p["pos"]) == (["half0"] * 2 + ["half1"] * 3, [0, 1, 0, 1, 2])
    assert plan(lp, [big], [[]] * 4, split_large=0)["cut"] == "ONE"
    assert plan(lp, [(1024, 2048, U)], [[]] * 4)["cut"] == "ONE"       # need 1024: blocks of 8
    assert plan(lp, [(4096, 8192 - 600, U)], [[]] * 4)["cut"] == "HALVES"   # need 4096
    p = plan(lp, [big], [[]] * 4, warm=[0] * 4)
    assert (p["route"], p["cut"]) == ("TABLEAU", "ONE_GATHERED")
    # halves go before the phase split
    kids = [FEAS] * 8 + [P1] * 8
    assert plan(lp, [big], kids)["cut"] == "HALVES"
    assert plan(lp, [big], kids, split_large=0)["cut"] == "PHASE_SPLIT"


def test_phase_split_needs_16_cold_relaxations_and_both_groups(lp):
    kids = [FEAS, P1] * 8
    p = plan(lp, [NARROW], kids)
    assert p["cut"] == "PHASE_SPLIT"
    assert p["groups"] == ["feasible", "phase1"] * 8 and p["pos"] == [i // 2 for i in range(16)]
    assert plan(lp, [NARROW], kids[:15])["cut"] == "ONE"
    assert plan(lp, [NARROW], kids, split_phase=0)["cut"] == "ONE"
    assert plan(lp, [NARROW], [FEAS] * 16)["cut"] == "ONE"
    assert plan(lp, [NARROW], [P1] * 16)["cut"] == "ONE"
    assert plan(lp, [NARROW], [FEAS] * 15 + [[(0, 1, 0.5), (1, -1, -1e-13)]])["cut"] == "ONE"          # -1e-13 is no Phase-I start
    assert plan(lp, [NARROW], [FEAS] * 15 + [[(0, 1, 0.5), (1, -1, -2e-13)]])["cut"] == "PHASE_SPLIT"
    # per root: children of a root with b < 0 are Phase-I starts, whatever their rows
    p = plan(lp, [NARROW, (96, 160, U | BNEG)], [FEAS] * 16, root_of=[0, 1] * 8)
    assert p["cut"] == "PHASE_SPLIT" and p["groups"] == ["feasible", "phase1"] * 8


def test_roots_the_pool_holds_and_roots_the_wave_uses(lp):
    bad = (96, 160, U | BAD)
    # the tableau schedule asks every root the pool holds, the revised schedule the roots the wave uses
    assert route(lp, [NARROW, bad], [FEAS] * 4, root_of=[0] * 4) == "WORKERS"
    assert route(lp, [WIDE, bad], [FEAS] * 4, root_of=[0] * 4) == "REVISED"
    assert route(lp, [WIDE, bad], [FEAS] * 4, root_of=[0, 0, 0, 1]) == "WORKERS"
    assert route(lp, [WIDE, NARROW], [FEAS] * 4, root_of=[0] * 4) == "REVISED"
    # a second root: with rev_roots = 0 only waves of root 0 alone
    wide2 = (400, 1300, U)
    assert route(lp, [WIDE, wide2], [FEAS] * 4, root_of=[0, 1, 0, 1]) == "REVISED"
    assert route(lp, [WIDE, wide2], [FEAS] * 4, root_of=[1] * 4) == "REVISED"
    assert route(lp, [WIDE, wide2], [FEAS] * 4, root_of=[0, 1, 0, 1], rev_roots=0) == "WORKERS"
    assert route(lp, [WIDE, wide2], [FEAS] * 4, root_of=[1] * 4, rev_roots=0) == "WORKERS"
    assert route(lp, [WIDE, wide2], [FEAS] * 4, root_of=[0] * 4, rev_roots=0) == "REVISED"
    # each used root with the K range of its own children: K = 3 is too many rows for WIDE, not for wide2
    assert route(lp, [WIDE, wide2], [FEAS, FEAS * 3], root_of=[0, 1]) == "REVISED"
    assert route(lp, [WIDE, wide2], [FEAS * 3, FEAS], root_of=[0, 1]) == "WORKERS"
    # two narrow roots in one tableau wave
    assert route(lp, [NARROW, (128, 200, U)], [FEAS] * 4, root_of=[0, 1, 0, 1]) == "TABLEAU"


def test_a_branch_row_on_a_slack_column(lp):
    first_slack = WIDE[1] - WIDE[0]
    assert route(lp, [WIDE], [FEAS, [(first_slack - 1, 1, 0.5)]]) == "REVISED"
    assert route(lp, [WIDE], [FEAS, [(first_slack, 1, 0.5)]]) == "WORKERS"
    assert route(lp, [NARROW], [FEAS, [(NARROW[1] - 1, 1, 0.5)]]) == "TABLEAU"   # (the tableau schedule takes such rows)


def test_warm_calls(lp):
    kids = [FEAS] * 8
    # no resident parent: still the gathered lists
    p = plan(lp, [NARROW], kids, warm=[0] * 8)
    assert (p["route"], p["cut"], p["groups"], p["pos"]) == ("TABLEAU", "ONE_GATHERED", ["whole"] * 8, list(range(8)))
    assert plan(lp, [NARROW], kids)["cut"] == "ONE"
    # wide waves: the workers, cold, unless warm_revised
    assert route(lp, [WIDE], kids, warm=[0] * 8) == "WORKERS"
    assert route(lp, [WIDE], kids, warm=[1] * 8) == "WORKERS"
    assert route(lp, [WIDE], kids, warm=[0] * 8, warm_revised=1) == "REVISED"
    assert route(lp, [WIDE], kids, warm_revised=1) == "REVISED"
    # warm starts first; a child without branch rows is no warm start; every one warm: nothing left for the cold part
    p = plan(lp, [NARROW], [FEAS, [], FEAS, FEAS], warm=[1, 1, 0, 1])
    assert (p["cut"], p["groups"], p["pos"]) == ("ONE_GATHERED", ["warm", "whole", "whole", "warm"], [0, 0, 1, 1])
    p = plan(lp, [NARROW], kids, warm=[1] * 8)
    assert (p["cut"], p["groups"]) == ("NONE", ["warm"] * 8)
    # the cold rest of a warm call is cut like a cold wave of that size
    wave = [FEAS, P1] * 10
    warm = [1] * 4 + [0] * 16
    p = plan(lp, [NARROW], wave, warm=warm)
    assert p["cut"] == "PHASE_SPLIT" and p["groups"] == ["warm"] * 4 + ["feasible", "phase1"] * 8
    assert plan(lp, [NARROW], wave, warm=[1] * 5 + [0] * 15)["cut"] == "ONE_GATHERED"   # 15 cold


def test_a_spent_warm_start_comes_back_in_sorted_position(lp):
    wave = [FEAS, P1] * 10
    warm = [0, 0, 1, 0, 0, 1, 0, 1] + [0] * 12
    p = plan(lp, [NARROW], wave, warm=warm, spent=[5, 2])
    assert p["cut"] == "PHASE_SPLIT"   # 17 cold + 2 spent
    assert p["groups"] == ["feasible", "phase1"] * 3 + ["feasible", "warm"] + ["feasible", "phase1"] * 6
    feas = [i for i in range(20) if p["groups"][i] == "feasible"]
    ph1 = [i for i in range(20) if p["groups"][i] == "phase1"]
    assert [p["pos"][i] for i in feas] == list(range(len(feas))) and 2 in feas      # ascending with the index: 2 sits between 0 and 4
    assert [p["pos"][i] for i in ph1] == list(range(len(ph1))) and 5 in ph1
    # 14 cold + 1 warm that stays + 1 spent: 15, one run on gathered lists, the spent one in its place
    p = plan(lp, [NARROW], wave[:16], warm=[0] * 7 + [1, 1] + [0] * 7, spent=[7])
    assert p["cut"] == "ONE_GATHERED" and p["groups"] == ["whole"] * 8 + ["warm"] + ["whole"] * 7
    assert p["pos"] == list(range(8)) + [1] + list(range(8, 15))
    # ... and with it the 16th: the split
    p = plan(lp, [NARROW], wave[:17], warm=[0] * 7 + [1, 1] + [0] * 8, spent=[7])
    assert p["cut"] == "PHASE_SPLIT" and p["groups"][7] == "phase1" and p["groups"][8] == "warm"


def test_refresh_keeps_wide_waves_on_the_workers(lp):
    assert route(lp, [WIDE], [FEAS] * 4, refresh=50) == "WORKERS"
    assert route(lp, [WIDE], [FEAS] * 4, refresh=0) == "REVISED"
    assert route(lp, [NARROW], [FEAS] * 4, refresh=50) == "TABLEAU"


def test_stored_knobs_are_accepted_and_route_nothing(lp):
    for key in ("rev_exchange", "max_pivots", "batch_virt", "batch_res", "batch_loop", "sample_batch", "lu_large"):
        for roots in ([NARROW], [WIDE]):
            assert plan(lp, roots, [FEAS, P1] * 8, **{key: 0}) == plan(lp, roots, [FEAS, P1] * 8, **{key: 1}) == plan(lp, roots, [FEAS, P1] * 8)


KNOBS = ("batched", "batch_revised", "split_large", "split_phase", "large_loop")


def _rule(shape, k):
    """the stated rule for the three waves below (16 children, half of them Phase-I starts; `shape`: narrow, large, wide)"""
    if not k["batched"]:
        return "WORKERS", "NONE"
    if shape == "wide":   # no tableau (n - m >= 2m)
        return ("REVISED" if k["batch_revised"] else "WORKERS"), "NONE"
    if shape == "large" and k["large_loop"]:   # need 1100 in 1025..2048; narrow: no revised route
        return "WORKERS", "NONE"
    if shape == "large" and k["split_large"]:   # 16 >= 4 relaxations on blocks of 16, a cold call
        return "TABLEAU", "HALVES"
    return "TABLEAU", ("PHASE_SPLIT" if k["split_phase"] else "ONE")


@pytest.mark.parametrize("shape,root", [("narrow", NARROW), ("large", (1100, 2200, U)), ("wide", WIDE)])
def test_every_combination_of_the_routing_switches(lp, shape, root):
    kids = [FEAS, P1] * 8
    for values in itertools.product((0, 1), repeat=len(KNOBS)):
        k = dict(zip(KNOBS, values))
        p = plan(lp, [root], kids, **k)
        assert (p["route"], p["cut"]) == _rule(shape, k), (shape, k)
