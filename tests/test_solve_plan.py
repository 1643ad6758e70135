"""Where a single solve goes: the engine's SolvePlan (gomilp_amd/csrc/engine.hpp, SolvePlan::make in engine.cpp) against the routing
table of DESIGN.md section 2.4 — host-only entry of the library, no GPU needed.  The expected values are literals, worked out from the
shape rules alone: ld = (m + 1) & ~1; the tableau row fits while n - m <= 8191; the block kernels take m <= 8192, ldt <= 8192,
ldt + ld <= 11946 with ldt = 512 * ceil((n - m + 1) / 512); the fused pipeline takes ld in {128, 256, 512, 1024, 2048, 4096}."""
import math

import pytest

THREE, FUSED, TABLEAU, BLOCKED = 0, 1, 2, 3
OK, UNSUPPORTED = 0, 13
INF = math.inf

# (start, m, n, scale_span, knobs) -> the fields asserted
TABLE = [
    ("slack", 8, 20, 1.0, {}, dict(pipeline=BLOCKED, guard=1e-9, cguard=0.0, replay_if_feasible=1)),
    ("slack", 8, 40, 1.0, {}, dict(pipeline=BLOCKED, guard=1e-9)),   # wide, exact steps wanted: the blocked tableau takes it
    ("slack", 8, 40, 1.0, dict(exact_degenerate=0), dict(pipeline=THREE, guard=0.0)),
    ("slack", 8, 40, 1.0, dict(blocked=0), dict(pipeline=THREE, guard=0.0)),
    ("slack", 128, 512, 1.0, dict(exact_degenerate=0), dict(pipeline=FUSED, guard=0.0)),
    ("slack", 128, 512, 1.0, dict(exact_degenerate=0, fused=0), dict(pipeline=THREE, guard=0.0)),
    ("slack", 300, 700, 1.0, {}, dict(pipeline=BLOCKED, guard=0.0, cguard=1e-9, replay_if_feasible=0)),
    ("slack", 300, 700, 1.0, dict(blocked=0), dict(pipeline=TABLEAU, guard=0.0)),
    ("slack", 300, 700, 1.0, dict(tableau=0), dict(pipeline=THREE, guard=0.0)),
    ("slack", 300, 1500, 1.0, {}, dict(pipeline=THREE, guard=0.0)),
    ("slack", 300, 1500, 1e10, {}, dict(pipeline=BLOCKED, guard=1e-9, badly_scaled=1)),
    ("slack", 300, 1500, 1.0, dict(exact_degenerate=2), dict(pipeline=BLOCKED, guard=1e-9)),
    ("slack", 300, 1500, 1.0, dict(exact_degenerate=3), dict(pipeline=BLOCKED, guard=INF)),
    ("slack", 300, 9000, 1.0, {}, dict(pipeline=THREE, guard=0.0)),
    ("slack", 300, 9000, 1.0, dict(exact_degenerate=3), None),
    ("slack", 8192, 11775, 1.0, {}, dict(pipeline=BLOCKED)),   # ldt 3584 + ld 8192 = 11776
    ("slack", 8192, 11776, 1.0, {}, dict(pipeline=TABLEAU)),   # ldt 4096: beyond bt_supported
    ("slack", 8194, 9000, 1.0, {}, dict(pipeline=THREE, use_tab=0)),   # beyond the LDS window
    ("supplied", 8194, 9000, 1.0, {}, None),
    ("searched", 8194, 9000, 1.0, {}, None),
    ("searched", 8, 20, 1.0, {}, dict(pipeline=BLOCKED, guard=1e-9, cguard=0.0, gen_start=1, gen_revised=0, needs_host_A=1)),
    ("searched", 300, 9000, 1.0, dict(exact_degenerate=1), dict(pipeline=THREE, gen_revised=1, guard=1e-9)),
    ("searched", 300, 9000, 1.0, dict(exact_degenerate=3), dict(pipeline=THREE, gen_revised=1, guard=INF)),
    ("searched", 300, 9000, 1.0, dict(exact_degenerate=0), dict(pipeline=THREE, gen_revised=1, guard=0.0)),
    ("searched", 128, 8400, 1.0, {}, dict(pipeline=THREE, gen_revised=1, guard=1e-9)),   # ld 128, yet never fused
    ("searched", 4000, 12200, 1.0, {}, None),   # m * n > 2^25: no host copy of A for the exact steps
]


def plan(m, n, start="slack", scale_span=1.0, **knobs):
    from gomilp_amd import lp
    return lp.debug_solve_plan(m, n, start, scale_span, **knobs)


@pytest.mark.parametrize("start,m,n,span,knobs,want", TABLE, ids=["%s-%dx%d-%g-%s" % (r[0], r[1], r[2], r[3], ",".join("%s=%d" % kv for kv in r[4].items())) for r in TABLE])
def test_table(start, m, n, span, knobs, want):
    p = plan(m, n, start, span, **knobs)
    if want is None:
        assert p["status"] == UNSUPPORTED, p
        return
    assert p["status"] == OK, p
    got = {k: p[k] for k in want}
    assert got == want, (start, m, n, span, knobs, p)
    assert p["blocked"] == (p["pipeline"] == BLOCKED) and p["use_tab"] == (p["pipeline"] >= TABLEAU)
    assert p["gen_start"] == p["needs_host_A"] == (start != "slack")


def test_search_on_device_follows_general_min_rows():
    assert plan(95, 200, "searched")["search_on_device"] == 0 and plan(96, 200, "searched")["search_on_device"] == 1
    assert plan(95, 200, "searched")["art_on_device"] == 0 and plan(96, 200, "searched")["art_on_device"] == 1
    assert plan(95, 200, "searched", general_min_rows=95)["search_on_device"] == 1
    assert plan(96, 200, "searched", general_min_rows=97)["search_on_device"] == 0
    p = plan(96, 200, "searched", general_device=0)   # (the artificial column follows the row count alone)
    assert p["search_on_device"] == 0 and p["art_on_device"] == 1
    assert plan(96, 200, "slack")["art_on_device"] == 0


def test_replay_up_to_64_rows():
    assert plan(64, 200)["replay_if_feasible"] == 1 and plan(65, 200)["replay_if_feasible"] == 0
    assert plan(64, 200)["cguard"] == 0.0 and plan(65, 200)["cguard"] == 1e-9
    assert plan(64, 200, "searched")["replay_if_feasible"] == 1
    assert plan(64, 200, "supplied")["replay_if_feasible"] == 0
    assert plan(64, 200, cond_guard=0)["replay_if_feasible"] == 0 and plan(65, 200, cond_guard=0)["cguard"] == 0.0


def test_exact_steps_up_to_256_rows():
    assert plan(256, 1280)["pipeline"] == BLOCKED and plan(257, 1285)["pipeline"] == THREE
    assert plan(256, 1280)["guard"] == 1e-9 and plan(257, 600)["guard"] == 0.0 and plan(257, 600)["pipeline"] == BLOCKED
    assert plan(257, 600, scale_span=1e9)["guard"] == 0.0 and plan(257, 600, scale_span=1.0001e9)["guard"] == 1e-9


def test_keys_and_shapes_are_checked():
    for bad in (dict(no_such_knob=1), dict(chunk=32), dict(lu_blocked=1), dict(exact_degenerate=4), dict(exact_degenerate=-1)):
        with pytest.raises(ValueError):
            plan(8, 20, **bad)
    for m, n in ((0, 4), (8, 8), (9, 8)):   # m == n and m > n are answered before any routing
        with pytest.raises(ValueError):
            plan(m, n)
