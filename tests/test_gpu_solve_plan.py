"""Single solves go where SolvePlan says (gomilp_amd/csrc/engine.hpp; the table of DESIGN.md section 2.4, asserted row by row on the
host by tests/test_solve_plan.py): the rows of that table with m <= 300 solved on the device — stats["pipeline"] against the literal
and against the host probe, the refusals — and one Phase-I instance per Phase-I path (slack / searched start on the revised / tableau
pipelines, b with negative entries) against the live oracle through test_gpu_wide's _check: status, trace, pivots per phase, positional
basis, x and z bits."""
import functools

import numpy as np
import pytest

from gomilp_amd import lp, synth
from oracle import oracle as O
from tests.test_gpu_wide import _check

pytestmark = pytest.mark.gpu

# (start, m, n, scale_span, knobs, pipeline; None: GOMILP_ERR_UNSUPPORTED)
ROWS = [
    ("slack", 8, 20, 1.0, {}, "blocked"),
    ("slack", 8, 40, 1.0, {}, "blocked"),
    ("slack", 8, 40, 1.0, dict(exact_degenerate=0), "three-kernel"),
    ("slack", 8, 40, 1.0, dict(blocked=0), "three-kernel"),
    ("slack", 128, 512, 1.0, dict(exact_degenerate=0), "fused"),
    ("slack", 128, 512, 1.0, dict(exact_degenerate=0, fused=0), "three-kernel"),
    ("slack", 300, 700, 1.0, {}, "blocked"),
    ("slack", 300, 700, 1.0, dict(blocked=0), "tableau"),
    ("slack", 300, 700, 1.0, dict(tableau=0), "three-kernel"),
    ("slack", 300, 1500, 1.0, {}, "three-kernel"),
    ("slack", 300, 1500, 1e10, {}, "blocked"),
    ("slack", 300, 1500, 1.0, dict(exact_degenerate=2), "blocked"),
    ("slack", 300, 1500, 1.0, dict(exact_degenerate=3), "blocked"),
    ("slack", 300, 9000, 1.0, {}, "three-kernel"),
    ("slack", 300, 9000, 1.0, dict(exact_degenerate=3), None),
    ("searched", 8, 20, 1.0, {}, "blocked"),
    ("searched", 300, 9000, 1.0, dict(exact_degenerate=1), "three-kernel"),
    ("searched", 300, 9000, 1.0, dict(exact_degenerate=3), "three-kernel"),
    ("searched", 300, 9000, 1.0, dict(exact_degenerate=0), "three-kernel"),
    ("searched", 128, 8400, 1.0, {}, "three-kernel"),
]
PIPELINES = ["three-kernel", "fused", "tableau", "blocked"]   # lp.py _stats_dict
# strict mode decides every pivot of the 300-row searched basis on fresh solves, 11 ms each, and this LP takes 5938 of them: the route
# shows in the first ones (max_pivots is no routing knob: it bounds the loop the plan has chosen)
BUDGET = {"searched-300x9000-1-exact_degenerate=3": dict(max_pivots=64)}


def row_id(r):
    return "%s-%dx%d-%g-%s" % (r[0], r[1], r[2], r[3], ",".join("%s=%d" % kv for kv in r[4].items()))


@functools.lru_cache(maxsize=None)
def problem(start, m, n, span=1.0, negative=0, seed=1):
    """Random dense rows (synth.dense_lp_inequality_form).  slack: [G | I].  searched: the first m // 4 (at least 2) rows are equalities
    without a slack column — the descending scan meets a dense column and the solve searches its basis.  span > 1: one entry scaled so
    that the entries span more than nine decades.  negative: that many rows negated around a feasible point x0, their b below zero."""
    E = 0 if start == "slack" else max(2, m // 4)
    nv = n - (m - E)
    c, G, h = synth.dense_lp_inequality_form(m, seed, nv)
    if negative:
        u = synth.splitmix64_uniform(seed + 77, nv + m)
        x0, s0 = 4.0 * u[:nv] * (u[:nv] > 0.7), u[nv:]
        G[m - negative:] *= -1.0
        h = G @ x0 + np.concatenate([np.zeros(E), s0[E:]])
        assert (h[m - negative:] < 0).all()
    A = np.zeros((m, n))
    A[:, :nv] = G
    A[E + np.arange(m - E), nv + np.arange(m - E)] = 1.0
    if span > 1.0:
        A[0, 0] *= 1e-3 / span
    return np.concatenate([c, np.zeros(m - E)]), A, h.copy()


def run_knobs(row):
    return dict(row[4], **BUDGET.get(row_id(row), {}))


def solve(key, knobs, trace=False):
    c, A, b = problem(*key)
    cx = lp.Context(**knobs)
    try:
        return cx.upload(c, A, b).solve(0.0, trace=trace)
    finally:
        cx.close()


@pytest.mark.parametrize("row", ROWS, ids=row_id)
def test_pipeline_of_the_table(row):
    start, m, n, span, knobs, want = row
    p = lp.debug_solve_plan(m, n, start, span, **knobs)
    g = solve((start, m, n, span), run_knobs(row))
    if want is None:
        assert p["status"] == lp.ERR_UNSUPPORTED and g.status == lp.ERR_UNSUPPORTED and g.x is None
        return
    assert p["status"] == lp.OK and g.status != lp.ERR_DEVICE, lp.STATUS_NAMES.get(g.status)
    assert g.stats["pipeline"] == want == PIPELINES[p["pipeline"]], (g.stats["pipeline"], p)
    assert g.stats["pivots_phase1"] + g.stats["pivots_phase2"] > 0


# one per Phase-I path: (start, m, n, knobs, pipeline); from 96 rows on a searched start builds its artificial column on the device
PHASE1 = {
    "slack-revised": ("slack", 48, 240, dict(tableau=0), "three-kernel"),
    "slack-blocked": ("slack", 48, 120, {}, "blocked"),
    "slack-tableau": ("slack", 48, 120, dict(blocked=0), "tableau"),
    "searched-blocked": ("searched", 48, 120, {}, "blocked"),
    "searched-tableau": ("searched", 48, 120, dict(blocked=0), "tableau"),
    "searched-revised": ("searched", 48, 120, dict(tableau=0), "three-kernel"),
    "searched-blocked-96": ("searched", 96, 240, {}, "blocked"),
    "searched-revised-96": ("searched", 96, 240, dict(tableau=0), "three-kernel"),
}


def phase1_key(name):
    start, m, n = PHASE1[name][:3]
    return (start, m, n, 1.0, m // 3)


@functools.lru_cache(maxsize=None)
def phase1_oracle(key):
    c, A, b = problem(*key)
    O.set_threads(8)
    return O.simplex(c, A, b, 0.0, None, fast_initial_basis=True, trace=True)


@pytest.mark.parametrize("name", sorted(PHASE1))
def test_phase1_paths_against_the_oracle(name):
    key = phase1_key(name)
    knobs, want = PHASE1[name][3:]
    o = phase1_oracle(key)
    g = solve(key, knobs, trace=True)
    assert g.stats["pipeline"] == want and g.stats["phase1_used"] == 1
    assert o.status == O.OK and o.pivots_phase1 > 0, (O.STATUS_NAMES.get(o.status), o.pivots_phase1)
    _check(g, o, name)
