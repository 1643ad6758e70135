"""The compressed LU rounds of the final solve for bases of 4097 .. 16384 rows (context knob lu_large, off by default): eight workgroups
of one XCD, four (up to 8192 rows) or eight rows per lane (lu_cross.hip k_luc_panel_x<8, 4 or 8, ..>), plain schedule — against one launch per column
(lu_blocked = 0), which tests/test_gpu_revised_reference.py pins to the reference at these sizes.  Bar: identical status and positional
basis, x and z BIT-IDENTICAL, no fall-back (stats.device_retries == 0).

Problems: min c^T x  s.t.  G x <= h, x >= 0 as [G | I], G in {0, 1, 2}, h = 2 * rowsum + 1 (the construction of
tests/test_gpu_large_rows.py): the first dense column already has many rows tied at |a| = 2, so the pivot search's tie path (the replay
of the interchanges from the log of pivot rows, the exchange of logical positions) runs.  The number of cost columns sets how many
structural columns end up basic, and with them the steps that do arithmetic (about three per structural column)."""
import functools

import numpy as np
import pytest

from gomilp_amd import lp, synth
from tests.test_gpu_large_rows import _certify

pytestmark = pytest.mark.gpu

# m: (structural columns, cost columns) — tuned on the device so that every case has lu_rounds >= 4 and 128 <= lu_dense_steps < m
# (measured rounds / dense steps: 4097 7 / 210, 8192 9 / 273, 8193 9 / 176, 12288 8 / 173; beyond 8192 rows the pivot loop is the
# three-kernel revised simplex at 0.4 - 0.7 ms per pivot, so fewer cost columns there)
SHAPES = {4097: (512, 128), 8192: (256, 128), 8193: (256, 64), 12288: (256, 64)}
NV_END = 64   # the cases that only bracket the range (16384 / 16385 rows)


def _gen(m, nv, ncost, seed=0):
    rng = np.random.default_rng(77000 + 31 * m + seed)
    G = rng.integers(0, 3, (m, nv), dtype=np.int8)
    h = 2.0 * G.sum(axis=1, dtype=np.int64) + 1.0
    c = np.zeros(nv + m)
    cols = rng.choice(nv, ncost, replace=False)
    c[cols] = -rng.integers(1, 10, ncost).astype(float)
    A = np.zeros((m, nv + m))
    A[:, :nv] = G
    A[np.arange(m), nv + np.arange(m)] = 1.0
    return c, A, h


@functools.lru_cache(maxsize=1)
def _problem(m):
    nv, ncost = SHAPES[m]
    return _gen(m, nv, ncost)


def _solve(c, A, b, reps=1, **knobs):
    cx = lp.Context(**knobs)
    try:
        rl = cx.upload(c, A, b)
        out = [rl.solve(0.0) for _ in range(reps)]
        rl.free()
    finally:
        cx.close()
    return out if reps > 1 else out[0]


def _same(got, want):
    assert got.status == want.status == lp.OK, (got.status, want.status)
    assert np.array_equal(got.basis, want.basis)
    assert got.x.tobytes() == want.x.tobytes() and np.float64(got.z).tobytes() == np.float64(want.z).tobytes()
    assert got.stats["device_retries"] == 0 and want.stats["device_retries"] == 0


def _note(label, g):
    print("%s: pipeline %s, pivots %d, lu_rounds %d, lu_dense_steps %d, final solve %.4f s (device %.4f, host %.4f)" % (
        label, g.stats["pipeline"], g.stats["pivots_phase2"], g.stats["lu_rounds"], g.stats["lu_dense_steps"],
        g.stats["seconds_final_solve"], g.stats["seconds_final_device"], g.stats["seconds_final_host"]))


_per_column = {}


def _reference(m):
    """One launch per column (lu_blocked = 0) on the LP of size m: computed once, never changed."""
    if m not in _per_column:
        _per_column[m] = _solve(*_problem(m), lu_blocked=0)
        _note("m %d per column" % m, _per_column[m])
        assert _per_column[m].stats["lu_rounds"] == 0
    return _per_column[m]


def _rounds_ran(g, m):
    assert g.stats["lu_rounds"] >= 4, g.stats["lu_rounds"]
    assert 128 <= g.stats["lu_dense_steps"] < m, g.stats["lu_dense_steps"]


@pytest.mark.parametrize("m", [4097, 8192, 8193, 12288])
def test_large_rounds_equal_the_per_column_lu_bitwise(m):
    """4097: the first size, four rows per lane, workgroup 4 holds one row.  8192: four rows per lane, full.  8193: the first size with
    eight rows per lane (one row in workgroup 4).  12288: every register row of the eight is live, workgroups 6 and 7 are empty."""
    want = _reference(m)
    got = _solve(*_problem(m), lu_large=1)
    _note("m %d lu_large" % m, got)
    _same(got, want)
    _rounds_ran(got, m)


def test_dense_4097_rows_in_both_schedule_knob_values():
    """The LP of the 4097-row test of tests/test_gpu_revised_reference.py (real data: no ties, thousands of dense steps): lu_blocked = 2
    and the default 3 name the same plain schedule beyond 4096 rows — same bits, same rounds."""
    c, A, b = synth.dense_lp_standard_form(4097, 5)
    two = _solve(c, A, b, lu_large=1, lu_blocked=2)
    _note("dense 4097 lu_blocked 2", two)
    three = _solve(c, A, b, lu_large=1)
    _note("dense 4097 lu_blocked 3", three)
    _same(three, two)
    assert two.stats["lu_rounds"] > 0 and three.stats["lu_rounds"] == two.stats["lu_rounds"]
    assert three.stats["lu_dense_steps"] == two.stats["lu_dense_steps"]


def test_upper_end_16384_rows():
    """The upper end of the range: the replicated maps at their full size (147,456 bytes of LDS), eight full workgroups.  No per-column
    run at this size: status, rounds, and the optimality certificate of tests/test_gpu_large_rows.py."""
    m = 16384
    c, A, b = _gen(m, NV_END, 48)
    g = _solve(c, A, b, lu_large=1)
    _note("m %d lu_large" % m, g)
    assert g.status == lp.OK, lp.STATUS_NAMES.get(g.status, g.status)
    assert g.stats["lu_rounds"] > 0 and g.stats["device_retries"] == 0
    _certify(c, A, b, g, NV_END)


def test_three_solves_on_one_context_give_the_same_bits():
    """The exchange records' sequence numbers go on from launch to launch and from solve to solve."""
    m = 4097
    want = _reference(m)
    out = _solve(*_problem(m), reps=3, lu_large=1)
    for r in out:
        _same(r, want)
        _rounds_ran(r, m)
        assert r.stats["lu_rounds"] == out[0].stats["lu_rounds"] and r.stats["lu_dense_steps"] == out[0].stats["lu_dense_steps"]


def test_default_knobs_stay_on_the_per_column_lu():
    m = 4097
    default = _solve(*_problem(m))
    assert default.stats["lu_rounds"] == 0
    _same(default, _reference(m))
    large = _solve(*_problem(m), lu_large=1)
    _same(large, default)
    assert large.stats["lu_rounds"] > 0


@pytest.mark.parametrize("blocked", [0, 1])
def test_lu_large_needs_the_compressed_schedule(blocked):
    """lu_large names a panel of the compressed rounds: with lu_blocked = 0 / 1 (one launch per column / the blocked LU, which ends at
    4096 rows) no round runs."""
    m = 4097
    g = _solve(*_problem(m), lu_large=1, lu_blocked=blocked)
    assert g.stats["lu_rounds"] == 0
    _same(g, _reference(m))


def test_beyond_the_range_no_rounds():
    m = 16385
    c, A, b = _gen(m, NV_END, 48)
    g = _solve(c, A, b, lu_large=1)
    _note("m %d lu_large" % m, g)
    assert g.status == lp.OK, lp.STATUS_NAMES.get(g.status, g.status)
    assert g.stats["lu_rounds"] == 0


def test_pool_keeps_its_workers_off_the_large_panel():
    """A pool accepts the knob and leaves it at 0 on its workers: 32 children (520 rows) of the 512-row frontier root, as without it."""
    from tests.test_gpu_golden import _load
    fx = _load("frontier_C5.npz")
    m, seed = synth.CONFIGS["C5"]
    c, A, b = synth.dense_lp_standard_form(m, seed)
    children = synth.frontier_children(fx["root_x"], synth.integrality_mask(m, m), int(fx["nvars"]))[:32]
    res = []
    for knobs in ({}, {"lu_large": 1}):
        pool = lp.FrontierPool(workers=4, **knobs)
        try:
            pool.set_root(c, A, b)
            res.append(pool.solve(children))
        finally:
            pool.close()
    a, g = res
    assert np.array_equal(a.status, g.status) and np.array_equal(a.has_x, g.has_x)
    assert a.z.tobytes() == g.z.tobytes() and a.x.tobytes() == g.x.tobytes()
    assert np.array_equal(g.status, fx["status"][:32])
