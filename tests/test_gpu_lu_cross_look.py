"""The 32-slot cross-workgroup LU panel of the final solve (lu_cross.hip, knob lu_cross = 2) — in the plain schedule and as the panel
role of the look-ahead launch (luc_role.h), the default for bases of 1281 .. 2048 rows — against the schedules it replaces.  Bar: identical
status and basis, x and z BIT-IDENTICAL, the same dense steps, no fall-back (stats.device_retries == 0)."""
import importlib.util
import os
import threading

import numpy as np
import pytest

from gomilp_amd import lp, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (rows, seed): just above the look-ahead threshold (4 workgroups) / the first size on 8 workgroups, with padded rows / the size at which the
# look-ahead's ordering bug once showed / the metric LP (full)
SIZES = [(770, 3), (1025, 3), (1100, 3), (2048, 2)]

_problems = {}


def _problem(m, seed):
    if (m, seed) not in _problems:
        _problems[(m, seed)] = synth.dense_lp_standard_form(m, seed)
    return _problems[(m, seed)]


def _solve(c, A, b, reps=1, **knobs):
    cx = lp.Context(**knobs)
    try:
        rl = cx.upload(c, A, b)
        out = [rl.solve(0.0) for _ in range(reps)]
        rl.free()
    finally:
        cx.close()
    return out if reps > 1 else out[0]


def _same(got, want, dense=True):
    assert got.status == want.status == lp.OK, (got.status, want.status)
    assert np.array_equal(got.basis, want.basis)
    assert np.array_equal(got.x, want.x) and got.z == want.z   # (array_equal on doubles: the same bits, no NaN in an optimal x)
    if dense:   # (one launch per column counts every step: the steps that did arithmetic are compared among the compressed schedules)
        assert got.stats["lu_dense_steps"] == want.stats["lu_dense_steps"]
    assert got.stats["device_retries"] == 0


_per_column = {}


def _reference(m, seed):
    """One launch per column (lu_blocked = 0), which the small cases pin to the oracle: computed once per size."""
    if (m, seed) not in _per_column:
        _per_column[(m, seed)] = _solve(*_problem(m, seed), lu_blocked=0)
    return _per_column[(m, seed)]


@pytest.mark.parametrize("m,seed", SIZES)
def test_default_final_solve_equals_per_column_lu_bitwise(m, seed):
    """Default knobs, and the 32-slot cross-workgroup panel inside the look-ahead launch (forced below the default's range: 4 workgroups
    at 770 rows, 8 with padded rows at 1025), against one launch per column; at the metric size the default takes strictly fewer rounds than
    the one-workgroup panel (16 slots at 2048 rows)."""
    want = _reference(m, seed)
    got = _solve(*_problem(m, seed))
    print("m %d: rounds %d dense steps %d final %.3f ms" % (m, got.stats["lu_rounds"], got.stats["lu_dense_steps"], 1e3 * got.stats["seconds_final_solve"]))
    _same(got, want, dense=False)
    assert got.stats["lu_rounds"] > 0
    one = _solve(*_problem(m, seed), lu_cross=0)   # the one-workgroup panel in the same schedule
    print("m %d: rounds %d with lu_cross = 0" % (m, one.stats["lu_rounds"]))
    _same(one, want, dense=False)
    _same(got, one)
    forced = _solve(*_problem(m, seed), lu_cross=2)   # (lu_blocked = 3 is the default: the look-ahead launch)
    _same(forced, one)
    assert forced.stats["lu_rounds"] > 0
    if m == 2048:
        assert got.stats["lu_rounds"] < one.stats["lu_rounds"] and forced.stats["lu_rounds"] == got.stats["lu_rounds"]


@pytest.mark.parametrize("m,seed", SIZES)
def test_32_slot_cross_panel_in_the_plain_schedule_equals_the_one_workgroup_panel_bitwise(m, seed):
    one = _solve(*_problem(m, seed), lu_cross=0, lu_blocked=2)
    got = _solve(*_problem(m, seed), lu_cross=2, lu_blocked=2)
    _same(got, one)
    _same(one, _reference(m, seed), dense=False)
    assert got.stats["lu_rounds"] > 0


def _lu_ties():
    spec = importlib.util.spec_from_file_location("lu_ties", os.path.join(ROOT, "tools", "lu_ties.py"))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("m", [150, 300])
def test_32_slot_cross_panel_where_the_pivot_search_ties(m):
    """Integer data: most pivot searches tie, so the replay of the interchanges from the log of pivot rows and the third exchange run with
    the 37-slot records (forced: these bases are below the default's range)."""
    c, A, b = _lu_ties().integer_lp(m, 0)
    one = _solve(c, A, b, lu_cross=0, lu_blocked=2, max_pivots=20000)
    got = _solve(c, A, b, lu_cross=2, lu_blocked=2, max_pivots=20000)
    _same(got, one)
    assert got.stats["lu_rounds"] > 0


def test_repeated_solves_on_one_context_give_the_same_bits():
    """The exchange records' sequence numbers and the arrival counters go on from launch to launch and from solve to solve."""
    m, seed = 1100, 3
    want = _reference(m, seed)
    out = _solve(*_problem(m, seed), reps=3, lu_cross=2)
    for r in out:
        _same(r, want, dense=False)
        _same(r, out[0])


def test_two_contexts_on_two_threads_give_the_single_threaded_bits():
    """Only one engine can hold the device's loop slots: the other's final solve takes the same panel in the plain schedule."""
    m, seed = 1100, 3
    c, A, b = _problem(m, seed)
    want = _reference(m, seed)
    out, err = {}, []

    def work(i):
        try:
            out[i] = _solve(c, A, b, reps=3, lu_cross=2)
        except BaseException as e:   # noqa: BLE001 (reported by the asserting thread)
            err.append(e)

    ts = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not err, err
    for i in range(2):
        for r in out[i]:
            _same(r, want, dense=False)
            _same(r, out[0][0])
            assert r.stats["lu_rounds"] == out[0][0].stats["lu_rounds"]
