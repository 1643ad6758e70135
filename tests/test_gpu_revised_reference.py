"""The revised-simplex pipelines and the per-column final solve against the reference, at the sizes where they are the default.

A. The fused and three-kernel pipelines (one-pass and chunked staging, knob row_chunk) on the committed oracle fixtures C2, M and C4,
   forced with knobs, at the bar of the tableau runs in tests/test_gpu_golden.py: every pivot, the positional basis, x and z bits.
   Since the one-pass and chunked kernels share one pivot body, the chunked-vs-one-pass identity of tests/test_gpu_large_rows.py cannot
   catch a wrong pivot rule; these runs can.
B. Beyond 4096 rows the compressed and blocked LU schedules do not run: the final x_B comes from k_lu_init / k_lu_step / k_lu_pack and
   the host triangular solves.  The bar is independent of the pivot path: the engine's status, and x and z bit for bit equal to the
   reference's solve of the engine's own positional basis (oracle.basis_solve, simplex.go:288-300).  It holds on the degenerate integer
   family too, where the revised pipelines may reach the optimum by another path than the reference's."""
import time

import numpy as np
import pytest

from gomilp_amd import lp, synth
from oracle import oracle as O
from tests.test_gpu_golden import _check_C4_against_fixtures, _check_lp_against_fixture, _load
from tests.test_gpu_large_rows import _gen

pytestmark = pytest.mark.gpu

ORACLE_THREADS = 16

REVISED = {"fused": dict(tableau=0, fused=1), "three-kernel": dict(tableau=0, fused=0),
           "chunk-512": dict(tableau=0, fused=0, row_chunk=512), "chunk-1536": dict(tableau=0, fused=0, row_chunk=1536)}


def _expected(pipe):
    return "fused" if pipe == "fused" else "three-kernel"


# ---- A. revised pipelines against the oracle fixtures --------------------------------------------------------------------------------

@pytest.mark.parametrize("pipe", list(REVISED))
@pytest.mark.parametrize("name", ["C2", "M"])
def test_revised_pipelines_match_the_oracle_fixture(name, pipe):
    """C2 (1024 x 2048, 1261 pivots) and M (2048 x 4096, 2936 pivots): row_chunk 512 gives 2 and 4 full chunks, 1536 a partial last one"""
    t = time.time()
    r = _check_lp_against_fixture(lp, synth, name, _load("lp_%s.npz" % name), **REVISED[pipe])
    print("%s %s: pipeline %s, %d pivots, %.2f s" % (name, pipe, r.stats["pipeline"], len(r.pivots), time.time() - t))
    assert r.stats["pipeline"] == _expected(pipe)


@pytest.mark.parametrize("pipe", ["fused", "three-kernel", "chunk-1536"])
def test_revised_pipelines_match_the_C4_fixtures(pipe):
    """C4 (4096 x 8192): the 1000-pivot prefix, 2750 continuation pairs, the end basis and the x / z bits of the end state"""
    t = time.time()
    r = _check_C4_against_fixtures(lp, synth, O, **REVISED[pipe])
    print("C4 %s: pipeline %s, %d pivots, %.2f s" % (pipe, r.stats["pipeline"], len(r.pivots), time.time() - t))
    assert r.stats["pipeline"] == _expected(pipe)


# ---- B. the per-column final solve beyond 4096 rows against the reference's solve of the same basis ----------------------------------

def _first_diff(got, want):
    i = int(np.argmax(got.view(np.int64) != want.view(np.int64)))
    return "x bits differ first at %d: %r vs %r (%d ulps)" % (i, got[i], want[i], int(got.view(np.int64)[i]) - int(want.view(np.int64)[i]))


def _against_basis_solve(label, c, A, b, g, pipeline, status=lp.OK):
    """status, pipeline, the per-column schedule (no compressed rounds), x and z bits of the reference's solve of g's basis"""
    assert g.status == status, lp.STATUS_NAMES.get(g.status, g.status)
    assert g.stats["pipeline"] == pipeline
    assert A.shape[0] > 4096 and g.stats["lu_rounds"] == 0
    O.set_threads(ORACLE_THREADS)
    t = time.time()
    s = O.basis_solve(c, A, b, g.basis)
    dt = time.time() - t
    print("%s: m %d n %d, pipeline %s, pivots %d + %d, drift_xb %.3g, final solve %.3f s; oracle basis_solve %.1f s (cond %.3g)" % (
        label, A.shape[0], A.shape[1], g.stats["pipeline"], g.stats["pivots_phase1"], g.stats["pivots_phase2"], g.stats["drift_xb"],
        g.stats["seconds_final_solve"], dt, s.cond))
    assert s.status == O.OK and not s.singular
    assert g.x.tobytes() == s.x.tobytes(), _first_diff(g.x, s.x)
    assert np.float64(g.z).tobytes() == np.float64(s.z).tobytes(), (g.z, s.z)
    return s


def _restart_pivots(label, c, A, b, g):
    """the oracle restarted from the engine's basis, at most one pivot: 0 = the reference's pricing calls the basis optimal too
    (printed only: on integer data the engine may stop on another optimal basis)"""
    t = time.time()
    o = O.simplex(c, A, b, 0.0, np.asarray(g.basis, dtype=np.int64), stop_after_pivots=1)
    print("%s: the oracle restarted from the engine's basis takes %s pivots (%.1f s)" % (
        label, "0" if o.pivots_phase2 == 0 else ">= 1", time.time() - t))


@pytest.mark.parametrize("pipe", ["default", "three-kernel"])
def test_dense_4097_rows_final_solve_and_stop_test(pipe):
    """the first size past the compressed / blocked LU: blocked tableau (default) and three-kernel.  Also the stop test: the oracle
    restarted from the engine's basis takes no pivot and returns the same bits"""
    c, A, b = synth.dense_lp_standard_form(4097, 5)
    cx = lp.Context(**({} if pipe == "default" else REVISED[pipe]))
    try:
        g = cx.upload(c, A, b).solve(0.0)
    finally:
        cx.close()
    _against_basis_solve("dense 4097 " + pipe, c, A, b, g, "blocked" if pipe == "default" else "three-kernel")
    t = time.time()
    o = O.simplex(c, A, b, 0.0, np.asarray(g.basis, dtype=np.int64))
    print("dense 4097 %s: oracle restart %.1f s" % (pipe, time.time() - t))
    assert o.status == O.OK and o.pivots_phase1 == 0 and o.pivots_phase2 == 0
    assert o.x.tobytes() == g.x.tobytes() and np.float64(o.z).tobytes() == np.float64(g.z).tobytes()


@pytest.mark.parametrize("m", [8192, 8193])
def test_integer_final_solve_at_the_one_pass_boundary(m):
    """8192 rows: the last size of the one-pass kernels; 8193: the first chunked one.  Integer data: ties in k_lu_step's pivot search
    across workgroup partials"""
    c, A, b = _gen(m, 2 * m, 0)
    g = lp.simplex(c, A, b, 0.0, None)
    _against_basis_solve("integer %d" % m, c, A, b, g, "three-kernel")
    _restart_pivots("integer %d" % m, c, A, b, g)


def test_phase1_final_solve_beyond_the_lds_window():
    c, A, b = _gen(8200, 16400, 1, "phase1")
    g = lp.simplex(c, A, b, 0.0, None)
    assert g.stats["phase1_used"] == 1
    _against_basis_solve("phase I 8200", c, A, b, g, "three-kernel")
    _restart_pivots("phase I 8200", c, A, b, g)


def test_device_child_final_solve_beyond_the_lds_window():
    """one branch row on the 8200-row root, the child assembled on the device (upload_child), against the reference's solve of the
    child's standard form (subproblem.go:55-78) on the engine's basis"""
    m, nv = 8200, 16400
    c0, A0, b0 = _gen(m, nv, 0)
    cx = lp.Context()
    try:
        root = cx.upload(c0, A0, b0)
        r = root.solve(0.0)
        assert r.status == lp.OK
        xs = r.x[:nv]
        j = int(np.argmax(xs))
        assert xs[j] > 0
        cons = [(j, 1.0, float(np.floor(xs[j] / 2)))]   # a bound that cuts the root's point off
        ch = root.child(cons)
        g = ch.solve(0.0)
        ch.free()
        root.free()
    finally:
        cx.close()
    cc, AA, bb = O.child_standard_form(c0, A0, b0, cons)
    _against_basis_solve("child %s" % (cons,), cc, AA, bb, g, "three-kernel")
    _restart_pivots("child", cc, AA, bb, g)


def test_narrow_12288_rows_final_solve():
    """12288 rows, n - m = m / 2: the largest factorization the suite asks of the oracle"""
    c, A, b = _gen(12288, 6144, 0)
    g = lp.simplex(c, A, b, 0.0, None)
    _against_basis_solve("narrow 12288", c, A, b, g, "three-kernel")
