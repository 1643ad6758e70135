"""CPU tests of the oracle's building blocks (no GPU): fast-path equivalence, LU blocking, generator."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from gomilp_amd import synth
from oracle import oracle as O


def test_splitmix64_reference_values():
    # splitmix64(seed=0): first outputs of the published reference implementation
    u = synth.splitmix64_uniform(0, 3)
    first = [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    assert [int(x * 2 ** 53) for x in u] == [v >> 11 for v in first]


def test_generator_shapes_and_structure():
    c, A, b = synth.dense_lp_standard_form(8, 3)
    assert A.shape == (8, 16) and c.shape == (16,) and b.shape == (8,)
    assert np.array_equal(A[:, 8:], np.eye(8)) and np.all(c[8:] == 0) and np.all(c[:8] <= 0)
    assert np.all((A[:, :8] >= 0) & (A[:, :8] < 1)) and np.all((b >= 1) & (b < 2))


@pytest.mark.parametrize("m,seed", [(5, 1), (12, 2), (40, 3), (96, 4)])
def test_unit_column_fast_path_is_equivalent(m, seed):
    """findLinearlyIndependent's cond test (simplex.go:630) is == 1 on distinct unit columns, so skipping it
    must not change anything: same basis, same pivots, same bits."""
    c, A, b = synth.dense_lp_standard_form(m, seed)
    full = O.simplex(c, A, b, 0.0, None, trace=True)
    fast = O.simplex(c, A, b, 0.0, None, trace=True, fast_initial_basis=True)
    assert full.cond_evaluations == m - 1 and fast.cond_evaluations == 0
    assert full.status == fast.status == O.OK
    assert full.pivots == fast.pivots
    assert np.array_equal(full.x, fast.x) and full.z == fast.z
    assert O.find_linearly_independent(A) == O.find_linearly_independent(A, fast=True) == list(range(2 * m - 1, m - 1, -1))


def test_unit_columns_have_cond_one():
    rng = np.random.default_rng(0)
    m = 30
    perm = rng.permutation(m)
    for k in (2, 7, 30):
        cols = np.zeros((m, k))
        cols[perm[:k], np.arange(k)] = 1.0
        assert O.cond1(cols) == 1.0


def test_blocked_lu_equals_unblocked_bitwise():
    """dgetrf.go (nb = 64 panels + Dtrsm + Dgemm) and dgetf2.go give the same bits."""
    L = O.lib()
    rng = np.random.default_rng(7)
    n = 150
    A = rng.standard_normal((n, n))
    a1, a2 = A.copy(), A.copy()
    p1, p2 = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int64)
    L.g_dgetrf(n, n, a1.ctypes.data_as(dp), n, p1.ctypes.data_as(ip))
    L.g_dgetf2(n, n, a2.ctypes.data_as(dp), n, p2.ctypes.data_as(ip))
    assert np.array_equal(p1, p2) and np.array_equal(a1, a2)


def test_threads_do_not_change_results():
    c, A, b = synth.dense_lp_standard_form(150, 9)
    O.set_threads(1)
    r1 = O.simplex(c, A, b, 0.0, None, fast_initial_basis=True)
    O.set_threads(4)
    r4 = O.simplex(c, A, b, 0.0, None, fast_initial_basis=True)
    O.set_threads(1)
    assert np.array_equal(r1.x, r4.x) and r1.z == r4.z and r1.pivots_phase2 == r4.pivots_phase2


def test_solve_matches_numpy():
    L = O.lib()
    rng = np.random.default_rng(3)
    dp = C.POINTER(C.c_double)
    for n in (1, 2, 17, 80):
        A = rng.standard_normal((n, n)) + n * np.eye(n)
        b = rng.standard_normal(n)
        x = b.copy()
        assert L.g_solve_vec(n, A.ctypes.data_as(dp), n, x.ctypes.data_as(dp)) == 0
        assert np.allclose(x, np.linalg.solve(A, b), rtol=1e-10, atol=1e-12)
        xt = b.copy()
        assert L.g_solve_vec_trans(n, A.ctypes.data_as(dp), n, xt.ctypes.data_as(dp)) == 0
        assert np.allclose(xt, np.linalg.solve(A.T, b), rtol=1e-10, atol=1e-12)


def test_cond_estimates_are_sane():
    rng = np.random.default_rng(5)
    for shape in ((20, 20), (40, 13), (300, 200)):   # square -> LU path; tall -> QR (300x200 takes the blocked Dgeqrf)
        A = rng.standard_normal(shape)
        est = O.cond1(A)
        if shape[0] == shape[1]:
            true = np.linalg.cond(A, 1)
        else:
            R = np.linalg.qr(A, mode="r")
            true = np.linalg.cond(R, 1)
        assert true / 10 <= est <= true * 1.0001, (shape, est, true)
    A = rng.standard_normal((30, 5))
    A[:, 4] = A[:, 0] + A[:, 1]
    assert O.cond1(A) > 1e12


def test_error_returns_follow_reference_conventions():
    # unbounded via verifyInputs: zero column with negative cost -> (-Inf, nil, ErrUnbounded)  simplex.go:96-98
    r = O.simplex([-1.0, 0.0, 0.0], [[0.0, 1.0, 1.0]], [1.0])
    assert r.status == O.ERR_UNBOUNDED and r.z == -math.inf and r.x is None
    r = O.simplex([1.0, 0.0, 0.0], [[0.0, 1.0, 1.0]], [1.0])
    assert r.status == O.ERR_ZERO_COLUMN and math.isnan(r.z) and r.x is None
    r = O.simplex([1.0, 0.0], [[0.0, 0.0], [1.0, 1.0]], [0.0, 1.0])
    assert r.status == O.ERR_ZERO_ROW
    r = O.simplex([1.0, 0.0], [[0.0, 0.0], [1.0, 1.0]], [1.0, 1.0])
    assert r.status == O.ERR_INFEASIBLE
    # size mismatch panics in the reference (simplex.go:387-398)
    r = O.simplex([1.0], [[1.0, 1.0]], [1.0])
    assert r.status == O.ERR_BAD_SHAPE


def test_bnb_child_layout_matches_convert_to_equalities():
    """subproblem_test.go:296-357 pins [[A,0],[G,I]]; children add ±e_j rows (subproblem.go:245-255)."""
    c0 = np.array([1.0, 2.0, 0.0])
    A0 = np.array([[1.0, 1.0, 1.0]])
    b0 = np.array([4.0])
    c, A, b = O.child_standard_form(c0, A0, b0, [(1, 1, 2.0), (0, -1, -3.0)])
    assert np.array_equal(c, [1, 2, 0, 0, 0])
    assert np.array_equal(A, [[1, 1, 1, 0, 0], [0, 1, 0, 1, 0], [-1, 0, 0, 0, 1]])
    assert np.array_equal(b, [4, 2, -3])


def test_wide_degenerate_family_keeps_its_degeneracy():
    """synth.wide_degenerate_lp is the family of tests/test_gpu_wide.py: its point is Bland steps and ties on wide LPs.  Over the GPU
    test's roots the oracle takes Bland steps by the dozen, and on the cycling instances the reference's rule never ends (truncated by
    stop_after_pivots) — an edit that made the family non-degenerate would fail here first."""
    c, A, b = synth.wide_degenerate_lp(24, 0, 2.5)
    m, nv = 24, 60
    assert A.shape == (m, nv + m) and np.array_equal(A[:, nv:], np.eye(m)) and np.all(c[nv:] == 0)
    G = A[:, :nv]
    assert np.all(G == np.floor(G)) and G.min() >= 0 and G.max() <= 3 and G[0].min() >= 1
    assert np.all((b >= 1) & (b <= 8) & (b == np.floor(b))) and np.all((c[:nv] <= 0) & (c[:nv] >= -4))
    rows = {tuple(G[i]) + (b[i],) for i in range(m)}
    assert len(rows) <= m - m // 4 + 1          # ~m // 4 duplicated rows (equal right-hand sides)
    bland = 0
    for m_ in (8, 24, 48, 64, 96, 128):
        for ratio in (2, 2.5, 4):
            for seed in (0, 1):
                o = O.simplex(*synth.wide_degenerate_lp(m_, seed, ratio), 0.0, None, fast_initial_basis=True, stop_after_pivots=400)
                bland += o.bland_steps
    assert bland >= 40, bland
    cyc = O.simplex(*synth.wide_degenerate_lp(32, 11, 2.5), 0.0, None, fast_initial_basis=True, stop_after_pivots=400)
    assert cyc.truncated and cyc.pivots_phase2 == 400


# ---- basis_solve: the reference's end state on a given basis (the yardstick of tests/test_gpu_revised_reference.py) ----------------

def _fixture(name):
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name), allow_pickle=False)


@pytest.fixture
def oracle_threads():
    O.set_threads(min(16, os.cpu_count() or 1))
    yield
    O.set_threads(1)


@pytest.mark.parametrize("name,end", [("C2", "lp_C2.npz"), ("M", "lp_M.npz"), ("C4", "lp_C4_end.npz")])
def test_basis_solve_reproduces_the_fixture_end_states(oracle_threads, name, end):
    """one factorization of the fixture's final positional basis gives the x and z bits the oracle's own loop ended on (C2, M: the full
    solves; C4: the oracle restarted from the engine's final basis)"""
    fx = _fixture(end)
    c, A, b = synth.dense_lp_standard_form(*synth.CONFIGS[name])
    s = O.basis_solve(c, A, b, fx["basis"])
    assert s.status == O.OK and not s.singular and 1 <= s.cond < 1e16
    assert s.x.tobytes() == np.ascontiguousarray(fx["x"], dtype=np.float64).tobytes()
    assert np.float64(s.z).tobytes() == np.float64(fx["z"]).tobytes()


def _small_lps():
    from tests.test_gpu_large_rows import _gen
    return {"dense64": synth.dense_lp_standard_form(64, 11), "dense200": synth.dense_lp_standard_form(200, 12),
            "wide96": synth.wide_degenerate_lp(96, 0), "int256": _gen(256, 512, 0), "phase1-256": _gen(256, 512, 1, "phase1"),
            "wide512": synth.wide_degenerate_lp(512, 1)}


@pytest.mark.parametrize("name", ["dense64", "dense200", "wide96", "int256", "phase1-256", "wide512"])
def test_basis_solve_equals_the_restarted_oracle(oracle_threads, name):
    """64 to 512 rows (dense, wide degenerate integer, Phase I): the oracle restarted from the LP's own optimal basis takes no pivot, and
    basis_solve of that basis gives its x and z bits, which are also the bits of the solve that found the basis"""
    c, A, b = _small_lps()[name]
    o = O.simplex(c, A, b, 0.0, None, fast_initial_basis=True)
    assert o.status == O.OK
    r = O.simplex(c, A, b, 0.0, o.basis)
    assert r.status == O.OK and r.pivots_phase1 == r.pivots_phase2 == 0
    s = O.basis_solve(c, A, b, o.basis)
    assert s.status == O.OK and not s.singular
    assert s.x.tobytes() == r.x.tobytes() == o.x.tobytes()
    assert np.float64(s.z).tobytes() == np.float64(r.z).tobytes() == np.float64(o.z).tobytes()


def test_basis_solve_of_a_basis_that_is_not_optimal(oracle_threads):
    """the loop's point after k pivots (stop_after_pivots) is the solve of its basis at that moment: basis_solve does not price"""
    c, A, b = synth.dense_lp_standard_form(200, 12)
    for k in (1, 30):
        t = O.simplex(c, A, b, 0.0, None, fast_initial_basis=True, stop_after_pivots=k)
        assert t.truncated and t.pivots_phase2 == k
        s = O.basis_solve(c, A, b, t.basis)
        assert s.status == O.OK
        assert s.x.tobytes() == t.x.tobytes() and np.float64(s.z).tobytes() == np.float64(t.z).tobytes()


def test_basis_solve_singular_and_bad_bases():
    """Det() == 0 (the slack column of row 0 twice, so row 1 has no pivot): mat.Condition, x_B left at zero; an index out of range or a
    basis of the wrong length is refused"""
    c, A, b = synth.dense_lp_standard_form(16, 2)
    basis = np.arange(16, 32)
    basis[1] = basis[0]
    s = O.basis_solve(c, A, b, basis)
    assert s.status == O.ERR_CONDITION and s.singular
    assert not s.x.any() and s.z == 0.0
    ok = O.basis_solve(c, A, b, np.arange(16, 32))
    assert ok.status == O.OK and ok.cond == 1.0 and np.array_equal(ok.x[16:], b) and ok.z == 0.0
    with pytest.raises(ValueError):
        O.basis_solve(c, A, b, np.arange(17, 33))
    with pytest.raises(ValueError):
        O.basis_solve(c, A, b, np.arange(16, 31))
