"""The host half of the bit-exact final solve (gomilp_amd/csrc/lu_host.cpp: Dlaswp and the two Dtrsm of Dgetrs on the packed factors,
and LU.Det() == 0) against the oracle's SolveVec, bit for bit — host-only entry of the library, no GPU needed."""
import ctypes as C

import numpy as np

SIZES = [1, 2, 3, 4, 5, 6, 7, 8, 9, 31, 33, 64, 65, 100, 130]


def _case(seed):
    rng = np.random.default_rng(7000 + seed)
    m = SIZES[seed % 15]
    kind = (seed // 15) % 5
    A = rng.standard_normal((m, m))
    b = rng.standard_normal(m)
    if kind in (1, 2):      # slack columns of a basis: unit vectors in distinct rows
        k = m // 2 if kind == 1 else (9 * m) // 10
        cols, rows = rng.choice(m, k, replace=False), rng.choice(m, k, replace=False)
        A[:, cols] = 0.0
        A[rows, cols] = 1.0
    elif kind == 3:         # determinants that underflow
        A *= 10.0 ** -int(rng.integers(5, 40))
    elif kind == 4 and m > 1:
        A[:, -1] = A[:, 0]
    return m, np.ascontiguousarray(A), b


def test_host_solve_of_packed_factors_is_gonums_solvevec_bit_for_bit():
    """300 bases of 1..130 rows (beyond 64 the oracle's Dgetrf blocks): random, with half / nine tenths of the columns unit vectors
    (most elimination steps do no arithmetic: nd < m), scaled until Det() underflows, with two equal columns.  The packed factors —
    the row permutation, the list dl of columns of the in-place L\\U with off-diagonal entries, the diagonal and those columns by
    physical row (or, coupled form, the nd x nd part at the positions dl) — are built here from the oracle's own Dgetrf, so what is
    compared is the order of the rounded operations in the solves: the same Det() == 0 verdict on every case, the same doubles in
    x (full form) and in x[dl] (coupled form) wherever the basis is not singular."""
    from gomilp_amd import lp
    from oracle import oracle as O
    L = O.lib()
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int64)
    singular = partial = full = 0
    res_rest, res_nd = set(), set()
    for seed in range(300):
        m, A, b = _case(seed)
        want = b.copy()
        rc = L.g_solve_vec(m, A.ctypes.data_as(dp), m, want.ctypes.data_as(dp))
        assert rc in (0, 1, 2), (seed, rc)   # 1: the condition warning, the solution is returned all the same
        LU = A.copy()
        ipiv = np.zeros(m, dtype=np.int64)
        L.g_dgetrf(m, m, LU.ctypes.data_as(dp), m, ipiv.ctypes.data_as(ip))
        phys = np.arange(m)
        for i in range(m):
            phys[[i, ipiv[i]]] = phys[[ipiv[i], i]]
        off = LU - np.diag(np.diag(LU))
        dl = np.flatnonzero((off != 0).any(axis=0))
        nd = dl.size
        diag = np.zeros(m)
        diag[phys] = np.diag(LU)
        W = np.zeros((m, nd))
        W[phys] = LU[:, dl]
        x, sing = lp.debug_lu_host_solve(dl, phys, diag, W, b)
        xdu, sing2 = lp.debug_lu_host_solve(dl, phys, diag, LU[np.ix_(dl, dl)], b, coupled=True)
        assert sing == sing2 == (rc == 2), (seed, m, rc, sing, sing2)
        singular += int(sing)
        partial += int(nd < m)
        full += int(nd == m)
        res_rest.add((m - nd) % 4)
        res_nd.add(nd % 4)
        if sing:
            continue
        assert np.array_equal(x.view(np.uint64), want.view(np.uint64)), (seed, m, nd)
        assert np.array_equal(xdu.view(np.uint64), want[dl].view(np.uint64)), (seed, m, nd)
    print("singular %d, nd < m %d, nd == m %d" % (singular, partial, full))
    assert singular >= 20 and partial >= 100 and full >= 100
    assert res_rest == {0, 1, 2, 3} and res_nd == {0, 1, 2, 3}
