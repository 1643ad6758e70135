"""Relaxations of more than 8192 rows: the three-kernel revised simplex runs them, its kernels staging their m-long vector through
LDS in chunks (simplex_kernels.hip, the CK = true kernel instances).  Slack-basis starts of 8193 to 12288 rows through the flat call, the resident
upload and device-assembled children, checked by an optimality certificate computed here; the chunked form forced below 8192 rows
(context knob row_chunk) bit-identical to the one-pass form; and the shapes that stay refused.

Problems: min c^T x  s.t.  G x <= h, x >= 0 in GoMILP's standard form [G | I], G small non-negative integers, h = 2 * rowsum + 1
(the slack start is feasible), c non-zero on 48 structural columns (a few hundred pivots)."""
import functools

import numpy as np
import pytest

from gomilp_amd import lp, synth
from oracle import oracle as O

pytestmark = pytest.mark.gpu

NCOST = 48


def _gen(m, nv, seed, variant=None):
    rng = np.random.default_rng(91000 + 31 * m + seed)
    G = rng.integers(0, 3, (m, nv), dtype=np.int8)
    h = 2.0 * G.sum(axis=1, dtype=np.int64) + 1.0
    c = np.zeros(nv + m)
    cols = rng.choice(nv, NCOST, replace=False)
    c[cols] = -rng.integers(1, 10, NCOST).astype(float)
    A = np.zeros((m, nv + m))
    A[:, :nv] = G
    A[np.arange(m), nv + np.arange(m)] = 1.0
    if variant == "phase1":      # 32 rows flipped to -G_i x <= -1: the slack start is infeasible, Phase I finds a vertex
        rows = rng.choice(m, 32, replace=False)
        A[rows, :nv] = -A[rows, :nv]
        h[rows] = -1.0
    elif variant == "infeasible":   # G_i >= 0, h_i = -1
        h[int(rng.integers(m))] = -1.0
    elif variant == "unbounded":    # c_j < 0, G[:, j] <= 0 (not all zero: the loop finds the ray, not the input check)
        j = int(cols[0])
        A[:, j] = 0.0
        A[rng.choice(m, 8, replace=False), j] = -1.0
    return c, A, h


@functools.lru_cache(maxsize=2)
def _problem(m, nv, seed=0, variant=None):
    return _gen(m, nv, seed, variant)


def _certify(c, A, b, g, nv):
    """primal feasibility of x, dual feasibility of y = B^-T c_B, c^T x == b^T y.  B's slack columns are unit vectors: y is zero on
    the rows whose slack is basic, and the structural columns of B fix y on the other rows (a square solve of their size)."""
    m, n = A.shape
    assert g.x is not None and g.basis is not None
    x, basis = g.x, np.asarray(g.basis)
    assert basis.min() >= 0 and basis.max() < n and len(set(basis.tolist())) == m
    bscale = max(1.0, float(np.abs(b).max()))
    assert x.min() >= -1e-9 * bscale
    assert np.abs(A @ x - b).max() <= 1e-9 * bscale * nv
    struct = basis[basis < nv]
    slack_rows = basis[basis >= nv] - nv
    rows = np.setdiff1d(np.arange(m), slack_rows)
    assert len(rows) == len(struct)
    y = np.zeros(m)
    if len(struct):
        y[rows] = np.linalg.solve(A[np.ix_(rows, struct)].T, c[struct])
    r = c - A[rows].T @ y[rows]
    cscale = max(1.0, float(np.abs(c).max()))
    assert r.min() >= -1e-9 * cscale * max(1.0, float(np.abs(y).max())), r.min()
    zp, zd = float(c @ x), float(b @ y)
    assert abs(zp - zd) <= 1e-9 * max(1.0, abs(zp)), (zp, zd)
    assert abs(g.z - zp) <= 1e-9 * max(1.0, abs(zp))


# ---- 1. beyond the old limit -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m,nv", [(8193, 2 * 8193), (12288, 12288 // 2)])
def test_beyond_the_lds_window_flat_call(m, nv):
    """8193 rows wide (n = 3m) and 12288 rows narrow (n - m = m / 2) through gomilp_lp_simplex: both on the three-kernel revised
    simplex with chunked staging (beyond 8192 rows the tableau pipelines do not run); until the chunked form these were UNSUPPORTED."""
    c, A, b = _problem(m, nv)
    g = lp.simplex(c, A, b, 0.0, None)
    print("m %d n %d: status %s pivots %d + %d pipeline %s, pivot loop %.3f s, final solve %.3f s, total %.3f s" % (
        m, nv + m, lp.STATUS_NAMES.get(g.status, g.status), g.stats["pivots_phase1"], g.stats["pivots_phase2"], g.stats["pipeline"],
        g.stats["seconds_pivot_loop"], g.stats["seconds_final_solve"], g.stats["seconds_total"]))
    assert g.status == lp.OK, lp.STATUS_NAMES.get(g.status, g.status)
    assert g.stats["pipeline"] == "three-kernel"
    assert g.stats["pivots_phase2"] > 0
    _certify(c, A, b, g, nv)


# ---- 2. Phase I, infeasible, unbounded ---------------------------------------------------------------------------------------------

VARIANTS = {"phase1": lp.OK, "infeasible": lp.ERR_INFEASIBLE, "unbounded": lp.ERR_UNBOUNDED}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_statuses_beyond_the_lds_window(variant):
    """the construction at 512 rows against the oracle (status, z), then the same status at 8200 rows (and the certificate)"""
    c, A, b = _gen(512, 1024, 1, variant)
    o = O.simplex(c, A, b, 0.0, None, fast_initial_basis=True)
    s = lp.simplex(c, A, b, 0.0, None)
    assert o.status == VARIANTS[variant] == s.status, (O.STATUS_NAMES.get(o.status), lp.STATUS_NAMES.get(s.status))
    if o.x is not None:
        assert abs(s.z - o.z) <= 1e-9 * max(1.0, abs(o.z))
    c, A, b = _problem(8200, 2 * 8200, 1, variant)
    g = lp.simplex(c, A, b, 0.0, None)
    print("%s: status %s pivots %d + %d" % (variant, lp.STATUS_NAMES.get(g.status, g.status), g.stats["pivots_phase1"], g.stats["pivots_phase2"]))
    assert g.status == VARIANTS[variant], lp.STATUS_NAMES.get(g.status, g.status)
    assert g.stats["pipeline"] == "three-kernel"
    if variant == "phase1":
        assert g.stats["phase1_used"] == 1
        _certify(c, A, b, g, 2 * 8200)


# ---- 3. children of a large root ---------------------------------------------------------------------------------------------------

def test_resident_root_and_its_children():
    """the 8200-row root through gomilp_lp_upload + gomilp_lp_solve_resident (certificate, bit-identical to the flat call); then one
    and three branch rows on it, assembled on the device (gomilp_lp_upload_child): certificate, and bit-identical to the flat call on
    the child assembled on the host"""
    m, nv = 8200, 2 * 8200
    c0, A0, b0 = _problem(m, nv)
    f = lp.simplex(c0, A0, b0, 0.0, None)
    cx = lp.Context()
    try:
        root = cx.upload(c0, A0, b0)
        r = root.solve(0.0)
        print("root m %d: status %s pivots %d, pivot loop %.3f s, final solve %.3f s" % (
            m, lp.STATUS_NAMES.get(r.status), r.stats["pivots_phase2"], r.stats["seconds_pivot_loop"], r.stats["seconds_final_solve"]))
        assert r.status == f.status == lp.OK
        assert r.stats["pipeline"] == "three-kernel"
        _certify(c0, A0, b0, r, nv)
        assert np.array_equal(r.basis, f.basis) and np.array_equal(r.x, f.x) and r.z == f.z
        xs = r.x[:nv]
        top = [int(j) for j in np.argsort(-xs)[:3]]
        assert xs[top[2]] > 0
        floor_ = lambda j: float(np.floor(xs[j] / 2))   # noqa: E731  (a bound that cuts the root's point off)
        children = [[(top[0], 1.0, floor_(top[0]))],
                    [(top[0], -1.0, -float(np.floor(xs[top[0]]) + 1.0)), (top[1], 1.0, floor_(top[1])), (top[2], 1.0, floor_(top[2]))]]
        for cons in children:
            ch = root.child(cons)
            g = ch.solve(0.0)
            ch.free()
            cc, AA, bb = O.child_standard_form(c0, A0, b0, cons)
            f = lp.simplex(cc, AA, bb, 0.0, None)
            print("child %s: status %s / flat %s, pivots %d + %d" % (cons, lp.STATUS_NAMES.get(g.status), lp.STATUS_NAMES.get(f.status),
                                                                     g.stats["pivots_phase1"], g.stats["pivots_phase2"]))
            assert g.status == f.status
            if f.status == lp.OK:
                _certify(cc, AA, bb, g, nv)   # (the child is [[G], [G#]] | I: its unit columns are the last m)
                assert np.array_equal(g.basis, f.basis) and np.array_equal(g.x, f.x) and g.z == f.z
        root.free()
    finally:
        cx.close()


# ---- 4. the chunked form forced below the window: bit-identical ---------------------------------------------------------------------

BUDGET = 400


@pytest.mark.parametrize("m", [300, 1000, 2050])
def test_forced_chunks_bit_identical(m):
    """row_chunk = 512 / 1536 doubles (neither divides ld) on synth.wide_degenerate_lp with tableau = 0, fused = 0: status, every trace
    field including bland, positional basis, the bits of x and z equal to the one-pass kernels; at 300 rows also the oracle"""
    c, A, b = synth.wide_degenerate_lp(m, 0)
    runs = {}
    for chunk in (0, 512, 1536):
        cx = lp.Context(tableau=0, fused=0, max_pivots=BUDGET, row_chunk=chunk)
        try:
            runs[chunk] = cx.upload(c, A, b).solve(0.0, trace=True)
        finally:
            cx.close()
    ref = runs[0]
    assert ref.stats["pipeline"] == "three-kernel"
    print("m %d: status %s, %d pivots (%d Bland steps)" % (m, lp.STATUS_NAMES.get(ref.status), len(ref.pivots), ref.stats["bland_steps"]))
    assert len(ref.pivots) > 0
    for chunk in (512, 1536):
        g = runs[chunk]
        assert g.stats["pipeline"] == "three-kernel"
        assert g.status == ref.status
        assert g.pivots == ref.pivots, "first differing pivot %d" % next(
            (i for i, (p, q) in enumerate(zip(g.pivots, ref.pivots)) if p != q), min(len(g.pivots), len(ref.pivots)))
        assert (g.stats["pivots_phase1"], g.stats["pivots_phase2"], g.stats["bland_steps"]) == \
            (ref.stats["pivots_phase1"], ref.stats["pivots_phase2"], ref.stats["bland_steps"])
        if ref.x is None:
            assert g.x is None
        else:
            assert np.array_equal(g.basis, ref.basis)
            assert g.x.tobytes() == ref.x.tobytes() and np.float64(g.z).tobytes() == np.float64(ref.z).tobytes()
    if m == 300:
        o = O.simplex(c, A, b, 0.0, None, fast_initial_basis=True, trace=True, stop_after_pivots=BUDGET)
        g = runs[512]
        if not o.truncated:
            assert g.status == o.status
            if o.x is not None:
                assert abs(g.z - o.z) <= 1e-9 * max(1.0, abs(o.z))


def test_forced_chunks_phase1_bit_identical():
    """a Phase-I start (forced pivot of the artificial column, refresh of x_B through the chunked matrix-vector kernel) at 600 rows"""
    c, A, b = _gen(600, 1200, 2, "phase1")
    runs = []
    for chunk in (0, 512):
        cx = lp.Context(tableau=0, fused=0, row_chunk=chunk)
        try:
            runs.append(cx.upload(c, A, b).solve(0.0, trace=True))
        finally:
            cx.close()
    a, g = runs
    assert a.status == g.status == lp.OK and a.stats["phase1_used"] == 1
    assert g.pivots == a.pivots
    assert np.array_equal(g.basis, a.basis) and g.x.tobytes() == a.x.tobytes() and g.z == a.z


def test_row_chunk_knob_values():
    cx = lp.Context()
    try:
        for v in (0, 512, 1536, 8192):
            cx.set("row_chunk", v)
        for v in (-512, 256, 1000, 8704):
            with pytest.raises(ValueError):
                cx.set("row_chunk", v)
    finally:
        cx.close()


# ---- 5. what stays refused ---------------------------------------------------------------------------------------------------------

def test_refusals_beyond_the_window_leave_the_context_usable():
    """8200 rows: an equality row (no slack basis), a supplied initial basis and a pool root stay UNSUPPORTED; the context then
    solves a small LP bit for bit like the oracle"""
    m, nv = 8200, 64
    c, A, b = _gen(m, nv, 3)
    Aeq, ceq = np.delete(A, nv, axis=1), np.delete(c, nv)   # row 0 loses its slack: an equality row
    cx = lp.Context()
    try:
        g = cx.upload(ceq, Aeq, b).solve(0.0)
        assert g.status == lp.ERR_UNSUPPORTED, lp.STATUS_NAMES.get(g.status)
        g = cx.upload(c, A, b).solve(0.0, initial_basic=np.arange(nv, nv + m))
        assert g.status == lp.ERR_UNSUPPORTED, lp.STATUS_NAMES.get(g.status)
        g = cx.upload(c, A, b).solve(0.0)
        assert g.status == lp.OK and g.stats["pipeline"] == "three-kernel"
        _certify(c, A, b, g, nv)
        cs, As, bs = synth.dense_lp_standard_form(96, 5)
        s = cx.upload(cs, As, bs).solve(0.0)
        o = O.simplex(cs, As, bs, 0.0, None, fast_initial_basis=True)
        assert s.status == o.status == lp.OK and np.array_equal(s.x, o.x) and s.z == o.z
    finally:
        cx.close()
    assert lp.simplex(ceq, Aeq, b, 0.0, None).status == lp.ERR_UNSUPPORTED
    pool = lp.FrontierPool(workers=1)
    try:
        with pytest.raises(RuntimeError, match="unsupported"):
            pool.set_root(c, A, b)
    finally:
        pool.close()
