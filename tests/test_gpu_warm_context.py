"""Warm start on a single context (gomilp_lp_solve_warm): a kept parent state, children started from it with the
dual simplex on the revised-simplex kernels (dual_kernels.hip), beyond 8192 rows included.

Parity as the pool's warm start: the status of the cold solve of the same problem on the same context, |z - z_cold| <= 1e-9
max(1, |z_cold|), and for OK an optimality certificate of the final basis computed here.  The fallbacks are bit-identical to the
cold solve.  Roots: min c^T x s.t. G x <= h, x >= 0 in GoMILP's standard form [G | I] (the generator of test_gpu_large_rows)."""
import math
import os

import numpy as np
import pytest

from gomilp_amd import bnb, lp, synth
from tests.test_gpu_large_rows import _certify, _gen

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DUAL_BUDGET_C5 = 1024   # eight new rows at once take more dual pivots than one


def _dense_child(c, A, b, rows):
    """host copy of a child (subproblem.go:81-139): [[A, 0], [g, I]], c' = [c, 0], b' = [b; h]"""
    m, n = A.shape
    K = len(rows)
    A2 = np.zeros((m + K, n + K))
    A2[:m, :n] = A
    for k, (v, s, h) in enumerate(rows):
        A2[m + k, v] = s
        A2[m + k, n + k] = 1.0
    return np.concatenate([c, np.zeros(K)]), A2, np.concatenate([b, [h for (_, _, h) in rows]])


def _parity(w, cold, label=""):
    assert w.status == cold.status, (label, w.status, cold.status)
    if cold.status == lp.OK:
        assert abs(w.z - cold.z) <= 1e-9 * max(1.0, abs(cold.z)), (label, w.z, cold.z)
    else:
        assert w.x is None


def _same_bits(a, b):
    assert a.status == b.status
    assert (math.isnan(a.z) and math.isnan(b.z)) or a.z == b.z
    assert (a.x is None) == (b.x is None)
    if a.x is not None:
        assert np.array_equal(a.x, b.x) and np.array_equal(a.basis, b.basis)
    assert a.pivots == b.pivots


def _most_fractional(x, nv):
    f = np.abs(x[:nv] - np.round(x[:nv]))
    j = int(np.argmax(f))
    return j if f[j] > 1e-6 else None


def _branch(x, nv):
    j = _most_fractional(x, nv)
    if j is None:
        return None
    fl = math.floor(x[j])
    return [(j, 1.0, float(fl)), (j, -1.0, -float(fl + 1))]


# ---- branching children, default knobs: tableau parents (the gather) and revised parents (the copy) ------------------------------

@pytest.mark.parametrize("m,nv", [(64, 56), (64, 200), (300, 150), (300, 700), (520, 260), (520, 1100), (1000, 500), (1000, 2048),
                                  (2050, 1025)])
def test_branching_children_warm(m, nv):
    c, A, b = _gen(m, nv, 7)
    cx = lp.Context()
    try:
        root = cx.upload(c, A, b)
        r0 = root.solve(keep=True)
        assert r0.status == lp.OK and r0.stats["warm"]["kept"] == 1 and r0.stats["warm"]["fallback"] == 1
        br = _branch(r0.x, nv)
        if br is None:
            pytest.skip("integral root")
        kids = []
        for row in br:
            ch = root.child([row])
            cold = ch.solve()
            w = ch.solve(parent=root, keep=True)
            ws = w.stats["warm"]
            assert ws["warm_started"] == 1 and ws["fallback"] == 0 and ws["new_rows"] == 1, ws
            assert ws["pivots_dual"] >= 1   # the root's x violates both branch rows
            _parity(w, cold, "child %s" % (row,))
            if w.status == lp.OK:
                _certify(*_dense_child(c, A, b, [row]), w, nv)
                assert ws["kept"] == 1
            kids.append((row, ch, w))
        # a grandchild from its child (J = 1) and from the root (J = 2)
        for row, ch, w in kids:
            if w.status != lp.OK:
                continue
            br2 = _branch(w.x, nv)
            if br2 is None:
                continue
            rows = [row, br2[0]]
            g = root.child(rows)
            cold = g.solve()
            for par, J in ((ch, 1), (root, 2)):
                gw = g.solve(parent=par)
                gs = gw.stats["warm"]
                assert gs["warm_started"] == 1 and gs["new_rows"] == J, gs
                _parity(gw, cold, "grandchild J=%d" % J)
                if gw.status == lp.OK:
                    _certify(*_dense_child(c, A, b, rows), gw, nv)
            g.free()
            break
        # a branch row the root already satisfies: no dual pivot, the root's z
        j = br[0][0]
        sat = root.child([(j, 1.0, float(math.floor(r0.x[j]) + 5))])
        s = sat.solve(parent=root)
        assert s.stats["warm"]["warm_started"] == 1 and s.stats["warm"]["pivots_dual"] == 0
        assert s.status == lp.OK and abs(s.z - r0.z) <= 1e-9 * max(1.0, abs(r0.z))
        sat.free()
        for _, ch, _ in kids:
            ch.free()
    finally:
        cx.close()


# ---- multi-row starts against the oracle fixture of C5 (J = 8) -----------------------------------------------------------------------

def test_C5_children_from_kept_root_match_fixture():
    fx = np.load(os.path.join(GOLD, "frontier_C5.npz"), allow_pickle=False)
    m, seed = synth.CONFIGS["C5"]
    c, A, b = synth.dense_lp_standard_form(m, seed)
    cx = lp.Context()
    try:
        root = cx.upload(c, A, b)
        r0 = root.solve(keep=True)
        assert r0.status == lp.OK and np.array_equal(r0.x, fx["root_x"])
        children = synth.frontier_children(r0.x, synth.integrality_mask(m, m), int(fx["nvars"]))
        started, dual = 0, []
        for i in range(0, len(children), 4):
            ch = root.child(children[i])
            w = ch.solve(parent=root, dual_budget=DUAL_BUDGET_C5)
            ws = w.stats["warm"]
            assert ws["new_rows"] == 8 and ws["fallback"] in (0, 4), ws
            started += ws["warm_started"]
            dual.append(ws["pivots_dual"])
            assert w.status == int(fx["status"][i]), "child %d" % i
            if w.status == lp.OK:
                zf = float(fx["z"][i])
                assert abs(w.z - zf) <= 1e-9 * max(1.0, abs(zf)), "child %d" % i
            ch.free()
        print("C5 children from the kept root: %d of %d warm, dual pivots per child: median %d, max %d" % (
            started, len(dual), int(np.median(dual)), max(dual)))
        assert started >= 48
    finally:
        cx.close()


# ---- the C3 tree on one context ---------------------------------------------------------------------------------------------------------

def test_C3_tree_on_a_context_matches_fixture():
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
    from gen_golden import DECISIONS
    fx = np.load(os.path.join(GOLD, "milp_C3.npz"), allow_pickle=False)
    m3, seed3 = synth.CONFIGS["C3"]
    c3, G3, h3 = synth.dense_lp_inequality_form(m3, seed3)
    int3 = [j % 4 == 0 for j in range(m3)]
    cx = lp.Context()
    try:
        runs = {w: bnb.solve_milp(c3, None, None, G3, h3, int3, max_nodes=127, context=cx, warm=w) for w in (False, True)}
    finally:
        cx.close()
    for w, res in runs.items():
        nodes = [nd for nd in res.nodes if nd.status != -1]
        assert len(nodes) == len(fx["ids"])
        for i, nd in enumerate(nodes):
            assert (nd.id, nd.parent) == (int(fx["ids"][i]), int(fx["parent"][i]))
            K = int(fx["ncons"][i])
            assert [(int(v), float(s), float(h)) for v, s, h in fx["constraints"][i][:K]] == [(v, float(s), float(h)) for v, s, h in nd.constraints]
            assert nd.status == int(fx["status"][i]) and nd.decision == DECISIONS[int(fx["decision"][i])], "warm %s node %d" % (w, nd.id)
            if nd.status == lp.OK:
                zf = float(fx["z"][i])
                assert abs(nd.z - zf) <= 1e-9 * max(1.0, abs(zf)), "warm %s node %d z" % (w, nd.id)
    warm, cold = runs[True], runs[False]
    assert warm.warm_started >= 120
    assert warm.pivots * 3 <= cold.pivots, (warm.pivots, cold.pivots)
    print("C3 tree on a context: cold %d pivots, warm %d (%d dual), %d started warm" % (cold.pivots, warm.pivots, warm.pivots_dual, warm.warm_started))


# ---- infeasible child, budget, cold fallbacks -------------------------------------------------------------------------------------------

def _root_and_branch(cx, m=300, nv=700, seed=7):
    c, A, b = _gen(m, nv, seed)
    root = cx.upload(c, A, b)
    r0 = root.solve(keep=True)
    assert r0.status == lp.OK
    return c, A, b, root, r0


def test_infeasible_child_from_the_dual_loop():
    cx = lp.Context()
    try:
        c, A, b, root, r0 = _root_and_branch(cx)
        j = _most_fractional(r0.x, 700)
        ch = root.child([(j, 1.0, -1.0)])   # x_j <= -1 with x >= 0
        cold = ch.solve()
        w = ch.solve(parent=root)
        assert cold.status == w.status == lp.ERR_INFEASIBLE and w.x is None
        assert w.stats["warm"]["warm_started"] == 1 and w.stats["warm"]["pivots_dual"] >= 1
        assert ch.solve().status == lp.ERR_INFEASIBLE   # the context is still usable
    finally:
        cx.close()


def test_budget_spent_is_the_cold_solve_bit_for_bit():
    cx = lp.Context()
    try:
        c, A, b, root, r0 = _root_and_branch(cx)
        g = None
        for row in _branch(r0.x, 700):   # a child that needs more than one dual pivot
            cand = root.child([row])
            if cand.solve(parent=root).stats["warm"]["pivots_dual"] >= 2:
                g = cand
                break
            cand.free()
        if g is None:
            pytest.skip("both children need a single dual pivot")
        cold = g.solve(trace=True)
        w = g.solve(parent=root, dual_budget=1, trace=True)
        assert w.stats["warm"]["fallback"] == 4 and w.stats["warm"]["warm_started"] == 0
        _same_bits(w, cold)
    finally:
        cx.close()


def test_cold_fallbacks_are_exact():
    cx = lp.Context()
    try:
        c, A, b, root, r0 = _root_and_branch(cx)
        br = _branch(r0.x, 700)
        ch = root.child(br[:1])
        cold = ch.solve(trace=True)
        # parent < 0
        w = ch.solve(keep=True, trace=True)
        assert w.stats["warm"]["fallback"] == 1 and w.stats["warm"]["kept"] == 1
        _same_bits(w, cold)
        # a parent without kept state: solved without keep, then a freed one
        other = root.child(br[1:])
        other.solve()
        w = ch.solve(parent=other, trace=True)
        assert w.stats["warm"]["fallback"] == 2
        _same_bits(w, cold)
        # not a descendant: other rows of the same root, another root
        other.solve(keep=True)
        w = ch.solve(parent=other, trace=True)
        assert w.stats["warm"]["fallback"] == 3
        _same_bits(w, cold)
        c2, A2, b2 = _gen(300, 700, 8)
        root2 = cx.upload(c2, A2, b2)
        assert root2.solve(keep=True).status == lp.OK
        w = ch.solve(parent=root2, trace=True)
        assert w.stats["warm"]["fallback"] == 3
        _same_bits(w, cold)
        other.free()
        # strict mode
        small = _gen(64, 200, 3)
        cxs = lp.Context(exact_degenerate=3)
        try:
            rs = cxs.upload(*small)
            r = rs.solve(keep=True)
            ks = rs.child(_branch(r.x, 200)[:1])
            colds = ks.solve(trace=True)
            ws = ks.solve(parent=rs, trace=True)
            assert ws.stats["warm"]["fallback"] == 5
            _same_bits(ws, colds)
        finally:
            cxs.close()
        # the context is still usable
        w = ch.solve(parent=root)
        assert w.stats["warm"]["warm_started"] == 1
        _parity(w, cold)
    finally:
        cx.close()


def test_non_slack_root_on_a_tableau_pipeline_goes_cold():
    # equality rows: no slack basis, the general start on the tableau pipelines
    rng = np.random.default_rng(5)
    mm, nv = 40, 90
    A = rng.integers(0, 3, (mm, nv)).astype(float)
    x0 = rng.random(nv)
    b = A @ x0
    c = rng.integers(1, 9, nv).astype(float)
    cx = lp.Context()
    try:
        root = cx.upload(c, A, b)
        r0 = root.solve(keep=True)
        if r0.status != lp.OK or r0.stats["pipeline"] not in ("tableau", "blocked"):
            pytest.skip("root did not solve on a tableau pipeline")
        assert r0.stats["warm"]["kept"] == 0
        j = _most_fractional(r0.x, nv)
        ch = root.child([(j, 1.0, float(math.floor(r0.x[j])))])
        cold = ch.solve(trace=True)
        w = ch.solve(parent=root, trace=True)
        assert w.stats["warm"]["fallback"] == 5
        _same_bits(w, cold)
    finally:
        cx.close()


# ---- the chunked dual kernels bit-identical to the one-pass form ------------------------------------------------------------------------

@pytest.mark.parametrize("m,nv,variant", [(300, 700, None), (1000, 2048, None), (2050, 4100, None), (1000, 2048, "phase1")])
def test_chunked_dual_kernels_bit_identical(m, nv, variant):
    c, A, b = _gen(m, nv, 11, variant)
    out = []
    for knobs in ({}, {"row_chunk": 512}):
        cx = lp.Context(**knobs)
        try:
            root = cx.upload(c, A, b)
            r0 = root.solve(keep=True)
            assert r0.status == lp.OK
            if variant == "phase1":
                assert r0.stats["phase1_used"] == 1
            res = []
            for row in _branch(r0.x, nv):
                ch = root.child([row])
                w = ch.solve(parent=root, trace=True)
                assert w.stats["warm"]["warm_started"] == 1
                res.append(w)
            out.append(res)
        finally:
            cx.close()
    for a, b2 in zip(*out):
        assert a.stats["warm"]["pivots_dual"] == b2.stats["warm"]["pivots_dual"]
        _same_bits(a, b2)


# ---- beyond 8192 rows -------------------------------------------------------------------------------------------------------------------

def test_warm_children_beyond_8192_rows():
    m, nv = 8200, 16400
    c, A, b = _gen(m, nv, 0)
    cx = lp.Context()
    try:
        root = cx.upload(c, A, b)
        r0 = root.solve(keep=True)
        assert r0.status == lp.OK and r0.stats["warm"]["kept"] == 1
        br = _branch(r0.x, nv)
        assert br is not None
        ws = []
        for k, row in enumerate(br):
            ch = root.child([row])
            w = ch.solve(parent=root)
            assert w.stats["warm"]["warm_started"] == 1, w.stats["warm"]
            assert w.status == lp.OK
            _certify(*_dense_child(c, A, b, [row]), w, nv)
            if k == 0:
                cold = ch.solve()
                _parity(w, cold)
                cold_piv = cold.stats["pivots_phase1"] + cold.stats["pivots_phase2"]
                assert w.stats["warm"]["pivots_dual"] <= 0.01 * cold_piv, (w.stats["warm"]["pivots_dual"], cold_piv)
                print("8200 rows: cold %d pivots %.2f s, warm %d dual + %d primal pivots, setup %.3f s, dual %.3f s, total %.2f s" % (
                    cold_piv, cold.stats["seconds_total"], w.stats["warm"]["pivots_dual"], w.stats["pivots_phase2"],
                    w.stats["warm"]["seconds_setup"], w.stats["warm"]["seconds_dual"], w.stats["seconds_total"]))
            ch.free()
    finally:
        cx.close()
