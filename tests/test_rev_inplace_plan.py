"""Pool knobs rev_inplace / rev_mem_limit without a device (DESIGN.md section 2.5e "Root in place"): the routing probe takes both keys
and does not route by them, and gomilp_debug_rev_footprint reports the two arenas of a wave of the batched revised simplex as
RevBatchEngine::layout lays them out — the function RevBatchEngine::run sizes its buffers from.

The expected doubles are computed here from the layout's own terms (engine_batch_revised.cpp): per relaxation of m rows, n columns,
ld = m rounded up to even, every buffer rounded up to an even count of doubles."""
import pytest

from tests.test_wave_plan import FEAS, NARROW, P1, WIDE

K_MAX_PARTIALS = 1024   # device_types.h kMaxPartials


@pytest.fixture(scope="module")
def lp():
    from gomilp_amd import lp
    return lp


def even(v):
    return (v + 1) & ~1


def at_doubles(m, n):
    return (n + 1) * even(m)


def work_doubles(m, n, state):
    """the work arena of one relaxation without the artificial row; `state` = doubles of its DevState"""
    ld = even(m)
    terms = [m * ld, m * ld, ld, ld, ld, ld, ld, n + 1 - m, n + 1, 64 * ld, (ld + 1) // 2, (n + 2 - m + 1) // 2, (n + 2 + 1) // 2,
             K_MAX_PARTIALS, K_MAX_PARTIALS, K_MAX_PARTIALS // 2, K_MAX_PARTIALS // 2, state]
    return sum(even(t) for t in terms)


@pytest.fixture(scope="module")
def state(lp):
    """doubles of a relaxation's DevState: what one 1 x 2 relaxation takes beyond its other terms (the same constant for every shape)"""
    _, wk = lp.debug_rev_footprint([(1, 2)], [0])
    s = wk - work_doubles(1, 2, 0)
    assert 0 < s <= 64 and s % 2 == 0
    return s


# ---- knob keys ----

@pytest.mark.parametrize("roots,kids", [([WIDE], [FEAS, P1, FEAS * 2, []]), ([NARROW], [FEAS] * 3 + [P1] * 3)])
def test_wave_plan_takes_the_keys_and_does_not_route_by_them(lp, roots, kids):
    base = lp.debug_wave_plan(roots, kids)
    assert base["route"] == ("REVISED" if roots[0] is WIDE else "TABLEAU")
    for knobs in (dict(rev_inplace=1), dict(rev_inplace=0), dict(rev_mem_limit=4096), dict(rev_inplace=1, rev_mem_limit=1)):
        assert lp.debug_wave_plan(roots, kids, **knobs) == base, knobs
    with pytest.raises(ValueError):
        lp.debug_wave_plan(roots, kids, rev_mem_limit=-1)


# ---- footprint ----

def _check(lp, state, roots, ks, root_of):
    shapes = [(roots[r][0] + k, roots[r][1] + k) for r, k in zip(root_of or [0] * len(ks), ks)]
    at0, wk0 = lp.debug_rev_footprint(roots, ks, root_of=root_of, inplace=False)
    at1, wk1 = lp.debug_rev_footprint(roots, ks, root_of=root_of, inplace=True)
    assert at0 == sum(at_doubles(m, n) for m, n in shapes)
    assert wk0 == sum(work_doubles(m, n, state) for m, n in shapes)
    assert at1 == 0
    assert wk1 - wk0 == sum(even(m) for m, _ in shapes)
    return at0, wk0, wk1


def test_footprint_odd_root_k_0_to_3(lp, state):
    """root 67 x 277 (odd m0): children of 67, 68, 69, 70 rows — ld 68, 68, 70, 70"""
    at0, wk0, wk1 = _check(lp, state, [(67, 277)], [0, 1, 2, 3], None)
    assert at0 == 278 * 68 + 279 * 68 + 280 * 70 + 281 * 70
    assert wk1 - wk0 == 68 + 68 + 70 + 70
    # the same wave as constraint lists
    assert lp.debug_rev_footprint([(67, 277)], [[], FEAS, FEAS * 2, FEAS * 3]) == (at0, wk0)


def test_footprint_two_roots_alternating(lp, state):
    roots = [(66, 266), (80, 410)]
    ks = [0, 1, 2, 3, 1, 0]
    _check(lp, state, roots, ks, [0, 1, 0, 1, 0, 1])
    # (root_of matters: the other assignment is another wave)
    assert lp.debug_rev_footprint(roots, ks, root_of=[0, 1, 0, 1, 0, 1]) != lp.debug_rev_footprint(roots, ks, root_of=[1, 0, 1, 0, 1, 0])


def test_footprint_refuses_a_bad_list(lp):
    roots = [(66, 266), (80, 410)]
    for bad in ([0, 2], [0, -1]):
        with pytest.raises(ValueError):
            lp.debug_rev_footprint(roots, [1, 1], root_of=bad)
    with pytest.raises(ValueError):
        lp.debug_rev_footprint([(0, 10)], [1])
    import ctypes as C
    import numpy as np
    out = np.zeros(2, dtype=np.int64)
    rm, rn = np.array([66], dtype=np.int64), np.array([266], dtype=np.int64)
    koff = np.array([0, 1], dtype=np.int64)
    rof = np.array([1], dtype=np.int32)
    ip = C.POINTER(C.c_int64)
    rc = lp.lib().gomilp_debug_rev_footprint(1, rm.ctypes.data_as(ip), rn.ctypes.data_as(ip), 1, rof.ctypes.data_as(C.POINTER(C.c_int32)),
                                             koff.ctypes.data_as(ip), 0, out.ctypes.data_as(ip))
    assert rc == -lp.ERR_BAD_SHAPE
