"""Which block kernel runs a relaxation on the blocked tableau, and in which shape: the engine's BtPlan (gomilp_amd/csrc/engine.hpp,
BtPlan::make in engine_tableau.cpp) against the routing table of DESIGN.md section 2.1 — host-only entry of the library, no GPU needed."""
import ctypes as C
import itertools

import pytest

SINGLE, GROUPS, LOOP = 0, 1, 2


def _plan(m, ldt, ncu=256, **knobs):
    from gomilp_amd import lp
    return lp.debug_bt_plan(m, ldt, ncu=ncu, **knobs)


def _check(m, ldt, knobs, want):
    p = _plan(m, ldt, **knobs)
    got = {k: p[k] for k in want}
    assert got == want, (m, ldt, knobs, p)
    return p


# (m, ldt) per class of need = max(m, ldt): both sides of every edge, m > ldt and m < ldt
SINGLE_WG = [(599, 512), (599, 1024), (300, 1024), (512, 512), (8, 512)]
PROMOTED = [(600, 512), (600, 1024), (1024, 1024), (1024, 512), (700, 1024)]
UP_TO_2048 = [(1025, 1024), (1025, 512), (600, 1536), (300, 1536), (2048, 2048), (2048, 1024), (1100, 2048)]
UP_TO_4096 = [(2049, 2048), (2049, 512), (1100, 2560), (4096, 4096), (4096, 2048), (3000, 4096)]
UP_TO_8192 = [(4097, 4096), (4097, 512), (2000, 4608), (8192, 8192), (8192, 3584), (5000, 8192)]
WAVE16 = dict(pipeline=LOOP, K=8, loop="16x128_wave", loop_groups=16, loop_nt=128, loop_wave_rec=1, loop_min_grid=136, slot_weight=1, upd_cap=0,
              cfg_groups=8, cfg_nt=256, cfg_ri=1, tiled=1, rep=None)
K16_BIG = dict(pipeline=LOOP, K=16, loop="16x256_k16", loop_groups=16, loop_nt=256, loop_kb=16, loop_wave_rec=0, loop_min_grid=128, slot_weight=4,
               upd_cap=112, cfg_groups=8, cfg_nt=512, cfg_ri=1, tiled=1, rep=None)


def test_default_routing_by_shape():
    for m, ldt in SINGLE_WG:
        p = _check(m, ldt, {}, dict(pipeline=SINGLE, cfg_groups=0, loop=None, rep=None, slot_weight=0))
        assert p["K"] in (8, 16) and (p["K"] == 8 or not p["tiled"]), p   # 8 where the block's terms fit in registers (bt_reg_k): only then tiled
    assert _plan(512, 512)["K"] == 8 and _plan(512, 512)["tiled"] == 1
    for m, ldt in PROMOTED + UP_TO_2048:
        _check(m, ldt, {}, WAVE16)
    for m, ldt in UP_TO_4096:
        _check(m, ldt, {}, K16_BIG)
    for m, ldt in UP_TO_8192:
        _check(m, ldt, {}, dict(pipeline=GROUPS, K=16, cfg_groups=8, cfg_nt=512, cfg_ri=2, tiled=1, loop=None, rep=None, slot_weight=0))
    for m, ldt in [(8193, 8192), (100, 8704)]:   # beyond every multi-workgroup shape
        _check(m, ldt, {}, dict(pipeline=SINGLE, cfg_groups=0, loop=None))


def test_grid_of_a_loop_launch():
    """min(ncu, max(64, one workgroup per 256 KB of tableau)), never below the instance's minimum; knob loop_grid overrides the formula only."""
    assert _plan(1100, 1536)["grid"] == 136            # 51 -> 64 -> the 16 x 128 instance's 136
    assert _plan(2048, 2048)["grid"] == 136            # 128 -> 136
    assert _plan(2048, 2048, loop_k=16)["grid"] == 128
    assert _plan(2048, 2048, loop_g=8)["grid"] == 128
    assert _plan(1100, 1536, loop_g=8)["grid"] == 64
    assert _plan(4096, 4096)["grid"] == 256            # 512 -> one per CU
    assert _plan(4096, 4096, ncu=304)["grid"] == 304
    assert _plan(3000, 2560)["grid"] == 234
    assert _plan(4096, 4096, loop_grid=100)["grid"] == 128
    assert _plan(4096, 4096, loop_grid=200)["grid"] == 200
    assert _plan(300, 512, bt_groups=2)["grid"] == 64 and _plan(300, 512, bt_groups=2, loop_grid=8)["grid"] == 16
    assert _plan(2048, 2048, loop_rep=1)["rep_grid"] == 136


def test_knobs_on_the_4096_row_class():
    for m, ldt in UP_TO_4096:
        _check(m, ldt, dict(loop_k=12), dict(pipeline=LOOP, K=12, loop="16x256_k12", loop_kb=12, loop_min_grid=136, upd_cap=112, slot_weight=4))
        _check(m, ldt, dict(loop_k=16), K16_BIG)
        _check(m, ldt, dict(loop_k=8), dict(pipeline=LOOP, K=8, loop="8x512", loop_groups=8, loop_nt=512, loop_min_grid=64, upd_cap=0, slot_weight=4))
        _check(m, ldt, dict(loop_g=8), dict(pipeline=LOOP, K=16, loop="8x512_k16", loop_kb=16, loop_min_grid=64, upd_cap=0, slot_weight=4))
        _check(m, ldt, dict(loop_g=8, loop_k=12), dict(pipeline=LOOP, K=16, loop="8x512_k16", slot_weight=4))
        _check(m, ldt, dict(loop_g=8, loop_k=8), dict(pipeline=LOOP, K=8, loop="8x512", slot_weight=4))
        _check(m, ldt, dict(loop_upd=90), dict(loop="16x256_k16", upd_cap=90))
        _check(m, ldt, dict(loop_rep=1), dict(loop="16x256_k16", rep=None))
        _check(m, ldt, dict(loop_wave_rec=0), K16_BIG)
        for stamps in (1, 2):   # no stamped loop instance in the class of 512 threads: launch pairs
            _check(m, ldt, dict(bt_stamps=stamps), dict(pipeline=GROUPS, K=16, cfg_groups=8, cfg_nt=512, loop=None, slot_weight=0))


def test_knobs_on_the_2048_row_class():
    for m, ldt in UP_TO_2048 + PROMOTED:
        promoted = max(m, ldt) <= 1024
        _check(m, ldt, dict(loop_wave_rec=0), dict(pipeline=LOOP, K=8, loop="16x128", loop_wave_rec=0, loop_min_grid=136, slot_weight=1, upd_cap=0))
        _check(m, ldt, dict(loop_k=16), dict(pipeline=LOOP, K=16, loop="16x256_k16", loop_min_grid=128, slot_weight=1, upd_cap=0, cfg_nt=256, rep=None))
        _check(m, ldt, dict(loop_k=12), WAVE16)
        _check(m, ldt, dict(loop_g=8), dict(pipeline=LOOP, K=8, loop="8x256", loop_groups=8, loop_nt=256, loop_min_grid=64, slot_weight=4, upd_cap=0))
        _check(m, ldt, dict(loop_g=8, loop_k=16), dict(pipeline=LOOP, K=8, loop="8x256", slot_weight=4))
        _check(m, ldt, dict(loop_g=8, loop_rep=1), dict(loop="8x256", rep=None))
        _check(m, ldt, dict(loop_k=16, loop_rep=1), dict(loop="16x256_k16", rep=None))
        small = m <= 1024 and ldt <= 1024
        _check(m, ldt, dict(loop_rep=1), dict(WAVE16, rep="rep_16x256" if small else "rep_16x512", rep_nt=256 if small else 512, rep_stamped=0))
        _check(m, ldt, dict(loop_upd=40, loop_rep=1), dict(upd_cap=40, rep_upd_cap=40))
        if promoted:   # a nonzero bt_stamps switches the promotion off
            _check(m, ldt, dict(bt_stamps=1), dict(pipeline=SINGLE, loop=None))
            _check(m, ldt, dict(bt_stamps=2), dict(pipeline=SINGLE, loop=None))
            continue
        _check(m, ldt, dict(bt_stamps=1), dict(pipeline=LOOP, K=8, loop="8x256_stamped", loop_stamped=1, slot_weight=4))
        _check(m, ldt, dict(bt_stamps=2), dict(pipeline=LOOP, K=8, loop="16x128_wave_stamped", loop_stamped=1, loop_wave_rec=1, slot_weight=1))
        _check(m, ldt, dict(bt_stamps=2, loop_wave_rec=0), dict(pipeline=LOOP, K=8, loop="16x128_stamped", loop_wave_rec=0, slot_weight=1))
        _check(m, ldt, dict(bt_stamps=2, loop_g=8), dict(loop="8x256_stamped", slot_weight=4))
        _check(m, ldt, dict(bt_stamps=2, loop_k=16), dict(K=8, loop="16x128_wave_stamped"))
        _check(m, ldt, dict(bt_stamps=2, loop_rep=1), dict(rep="rep_16x256" if small else "rep_16x512_stamped", rep_stamped=0 if small else 1))
    for m, ldt in SINGLE_WG:   # the loop shapes below their default range: measurement knob bt_groups = 16
        _check(m, ldt, dict(bt_groups=16), WAVE16)
        _check(m, ldt, dict(bt_groups=16, bt_stamps=2), dict(pipeline=LOOP, loop="16x128_wave_stamped"))


def test_forced_and_fallback_routing():
    every = SINGLE_WG + PROMOTED + UP_TO_2048 + UP_TO_4096 + UP_TO_8192
    for m, ldt in every:
        need = max(m, ldt)
        for knobs in (dict(bt_groups=-1), dict(bt_old=1), dict(bt_old=1, bt_groups=8)):
            _check(m, ldt, knobs, dict(pipeline=SINGLE, cfg_groups=0, loop=None, rep=None, slot_weight=0))
        assert _plan(m, ldt, bt_old=1)["tiled"] == 0 and _plan(m, ldt, bt_old=1)["tiled_forced"] == 0
        # no loop: launch pairs in the shape class, K = min(block_k, 16) or 16; the 600..1024-row promotion is off
        for knobs, K in ((dict(bt_lag=0), 16), (dict(block_k=8), 8), (dict(block_k=32), 16), (dict(max_pivots=100), 16)):
            p = _check(m, ldt, knobs, dict(loop=None, rep=None, slot_weight=0))
            if need <= 1024:
                assert p["pipeline"] == SINGLE and p["K"] == (knobs.get("block_k") or p["K"]), p
            else:
                assert (p["pipeline"], p["K"], p["cfg_groups"], p["tiled"]) == (GROUPS, K, 8, 1), p
        for G in (2, 4, 8):
            p = _plan(m, ldt, bt_groups=G)
            if G * 512 >= need:      # one row per thread
                inst = {2: "2x512", 4: "4x512", 8: "16x256_k16"}[G]
                assert (p["pipeline"], p["K"], p["loop"], p["slot_weight"], p["cfg_groups"], p["cfg_nt"], p["cfg_ri"]) == (LOOP, 8 if G < 8 else 16, inst, 4, G, 512, 1), p
                assert p["upd_cap"] == (112 if G == 8 else 0) and p["loop_min_grid"] == (8 * G if G < 8 else 128), p
                _check(m, ldt, dict(bt_groups=G, bt_lag=0), dict(pipeline=GROUPS, K=16, cfg_groups=G, cfg_ri=1, loop=None))
                _check(m, ldt, dict(bt_groups=G, bt_stamps=1), dict(pipeline=GROUPS, K=16, loop=None))
            elif G * 1024 >= need:   # two rows per thread: no loop instance
                assert (p["pipeline"], p["K"], p["loop"], p["slot_weight"], p["cfg_groups"], p["cfg_nt"], p["cfg_ri"]) == (GROUPS, 16, None, 0, G, 512, 2), p
            else:
                assert (p["pipeline"], p["cfg_groups"], p["loop"]) == (SINGLE, 0, None), p
        _check(m, ldt, dict(bt_groups=8, loop_k=8), dict(loop="8x512" if need <= 4096 else None))
        _check(m, ldt, dict(bt_groups=8, loop_g=8), dict(loop="8x512_k16" if need <= 4096 else None))
        _check(m, ldt, dict(bt_groups=8, loop_k=12), dict(loop="16x256_k12" if need <= 4096 else None))
        # pivots between two looks at the state: a launch of loop_chunk pivots (at least 4 blocks), else chunk pivots (at least a block)
        p = _plan(m, ldt)
        assert p["blocks_per_chunk"] == (max(4, 512 // p["K"]) if p["pipeline"] == LOOP else max(1, 32 // p["K"])), p
        p = _plan(m, ldt, loop_chunk=32, chunk=4)
        assert p["blocks_per_chunk"] == (4 if p["pipeline"] == LOOP else 1), p


def test_knob_ranges_are_those_of_ctx_set():
    for bad in (dict(bt_groups=3), dict(loop_g=4), dict(loop_k=10), dict(bt_nt=128), dict(block_k=-1), dict(block_k=1000), dict(loop_chunk=16),
                dict(loop_grid=5000), dict(loop_upd=-1), dict(chunk=0), dict(tableau=0), dict(no_such_knob=1)):
        with pytest.raises(ValueError):
            _plan(1100, 1536, **bad)
    assert _plan(1100, 1536, bt_stamps=7)["loop"] == "16x128_wave_stamped"   # clamped to 2
    assert _plan(1100, 1536, bt_stamps=-3)["loop"] == "16x128_wave"
    assert _plan(1100, 1536, loop_wave_rec=5)["loop"] == "16x128_wave"
    with pytest.raises(ValueError):
        _plan(0, 512)


def test_every_plan_of_the_knob_product_is_consistent():
    """Over the product of the edge shapes with every legal value of the routing knobs: a loop plan names an instance of the enum whose
    G x NT threads cover max(m, ldt) and whose block size is the plan's K; the slot weight is 1 exactly for the 16 x 128 instances and for
    16 x 256 in blocks of 16 on the class of 256 threads (up to 2048 rows); a plan without the loop kernel names none."""
    from gomilp_amd import lp
    shapes = [(599, 512), (600, 512), (599, 1024), (600, 1024), (1024, 1024), (1025, 1024), (600, 1536), (2048, 1024), (2049, 2048), (1100, 2560),
              (4096, 4096), (4097, 4096), (3000, 4608), (8192, 8192)]
    names = ["bt_groups", "bt_lag", "bt_stamps", "loop_k", "loop_g", "loop_rep", "loop_wave_rec", "block_k"]
    values = [(-1, 0, 2, 4, 8, 16), (0, 1), (0, 1, 2), (0, 8, 12, 16), (0, 8, 16), (0, 1), (0, 1), (0, 8, 32)]
    F = {k: i for i, k in enumerate(lp.BT_PLAN_FIELDS)}
    inst = lp.BT_LOOP_INSTANCES
    f = lp.lib().gomilp_debug_bt_plan
    keys = (C.c_char_p * len(names))(*[k.encode() for k in names])
    vals = (C.c_int64 * len(names))()
    out = (C.c_int64 * len(lp.BT_PLAN_FIELDS))()
    seen = set()
    for combo in itertools.product(*values):
        vals[:] = combo
        for m, ldt in shapes:
            assert f(m, ldt, len(names), keys, vals, 256, out) == len(out)
            p = out[:]
            ctx = (m, ldt, combo, p)
            loop, rep = p[F["loop"]], p[F["rep"]]
            if p[F["pipeline"]] != LOOP:
                assert loop == 0 and rep == 0 and p[F["slot_weight"]] == 0 and p[F["grid"]] == 0 and p[F["rep_grid"]] == 0, ctx
                assert (p[F["pipeline"]] == GROUPS) == (p[F["cfg_groups"]] > 0), ctx
                continue
            seen.add(inst[loop])
            assert 1 <= loop < len(inst) and not inst[loop].startswith("rep_"), ctx
            assert p[F["loop_groups"]] * p[F["loop_nt"]] >= max(m, ldt) and p[F["loop_kb"]] == p[F["K"]], ctx
            assert p[F["cfg_groups"]] * p[F["cfg_nt"]] * p[F["cfg_ri"]] >= max(m, ldt) and p[F["cfg_ri"]] == 1 and p[F["tiled"]] == 1, ctx
            shared = inst[loop].startswith("16x128") or (inst[loop] == "16x256_k16" and p[F["cfg_nt"]] == 256)
            assert p[F["slot_weight"]] == (1 if shared else 4), ctx
            assert p[F["grid"]] >= p[F["loop_min_grid"]] >= 8 * p[F["loop_groups"]], ctx
            assert p[F["loop_stamped"]] == (1 if combo[2] else 0), ctx
            if rep:
                seen.add(inst[rep])
                assert inst[rep].startswith("rep_") and combo[5] == 1 and p[F["K"]] == 8 and p[F["cfg_nt"]] == 256, ctx
                assert 16 * p[F["rep_nt"]] * 4 >= max(m, ldt) and p[F["rep_grid"]] >= 136, ctx   # four columns per thread
    assert seen == set(inst[1:]), seen
