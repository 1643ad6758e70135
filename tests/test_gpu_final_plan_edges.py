"""The final solve on either side of each row count at which its schedule plan (LuPlan, gomilp_amd/csrc/engine_final.cpp) changes: 128 / 129
(one-shot small pack), 768 / 769 (look-ahead rounds), 1023 / 1024 (split pack: only the coupled part goes to the host), 1280 / 1281 (32-slot
cross-workgroup panel).  Bar: default knobs against one launch per column (lu_blocked = 0), a fresh context each — identical status and
basis, x and z BIT-IDENTICAL, no fall-back (stats.device_retries == 0); the default runs compressed rounds, the other none."""
import numpy as np
import pytest

from gomilp_amd import lp, synth

pytestmark = pytest.mark.gpu


def _solve(c, A, b, **knobs):
    cx = lp.Context(**knobs)
    try:
        rl = cx.upload(c, A, b)
        out = rl.solve(0.0)
        rl.free()
    finally:
        cx.close()
    return out


@pytest.mark.parametrize("m", [128, 129, 768, 769, 1023, 1024, 1280, 1281])
def test_default_final_solve_equals_per_column_lu_at_the_plan_edges(m):
    c, A, b = synth.dense_lp_standard_form(m, 3)
    got = _solve(c, A, b)
    want = _solve(c, A, b, lu_blocked=0)
    print("m %d: rounds %d dense steps %d final %.3f ms (per column %.3f ms)" % (
        m, got.stats["lu_rounds"], got.stats["lu_dense_steps"], 1e3 * got.stats["seconds_final_solve"], 1e3 * want.stats["seconds_final_solve"]))
    assert got.status == want.status == lp.OK, (got.status, want.status)
    assert np.array_equal(got.basis, want.basis)
    assert np.array_equal(got.x.view(np.uint64), want.x.view(np.uint64)) and got.z == want.z
    assert got.stats["device_retries"] == 0 and want.stats["device_retries"] == 0
    assert got.stats["lu_rounds"] > 0
    assert want.stats["lu_rounds"] == 0
