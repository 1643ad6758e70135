"""Developer tool: the compressed LU rounds beyond 4096 rows (lu_cross.hip k_luc_panel_x with four or eight rows per lane, knob lu_large) against one launch per column
(lu_blocked = 0: the path these sizes take by default) — same bits — and what the final solve costs with each.  The LPs are those of
tests/test_gpu_large_rows.py; per schedule one warm-up solve, then three.  lu_cross = 1 / 2 name 16 / 32 register slots where a lane
holds four rows (up to 8192 rows); eight rows per lane always have 16.
usage: lu_large_check.py [rows ...]   (4097 8200 12288)"""
import sys, os; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from gomilp_amd import lp
from tests.test_gpu_large_rows import _gen
sizes = [int(a) for a in sys.argv[1:]] or [4097, 8200, 12288]
SCHEDULES = [("per column", dict(lu_blocked=0)), ("lu_large 16 slots", dict(lu_large=1, lu_cross=1)), ("lu_large 32 slots", dict(lu_large=1, lu_cross=2))]
bad = 0
for m in sizes:
    nv = m // 2 if m > 8200 else 2 * m
    c, A, b = _gen(m, nv, 0)
    res = {}
    for name, knobs in SCHEDULES:
        if m > 8192 and knobs.get("lu_cross") == 2: continue   # (eight rows per lane: 16 slots)
        cx = lp.Context(**knobs)
        p = cx.upload(c, A, b)
        p.solve(0.0)
        runs = [p.solve(0.0) for _ in range(3)]
        cx.close()
        res[name] = runs[0]
        for i, r in enumerate(runs):
            s = r.stats
            print("m %5d %-18s run %d: status %d pivots %d seconds_final_solve %.4f seconds_final_device %.4f seconds_final_host %.4f lu_rounds %d lu_dense_steps %d retries %d" % (
                m, name, i, r.status, s["pivots_phase1"] + s["pivots_phase2"], s["seconds_final_solve"], s["seconds_final_device"], s["seconds_final_host"],
                s["lu_rounds"], s["lu_dense_steps"], s["device_retries"]), flush=True)
    a = res["per column"]
    for name, g in res.items():
        same = a.status == g.status and np.array_equal(a.basis, g.basis) and a.x.tobytes() == g.x.tobytes() and a.z == g.z
        if name != "per column": print("m %5d %-18s same bits as per column: %s" % (m, name, same), flush=True)
        bad += 0 if same else 1
print("TOTAL mismatches", bad)
