"""Developer tool (diagnostic flavour: GOMILP_DEBUG_BUILD=1): cycles per segment of a dense step of the final-solve panel kernel.
usage: GOMILP_DEBUG_BUILD=1 python tools/lu_stamps.py M [knob=value ...]   (the one-workgroup panel: lu_cross=0 unless given; tools/lux_stamps.py stamps the cross-workgroup panel)"""
import sys, os, ctypes; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from gomilp_amd import lp, synth
name = sys.argv[1] if len(sys.argv) > 1 else "M"
m, seed = synth.CONFIGS[name]
c, A, b = synth.dense_lp_standard_form(m, seed)
knobs = {"lu_cross": 0}; knobs.update({k: int(v) for k, v in (a.split("=") for a in sys.argv[2:])})
cx = lp.Context(**knobs); p = cx.upload(c, A, b)
for _ in range(3):
    r = p.solve(0.0)
buf = (ctypes.c_ulonglong * 64)()
lp.lib().gomilp_debug_luc_stamps(buf)
a = np.array(buf[:], dtype=np.float64).reshape(4, 16)
steps = max(1.0, a[0, 15])
names = ["wave0 top", "barrier1", "retire", "own search", "barrier2", "wg pivot+publish", "barrier3", "elimination"]
print(name, knobs, "dense steps", int(steps), "final solve %.3f ms" % (1e3 * r.stats["seconds_final_solve"]))
for w in range(4):
    print("wave", w, " ".join("%s %.0f" % (names[i], a[w, i] / steps) for i in range(8)), "| sum %.0f cycles per dense step" % (a[w, :8].sum() / steps))
cx.close()
