"""lp.FrontierStats mirrors gomilp_frontier_stats of include/gomilp_lp.h: the field the batched revised simplex's artificial exchange
added (art_exchanges) is the last one, and the ctypes structure has the size a C compiler gives the header's struct."""
import ctypes
import os
import shutil
import subprocess

from gomilp_amd import lp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_frontier_stats_ends_with_art_exchanges():
    name, ctype = lp.FrontierStats._fields_[-1]
    assert name == "art_exchanges" and ctype is ctypes.c_int64
    assert lp.FrontierStats._fields_[-2][0] == "pivots_dual"


def test_frontier_stats_size_matches_the_header(tmp_path):
    cc = next((p for p in (shutil.which("cc"), shutil.which("gcc"), shutil.which("clang"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc")
               if p and os.path.exists(p)), None)
    assert cc, "no C compiler found"
    src, exe = tmp_path / "size.c", tmp_path / "size"
    src.write_text('#include <stdio.h>\n#include "gomilp_lp.h"\n'
                   'int main(void) { printf("%zu %zu\\n", sizeof(gomilp_frontier_stats), offsetof(gomilp_frontier_stats, art_exchanges)); return 0; }\n')
    subprocess.run([cc, "-x", "c", "-I", os.path.join(ROOT, "include"), "-include", "stddef.h", str(src), "-o", str(exe)], check=True)
    size, off = (int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert ctypes.sizeof(lp.FrontierStats) == size
    assert lp.FrontierStats.art_exchanges.offset == off == size - 8
