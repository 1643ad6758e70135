"""The C-ABI of the single-context warm start (no GPU): gomilp_lp_solve_warm is exported, lp.py's mirror of gomilp_warm_stats has
the header's fields in the header's order and size, and gomilp_lp_stats keeps the size callers compiled against the old header pass."""
import ctypes as C
import os
import re

from gomilp_amd import lp

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "gomilp_lp.h")
CTYPES = {"int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double}


def _header_struct(name):
    src = open(HEADER).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        mm = re.match(r"\s*(int32_t|int64_t|double)\s+(\w+)(?:\[(\d+)\])?\s*$", decl)
        if mm:
            fields.append((mm.group(2), mm.group(1), int(mm.group(3) or 1)))
    return fields


def test_solve_warm_is_exported():
    L = lp.lib()
    assert hasattr(L, "gomilp_lp_solve_warm")
    assert "gomilp_lp_solve_warm" in lp.EXPORTS


def test_warm_stats_mirror_matches_header():
    fields = _header_struct("gomilp_warm_stats")
    assert [f[0] for f in fields] == [f[0] for f in lp.WarmStats._fields_]
    for (name, ctype, cnt), (pname, ptype) in zip(fields, lp.WarmStats._fields_):
        assert C.sizeof(ptype) == C.sizeof(CTYPES[ctype]) * cnt, name
    assert C.sizeof(lp.WarmStats) == 48


def test_lp_stats_size_unchanged():
    fields = _header_struct("gomilp_lp_stats")
    assert [f[0] for f in fields] == [f[0] for f in lp.Stats._fields_]
    assert C.sizeof(lp.Stats) == 200   # the size before the warm start: callers of gomilp_lp_solve_resident pass it
