"""rt_bvh_quality_get / rt_rebuild's C ABI without a GPU: the entry points exist, the ctypes views have the header's layout,
and the argument checks that come before any device work answer RT_ERR_INVALID."""
import ctypes as C
import os
import subprocess

import pytest

import pyrt

ROOT = pyrt.ROOT
STRUCTS = (("rt_bvh_quality", pyrt.BvhQuality), ("rt_rebuild_params", pyrt.RebuildParams), ("rt_rebuild_report", pyrt.RebuildReport))


def test_rebuild_entry_points_exist():
    L = pyrt.amd()
    for name in ("rt_bvh_quality_get", "rt_rebuild"):
        assert hasattr(L, name) and name in pyrt.AMD_SYMBOLS
    assert L.rt_abi_version() == 2


def test_rebuild_structs_match_header(tmp_path):
    """sizeof and field offsets of the three new structs as the C compiler lays them out."""
    src = tmp_path / "layout.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rt_amd.h"', "int main(void) {"]
    for st, cls in STRUCTS:
        lines.append('  printf("%%s %%zu\\n", "%s", sizeof(%s));' % (st, st))
        for n, _ in cls._fields_:
            lines.append('  printf("%%s.%%s %%zu\\n", "%s", "%s", offsetof(%s, %s));' % (st, n, st, n))
    lines += ["  return 0;", "}"]
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for st, cls in STRUCTS:
        assert int(got[st]) == C.sizeof(cls)
        for n, _ in cls._fields_:
            assert int(got["%s.%s" % (st, n)]) == getattr(cls, n).offset, (st, n)


def test_null_arguments_are_invalid_without_a_device():
    L = pyrt.amd()
    rep = pyrt.RebuildReport()
    rep.rebuilt, rep.cost_after = 7, 3.0
    assert L.rt_rebuild(None, None, C.byref(rep)) == 1 and rep.rebuilt == 0 and rep.cost_after == 0.0
    assert b"null" in L.rt_last_error()
    assert L.rt_rebuild(None, C.byref(pyrt.RebuildParams()), None) == 1 and b"null" in L.rt_last_error()
    q = pyrt.BvhQuality()
    assert L.rt_bvh_quality_get(None, C.byref(q)) == 1 and b"null" in L.rt_last_error()


@pytest.mark.parametrize("ratio", [0.5, float("nan"), float("inf"), -1.0, float.fromhex("0x1.fffffep-1")])
def test_bad_min_ratio_is_invalid_before_the_context(ratio):
    """min_ratio in (0, 1), negative or non-finite: refused on the parameters alone (the null context is not reached)."""
    L = pyrt.amd()
    p = pyrt.RebuildParams()
    p.min_ratio = ratio
    rep = pyrt.RebuildReport()
    rep.rebuilt = 7
    assert L.rt_rebuild(None, C.byref(p), C.byref(rep)) == 1 and rep.rebuilt == 0
    assert b"min_ratio" in L.rt_last_error()


def test_reserved_words_must_be_zero():
    L = pyrt.amd()
    for i in range(7):
        p = pyrt.RebuildParams()
        p.reserved[i] = 1
        assert L.rt_rebuild(None, C.byref(p), None) == 1 and b"reserved" in L.rt_last_error()
    for ok in (0.0, 1.0, 1.5):  # valid parameters reach the context check
        p = pyrt.RebuildParams()
        p.min_ratio = ok
        assert L.rt_rebuild(None, C.byref(p), None) == 1 and b"null" in L.rt_last_error()
