"""rt_update's C ABI without a GPU: the entry points exist, the ctypes views have the header's layout, and the argument
checks that come before any device work answer RT_ERR_INVALID."""
import ctypes as C
import os
import subprocess

import pyrt

ROOT = pyrt.ROOT


def test_update_entry_points_exist():
    L = pyrt.amd()
    for name in ("rt_update", "rt_update_vertices_device", "rt_group_update"):
        assert hasattr(L, name) and name in pyrt.AMD_SYMBOLS


def test_update_structs_match_header(tmp_path):
    """sizeof and field offsets of rt_scene_update / rt_update_report as the C compiler lays them out."""
    src = tmp_path / "layout.c"
    fields = {"rt_scene_update": [n for n, _ in pyrt.SceneUpdate._fields_],
              "rt_update_report": [n for n, _ in pyrt.UpdateReport._fields_]}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rt_amd.h"', "int main(void) {"]
    for st, names in fields.items():
        lines.append('  printf("%%s %%zu\\n", "%s", sizeof(%s));' % (st, st))
        for n in names:
            lines.append('  printf("%%s.%%s %%zu\\n", "%s", "%s", offsetof(%s, %s));' % (st, n, st, n))
    lines += ["  return 0;", "}"]
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for st, cls in (("rt_scene_update", pyrt.SceneUpdate), ("rt_update_report", pyrt.UpdateReport)):
        assert int(got[st]) == C.sizeof(cls)
        for n, _ in cls._fields_:
            assert int(got["%s.%s" % (st, n)]) == getattr(cls, n).offset, (st, n)


def test_null_arguments_are_invalid_without_a_device():
    L = pyrt.amd()
    u = pyrt.SceneUpdate()
    rep = pyrt.UpdateReport()
    rep.refitted = 7
    assert L.rt_update(None, C.byref(u), C.byref(rep)) == 1 and rep.refitted == 0
    assert b"null" in L.rt_last_error()
    assert L.rt_update_vertices_device(None, None, None, None, None) == 1
    assert L.rt_group_update(None, C.byref(u), None) == 1
