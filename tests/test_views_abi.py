"""rt_render_views' C ABI without a GPU: the entry points exist, the ctypes view of rt_views has the header's layout, and
the null-argument checks that come before any device work answer RT_ERR_INVALID and write nothing."""
import ctypes as C
import os
import subprocess

import numpy as np

import pyrt

ROOT = pyrt.ROOT


def test_views_entry_points_exist():
    L = pyrt.amd()
    for name in ("rt_render_views", "rt_render_views_device"):
        assert hasattr(L, name) and name in pyrt.AMD_SYMBOLS


def test_views_struct_matches_header(tmp_path):
    """sizeof and field offsets of rt_views as the C compiler lays them out."""
    src = tmp_path / "layout.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rt_amd.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(rt_views));']
    for n, _ in pyrt.Views._fields_:
        lines.append('  printf("%%s %%zu\\n", "%s", offsetof(rt_views, %s));' % (n, n))
    lines += ["  return 0;", "}"]
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(pyrt.Views) == 48
    for n, _ in pyrt.Views._fields_:
        assert int(got[n]) == getattr(pyrt.Views, n).offset, n


def test_make_views_layout():
    cams = np.arange(2 * 12, dtype=np.float32).reshape(2, 4, 3)
    v, keep = pyrt.make_views(cams, seeds=[5, 9])
    assert v.n_views == 2 and v.reserved0 == 0 and list(v.reserved) == [0] * 6
    assert list(v.cameras[1].lower_left) == [15., 16., 17.] and (v.seeds[0], v.seeds[1]) == (5, 9)
    v, _ = pyrt.make_views(cams)
    assert not v.seeds


def test_null_arguments_are_invalid_without_a_device():
    L = pyrt.amd()
    p = pyrt.make_params(16, 16, 4)
    cams = np.zeros((1, 4, 3), np.float32)
    v, _keep = pyrt.make_views(cams)
    st = pyrt.Stats()
    st.rays_closest = 7
    out = np.full((1, 16, 16, 3), 3.0, np.float32)
    acc = np.full((1, 16, 16, 4), 3.0, np.float32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.rt_render_views(None, C.byref(p), C.byref(v), None, ptr(out), ptr(acc), C.byref(st)) == 1
    assert b"null" in L.rt_last_error()
    assert L.rt_render_views_device(None, C.byref(p), C.byref(v), ptr(acc), None, C.byref(st)) == 1
    # (a context handle is never dereferenced before the other pointers are checked: none of these reach it)
    fake = C.c_void_p(1)
    assert L.rt_render_views(fake, None, C.byref(v), None, ptr(out), ptr(acc), C.byref(st)) == 1
    assert L.rt_render_views(fake, C.byref(p), None, None, ptr(out), ptr(acc), C.byref(st)) == 1
    nocam = pyrt.Views()
    nocam.n_views = 1
    assert L.rt_render_views(fake, C.byref(p), C.byref(nocam), None, ptr(out), ptr(acc), C.byref(st)) == 1
    assert L.rt_render_views_device(fake, C.byref(p), C.byref(nocam), ptr(acc), None, C.byref(st)) == 1
    # a rejected call writes nothing
    assert st.rays_closest == 7 and (out == 3.0).all() and (acc == 3.0).all()
