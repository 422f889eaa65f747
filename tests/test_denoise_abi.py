"""rt_denoise's C ABI without a GPU: the entry points exist, the ctypes view of rt_denoise_params has the header's layout,
and every check that comes before the context is looked at answers RT_ERR_INVALID and writes nothing."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pyrt

ROOT = pyrt.ROOT
W, H = 12, 8
GUIDES = ("albedo", "normal", "position", "hits")


def test_entry_points_exist():
    L = pyrt.amd()
    for name in ("rt_denoise", "rt_denoise_device"):
        assert hasattr(L, name) and name in pyrt.AMD_SYMBOLS


def test_struct_matches_header(tmp_path):
    """sizeof and field offsets as the C compiler lays them out."""
    view, cname, size = pyrt.DenoiseParams, "rt_denoise_params", 48
    src = tmp_path / "layout.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rt_amd.h"', "int main(void) {",
             '  printf("size %%zu\\n", sizeof(%s));' % cname]
    for n, _ in view._fields_:
        lines.append('  printf("%%s %%zu\\n", "%s", offsetof(%s, %s));' % (n, cname, n))
    lines += ["  return 0;", "}"]
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(view) == size
    for n, _ in view._fields_:
        assert int(got[n]) == getattr(view, n).offset, n


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class Frame:
    """Host buffers of one rt_denoise call, every one filled with 3."""

    def __init__(self):
        f = lambda *s: np.full(s, 3.0, np.float32)
        self.rgb, self.out = f(H, W, 3), f(H, W, 3)
        self.aov = dict(albedo=f(H, W, 3), normal=f(H, W, 3), position=f(H, W, 3), hits=np.full((H, W), 3, np.uint32))
        self.a = pyrt.Aov()
        for k, v in self.aov.items():
            setattr(self.a, k, v.ctypes.data)

    def untouched(self):
        return all((a == 3).all() for a in [self.rgb, self.out] + list(self.aov.values()))


def params(width=W, height=H):
    d = pyrt.DenoiseParams()
    d.width, d.height = width, height
    return d


def call(L, fr, d, device, ctx=C.c_void_p(1), skip=()):
    """(the context handle is not a context: only calls that are refused before it is looked at)"""
    args = [ctx, C.byref(d), ptr(fr.rgb), C.byref(fr.a), ptr(fr.out)]
    for i in skip:
        args[i] = None
    return L.rt_denoise_device(*args, None) if device else L.rt_denoise(*args)


@pytest.mark.parametrize("device", (False, True), ids=("host", "device"))
def test_null_arguments_and_missing_guides_are_invalid_and_write_nothing(device):
    L = pyrt.amd()
    fr, d = Frame(), params()
    assert call(L, fr, d, device, ctx=None) == 1 and b"null" in L.rt_last_error()
    for i in range(1, 5):
        assert call(L, fr, d, device, skip=(i,)) == 1 and b"null" in L.rt_last_error(), i
    for k in GUIDES:
        keep = getattr(fr.a, k)
        setattr(fr.a, k, None)
        assert call(L, fr, d, device) == 1 and b"channels" in L.rt_last_error(), k
        setattr(fr.a, k, keep)
    assert fr.untouched()


def test_host_form_refuses_sizes_out_of_range_and_writes_nothing():
    """(rt_denoise_device looks at the context before the size: not for a handle that is no context)"""
    L = pyrt.amd()
    fr = Frame()
    for kw in (dict(width=0), dict(height=0), dict(width=65536), dict(height=70000)):
        assert call(L, fr, params(**kw), False) == 1 and b"out of range" in L.rt_last_error(), kw
    assert fr.untouched()
