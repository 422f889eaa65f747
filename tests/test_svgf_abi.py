"""rt_svgf's C ABI without a GPU: the entry points exist, the ctypes views of the three structs have the header's layout,
every check that comes before any device work answers RT_ERR_INVALID and writes nothing, and a call that passes them
answers RT_ERR_NO_DEVICE where there is no device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pyrt

ROOT = pyrt.ROOT
STRUCTS = [("rt_svgf_params", "SvgfParams", 64), ("rt_svgf_history", "SvgfHistory", 40), ("rt_svgf_out", "SvgfOut", 64)]
W, H = 12, 8


def test_entry_points_exist():
    L = pyrt.amd()
    for name in ("rt_svgf", "rt_svgf_device"):
        assert hasattr(L, name) and name in pyrt.AMD_SYMBOLS


@pytest.mark.parametrize("cname,pyname,size", STRUCTS)
def test_struct_matches_header(tmp_path, cname, pyname, size):
    """sizeof and field offsets as the C compiler lays them out."""
    view = getattr(pyrt, pyname)
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
    """Host buffers of one rt_svgf call, every one filled with 3."""

    def __init__(self):
        f = lambda *s: np.full(s, 3.0, np.float32)
        u = lambda *s: np.full(s, 3, np.uint32)
        self.cur_rgb = f(H, W, 3)
        self.aov = dict(albedo=f(H, W, 3), normal=f(H, W, 3), position=f(H, W, 3), hits=u(H, W))
        self.cur = dict(motion=f(H, W, 2), position=f(H, W, 3), prev_position=f(H, W, 3), mesh=u(H, W))
        self.hist = dict(color=f(H, W, 3), moments=f(H, W, 2), position=f(H, W, 3), mesh=u(H, W), length=f(H, W))
        self.out = dict(rgb=f(H, W, 3), color=f(H, W, 3), moments=f(H, W, 2), length=f(H, W), accum=f(H, W, 3), variance=f(H, W))
        self.a, self.m, self.h, self.o = pyrt.Aov(), pyrt.Motion(), pyrt.SvgfHistory(), pyrt.SvgfOut()
        for st, d in ((self.a, self.aov), (self.m, self.cur), (self.h, self.hist), (self.o, self.out)):
            for k, v in d.items():
                setattr(st, k, v.ctypes.data)

    def untouched(self):
        arrays = [self.cur_rgb] + [v for d in (self.aov, self.cur, self.hist, self.out) for v in d.values()]
        return all((a == 3).all() for a in arrays)


def call(L, fr, s, device, ctx=C.c_void_p(1), skip=()):
    """(a context handle is never dereferenced before the other arguments are checked)"""
    args = [ctx, C.byref(s), ptr(fr.cur_rgb), C.byref(fr.a), C.byref(fr.m), C.byref(fr.h), C.byref(fr.o)]
    for i in skip:
        args[i] = None
    return L.rt_svgf_device(*args, None) if device else L.rt_svgf(*args)


@pytest.mark.parametrize("device", (False, True), ids=("host", "device"))
def test_null_bad_and_aliasing_arguments_are_invalid_and_write_nothing(device):
    L = pyrt.amd()
    fr, s = Frame(), pyrt.make_svgf(W, H)
    assert call(L, fr, s, device, ctx=None) == 1 and b"null" in L.rt_last_error()
    for i in range(1, 7):
        assert call(L, fr, s, device, skip=(i,)) == 1 and b"null" in L.rt_last_error(), i
    # required channels and outputs
    for st, names, word in ((fr.a, ("albedo", "normal", "position", "hits"), b"channels"),
                            (fr.m, ("motion", "prev_position", "mesh"), b"channels"),
                            (fr.h, pyrt.SVGF_HISTORY_CHANNELS, b"history"), (fr.o, ("rgb", "color", "moments", "length"), b"required")):
        for k in names:
            keep = getattr(st, k)
            setattr(st, k, None)
            assert call(L, fr, s, device) == 1 and word in L.rt_last_error(), k
            setattr(st, k, keep)
    # sizes, iterations, sigmas, alphas
    bads = [dict(width=0), dict(height=0), dict(width=65536), dict(height=70000), dict(iterations=9)]
    for k in ("sigma_luminance", "sigma_normal", "sigma_position", "sigma_reproject"):
        bads += [{k: -1.0}, {k: np.nan}, {k: np.inf}]
    for k in ("alpha_min", "alpha_min_moments"):
        bads += [{k: -0.5}, {k: np.nan}, {k: np.inf}, {k: 1.5}]
    for kw in bads:
        bad = pyrt.make_svgf(W, H)
        for k, v in kw.items():
            setattr(bad, k, v)
        assert call(L, fr, bad, device) == 1, kw
    # reserved words
    bad = pyrt.make_svgf(W, H)
    bad.reserved[2] = 7
    assert call(L, fr, bad, device) == 1 and b"reserved" in L.rt_last_error()
    for st in (fr.a, fr.m, fr.o):
        st.reserved[1] = 1
        assert call(L, fr, s, device) == 1 and b"reserved" in L.rt_last_error()
        st.reserved[1] = 0
    # every output against every history buffer and every other output: the same pointer, and a mere overlap
    outs = [k for k, _ in pyrt.SVGF_OUT_CHANNELS]
    for o in outs:
        keep = getattr(fr.o, o)
        for k in pyrt.SVGF_HISTORY_CHANNELS:
            setattr(fr.o, o, fr.hist[k].ctypes.data)
            assert call(L, fr, s, device) == 1 and b"alias" in L.rt_last_error(), (o, k)
        for k in outs:
            if k != o:
                setattr(fr.o, o, fr.out[k].ctypes.data)
                assert call(L, fr, s, device) == 1 and b"alias" in L.rt_last_error(), (o, k)
        setattr(fr.o, o, keep)
    fr.o.length = fr.hist["color"].ctypes.data + 4 * (3 * W * H - 1)  # the history's last float
    assert call(L, fr, s, device) == 1 and b"alias" in L.rt_last_error()
    fr.o.length = fr.out["moments"].ctypes.data + 4 * (2 * W * H - 1)
    assert call(L, fr, s, device) == 1 and b"alias" in L.rt_last_error()
    assert fr.untouched()


def _has_gpu():
    import torch
    return torch.cuda.device_count() > 0


@pytest.mark.skipif(_has_gpu(), reason="a GPU is present")
@pytest.mark.parametrize("device", (False, True), ids=("host", "device"))
def test_a_valid_call_without_a_device_is_no_device(device):
    """Also with the optional outputs left out and out.rgb aliasing cur_rgb, which is allowed."""
    L = pyrt.amd()
    fr, s = Frame(), pyrt.make_svgf(W, H, iterations=8, alpha_min=1.0, alpha_min_moments=0.2, sigma_luminance=4.0)
    assert call(L, fr, s, device) == 2 and b"no CPU path" in L.rt_last_error()
    fr.o.accum, fr.o.variance, fr.o.rgb = None, None, fr.cur_rgb.ctypes.data
    assert call(L, fr, s, device) == 2
    assert fr.untouched()
