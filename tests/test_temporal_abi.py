"""rt_render_motion's and rt_temporal_accumulate's C ABI without a GPU: the entry points exist, the ctypes views of the
four structs have the header's layout, and the null, reserved-word, range and aliasing checks that come before any device
work answer RT_ERR_INVALID and write nothing."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pyrt

ROOT = pyrt.ROOT
NAMES = ("rt_render_motion", "rt_render_motion_device", "rt_temporal_accumulate", "rt_temporal_accumulate_device")
STRUCTS = [("rt_motion_prev", "MotionPrev", 40), ("rt_motion", "Motion", 48), ("rt_temporal_params", "TemporalParams", 44),
           ("rt_history", "History", 32)]
W, H = 12, 8


def test_entry_points_exist():
    L = pyrt.amd()
    for name in NAMES:
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
    """Host buffers of one rt_temporal_accumulate call, every one filled with 3."""

    def __init__(self):
        f = lambda *s: np.full(s, 3.0, np.float32)
        u = lambda *s: np.full(s, 3, np.uint32)
        self.cur_rgb, self.out_rgb, self.out_len = f(H, W, 3), f(H, W, 3), f(H, W)
        self.cur = dict(motion=f(H, W, 2), position=f(H, W, 3), prev_position=f(H, W, 3), mesh=u(H, W))
        self.hist = dict(rgb=f(H, W, 3), position=f(H, W, 3), mesh=u(H, W), length=f(H, W))
        self.m, self.h = pyrt.Motion(), pyrt.History()
        for k, v in self.cur.items():
            setattr(self.m, k, v.ctypes.data)
        for k, v in self.hist.items():
            setattr(self.h, k, v.ctypes.data)

    def untouched(self):
        arrays = [self.cur_rgb, self.out_rgb, self.out_len] + list(self.cur.values()) + list(self.hist.values())
        return all((a == 3).all() for a in arrays)


def test_motion_null_and_bad_arguments_are_invalid_without_a_device():
    L = pyrt.amd()
    p = pyrt.make_params(W, H, 4)
    fr = Frame()
    prev = pyrt.MotionPrev()
    fake = C.c_void_p(1)  # (a context handle is never dereferenced before the other arguments are checked)
    for fn, tail in ((L.rt_render_motion, ()), (L.rt_render_motion_device, (None,))):
        assert fn(None, C.byref(p), C.byref(prev), C.byref(fr.m), *tail) == 1
        assert b"null" in L.rt_last_error()
        assert fn(fake, None, C.byref(prev), C.byref(fr.m), *tail) == 1
        assert fn(fake, C.byref(p), None, C.byref(fr.m), *tail) == 1
        assert fn(fake, C.byref(p), C.byref(prev), None, *tail) == 1
        bad = pyrt.MotionPrev()
        bad.reserved[5] = 1
        assert fn(fake, C.byref(p), C.byref(bad), C.byref(fr.m), *tail) == 1
        assert b"reserved" in L.rt_last_error()
        fr.m.reserved[0] = 1
        assert fn(fake, C.byref(p), C.byref(prev), C.byref(fr.m), *tail) == 1
        fr.m.reserved[0] = 0
        for v in (np.nan, np.inf):
            cam = np.ones((4, 3), np.float32)
            cam[2, 1] = v
            nonfinite = pyrt.MotionPrev()
            nonfinite.camera = C.cast(cam.ctypes.data, C.POINTER(pyrt.Camera))
            assert fn(fake, C.byref(p), C.byref(nonfinite), C.byref(fr.m), *tail) == 1
            assert b"finite" in L.rt_last_error()
    assert fr.untouched()


def test_temporal_null_bad_and_aliasing_arguments_are_invalid_without_a_device():
    L = pyrt.amd()
    fake = C.c_void_p(1)

    def call(fr, t, device=False, ctx=fake, t_null=False, cur_rgb=True, cur=True, hist=True, out_rgb=None, out_len=None):
        args = [ctx, None if t_null else C.byref(t), ptr(fr.cur_rgb) if cur_rgb else None, C.byref(fr.m) if cur else None,
                C.byref(fr.h) if hist else None, out_rgb if out_rgb is not None else ptr(fr.out_rgb),
                out_len if out_len is not None else ptr(fr.out_len)]
        return L.rt_temporal_accumulate_device(*args, None) if device else L.rt_temporal_accumulate(*args)

    for device in (False, True):
        fr, t = Frame(), pyrt.make_temporal(W, H)
        assert call(fr, t, device, ctx=None) == 1 and b"null" in L.rt_last_error()
        assert call(fr, t, device, t_null=True) == 1
        assert call(fr, t, device, cur_rgb=False) == 1
        assert call(fr, t, device, cur=False) == 1
        assert call(fr, t, device, hist=False) == 1
        assert call(fr, t, device, out_rgb=C.c_void_p(None)) == 1
        assert call(fr, t, device, out_len=C.c_void_p(None)) == 1
        # required channels
        for k in ("motion", "prev_position", "mesh"):
            keep = getattr(fr.m, k)
            setattr(fr.m, k, None)
            assert call(fr, t, device) == 1 and b"channels" in L.rt_last_error(), k
            setattr(fr.m, k, keep)
        for k in pyrt.HISTORY_CHANNELS:
            keep = getattr(fr.h, k)
            setattr(fr.h, k, None)
            assert call(fr, t, device) == 1 and b"history" in L.rt_last_error(), k
            setattr(fr.h, k, keep)
        # sizes, sigma, alpha, reserved
        for kw in (dict(width=0), dict(height=0), dict(width=65536), dict(height=70000), dict(sigma_position=-1.0),
                   dict(sigma_position=np.nan), dict(sigma_position=np.inf), dict(alpha_min=-0.5), dict(alpha_min=np.nan),
                   dict(alpha_min=np.inf), dict(alpha_min=1.5)):
            bad = pyrt.make_temporal(W, H)
            for k, v in kw.items():
                setattr(bad, k, v)
            assert call(fr, bad, device) == 1, kw
        bad = pyrt.make_temporal(W, H)
        bad.reserved[2] = 7
        assert call(fr, bad, device) == 1 and b"reserved" in L.rt_last_error()
        # the outputs must not alias the history: the same pointer, and a buffer that merely overlaps one
        for k in pyrt.HISTORY_CHANNELS:
            assert call(fr, t, device, out_rgb=ptr(fr.hist[k])) == 1 and b"alias" in L.rt_last_error(), k
            assert call(fr, t, device, out_len=ptr(fr.hist[k])) == 1 and b"alias" in L.rt_last_error(), k
        inside = C.c_void_p(fr.hist["rgb"].ctypes.data + 4 * (3 * W * H - 1))  # the history's last float
        assert call(fr, t, device, out_len=inside) == 1 and b"alias" in L.rt_last_error()
        assert fr.untouched()
