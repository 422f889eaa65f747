"""The C ABI of rt_render_aov_views, rt_render_motion_views and rt_denoise_batch without a GPU: the six entry points exist,
rt_motion_prev_views has the header's layout, every rejection that can be told from the arguments alone comes before any
device work and writes nothing, and a valid call answers RT_ERR_NO_DEVICE (a context exists only where a device does,
so the handle is never looked at here)."""
import ctypes as C
import os
import subprocess

import numpy as np
import torch

import pyrt

ROOT = pyrt.ROOT
NAMES = ("rt_render_aov_views", "rt_render_aov_views_device", "rt_render_motion_views", "rt_render_motion_views_device",
         "rt_denoise_batch", "rt_denoise_batch_device")
INVALID, NO_DEVICE, UNSUPPORTED = 1, 2, 4
W, H, N = 12, 8, 3
FAKE = C.c_void_p(1)

def test_entry_points_exist():
    L = pyrt.amd()
    for name in NAMES:
        assert hasattr(L, name) and name in pyrt.AMD_SYMBOLS


def test_error_codes_are_the_headers():
    text = open(os.path.join(ROOT, "include", "rt_amd.h")).read()
    for name, code in (("RT_ERR_INVALID", INVALID), ("RT_ERR_NO_DEVICE", NO_DEVICE), ("RT_ERR_UNSUPPORTED", UNSUPPORTED)):
        assert "%s = %d" % (name, code) in " ".join(text.split()), name


def test_prev_views_struct_matches_header(tmp_path):
    src = tmp_path / "layout.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rt_amd.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(rt_motion_prev_views));']
    for n, _ in pyrt.MotionPrevViews._fields_:
        lines.append('  printf("%%s %%zu\\n", "%s", offsetof(rt_motion_prev_views, %s));' % (n, n))
    lines += ["  return 0;", "}"]
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(pyrt.MotionPrevViews) == 40
    for n, _ in pyrt.MotionPrevViews._fields_:
        assert int(got[n]) == getattr(pyrt.MotionPrevViews, n).offset, n


class Buffers:
    """Host buffers of the three calls for N views of W x H, every one filled with 3."""

    def __init__(self):
        f = lambda *s: np.full(s, 3.0, np.float32)
        u = lambda *s: np.full(s, 3, np.uint32)
        self.aov = dict(albedo=f(N, H, W, 3), normal=f(N, H, W, 3), position=f(N, H, W, 3), depth=f(N, H, W), hits=u(N, H, W),
                        mesh=u(N, H, W), tri=u(N, H, W))
        self.mot = dict(motion=f(N, H, W, 2), position=f(N, H, W, 3), prev_position=f(N, H, W, 3), mesh=u(N, H, W))
        self.rgb, self.out = f(N, H, W, 3), f(N, H, W, 3)
        self.a, self.m = pyrt.Aov(), pyrt.Motion()
        for k, v in self.aov.items():
            setattr(self.a, k, v.ctypes.data)
        for k, v in self.mot.items():
            setattr(self.m, k, v.ctypes.data)

    def untouched(self):
        return all((x == 3).all() for x in list(self.aov.values()) + list(self.mot.values()) + [self.rgb, self.out])


def cameras(n=N):
    return np.arange(n * 12, dtype=np.float32).reshape(n, 4, 3) + 1


def aov_calls(L, b):
    """[(name, call(ctx, p, v, out))] of the two AOV forms."""
    ref = lambda x: None if x is None else C.byref(x)
    return [("host", lambda c, p, v, o=b.a: L.rt_render_aov_views(c, ref(p), ref(v), ref(o))),
            ("device", lambda c, p, v, o=b.a: L.rt_render_aov_views_device(c, ref(p), ref(v), ref(o), None))]


def motion_calls(L, b):
    ref = lambda x: None if x is None else C.byref(x)
    return [("host", lambda c, p, v, pr, o=b.m: L.rt_render_motion_views(c, ref(p), ref(v), ref(pr), ref(o))),
            ("device", lambda c, p, v, pr, o=b.m: L.rt_render_motion_views_device(c, ref(p), ref(v), ref(pr), ref(o), None))]


BAD_PARAMS = [(dict(width=0), INVALID), (dict(height=0), INVALID), (dict(width=65536), INVALID), (dict(spp=0), INVALID),
              (dict(spp_begin=3, spp_count=2), INVALID), (dict(tile=4), INVALID), (dict(rank=2, world=2), INVALID),
              (dict(world=2), UNSUPPORTED), (dict(rng_mode=pyrt.RNG_LEGACY), UNSUPPORTED)]


def params(**kw):
    base = dict(width=W, height=H, spp=4)
    base.update(kw)
    w, h, spp = base.pop("width"), base.pop("height"), base.pop("spp")
    return pyrt.make_params(w, h, spp, **base)


def bad_views():
    """[(what, views, keep-alive, word expected in rt_last_error)]"""
    out = []
    v, k = pyrt.make_views(cameras())
    v.reserved0 = 1
    out.append(("reserved0", v, k, b"reserved"))
    v, k = pyrt.make_views(cameras())
    v.reserved[5] = 1
    out.append(("reserved", v, k, b"reserved"))
    v, k = pyrt.make_views(cameras())
    v.n_views = 0
    out.append(("n_views 0", v, k, b"n_views"))
    v, k = pyrt.make_views(cameras())
    v.n_views = 65536
    out.append(("n_views 65536", v, k, b"n_views"))
    v = pyrt.Views()
    v.n_views = N
    out.append(("no cameras", v, None, b"null"))
    for bad in (np.nan, np.inf):
        cams = cameras()
        cams[2, 3, 1] = bad
        v, k = pyrt.make_views(cams)
        out.append(("non-finite camera", v, k, b"view 2"))
    return out


def test_aov_views_rejections_come_before_any_device_work():
    L, b = pyrt.amd(), Buffers()
    v, _keep = pyrt.make_views(cameras(), seeds=[1, 2, 40000])
    p = params()
    for name, call in aov_calls(L, b):
        assert call(None, p, v) == INVALID and b"null" in L.rt_last_error(), name
        assert call(FAKE, None, v) == INVALID, name
        assert call(FAKE, p, None) == INVALID, name
        assert call(FAKE, p, v, None) == INVALID, name
        b.a.reserved[3] = 1
        assert call(FAKE, p, v) == INVALID and b"reserved" in L.rt_last_error(), name
        b.a.reserved[3] = 0
        for kw, code in BAD_PARAMS:
            assert call(FAKE, params(**kw), v) == code, (name, kw)
        for what, bv, _k, word in bad_views():
            assert call(FAKE, p, bv) == INVALID and word in L.rt_last_error(), (name, what)
        # 2^31 pixels or more over the views
        many, _k = pyrt.make_views(np.repeat(cameras(1), 40000, axis=0))
        assert call(FAKE, params(width=256, height=256), many) == INVALID and b"2^31" in L.rt_last_error(), name
    assert b.untouched()


def test_motion_views_rejections_come_before_any_device_work():
    L, b = pyrt.amd(), Buffers()
    v, _keep = pyrt.make_views(cameras())
    p, prev = params(), pyrt.MotionPrevViews()
    for name, call in motion_calls(L, b):
        assert call(None, p, v, prev) == INVALID and b"null" in L.rt_last_error(), name
        assert call(FAKE, None, v, prev) == INVALID, name
        assert call(FAKE, p, None, prev) == INVALID, name
        assert call(FAKE, p, v, None) == INVALID, name
        assert call(FAKE, p, v, prev, None) == INVALID, name
        bad = pyrt.MotionPrevViews()
        bad.reserved[0] = 1
        assert call(FAKE, p, v, bad) == INVALID and b"reserved" in L.rt_last_error(), name
        b.m.reserved[2] = 1
        assert call(FAKE, p, v, prev) == INVALID and b"reserved" in L.rt_last_error(), name
        b.m.reserved[2] = 0
        for kw, code in BAD_PARAMS:
            assert call(FAKE, params(**kw), v, prev) == code, (name, kw)
        for what, bv, _k, word in bad_views():
            assert call(FAKE, p, bv, prev) == INVALID and word in L.rt_last_error(), (name, what)
        for x in (np.nan, -np.inf):
            pc = cameras()
            pc[1, 0, 2] = x
            nonfinite = pyrt.MotionPrevViews()
            nonfinite.cameras = C.cast(pc.ctypes.data, C.POINTER(pyrt.Camera))
            assert call(FAKE, p, v, nonfinite) == INVALID, name
            assert b"view 1" in L.rt_last_error() and b"previous camera" in L.rt_last_error(), name
    assert b.untouched()


def denoise_call(L, b, device, ctx=FAKE, d=None, n=N, rgb=True, aov=True, out=True):
    d = pyrt.Context._denoise_params(W, H, 0, 0., 0., 0.) if d is None else d
    ptr = lambda x: x.ctypes.data_as(C.c_void_p)
    args = [ctx, C.byref(d) if d is not False else None, n, ptr(b.rgb) if rgb else None, C.byref(b.a) if aov else None,
            ptr(b.out) if out else None]
    return L.rt_denoise_batch_device(*args, None) if device else L.rt_denoise_batch(*args)


def test_denoise_batch_rejections_come_before_any_device_work():
    L, b = pyrt.amd(), Buffers()
    for device in (False, True):
        assert denoise_call(L, b, device, ctx=None) == INVALID and b"null" in L.rt_last_error()
        assert denoise_call(L, b, device, d=False) == INVALID
        assert denoise_call(L, b, device, rgb=False) == INVALID
        assert denoise_call(L, b, device, aov=False) == INVALID
        assert denoise_call(L, b, device, out=False) == INVALID
        for k in ("albedo", "normal", "position", "hits"):
            keep = getattr(b.a, k)
            setattr(b.a, k, None)
            assert denoise_call(L, b, device) == INVALID and b"channels" in L.rt_last_error(), k
            setattr(b.a, k, keep)
        b.a.reserved[0] = 1
        assert denoise_call(L, b, device) == INVALID and b"reserved" in L.rt_last_error()
        b.a.reserved[0] = 0
        for kw in (dict(width=0), dict(height=0), dict(width=65536), dict(iterations=9), dict(sigma_color=-1.0),
                   dict(sigma_normal=np.nan), dict(sigma_position=np.inf)):
            d = pyrt.Context._denoise_params(W, H, 0, 0., 0., 0.)
            for k, x in kw.items():
                setattr(d, k, x)
            assert denoise_call(L, b, device, d=d) == INVALID, kw
        d = pyrt.Context._denoise_params(W, H, 0, 0., 0., 0.)
        d.reserved[4] = 1
        assert denoise_call(L, b, device, d=d) == INVALID and b"reserved" in L.rt_last_error()
        assert denoise_call(L, b, device, n=0) == INVALID and b"n_frames" in L.rt_last_error()
        big = pyrt.Context._denoise_params(32768, 32768, 0, 0., 0., 0.)
        assert denoise_call(L, b, device, d=big, n=2) == INVALID and b"2^31" in L.rt_last_error()
        assert denoise_call(L, b, device, d=pyrt.Context._denoise_params(1, 1, 0, 0., 0., 0.), n=1 << 31) == INVALID
    assert b.untouched()


def test_valid_calls_answer_no_device_or_run():
    """Without a device a valid call answers RT_ERR_NO_DEVICE and never looks at the handle; with one, the same arguments
    on a real context succeed."""
    L, b = pyrt.amd(), Buffers()
    have = torch.cuda.is_available()
    ctx = pyrt.Context(pyrt.Scene("cubes", W, H)) if have else None
    handle, want = (ctx._h, pyrt.RT_OK) if have else (FAKE, NO_DEVICE)
    cams = np.repeat(pyrt.Scene("cubes", W, H).arrays()["camera"][None], N, axis=0)
    v, _keep = pyrt.make_views(cams, seeds=[1, 2, 40000])
    prev = pyrt.MotionPrevViews()
    prev.cameras = C.cast(cams.ctypes.data, C.POINTER(pyrt.Camera))
    # (the photon fields and the wavefront bit do not matter to these passes: still valid)
    # (with a device only the host forms: the buffers are host memory)
    forms = slice(0, 1) if have else slice(0, 2)
    for p in (params(), params(use_photons=1, k=300, photons_requested=0, wavefront=True, max_depth=9, mode=7)):
        for name, call in aov_calls(L, b)[forms]:
            assert call(handle, p, v) == want, (name, L.rt_last_error())
        for name, call in motion_calls(L, b)[forms]:
            assert call(handle, p, v, prev) == want and call(handle, p, v, pyrt.MotionPrevViews()) == want, (name, L.rt_last_error())
    if have:
        assert denoise_call(L, b, False, ctx=handle) == pyrt.RT_OK, L.rt_last_error()
        ctx.close()
        return
    for device in (False, True):
        assert denoise_call(L, b, device) == NO_DEVICE
        assert denoise_call(L, b, device, n=(1 << 31) // (W * H) - 1) == NO_DEVICE  # (just below 2^31 pixels)
    assert b.untouched()
