"""The C ABI of rt_render_shutter without a GPU: the entry points exist, rt_shutter has the header's layout, every
rejection that can be told from the arguments alone comes before any device work and writes nothing, and a valid call
answers RT_ERR_NO_DEVICE (a context exists only where a device does, so the handle is never looked at here).  The
rejections that read the context's camera — the origin bound, the axes and the fs rule — need a context:
tests/test_gpu_shutter.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import torch

import pyrt

ROOT = pyrt.ROOT
NAMES = ("rt_render_shutter", "rt_render_shutter_device")
INVALID, NO_DEVICE, UNSUPPORTED = 1, 2, 4
W, H = 5, 3
FAKE = C.c_void_p(1)
CAM = np.array([[0.5, 0.25, 4.0], [-1.5, -1.0, 2.0], [3.0, 0.0, 0.0], [0.0, 2.0, 0.0]], np.float32)


def test_entry_points_exist_and_the_abi_version_stays():
    L = pyrt.amd()
    for name in NAMES:
        assert hasattr(L, name) and name in pyrt.AMD_SYMBOLS
    text = " ".join(open(os.path.join(ROOT, "include", "rt_amd.h")).read().split())
    assert "#define RT_ABI_VERSION 2" in text and L.rt_abi_version() == 2
    assert "typedef struct rt_shutter {" in text
    pix = " ".join(open(os.path.join(ROOT, "include", "rt_pixelmode.h")).read().split())
    assert "#define RT_STREAM_SHUTTER 4u" in pix
    # the header's list of stream orders names the device form in both places
    assert text.count("rt_render_shutter_device") >= 4


def test_struct_matches_header(tmp_path):
    src = tmp_path / "layout.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rt_amd.h"', '#include "rt_pixelmode.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(rt_shutter));', '  printf("stream %u\\n", RT_STREAM_SHUTTER);']
    for n, _t in pyrt.Shutter._fields_:
        lines.append('  printf("%s %%zu\\n", offsetof(rt_shutter, %s));' % (n, n))
    lines += ["  return 0;", "}"]
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(pyrt.Shutter) == 80
    assert int(got["stream"]) == 4
    for n, _t in pyrt.Shutter._fields_:
        assert int(got[n]) == getattr(pyrt.Shutter, n).offset, n


def test_make_shutter_fills_the_record():
    s = pyrt.make_shutter(CAM, 0.25, 0.5, 0.1, 2.0)
    assert np.array_equal(np.frombuffer(bytes(s)[:48], np.float32).reshape(4, 3), CAM)
    assert (s.open, s.close, s.aperture, s.focus_distance) == (0.25, 0.5, np.float32(0.1), 2.0) and not any(s.reserved)
    d = pyrt.make_shutter(CAM)
    assert (d.open, d.close, d.aperture, d.focus_distance) == (0.0, 1.0, 0.0, 0.0)


class Buffers:
    """The arrays of a call for a W x H frame; every output filled with 3."""

    def __init__(self):
        self.bg = np.full((H, W, 3), 0.5, np.float32)
        self.out = np.full((H, W, 3), 3.0, np.float32)
        self.acc = np.full((H, W, 4), 3.0, np.float32)

    def untouched(self):
        return (self.out == 3).all() and (self.acc == 3).all()


def calls(L, bufs):
    ref = lambda x: None if x is None else C.byref(x)
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

    def host(c, p, s, bg=bufs.bg, out=bufs.out, acc=bufs.acc):
        return L.rt_render_shutter(c, ref(p), ref(s), ptr(bg), ptr(out), ptr(acc), None)

    def device(c, p, s, acc=bufs.acc, **_):
        return L.rt_render_shutter_device(c, ref(p), ref(s), ptr(acc), None, None)

    return [("host", host), ("device", device)]


def params(**kw):
    base = dict(spp=4, width=W, height=H)
    base.update(kw)
    spp, w, h = base.pop("spp"), base.pop("width"), base.pop("height")
    return pyrt.make_params(w, h, spp, **base)


BAD_PARAMS = [(dict(spp=0), INVALID), (dict(spp_begin=3, spp_count=2), INVALID), (dict(tile=4), INVALID),
              (dict(rank=2, world=2), INVALID), (dict(mode=2), INVALID), (dict(width=0), INVALID), (dict(height=70000), INVALID),
              (dict(max_depth=0), UNSUPPORTED), (dict(max_depth=4), UNSUPPORTED), (dict(world=2), UNSUPPORTED),
              (dict(rng_mode=pyrt.RNG_LEGACY), UNSUPPORTED), (dict(use_photons=1, k=4, photons_requested=100), UNSUPPORTED),
              (dict(wavefront=True), UNSUPPORTED)]
NAN, INF = float("nan"), float("inf")
# (open, close)
BAD_EXPOSURES = [(-0.1, 1.0), (0.0, 1.5), (0.6, 0.5), (NAN, 1.0), (0.0, NAN), (0.0, INF), (-INF, 1.0), (1.0000001, 1.0000001),
                 (-1e-30, 0.5)]
# (aperture, focus_distance, a word of the message)
BAD_LENSES = [(-0.1, 1.0, b"aperture"), (NAN, 1.0, b"aperture"), (INF, 1.0, b"aperture"), (-INF, 1.0, b"aperture"),
              (0.1, 0.0, b"focus_distance"), (0.1, -2.0, b"focus_distance"), (0.1, NAN, b"focus_distance"),
              (0.1, INF, b"focus_distance"), (1e-30, -0.0, b"focus_distance")]


def test_rejections_come_before_any_device_work():
    L, bufs = pyrt.amd(), Buffers()
    p, sh = params(), pyrt.make_shutter(CAM, 0.0, 1.0, 0.1, 2.0)
    for name, call in calls(L, bufs):
        assert call(None, p, sh) == INVALID and b"null" in L.rt_last_error(), name
        assert call(FAKE, None, sh) == INVALID and b"null" in L.rt_last_error(), name
        assert call(FAKE, p, None) == INVALID and b"null" in L.rt_last_error(), name
        for j in range(4):
            bad = pyrt.make_shutter(CAM, 0.0, 1.0, 0.1, 2.0)
            bad.reserved[j] = 1
            assert call(FAKE, p, bad) == INVALID and b"reserved" in L.rt_last_error(), (name, j)
        for k in range(12):
            for v in (NAN, INF, -INF):
                cam = CAM.copy()
                cam.reshape(-1)[k] = v
                assert call(FAKE, p, pyrt.make_shutter(cam)) == INVALID and b"camera_close" in L.rt_last_error(), (name, k, v)
        for op, cl in BAD_EXPOSURES:
            assert call(FAKE, p, pyrt.make_shutter(CAM, op, cl)) == INVALID and b"exposure" in L.rt_last_error(), (name, op, cl)
        for a, f, word in BAD_LENSES:
            assert call(FAKE, p, pyrt.make_shutter(CAM, 0.0, 1.0, a, f)) == INVALID and word in L.rt_last_error(), (name, a, f, L.rt_last_error())
        for kw, code in BAD_PARAMS:
            for s in (sh, pyrt.make_shutter(CAM)):
                assert call(FAKE, params(**kw), s) == code, (name, kw, L.rt_last_error())
    host, device = calls(L, bufs)[0][1], calls(L, bufs)[1][1]
    assert host(FAKE, p, sh, out=None, acc=None) == INVALID and b"neither" in L.rt_last_error()
    assert host(FAKE, p, sh, bg=None) == INVALID and b"background" in L.rt_last_error()
    assert device(FAKE, p, sh, acc=None) == INVALID and b"d_accum" in L.rt_last_error()
    assert bufs.untouched()


def test_valid_calls_answer_no_device_or_run():
    """Without a device a valid call answers RT_ERR_NO_DEVICE and never looks at the handle; with one, the same arguments
    on a real context succeed (the host form: the buffers are host memory).  At aperture 0 the focus distance is ignored,
    whatever it holds, and the ends of the exposure rule are valid."""
    L, bufs = pyrt.amd(), Buffers()
    have = torch.cuda.is_available()
    scene = pyrt.Scene("cubes", W, H) if have else None
    ctx = pyrt.Context(scene) if have else None
    handle, want = (ctx._h, pyrt.RT_OK) if have else (FAKE, NO_DEVICE)
    B = CAM if not have else np.asarray(scene.arrays()["camera"], np.float32).reshape(4, 3) + np.float32(0.125)
    forms = slice(0, 1) if have else slice(0, 2)
    for p in (params(), params(spp=7, spp_begin=3, spp_count=4, mode=pyrt.MODE_RAY, max_depth=1),
              params(accel=pyrt.ACCEL_BRUTE, collect_stats=1, no_pool=True, lanes_per_pixel=4)):
        for sh in (pyrt.make_shutter(B, 0.0, 1.0, 0.1, 2.0), pyrt.make_shutter(B), pyrt.make_shutter(B, 0.0, 0.0), pyrt.make_shutter(B, 1.0, 1.0),
                   pyrt.make_shutter(B, 0.25, 0.5, 0.0, NAN), pyrt.make_shutter(B, 0.0, 1.0, 0.0, -1.0), pyrt.make_shutter(B, -0.0, 1.0, -0.0, 1.0)):
            for name, call in calls(L, bufs)[forms]:
                assert call(handle, p, sh) == want, (name, L.rt_last_error())
    host = calls(L, bufs)[0][1]
    assert host(handle, params(), pyrt.make_shutter(B, 0.0, 1.0, 0.1, 2.0), bg=None, out=None) == want  # (the accumulator alone)
    if have:
        ctx.close()
    else:
        assert bufs.untouched()
