"""The C ABI of rt_set_vertex_colors, rt_render_colors and rt_render_aov_colors without a GPU: the entry points exist,
every rejection that can be told from the arguments alone comes before any device work, in the header's order, and
writes nothing, and a valid frame call answers RT_ERR_NO_DEVICE (a context exists only where a device does, so the handle
is never looked at here).  The rejections that read the context — a vertex count that is not the context's, no resident
colours — need a context: tests/test_gpu_vcol.py."""
import ctypes as C
import os

import numpy as np
import torch

import pyrt

ROOT = pyrt.ROOT
NAMES = ("rt_set_vertex_colors", "rt_render_colors", "rt_render_colors_device", "rt_render_aov_colors",
         "rt_render_aov_colors_device")
INVALID, NO_DEVICE, UNSUPPORTED = 1, 2, 4
W, H = 5, 3
FAKE = C.c_void_p(1)


def test_entry_points_exist_and_the_abi_version_stays():
    L = pyrt.amd()
    for name in NAMES:
        assert hasattr(L, name) and name in pyrt.AMD_SYMBOLS
    text = " ".join(open(os.path.join(ROOT, "include", "rt_amd.h")).read().split())
    assert "#define RT_ABI_VERSION 2" in text and L.rt_abi_version() == 2
    for name in NAMES:
        assert "int %s(rt_ctx* ctx" % name in text, name
    # the header's list of stream orders names the device forms
    assert text.count("rt_render_colors_device") >= 3 and text.count("rt_render_aov_colors_device") >= 2
    for name in ("set_vertex_colors", "render_colors", "render_colors_device", "render_aov_colors", "render_aov_colors_device"):
        assert callable(getattr(pyrt.Context, name))


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

    def host(c, p, bg=bufs.bg, out=bufs.out, acc=bufs.acc):
        return L.rt_render_colors(c, ref(p), ptr(bg), ptr(out), ptr(acc), None)

    def device(c, p, acc=bufs.acc, **_):
        return L.rt_render_colors_device(c, ref(p), ptr(acc), None, None)

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


def test_frame_rejections_come_before_any_device_work():
    L, bufs = pyrt.amd(), Buffers()
    p = params()
    for name, call in calls(L, bufs):
        assert call(None, p) == INVALID and b"null" in L.rt_last_error(), name
        assert call(FAKE, None) == INVALID and b"null" in L.rt_last_error(), name
        for kw, code in BAD_PARAMS:
            assert call(FAKE, params(**kw)) == code, (name, kw, L.rt_last_error())
    host, device = calls(L, bufs)[0][1], calls(L, bufs)[1][1]
    # the form's own buffers come before p's numbers
    assert host(FAKE, params(spp=0), out=None, acc=None) == INVALID and b"neither" in L.rt_last_error()
    assert host(FAKE, p, bg=None) == INVALID and b"background" in L.rt_last_error()
    assert device(FAKE, params(world=2), acc=None) == INVALID and b"d_accum" in L.rt_last_error()
    # ... and an invalid p before an unsupported one
    assert host(FAKE, params(spp=0, world=2)) == INVALID
    assert bufs.untouched()


def test_set_vertex_colors_rejections_name_the_first_bad_value():
    L = pyrt.amd()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.rt_set_vertex_colors(None, None, 0) == INVALID and b"null" in L.rt_last_error()
    ok = np.full((6, 3), 0.5, np.float32)
    assert L.rt_set_vertex_colors(None, ptr(ok), 6) == INVALID and b"null" in L.rt_last_error()
    for j, v in ((0, float("nan")), (7, float("inf")), (17, float("-inf")), (4, float("nan"))):
        bad = ok.copy()
        bad.reshape(-1)[j] = v
        bad.reshape(-1)[17] = v if j == 17 else float("nan")  # (a later bad value is not the one named)
        assert L.rt_set_vertex_colors(FAKE, ptr(bad), 6) == INVALID
        msg = L.rt_last_error()
        assert b"rgb[%d]" % j in msg and b"vertex %d," % (j // 3) in msg, msg
    # no range is imposed: negative, zero and large finite values pass the argument checks (the handle is looked at next)
    wide = np.array([[-1.0, 0.0, 3e38]] * 2, np.float32)
    assert L.rt_set_vertex_colors(None, ptr(wide), 2) == INVALID and b"null" in L.rt_last_error()


def test_aov_forms_refuse_null_arguments():
    L = pyrt.amd()
    p, a = params(), pyrt.Aov()
    assert L.rt_render_aov_colors(None, C.byref(p), C.byref(a)) == INVALID
    assert L.rt_render_aov_colors_device(None, C.byref(p), C.byref(a), None) == INVALID


def test_valid_calls_answer_no_device_or_run():
    """Without a device a valid frame call answers RT_ERR_NO_DEVICE and never looks at the handle; with one, the same
    arguments on a context with resident colours succeed (the host form: the buffers are host memory)."""
    L, bufs = pyrt.amd(), Buffers()
    have = torch.cuda.is_available()
    scene = pyrt.Scene("cubes", W, H)
    ctx = pyrt.Context(scene) if have else None
    if have:
        ctx.set_vertex_colors(np.full((scene.desc.n_vertices, 3), 0.5, np.float32))
    handle, want = (ctx._h, pyrt.RT_OK) if have else (FAKE, NO_DEVICE)
    forms = slice(0, 1) if have else slice(0, 2)
    for p in (params(), params(spp=7, spp_begin=3, spp_count=4, mode=pyrt.MODE_RAY, max_depth=1),
              params(accel=pyrt.ACCEL_BRUTE, collect_stats=1, no_pool=True, lanes_per_pixel=4)):
        for name, call in calls(L, bufs)[forms]:
            assert call(handle, p) == want, (name, L.rt_last_error())
    host = calls(L, bufs)[0][1]
    assert host(handle, params(), bg=None, out=None) == want  # (the accumulator alone)
    if have:
        ctx.close()
    else:
        assert bufs.untouched()
