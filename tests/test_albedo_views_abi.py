"""The C ABI of rt_render_views_shutter_albedo and rt_render_aov_views_albedo without a GPU: the four entry points exist,
RT_ABI_VERSION stays 2 and pyrt exposes the three RT_ALBEDO_* constants; every rejection that can be told from the
arguments alone comes before any device work, in rt_render_views_shutter's (rt_render_aov_views') order with the albedo
argument's check after the outputs (the reserved words) and before p, under every value of `albedo`, and writes nothing;
and a valid call answers RT_ERR_NO_DEVICE (a context exists only where a device does, so the handle is never looked at
here).  The rejections that read the context — no resident colours, no resident textures — need one:
tests/test_gpu_albedo_views.py."""
import ctypes as C
import os
import re

import numpy as np
import torch

import pyrt
from test_views_shutter_abi import (BAD_PARAMS, CAMS, FAKE, H, INVALID, N, NAN, NO_DEVICE, UNSUPPORTED, W, Buffers, bad_records,
                                    params, ptr, ref, shutters, views)

NAMES = ("rt_render_views_shutter_albedo", "rt_render_views_shutter_albedo_device", "rt_render_aov_views_albedo",
         "rt_render_aov_views_albedo_device")
ALBEDOS = (pyrt.ALBEDO_MATERIAL, pyrt.ALBEDO_COLORS, pyrt.ALBEDO_TEXTURES)
UNKNOWN = (3, 4, 0xffffffff)


def test_entry_points_exist_the_constants_match_and_the_abi_version_stays():
    L = pyrt.amd()
    text = " ".join(open(os.path.join(pyrt.ROOT, "include", "rt_amd.h")).read().split())
    assert "#define RT_ABI_VERSION 2" in text and L.rt_abi_version() == 2
    for name in NAMES:
        assert hasattr(L, name) and name in pyrt.AMD_SYMBOLS
        assert "int %s(rt_ctx* ctx" % name in text
    for name, value in (("MATERIAL", pyrt.ALBEDO_MATERIAL), ("COLORS", pyrt.ALBEDO_COLORS), ("TEXTURES", pyrt.ALBEDO_TEXTURES)):
        assert re.search(r"#define RT_ALBEDO_%s %du " % (name, value), text), name
    assert ALBEDOS == (0, 1, 2)
    for method in ("render_views_shutter_albedo", "render_views_shutter_albedo_device", "render_aov_views_albedo",
                   "render_aov_views_albedo_device"):
        assert callable(getattr(pyrt.Context, method))


def frame_calls(L, b, albedo):
    def host(c, p, v, sh, bg=b.bg, out=b.out, acc=b.acc, albedo=albedo):
        return L.rt_render_views_shutter_albedo(c, ref(p), ref(v), sh, albedo, ptr(bg), ptr(out), ptr(acc), C.byref(b.st))

    def device(c, p, v, sh, acc=b.acc, albedo=albedo, **_):
        return L.rt_render_views_shutter_albedo_device(c, ref(p), ref(v), sh, albedo, ptr(acc), None, C.byref(b.st))

    return [("host", host), ("device", device)]


def test_frame_rejections_come_before_any_device_work_in_the_stated_order():
    L, b = pyrt.amd(), Buffers()
    p, (v, _keep), sh = params(), views(), shutters()
    bad_p = params(spp=0)
    for albedo in ALBEDOS:
        for name, call in frame_calls(L, b, albedo):
            assert call(None, p, v, sh) == INVALID and b"null" in L.rt_last_error(), name
            assert call(FAKE, None, v, sh) == INVALID and b"null" in L.rt_last_error(), name
            assert call(FAKE, p, None, sh) == INVALID and b"null" in L.rt_last_error(), name
            nocam = pyrt.Views()
            nocam.n_views = N
            assert call(FAKE, p, nocam, sh) == INVALID and b"null" in L.rt_last_error(), name
            # a null shutters, also ahead of an unknown albedo
            for alb in (albedo, 3):
                assert call(FAKE, p, v, None, albedo=alb) == INVALID and b"shutters is null" in L.rt_last_error(), name
            # the unknown albedo: after the outputs (below), ahead of everything of p, v and the records
            for alb in UNKNOWN:
                for args in ((p, v, sh), (bad_p, v, sh), (params(world=2), v, sh), (p, views(n=0)[0], sh),
                             (p, v, shutters(**{"0": bad_records(CAMS[0])[0][0]}))):
                    assert call(FAKE, *args, albedo=alb) == INVALID, (name, alb)
                    assert b"albedo %d" % alb in L.rt_last_error() and b"RT_ALBEDO_TEXTURES" in L.rt_last_error(), L.rt_last_error()
            # then rt_render_views_shutter's own order: p, then v, then the views one by one
            assert call(FAKE, bad_p, views(n=0)[0], sh) == INVALID and b"n_views" not in L.rt_last_error(), name
            assert call(FAKE, p, views(n=0)[0], sh) == INVALID, name
            r0, _k0 = views()
            r0.reserved0 = 1
            assert call(FAKE, p, r0, sh) == INVALID and b"reserved" in L.rt_last_error(), name
            for kw, code in BAD_PARAMS + [(dict(spp_begin=3, spp_count=2), INVALID)]:
                assert call(FAKE, params(**kw), v, sh) == code, (name, kw, L.rt_last_error())
            for j in (0, N - 1):
                cams = CAMS.copy()
                cams[j, 2, 1] = NAN
                assert call(FAKE, p, views(cams)[0], sh) == INVALID and b"view %d" % j in L.rt_last_error(), (name, j)
                for rec, word in bad_records(CAMS[j]):
                    code = call(FAKE, p, v, shutters(**{str(j): rec}))
                    msg = L.rt_last_error()
                    assert code == INVALID and word in msg and b"view %d: " % j in msg, (name, j, msg)
        host, device = (c for _, c in frame_calls(L, b, albedo))
        for alb in (albedo, 3):  # (the outputs come ahead of the albedo argument)
            assert host(FAKE, p, v, sh, out=None, acc=None, albedo=alb) == INVALID and b"neither" in L.rt_last_error()
            assert host(FAKE, p, v, sh, bg=None, albedo=alb) == INVALID and b"background" in L.rt_last_error()
            assert device(FAKE, p, v, sh, acc=None, albedo=alb) == INVALID and b"d_accum" in L.rt_last_error()
    assert b.untouched()


class AovBuffers:
    """Every channel of N views of W x H, filled with 3."""

    def __init__(self):
        self.f3 = {k: np.full((N, H, W, 3), 3.0, np.float32) for k in ("albedo", "normal", "position")}
        self.depth = np.full((N, H, W), 3.0, np.float32)
        self.words = {k: np.full((N, H, W), 3, np.uint32) for k in ("hits", "mesh", "tri")}

    def aov(self):
        a = pyrt.Aov()
        for k, x in list(self.f3.items()) + [("depth", self.depth)] + list(self.words.items()):
            setattr(a, k, x.ctypes.data)
        return a

    def untouched(self):
        return all((x == 3).all() for x in list(self.f3.values()) + [self.depth] + list(self.words.values()))


def aov_calls(L, albedo):
    def host(c, p, v, a, albedo=albedo):
        return L.rt_render_aov_views_albedo(c, ref(p), ref(v), albedo, ref(a))

    def device(c, p, v, a, albedo=albedo):
        return L.rt_render_aov_views_albedo_device(c, ref(p), ref(v), albedo, ref(a), None)

    return [("host", host), ("device", device)]


def test_aov_rejections_come_before_any_device_work_in_the_stated_order():
    L, b = pyrt.amd(), AovBuffers()
    p, (v, _keep), a = params(), views(), b.aov()
    for albedo in ALBEDOS:
        for name, call in aov_calls(L, albedo):
            for args in ((None, p, v, a), (FAKE, None, v, a), (FAKE, p, None, a), (FAKE, p, v, None)):
                for alb in (albedo, 3):
                    assert call(*args, albedo=alb) == INVALID and b"null" in L.rt_last_error(), name
            nocam = pyrt.Views()
            nocam.n_views = N
            assert call(FAKE, p, nocam, a) == INVALID and b"null" in L.rt_last_error(), name
            for j in range(4):
                r = b.aov()
                r.reserved[j] = 1
                for alb in (albedo, 3):
                    assert call(FAKE, p, v, r, albedo=alb) == INVALID and b"reserved" in L.rt_last_error(), (name, j)
            for alb in UNKNOWN:
                for args in ((p, v), (params(spp=0), v), (params(world=2), v), (p, views(n=0)[0])):
                    assert call(FAKE, *args, a, albedo=alb) == INVALID and b"albedo %d" % alb in L.rt_last_error(), (name, alb)
            # then rt_render_aov_views' own checks
            for kw, code in ((dict(spp=0), INVALID), (dict(width=0), INVALID), (dict(spp_begin=3, spp_count=2), INVALID),
                             (dict(world=2), UNSUPPORTED)):
                assert call(FAKE, params(**kw), v, a) == code, (name, kw, L.rt_last_error())
            assert call(FAKE, p, views(n=0)[0], a) == INVALID, name
            for j in (0, N - 1):
                cams = CAMS.copy()
                cams[j, 0, 2] = NAN
                assert call(FAKE, p, views(cams)[0], a) == INVALID and b"view %d" % j in L.rt_last_error(), (name, j)
    assert b.untouched()


def test_valid_calls_answer_no_device():
    """Without a device a valid call answers RT_ERR_NO_DEVICE under each of the three albedo values and never looks at the
    handle (with one, the GPU tests make these calls on real contexts)."""
    if torch.cuda.is_available():
        return
    L, b, ab = pyrt.amd(), Buffers(), AovBuffers()
    for albedo in ALBEDOS:
        for p in (params(), params(spp=7, spp_begin=3, spp_count=4, mode=pyrt.MODE_RAY, max_depth=1),
                  params(accel=pyrt.ACCEL_BRUTE, collect_stats=1, no_pool=True, lanes_per_pixel=4)):
            for seeds in (None, [4, 5, 6]):
                v, _keep = views(seeds=seeds)
                for name, call in frame_calls(L, b, albedo):
                    assert call(FAKE, p, v, shutters()) == NO_DEVICE, (name, L.rt_last_error())
                for name, call in aov_calls(L, albedo):
                    assert call(FAKE, p, v, ab.aov()) == NO_DEVICE, (name, L.rt_last_error())
        host = frame_calls(L, b, albedo)[0][1]
        assert host(FAKE, params(), views()[0], shutters(), bg=None, out=None) == NO_DEVICE  # (the accumulator alone)
        only = pyrt.Aov()
        only.albedo = ab.f3["albedo"].ctypes.data
        assert aov_calls(L, albedo)[0][1](FAKE, params(), views()[0], only) == NO_DEVICE
    assert b.untouched() and ab.untouched()
