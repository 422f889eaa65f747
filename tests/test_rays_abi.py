"""The C ABI of rt_render_rays without a GPU: the entry points exist, rt_ray_batch has the header's layout, every
rejection that can be told from the arguments alone comes before any device work and writes nothing, and a valid call
answers RT_ERR_NO_DEVICE (a context exists only where a device does, so the handle is never looked at here)."""
import ctypes as C
import os
import subprocess

import numpy as np
import torch

import pyrt

ROOT = pyrt.ROOT
NAMES = ("rt_render_rays", "rt_render_rays_device")
INVALID, NO_DEVICE, UNSUPPORTED = 1, 2, 4
N = 5
FAKE = C.c_void_p(1)


def test_entry_points_exist_and_the_abi_version_stays():
    L = pyrt.amd()
    for name in NAMES:
        assert hasattr(L, name) and name in pyrt.AMD_SYMBOLS
    text = " ".join(open(os.path.join(ROOT, "include", "rt_amd.h")).read().split())
    assert "#define RT_ABI_VERSION 2" in text and L.rt_abi_version() == 2
    assert "typedef struct rt_ray_batch {" in text


def test_struct_matches_header(tmp_path):
    src = tmp_path / "layout.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rt_amd.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(rt_ray_batch));', '  printf("ray %zu\\n", sizeof(rt_ray));']
    for n, _t in pyrt.RayBatch._fields_:
        lines.append('  printf("%s %%zu\\n", offsetof(rt_ray_batch, %s));' % (n, n))
    lines += ["  return 0;", "}"]
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(pyrt.RayBatch) == 48
    assert int(got["ray"]) == pyrt.RAY_DTYPE.itemsize == 24
    for n, _t in pyrt.RayBatch._fields_:
        assert int(got[n]) == getattr(pyrt.RayBatch, n).offset, n


class Buffers:
    """The arrays of a call for N rays; every output filled with 3."""

    def __init__(self):
        self.rays = np.zeros(N, pyrt.RAY_DTYPE)
        self.rays["origin"] = [0.5, 0.25, -2.0]
        self.rays["direction"] = [[0, 0, 2.5], [1, 1, 1], [1e-3, 0, 1e-3], [0, -3, 0], [1e18, 1e18, 1e18]]
        self.index = np.arange(N, dtype=np.uint32)[::-1].copy()
        self.bg = np.full((N, 3), 0.5, np.float32)
        self.out = np.full((N, 3), 3.0, np.float32)
        self.acc = np.full((N, 4), 3.0, np.float32)

    def batch(self, n=N, rays=True, index=False):
        b = pyrt.RayBatch()
        b.n, b.rays, b.stream_index = n, self.rays.ctypes.data if rays else None, self.index.ctypes.data if index else None
        return b

    def untouched(self):
        return (self.out == 3).all() and (self.acc == 3).all()


def calls(L, bufs):
    ref = lambda x: None if x is None else C.byref(x)
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

    def host(c, p, b, bg=bufs.bg, out=bufs.out, acc=bufs.acc):
        return L.rt_render_rays(c, ref(p), ref(b), ptr(bg), ptr(out), ptr(acc), None)

    def device(c, p, b, acc=bufs.acc, **_):
        return L.rt_render_rays_device(c, ref(p), ref(b), ptr(acc), None, None)

    return [("host", host), ("device", device)]


def params(**kw):
    base = dict(spp=4)
    base.update(kw)
    spp, w, h = base.pop("spp"), base.pop("width", 0), base.pop("height", 0)
    return pyrt.make_params(w, h, spp, **base)


BAD_PARAMS = [(dict(spp=0), INVALID), (dict(spp_begin=3, spp_count=2), INVALID), (dict(tile=4), INVALID),
              (dict(rank=2, world=2), INVALID), (dict(mode=2), INVALID), (dict(max_depth=0), UNSUPPORTED),
              (dict(max_depth=4), UNSUPPORTED), (dict(world=2), UNSUPPORTED), (dict(rng_mode=pyrt.RNG_LEGACY), UNSUPPORTED),
              (dict(use_photons=1, k=4, photons_requested=100), UNSUPPORTED), (dict(wavefront=True), UNSUPPORTED)]


def test_rejections_come_before_any_device_work():
    L, bufs = pyrt.amd(), Buffers()
    p = params()
    for name, call in calls(L, bufs):
        b = bufs.batch()
        assert call(None, p, b) == INVALID and b"null" in L.rt_last_error(), name
        assert call(FAKE, None, b) == INVALID, name
        assert call(FAKE, p, None) == INVALID, name
        assert call(FAKE, p, bufs.batch(rays=False)) == INVALID and b"null" in L.rt_last_error(), name
        for n in (0, 1 << 31, (1 << 32) - 1):
            assert call(FAKE, p, bufs.batch(n=n)) == INVALID and b"outside" in L.rt_last_error(), (name, n)
        bad = bufs.batch()
        bad.reserved0 = 1
        assert call(FAKE, p, bad) == INVALID and b"reserved" in L.rt_last_error(), name
        for j in range(6):
            bad = bufs.batch()
            bad.reserved[j] = 1
            assert call(FAKE, p, bad) == INVALID and b"reserved" in L.rt_last_error(), (name, j)
        for kw, code in BAD_PARAMS:
            assert call(FAKE, params(**kw), b) == code, (name, kw, L.rt_last_error())
    host, device = calls(L, bufs)[0][1], calls(L, bufs)[1][1]
    b = bufs.batch()
    assert host(FAKE, p, b, out=None, acc=None) == INVALID and b"neither" in L.rt_last_error()
    assert host(FAKE, p, b, bg=None) == INVALID and b"background" in L.rt_last_error()
    assert device(FAKE, p, b, acc=None) == INVALID and b"d_accum" in L.rt_last_error()
    assert bufs.untouched()


def test_host_form_names_the_ray_it_refuses():
    """A non-finite origin, and a direction that cannot be normalised — null, not finite, or finite and so long that its
    squared length overflows float32 — are RT_ERR_INVALID in the host form, naming the ray; a direction whose squared
    length merely underflows, or lies just below the overflow, is fine."""
    L, bufs = pyrt.amd(), Buffers()
    host = calls(L, bufs)[0][1]
    p = params()
    good = bufs.rays.copy()
    big = np.float32(1.8e19)  # (3 big^2 = 9.7e38 overflows; 1e18's 3e36 does not)
    for r, field, value, word in ((2, "origin", [np.nan, 0, 0], b"origin"), (4, "origin", [0, np.inf, 0], b"origin"),
                                  (0, "origin", [0, 0, -np.inf], b"origin"), (1, "direction", [0, 0, 0], b"direction"),
                                  (3, "direction", [-0.0, 0.0, -0.0], b"direction"), (2, "direction", [np.nan, 1, 0], b"direction"),
                                  (4, "direction", [1, -np.inf, 0], b"direction"), (0, "direction", [big, big, big], b"direction"),
                                  (3, "direction", [0, 2e19, 0], b"direction")):
        bufs.rays[:] = good
        bufs.rays[field][r] = value
        assert host(FAKE, p, bufs.batch()) == INVALID, (r, field, value)
        err = L.rt_last_error()
        assert word in err and (b"ray %d:" % r) in err, err
    assert bufs.untouched()
    have = torch.cuda.is_available()
    ctx = pyrt.Context(pyrt.Scene("cubes", 8, 8)) if have else None
    handle, want = (ctx._h, pyrt.RT_OK) if have else (FAKE, NO_DEVICE)
    for value in ([1e-30, 0, 0], [1e19, 1e19, 0], [0, 0, -1e-45]):
        bufs.rays[:] = good
        bufs.rays["direction"][2] = value
        assert host(handle, p, bufs.batch()) == want, (value, L.rt_last_error())
    if have:
        ctx.close()


def test_valid_calls_answer_no_device_or_run():
    """Without a device a valid call answers RT_ERR_NO_DEVICE and never looks at the handle; with one, the same arguments
    on a real context succeed (the host form: the buffers are host memory).  width and height are ignored, whatever
    they hold."""
    L, bufs = pyrt.amd(), Buffers()
    have = torch.cuda.is_available()
    ctx = pyrt.Context(pyrt.Scene("cubes", 8, 8)) if have else None
    handle, want = (ctx._h, pyrt.RT_OK) if have else (FAKE, NO_DEVICE)
    forms = slice(0, 1) if have else slice(0, 2)
    for p in (params(), params(width=0, height=70000), params(spp=7, spp_begin=3, spp_count=4, mode=pyrt.MODE_RAY, max_depth=1),
              params(accel=pyrt.ACCEL_BRUTE, collect_stats=1, no_pool=True, lanes_per_pixel=4)):
        for b in (bufs.batch(), bufs.batch(index=True), bufs.batch(n=1)):
            for name, call in calls(L, bufs)[forms]:
                assert call(handle, p, b) == want, (name, L.rt_last_error())
    if have:
        ctx.close()
    else:
        assert bufs.untouched()
