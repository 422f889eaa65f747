"""The C ABI of rt_render_lights without a GPU: the entry points exist, rt_light_groups has the header's layout, every
rejection that can be told from the arguments alone comes before any device work and writes nothing, and a valid call
answers RT_ERR_NO_DEVICE (a context exists only where a device does, so the handle is never looked at here).  The
rejections that read the context — a mask bit at or above n_lights — need a context: tests/test_gpu_lights.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import pyrt

ROOT = pyrt.ROOT
NAMES = ("rt_render_lights", "rt_render_lights_device")
INVALID, NO_DEVICE, UNSUPPORTED = 1, 2, 4
W, H, G = 5, 3, 4
FAKE = C.c_void_p(1)


def test_entry_points_exist_and_the_abi_version_stays():
    L = pyrt.amd()
    for name in NAMES:
        assert hasattr(L, name) and name in pyrt.AMD_SYMBOLS
    text = " ".join(open(os.path.join(ROOT, "include", "rt_amd.h")).read().split())
    assert "#define RT_ABI_VERSION 2" in text and L.rt_abi_version() == 2
    assert "typedef struct rt_light_groups {" in text and "#define RT_LIGHT_GROUPS_MAX 4" in text
    assert pyrt.LIGHT_GROUPS_MAX == 4
    # the header's list of stream orders names the device form in both places
    assert text.count("rt_render_lights_device") >= 3


def test_struct_matches_header(tmp_path):
    src = tmp_path / "layout.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rt_amd.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(rt_light_groups));', '  printf("max %d\\n", RT_LIGHT_GROUPS_MAX);']
    for n, _t in pyrt.LightGroups._fields_:
        lines.append('  printf("%s %%zu\\n", offsetof(rt_light_groups, %s));' % (n, n))
    lines += ["  return 0;", "}"]
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(pyrt.LightGroups) == 32
    assert int(got["max"]) == 4
    for n, _t in pyrt.LightGroups._fields_:
        assert int(got[n]) == getattr(pyrt.LightGroups, n).offset, n


def test_make_light_groups_fills_the_record():
    g = pyrt.make_light_groups([0b101, 0, 0b11])
    assert g.n_groups == 3 and list(g.masks) == [0b101, 0, 0b11, 0] and not any(g.reserved)
    assert pyrt.make_light_groups([7]).n_groups == 1
    with pytest.raises(ValueError):
        pyrt.make_light_groups([1, 2, 4, 8, 16])


class Buffers:
    """The arrays of a call for G slices of a W x H frame; every output filled with 3."""

    def __init__(self):
        self.bg = np.full((H, W, 3), 0.5, np.float32)
        self.out = np.full((G, H, W, 3), 3.0, np.float32)
        self.acc = np.full((G, H, W, 4), 3.0, np.float32)

    def untouched(self):
        return (self.out == 3).all() and (self.acc == 3).all()


def calls(L, bufs):
    ref = lambda x: None if x is None else C.byref(x)
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

    def host(c, p, g, bg=bufs.bg, out=bufs.out, acc=bufs.acc):
        return L.rt_render_lights(c, ref(p), ref(g), ptr(bg), ptr(out), ptr(acc), None)

    def device(c, p, g, acc=bufs.acc, **_):
        return L.rt_render_lights_device(c, ref(p), ref(g), ptr(acc), None, None)

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


def groups(masks, n=None):
    g = pyrt.LightGroups()
    g.n_groups = len(masks) if n is None else n
    for j, m in enumerate(masks):
        g.masks[j] = m
    return g


def test_rejections_come_before_any_device_work():
    L, bufs = pyrt.amd(), Buffers()
    p, gr = params(), groups([1, 2, 4])
    for name, call in calls(L, bufs):
        assert call(None, p, gr) == INVALID and b"null" in L.rt_last_error(), name
        assert call(FAKE, None, gr) == INVALID and b"null" in L.rt_last_error(), name
        assert call(FAKE, p, None) == INVALID and b"null" in L.rt_last_error(), name
        for n in (0, 5, 6, 0xffffffff):
            assert call(FAKE, p, groups([0, 0, 0, 0], n=n)) == INVALID and b"n_groups" in L.rt_last_error(), (name, n)
        for j in range(3):
            bad = groups([1, 2, 4])
            bad.reserved[j] = 1
            assert call(FAKE, p, bad) == INVALID and b"reserved" in L.rt_last_error(), (name, j)
        for n in (1, 2, 3):
            for j in range(n, 4):
                masks = [1] * n + [0] * (4 - n)
                masks[j] = 1 << (5 * j)
                assert call(FAKE, p, groups(masks, n=n)) == INVALID and b"beyond n_groups" in L.rt_last_error(), (name, n, j)
        for kw, code in BAD_PARAMS:
            for g in (gr, groups([0]), groups([0xffffffff, 0, 1, 3])):
                assert call(FAKE, params(**kw), g) == code, (name, kw, L.rt_last_error())
    host, device = calls(L, bufs)[0][1], calls(L, bufs)[1][1]
    assert host(FAKE, p, gr, out=None, acc=None) == INVALID and b"neither" in L.rt_last_error()
    assert host(FAKE, p, gr, bg=None) == INVALID and b"background" in L.rt_last_error()
    assert device(FAKE, p, gr, acc=None) == INVALID and b"d_accum" in L.rt_last_error()
    assert bufs.untouched()


def test_valid_calls_answer_no_device_or_run():
    """Without a device a valid call answers RT_ERR_NO_DEVICE and never looks at the handle — whatever bits the masks hold:
    which lights exist is the context's to say; with one, the same arguments on a real context succeed (the host form: the
    buffers are host memory; masks within the preset's three lights)."""
    L, bufs = pyrt.amd(), Buffers()
    have = torch.cuda.is_available()
    ctx = pyrt.Context(pyrt.Scene("cubes", W, H)) if have else None
    handle, want = (ctx._h, pyrt.RT_OK) if have else (FAKE, NO_DEVICE)
    forms = slice(0, 1) if have else slice(0, 2)
    tables = [groups([1, 2, 4]), groups([7]), groups([0]), groups([3, 6, 0, 7]), groups([5, 5])]
    if not have:
        tables += [groups([0xffffffff]), groups([1 << 31, 1 << 20])]
    for p in (params(), params(spp=7, spp_begin=3, spp_count=4, mode=pyrt.MODE_RAY, max_depth=1),
              params(accel=pyrt.ACCEL_BRUTE, collect_stats=1, no_pool=True, lanes_per_pixel=4)):
        for g in tables:
            for name, call in calls(L, bufs)[forms]:
                assert call(handle, p, g) == want, (name, L.rt_last_error())
    host = calls(L, bufs)[0][1]
    assert host(handle, params(), groups([1, 2]), bg=None, out=None) == want  # (the accumulators alone)
    if have:
        ctx.close()
    else:
        assert bufs.untouched()
