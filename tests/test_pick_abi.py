"""The C ABI of rt_render_pick without a GPU: the entry points exist, rt_light_pick has the header's layout, every
rejection that can be told from the arguments alone comes before any device work and writes nothing, and a valid call
answers RT_ERR_NO_DEVICE (a context exists only where a device does, so the handle is never looked at here).  The
rejections that read the context — no lights, an n_importance that is not n_lights, a weight that is not finite — need a
context: tests/test_gpu_pick.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import torch

import pyrt

ROOT = pyrt.ROOT
NAMES = ("rt_render_pick", "rt_render_pick_device")
INVALID, NO_DEVICE, UNSUPPORTED = 1, 2, 4
W, H = 5, 3
FAKE = C.c_void_p(1)


def test_entry_points_exist_and_the_abi_version_stays():
    L = pyrt.amd()
    for name in NAMES:
        assert hasattr(L, name) and name in pyrt.AMD_SYMBOLS
    text = " ".join(open(os.path.join(ROOT, "include", "rt_amd.h")).read().split())
    assert "#define RT_ABI_VERSION 2" in text and L.rt_abi_version() == 2
    assert "typedef struct rt_light_pick {" in text and "#define RT_PICK_SLOTS_MAX 3" in text
    assert pyrt.PICK_SLOTS_MAX == 3
    pix = " ".join(open(os.path.join(ROOT, "include", "rt_pixelmode.h")).read().split())
    assert "#define RT_STREAM_PICK 5u" in pix
    # the header's list of stream orders names the device form in both places
    assert text.count("rt_render_pick_device") >= 3


def test_struct_matches_header(tmp_path):
    src = tmp_path / "layout.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rt_amd.h"', '#include "rt_pixelmode.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(rt_light_pick));', '  printf("max %d\\n", RT_PICK_SLOTS_MAX);',
             '  printf("stream %u\\n", RT_STREAM_PICK);']
    for n, _t in pyrt.LightPick._fields_:
        lines.append('  printf("%s %%zu\\n", offsetof(rt_light_pick, %s));' % (n, n))
    lines += ["  return 0;", "}"]
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(pyrt.LightPick) == 40
    assert int(got["max"]) == 3 and int(got["stream"]) == 5
    for n, _t in pyrt.LightPick._fields_:
        assert int(got[n]) == getattr(pyrt.LightPick, n).offset, n


def test_make_light_pick_fills_the_record():
    k = pyrt.make_light_pick(2)
    assert (k.slots, k.n_importance, k.importance) == (2, 0, None) and not any(k.reserved)
    q = [1.0, 0.0, 2.5]
    k = pyrt.make_light_pick(3, q)
    assert (k.slots, k.n_importance) == (3, 3)
    assert list(np.ctypeslib.as_array(C.cast(k.importance, C.POINTER(C.c_float)), (3,))) == q
    q[0] = 9.0  # (the record holds a copy)
    assert np.ctypeslib.as_array(C.cast(k.importance, C.POINTER(C.c_float)), (3,))[0] == 1.0


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

    def host(c, p, k, bg=bufs.bg, out=bufs.out, acc=bufs.acc):
        return L.rt_render_pick(c, ref(p), ref(k), ptr(bg), ptr(out), ptr(acc), None)

    def device(c, p, k, acc=bufs.acc, **_):
        return L.rt_render_pick_device(c, ref(p), ref(k), ptr(acc), None, None)

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


def test_rejections_come_before_any_device_work():
    L, bufs = pyrt.amd(), Buffers()
    p, pk = params(), pyrt.make_light_pick(2)
    three = pyrt.make_light_pick(3, [1.0, 2.0, 0.0])
    for name, call in calls(L, bufs):
        assert call(None, p, pk) == INVALID and b"null" in L.rt_last_error(), name
        assert call(FAKE, None, pk) == INVALID and b"null" in L.rt_last_error(), name
        assert call(FAKE, p, None) == INVALID and b"null" in L.rt_last_error(), name
        for m in (0, 4, 5, 0xffffffff):
            assert call(FAKE, p, pyrt.make_light_pick(m)) == INVALID and b"slots" in L.rt_last_error(), (name, m)
        for j in range(5):
            bad = pyrt.make_light_pick(1)
            bad.reserved[j] = 1
            assert call(FAKE, p, bad) == INVALID and b"reserved" in L.rt_last_error(), (name, j)
        # importance without n_importance, and the reverse
        bad = pyrt.make_light_pick(2, [1.0, 2.0])
        bad.n_importance = 0
        assert call(FAKE, p, bad) == INVALID and b"n_importance 0" in L.rt_last_error(), name
        bad = pyrt.make_light_pick(2)
        bad.n_importance = 2
        assert call(FAKE, p, bad) == INVALID and b"importance is null" in L.rt_last_error(), name
        # a negative or non-finite entry is named; an all-zero array
        for j, v in ((0, -1.0), (2, float("nan")), (1, float("inf")), (3, -0.5), (2, float("-inf"))):
            q = [1.0, 2.0, 3.0, 4.0]
            q[j] = v
            assert call(FAKE, p, pyrt.make_light_pick(2, q)) == INVALID, (name, j, v)
            assert b"importance[%d]" % j in L.rt_last_error(), (name, L.rt_last_error())
        assert call(FAKE, p, pyrt.make_light_pick(1, [0.0, 0.0, 0.0])) == INVALID and b"zero" in L.rt_last_error(), name
        assert call(FAKE, p, pyrt.make_light_pick(1, [0.0, -0.0])) == INVALID and b"zero" in L.rt_last_error(), name
        for kw, code in BAD_PARAMS:
            for k in (pk, three, pyrt.make_light_pick(1)):
                assert call(FAKE, params(**kw), k) == code, (name, kw, L.rt_last_error())
    host, device = calls(L, bufs)[0][1], calls(L, bufs)[1][1]
    assert host(FAKE, p, pk, out=None, acc=None) == INVALID and b"neither" in L.rt_last_error()
    assert host(FAKE, p, pk, bg=None) == INVALID and b"background" in L.rt_last_error()
    assert device(FAKE, p, pk, acc=None) == INVALID and b"d_accum" in L.rt_last_error()
    assert bufs.untouched()


def test_valid_calls_answer_no_device_or_run():
    """Without a device a valid call answers RT_ERR_NO_DEVICE and never looks at the handle — whatever n_importance is: how
    many lights there are is the context's to say; with one, the same arguments on a real context succeed (the host form:
    the buffers are host memory; importance arrays of the preset's three lights)."""
    L, bufs = pyrt.amd(), Buffers()
    have = torch.cuda.is_available()
    ctx = pyrt.Context(pyrt.Scene("cubes", W, H)) if have else None
    handle, want = (ctx._h, pyrt.RT_OK) if have else (FAKE, NO_DEVICE)
    forms = slice(0, 1) if have else slice(0, 2)
    tables = [pyrt.make_light_pick(1), pyrt.make_light_pick(2), pyrt.make_light_pick(3), pyrt.make_light_pick(2, [1.0, 0.0, 3.0]),
              pyrt.make_light_pick(3, [0.0, 0.0, 1e-30])]
    if not have:
        tables += [pyrt.make_light_pick(1, [1.0] * 200), pyrt.make_light_pick(3, [2.0])]
    for p in (params(), params(spp=7, spp_begin=3, spp_count=4, mode=pyrt.MODE_RAY, max_depth=1),
              params(accel=pyrt.ACCEL_BRUTE, collect_stats=1, no_pool=True, lanes_per_pixel=4)):
        for k in tables:
            for name, call in calls(L, bufs)[forms]:
                assert call(handle, p, k) == want, (name, L.rt_last_error())
    host = calls(L, bufs)[0][1]
    assert host(handle, params(), pyrt.make_light_pick(2), bg=None, out=None) == want  # (the accumulator alone)
    if have:
        ctx.close()
    else:
        assert bufs.untouched()
