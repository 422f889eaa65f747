"""The C ABI of rt_set_normal_maps, rt_render_normal_mapped and rt_render_normal_mapped_device without a GPU: the entry
points exist, every rejection that can be told from the arguments alone comes before any device work, in the header's
order, and writes nothing, and a valid frame call answers RT_ERR_NO_DEVICE (a context exists only where a device does, so
the handle is never looked at here).  The rejections that read the context — a mesh count that is not the context's, no
resident set, an index beyond it, no maps, stale maps — need a context: tests/test_gpu_nmap.py."""
import ctypes as C
import os

import numpy as np
import torch

import pyrt
from test_vcol_abi import BAD_PARAMS, FAKE, Buffers, H, INVALID, NO_DEVICE, W, params

ROOT = pyrt.ROOT
NAMES = ("rt_set_normal_maps", "rt_render_normal_mapped", "rt_render_normal_mapped_device")
F32 = np.float32


def test_entry_points_exist_and_the_abi_version_stays():
    L = pyrt.amd()
    for name in NAMES:
        assert hasattr(L, name) and name in pyrt.AMD_SYMBOLS
    text = " ".join(open(os.path.join(ROOT, "include", "rt_amd.h")).read().split())
    assert "#define RT_ABI_VERSION 2" in text and L.rt_abi_version() == 2
    for name in NAMES:
        assert "int %s(rt_ctx* ctx" % name in text, name
    assert "typedef struct rt_normal_maps {" in text and "uint32_t reserved[6];" in text
    # the header's lists of stream orders name the device form: asynchronous, and synchronising with stats
    assert text.count("rt_render_normal_mapped_device") >= 3
    # the header lists the operations that form N' one by one
    for op in ("r = a1 * b2 - a2 * b1", "Tr = b2 * e1 - b1 * e2", "Br = a1 * e2 - a2 * e1", "Tp = Tr - dot3(N, Tr) * N", "T = unit3(Tp)",
               "B = cross3(N, T)", "x = 2 * m.r - 1", "V = (x * T + y * B) + z * N", "N' = unit3(V)"):
        assert op in text, op
    for name in ("set_normal_maps", "render_normal_mapped", "render_normal_mapped_device"):
        assert callable(getattr(pyrt.Context, name))
    # the structure is the header's: a count, one pointer, six words
    assert C.sizeof(pyrt.NormalMaps) == 40 and pyrt.NormalMaps.mesh_normal.offset == 8 and pyrt.NormalMaps.reserved.offset == 16


def calls(L, bufs):
    ref = lambda x: None if x is None else C.byref(x)
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

    def host(c, p, bg=bufs.bg, out=bufs.out, acc=bufs.acc):
        return L.rt_render_normal_mapped(c, ref(p), ptr(bg), ptr(out), ptr(acc), None)

    def device(c, p, acc=bufs.acc, **_):
        return L.rt_render_normal_mapped_device(c, ref(p), ptr(acc), None, None)

    return [("host", host), ("device", device)]


def test_frame_rejections_come_before_any_device_work():
    """rt_render_textured's order and codes (tests/test_vcol_abi.py's list of parameters)."""
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
    for kw in (dict(world=2), dict(use_photons=1, k=4, photons_requested=100), dict(wavefront=True)):
        assert host(FAKE, params(**kw)) == 4 and b"normal-mapped" in L.rt_last_error(), kw
        assert device(FAKE, params(**kw)) == 4 and b"normal-mapped" in L.rt_last_error(), kw
    assert bufs.untouched()


def test_set_normal_maps_rejections_in_the_headers_order():
    L = pyrt.amd()
    # a null maps with a null ctx
    assert L.rt_set_normal_maps(None, None) == INVALID and b"null" in L.rt_last_error()
    # a non-zero reserved word comes before the null ctx, and the first one is named
    for k in range(6):
        m, keep = pyrt.normal_maps(3, np.zeros(3, np.uint32))
        m.reserved[k] = 7 + k
        if k < 5:
            m.reserved[5] = 1  # (a later one is not the one named)
        for handle in (None, FAKE):
            assert L.rt_set_normal_maps(handle, C.byref(m)) == INVALID
            msg = L.rt_last_error()
            assert b"normal maps: reserved[%d]" % k in msg and b"%d" % (7 + k) in msg, msg
    # clean maps end at the null ctx, whatever their table
    for table in (None, np.zeros(3, np.uint32), np.full(3, pyrt.TEX_NONE, np.uint32), np.array([0, 99, 1], np.uint32)):
        m, keep = pyrt.normal_maps(3, table)
        assert L.rt_set_normal_maps(None, C.byref(m)) == INVALID and b"ctx" in L.rt_last_error()


def test_valid_calls_answer_no_device_or_run():
    """Without a device a valid frame call answers RT_ERR_NO_DEVICE and never looks at the handle; with one, the same
    arguments on a context with a resident set and normal maps (and no material maps) succeed (the host form: the buffers
    are host memory)."""
    L, bufs = pyrt.amd(), Buffers()
    have = torch.cuda.is_available()
    scene = pyrt.Scene("cubes", W, H)
    ctx = pyrt.Context(scene) if have else None
    if have:
        d = scene.desc
        ctx.set_textures([np.full((2, 3, 3), 0.5, F32)], np.zeros(d.n_meshes, np.uint32), np.full((d.n_vertices, 2), 0.3, F32))
        ctx.set_normal_maps(np.zeros(d.n_meshes, np.uint32))
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
