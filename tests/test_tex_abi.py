"""The C ABI of rt_set_textures, rt_render_textured and rt_render_aov_textured without a GPU: the entry points exist,
every rejection that can be told from the arguments alone comes before any device work, in the header's order, and
writes nothing, and a valid frame call answers RT_ERR_NO_DEVICE (a context exists only where a device does, so the handle
is never looked at here).  The rejections that read the context — counts that are not the context's, no resident set —
need a context: tests/test_gpu_tex.py."""
import ctypes as C
import os

import numpy as np
import torch

import pyrt
from test_vcol_abi import BAD_PARAMS, FAKE, Buffers, H, INVALID, NO_DEVICE, W, params

ROOT = pyrt.ROOT
NAMES = ("rt_set_textures", "rt_render_textured", "rt_render_textured_device", "rt_render_aov_textured",
         "rt_render_aov_textured_device")
F32 = np.float32


def test_entry_points_exist_and_the_abi_version_stays():
    L = pyrt.amd()
    for name in NAMES:
        assert hasattr(L, name) and name in pyrt.AMD_SYMBOLS
    text = " ".join(open(os.path.join(ROOT, "include", "rt_amd.h")).read().split())
    assert "#define RT_ABI_VERSION 2" in text and L.rt_abi_version() == 2
    for name in NAMES:
        assert "int %s(rt_ctx* ctx" % name in text, name
    assert "#define RT_TEX_NONE 0xffffffffu" in text
    assert "enum { RT_TEX_REPEAT = 0, RT_TEX_CLAMP = 1 };" in text and "enum { RT_TEX_NEAREST = 0, RT_TEX_BILINEAR = 1 };" in text
    # the header's list of stream orders names the device forms
    assert text.count("rt_render_textured_device") >= 3 and text.count("rt_render_aov_textured_device") >= 2
    for name in ("set_textures", "render_textured", "render_textured_device", "render_aov_textured", "render_aov_textured_device"):
        assert callable(getattr(pyrt.Context, name))
    # the structures are the header's: five words, three reserved, a pointer; three counts, three pointers, four words
    assert C.sizeof(pyrt.Texture) == 40 and pyrt.Texture.texels.offset == 32
    assert C.sizeof(pyrt.TextureSet) == 56 and pyrt.TextureSet.textures.offset == 16 and pyrt.TextureSet.reserved.offset == 40
    assert (pyrt.TEX_NONE, pyrt.TEX_REPEAT, pyrt.TEX_CLAMP, pyrt.TEX_NEAREST, pyrt.TEX_BILINEAR) == (0xffffffff, 0, 1, 0, 1)


def calls(L, bufs):
    ref = lambda x: None if x is None else C.byref(x)
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

    def host(c, p, bg=bufs.bg, out=bufs.out, acc=bufs.acc):
        return L.rt_render_textured(c, ref(p), ptr(bg), ptr(out), ptr(acc), None)

    def device(c, p, acc=bufs.acc, **_):
        return L.rt_render_textured_device(c, ref(p), ptr(acc), None, None)

    return [("host", host), ("device", device)]


def test_frame_rejections_come_before_any_device_work():
    """rt_render_colors' order and codes (tests/test_vcol_abi.py's list of parameters)."""
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
    assert host(FAKE, params(world=2)) == 4 and b"textured" in L.rt_last_error()
    assert bufs.untouched()


def good_set():
    """A valid set of two textures (5x3 and 2x2) for 3 meshes and 6 vertices, as Context.set_textures' arguments."""
    tex = [dict(texels=np.full((3, 5, 3), 0.5, F32), wrap_s=pyrt.TEX_CLAMP, filter=pyrt.TEX_NEAREST), np.full((2, 2, 3), 0.25, F32)]
    return tex, np.array([1, pyrt.TEX_NONE, 0], np.uint32), np.linspace(-2, 2, 12).astype(F32).reshape(6, 2)


def refused(ts, *words):
    L = pyrt.amd()
    assert L.rt_set_textures(FAKE, C.byref(ts)) == INVALID
    msg = L.rt_last_error()
    for w in words:
        assert w in msg, (w, msg)


def test_set_textures_rejections_name_the_first_bad_value():
    L = pyrt.amd()
    assert L.rt_set_textures(None, None) == INVALID and b"null" in L.rt_last_error()
    # a valid set passes every argument check: the handle is looked at next
    ts, keep = pyrt.texture_set(*good_set())
    assert L.rt_set_textures(None, C.byref(ts)) == INVALID and b"ctx" in L.rt_last_error()
    # null pointers
    for field in ("textures", "mesh_texture", "vertex_uv"):
        ts, keep = pyrt.texture_set(*good_set())
        setattr(ts, field, None)
        refused(ts, b"null")
    ts, keep = pyrt.texture_set(*good_set())
    ts.n_textures = 0
    refused(ts, b"n_textures is 0")
    ts, keep = pyrt.texture_set(*good_set())
    ts.reserved[2] = 7
    refused(ts, b"reserved[2]", b"7")
    # per texture: the sizes, the wraps, the filter, the reserved words, the texel pointer — the first offender is named
    for field, value, words in (("width", 0, (b"texture 1", b"width 0")), ("width", 16385, (b"texture 1", b"width 16385")),
                                ("height", 0, (b"texture 1", b"height 0")), ("height", 70000, (b"texture 1", b"height 70000")),
                                ("wrap_s", 2, (b"texture 1", b"wrap_s 2")), ("wrap_t", 9, (b"texture 1", b"wrap_t 9")),
                                ("filter", 2, (b"texture 1", b"filter 2")), ("texels", None, (b"texture 1", b"texels is null"))):
        ts, keep = pyrt.texture_set(*good_set())
        setattr(ts.textures[1], field, value)
        refused(ts, *words)
    ts, keep = pyrt.texture_set(*good_set())
    ts.textures[0].reserved[1] = 3
    ts.textures[1].width = 0  # (a later bad value is not the one named)
    refused(ts, b"texture 0", b"reserved[1]")
    # a texel that is not finite: the first one, with its row, column and component
    for j, v in ((0, float("nan")), (22, float("inf")), (44, float("-inf"))):
        tex, mt, uv = good_set()
        tex[0]["texels"].reshape(-1)[j] = v
        tex[1].reshape(-1)[5] = float("nan")
        ts, keep = pyrt.texture_set(tex, mt, uv)
        refused(ts, b"texture 0", b"texels[%d]" % j, b"row %d, column %d, component %d" % (j // 3 // 5, j // 3 % 5, j % 3))
    tex, mt, uv = good_set()
    tex[1].reshape(-1)[5] = float("nan")
    ts, keep = pyrt.texture_set(tex, mt, uv)
    refused(ts, b"texture 1", b"texels[5]", b"row 0, column 1, component 2")
    # a mesh's index that is neither a texture nor RT_TEX_NONE
    for bad in (2, 0xfffffffe):
        tex, mt, uv = good_set()
        mt[2] = bad
        mt[1] = pyrt.TEX_NONE
        ts, keep = pyrt.texture_set(tex, mt, uv)
        refused(ts, b"mesh_texture[2]", b"%d" % bad)
    # a uv that is not finite or beyond 1024
    for j, v, shown in ((3, float("nan"), b"nan"), (0, float("inf"), b"inf"), (7, 1024.5, b"1024.5"), (11, -1025.0, b"-1025")):
        tex, mt, uv = good_set()
        uv.reshape(-1)[j] = v
        uv.reshape(-1)[11] = v if j == 11 else float("nan")
        ts, keep = pyrt.texture_set(tex, mt, uv)
        refused(ts, b"vertex_uv[%d]" % j, b"vertex %d, component %d" % (j // 2, j % 2), shown)
    tex, mt, uv = good_set()
    uv[0], uv[5] = (1024.0, -1024.0), (-1024.0, 1024.0)  # (the limit itself passes)
    ts, keep = pyrt.texture_set(tex, mt, uv)
    assert L.rt_set_textures(None, C.byref(ts)) == INVALID and b"ctx" in L.rt_last_error()


def test_a_set_of_more_than_2_to_the_28_texels_is_refused_before_a_texel_is_read():
    """Two 16384 x 16384 headers over one small array: the total is checked from the headers alone."""
    L = pyrt.amd()
    tex, mt, uv = good_set()
    ts, keep = pyrt.texture_set(tex, mt, uv)
    for k in range(2):
        ts.textures[k].width = ts.textures[k].height = 16384
    assert L.rt_set_textures(FAKE, C.byref(ts)) == INVALID
    msg = L.rt_last_error()
    assert b"536870912 texels" in msg and b"texture 1" in msg and b"268435456" in msg, msg


def test_aov_forms_refuse_null_arguments():
    L = pyrt.amd()
    p, a = params(), pyrt.Aov()
    assert L.rt_render_aov_textured(None, C.byref(p), C.byref(a)) == INVALID
    assert L.rt_render_aov_textured_device(None, C.byref(p), C.byref(a), None) == INVALID


def test_valid_calls_answer_no_device_or_run():
    """Without a device a valid frame call answers RT_ERR_NO_DEVICE and never looks at the handle; with one, the same
    arguments on a context with a resident set succeed (the host form: the buffers are host memory)."""
    L, bufs = pyrt.amd(), Buffers()
    have = torch.cuda.is_available()
    scene = pyrt.Scene("cubes", W, H)
    ctx = pyrt.Context(scene) if have else None
    if have:
        d = scene.desc
        ctx.set_textures([np.full((2, 3, 3), 0.5, F32)], np.zeros(d.n_meshes, np.uint32), np.full((d.n_vertices, 2), 0.3, F32))
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
