"""The C ABI of rt_render_views_shutter and rt_render_adaptive_shutter without a GPU: the four entry points exist,
RT_ABI_VERSION stays 2 and the structs keep their layouts; every rejection that can be told from the arguments alone —
of both forms of both calls, with a bad shutter record at view 0 and at the last view only — comes before any device work
and writes nothing; and a valid call answers RT_ERR_NO_DEVICE (a context exists only where a device does, so the handle
is never looked at here).  The rejections that read the context and the view cameras need a context:
tests/test_gpu_views_shutter.py and tests/test_gpu_adaptive_shutter.py."""
import ctypes as C
import os

import numpy as np
import torch

import pyrt

ROOT = pyrt.ROOT
NAMES = ("rt_render_views_shutter", "rt_render_views_shutter_device", "rt_render_adaptive_shutter",
         "rt_render_adaptive_shutter_device")
INVALID, NO_DEVICE, UNSUPPORTED = 1, 2, 4
W, H, N = 5, 3, 3
FAKE = C.c_void_p(1)
CAM = np.array([[0.5, 0.25, 4.0], [-1.5, -1.0, 2.0], [3.0, 0.0, 0.0], [0.0, 2.0, 0.0]], np.float32)
CAMS = np.stack([CAM, CAM + np.float32(0.125), CAM + np.float32(0.25)])
NAN, INF = float("nan"), float("inf")
ref = lambda x: None if x is None else C.byref(x)
ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)


def test_entry_points_exist_and_the_abi_version_stays():
    L = pyrt.amd()
    for name in NAMES:
        assert hasattr(L, name) and name in pyrt.AMD_SYMBOLS
    text = " ".join(open(os.path.join(ROOT, "include", "rt_amd.h")).read().split())
    assert "#define RT_ABI_VERSION 2" in text and L.rt_abi_version() == 2
    for name in NAMES:
        assert "int %s(rt_ctx* ctx" % name in text
    # the layouts the calls share with rt_render_views, rt_render_shutter and rt_render_adaptive
    assert (C.sizeof(pyrt.Views), C.sizeof(pyrt.Shutter), C.sizeof(pyrt.AdaptiveParams)) == (48, 80, 40)


def test_make_shutters_copies_the_records():
    recs = [pyrt.make_shutter(CAMS[j], 0.0, 0.25 * j, 0.1 * j, 2.0) for j in range(N)]
    arr = pyrt.make_shutters(recs, N)
    assert C.sizeof(arr) == N * 80
    for j in range(N):
        assert bytes(arr[j]) == bytes(recs[j])
    try:
        pyrt.make_shutters(recs[:2], N)
    except ValueError:
        pass
    else:
        raise AssertionError("a short list of records was taken")


class Buffers:
    """The arrays of a call for N views of W x H; every output filled with 3."""

    def __init__(self):
        self.bg = np.full((H, W, 3), 0.5, np.float32)
        self.out = np.full((N, H, W, 3), 3.0, np.float32)
        self.acc = np.full((N, H, W, 4), 3.0, np.float32)
        self.spp = np.full((H, W), 3, np.uint32)
        self.rep = pyrt.AdaptiveReport()
        self.rep.passes = 7
        self.st = pyrt.Stats()
        self.st.rays_closest = 7

    def untouched(self):
        return ((self.out == 3).all() and (self.acc == 3).all() and (self.spp == 3).all() and self.rep.passes == 7
                and self.st.rays_closest == 7)


def params(**kw):
    base = dict(spp=4, width=W, height=H)
    base.update(kw)
    spp, w, h = base.pop("spp"), base.pop("width"), base.pop("height")
    return pyrt.make_params(w, h, spp, **base)


def shutters(**bad):
    """Three valid records (no optics, a lens at rest, a move with a lens); bad = {view: record} replaces some."""
    recs = [pyrt.make_shutter(CAMS[0], 0.0, 0.0), pyrt.make_shutter(CAMS[1], 0.0, 0.0, 0.1, 2.0),
            pyrt.make_shutter(CAMS[2] + np.float32(0.5), 0.0, 1.0, 0.1, 2.0)]
    for j, r in bad.items():
        recs[int(j)] = r
    return pyrt.make_shutters(recs, N)


def views(cams=CAMS, seeds=None, n=None):
    v, keep = pyrt.make_views(cams, seeds)
    if n is not None:
        v.n_views = n
    return v, keep


def view_calls(L, b):
    def host(c, p, v, sh, bg=b.bg, out=b.out, acc=b.acc):
        return L.rt_render_views_shutter(c, ref(p), ref(v), sh, ptr(bg), ptr(out), ptr(acc), C.byref(b.st))

    def device(c, p, v, sh, acc=b.acc, **_):
        return L.rt_render_views_shutter_device(c, ref(p), ref(v), sh, ptr(acc), None, C.byref(b.st))

    return [("host", host), ("device", device)]


def adaptive_calls(L, b):
    def host(c, p, a, sh, bg=b.bg, out=b.out, acc=b.acc):
        return L.rt_render_adaptive_shutter(c, ref(p), ref(a), ref(sh), ptr(bg), ptr(out), ptr(acc), ptr(b.spp), C.byref(b.rep), C.byref(b.st))

    def device(c, p, a, sh, bg=b.bg, out=b.out, acc=b.acc):
        return L.rt_render_adaptive_shutter_device(c, ref(p), ref(a), ref(sh), ptr(bg), ptr(acc), ptr(out), ptr(b.spp), None,
                                                   C.byref(b.rep), C.byref(b.st))

    return [("host", host), ("device", device)]


BAD_PARAMS = [(dict(spp=0), INVALID), (dict(tile=4), INVALID), (dict(rank=2, world=2), INVALID), (dict(mode=2), INVALID),
              (dict(width=0), INVALID), (dict(height=70000), INVALID), (dict(max_depth=0), UNSUPPORTED),
              (dict(max_depth=4), UNSUPPORTED), (dict(world=2), UNSUPPORTED), (dict(rng_mode=pyrt.RNG_LEGACY), UNSUPPORTED),
              (dict(use_photons=1, k=4, photons_requested=100), UNSUPPORTED), (dict(wavefront=True), UNSUPPORTED)]
# (open, close)
BAD_EXPOSURES = [(-0.1, 1.0), (0.0, 1.5), (0.6, 0.5), (NAN, 1.0), (0.0, NAN), (0.0, INF), (-INF, 1.0), (1.0000001, 1.0000001)]
# (aperture, focus_distance, a word of the message)
BAD_LENSES = [(-0.1, 1.0, b"aperture"), (NAN, 1.0, b"aperture"), (INF, 1.0, b"aperture"), (0.1, 0.0, b"focus_distance"),
              (0.1, -2.0, b"focus_distance"), (0.1, NAN, b"focus_distance"), (0.1, INF, b"focus_distance")]


def bad_records(cam):
    """(record, a word of the message) for every rejection rt_render_shutter makes from the record alone."""
    out = []
    for j in range(4):
        r = pyrt.make_shutter(cam, 0.0, 1.0, 0.1, 2.0)
        r.reserved[j] = 1
        out.append((r, b"reserved"))
    for k in range(12):
        for v in (NAN, INF, -INF):
            c = np.array(cam, np.float32)
            c.reshape(-1)[k] = v
            out.append((pyrt.make_shutter(c), b"camera_close"))
    out += [(pyrt.make_shutter(cam, op, cl), b"exposure") for op, cl in BAD_EXPOSURES]
    out += [(pyrt.make_shutter(cam, 0.0, 1.0, a, f), word) for a, f, word in BAD_LENSES]
    return out


def test_views_rejections_come_before_any_device_work():
    L, b = pyrt.amd(), Buffers()
    p, (v, _keep), sh = params(), views(), shutters()
    for name, call in view_calls(L, b):
        assert call(None, p, v, sh) == INVALID and b"null" in L.rt_last_error(), name
        assert call(FAKE, None, v, sh) == INVALID and b"null" in L.rt_last_error(), name
        assert call(FAKE, p, None, sh) == INVALID and b"null" in L.rt_last_error(), name
        nocam = pyrt.Views()
        nocam.n_views = N
        assert call(FAKE, p, nocam, sh) == INVALID and b"null" in L.rt_last_error(), name
        assert call(FAKE, p, v, None) == INVALID and b"shutters is null" in L.rt_last_error(), name
        # rt_render_views' checks of v
        assert call(FAKE, p, views(n=0)[0], sh) == INVALID, name
        big = views(np.repeat(CAMS[:1], 65536, axis=0))
        assert call(FAKE, params(width=1, height=1, spp=1), big[0], sh) == INVALID and b"n_views" in L.rt_last_error(), name
        r0, _k0 = views()
        r0.reserved0 = 1
        assert call(FAKE, p, r0, sh) == INVALID and b"reserved" in L.rt_last_error(), name
        for j in range(6):
            r, _k = views()
            r.reserved[j] = 1
            assert call(FAKE, p, r, sh) == INVALID and b"reserved" in L.rt_last_error(), (name, j)
        # rt_render's and rt_render_shutter's checks of p; a sample range is fine, one beyond spp is not
        for kw, code in BAD_PARAMS + [(dict(spp_begin=3, spp_count=2), INVALID)]:
            assert call(FAKE, params(**kw), v, sh) == code, (name, kw, L.rt_last_error())
        # a view camera that is not finite, naming the view
        for j in (0, N - 1):
            cams = CAMS.copy()
            cams[j, 2, 1] = NAN
            assert call(FAKE, p, views(cams)[0], sh) == INVALID and b"view %d" % j in L.rt_last_error(), (name, j)
        # every record-only rejection of rt_render_shutter, at view 0 and at the last view only, naming the view
        for j in (0, N - 1):
            for rec, word in bad_records(CAMS[j]):
                code = call(FAKE, p, v, shutters(**{str(j): rec}))
                msg = L.rt_last_error()
                assert code == INVALID and word in msg and b"view %d: " % j in msg, (name, j, msg)
    host, device = view_calls(L, b)[0][1], view_calls(L, b)[1][1]
    assert host(FAKE, p, v, sh, out=None, acc=None) == INVALID and b"neither" in L.rt_last_error()
    assert host(FAKE, p, v, sh, bg=None) == INVALID and b"background" in L.rt_last_error()
    assert device(FAKE, p, v, sh, acc=None) == INVALID and b"d_accum" in L.rt_last_error()
    assert b.untouched()


def test_adaptive_rejections_come_before_any_device_work():
    L, b = pyrt.amd(), Buffers()
    p, a, sh = params(), pyrt.make_adaptive(0.1, 4), pyrt.make_shutter(CAM, 0.0, 1.0, 0.1, 2.0)
    for name, call in adaptive_calls(L, b):
        assert call(None, p, a, sh) == INVALID and b"null" in L.rt_last_error(), name
        assert call(FAKE, None, a, sh) == INVALID and b"null" in L.rt_last_error(), name
        assert call(FAKE, p, None, sh) == INVALID and b"null" in L.rt_last_error(), name
        assert call(FAKE, p, a, None) == INVALID and b"null" in L.rt_last_error(), name
        for rec, word in bad_records(CAM):
            assert call(FAKE, p, a, rec) == INVALID and word in L.rt_last_error(), (name, L.rt_last_error())
        for kw, code in BAD_PARAMS + [(dict(spp=7, spp_begin=3, spp_count=4), INVALID), (dict(spp_begin=1), INVALID)]:
            assert call(FAKE, params(**kw), a, sh) == code, (name, kw, L.rt_last_error())
        # rt_render_adaptive's checks of a
        for bad in (pyrt.make_adaptive(0.1, 0), pyrt.make_adaptive(0.1, 4, min_passes=1), pyrt.make_adaptive(0.1, 4, min_passes=5),
                    pyrt.make_adaptive(-0.1, 4), pyrt.make_adaptive(NAN, 4), pyrt.make_adaptive(INF, 4),
                    pyrt.make_adaptive(0.1, 4, floor=-1.0), pyrt.make_adaptive(0.1, 4, floor=NAN), pyrt.make_adaptive(0.1, 1 << 30)):
            assert call(FAKE, p, bad, sh) == INVALID, (name, L.rt_last_error())
        for j in range(6):
            bad = pyrt.make_adaptive(0.1, 4)
            bad.reserved[j] = 1
            assert call(FAKE, p, bad, sh) == INVALID and b"reserved" in L.rt_last_error(), (name, j)
        assert call(FAKE, p, a, sh, bg=None) == INVALID and b"null" in L.rt_last_error(), name
        assert call(FAKE, p, a, sh, out=None) == INVALID and b"null" in L.rt_last_error(), name
    device = adaptive_calls(L, b)[1][1]
    assert device(FAKE, p, a, sh, acc=None) == INVALID and b"null" in L.rt_last_error()
    assert b.untouched()


def test_valid_calls_answer_no_device():
    """Without a device a valid call answers RT_ERR_NO_DEVICE and never looks at the handle (with one, the GPU tests make
    these calls on real contexts).  At aperture 0 the focus distance is ignored; the ends of the exposure rule are valid."""
    if torch.cuda.is_available():
        return
    L, b = pyrt.amd(), Buffers()
    recs = [shutters(), shutters(**{"0": pyrt.make_shutter(CAMS[0], 1.0, 1.0, 0.0, NAN)}),
            shutters(**{"2": pyrt.make_shutter(CAMS[2], 0.25, 0.5, 0.0, -1.0)})]
    for p in (params(), params(spp=7, spp_begin=3, spp_count=4, mode=pyrt.MODE_RAY, max_depth=1),
              params(accel=pyrt.ACCEL_BRUTE, collect_stats=1, no_pool=True, lanes_per_pixel=4)):
        for sh in recs:
            for seeds in (None, [4, 5, 6]):
                v, _keep = views(seeds=seeds)
                for name, call in view_calls(L, b):
                    assert call(FAKE, p, v, sh) == NO_DEVICE, (name, L.rt_last_error())
    host = view_calls(L, b)[0][1]
    assert host(FAKE, params(), views()[0], shutters(), bg=None, out=None) == NO_DEVICE  # (the accumulator alone)
    for p in (params(), params(accel=pyrt.ACCEL_BRUTE, collect_stats=1, no_pool=True, lanes_per_pixel=4)):
        for a in (pyrt.make_adaptive(0.0, 1), pyrt.make_adaptive(0.1, 5, min_passes=2, floor=0.5)):
            for sh in (pyrt.make_shutter(CAM), pyrt.make_shutter(CAM, 0.0, 0.0, 0.1, 2.0), pyrt.make_shutter(CAM, 0.25, 0.5, 0.0, NAN)):
                for name, call in adaptive_calls(L, b):
                    assert call(FAKE, p, a, sh) == NO_DEVICE, (name, L.rt_last_error())
    assert b.untouched()
