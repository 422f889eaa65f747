"""The C ABI of rt_render_ao without a GPU: the entry points exist, rt_ao_params and rt_ao have the header's layout,
every rejection that can be told from the arguments alone comes before any device work and writes nothing, and a valid
call answers RT_ERR_NO_DEVICE (a context exists only where a device does, so the handle is never looked at here)."""
import ctypes as C
import os
import subprocess

import numpy as np
import torch

import pyrt

ROOT = pyrt.ROOT
NAMES = ("rt_render_ao", "rt_render_ao_device")
INVALID, NO_DEVICE, UNSUPPORTED = 1, 2, 4
W, H = 12, 8
FAKE = C.c_void_p(1)


def test_entry_points_and_constants_exist():
    L = pyrt.amd()
    for name in NAMES:
        assert hasattr(L, name) and name in pyrt.AMD_SYMBOLS
    text = " ".join(open(os.path.join(ROOT, "include", "rt_amd.h")).read().split())
    assert "#define RT_AO_MAX_RAYS %d" % pyrt.AO_MAX_RAYS in text and pyrt.AO_MAX_RAYS == 256
    assert "RT_UNIT_HEMISPHERE = %d" % pyrt.UNIT_HEMISPHERE in text and pyrt.UNIT_HEMISPHERE == 13
    assert pyrt._UNIT_IO[pyrt.UNIT_HEMISPHERE] == (np.uint32, 4, np.uint32, 4)
    mode = " ".join(open(os.path.join(ROOT, "include", "rt_pixelmode.h")).read().split())
    assert "#define RT_STREAM_AO 2u" in mode


def test_structs_match_header(tmp_path):
    src = tmp_path / "layout.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rt_amd.h"', "int main(void) {"]
    structs = (("rt_ao_params", pyrt.AoParams, 32), ("rt_ao", pyrt.Ao, 40))
    for cname, cls, _ in structs:
        lines.append('  printf("%s.size %%zu\\n", sizeof(%s));' % (cname, cname))
        for n, _t in cls._fields_:
            lines.append('  printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, n, cname, n))
    lines += ["  return 0;", "}"]
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for cname, cls, size in structs:
        assert int(got[cname + ".size"]) == C.sizeof(cls) == size
        for n, _t in cls._fields_:
            assert int(got["%s.%s" % (cname, n)]) == getattr(cls, n).offset, (cname, n)


class Buffers:
    """Host buffers of the call for W x H, every one filled with 3."""

    def __init__(self):
        self.arr = dict(unoccluded=np.full((H, W), 3, np.uint32), hits=np.full((H, W), 3, np.uint32), bent=np.full((H, W, 3), 3.0, np.float32))
        self.o = pyrt.Ao()
        for k, v in self.arr.items():
            setattr(self.o, k, v.ctypes.data)

    def untouched(self):
        return all((x == 3).all() for x in self.arr.values())


def calls(L, b):
    ref = lambda x: None if x is None else C.byref(x)
    return [("host", lambda c, p, a, o=b.o: L.rt_render_ao(c, ref(p), ref(a), ref(o))),
            ("device", lambda c, p, a, o=b.o: L.rt_render_ao_device(c, ref(p), ref(a), ref(o), None))]


def params(**kw):
    base = dict(width=W, height=H, spp=4)
    base.update(kw)
    w, h, spp = base.pop("width"), base.pop("height"), base.pop("spp")
    return pyrt.make_params(w, h, spp, **base)


def ao_params(n_rays=4, bias=0., max_distance=0.):
    return pyrt.Context._ao_params(n_rays, bias, max_distance)


BAD_PARAMS = [(dict(width=0), INVALID), (dict(height=0), INVALID), (dict(width=65536), INVALID), (dict(spp=0), INVALID),
              (dict(spp_begin=3, spp_count=2), INVALID), (dict(tile=4), INVALID), (dict(rank=2, world=2), INVALID),
              (dict(world=2), UNSUPPORTED), (dict(rng_mode=pyrt.RNG_LEGACY), UNSUPPORTED)]


def test_rejections_come_before_any_device_work():
    L, b = pyrt.amd(), Buffers()
    p, a = params(), ao_params()
    for name, call in calls(L, b):
        assert call(None, p, a) == INVALID and b"null" in L.rt_last_error(), name
        assert call(FAKE, None, a) == INVALID, name
        assert call(FAKE, p, None) == INVALID, name
        assert call(FAKE, p, a, None) == INVALID, name
        b.o.reserved[3] = 1
        assert call(FAKE, p, a) == INVALID and b"reserved" in L.rt_last_error(), name
        b.o.reserved[3] = 0
        bad = ao_params()
        bad.reserved[4] = 1
        assert call(FAKE, p, bad) == INVALID and b"reserved" in L.rt_last_error(), name
        for n in (0, 257, 1 << 31):
            assert call(FAKE, p, ao_params(n_rays=n)) == INVALID and b"n_rays" in L.rt_last_error(), (name, n)
        # spp * n_rays must fit 32 bits: 2^24 * 256 = 2^32 does not, one sample fewer does (and is then answered
        # as every valid call is)
        assert call(FAKE, params(spp=1 << 24), ao_params(n_rays=256)) == INVALID and b"32 bits" in L.rt_last_error(), name
        for x in (-1.0, np.nan, np.inf, -np.inf):
            assert call(FAKE, p, ao_params(bias=x)) == INVALID and b"bias" in L.rt_last_error(), (name, x)
            assert call(FAKE, p, ao_params(max_distance=x)) == INVALID and b"max_distance" in L.rt_last_error(), (name, x)
        for kw, code in BAD_PARAMS:
            assert call(FAKE, params(**kw), a) == code, (name, kw)
    assert b.untouched()


def test_valid_calls_answer_no_device_or_run():
    """Without a device a valid call answers RT_ERR_NO_DEVICE and never looks at the handle; with one, the same arguments
    on a real context succeed (the host form: the buffers are host memory)."""
    L, b = pyrt.amd(), Buffers()
    have = torch.cuda.is_available()
    ctx = pyrt.Context(pyrt.Scene("cubes", W, H)) if have else None
    handle, want = (ctx._h, pyrt.RT_OK) if have else (FAKE, NO_DEVICE)
    forms = slice(0, 1) if have else slice(0, 2)
    # (mode, max_depth, the photon fields and the wavefront bit do not matter to the pass: still valid)
    for p in (params(), params(use_photons=1, k=300, photons_requested=0, wavefront=True, max_depth=9, mode=7),
              params(spp=(1 << 24) - 1, spp_begin=5, spp_count=1)):
        for a in (ao_params(), ao_params(n_rays=256, bias=1e-3, max_distance=2.5), ao_params(n_rays=1, max_distance=1e30)):
            if p.spp > 4 and a.n_rays != 256:
                continue
            for name, call in calls(L, b)[forms]:
                assert call(handle, p, a) == want, (name, L.rt_last_error())
    if have:
        ctx.close()
    else:
        assert b.untouched()


def test_command_line_refuses_bad_ao_flags_before_rendering(tmp_path):
    """-ao above RT_AO_MAX_RAYS or negative and a negative or non-finite -aodist are refused up front: no frame is
    rendered (so none is lost to a late RT_ERR_INVALID) and no device is needed."""
    app = os.path.join(ROOT, "ray-tracing-engine_amd", "bin", "RayTracer")
    for flags, word in ((["-ao", "257"], "-ao"), (["-ao", "-1"], "-ao"), (["-ao", "4", "-aodist", "-0.5"], "-aodist"),
                        (["-ao", "4", "-aodist", "inf"], "-aodist"), (["-ao", "4", "-aodist", "nan"], "-aodist")):
        r = subprocess.run([app, "-width", "16", "-height", "8", "-N", "1", "-o", "f.ppm"] + flags, cwd=tmp_path, capture_output=True,
                           text=True, timeout=60)
        assert r.returncode != 0 and "error: " + word in r.stderr, (flags, r.stderr)
        assert not (tmp_path / "f.ppm").exists() and not (tmp_path / "f_ao.ppm").exists()
