"""rt_render_textured at 2 to 5 stack rows: depth_scenes A..G and their four-light variants (the sequential body), and B,
D, F with D4 and F4 under RT_NODES_Q8, bit for bit against tests/tex_ref.py under every schedule.  A textured launch parks
the vertex's kdDiffuse at max(stackLevels, 4) * 64 + the pool's words while the pool starts at stackLevels * 64: below four
rows the two offsets are formed differently, and at five the clamp no longer applies."""
import numpy as np
import pytest

import depth_scenes as ds
import lights_ref
import pyrt
import tex_ref
from test_gpu_lights import SCHEDULES, assert_frames_equal

pytestmark = pytest.mark.gpu

F32 = np.float32
Q8 = dict(bvh_builder=pyrt.BVH_HOST, node_format=pyrt.NODES_Q8)
_ref = {}


def check_textured(name, ctx_kw):
    preset = ds.PREFIX + name
    s = lights_ref.scene((preset, False), ds.W, ds.H)
    nl = len(s.arrays()["lights"])
    assert (nl > 3) == (name in ds.FOUR_LIGHTS)  # (more than three lights: the pool is refused, the sequential body runs)
    tset = tex_ref.texture_set(s, tex_ref.T_MIXED, shift=ds.NAMES.index(ds.base(name)))
    bg = np.random.default_rng(5).uniform(0, 1, (ds.H, ds.W, 3)).astype(F32)
    ctx = pyrt.Context(s, **ds.context_options(preset), **ctx_kw)
    try:
        info = ctx.bvh_info()
        print("%s: max_depth %d, %d stack rows, node format %d" % (name, info.max_depth, info.max_depth + 1, info.node_format))
        assert info.max_depth == ds.max_depth(preset)
        if ctx_kw:
            assert info.node_format == pyrt.NODES_Q8
        ctx.set_textures(*tex_ref.set_args(tset))
        for sched, kw, brute in SCHEDULES:
            key = (name, brute)
            if key not in _ref:
                _ref[key] = tex_ref.frame(s, ds.params(), tset, bg, brute, touched=False)
            ref = _ref[key]
            out, acc, st = ctx.render_textured(ds.params(**kw), bg=bg)
            what = "%s, %s" % (name, sched)
            assert_frames_equal(acc, ref["accum"], "accum " + what)
            assert_frames_equal(out, ref["out"], "out " + what)
            assert (st.rays_closest, st.rays_shadow) == (ref["closest"], ref["shadow"]), what
            assert st.samples == ds.W * ds.H * ds.SPP7_34["spp_count"], what
        # the frame is not the plain one
        _, plain, _ = ctx.render(ds.params())
        assert (np.ascontiguousarray(_ref[(name, False)]["accum"]).view(np.uint32) != plain.view(np.uint32)).any(), name
    finally:
        ctx.close()


@pytest.mark.parametrize("name", ds.NAMES + ds.FOUR_LIGHTS)
def test_textured(name):
    check_textured(name, {})


@pytest.mark.parametrize("name", ds.Q8_NAMES + ("D4", "F4"))
def test_textured_q8(name):
    check_textured(name, Q8)
