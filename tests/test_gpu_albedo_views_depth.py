"""rt_render_views_shutter_albedo at 2 to 5 stack rows: depth_scenes B, D, F and the four-light D4, F4 (the sequential
body), and B and F under RT_NODES_Q8.  A coloured or textured launch parks the vertex's kdDiffuse at
max(stackLevels, 4) * 64 + the pool's words while the pool starts at stackLevels * 64: on one-leaf and shallow trees the
parked rows sit behind kParkMinRows rows rather than behind the stack, and at five rows the clamp no longer applies.
Two views — the scene's own camera, still and pinhole, and a second camera with a lens — under both surfaces and every
schedule, bit for bit against tests/albedo_views_ref.py; slice 0 is rt_render_textured / rt_render_colors (X2), slice 1
the single-view call of the form itself (X1)."""
import numpy as np
import pytest

import albedo_views_ref as avr
import depth_scenes as ds
import lens_ref
import lights_ref
import pyrt
import tex_ref
import vcol_ref
import views_shutter_ref
from albedo_views_ref import COL, COLORS, TEX, TEXTURES
from test_gpu_lights import SCHEDULES, assert_frames_equal

pytestmark = pytest.mark.gpu

F32 = np.float32
Q8 = dict(bvh_builder=pyrt.BVH_HOST, node_format=pyrt.NODES_Q8)
SEEDS = [11, 29]
LENS = (0, 1)
_ref = {}


def setup(name, surface):
    """(scene, cameras [2][4][3], records, the resident data, its albedo function)."""
    s = lights_ref.scene((ds.PREFIX + name, False), ds.W, ds.H)
    cams = views_shutter_ref.orbit(avr.no_negative_zero(s.arrays()["camera"]), views_shutter_ref.ORBIT_DEGREES,
                                   views_shutter_ref.ORBIT_SCALES)[:2]
    recs = [avr.record("none", cams[0], LENS), avr.record("lens", cams[1], LENS)]
    if surface == TEX:
        data = tex_ref.texture_set(s, tex_ref.T_MIXED, shift=ds.NAMES.index(ds.base(name)))
        fn = avr.texture_albedo(data)
    else:
        data = vcol_ref.smooth_colors(s)
        fn = avr.color_albedo(data)
    return s, cams, recs, data, fn


def view_params(j, **kw):
    p = ds.params(**kw)
    p.seed = SEEDS[j]
    return p


def expected(name, surface, brute):
    key = (name, surface, brute)
    if key not in _ref:
        s, cams, recs, _, fn = setup(name, surface)
        _ref[key] = [avr.view_frame(s, cams[j], recs[j], view_params(j), fn, brute) for j in range(2)]
    return _ref[key]


def check(name, surface, ctx_kw):
    preset = ds.PREFIX + name
    s, cams, recs, data, _ = setup(name, surface)
    nl = len(s.arrays()["lights"])
    assert (nl > 3) == (name in ds.FOUR_LIGHTS)  # (more than three lights: the pool is refused, the sequential body runs)
    sh = [views_shutter_ref.shutter_of(r) for r in recs]
    albedo = TEXTURES if surface == TEX else COLORS
    bg = np.random.default_rng(5).uniform(0, 1, (ds.H, ds.W, 3)).astype(F32)
    ctx = pyrt.Context(s, **ds.context_options(preset), **ctx_kw)
    try:
        info = ctx.bvh_info()
        print("%s: max_depth %d, %d stack rows, node format %d" % (name, info.max_depth, info.max_depth + 1, info.node_format))
        assert info.max_depth == ds.max_depth(preset)
        if ctx_kw:
            assert info.node_format == pyrt.NODES_Q8
        if surface == TEX:
            ctx.set_textures(*tex_ref.set_args(data))
        else:
            ctx.set_vertex_colors(data)
        for sched, kw, brute in SCHEDULES:
            ref = expected(name, surface, brute)
            what = "%s, %s, %s" % (name, surface, sched)
            out, acc, st = ctx.render_views_shutter_albedo(ds.params(**kw), cams, sh, albedo=albedo, bg=bg, seeds=SEEDS)
            for j in range(2):
                assert_frames_equal(acc[j], ref[j]["accum"], "accum %d %s" % (j, what))
                assert_frames_equal(out[j], lens_ref.resolve(ref[j]["accum"], bg, ds.params().spp), "out %d %s" % (j, what))
            assert (st.rays_closest, st.rays_shadow) == (sum(r["closest"] for r in ref), sum(r["shadow"] for r in ref)), what
            assert st.samples == 2 * ds.W * ds.H * ds.SPP7_34["spp_count"], what
            # X2: slice 0 is the single-view coloured / textured frame; X1: slice 1 the one-view call
            single = ctx.render_textured if surface == TEX else ctx.render_colors
            _, one, _ = single(view_params(0, **kw), bg=bg)
            assert_frames_equal(acc[0], one, "X2 " + what)
            _, lens, _ = ctx.render_views_shutter_albedo(ds.params(**kw), cams[1:], sh[1:], albedo=albedo, seeds=SEEDS[1:])
            assert_frames_equal(acc[1], lens[0], "X1 " + what)
        # the frame is not the untextured one
        _, plain, _ = ctx.render_views_shutter(ds.params(), cams, sh, seeds=SEEDS)
        assert (np.ascontiguousarray(acc).view(np.uint32) != plain.view(np.uint32)).any(), name
    finally:
        ctx.close()


@pytest.mark.parametrize("surface", [TEX, COL])
@pytest.mark.parametrize("name", ("B", "D", "F", "D4", "F4"))
def test_albedo_views(name, surface):
    check(name, surface, {})


@pytest.mark.parametrize("surface", [TEX, COL])
@pytest.mark.parametrize("name", ("B", "F"))
def test_albedo_views_q8(name, surface):
    check(name, surface, Q8)
