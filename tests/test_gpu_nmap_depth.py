"""rt_render_normal_mapped at 2 to 5 stack rows: depth_scenes B, D, F, G (the pooled body) and their four-light variants
D4, F4 and G4 (the sequential body), and B and F under RT_NODES_Q8, bit for bit against tests/nmap_ref.py under every
schedule.  A normal-mapped launch parks the vertex's material in the material frame's EIGHT rows at
max(stackLevels, kParkMinRows) * 64 + the pool's words while the pool starts at stackLevels * 64: below four rows the two
offsets are formed differently, at five the clamp no longer applies, and rows that ran into the stack or the pool would
show in the bits here — as would a bent normal that reached the pool's hemisphere sample but not its BSDF half, or the
other way round."""
import numpy as np
import pytest

import depth_scenes as ds
import lights_ref
import mat_ref
import nmap_ref
import pyrt
from test_gpu_lights import SCHEDULES, assert_frames_equal

pytestmark = pytest.mark.gpu

F32 = np.float32
Q8 = dict(bvh_builder=pyrt.BVH_HOST, node_format=pyrt.NODES_Q8)
_ref = {}


def check_normal_mapped(name, ctx_kw):
    preset = ds.PREFIX + name
    s = lights_ref.scene((preset, False), ds.W, ds.H)
    nl = len(s.arrays()["lights"])
    assert (nl > 3) == (name in ds.FOUR_LIGHTS)  # (more than three lights: the pool is refused, the sequential body runs)
    shift = ds.NAMES.index(ds.base(name))
    mset = nmap_ref.nmap_set(mat_ref.map_set(s, mat_ref.T_MIXED, shift=shift), s, shift)
    bg = np.random.default_rng(5).uniform(0, 1, (ds.H, ds.W, 3)).astype(F32)
    ctx = pyrt.Context(s, **ds.context_options(preset), **ctx_kw)
    try:
        info = ctx.bvh_info()
        print("%s: max_depth %d, %d stack rows, node format %d" % (name, info.max_depth, info.max_depth + 1, info.node_format))
        assert info.max_depth == ds.max_depth(preset)
        if ctx_kw:
            assert info.node_format == pyrt.NODES_Q8
        ctx.set_textures(*nmap_ref.set_args(mset))
        ctx.set_material_maps(*nmap_ref.map_args(mset))
        ctx.set_normal_maps(mset["mesh_normal"])
        for sched, kw, brute in SCHEDULES:
            key = (name, brute)
            if key not in _ref:
                _ref[key] = nmap_ref.frame(s, ds.params(), mset, bg, brute)
                assert np.isfinite(_ref[key]["accum"]).all() and _ref[key]["bent"] > 0
            ref = _ref[key]
            out, acc, st = ctx.render_normal_mapped(ds.params(**kw), bg=bg)
            what = "%s, %s" % (name, sched)
            assert_frames_equal(acc, ref["accum"], "accum " + what)
            assert_frames_equal(out, ref["out"], "out " + what)
            assert (st.rays_closest, st.rays_shadow) == (ref["closest"], ref["shadow"]), what
            assert st.samples == ds.W * ds.H * ds.SPP7_34["spp_count"], what
        # the frame is not the material one
        _, mat, _ = ctx.render_material(ds.params())
        assert (np.ascontiguousarray(_ref[(name, False)]["accum"]).view(np.uint32) != mat.view(np.uint32)).any(), name
    finally:
        ctx.close()


@pytest.mark.parametrize("name", ("B", "D", "F", "G", "D4", "F4", "G4"))
def test_normal_mapped(name):
    check_normal_mapped(name, {})


@pytest.mark.parametrize("name", ("B", "F"))
def test_normal_mapped_q8(name):
    check_normal_mapped(name, Q8)
