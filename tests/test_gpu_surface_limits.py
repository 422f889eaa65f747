"""The sampler, the material maps and the normal maps at the limits include/rt_amd.h allows, on the probe card
(tests/probe_card.py; tests/test_probe_card_cpu.py shows from the references alone that the card reaches each limit):
the sampler on its own through rt_render_aov_textured's albedo channel, every texture of the set read as an albedo in
turn, per probe; rt_render_textured, rt_render_material and rt_render_normal_mapped bit for bit against tex_ref, mat_ref
and nmap_ref under the eight schedules of test_gpu_lights.SCHEDULES, three lights and one, path depths 1 to 3; a Q8
context and the exhaustive loop; N2 under rt_update_skin; and a texture that starts more than 2^31 bytes into the
resident array.

Frames are compared word by word as 32-bit patterns.  A NaN the reference has must be met by a NaN (x86 and gfx950 make
different default NaNs, so sign and payload are free); everything else, infinities and signed zeros included, bit for
bit.  The references' accumulators hold no NaN (the per-sample clamp turns a NaN into 1), so for them this is
test_gpu_lights.assert_frames_equal's comparison."""
import time

import numpy as np
import pytest

import mat_ref
import nmap_ref
import probe_card as pc
import pyrt
import skin_ref
import tex_ref
from test_gpu_lights import SCHEDULES

pytestmark = pytest.mark.gpu

F32 = np.float32
LIGHTS = (3, 1)
_ctx, _ref = {}, {}


@pytest.fixture(scope="module", autouse=True)
def contexts():
    yield
    for c in _ctx.values():
        c.close()
    _ctx.clear()
    _ref.clear()


def resident(ctx, mset):
    ctx.set_textures(*tex_ref.set_args(mset))
    ctx.set_material_maps(*mat_ref.map_args(mset))
    ctx.set_normal_maps(mset["mesh_normal"])
    return ctx


def context(nl, **kw):
    """One context per light count and option set, the card's whole set resident."""
    key = (nl, tuple(sorted(kw.items())))
    if key not in _ctx:
        _ctx[key] = resident(pyrt.Context(pc.scene(nl), **kw), pc.map_set())
    return _ctx[key]


def differing(got, exp):
    """[...] bool: the pixels (all but the last axis) at which got is not exp, by the rule of the module's docstring."""
    got, exp = np.ascontiguousarray(got), np.ascontiguousarray(exp)
    assert got.shape == exp.shape and got.dtype == exp.dtype, (got.shape, exp.shape, got.dtype, exp.dtype)
    nan = np.isnan(exp)
    bad = np.where(nan, ~np.isnan(got), got.view(np.uint32) != exp.view(np.uint32))
    return bad.any(axis=-1)


def assert_same(got, exp, what, meshes=None):
    """meshes [h][w][samples]: the first-hit mesh of every sample, to name the probes of the pixels that differ."""
    bad = differing(got, exp)
    if not bad.any():
        return
    first = tuple(np.argwhere(bad)[0])
    where = ""
    if meshes is not None:
        hit = {}
        for y, x in np.argwhere(bad):
            for m in set(meshes[y, x].tolist()):
                hit[m] = hit.get(m, 0) + 1
        where = "; by probe: " + ", ".join("%s: %d" % (pc.probe_name(m) if m >= 0 else "miss", n) for m, n in sorted(hit.items()))
    raise AssertionError("%s: %d of %d pixels differ, first (y, x) = %s: got %s, expected %s%s"
                         % (what, int(bad.sum()), bad.size, first, got[first], exp[first], where))


# ---- the sampler alone ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("table", pc.TABLES)
def test_the_sampler_alone_per_probe(table):
    """rt_render_aov_textured's albedo channel with every texture `table` names read as the albedo: at one sample per
    pixel the first hit's c itself, probe by probe, then the float32 sums of four samples; first hits and hit counts are
    the reference's."""
    s = pc.scene(3)
    mset = pc.albedo_set(table)
    ctx = pyrt.Context(s)
    try:
        ctx.set_textures(*tex_ref.set_args(mset))
        for p, name in ((pc.one_sample(), "one sample"), (pc.params(4, 1), "four samples")):
            exp = tex_ref.frame(s, p, mset, touched=False)
            meshes = pc.first_hit_mesh(s, p)
            for accel in (pyrt.ACCEL_BVH, pyrt.ACCEL_BRUTE):
                q = pc.one_sample(accel=accel) if p.spp_count else pc.params(4, 1, accel=accel)
                got = ctx.render_aov_textured(q, raw=True)
                what = "%s as albedo, %s, accel %d" % (table, name, accel)
                assert (got["hits"] == (meshes >= 0).sum(axis=2)).all(), what
                if p.spp_count:
                    assert np.array_equal(got["mesh"].astype(np.int64), meshes[..., 0]), what
                    failed = []
                    for m in range(pc.N_QUADS + 2):  # probe by probe, so that a failure names them all
                        at = meshes[..., 0] == m
                        n = int(differing(got["albedo"], exp["albedo"])[at].sum())
                        if n:
                            failed.append("%s: %d of %d pixels" % (pc.probe_name(m), n, int(at.sum())))
                    assert not failed, "%s: %s" % (what, "; ".join(failed))
                assert_same(got["albedo"], exp["albedo"], what, meshes)
    finally:
        ctx.close()


# ---- the three frames ----------------------------------------------------------------------------------------------------
FORMS = {
    "textured": (lambda ctx, p, bg: ctx.render_textured(p, bg=bg), tex_ref.frame),
    "material": (lambda ctx, p, bg: ctx.render_material(p, bg=bg), mat_ref.frame),
    "normal_mapped": (lambda ctx, p, bg: ctx.render_normal_mapped(p, bg=bg), nmap_ref.frame),
}


def background():
    return np.random.default_rng(4832).uniform(0, 1, (pc.H, pc.W, 3)).astype(F32)


def reference(form, s, depth, brute=False, key=None):
    """The reference frame of a form on scene s at four samples (computed once per key, shared)."""
    key = (form, key, depth, brute)
    if key[1] is None or key not in _ref:
        kw = dict(touched=False) if form == "textured" else {}
        ref = FORMS[form][1](s, pc.params(4, depth), pc.map_set(), background(), brute, **kw)
        if key[1] is None:
            return ref
        _ref[key] = ref
    return _ref[key]


def check(got, ref, what, meshes=None):
    out, acc, st = got
    assert_same(acc, ref["accum"], "accum " + what, meshes)
    assert_same(out, ref["out"], "out " + what, meshes)
    assert (st.rays_closest, st.rays_shadow) == (ref["closest"], ref["shadow"]), what


@pytest.mark.parametrize("depth", [1, 2, 3])
@pytest.mark.parametrize("nl", LIGHTS)
@pytest.mark.parametrize("form", list(FORMS))
def test_frames_bit_exact(form, nl, depth):
    """Accumulator, image, samples and both ray counts, whatever the schedule."""
    ctx, s, bg = context(nl), pc.scene(nl), background()
    meshes = pc.first_hit_mesh(s, pc.params(4, depth))
    for name, kw, brute in SCHEDULES:
        ref = reference(form, s, depth, brute, key=nl)
        what = "%s, %d lights, depth %d, %s" % (form, nl, depth, name)
        got = FORMS[form][0](ctx, pc.params(4, depth, **kw), bg)
        check(got, ref, what, meshes)
        assert got[2].samples == pc.W * pc.H * 4 and got[2].kernel_ms > 0, what


def test_the_three_frames_differ():
    """What the frames compare is not one frame three times."""
    ctx, p = context(3), pc.params(4, 3)
    _, tex, _ = ctx.render_textured(p)
    _, mat, mst = ctx.render_material(p)
    _, nrm, nst = ctx.render_normal_mapped(p)
    assert differing(tex, mat).any() and differing(mat, nrm).any()
    assert (mst.rays_closest, mst.rays_shadow) != (nst.rays_closest, nst.rays_shadow)


def test_q8_context_and_the_exhaustive_loop():
    """The normal-mapped card frame on an RT_NODES_Q8 context (leaves of two triangles) and under RT_ACCEL_BRUTE (N4)."""
    s = pc.scene(3)
    ctx = context(3, bvh_builder=pyrt.BVH_HOST, node_format=pyrt.NODES_Q8, bvh_leaf_max=2)
    assert ctx.bvh_info().node_format == pyrt.NODES_Q8
    ref = reference("normal_mapped", s, 3, False, key=3)
    for no_pool in (False, True):
        check(ctx.render_normal_mapped(pc.params(4, 3, no_pool=no_pool), bg=background()), ref, "Q8 context, no_pool %d" % no_pool)
    brute = reference("normal_mapped", s, 3, True, key=3)
    check(context(3).render_normal_mapped(pc.params(4, 3, accel=pyrt.ACCEL_BRUTE), bg=background()), brute, "exhaustive loop")


# ---- N2 under skinning ---------------------------------------------------------------------------------------------------
def test_n2_the_frames_follow_rt_update_skin():
    """A two-bone skin over the card: after rt_update_skin the normal-mapped frame is the reference's on the blended
    scene (skin_ref.apply) and a fresh context's created on it, and not the rest pose's; the material and textured frames
    follow too."""
    s, mset = pc.scene(3), pc.map_set()
    a = s.arrays()
    bone, weight, bones = pc.skin()
    pos, nrm = skin_ref.apply(a, bone, weight, bones)
    assert not np.array_equal(pos, a["pos"]) and not np.array_equal(nrm, a["nrm"])
    moved = pyrt.ArrayScene(pos, nrm, a["tri"], a["tri_begin"], a["vtx_begin"], a["materials"], a["lights"], a["camera"])
    ctx, other = pyrt.Context(s), pyrt.Context(moved)
    try:
        resident(ctx, mset), resident(other, mset)
        ctx.set_skin(bone, weight, len(bones))
        ctx.update_skin(bones)
        for depth in (3, 1):
            exp = reference("normal_mapped", moved, depth)
            for no_pool in (False, True):
                p = pc.params(4, depth, no_pool=no_pool)
                got = ctx.render_normal_mapped(p, bg=background())
                check(got, exp, "after rt_update_skin, depth %d, no_pool %d" % (depth, no_pool))
                fresh = other.render_normal_mapped(p, bg=background())
                assert_same(got[1], fresh[1], "against a fresh context")
                assert (got[2].rays_closest, got[2].rays_shadow) == (fresh[2].rays_closest, fresh[2].rays_shadow)
        rest = reference("normal_mapped", s, 1, False, key=3)
        assert differing(exp["accum"], rest["accum"]).mean() > 0.25
        for form in ("material", "textured"):
            check(FORMS[form][0](ctx, pc.params(4, 3), background()), reference(form, moved, 3), form + " after rt_update_skin")
    finally:
        ctx.close(), other.close()


# ---- a texture beyond 2^31 bytes -------------------------------------------------------------------------------------------
def test_a_texture_that_starts_beyond_two_gib():
    """The set's first texture is 16384 x 11000 (zeros: 2.16e9 bytes), so the second — S6's 8 x 8 map on quad 0 — starts
    more than 2^31 bytes into the resident array; quad 1 reads the big texture's last rows.  The sampler alone, at one
    sample per pixel.  The wall time of the upload and the two frames is printed."""
    s, base = pc.scene(3), pc.map_set()
    big = np.zeros((11000, 16384, 3), F32)
    big[-2:] = tex_ref.random_texels(16384, 2, 77)  # (rows 10998 and 10999: the texels just below the 2^31-byte mark and on)
    small = base["textures"][base["names"].index("rand8")]
    assert big.nbytes > 2 ** 31 and big.size // 3 + 64 <= 2 ** 28
    which = np.full(pc.N_QUADS + 2, pc.NONE, np.uint32)
    which[0], which[1] = 1, 0
    uv = base["uv"].copy()
    uv[4:8] = np.array(pc.rect(0.05, 0.95, 10997.5 / 11000, 1.0), F32)  # quad 1: t over the big texture's last rows
    mset = dict(textures=[(big, tex_ref.REPEAT, tex_ref.CLAMP, tex_ref.BILINEAR), small], mesh_texture=which, uv=uv)
    p = pc.one_sample()
    exp = tex_ref.frame(s, p, mset, touched=False)
    meshes = pc.first_hit_mesh(s, p)
    at0, at1 = meshes[..., 0] == 0, meshes[..., 0] == 1
    assert at0.sum() >= 40 and at1.sum() >= 40 and (exp["albedo"][at1] != 0).any()
    ctx = pyrt.Context(s)
    try:
        t0 = time.perf_counter()
        ctx.set_textures(*tex_ref.set_args(mset))
        t1 = time.perf_counter()
        got = ctx.render_aov_textured(p, raw=True)
        print("rt_set_textures of %.2f GB: %.2f s; the frame: %.3f s" % (big.nbytes / 1e9, t1 - t0, time.perf_counter() - t1))
        for m, at in ((0, at0), (1, at1)):
            n = int(differing(got["albedo"], exp["albedo"])[at].sum())
            assert n == 0, "%s: %d of %d pixels differ" % (pc.probe_name(m), n, int(at.sum()))
        assert_same(got["albedo"], exp["albedo"], "the whole frame", meshes)
    finally:
        ctx.close()
