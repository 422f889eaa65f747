"""Every frame form at every stack-row count: 2, 3, 4 and 5 rows on depth_scenes' sub-scenes of cubes (A .. G, and their
four-light versions for the sequential body), 17 rows on hires and 25 on stress.  The frame kernels carve their per-wave
LDS from BVH max_depth + 1 rows and every launcher clamps that number in its own way ("Stack rows"); a
misplaced region does not fault, it shows in the bits, so every comparison is bit for bit — accumulator, resolved image
where the form has one, samples and both ray counts — against the reference the form's own test module uses.  Every test
asserts the context's max_depth first and prints it; tests/test_depth_scenes_cpu.py shows on the CPU that the scenes have
occluded shadow rays and bounce rays that hit.

Shallow frames: 13x9, samples 3..6 of 7, path mode at max_depth 3 (rt_render and rt_render_lights in ray mode too), under
all eight of test_gpu_lights.SCHEDULES.  Deep frames: hires 13x9 and stress 8x6 with one sample, under default, no pool,
counted, and counted without pool.

What was chosen so that a test's reference stays within seconds (an oracle frame of stress costs 0.65 s whatever its
size, because it builds the oracle's tree):
  rt_render_pick on stress     4 lights (more than the pool's three) and one slot: at most 4 frames
  lens, shutter on stress      the 8x6 frame is rendered whole under every schedule and every schedule's frame must be the
                               default's bit for bit; the oracle's row (lens_ref / shutter_ref over rays_ref.row, without
                               the ray counts, which cost a second frame each) is compared at STRESS_PIXELS, five pixels
  rt_render_rays on stress     5 rays, rows without the counts; the shuffled stream_index on hires and the shallow scenes
  views+shutter, adaptive      on hires, not on stress (an 8x6 frame is one granule: nothing can retire beside a kept one)
  rt_render_adaptive_shutter   its chain is the library's own rt_render_shutter_device frames (as in
                               test_gpu_adaptive_shutter.py), which test_shutter compares with the oracle on the same scenes
  the row-built references     (lens, shutter, views+shutter, rays) are the oracle's tree throughout; the exhaustive
                               schedules are compared with them too (the oracle's two loops agree: test_oracle_bvh.py)
  RT_NODES_Q8                  holds leaves of at most two triangles, so the Q8 contexts are B, D and F (rows 2, 3, 4), not
                               C and G

Not in scope: k_aov, k_ao and k_motion have static LDS of (kMaxDepth + 1) * 64 words whatever the tree, and the photon
frames size their rows from the kd tree."""
import numpy as np
import pytest

import adaptive_ref
import depth_scenes as ds
import lens_ref
import lights_ref
import orc
import pick_ref
import pyrt
import rays_ref
import shutter_ref
import vcol_ref
import views_shutter_ref
from adaptive_cases import check_result
from test_gpu_lights import SCHEDULES, assert_frames_equal, bits

pytestmark = pytest.mark.gpu

F32 = np.float32
PATH, RAY = pyrt.MODE_PATH, pyrt.MODE_RAY
SPP1, SPP7_34 = lens_ref.SPP1, lens_ref.SPP7_34
DEEP_SCHEDULES = [SCHEDULES[i] for i in (0, 1, 4, 5)]
assert [s[0] for s in DEEP_SCHEDULES] == ["default", "no pool", "counted", "counted, no pool"]
STRESS_PIXELS = (0, 13, 26, 39, 47)
_ctx, _ref = {}, {}


def target(preset):
    """(preset, w, h, sample range, schedules)"""
    if ds.is_depth(preset):
        return preset, ds.W, ds.H, SPP7_34, SCHEDULES
    return (preset, 13, 9, SPP1, DEEP_SCHEDULES) if preset == "hires" else (preset, 8, 6, SPP1, DEEP_SCHEDULES)


def ident(t):
    return "%s-depth%d" % (t[0].replace(ds.PREFIX, ""), ds.max_depth(t[0]))


THREE = [target(ds.PREFIX + n) for n in ds.NAMES]
FOUR = [target(ds.PREFIX + n) for n in ds.FOUR_LIGHTS]
HIRES, STRESS = target("hires"), target("stress")
ALL = THREE + [HIRES, STRESS]
Q8_THREE = [target(ds.PREFIX + n) for n in ds.Q8_NAMES]
Q8_FOUR = [target(ds.PREFIX + n) for n in ("D4", "F4")]
Q8 = dict(bvh_builder=pyrt.BVH_HOST, node_format=pyrt.NODES_Q8)


@pytest.fixture(scope="module", autouse=True)
def contexts():
    yield
    for c in _ctx.values():
        c.close()
    _ctx.clear()


def context(t, scene, variant="", colors=None, **kw):
    """One context per scene, variant (whose lights or aspect differ, or whose tree a call may refit) and option set,
    created with the scene's bvh_leaf_max; its max_depth is asserted and shown."""
    key = (t[0], variant, tuple(sorted(kw.items())))
    if key not in _ctx:
        _ctx[key] = pyrt.Context(scene, **ds.context_options(t[0]), **kw)
        if colors is not None:
            _ctx[key].set_vertex_colors(colors)
    info = _ctx[key].bvh_info()
    print("%s%s: max_depth %d, %d stack rows (%d nodes, leaf_max %d, builder %d, node format %d)" % (
        t[0], " " + variant if variant else "", info.max_depth, info.max_depth + 1, info.n_nodes, info.leaf_max, info.builder, info.node_format))
    assert info.max_depth == ds.max_depth(t[0]), (t[0], info.max_depth)
    if "node_format" in kw:
        assert info.node_format == kw["node_format"]
    return _ctx[key]


def plain_scene(t):
    return lens_ref.scene(t[0], False, t[1], t[2])


def params(t, mode=PATH, seed=ds.SEED, **kw):
    args = dict(mode=mode, max_depth=ds.MAX_DEPTH if mode == PATH else 1, seed=seed)
    args.update(t[3])
    args.update(kw)
    return pyrt.make_params(t[1], t[2], args.pop("spp"), **args)


def samples_of(t, views=1):
    return views * t[1] * t[2] * t[3].get("spp_count", t[3]["spp"])


def background(t):
    return np.random.default_rng(t[1] * 100 + t[2] + 3).uniform(0, 1, (t[2], t[1], 3)).astype(F32)


def oracle_frame(t, scene, tag, p, brute=False):
    """The oracle's frame (computed once per tag, shared, never written to): dict(accum, out, closest, shadow)."""
    key = ("frame", t[0], tag, brute)
    if key not in _ref:
        out, acc, st = orc.render(scene, p, math_mode=orc.MATH_DET, bg=background(t), accel=orc.ACCEL_LOOP if brute else orc.ACCEL_OBVH)
        out.setflags(write=False), acc.setflags(write=False)
        _ref[key] = dict(accum=acc, out=out, closest=st.rays_closest, shadow=st.rays_shadow)
    return _ref[key]


def check(got, ref, samples, what):
    out, acc, st = got
    assert_frames_equal(acc, ref["accum"], "accum " + what)
    if ref.get("out") is not None:
        assert_frames_equal(out, ref["out"], "out " + what)
    assert (st.rays_closest, st.rays_shadow) == (ref["closest"], ref["shadow"]), what
    assert st.samples == samples and st.kernel_ms > 0, what


# ---- rt_render ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", ALL + FOUR, ids=ident)
def test_render(t):
    """rt_render under every schedule and with the wavefront bit; on the four-light scenes the pool is refused and the
    sequential body runs."""
    s = plain_scene(t)
    ctx, bg = context(t, s), background(t)
    for mode in (PATH, RAY) if ds.is_depth(t[0]) else (PATH,):
        for name, kw, brute in t[4] + [("wavefront", dict(wavefront=True), False)]:
            ref = oracle_frame(t, s, ("render", mode), params(t, mode), brute)
            check(ctx.render(params(t, mode, **kw), bg), ref, samples_of(t), "%s, mode %d, %s" % (ident(t), mode, name))


@pytest.mark.parametrize("t", Q8_THREE + Q8_FOUR, ids=ident)
def test_render_q8(t):
    s = plain_scene(t)
    ctx, bg = context(t, s, **Q8), background(t)
    for name, kw, brute in t[4]:
        ref = oracle_frame(t, s, ("render", PATH), params(t), brute)
        check(ctx.render(params(t, **kw), bg), ref, samples_of(t), "%s, Q8, %s" % (ident(t), name))


# ---- rt_render_views ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", ALL, ids=ident)
def test_views(t):
    """Three cameras on an orbit, a seed per view: every slice is the oracle's frame of that camera."""
    s = plain_scene(t)
    ctx, bg = context(t, s, "views"), background(t)
    cams = views_shutter_ref.orbit(s.arrays()["camera"], views_shutter_ref.ORBIT_DEGREES, views_shutter_ref.ORBIT_SCALES)
    seeds = list(views_shutter_ref.VIEW_SEEDS)
    frames = [oracle_frame(t, shutter_ref.with_camera(s, cams[j]), ("view", j), params(t, seed=seeds[j])) for j in range(len(cams))]
    ref = dict(accum=np.stack([f["accum"] for f in frames]), out=np.stack([f["out"] for f in frames]),
               closest=sum(f["closest"] for f in frames), shadow=sum(f["shadow"] for f in frames))
    assert (bits(ref["accum"][0]) != bits(ref["accum"][1])).any() and (bits(ref["accum"][1]) != bits(ref["accum"][2])).any()
    for name, kw, brute in t[4]:
        if not brute:
            check(ctx.render_views(params(t, **kw), cams, bg, seeds=seeds), ref, samples_of(t, 3), "%s, %s" % (ident(t), name))


# ---- rt_render_lens, rt_render_shutter -----------------------------------------------------------------------------------
def lens_case(t):
    return (t[0], False, t[1], t[2], t[3], PATH, ds.MAX_DEPTH, False, 1, 0)


def shutter_case(t):
    return lens_case(t)[:8] + ("turn", 0, (0, 1))


def sampled_rows(t, o, F, p):
    """The oracle's rows of a one-sample frame at STRESS_PIXELS: [n][4]."""
    rows = []
    for pix in STRESS_PIXELS:
        y, x = divmod(pix, t[1])
        rows.append(rays_ref.row(plain_scene(t), o[y, x, 0], F[y, x, 0], pix, lens_ref._one_sample(p, 0), orc.ACCEL_OBVH, counts=False)[0])
    return np.stack(rows)


def check_rows_form(t, render, reference, rays, what):
    """A form whose reference is built row by row: whole on the shallow scenes and hires; on stress the rows of
    STRESS_PIXELS, and every schedule's frame the default's."""
    bg = background(t)
    if t[0] != "stress":
        ref = reference()
        for name, kw, _ in t[4]:
            check(render(kw, bg), ref, samples_of(t), "%s %s, %s" % (what, ident(t), name))
        return
    assert t[3] == SPP1
    first = None
    for name, kw, _ in t[4]:
        out, acc, st = render(kw, bg)
        if first is None:
            first = (out, acc, st)
            o, F = rays()
            got = acc.reshape(-1, 4)[list(STRESS_PIXELS)]
            exp = sampled_rows(t, o, F, lens_ref.case_params(lens_case(t)))
            assert_frames_equal(got, exp, "%s %s: the rows of pixels %s" % (what, ident(t), STRESS_PIXELS))
            assert_frames_equal(out, lens_ref.resolve(acc, bg, 1), "out " + what)
        assert_frames_equal(acc, first[1], "accum %s, %s against default" % (what, name))
        assert_frames_equal(out, first[0], "out %s, %s against default" % (what, name))
        assert (st.rays_closest, st.rays_shadow, st.samples) == (first[2].rays_closest, first[2].rays_shadow, samples_of(t))
        assert st.rays_closest >= samples_of(t) and st.rays_shadow > 0


@pytest.mark.parametrize("t", ALL, ids=ident)
def test_lens(t):
    c = lens_case(t)
    a, f = lens_ref.case_lens(c)
    assert a > 0
    s = lens_ref.case_scene(c)
    ctx = context(t, s)
    check_rows_form(t, lambda kw, bg: ctx.render_lens(lens_ref.case_params(c, **kw), pyrt.make_lens(a, f), bg=bg),
                    lambda: dict(lens_ref.expected(s, lens_ref.case_params(c), a, f, bg=background(t))),
                    lambda: lens_ref.lens_rays(s.arrays()["camera"], lens_ref.case_params(c), a, f), "lens")


@pytest.mark.parametrize("t", ALL, ids=ident)
def test_shutter(t):
    """A translated and turned camera_close with an aperture."""
    c = shutter_case(t)
    k = shutter_ref.case_shutter_args(c)
    assert k["aperture"] > 0
    s, B = shutter_ref.case_scene(c), shutter_ref.case_cameras(c)[1]
    ctx = context(t, s)
    sh = pyrt.make_shutter(B, **k)
    p = shutter_ref.case_params(c)
    check_rows_form(t, lambda kw, bg: ctx.render_shutter(shutter_ref.case_params(c, **kw), sh, bg=bg),
                    lambda: shutter_ref.expected(s, B, p, k["open"], k["close"], k["aperture"], k["focus_distance"], bg=background(t)),
                    lambda: shutter_ref.shutter_rays(s.arrays()["camera"], B, p, k["open"], k["close"], k["aperture"], k["focus_distance"]),
                    "shutter")


@pytest.mark.parametrize("t", THREE + [HIRES], ids=ident)
def test_views_shutter(t):
    c = lens_case(t)[:8] + (("none", "move_lens", "turn"), (0, 0), shutter_ref.SMALL, views_shutter_ref.VIEW_SEEDS)
    s = views_shutter_ref.case_scene(c)
    ctx, bg = context(t, s, "views"), views_shutter_ref.case_background(c)
    ref = views_shutter_ref.case_reference(c)
    for name, kw, _ in t[4]:
        got = ctx.render_views_shutter(views_shutter_ref.case_params(c, **kw), views_shutter_ref.case_cameras(c),
                                       views_shutter_ref.case_shutters(c), bg, seeds=views_shutter_ref.case_seeds(c))
        check(got, ref, samples_of(t, 3), "views+shutter %s, %s" % (ident(t), name))


# ---- rt_render_lights ----------------------------------------------------------------------------------------------------
MASKS = {3: [(0b111, 0b001, 0b000, 0b110), (0b101,)], 4: [(0b0001, 0b0110, 0b1111, 0b1000), (0b1010,)]}


def check_lights(t, key, ctx):
    modes = (PATH, RAY) if ds.is_depth(t[0]) else (PATH,)
    n = lights_ref.n_lights(lights_ref.scene(key, t[1], t[2]))
    for mode in modes:
        for masks in MASKS[n][:2 if mode == PATH else 1]:
            c = (key, t[1], t[2], t[3], mode, ds.MAX_DEPTH if mode == PATH else 1, masks)
            bg = lights_ref.case_background(c)
            for name, kw, brute in t[4]:
                ref = lights_ref.case_reference(c, brute)
                got = ctx.render_lights(lights_ref.case_params(c, **kw), masks, bg=bg)
                check(got, ref, samples_of(t), "lights %s, %d lights, mode %d, %d groups, %s" % (ident(t), n, mode, len(masks), name))


@pytest.mark.parametrize("t", ALL + FOUR, ids=ident)
def test_lights(t):
    """Four groups and one group; three lights: pooled, the hand-over in the pool's words (and, under no pool, in 13 stack
    rows); four lights: sequential."""
    key = (t[0], False)
    check_lights(t, key, context(t, lights_ref.scene(key, t[1], t[2])))


@pytest.mark.parametrize("preset", ["hires", "stress"])
def test_lights_sequential_deep(preset):
    """The deep presets under the four lights of shading_sweep's scene 3: the hand-over in 13 stack rows of 17 and 25."""
    t = target(preset)
    key = ("sweep", preset, 3)
    s = lights_ref.scene(key, t[1], t[2])
    assert lights_ref.n_lights(s) == 4
    check_lights(t, key, context(t, s, "sweep3"))


@pytest.mark.parametrize("t", Q8_THREE + Q8_FOUR, ids=ident)
def test_lights_q8(t):
    key = (t[0], False)
    check_lights(t, key, context(t, lights_ref.scene(key, t[1], t[2]), **Q8))


# ---- rt_render_pick ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", ALL, ids=ident)
def test_pick(t):
    """Five lights with two and three slots (stress: four lights, one slot)."""
    for n, m in ((4, 1),) if t[0] == "stress" else ((5, 2), (5, 3)):
        c = ((t[0], False, n), t[1], t[2], t[3], PATH, ds.MAX_DEPTH, m, None)
        s = pick_ref.case_scene(c)
        assert len(pick_ref.scene_lights(s)) == n
        ctx, bg = context(t, s, "%d lights" % n), pick_ref.case_background(c)
        for name, kw, brute in t[4]:
            ref = pick_ref.case_reference(c, brute)
            got = ctx.render_pick(pick_ref.case_params(c, **kw), pick_ref.case_pick(c), bg=bg)
            check(got, ref, samples_of(t), "pick %s, n %d, m %d, %s" % (ident(t), n, m, name))


# ---- rt_render_colors ----------------------------------------------------------------------------------------------------
def check_colors(t, ctx_kw):
    s = lights_ref.scene((t[0], False), t[1], t[2])
    colors = vcol_ref.smooth_colors(s)
    ctx, bg = context(t, s, "smooth", colors=colors, **ctx_kw), background(t)
    c = ((t[0], False), t[1], t[2], t[3], PATH, ds.MAX_DEPTH, vcol_ref.SMOOTH)
    for name, kw, brute in t[4]:
        key = ("colors", t[0], brute)
        if key not in _ref:
            _ref[key] = vcol_ref.frame(s, vcol_ref.case_params(c), colors, bg, brute, touched=False)
        check(ctx.render_colors(vcol_ref.case_params(c, **kw), bg=bg), _ref[key], samples_of(t), "colours %s, %s" % (ident(t), name))
    return s, c, bg


@pytest.mark.parametrize("t", ALL + FOUR, ids=ident)
def test_colors(t):
    """The smooth colouring against vcol_ref.frame; on the shallow scenes C1 too: the materials' albedo on every vertex
    gives rt_render's own frame."""
    s, c, bg = check_colors(t, {})
    if ds.is_depth(t[0]):
        ctx = context(t, s, "albedo", colors=vcol_ref.albedo_colors(s))
        for name, kw, _ in t[4]:
            p = vcol_ref.case_params(c, **kw)
            eout, eacc, est = ctx.render(p, bg)
            check(ctx.render_colors(p, bg=bg), dict(accum=eacc, out=eout, closest=est.rays_closest, shadow=est.rays_shadow),
                  samples_of(t), "C1 %s, %s" % (ident(t), name))


@pytest.mark.parametrize("t", Q8_THREE + Q8_FOUR, ids=ident)
def test_colors_q8(t):
    check_colors(t, Q8)


# ---- rt_render_rays ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", ALL, ids=ident)
def test_rays(t):
    """Pooled and unpooled, on the primary rays of an 8x6 frame (scaled) and rays from their hit points, keyed by their
    own index and by a shuffled stream_index."""
    n = 5 if t[0] == "stress" else 70
    c = (t[0], False, n, t[3], PATH, ds.MAX_DEPTH, False)
    s = rays_ref.scene(t[0], False)
    ctx = context(t, s, "rays")
    rays, ll = rays_ref.batch(t[0], False, n)
    bg = rays_ref.case_background(n)
    p = rays_ref.case_params(c)
    ref = rays_ref.rows(s, rays, ll, p, bg=bg, counts=t[0] != "stress")
    perm = np.random.default_rng(4).permutation(n).astype(np.uint32)
    shuffled = None if t[0] == "stress" else rays_ref.rows(s, rays, ll, p, stream_index=perm)
    for name, kw, _ in t[4]:
        what = "rays %s, %s" % (ident(t), name)
        out, acc, st = ctx.render_rays(rays_ref.case_params(c, **kw), rays, bg=bg)
        assert_frames_equal(acc, ref["accum"], "accum " + what)
        assert_frames_equal(out, ref["out"], "out " + what)
        assert st.samples == n * t[3].get("spp_count", t[3]["spp"]) and st.rays_closest >= st.samples
        if shuffled is not None:
            assert (st.rays_closest, st.rays_shadow) == (ref["closest"], ref["shadow"]), what
            _, acc, st = ctx.render_rays(rays_ref.case_params(c, **kw), rays, stream_index=perm)
            assert_frames_equal(acc, shuffled["accum"], "shuffled stream_index, " + what)
            assert (st.rays_closest, st.rays_shadow) == (shuffled["closest"], shuffled["shadow"]), what
    if shuffled is not None:  # (another key is another stream)
        assert (bits(shuffled["accum"]) != bits(ref["accum"])).any()


# ---- rt_render_adaptive, rt_render_adaptive_shutter ----------------------------------------------------------------------
A_P, A_PASSES, A_SEED = 2, 5, 17


def adaptive_params(t, **kw):
    return pyrt.make_params(t[1], t[2], A_P, mode=PATH, seed=A_SEED, **kw)


@pytest.mark.parametrize("t", THREE + [HIRES], ids=ident)
def test_adaptive(t):
    """The chain from the oracle (every sample of pass k is the oracle's one-sample frame under seed + k, added in float32
    in sample order); a threshold that retires some granules and keeps others, and threshold 0."""
    from test_gpu_adaptive_shutter import P, PASSES, splitting_threshold, with_seed
    assert (P, PASSES) == (A_P, A_PASSES)  # (splitting_threshold's)
    s = plain_scene(t)
    ctx, bg = context(t, s), pyrt.background(t[1], t[2])
    p = adaptive_params(t)
    acc, chain = np.zeros((t[2], t[1], 4), F32), []
    for k in range(A_PASSES):
        for i in range(A_P):
            q = with_seed(p, k)
            q.spp_begin, q.spp_count = i, 1
            acc = (acc + orc.render(s, q, math_mode=orc.MATH_DET, accel=orc.ACCEL_OBVH)[1]).astype(F32)
        chain.append(acc.copy())
    thr, K, active = splitting_threshold(chain, bg)
    for kw in (dict(), dict(no_pool=True)):
        check_result(p, bg, chain, K, active, ctx.render_adaptive(adaptive_params(t, **kw), bg, thr, A_PASSES))
    K0, active0 = adaptive_ref.run_rule(chain, bg, A_P, 0.0, A_PASSES)
    check_result(p, bg, chain, K0, active0, ctx.render_adaptive(p, bg, 0.0, A_PASSES))


@pytest.mark.parametrize("t", THREE + [HIRES], ids=ident)
def test_adaptive_shutter(t):
    """The chain from rt_render_shutter_device (test_shutter compares that form with the oracle on these scenes)."""
    from test_gpu_adaptive_shutter import P, PASSES, gpu_chain, splitting_threshold
    assert (P, PASSES) == (A_P, A_PASSES)
    c = shutter_case(t)
    s, B = shutter_ref.case_scene(c), shutter_ref.case_cameras(c)[1]
    ctx, bg = context(t, s), pyrt.background(t[1], t[2])
    sh = pyrt.make_shutter(B, **shutter_ref.case_shutter_args(c))
    for kw in (dict(), dict(no_pool=True)):
        p = adaptive_params(t, **kw)
        chain = gpu_chain(ctx, p, sh, A_PASSES)
        thr, K, active = splitting_threshold(chain, bg)
        check_result(p, bg, chain, K, active, ctx.render_adaptive_shutter(p, sh, bg, thr, A_PASSES))


# ---- rt_trace, rt_trace_stream_device ------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", ALL, ids=ident)
def test_trace(t):
    """Closest and any-hit on every ray the frame casts (the oracle's dump), against the oracle's trace of them."""
    import torch
    s = plain_scene(t)
    ctx, a = context(t, s), s.arrays()
    p = params(t)
    d = orc.dump_rays(s, p, cap=samples_of(t) * 3 * (1 + len(a["lights"])) + 16)
    rays = np.zeros(len(d), pyrt.RAY_DTYPE)
    rays["origin"], rays["direction"] = d[:, 0:3], d[:, 4:7]
    n = len(rays)
    assert n > samples_of(t)
    want = orc.trace(s, rays, accel=orc.ACCEL_OBVH)
    want_any = orc.trace(s, rays, accel=orc.ACCEL_OBVH, kind=pyrt.TRACE_ANY)["hit"]
    assert 0 < (want["hit"] != 0).sum() and 0 < (want_any != 0).sum() < n
    for accel in (pyrt.ACCEL_BVH, pyrt.ACCEL_BRUTE) if ds.is_depth(t[0]) else (pyrt.ACCEL_BVH,):
        got = ctx.trace(rays, accel)
        diff = (got.view(np.uint8).reshape(n, -1) != want.view(np.uint8).reshape(n, -1)).any(axis=1)
        assert not diff.any(), "closest, accel %d: %d of %d rays, first %d: got %s expected %s" % (
            accel, diff.sum(), n, np.argmax(diff), got[np.argmax(diff)], want[np.argmax(diff)])
        diff = ctx.trace(rays, accel, pyrt.TRACE_ANY)["hit"] != want_any
        assert not diff.any(), "any, accel %d: %d of %d rays, first %d" % (accel, diff.sum(), n, np.argmax(diff))
    hit = want["hit"] != 0
    gid = np.where(hit, a["tri_begin"][np.where(hit, want["mesh"], 0)].astype(np.int64) + want["tri"], 0)
    exp = np.full((n, 2), 0xFFFFFFFF, np.uint32)
    exp[hit, 0], exp[hit, 1] = bits(want["d"])[hit], gid[hit]
    for anyk in (0, 1):
        O, D = np.zeros((n, 4), F32), np.zeros((n, 4), F32)
        O[:, 0:3], D[:, 0:3] = rays["origin"], rays["direction"]
        O[:, 3] = np.full(n, anyk, np.uint32).view(F32)
        dO, dD = torch.from_numpy(O).cuda(), torch.from_numpy(D).cuda()
        res = torch.full((n, 2), 7, dtype=torch.int32, device="cuda")
        ctx.trace_stream_device(dO.data_ptr(), dD.data_ptr(), n, res.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        got = res.cpu().numpy().view(np.uint32)
        diff = (got[:, 0] != want_any.astype(np.uint32)) | (got[:, 1] != 0) if anyk else (got != exp).any(axis=1)
        assert not diff.any(), "stream %s: %d of %d rays, first %d got %s" % ("any" if anyk else "closest", diff.sum(), n, np.argmax(diff), got[np.argmax(diff)])
