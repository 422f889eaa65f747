"""rt_render_aov_views, rt_render_motion_views and rt_denoise_batch: the AOVs, motion vectors and denoised frames of many
cameras of one resident scene, one launch each.  Slice j of every output equals, bit for bit, the single-view call on a
second context after a camera-only update to cameras[j] (seeds[j]); the AOVs and the motion also equal the CPU
restatements (tests/aov_ref.py, tests/temporal_ref.py); the batched filter equals rt_denoise of every slice and no tap
crosses a frame boundary; the context's camera, padding rule and Q8 trees behave as rt_render_views documents."""
import ctypes as C

import numpy as np
import pytest
import torch

import aov_ref
import filter_cases as fc
import orc
import pyrt
import temporal_ref as tr

pytestmark = pytest.mark.gpu

AOV = pyrt.AOV_CHANNELS
MOTION = pyrt.MOTION_CHANNELS
GUIDES = ("albedo", "normal", "position", "hits")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def scene_of(a, **kw):
    d = dict(a)
    d.update(kw)
    return pyrt.ArrayScene(d["pos"], d["nrm"], d["tri"], d["tri_begin"], d["vtx_begin"], d["materials"], d["lights"], d["camera"])


def pad_rule(a):
    """bvh_build.cpp paddingRule in float32: the padding of a scene description."""
    ref = np.abs(a["pos"][a["tri"].reshape(-1)]).max()
    pr = np.float32(max(np.float32(1), ref))
    for v in list(a["camera"][0]) + list(a["lights"][:, 0:3].reshape(-1)):
        if np.isfinite(v):
            pr = max(pr, np.float32(abs(v)))
    return np.float32(np.float32(6e-5) * pr)


def look_at(eye, target, half_w, half_h):
    """Camera.h's look-at camera (up = +y) in float32: [position, lower_left, horizontal, vertical]."""
    eye, target = np.float32(eye), np.float32(target)
    w = eye - target
    w = (w / np.linalg.norm(w)).astype(np.float32)
    u = np.cross(np.float32([0, 1, 0]), w).astype(np.float32)
    u = (u / np.linalg.norm(u)).astype(np.float32)
    v = np.cross(w, u).astype(np.float32)
    ll = (eye - half_w * u - half_h * v - w).astype(np.float32)
    return np.stack([eye, ll, (2 * half_w * u).astype(np.float32), (2 * half_h * v).astype(np.float32)]).astype(np.float32)


def orbit(cam, degs, scales):
    """Look-at cameras on orbits about the point the context camera looks at (at its own distance from the origin), one
    per (angle, distance scale): scale > 1 farther from the scene than the context camera, < 1 nearer."""
    cam = np.asarray(cam, np.float32)
    eye0 = cam[0].astype(np.float64)
    centre = cam[1] + cam[2] / 2 + cam[3] / 2
    fwd = (centre - eye0) / np.linalg.norm(centre - eye0)
    target = eye0 + fwd * max(np.linalg.norm(eye0), 1.0)
    half_w, half_h = np.float32(np.linalg.norm(cam[2]) / 2), np.float32(np.linalg.norm(cam[3]) / 2)
    out = []
    for deg, f in zip(degs, scales):
        phi = np.deg2rad(deg)
        R = np.array([[np.cos(phi), 0, np.sin(phi)], [0, 1, 0], [-np.sin(phi), 0, np.cos(phi)]])
        eye = target + R @ (eye0 - target) * f
        out.append(look_at(eye, target, half_w, half_h))
    return np.stack(out).astype(np.float32)


def with_seed(p, seeds, j):
    q = pyrt.Params.from_buffer_copy(p)
    if seeds is not None:
        q.seed = int(seeds[j])
    return q


def loop_aov(ref, p, cams, seeds, channels=AOV):
    """rt_render_aov on `ref` after a camera-only update to each camera, stacked."""
    outs = []
    for j, c in enumerate(cams):
        ref.update(camera=c)
        outs.append(ref.render_aov(with_seed(p, seeds, j), raw=True, channels=channels))
    return {k: np.stack([o[k] for o in outs]) for k in channels}


def loop_motion(ref, p, cams, seeds, prev_pos, prev_cams, channels=MOTION):
    outs = []
    for j, c in enumerate(cams):
        ref.update(camera=c)
        outs.append(ref.render_motion(with_seed(p, seeds, j), prev_pos=prev_pos, prev_camera=None if prev_cams is None else prev_cams[j],
                                      channels=channels))
    return {k: np.stack([o[k] for o in outs]) for k in channels}


def assert_stacks_equal(got, exp, what=""):
    assert sorted(got) == sorted(exp), what
    for k in exp:
        assert got[k].shape == exp[k].shape and got[k].dtype == exp[k].dtype, (what, k)
        ne = (bits(got[k]) != bits(exp[k])).reshape(len(got[k]), -1).any(axis=1)
        assert not ne.any(), "%s: channel %s differs in views %s" % (what, k, np.nonzero(ne)[0].tolist())


def three_cameras(a):
    return np.concatenate([a["camera"][None], orbit(a["camera"], [35.0, -60.0], [1.6, 0.7])])


SEEDS = [11, 12, 40000]


# ---- 1. the AOVs against the CPU restatement ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["cubes", "lowres"])
@pytest.mark.parametrize("w,h", [(24, 24), (37, 29)])
def test_aov_views_equal_restatement(kind, w, h):
    """Same rule as the single-view pass (tests/test_gpu_aov.py): every channel bit for bit."""
    s = pyrt.Scene(kind, w, h)
    a = s.arrays()
    ctx = pyrt.Context(s)
    cams = three_cameras(a)
    got = ctx.render_aov_views(pyrt.make_params(w, h, 3, seed=5), cams, seeds=SEEDS)
    for j, c in enumerate(cams):
        exp = aov_ref.aov_sums(scene_of(a, camera=c), pyrt.make_params(w, h, 3, seed=SEEDS[j]), accel=orc.ACCEL_LOOP)
        assert_stacks_equal({k: got[k][j][None] for k in AOV}, {k: exp[k][None] for k in AOV}, "%s view %d" % (kind, j))
    ctx.close()


# ---- 2. the AOVs against the per-view loop -----------------------------------------------------------------------------
LOOP_CASES = [
    ("seeds", "cubes", 37, 29, 3, SEEDS, dict(spp=3)),
    ("no_seeds", "lowres", 24, 24, 3, None, dict(spp=3)),
    ("one_view", "lowres", 37, 29, 1, [40000], dict(spp=2)),
    ("65_views_9x7", "cubes", 9, 7, 65, "arange", dict(spp=2)),
    ("brute", "cubes", 24, 24, 3, SEEDS, dict(spp=2, accel=pyrt.ACCEL_BRUTE)),
    ("photon_fields_ignored", "cubes", 24, 24, 3, SEEDS, dict(spp=2, use_photons=1, k=4, photons_requested=100, wavefront=True)),
]


def case_cameras(a, n):
    if n == 1:
        return orbit(a["camera"], [20.0], [0.9])
    if n == 3:
        return three_cameras(a)
    return orbit(a["camera"], np.linspace(0, 360, n, endpoint=False), np.linspace(0.6, 1.0, n))


@pytest.mark.parametrize("name,kind,w,h,n,seeds,kw", LOOP_CASES, ids=[c[0] for c in LOOP_CASES])
def test_aov_views_equal_per_view_loop(name, kind, w, h, n, seeds, kw):
    s = pyrt.Scene(kind, w, h)
    a = s.arrays()
    ctx, ref = pyrt.Context(s), pyrt.Context(s)
    cams = case_cameras(a, n)
    if isinstance(seeds, str):
        seeds = np.arange(n, dtype=np.uint32) * 1000 + 1  # (above 2^15 from view 33)
    p = pyrt.make_params(w, h, seed=9, **kw)
    ploop = pyrt.make_params(w, h, seed=9, **{k: v for k, v in kw.items() if k in ("spp", "accel")})
    assert_stacks_equal(ctx.render_aov_views(p, cams, seeds=seeds), loop_aov(ref, ploop, cams, seeds), name)
    ctx.close(), ref.close()


def test_aov_views_sample_ranges_chain():
    """Two sub-ranges, each the loop's for the same range: their sums add up to the frame's as the single-view sums do."""
    w, h = 37, 29
    s = pyrt.Scene("lowres", w, h)
    a = s.arrays()
    ctx, ref = pyrt.Context(s), pyrt.Context(s)
    cams = three_cameras(a)
    parts = []
    for b, c in ((0, 2), (2, 3)):
        p = pyrt.make_params(w, h, 5, seed=3, spp_begin=b, spp_count=c)
        parts.append(ctx.render_aov_views(p, cams, seeds=SEEDS))
        assert_stacks_equal(parts[-1], loop_aov(ref, p, cams, SEEDS), "range %d+%d" % (b, c))
    whole = ctx.render_aov_views(pyrt.make_params(w, h, 5, seed=3), cams, seeds=SEEDS)
    assert np.array_equal(parts[0]["hits"] + parts[1]["hits"], whole["hits"])
    assert np.array_equal(parts[0]["mesh"], whole["mesh"])
    ctx.close(), ref.close()


def test_aov_views_null_channels_do_not_shift_slices():
    w, h = 37, 29
    s = pyrt.Scene("cubes", w, h)
    a = s.arrays()
    ctx, ref = pyrt.Context(s), pyrt.Context(s)
    cams = three_cameras(a)
    p = pyrt.make_params(w, h, 2, seed=4)
    full = loop_aov(ref, p, cams, SEEDS)
    for sub in (("normal", "tri"), ("depth",), ("albedo", "hits", "mesh")):
        got = ctx.render_aov_views(p, cams, seeds=SEEDS, channels=sub)
        assert_stacks_equal(got, {k: full[k] for k in sub}, str(sub))
    ctx.close(), ref.close()


def test_aov_views_device_form_on_a_stream():
    w, h = 37, 29
    s = pyrt.Scene("lowres", w, h)
    a = s.arrays()
    ctx = pyrt.Context(s)
    cams = three_cameras(a)
    p = pyrt.make_params(w, h, 3, seed=8)
    host = ctx.render_aov_views(p, cams, seeds=SEEDS)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        dev = {k: torch.full((3, h, w, 3) if k in pyrt.AOV_FLOAT3 else (3, h, w), -7,
                             dtype=torch.float32 if k in pyrt.AOV_FLOAT3 or k == "depth" else torch.int32, device="cuda") for k in AOV}
        for _ in range(2):  # (the second call waits for the first one's upload of the view records)
            ctx.render_aov_views_device(p, cams, {k: v.data_ptr() for k, v in dev.items()}, stream=stream.cuda_stream, seeds=SEEDS)
    stream.synchronize()
    assert_stacks_equal({k: dev[k].cpu().numpy().view(host[k].dtype) for k in AOV}, host, "device form")
    ctx.close()


# ---- 3. a farther view: one refit, the context keeps the padding and its camera -----------------------------------------
def test_farther_view_refits_and_keeps_the_camera():
    w, h = 24, 24
    s = pyrt.Scene("cubes", w, h)
    a = s.arrays()
    ctx, ref = pyrt.Context(s), pyrt.Context(s)
    p = pyrt.make_params(w, h, 2, seed=6)
    before = ctx.render_aov(p, raw=True)
    pad0 = ctx.bvh_info().pad
    assert pad0 == pad_rule(a)
    far = orbit(a["camera"], [10.0, 70.0, -120.0], [3.0, 9.0, 5.0])
    assert_stacks_equal(ctx.render_aov_views(p, far), loop_aov(ref, p, far, None), "far views")
    farthest = far[int(np.argmax([pad_rule(dict(a, camera=c)) for c in far]))]
    assert ctx.bvh_info().pad == pad_rule(dict(a, camera=farthest)) > pad0
    after = ctx.render_aov(p, raw=True)
    assert_stacks_equal({k: after[k][None] for k in AOV}, {k: before[k][None] for k in AOV}, "the context's camera moved")
    # the motion pass on a fresh context refits the same way
    ctx2 = pyrt.Context(s)
    assert_stacks_equal(ctx2.render_motion_views(p, far), loop_motion(ref, p, far, None, None, far), "far views, motion")
    assert ctx2.bvh_info().pad == ctx.bvh_info().pad
    ctx.close(), ref.close(), ctx2.close()


# ---- 4. Q8 contexts ---------------------------------------------------------------------------------------------------
def _raw_aov(ctx, p, cams, arrays):
    v, keep = pyrt.make_views(cams)
    a = pyrt.Aov()
    for k, x in arrays.items():
        setattr(a, k, x.ctypes.data)
    return pyrt.amd().rt_render_aov_views(ctx._h, C.byref(p), C.byref(v), C.byref(a))


def test_q8_context_walks_its_records_and_refuses_a_refit():
    w, h = 24, 24
    s = pyrt.Scene("lowres", w, h)
    a = s.arrays()
    q8, f16 = pyrt.Context(s, node_format=pyrt.NODES_Q8), pyrt.Context(s)
    assert q8.bvh_info().node_format == pyrt.NODES_Q8
    p = pyrt.make_params(w, h, 3, seed=2)
    near = orbit(a["camera"], [15.0, -40.0, 90.0], [0.7, 0.9, 0.5])
    assert_stacks_equal(q8.render_aov_views(p, near, seeds=SEEDS), f16.render_aov_views(p, near, seeds=SEEDS), "q8 aov")
    assert_stacks_equal(q8.render_motion_views(p, near, prev_cameras=near[::-1], seeds=SEEDS),
                        f16.render_motion_views(p, near, prev_cameras=near[::-1], seeds=SEEDS), "q8 motion")
    far = orbit(a["camera"], [15.0], [6.0])
    out = dict(albedo=np.full((1, h, w, 3), 5.0, np.float32), hits=np.full((1, h, w), 5, np.uint32))
    assert _raw_aov(q8, p, far, out) == 4 and (out["albedo"] == 5.0).all() and (out["hits"] == 5).all()
    mo = np.full((1, h, w, 2), 5.0, np.float32)
    v, _keep = pyrt.make_views(far)
    m, prev = pyrt.Motion(), pyrt.MotionPrevViews()
    m.motion = mo.ctypes.data
    assert pyrt.amd().rt_render_motion_views(q8._h, C.byref(p), C.byref(v), C.byref(prev), C.byref(m)) == 4 and (mo == 5.0).all()
    q8.close(), f16.close()


def test_rejections_on_a_live_context_write_nothing():
    w, h = 16, 16
    s = pyrt.Scene("cubes", w, h)
    a = s.arrays()
    ctx = pyrt.Context(s)
    cams = orbit(a["camera"], [0.0, 20.0], [1.0, 1.1])
    out = dict(normal=np.full((2, h, w, 3), 5.0, np.float32))
    p = pyrt.make_params(w, h, 2)
    bad = cams.copy()
    bad[1, 2, 0] = np.nan
    assert _raw_aov(ctx, p, bad, out) == 1 and b"view 1" in pyrt.amd().rt_last_error()
    assert _raw_aov(ctx, pyrt.make_params(w, h, 2, world=2), cams, out) == 4
    assert _raw_aov(ctx, pyrt.make_params(w, h, 2, spp_begin=1, spp_count=2), cams, out) == 1
    assert (out["normal"] == 5.0).all() and ctx.bvh_info().pad == pad_rule(a)
    ctx.close()


# ---- 5. motion --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,w,h", [("lowres", 24, 24), ("lowres", 37, 29), ("cubes", 37, 29)])
def test_motion_views_equal_restatement_and_loop(kind, w, h):
    """Moved geometry (the context's scene has slot 3 turned; last frame's positions are the preset's) and a previous
    camera of its own per view."""
    a = pyrt.Scene(kind, w, h).arrays()
    pos, nrm = tr.turned(a, 10.0)
    cur = scene_of(a, pos=pos, nrm=nrm)
    ctx, ref = pyrt.Context(cur), pyrt.Context(cur)
    cams = three_cameras(a)
    prev_cams = np.stack([tr.moved_camera(cams[0], (0.05, 0.0, 0.0)), cams[2], tr.panned_camera(cams[2], 0.2)])
    for kw in (dict(spp=3), dict(spp=5, spp_begin=2, spp_count=2), dict(spp=2, accel=pyrt.ACCEL_BRUTE)):
        p = pyrt.make_params(w, h, seed=7, **kw)
        got = ctx.render_motion_views(p, cams, prev_pos=a["pos"], prev_cameras=prev_cams, seeds=SEEDS)
        assert_stacks_equal(got, loop_motion(ref, p, cams, SEEDS, a["pos"], prev_cams), "%s %s" % (kind, kw))
        if "accel" in kw:
            continue
        for j, c in enumerate(cams):
            exp = tr.motion_ref(scene_of(a, pos=pos, nrm=nrm, camera=c), with_seed(p, SEEDS, j), prev_pos=a["pos"], prev_camera=prev_cams[j])
            assert_stacks_equal({k: got[k][j][None] for k in MOTION}, {k: exp[k][None] for k in MOTION}, "%s %s view %d" % (kind, kw, j))
        hit = got["mesh"] != tr.MISS
        assert (got["motion"][hit] != 0).any(), "the case moves nothing"
    ctx.close(), ref.close()


def test_motion_views_null_prev_is_zero_motion():
    w, h = 37, 29
    s = pyrt.Scene("lowres", w, h)
    a = s.arrays()
    ctx = pyrt.Context(s)
    cams = three_cameras(a)
    got = ctx.render_motion_views(pyrt.make_params(w, h, 2, seed=3), cams, seeds=SEEDS)
    hit = got["mesh"] != tr.MISS
    assert hit.reshape(3, -1).any(axis=1).all() and not got["motion"].any()
    assert np.array_equal(bits(got["prev_position"]), bits(got["position"]))
    part = ctx.render_motion_views(pyrt.make_params(w, h, 2, seed=3), cams, seeds=SEEDS, channels=("mesh", "motion"))
    assert sorted(part) == ["mesh", "motion"] and np.array_equal(part["mesh"], got["mesh"])
    ctx.close()


def test_motion_views_behind_a_previous_camera_and_device_form():
    """One view's previous camera stands inside the room (points behind it: motion (+inf, +inf)), the others' do not; the
    device form on a stream of its own equals the host form."""
    w, h = 37, 29
    s = pyrt.Scene("lowres", w, h)
    a = s.arrays()
    ctx, ref = pyrt.Context(s), pyrt.Context(s)
    cams = np.stack([a["camera"], tr.moved_camera(a["camera"], (0.05, 0.0, 0.0)), a["camera"]])
    prev_cams = np.stack([a["camera"], tr.moved_camera(a["camera"], (0.0, 0.0, -3.0)), tr.moved_camera(a["camera"], (0.0, 0.1, 0.0))])
    p = pyrt.make_params(w, h, 4, seed=24)
    got = ctx.render_motion_views(p, cams, prev_cameras=prev_cams, seeds=SEEDS)
    assert_stacks_equal(got, loop_motion(ref, p, cams, SEEDS, None, prev_cams), "behind")
    inf = np.isposinf(got["motion"])
    assert inf[1, ..., 0].sum() > 20 and np.array_equal(inf[..., 0], inf[..., 1]) and not inf[0].any() and not inf[2].any()
    assert np.isfinite(got["motion"][~inf]).all()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        shape = dict(motion=(3, h, w, 2), position=(3, h, w, 3), prev_position=(3, h, w, 3), mesh=(3, h, w))
        dev = {k: torch.full(shape[k], -7, dtype=torch.int32 if k == "mesh" else torch.float32, device="cuda") for k in MOTION}
        d_prev = torch.from_numpy(a["pos"]).cuda()
        ctx.render_motion_views_device(p, cams, {k: v.data_ptr() for k, v in dev.items()}, d_prev_pos=d_prev.data_ptr(),
                                       prev_cameras=prev_cams, stream=stream.cuda_stream, seeds=SEEDS)
    stream.synchronize()
    assert_stacks_equal({k: dev[k].cpu().numpy().view(got[k].dtype) for k in MOTION}, got, "device form")
    ctx.close(), ref.close()


# ---- 6. the batched denoiser -------------------------------------------------------------------------------------------
def loop_denoise(ctx, rgb, sums, **kw):
    return np.stack([ctx.denoise(rgb[j], {k: sums[k][j] for k in GUIDES}, **kw) for j in range(len(rgb))])


@pytest.mark.parametrize("kind,w,h", [("cubes", 37, 29), ("lowres", 24, 24)])
def test_denoise_batch_of_rendered_views(kind, w, h):
    s = pyrt.Scene(kind, w, h)
    a = s.arrays()
    ctx = pyrt.Context(s)
    cams = three_cameras(a)
    p = pyrt.make_params(w, h, 3, seed=5)
    rgb, _, _ = ctx.render_views(p, cams, pyrt.background(w, h), seeds=SEEDS)
    sums = ctx.render_aov_views(p, cams, seeds=SEEDS)
    for kw in (dict(), dict(iterations=2, sigma_color=1.0, sigma_normal=0.3, sigma_position=0.5)):
        got = ctx.denoise_batch(rgb, sums, **kw)
        assert np.array_equal(bits(got), bits(loop_denoise(ctx, rgb, sums, **kw))), kw
        assert not np.array_equal(bits(got), bits(rgb))
    ctx.close()


def synthetic_stack(w, h, n, same_guides):
    """n frames of filter_cases' base generator.  same_guides: every frame has frame 0's guides, every other one upside
    down so that the rows on both sides of a frame boundary belong to the same region, and a colour of its own (scaled
    and offset): a tap that strays into a neighbouring frame meets matching guides, gets a weight and changes the
    result.  Otherwise every frame is its own draw with positions far from its neighbours'."""
    rng = np.random.default_rng(1234 + w * 100 + h)
    frames = [fc.base(w, h, rng, 0.01, False)[:2] for _ in range(n)]
    rgb, sums = [], {k: [] for k in GUIDES}
    for j, (r, sm) in enumerate(frames):
        g = ({k: x[::-1] for k, x in frames[0][1].items()} if j % 2 else frames[0][1]) if same_guides else sm
        rgb.append((r * np.float32(0.3 + 0.9 * j) + np.float32(0.2 * j)).astype(np.float32))
        for k in GUIDES:
            x = g[k].copy()
            if k == "position" and not same_guides:
                x += np.float32(50.0 * j) * g["hits"].astype(np.float32)[..., None]
            sums[k].append(x)
    holes = sums["hits"][n - 1]
    holes[0, 0] = holes[h - 1, w - 1] = holes[h // 2, w // 2] = 0  # (pixels without a hit pass through)
    return np.stack(rgb), {k: np.stack(v) for k, v in sums.items()}


@pytest.mark.parametrize("same_guides", [True, False], ids=["same_guides", "own_guides"])
@pytest.mark.parametrize("w,h", [(16, 16), (17, 15)])
def test_denoise_batch_synthetic_frames_do_not_leak(w, h, same_guides):
    ctx = pyrt.Context(pyrt.Scene("cubes", w, h))
    rgb, sums = synthetic_stack(w, h, 3, same_guides)
    for kw in (dict(iterations=5, sigma_color=8.0, sigma_position=fc.SIGMA_POSITION), dict(iterations=5),
               dict(iterations=1, sigma_color=8.0, sigma_position=fc.SIGMA_POSITION)):
        exp = loop_denoise(ctx, rgb, sums, **kw)
        got = ctx.denoise_batch(rgb, sums, **kw)
        assert np.array_equal(bits(got), bits(exp)), kw
        if same_guides and "sigma_position" in kw:
            # the check can see a leak: the stack filtered as one tall image differs from the per-frame result
            tall = ctx.denoise(rgb.reshape(3 * h, w, 3), {k: sums[k].reshape((3 * h, w) + sums[k].shape[3:]) for k in GUIDES}, **kw)
            assert not np.array_equal(bits(tall.reshape(rgb.shape)), bits(exp))
        inplace = rgb.copy()
        assert ctx.denoise_batch(inplace, sums, out=inplace, **kw) is inplace and np.array_equal(bits(inplace), bits(exp))
    ctx.close()


def test_denoise_batch_device_form_in_place_on_a_stream():
    w, h, n = 17, 15, 3
    ctx = pyrt.Context(pyrt.Scene("cubes", w, h))
    rgb, sums = synthetic_stack(w, h, n, True)
    exp = loop_denoise(ctx, rgb, sums)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        d_rgb = torch.from_numpy(rgb).cuda()
        d = {k: torch.from_numpy(sums[k].view(np.int32) if k == "hits" else sums[k]).cuda() for k in GUIDES}
        d_out = torch.empty_like(d_rgb)
        ctx.denoise_batch_device(w, h, n, d_rgb.data_ptr(), {k: v.data_ptr() for k, v in d.items()}, d_out.data_ptr(), stream=stream.cuda_stream)
        ctx.denoise_batch_device(w, h, n, d_rgb.data_ptr(), {k: v.data_ptr() for k, v in d.items()}, d_rgb.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    assert np.array_equal(bits(d_out.cpu().numpy()), bits(exp)) and np.array_equal(bits(d_rgb.cpu().numpy()), bits(exp))
    ctx.close()
