"""rt_render_views: many cameras of one resident scene in one launch.  Slice j of the accumulator and image j equal, bit
for bit, the frame of cameras[j] and seeds[j] — from the CPU oracle, from rt_render on a second context after a
camera-only update, and across sample ranges and the device form; the context's own camera, padding rule and photon map
behave as documented; rejected calls write nothing."""
import ctypes as C

import numpy as np
import pytest
import torch

import orc
import pyrt

pytestmark = pytest.mark.gpu


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


def per_view_frames(ref, p, cams, seeds, bg=None):
    """rt_render on `ref` after a camera-only update to each camera: (images, accumulators, summed ray counts)."""
    outs, accs, rays = [], [], [0, 0, 0]
    for j, c in enumerate(cams):
        ref.update(camera=c)
        q = pyrt.Params.from_buffer_copy(p)
        if seeds is not None:
            q.seed = int(seeds[j])
        out, acc, st = ref.render(q, bg)
        outs.append(out), accs.append(acc)
        rays = [rays[0] + st.rays_closest, rays[1] + st.rays_shadow, rays[2] + st.knn_queries]
    return outs, accs, rays


def assert_views_equal_per_view(ctx, ref, p, cams, seeds, bg=None):
    out, acc, st = ctx.render_views(p, cams, bg, seeds=seeds)
    routs, raccs, rays = per_view_frames(ref, p, cams, seeds, bg)
    for j in range(len(cams)):
        assert np.array_equal(bits(acc[j]), bits(raccs[j])), "view %d: accumulator differs from its rt_render frame" % j
        if bg is not None:
            assert np.array_equal(bits(out[j]), bits(routs[j])), "view %d: image differs" % j
    assert [st.rays_closest, st.rays_shadow, st.knn_queries] == rays
    assert st.samples == len(cams) * p.width * p.height * (p.spp_count or p.spp)
    return st


# ---- 1. the oracle ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["cubes", "lowres"])
@pytest.mark.parametrize("w,h", [(24, 24), (37, 29)])
def test_views_equal_oracle(kind, w, h):
    s = pyrt.Scene(kind, w, h)
    a = s.arrays()
    ctx = pyrt.Context(s)
    cams = np.concatenate([a["camera"][None], orbit(a["camera"], [35.0, -60.0], [1.6, 0.7])])
    seeds = [11, 12, 40000]
    bg = pyrt.background(w, h)
    for mode in (pyrt.MODE_PATH, pyrt.MODE_RAY):
        p = pyrt.make_params(w, h, 3, mode=mode, seed=5)
        out, acc, st = ctx.render_views(p, cams, bg, seeds=seeds)
        rays = [0, 0]
        for j, c in enumerate(cams):
            q = pyrt.make_params(w, h, 3, mode=mode, seed=seeds[j])
            ref_out, ref_acc, ref_st = orc.render(scene_of(a, camera=c), q, math_mode=orc.MATH_DET, bg=bg, accel=orc.ACCEL_OBVH)
            assert np.array_equal(bits(acc[j]), bits(ref_acc)), "mode %d view %d: accumulator differs from the oracle" % (mode, j)
            assert np.array_equal(bits(out[j]), bits(ref_out)), "mode %d view %d: image differs from the oracle" % (mode, j)
            rays = [rays[0] + ref_st.rays_closest, rays[1] + ref_st.rays_shadow]
        assert [st.rays_closest, st.rays_shadow] == rays
    ctx.close()


# ---- 2. every integrator path against per-view rt_render -------------------------------------------------------------
CASES = [
    dict(),                                            # pooled direct lighting (the persistent kernel)
    dict(no_pool=True),                                # sequential direct lighting (reserved[1] bit 0)
    dict(accel=pyrt.ACCEL_BRUTE),
    dict(lanes_per_pixel=1),                           # explicit reserved[0]
    dict(lanes_per_pixel=64),
    dict(collect_stats=1),
    dict(photons=10), dict(photons=64),                # photon shading: k <= 16 and the wide walk
]


def _case_id(c):
    return "-".join("%s%s" % kv for kv in c.items()) or "pooled"


# (photon frames on hires only; the exhaustive loop over the million triangles of stress at a smaller frame)
PER_VIEW = [pytest.param("hires", 21, 19, c, id="hires-" + _case_id(c)) for c in CASES] + \
           [pytest.param("stress", 8 if c.get("accel") else 16, 6 if c.get("accel") else 12, c, id="stress-" + _case_id(c))
            for c in CASES if "photons" not in c]


@pytest.mark.parametrize("kind,w,h,case", PER_VIEW)
def test_views_equal_per_view_render(kind, w, h, case):
    case = dict(case)
    k = case.pop("photons", 0)
    s = pyrt.Scene(kind, w, h)
    a = s.arrays()
    ctx, ref = pyrt.Context(s), pyrt.Context(s)
    spp = 4
    if k:
        for c in (ctx, ref):
            c.build_photon_map(3000, seed=2)
        case.update(use_photons=1, k=k, photons_requested=3000)
        spp = 2
    cams = orbit(a["camera"], [20.0, 150.0, -90.0], [1.3, 0.8, 1.0])
    p = pyrt.make_params(w, h, spp, mode=pyrt.MODE_PATH, seed=9, **case)
    st = assert_views_equal_per_view(ctx, ref, p, cams, [3, 4, 5], pyrt.background(w, h))
    if case.get("collect_stats"):
        assert st.nodes_visited > 0
    ctx.close(), ref.close()


# ---- 3. one view is rt_render ------------------------------------------------------------------------------------------
def test_one_view_is_render():
    s = pyrt.Scene("cubes", 40, 24)
    ctx = pyrt.Context(s)
    bg = pyrt.background(40, 24)
    p = pyrt.make_params(40, 24, 8, mode=pyrt.MODE_PATH, seed=7)
    out, acc, st = ctx.render_views(p, s.arrays()["camera"][None], bg)
    rout, racc, rst = ctx.render(p, bg)
    assert np.array_equal(bits(acc[0]), bits(racc)) and np.array_equal(bits(out[0]), bits(rout))
    assert (st.rays_closest, st.rays_shadow, st.samples) == (rst.rays_closest, rst.rays_shadow, rst.samples)
    ctx.close()


# ---- 4. many small views -----------------------------------------------------------------------------------------------
def test_many_small_views():
    s = pyrt.Scene("cubes", 16, 16)
    a = s.arrays()
    ctx, ref = pyrt.Context(s), pyrt.Context(s)
    n = 256
    cams = orbit(a["camera"], np.linspace(0, 360, n, endpoint=False), np.linspace(0.6, 1.8, n))
    seeds = np.arange(n, dtype=np.uint32) * 7 + 1
    assert_views_equal_per_view(ctx, ref, pyrt.make_params(16, 16, 4, mode=pyrt.MODE_PATH), cams, seeds)
    ctx.close(), ref.close()


# ---- 5. the device form ------------------------------------------------------------------------------------------------
def test_device_form_chains_and_resolves():
    w, h, spp = 29, 21, 8
    s = pyrt.Scene("lowres", w, h)
    a = s.arrays()
    ctx = pyrt.Context(s)
    cams = orbit(a["camera"], [0.0, 45.0, 200.0, 300.0], [1.0, 1.2, 0.9, 2.0])
    seeds = [1, 2, 3, 4]
    bg = pyrt.background(w, h)
    host_out, host_acc, _ = ctx.render_views(pyrt.make_params(w, h, spp, seed=1), cams, bg, seeds=seeds)
    d_acc = torch.zeros((4, h, w, 4), dtype=torch.float32, device="cuda")
    for b, c in ((0, 3), (3, 5)):
        p = pyrt.make_params(w, h, spp, seed=1, spp_begin=b, spp_count=c)
        ctx.render_views_device(p, cams, d_acc.data_ptr(), seeds=seeds)
    torch.cuda.synchronize()
    assert np.array_equal(bits(d_acc.cpu().numpy()), bits(host_acc))
    d_bg = torch.from_numpy(bg).cuda()
    d_out = torch.empty((4, h, w, 3), dtype=torch.float32, device="cuda")
    for j in range(4):
        ctx.resolve_device(w, h, spp, d_acc[j].data_ptr(), d_bg.data_ptr(), d_out[j].data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(bits(d_out.cpu().numpy()), bits(host_out))
    st = ctx.render_views_device(pyrt.make_params(w, h, spp, seed=1), cams, torch.zeros_like(d_acc).data_ptr(), seeds=seeds,
                                 stats=True)
    assert st.samples == 4 * w * h * spp and st.rays_closest > 0 and st.kernel_ms > 0
    ctx.close()


# ---- 6. the context's state --------------------------------------------------------------------------------------------
def test_context_state():
    w, h = 24, 20
    s = pyrt.Scene("cubes", w, h)
    a = s.arrays()
    ctx = pyrt.Context(s)
    nph = 4000
    ctx.build_photon_map(nph, seed=4)
    pp = pyrt.make_params(w, h, 2, mode=pyrt.MODE_RAY, seed=3, use_photons=1, k=10, photons_requested=nph)
    p = pyrt.make_params(w, h, 4, seed=6)
    _, before, _ = ctx.render(p)
    _, ph_before, _ = ctx.render(pp)
    pad0 = ctx.bvh_info().pad
    assert pad0 == pad_rule(a)
    near = orbit(a["camera"], [30.0, -30.0], [0.8, 0.9])
    ctx.render_views(p, near)
    assert ctx.bvh_info().pad == pad0  # covered by the current padding: nothing changes
    far = orbit(a["camera"], [10.0, 70.0, -120.0], [3.0, 9.0, 5.0])
    ref = pyrt.Context(s)
    ref.build_photon_map(nph, seed=4)
    assert_views_equal_per_view(ctx, ref, p, far, None)
    farthest = far[int(np.argmax([pad_rule(dict(a, camera=c)) for c in far]))]
    assert ctx.bvh_info().pad == pad_rule(dict(a, camera=farthest)) > pad0
    _, after, _ = ctx.render(p)
    assert np.array_equal(bits(before), bits(after))  # the context's camera did not move
    _, ph_after, _ = ctx.render(pp)  # the photon map survived
    assert np.array_equal(bits(ph_before), bits(ph_after))
    assert_views_equal_per_view(ctx, ref, pp, far, [1, 2, 3])
    ctx.close(), ref.close()


# ---- 7. rejections -----------------------------------------------------------------------------------------------------
def _raw(ctx, p, cams, n=None, out=None, acc=None):
    v, keep = pyrt.make_views(cams)
    if n is not None:
        v.n_views = n
    bg = pyrt.background(p.width, p.height)
    ptr = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)
    return pyrt.amd().rt_render_views(ctx._h, C.byref(p), C.byref(v), ptr(bg), ptr(out), ptr(acc), None)


def test_rejections_write_nothing():
    w, h = 16, 16
    s = pyrt.Scene("cubes", w, h)
    a = s.arrays()
    ctx = pyrt.Context(s)
    cams = orbit(a["camera"], [0.0, 20.0], [1.0, 1.1])
    out = np.full((2, h, w, 3), 5.0, np.float32)
    acc = np.full((2, h, w, 4), 5.0, np.float32)
    p = pyrt.make_params(w, h, 2)
    bad = cams.copy()
    bad[1, 2, 0] = np.nan
    assert _raw(ctx, p, bad, out=out, acc=acc) == 1 and b"view 1" in pyrt.amd().rt_last_error()
    bad = cams.copy()
    bad[0, 0, 1] = np.inf
    assert _raw(ctx, p, bad, out=out, acc=acc) == 1 and b"view 0" in pyrt.amd().rt_last_error()
    assert _raw(ctx, p, cams, n=0, out=out, acc=acc) == 1
    big = np.repeat(cams[:1], 65536, axis=0)
    assert _raw(ctx, pyrt.make_params(1, 1, 1), big, out=out, acc=acc) == 1
    assert _raw(ctx, pyrt.make_params(w, h, 2, world=2), cams, out=out, acc=acc) == 4
    assert _raw(ctx, pyrt.make_params(w, h, 2, wavefront=True), cams, out=out, acc=acc) == 4
    assert _raw(ctx, pyrt.make_params(w, h, 2, use_photons=1, k=4, photons_requested=100), cams, out=out, acc=acc) == 5
    assert (out == 5.0).all() and (acc == 5.0).all()
    # the padding did not move either
    assert ctx.bvh_info().pad == pad_rule(a)
    ctx.close()


def test_q8_context_renders_covered_views_and_refuses_a_refit():
    w, h = 20, 16
    s = pyrt.Scene("lowres", w, h)
    a = s.arrays()
    q8, ref = pyrt.Context(s, node_format=pyrt.NODES_Q8), pyrt.Context(s)
    assert q8.bvh_info().node_format == pyrt.NODES_Q8
    p = pyrt.make_params(w, h, 4, seed=2)
    near = orbit(a["camera"], [15.0, -40.0, 90.0], [0.7, 0.9, 0.5])
    assert_views_equal_per_view(q8, ref, p, near, [7, 8, 9], pyrt.background(w, h))
    far = orbit(a["camera"], [15.0], [6.0])
    out = np.full((1, h, w, 3), 5.0, np.float32)
    assert _raw(q8, p, far, out=out) == 4 and (out == 5.0).all()
    q8.close(), ref.close()
