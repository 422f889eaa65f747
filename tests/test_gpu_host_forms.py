"""The host forms of the integrators share one staging, stats and scratch path.  What that path makes
common and the other suites exercise in one variant only, on the cubes scene at 16x12, 2 spp, path mode: every allowed
combination of optional outputs against the call with all of them, scratch that grows and is used small again against
fresh contexts, the stats of the three timed forms against their device forms and the header's sample counts, and
rt_render_passes over two ranges against one rt_render."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import pyrt

pytestmark = pytest.mark.gpu

W, H, SPP, NRAYS = 16, 12, 2, 70


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def params(w=W, h=H, **kw):
    return pyrt.make_params(w, h, SPP, mode=pyrt.MODE_PATH, seed=5, **kw)


@pytest.fixture(scope="module")
def scene():
    s = pyrt.Scene("cubes", W, H)
    yield s
    s.close()


@pytest.fixture(scope="module")
def ctx(scene):
    c = pyrt.Context(scene)
    yield c
    c.close()


def cameras(scene, n):
    """n views from the scene camera's position (no view is farther: no refit), each window shifted sideways."""
    cam = np.asarray(scene.arrays()["camera"], np.float32).reshape(4, 3)
    out = np.repeat(cam[None], n, axis=0)
    for j in range(n):
        out[j, 1] = cam[1] + np.float32(0.05 * j) * cam[2]
    return out


def rays_of(scene, n):
    return pyrt.pixel_rays(scene.arrays()["camera"], W, H)[:n].copy()


def permutation(n):
    return np.random.default_rng(3).permutation(n).astype(np.uint32)


def stats_dict(st):
    d = st.as_dict()
    d.pop("kernel_ms")
    return d


# ---- optional outputs: each returned buffer equals the one of the call that asks for everything ------------------------
def call_render(ctx, p, bg, want_out, want_acc, want_stats=True):
    out = np.full((p.height, p.width, 3), 7, np.float32) if want_out else None
    acc = np.full((p.height, p.width, 4), 7, np.float32) if want_acc else None
    st = pyrt.Stats()
    pyrt._check(pyrt.amd().rt_render(ctx._h, C.byref(p), pyrt._ptr(bg), pyrt._ptr(out), pyrt._ptr(acc),
                                     C.byref(st) if want_stats else None))
    return out, acc


def call_views(ctx, p, cams, bg, want_out, want_acc, want_stats=True):
    v, _keep = pyrt.make_views(cams)
    n = v.n_views
    out = np.full((n, p.height, p.width, 3), 7, np.float32) if want_out else None
    acc = np.full((n, p.height, p.width, 4), 7, np.float32) if want_acc else None
    st = pyrt.Stats()
    pyrt._check(pyrt.amd().rt_render_views(ctx._h, C.byref(p), C.byref(v), pyrt._ptr(bg), pyrt._ptr(out), pyrt._ptr(acc),
                                           C.byref(st) if want_stats else None))
    return out, acc


def call_rays(ctx, p, rays, idx, bg, want_out, want_acc, want_stats=True):
    b = pyrt.RayBatch()
    b.n, b.rays, b.stream_index = len(rays), rays.ctypes.data, None if idx is None else idx.ctypes.data
    out = np.full((len(rays), 3), 7, np.float32) if want_out else None
    acc = np.full((len(rays), 4), 7, np.float32) if want_acc else None
    st = pyrt.Stats()
    pyrt._check(pyrt.amd().rt_render_rays(ctx._h, C.byref(p), C.byref(b), pyrt._ptr(bg), pyrt._ptr(out), pyrt._ptr(acc),
                                          C.byref(st) if want_stats else None))
    return out, acc


def call_adaptive(ctx, p, bg, want_acc, want_spp, want_rep=True, want_stats=True):
    out = np.full((p.height, p.width, 3), 7, np.float32)
    acc = np.full((p.height, p.width, 4), 7, np.float32) if want_acc else None
    spp = np.full((p.height, p.width), 7, np.uint32) if want_spp else None
    rep, st = pyrt.AdaptiveReport(), pyrt.Stats()
    a = pyrt.make_adaptive(0.05, 3, 2)
    pyrt._check(pyrt.amd().rt_render_adaptive(ctx._h, C.byref(p), C.byref(a), pyrt._ptr(bg), pyrt._ptr(out), pyrt._ptr(acc),
                                              pyrt._ptr(spp), C.byref(rep) if want_rep else None,
                                              C.byref(st) if want_stats else None))
    return out, acc, spp


def check_against(full, got, what):
    for name, f, g in zip(("out", "accum", "spp"), full, got):
        if g is not None:
            assert same(f, g), "%s: %s differs from the call with every output" % (what, name)


OUT_ACC = list(itertools.product((True, False), repeat=2))


@pytest.mark.parametrize("want_out,want_acc", OUT_ACC)
def test_render_optional_outputs(ctx, want_out, want_acc):
    p, bg = params(), pyrt.background(W, H)
    full = call_render(ctx, p, bg, True, True)
    assert not (full[0] == 7).all() and not (full[1] == 7).all()
    for want_stats in (True, False):
        # (a call without out_rgb may come without a background too)
        got = call_render(ctx, p, bg if want_out else None, want_out, want_acc, want_stats)
        check_against(full, got, "rt_render out=%d accum=%d stats=%d" % (want_out, want_acc, want_stats))


@pytest.mark.parametrize("want_out,want_acc", OUT_ACC)
def test_views_optional_outputs(ctx, scene, want_out, want_acc):
    p, bg, cams = params(), pyrt.background(W, H), cameras(scene, 3)
    full = call_views(ctx, p, cams, bg, True, True)
    assert not same(full[1][0], full[1][1]) and not same(full[1][1], full[1][2])
    for want_stats in (True, False):
        got = call_views(ctx, p, cams, bg if want_out else None, want_out, want_acc, want_stats)
        check_against(full, got, "rt_render_views out=%d accum=%d stats=%d" % (want_out, want_acc, want_stats))


@pytest.mark.parametrize("indexed", (False, True), ids=("own_index", "stream_index"))
@pytest.mark.parametrize("want_out,want_acc", [c for c in OUT_ACC if c != (False, False)])  # (neither: rejected)
def test_rays_optional_outputs(ctx, scene, want_out, want_acc, indexed):
    p, rays = params(), rays_of(scene, NRAYS)
    idx = permutation(NRAYS) if indexed else None
    bg = np.ascontiguousarray(pyrt.background(W, H).reshape(-1, 3)[:NRAYS])
    full = call_rays(ctx, p, rays, idx, bg, True, True)
    assert not (full[1] == 7).all()
    for want_stats in (True, False):
        got = call_rays(ctx, p, rays, idx, bg if want_out else None, want_out, want_acc, want_stats)
        check_against(full, got, "rt_render_rays out=%d accum=%d stats=%d" % (want_out, want_acc, want_stats))


@pytest.mark.parametrize("want_acc,want_spp", OUT_ACC)
def test_adaptive_optional_outputs(ctx, want_acc, want_spp):
    p, bg = params(), pyrt.background(W, H)
    full = call_adaptive(ctx, p, bg, True, True)
    assert full[2].min() >= SPP and full[2].max() <= 3 * SPP
    for want_rep, want_stats in ((True, True), (False, False)):
        got = call_adaptive(ctx, p, bg, want_acc, want_spp, want_rep, want_stats)
        check_against(full, got, "rt_render_adaptive accum=%d spp=%d rep/stats=%d" % (want_acc, want_spp, want_rep))


# ---- scratch that grows: small, larger, small again on one context, each as on a fresh context ------------------------
def grown(scene, steps, call):
    """call(ctx, step) for every step on ONE context against the same call on a context of its own."""
    one = pyrt.Context(scene)
    try:
        for i, step in enumerate(steps):
            got = call(one, step)
            fresh = pyrt.Context(scene)
            try:
                exp = call(fresh, step)
            finally:
                fresh.close()
            for g, e in zip(got, exp):
                assert same(g, e), "call %d (%r) on the used context differs from a fresh context's" % (i, step)
    finally:
        one.close()


def test_views_scratch_grows(scene):
    bg = pyrt.background(W, H)
    grown(scene, (1, 3, 1), lambda c, n: c.render_views(params(), cameras(scene, n), bg)[:2])


def test_rays_scratch_grows(scene):
    def call(c, step):
        n, indexed = step
        bg = np.ascontiguousarray(pyrt.background(W, H).reshape(-1, 3)[:n])
        return c.render_rays(params(), rays_of(scene, n), bg=bg, stream_index=permutation(n) if indexed else None)[:2]
    grown(scene, ((5, False), (NRAYS, True), (5, False)), call)


def test_denoise_scratch_grows(ctx, scene):
    frames = {}
    for w, h in ((8, 8), (24, 16)):
        p = params(w, h)
        frames[(w, h)] = (ctx.render(p, pyrt.background(w, h))[0], ctx.render_aov(p, raw=True))
    grown(scene, ((8, 8), (24, 16), (8, 8)), lambda c, wh: (c.denoise(*frames[wh]),))


def test_adaptive_scratch_grows(scene):
    def call(c, wh):
        return c.render_adaptive(params(*wh), pyrt.background(*wh), 0.05, 3, 2)[:3]
    grown(scene, ((8, 8), (24, 16), (8, 8)), call)


# ---- stats: the device form's counters, the header's sample counts ------------------------------------------------------
RANGES = [dict(), dict(spp_begin=1, spp_count=1, collect_stats=1)]
RANGE_IDS = ["all_samples", "one_sample_counted"]


def sample_count(rng):
    return rng.get("spp_count", SPP)


def device_accum(rows):
    return torch.zeros((rows, 4), dtype=torch.float32, device="cuda")


@pytest.mark.parametrize("rng", RANGES, ids=RANGE_IDS)
@pytest.mark.parametrize("w,h", [(W, H), (13, 9)])  # (13x9: the last granule column and row are clipped)
def test_render_stats(ctx, w, h, rng):
    p = params(w, h, **rng)
    _, acc, st = ctx.render(p, pyrt.background(w, h))
    d_acc = device_accum(w * h)
    dst = ctx.render_device(p, d_acc.data_ptr(), stream=torch.cuda.current_stream().cuda_stream, stats=True)
    torch.cuda.synchronize()
    assert same(acc.reshape(-1, 4), d_acc.cpu().numpy())
    assert stats_dict(st) == stats_dict(dst)
    assert st.samples == w * h * sample_count(rng)  # owned pixels (all of them: world 1) x samples of the range
    assert st.rays_closest > 0 and st.kernel_ms > 0 and dst.kernel_ms > 0
    if rng.get("collect_stats"):
        assert st.nodes_visited > 0 and st.tris_tested > 0


@pytest.mark.parametrize("rng", RANGES, ids=RANGE_IDS)
def test_views_stats(ctx, scene, rng):
    p, cams = params(**rng), cameras(scene, 3)
    _, acc, st = ctx.render_views(p, cams, pyrt.background(W, H))
    d_acc = device_accum(3 * W * H)
    dst = ctx.render_views_device(p, cams, d_acc.data_ptr(), stream=torch.cuda.current_stream().cuda_stream, stats=True)
    torch.cuda.synchronize()
    assert same(acc.reshape(-1, 4), d_acc.cpu().numpy())
    assert stats_dict(st) == stats_dict(dst)
    assert st.samples == 3 * W * H * sample_count(rng)
    assert st.rays_closest > 0 and st.kernel_ms > 0 and dst.kernel_ms > 0


@pytest.mark.parametrize("rng", RANGES, ids=RANGE_IDS)
def test_rays_stats(ctx, scene, rng):
    p, rays = params(**rng), rays_of(scene, NRAYS)
    _, acc, st = ctx.render_rays(p, rays)
    d_rays = torch.from_numpy(rays.view(np.float32).reshape(NRAYS, 6).copy()).cuda()
    d_acc = device_accum(NRAYS)
    dst = ctx.render_rays_device(p, d_rays.data_ptr(), NRAYS, d_acc.data_ptr(),
                                 stream=torch.cuda.current_stream().cuda_stream, stats=True)
    torch.cuda.synchronize()
    assert same(acc, d_acc.cpu().numpy())
    assert stats_dict(st) == stats_dict(dst)
    assert st.samples == NRAYS * sample_count(rng)  # n x (s1 - s0)
    assert st.rays_closest > 0 and st.kernel_ms > 0 and dst.kernel_ms > 0


# ---- rt_render_passes: [0, 1) then [1, 2) into one accumulator is one rt_render of 2 spp --------------------------------
def test_passes_chain_to_the_whole_frame(ctx):
    bg = pyrt.background(W, H)
    out, acc, _ = ctx.render(params(), bg)
    acc_io = np.zeros((H, W, 4), np.float32)
    first, _ = ctx.render_passes(params(spp_begin=0, spp_count=1), bg, acc_io)
    assert acc_io.any() and not same(acc_io, acc)
    last, st = ctx.render_passes(params(spp_begin=1, spp_count=1), bg, acc_io)
    assert same(acc_io, acc), "the accumulator of the two ranges differs from the whole frame's"
    assert same(last, out), "the image after the last range differs from the whole frame's"
    assert not same(first, out)  # (resolved over one sample)
    assert st.samples == W * H
