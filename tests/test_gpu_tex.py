"""rt_set_textures, rt_render_textured and rt_render_aov_textured, bit for bit against tests/tex_ref.py — the oracle's
rays, hits, BSDF and light evaluation under the sampled albedo — on tex_ref.CASES: accumulator, resolved image, samples
and both ray counts under the eight schedules of test_gpu_lights.SCHEDULES; then T1 against the library's own rt_render,
T2 against rt_render_colors and against rt_render on a second context of the per-triangle-mesh scene, chained ranges,
host against device form, a Q8 context, two sets with frames between them back to back on a busy non-blocking stream, the
set kept across rt_update and rt_rebuild, the release, an untouched context, and the textured AOV pass, whose albedo
channel at one sample is the first hit's sample on its own."""
import ctypes as C

import numpy as np
import pytest

import pyrt
import tex_ref
from busystream import Busy
from test_gpu_lights import SCHEDULES, assert_frames_equal, bits
from tex_ref import T_ALBEDO, T_FACES, T_MIXED, T_NONE, set_args

pytestmark = pytest.mark.gpu

INVALID, STATE = 1, 5
F32 = np.float32
_ctx = {}


@pytest.fixture(scope="module", autouse=True)
def contexts():
    yield
    for c in _ctx.values():
        c.close()
    _ctx.clear()


def context(c, **kw):
    """One context per case's scene and texture set and option set, with the case's set resident."""
    key = (tex_ref.case_id(c) if c[6] == T_MIXED else (c[0], c[1], c[2], c[6]), tuple(sorted(kw.items())))
    if key not in _ctx:
        _ctx[key] = pyrt.Context(tex_ref.case_scene(c), **kw)
        _ctx[key].set_textures(*set_args(tex_ref.case_textures(c)))
    return _ctx[key]


def samples_of(c):
    p = tex_ref.case_params(c)
    return c[1] * c[2] * (p.spp_count if p.spp_count else p.spp)


def first(kind, field, value):
    """The first case of a texturing whose field (an index into the case) is value."""
    return next(c for c in tex_ref.CASES if c[6] == kind and c[field] == value)


def check(got, ref, what):
    out, acc, st = got
    assert_frames_equal(acc, ref["accum"], "accum " + what)
    assert_frames_equal(out, ref["out"], "out " + what)
    assert (st.rays_closest, st.rays_shadow) == (ref["closest"], ref["shadow"]), what


@pytest.mark.parametrize("case", tex_ref.CASES, ids=tex_ref.case_id)
def test_textured_bit_exact(case):
    """Accumulator, resolved image, samples and both ray counts, whatever the schedule (T4)."""
    ctx, bg = context(case), tex_ref.case_background(case)
    for name, kw, brute in SCHEDULES:
        ref = tex_ref.case_reference(case, brute)
        what = "%s, %s" % (tex_ref.case_id(case), name)
        out, acc, st = ctx.render_textured(tex_ref.case_params(case, **kw), bg=bg)
        check((out, acc, st), ref, what)
        assert st.samples == samples_of(case) and st.kernel_ms > 0, what
        if kw.get("collect_stats"):
            assert st.tris_tested > 0 and (brute or st.nodes_visited > st.rays_closest), what


def test_the_mixed_texturing_shows():
    """The frames the cases compare are not the plain ones (tex_ref.MIN_CHANGED, from the oracle alone)."""
    for case in tex_ref.CASES:
        if case[6] == T_MIXED:
            ctx = context(case)
            _, plain, _ = ctx.render(tex_ref.case_params(case))
            _, acc, _ = ctx.render_textured(tex_ref.case_params(case))
            assert tex_ref.changed_rgb_words(acc, plain) > tex_ref.MIN_CHANGED, tex_ref.case_id(case)
            assert (bits(acc[..., 3]) == bits(plain[..., 3])).all()


@pytest.mark.parametrize("kind", [T_NONE, T_ALBEDO])
@pytest.mark.parametrize("case", tex_ref.CASES[::2], ids=tex_ref.case_id)
def test_t1_no_texture_and_albedo_texels_are_rt_render(case, kind):
    """T1 on the library's own frames, under every schedule: accumulator, image, samples and both ray counts."""
    s, bg = tex_ref.case_scene(case), tex_ref.case_background(case)
    ctx = pyrt.Context(s)
    try:
        ctx.set_textures(*set_args(tex_ref.texture_set(s, kind)))
        for name, kw, _ in SCHEDULES:
            p = tex_ref.case_params(case, **kw)
            eout, eacc, est = ctx.render(p, bg)
            out, acc, st = ctx.render_textured(p, bg=bg)
            check((out, acc, st), dict(accum=eacc, out=eout, closest=est.rays_closest, shadow=est.rays_shadow), "%s, %s" % (kind, name))
            assert st.samples == est.samples, name
    finally:
        ctx.close()


@pytest.mark.parametrize("case", [c for c in tex_ref.CASES if c[6] == T_FACES], ids=tex_ref.case_id)
def test_t2_the_strip_texture_is_rt_render_colors_and_rt_render_of_one_mesh_per_triangle(case):
    ctx, bg = context(case), tex_ref.case_background(case)
    rgb, tri_scene = tex_ref.case_face_colors(case)
    ctx.set_vertex_colors(rgb)
    other = pyrt.Context(tri_scene)
    try:
        for name, kw, _ in SCHEDULES[:2] + SCHEDULES[6:7]:
            p = tex_ref.case_params(case, **kw)
            got = ctx.render_textured(p, bg=bg)
            for what, (eout, eacc, est) in (("rt_render_colors", ctx.render_colors(p, bg=bg)), ("rt_render", other.render(p, bg))):
                check(got, dict(accum=eacc, out=eout, closest=est.rays_closest, shadow=est.rays_shadow), "%s, %s" % (what, name))
                assert got[2].samples == est.samples, name
    finally:
        other.close()
        ctx.set_vertex_colors(None)


@pytest.mark.parametrize("pooled", [True, False])
def test_sample_ranges_chain_and_host_equals_device(pooled):
    """T3: [0, 3) then [3, 7) into one device accumulator is [0, 7), which is the host form's frame; the tail alone is the
    [3, 7) case's own reference; the accumulator resolves with rt_resolve_device to the host form's image."""
    import torch
    tail = first(T_MIXED, 3, tex_ref.SPP7_34)
    w, h = tail[1], tail[2]
    kw = dict() if pooled else dict(no_pool=True)
    ctx, bg = context(tail), tex_ref.case_background(tail)
    acc = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    whole = torch.zeros_like(acc)
    stream = torch.cuda.current_stream()
    for b, cnt in ((0, 3), (3, 4)):
        ctx.render_textured_device(tex_ref.case_params(tail, spp_begin=b, spp_count=cnt, **kw), acc.data_ptr(), stream=stream.cuda_stream)
        if b == 0:
            stream.synchronize()
            head = acc.cpu().numpy().copy()
    full = tex_ref.case_params(tail, spp_begin=0, spp_count=0, **kw)
    st = ctx.render_textured_device(full, whole.data_ptr(), stream=stream.cuda_stream, stats=True)
    dbg = torch.from_numpy(bg).cuda()
    dout = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
    ctx.resolve_device(w, h, full.spp, whole.data_ptr(), dbg.data_ptr(), dout.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    hout, host, hst = ctx.render_textured(full, bg=bg)
    assert_frames_equal(whole.cpu().numpy(), host, "device form against host form")
    assert_frames_equal(dout.cpu().numpy(), hout, "rt_resolve_device against the host form's image")
    assert (st.rays_closest, st.rays_shadow, st.samples) == (hst.rays_closest, hst.rays_shadow, hst.samples)
    assert_frames_equal(acc.cpu().numpy(), host, "[0, 3) then [3, 7)")
    assert head[..., 3].max() == 3 and (bits(head) != bits(host)).any()
    _, alone, _ = ctx.render_textured(tex_ref.case_params(tail, **kw))
    assert_frames_equal(alone, tex_ref.case_reference(tail)["accum"], "[3, 7) alone")
    only, _, _ = ctx.render_textured(full, bg=bg, want_accum=False)
    assert_frames_equal(only, hout, "the image alone")


def test_q8_context_gives_the_same_bits():
    """An RT_NODES_Q8 context walks its resident 32-byte records: the same frame."""
    case = first(T_MIXED, 0, ("lowres", True))
    ctx = context(case, bvh_builder=pyrt.BVH_HOST, node_format=pyrt.NODES_Q8)
    assert ctx.bvh_info().node_format == pyrt.NODES_Q8
    ref = tex_ref.case_reference(case)
    for no_pool in (False, True):
        _, acc, st = ctx.render_textured(tex_ref.case_params(case, no_pool=no_pool))
        assert_frames_equal(acc, ref["accum"], "Q8 context")
        assert (st.rays_closest, st.rays_shadow) == (ref["closest"], ref["shadow"])


def test_two_sets_with_frames_between_them_on_a_busy_non_blocking_stream():
    """set A, a frame, set B, a frame, on a non-blocking stream that is still busy: the first frame reads A — the arrays
    it replaces are freed only once the launches that read them have run — and the second B."""
    case = first(T_MIXED, 0, ("cubes", False))
    s, (w, h) = tex_ref.case_scene(case), case[1:3]
    set_a, set_b = tex_ref.case_textures(case), tex_ref.texture_set(s, T_ALBEDO)
    ctx = pyrt.Context(s)
    busy = Busy()
    acc_a = busy.out((h, w, 4), zeroed=True)
    acc_b = busy.out((h, w, 4), zeroed=True)
    ctx.set_textures(*set_args(set_a))
    busy.start()
    ctx.render_textured_device(tex_ref.case_params(case), acc_a.ptr, stream=busy.ptr)
    was_busy = busy.issued()
    ctx.set_textures(*set_args(set_b))
    ctx.render_textured_device(tex_ref.case_params(case), acc_b.ptr, stream=busy.ptr)
    got_a, got_b = busy.fetch(acc_a), busy.fetch(acc_b)
    busy.finish()
    _, plain, _ = ctx.render(tex_ref.case_params(case))
    ctx.close()
    assert_frames_equal(got_a.numpy(), tex_ref.case_reference(case)["accum"], "first set")
    assert_frames_equal(got_b.numpy(), plain, "second set (T1)")
    assert (bits(got_a.numpy()) != bits(got_b.numpy())).any()
    assert was_busy, "the delay ended before the first call was issued (%.3f ms)" % busy.issue_ms


def test_the_set_stays_across_rt_update_and_rt_rebuild():
    """New vertex positions refit the tree, rt_rebuild builds it again: the uvs are indexed by vertex id and stay."""
    case = first(T_MIXED, 0, ("cubes", True))
    s = tex_ref.case_scene(case)
    a = s.arrays()
    pos = (a["pos"] * F32(1.03) + F32(0.01)).astype(F32)
    moved = pyrt.ArrayScene(pos, a["nrm"], a["tri"], a["tri_begin"], a["vtx_begin"], a["materials"], a["lights"], a["camera"])
    p = tex_ref.case_params(case)
    exp = tex_ref.frame(moved, p, tex_ref.case_textures(case))
    ctx = pyrt.Context(s)
    try:
        ctx.set_textures(*set_args(tex_ref.case_textures(case)))
        ctx.update(pos=pos)
        _, acc, st = ctx.render_textured(p)
        assert_frames_equal(acc, exp["accum"], "after rt_update")
        assert (st.rays_closest, st.rays_shadow) == (exp["closest"], exp["shadow"])
        ctx.rebuild()
        _, acc, st = ctx.render_textured(p)
        assert_frames_equal(acc, exp["accum"], "after rt_rebuild")
        assert (bits(exp["accum"]) != bits(tex_ref.case_reference(case)["accum"])).any()
    finally:
        ctx.close()


def test_release_then_state_and_the_rejections_that_read_the_context():
    """A context without a set answers the render calls with RT_ERR_STATE and writes nothing; counts that are not the
    context's are RT_ERR_INVALID; a NULL call releases the set."""
    L = pyrt.amd()
    case = tex_ref.CASES[0]
    w, h, p = case[1], case[2], tex_ref.case_params(case)
    s = tex_ref.case_scene(case)
    t = tex_ref.case_textures(case)
    nv, nm = len(s.arrays()["pos"]), len(s.arrays()["tri_begin"]) - 1
    acc = np.full((h, w, 4), 3.0, F32)
    ptr = lambda x: x.ctypes.data_as(C.c_void_p)
    ctx = pyrt.Context(s)
    try:
        def frame_calls():
            import torch
            d = torch.full((h, w, 4), 3.0, dtype=torch.float32, device="cuda")
            a = pyrt.Aov()
            alb = np.full((h, w, 3), 3.0, F32)
            a.albedo = alb.ctypes.data
            rcs = [L.rt_render_textured(ctx._h, C.byref(p), None, None, ptr(acc), None),
                   L.rt_render_textured_device(ctx._h, C.byref(p), C.c_void_p(d.data_ptr()), None, None),
                   L.rt_render_aov_textured(ctx._h, C.byref(p), C.byref(a))]
            torch.cuda.synchronize()
            return rcs, (acc == 3).all() and bool((d == 3).all()) and (alb == 3).all()

        rcs, untouched = frame_calls()
        assert rcs == [STATE] * 3 and untouched and b"rt_set_textures" in L.rt_last_error()
        for n in (nv - 1, nv + 1, 0):
            ts, keep = pyrt.texture_set(t["textures"], t["mesh_texture"], np.zeros((n, 2), F32))
            assert L.rt_set_textures(ctx._h, C.byref(ts)) == INVALID
            assert b"%d vertices" % n in L.rt_last_error() and b"of %d" % nv in L.rt_last_error(), L.rt_last_error()
        for n in (nm - 1, nm + 1):
            ts, keep = pyrt.texture_set(t["textures"], np.zeros(n, np.uint32), t["uv"])
            assert L.rt_set_textures(ctx._h, C.byref(ts)) == INVALID
            assert b"%d meshes" % n in L.rt_last_error() and b"of %d" % nm in L.rt_last_error(), L.rt_last_error()
        rcs, untouched = frame_calls()
        assert rcs == [STATE] * 3 and untouched
        ctx.set_textures(*set_args(t))
        _, got, _ = ctx.render_textured(p)
        assert_frames_equal(got, tex_ref.case_reference(case)["accum"], "after the rejected calls")
        # a refused set leaves the resident one in place
        ts, keep = pyrt.texture_set(t["textures"], t["mesh_texture"], np.zeros((nv + 1, 2), F32))
        assert L.rt_set_textures(ctx._h, C.byref(ts)) == INVALID
        _, got, _ = ctx.render_textured(p)
        assert_frames_equal(got, tex_ref.case_reference(case)["accum"], "after a refused set")
        ctx.set_textures(None)
        rcs, untouched = frame_calls()
        assert rcs == [STATE] * 3 and untouched
        ctx.set_textures(None)  # (releasing nothing is not an error)
    finally:
        ctx.close()


def test_context_untouched_and_vertex_colours_not_read():
    """rt_set_textures and the textured calls change nothing rt_render, rt_render_aov or rt_render_colors read, and
    resident vertex colours change nothing of a textured frame; a context that never called rt_set_textures renders as
    it did."""
    import vcol_ref
    case = tex_ref.CASES[0]
    s = tex_ref.case_scene(case)
    ctx = pyrt.Context(s)
    fp = pyrt.make_params(case[1], case[2], 4, seed=3)
    colors = vcol_ref.smooth_colors(s)
    ctx.set_vertex_colors(colors)
    _, frame0, st0 = ctx.render(fp)
    _, col0, _ = ctx.render_colors(fp)
    aov0 = ctx.render_aov(fp, raw=True)
    info0 = ctx.bvh_info()
    ctx.set_textures(*set_args(tex_ref.case_textures(case)))
    _, tex1, _ = ctx.render_textured(tex_ref.case_params(case))
    ctx.render_aov_textured(fp)
    _, frame1, st1 = ctx.render(fp)
    _, col1, _ = ctx.render_colors(fp)
    aov1 = ctx.render_aov(fp, raw=True)
    assert (ctx.bvh_info().pad, ctx.bvh_info().n_nodes) == (info0.pad, info0.n_nodes)
    ctx.close()
    assert_frames_equal(tex1, tex_ref.case_reference(case)["accum"], "with vertex colours resident")
    assert (bits(frame0) == bits(frame1)).all() and (bits(col0) == bits(col1)).all()
    assert (st0.rays_closest, st0.rays_shadow) == (st1.rays_closest, st1.rays_shadow)
    for k in aov0:
        assert (bits(aov0[k]) == bits(aov1[k])).all(), k


@pytest.mark.parametrize("case", [c for c in tex_ref.CASES if c[6] in (T_MIXED, T_FACES)][::2], ids=tex_ref.case_id)
def test_aov_textured(case):
    """The albedo channel is the reference's first-hit sums of c (at one sample: the first hit's sample itself, the
    sampler outside shading); every other channel is rt_render_aov's bit for bit; the device form writes the same sums;
    the exhaustive loop the same."""
    import torch
    ctx, p = context(case), tex_ref.case_params(case)
    ref = tex_ref.case_reference(case)
    plain = ctx.render_aov(p, raw=True)
    for accel in (pyrt.ACCEL_BVH, pyrt.ACCEL_BRUTE):
        got = ctx.render_aov_textured(tex_ref.case_params(case, accel=accel), raw=True)
        assert_frames_equal(got["albedo"], ref["albedo"], "albedo")
        for k in plain:
            if k != "albedo":
                assert (bits(got[k]) == bits(plain[k])).all(), k
    assert (bits(got["albedo"]) != bits(plain["albedo"])).any()
    h, w = case[2], case[1]
    d = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
    ctx.render_aov_textured_device(p, dict(albedo=d.data_ptr()), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert_frames_equal(d.cpu().numpy(), ref["albedo"], "device form")


def test_the_sampler_alone_at_one_sample_per_pixel():
    """Every T_MIXED case's first sample alone (spp_count 1): the albedo channel is the first hit's c, no sums."""
    for case in tex_ref.CASES:
        if case[6] != T_MIXED:
            continue
        rng = tex_ref.case_params(case)
        one = tex_ref.case_params(case, spp_begin=rng.spp_begin, spp_count=1)
        exp = tex_ref.frame(tex_ref.case_scene(case), one, tex_ref.case_textures(case), touched=False)
        got = context(case).render_aov_textured(one, raw=True)
        assert got["hits"].max() == 1
        assert_frames_equal(got["albedo"], exp["albedo"], tex_ref.case_id(case))
