"""rt_set_vertex_colors, rt_render_colors and rt_render_aov_colors, bit for bit against tests/vcol_ref.py — the oracle's
rays, hits, BSDF and light evaluation under the interpolated colour — on vcol_ref.CASES: accumulator, resolved image,
samples and both ray counts under the eight schedules of test_gpu_lights.SCHEDULES; then C1 against the library's own
rt_render, C2 against rt_render on a second context of the per-triangle-mesh scene, chained ranges, host against device
form, a Q8 context, two colourings with frames between them back to back on a busy non-blocking stream, colours kept across
rt_update and rt_rebuild, the release, an untouched context, and the coloured AOV pass."""
import ctypes as C

import numpy as np
import pytest

import pyrt
import vcol_ref
from busystream import Busy
from test_gpu_lights import SCHEDULES, assert_frames_equal, bits
from vcol_ref import ALBEDO, FACES, SMOOTH

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
    """One context per scene, frame aspect, colouring and option set, with the case's colours resident."""
    key = (c[0], c[1], c[2], c[6], tuple(sorted(kw.items())))
    if key not in _ctx:
        _ctx[key] = pyrt.Context(vcol_ref.case_scene(c), **kw)
        _ctx[key].set_vertex_colors(vcol_ref.case_colors(c))
    return _ctx[key]


def samples_of(c):
    p = vcol_ref.case_params(c)
    return c[1] * c[2] * (p.spp_count if p.spp_count else p.spp)


def first(colouring, field, value):
    """The first case of a colouring whose field (an index into the case) is value."""
    return next(c for c in vcol_ref.CASES if c[6] == colouring and c[field] == value)


@pytest.mark.parametrize("case", vcol_ref.CASES, ids=vcol_ref.case_id)
def test_colors_bit_exact(case):
    """Accumulator, resolved image, samples and both ray counts, whatever the schedule (C4)."""
    ctx, bg = context(case), vcol_ref.case_background(case)
    for name, kw, brute in SCHEDULES:
        ref = vcol_ref.case_reference(case, brute)
        what = "%s, %s" % (vcol_ref.case_id(case), name)
        out, acc, st = ctx.render_colors(vcol_ref.case_params(case, **kw), bg=bg)
        assert_frames_equal(acc, ref["accum"], "accum " + what)
        assert_frames_equal(out, ref["out"], "out " + what)
        assert (st.rays_closest, st.rays_shadow) == (ref["closest"], ref["shadow"]), what
        assert st.samples == samples_of(case) and st.kernel_ms > 0, what
        if kw.get("collect_stats"):
            assert st.tris_tested > 0 and (brute or st.nodes_visited > st.rays_closest), what


def test_the_smooth_colouring_shows():
    """The frames the cases compare are not the uncoloured ones (vcol_ref.MIN_CHANGED, from the oracle alone)."""
    for case in vcol_ref.CASES:
        if case[6] == SMOOTH:
            ctx = context(case)
            _, plain, _ = ctx.render(vcol_ref.case_params(case))
            _, acc, _ = ctx.render_colors(vcol_ref.case_params(case))
            assert vcol_ref.changed_rgb_words(acc, plain) > vcol_ref.MIN_CHANGED, vcol_ref.case_id(case)
            assert (bits(acc[..., 3]) == bits(plain[..., 3])).all()


@pytest.mark.parametrize("case", vcol_ref.CASES[::2], ids=vcol_ref.case_id)
def test_c1_the_materials_albedo_is_rt_render(case):
    """C1 on the library's own frames, under every schedule: accumulator, image, samples and both ray counts."""
    s, bg = vcol_ref.case_scene(case), vcol_ref.case_background(case)
    ctx = pyrt.Context(s)
    try:
        ctx.set_vertex_colors(vcol_ref.albedo_colors(s))
        for name, kw, _ in SCHEDULES:
            p = vcol_ref.case_params(case, **kw)
            eout, eacc, est = ctx.render(p, bg)
            out, acc, st = ctx.render_colors(p, bg=bg)
            assert_frames_equal(acc, eacc, "accum " + name)
            assert_frames_equal(out, eout, "out " + name)
            assert (st.rays_closest, st.rays_shadow, st.samples) == (est.rays_closest, est.rays_shadow, est.samples), name
    finally:
        ctx.close()


@pytest.mark.parametrize("case", [c for c in vcol_ref.CASES if c[6] == FACES], ids=vcol_ref.case_id)
def test_c2_one_colour_per_triangle_is_rt_render_of_one_mesh_per_triangle(case):
    ctx, bg = context(case), vcol_ref.case_background(case)
    other = pyrt.Context(vcol_ref.case_triangle_scene(case))
    try:
        for name, kw, _ in SCHEDULES[:2] + SCHEDULES[6:7]:
            p = vcol_ref.case_params(case, **kw)
            eout, eacc, est = other.render(p, bg)
            out, acc, st = ctx.render_colors(p, bg=bg)
            assert_frames_equal(acc, eacc, "accum " + name)
            assert_frames_equal(out, eout, "out " + name)
            assert (st.rays_closest, st.rays_shadow, st.samples) == (est.rays_closest, est.rays_shadow, est.samples), name
    finally:
        other.close()


@pytest.mark.parametrize("pooled", [True, False])
def test_sample_ranges_chain_and_host_equals_device(pooled):
    """C3: [0, 3) then [3, 7) into one device accumulator is [0, 7), which is the host form's frame; the tail alone is the
    [3, 7) case's own reference; the accumulator resolves with rt_resolve_device to the host form's image."""
    import torch
    tail = first(SMOOTH, 3, vcol_ref.SPP7_34)
    w, h = tail[1], tail[2]
    kw = dict() if pooled else dict(no_pool=True)
    ctx, bg = context(tail), vcol_ref.case_background(tail)
    acc = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    whole = torch.zeros_like(acc)
    stream = torch.cuda.current_stream()
    for b, cnt in ((0, 3), (3, 4)):
        ctx.render_colors_device(vcol_ref.case_params(tail, spp_begin=b, spp_count=cnt, **kw), acc.data_ptr(), stream=stream.cuda_stream)
        if b == 0:
            stream.synchronize()
            head = acc.cpu().numpy().copy()
    full = vcol_ref.case_params(tail, spp_begin=0, spp_count=0, **kw)
    st = ctx.render_colors_device(full, whole.data_ptr(), stream=stream.cuda_stream, stats=True)
    dbg = torch.from_numpy(bg).cuda()
    dout = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
    ctx.resolve_device(w, h, full.spp, whole.data_ptr(), dbg.data_ptr(), dout.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    hout, host, hst = ctx.render_colors(full, bg=bg)
    assert_frames_equal(whole.cpu().numpy(), host, "device form against host form")
    assert_frames_equal(dout.cpu().numpy(), hout, "rt_resolve_device against the host form's image")
    assert (st.rays_closest, st.rays_shadow, st.samples) == (hst.rays_closest, hst.rays_shadow, hst.samples)
    assert_frames_equal(acc.cpu().numpy(), host, "[0, 3) then [3, 7)")
    assert head[..., 3].max() == 3 and (bits(head) != bits(host)).any()
    _, alone, _ = ctx.render_colors(vcol_ref.case_params(tail, **kw))
    assert_frames_equal(alone, vcol_ref.case_reference(tail)["accum"], "[3, 7) alone")
    only, _, _ = ctx.render_colors(full, bg=bg, want_accum=False)
    assert_frames_equal(only, hout, "the image alone")


def test_q8_context_gives_the_same_bits():
    """An RT_NODES_Q8 context walks its resident 32-byte records: the same frame."""
    case = first(SMOOTH, 0, ("lowres", True))
    ctx = context(case, bvh_builder=pyrt.BVH_HOST, node_format=pyrt.NODES_Q8)
    assert ctx.bvh_info().node_format == pyrt.NODES_Q8
    ref = vcol_ref.case_reference(case)
    for no_pool in (False, True):
        _, acc, st = ctx.render_colors(vcol_ref.case_params(case, no_pool=no_pool))
        assert_frames_equal(acc, ref["accum"], "Q8 context")
        assert (st.rays_closest, st.rays_shadow) == (ref["closest"], ref["shadow"])


def test_two_colourings_with_frames_between_them_on_a_busy_non_blocking_stream():
    """colours A, a frame, colours B, a frame, on a non-blocking stream that is still busy: the first frame reads A — the
    array it replaces is freed only once the launches that read it have run — and the second B."""
    case = first(SMOOTH, 0, ("cubes", False))
    s, (w, h) = vcol_ref.case_scene(case), case[1:3]
    col_a, col_b = vcol_ref.case_colors(case), vcol_ref.albedo_colors(s)
    ctx = pyrt.Context(s)
    busy = Busy()
    acc_a = busy.out((h, w, 4), zeroed=True)
    acc_b = busy.out((h, w, 4), zeroed=True)
    ctx.set_vertex_colors(col_a)
    busy.start()
    ctx.render_colors_device(vcol_ref.case_params(case), acc_a.ptr, stream=busy.ptr)
    was_busy = busy.issued()
    ctx.set_vertex_colors(col_b)
    ctx.render_colors_device(vcol_ref.case_params(case), acc_b.ptr, stream=busy.ptr)
    got_a, got_b = busy.fetch(acc_a), busy.fetch(acc_b)
    busy.finish()
    _, plain, _ = ctx.render(vcol_ref.case_params(case))
    ctx.close()
    assert_frames_equal(got_a.numpy(), vcol_ref.case_reference(case)["accum"], "first colouring")
    assert_frames_equal(got_b.numpy(), plain, "second colouring (C1)")
    assert (bits(got_a.numpy()) != bits(got_b.numpy())).any()
    assert was_busy, "the delay ended before the first call was issued (%.3f ms)" % busy.issue_ms


def test_colours_stay_across_rt_update_and_rt_rebuild():
    """New vertex positions refit the tree, rt_rebuild builds it again: the colours are indexed by vertex id and stay."""
    case = first(SMOOTH, 0, ("cubes", True))
    s = vcol_ref.case_scene(case)
    a = s.arrays()
    pos = (a["pos"] * F32(1.03) + F32(0.01)).astype(F32)
    moved = pyrt.ArrayScene(pos, a["nrm"], a["tri"], a["tri_begin"], a["vtx_begin"], a["materials"], a["lights"], a["camera"])
    p = vcol_ref.case_params(case)
    exp = vcol_ref.frame(moved, p, vcol_ref.case_colors(case))
    ctx = pyrt.Context(s)
    try:
        ctx.set_vertex_colors(vcol_ref.case_colors(case))
        ctx.update(pos=pos)
        _, acc, st = ctx.render_colors(p)
        assert_frames_equal(acc, exp["accum"], "after rt_update")
        assert (st.rays_closest, st.rays_shadow) == (exp["closest"], exp["shadow"])
        ctx.rebuild()
        _, acc, st = ctx.render_colors(p)
        assert_frames_equal(acc, exp["accum"], "after rt_rebuild")
        assert (bits(exp["accum"]) != bits(vcol_ref.case_reference(case)["accum"])).any()
    finally:
        ctx.close()


def test_release_then_state_and_the_rejections_that_read_the_context():
    """A context without colours answers the render calls with RT_ERR_STATE and writes nothing; a vertex count that is not
    the context's is RT_ERR_INVALID; a NULL call releases the colours."""
    L = pyrt.amd()
    case = vcol_ref.CASES[0]
    w, h, p = case[1], case[2], vcol_ref.case_params(case)
    s = vcol_ref.case_scene(case)
    nv = len(s.arrays()["pos"])
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
            rcs = [L.rt_render_colors(ctx._h, C.byref(p), None, None, ptr(acc), None),
                   L.rt_render_colors_device(ctx._h, C.byref(p), C.c_void_p(d.data_ptr()), None, None),
                   L.rt_render_aov_colors(ctx._h, C.byref(p), C.byref(a))]
            torch.cuda.synchronize()
            return rcs, (acc == 3).all() and bool((d == 3).all()) and (alb == 3).all()

        rcs, untouched = frame_calls()
        assert rcs == [STATE] * 3 and untouched and b"rt_set_vertex_colors" in L.rt_last_error()
        for n in (nv - 1, nv + 1, 0):
            col = np.zeros((max(n, 1), 3), F32)
            assert L.rt_set_vertex_colors(ctx._h, ptr(col), n) == INVALID
            assert b"%d vertices" % n in L.rt_last_error() and b"of %d" % nv in L.rt_last_error(), L.rt_last_error()
        rcs, untouched = frame_calls()
        assert rcs == [STATE] * 3 and untouched
        ctx.set_vertex_colors(vcol_ref.case_colors(case))
        _, got, _ = ctx.render_colors(p)
        assert_frames_equal(got, vcol_ref.case_reference(case)["accum"], "after the rejected calls")
        ctx.set_vertex_colors(None)
        rcs, untouched = frame_calls()
        assert rcs == [STATE] * 3 and untouched
        ctx.set_vertex_colors(None)  # (releasing nothing is not an error)
    finally:
        ctx.close()


def test_context_untouched():
    """rt_set_vertex_colors and the coloured calls change nothing rt_render or rt_render_aov read."""
    case = vcol_ref.CASES[0]
    ctx = pyrt.Context(vcol_ref.case_scene(case))
    fp = pyrt.make_params(case[1], case[2], 4, seed=3)
    _, frame0, st0 = ctx.render(fp)
    aov0 = ctx.render_aov(fp, raw=True)
    info0 = ctx.bvh_info()
    ctx.set_vertex_colors(vcol_ref.case_colors(case))
    ctx.render_colors(vcol_ref.case_params(case))
    ctx.render_aov_colors(fp)
    _, frame1, st1 = ctx.render(fp)
    aov1 = ctx.render_aov(fp, raw=True)
    assert (ctx.bvh_info().pad, ctx.bvh_info().n_nodes) == (info0.pad, info0.n_nodes)
    ctx.close()
    assert (bits(frame0) == bits(frame1)).all()
    assert (st0.rays_closest, st0.rays_shadow) == (st1.rays_closest, st1.rays_shadow)
    for k in aov0:
        assert (bits(aov0[k]) == bits(aov1[k])).all(), k


@pytest.mark.parametrize("case", [c for c in vcol_ref.CASES if c[6] != ALBEDO][::2], ids=vcol_ref.case_id)
def test_aov_colors(case):
    """The albedo channel is the reference's first-hit sums of c; every other channel is rt_render_aov's bit for bit;
    the device form writes the same sums; the exhaustive loop the same."""
    import torch
    ctx, p = context(case), vcol_ref.case_params(case)
    ref = vcol_ref.case_reference(case)
    plain = ctx.render_aov(p, raw=True)
    for accel in (pyrt.ACCEL_BVH, pyrt.ACCEL_BRUTE):
        got = ctx.render_aov_colors(vcol_ref.case_params(case, accel=accel), raw=True)
        assert_frames_equal(got["albedo"], ref["albedo"], "albedo")
        for k in plain:
            if k != "albedo":
                assert (bits(got[k]) == bits(plain[k])).all(), k
    if case[6] == SMOOTH:
        assert (bits(got["albedo"]) != bits(plain["albedo"])).any()
    h, w = case[2], case[1]
    d = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
    ctx.render_aov_colors_device(p, dict(albedo=d.data_ptr()), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert_frames_equal(d.cpu().numpy(), ref["albedo"], "device form")
