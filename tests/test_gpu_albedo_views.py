"""rt_render_views_shutter_albedo and rt_render_aov_views_albedo, bit for bit: the mixed cases of
tests/albedo_views_ref.py — the oracle's rays, hits, BSDF and light evaluation under the sampled albedo, for the primary
rays of shutter_ref's generator — on accumulator, resolved image, samples and both ray counts under the eight schedules of
test_gpu_lights.SCHEDULES; then the guarantees of include/rt_amd.h on the library's own frames: X1 against single-view
calls, X2 against rt_render_textured_device / rt_render_colors_device, X3 against rt_render_views_shutter in all three
ways, X4 against rt_render_views_shutter of the per-triangle scene, X5's chained ranges and a Q8 context (the exhaustive
loop is among the schedules); host against device form and the images against rt_resolve_device of each slice; two calls
with different texture sets on a busy non-blocking stream; the set kept across rt_update and rt_rebuild; RT_ERR_STATE
after the release, the accumulator untouched; the change floors of the reference module; and the AOV form slice by
slice."""
import ctypes as C

import numpy as np
import pytest

import albedo_views_ref as avr
import pyrt
import tex_ref
import vcol_ref
from albedo_views_ref import COL, COLORS, MATERIAL, TEX, TEXTURES
from busystream import Busy
from test_gpu_lights import SCHEDULES, assert_frames_equal, bits
from tex_ref import T_ALBEDO, T_FACES, T_MIXED, T_NONE

pytestmark = pytest.mark.gpu

INVALID, STATE = 1, 5
F32 = np.float32
_ctx = {}
EXACT = [c for c in avr.CASES if c[6][1] in (T_ALBEDO, T_NONE, vcol_ref.ALBEDO)]
PER_FACE = [c for c in avr.CASES if c[6][1] in (T_FACES, vcol_ref.FACES)]


@pytest.fixture(scope="module", autouse=True)
def contexts():
    yield
    for c in _ctx.values():
        c.close()
    _ctx.clear()


def context(c, **kw):
    """One context per case and option set, with the case's surface resident."""
    key = (avr.case_id(c), tuple(sorted(kw.items())))
    if key not in _ctx:
        _ctx[key] = pyrt.Context(avr.case_scene(c), **kw)
        avr.set_surface(_ctx[key], c)
    return _ctx[key]


def call(ctx, c, albedo=None, views=None, still=False, bg=True, **kw):
    """The host form on a case: (out, accum, stats).  views: the indices of the views to render (all)."""
    j = list(range(avr.n_views(c))) if views is None else list(views)
    cams, sh, seeds = avr.case_cameras(c)[j], avr.case_shutters(c, still), avr.case_seeds(c)
    return ctx.render_views_shutter_albedo(avr.case_params(c, **kw), cams, [sh[k] for k in j],
                                           albedo=avr.albedo_of_case(c) if albedo is None else albedo,
                                           bg=avr.case_background(c) if bg else None, seeds=None if seeds is None else [seeds[k] for k in j])


def plain(ctx, c, **kw):
    """rt_render_views_shutter on a case."""
    return ctx.render_views_shutter(avr.case_params(c, **kw), avr.case_cameras(c), avr.case_shutters(c), bg=avr.case_background(c),
                                    seeds=avr.case_seeds(c))


def check(got, ref, what):
    out, acc, st = got
    assert_frames_equal(acc, ref["accum"], "accum " + what)
    assert_frames_equal(out, ref["out"], "out " + what)
    assert (st.rays_closest, st.rays_shadow) == (ref["closest"], ref["shadow"]), what


def as_ref(frame):
    out, acc, st = frame
    return dict(accum=acc, out=out, closest=st.rays_closest, shadow=st.rays_shadow)


@pytest.mark.parametrize("case", avr.MIXED, ids=avr.case_id)
def test_mixed_surfaces_bit_exact_under_every_schedule(case):
    ctx = context(case)
    for name, kw, brute in SCHEDULES:
        what = "%s, %s" % (avr.case_id(case), name)
        out, acc, st = call(ctx, case, **kw)
        check((out, acc, st), avr.case_reference(case, brute), what)
        assert st.samples == avr.samples_of(case) and st.kernel_ms > 0, what
        if kw.get("collect_stats"):
            assert st.tris_tested > 0 and (brute or st.nodes_visited > st.rays_closest), what


def test_the_surface_and_the_optics_show():
    """The frames the mixed cases compare are neither the untextured ones nor the still ones (the floors of
    albedo_views_ref, from the oracle alone); the hit counts are the generator's."""
    for case in avr.MIXED:
        ctx = context(case)
        _, acc, _ = call(ctx, case)
        _, untextured, _ = plain(ctx, case)
        _, still, _ = call(ctx, case, still=True)
        assert avr.changed_rgb_words(acc, untextured) > avr.MIN_CHANGED_SURFACE, avr.case_id(case)
        assert avr.changed_rgb_words(acc, still) > avr.MIN_CHANGED_OPTICS, avr.case_id(case)
        assert (bits(acc[..., 3]) == bits(untextured[..., 3])).all()


@pytest.mark.parametrize("case", [c for c in avr.CASES if avr.n_views(c) > 1][::2], ids=avr.case_id)
def test_x1_slices_are_single_view_calls(case):
    import torch
    ctx, bg = context(case), avr.case_background(case)
    w, h = case[1], case[2]
    for kw in (dict(), dict(no_pool=True)):
        out, acc, st = call(ctx, case, **kw)
        nc = ns = 0
        for j in range(avr.n_views(case)):
            o1, a1, s1 = call(ctx, case, views=[j], **kw)
            assert_frames_equal(acc[j], a1[0], "slice %d" % j)
            assert_frames_equal(out[j], o1[0], "image %d" % j)
            nc, ns = nc + s1.rays_closest, ns + s1.rays_shadow
            # ... and the image is rt_resolve_device of the slice
            d_acc, d_bg = torch.from_numpy(acc[j].copy()).cuda(), torch.from_numpy(bg).cuda()
            d_out = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
            ctx.resolve_device(w, h, avr.case_params(case).spp, d_acc.data_ptr(), d_bg.data_ptr(), d_out.data_ptr(),
                               stream=torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            assert_frames_equal(d_out.cpu().numpy(), out[j], "rt_resolve_device of slice %d" % j)
        assert (st.rays_closest, st.rays_shadow) == (nc, ns)
        if avr.n_views(case) > 1:
            assert (bits(acc[0]) != bits(acc[1])).any()


@pytest.mark.parametrize("case", avr.MIXED, ids=avr.case_id)
def test_x2_no_optics_is_the_single_view_form(case):
    """View 0 is the scene's own camera, which the shared context still has: under a record that changes nothing the call
    is rt_render_textured_device / rt_render_colors_device with the view's seed."""
    import torch
    ctx = context(case)
    w, h = case[1], case[2]
    stream = torch.cuda.current_stream().cuda_stream
    for name, kw, _ in SCHEDULES[:2] + SCHEDULES[4:5] + SCHEDULES[6:7]:
        out, acc, st = call(ctx, case, views=[0], still=True, **kw)
        p = avr.view_params(case, 0, **kw)
        d = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
        single = ctx.render_textured_device if case[6][0] == TEX else ctx.render_colors_device
        est = single(p, d.data_ptr(), stream=stream, stats=True)
        torch.cuda.synchronize()
        assert_frames_equal(acc[0], d.cpu().numpy(), "%s, %s" % (avr.case_id(case), name))
        assert (st.rays_closest, st.rays_shadow, st.samples) == (est.rays_closest, est.rays_shadow, est.samples), name


@pytest.mark.parametrize("case", avr.CASES[::3], ids=avr.case_id)
def test_x3_the_material_albedo_is_rt_render_views_shutter(case):
    """RT_ALBEDO_MATERIAL, whatever is resident — and on a context that holds neither colours nor textures."""
    ctx = context(case)
    bare = pyrt.Context(avr.case_scene(case))
    try:
        for name, kw, _ in SCHEDULES:
            exp = as_ref(plain(ctx, case, **kw))
            for c in (ctx, bare):
                got = call(c, case, albedo=MATERIAL, **kw)
                check(got, exp, "%s, %s" % (avr.case_id(case), name))
                assert got[2].samples == avr.samples_of(case)
    finally:
        bare.close()


@pytest.mark.parametrize("case", EXACT, ids=avr.case_id)
def test_x3_albedo_colours_and_albedo_texels_are_rt_render_views_shutter(case):
    ctx = context(case)
    for name, kw, _ in SCHEDULES:
        check(call(ctx, case, **kw), as_ref(plain(ctx, case, **kw)), "%s, %s" % (avr.case_id(case), name))


@pytest.mark.parametrize("case", PER_FACE, ids=avr.case_id)
def test_x4_per_face_data_is_rt_render_views_shutter_of_one_mesh_per_triangle(case):
    ctx = context(case)
    other = pyrt.Context(avr.case_triangle_scene(case))
    try:
        for name, kw, _ in SCHEDULES[:2] + SCHEDULES[4:7]:
            check(call(ctx, case, **kw), as_ref(plain(other, case, **kw)), "%s, %s" % (avr.case_id(case), name))
    finally:
        other.close()


@pytest.mark.parametrize("pooled", [True, False])
@pytest.mark.parametrize("surface", [TEX, COL])
def test_x5_sample_ranges_chain_and_host_equals_device(surface, pooled):
    """[0, 3) then [3, 7) into one device accumulator is [0, 7), which is the host form's frame; the tail alone is the
    [3, 7) case's own reference where the case has that range."""
    import torch
    case = next(c for c in avr.MIXED if c[6][0] == surface and c[3] in (avr.SPP7, avr.SPP7_34))
    w, h, n = case[1], case[2], avr.n_views(case)
    kw = dict() if pooled else dict(no_pool=True)
    ctx, bg = context(case), avr.case_background(case)
    cams, sh, seeds, alb = avr.case_cameras(case), avr.case_shutters(case), avr.case_seeds(case), avr.albedo_of_case(case)
    acc = torch.zeros((n, h, w, 4), dtype=torch.float32, device="cuda")
    whole = torch.zeros_like(acc)
    stream = torch.cuda.current_stream()
    for b, cnt in ((0, 3), (3, 4)):
        ctx.render_views_shutter_albedo_device(avr.case_params(case, spp_begin=b, spp_count=cnt, **kw), cams, sh, acc.data_ptr(),
                                               albedo=alb, stream=stream.cuda_stream, seeds=seeds)
        if b == 0:
            stream.synchronize()
            head = acc.cpu().numpy().copy()
    full = avr.case_params(case, spp_begin=0, spp_count=0, **kw)
    st = ctx.render_views_shutter_albedo_device(full, cams, sh, whole.data_ptr(), albedo=alb, stream=stream.cuda_stream, seeds=seeds,
                                                stats=True)
    stream.synchronize()
    hout, host, hst = ctx.render_views_shutter_albedo(full, cams, sh, albedo=alb, bg=bg, seeds=seeds)
    assert_frames_equal(whole.cpu().numpy(), host, "device form against host form")
    assert (st.rays_closest, st.rays_shadow, st.samples) == (hst.rays_closest, hst.rays_shadow, hst.samples)
    assert_frames_equal(acc.cpu().numpy(), host, "[0, 3) then [3, 7)")
    assert head[..., 3].max() <= 3 and (bits(head) != bits(host)).any()
    if case[3] is avr.SPP7_34:
        _, alone, _ = call(ctx, case, **kw)
        assert_frames_equal(alone, avr.case_reference(case)["accum"], "[3, 7) alone")
    only, none, _ = ctx.render_views_shutter_albedo(full, cams, sh, albedo=alb, bg=bg, seeds=seeds, want_accum=False)
    assert none is None
    assert_frames_equal(only, hout, "the image alone")


@pytest.mark.parametrize("case", [c for c in avr.MIXED if c[0] == ("lowres", False)], ids=avr.case_id)
def test_x5_a_q8_context_gives_the_same_bits(case):
    """An RT_NODES_Q8 context walks its resident 32-byte records: the frame of a default context."""
    ctx = context(case, bvh_builder=pyrt.BVH_HOST, node_format=pyrt.NODES_Q8)
    assert ctx.bvh_info().node_format == pyrt.NODES_Q8
    ref = avr.case_reference(case)
    for no_pool in (False, True):
        _, acc, st = call(ctx, case, no_pool=no_pool)
        assert_frames_equal(acc, ref["accum"], "Q8 context")
        assert (st.rays_closest, st.rays_shadow) == (ref["closest"], ref["shadow"])


def test_two_texture_sets_with_frames_between_them_on_a_busy_non_blocking_stream():
    """set A, a frame, set B, a frame, on a non-blocking stream that is still busy: the first frame reads A — the arrays
    it replaces are freed only once the launches that read them have run — and the second B; each call takes a slot of
    the ring of pinned view and shutter records."""
    case = avr.MIXED[0]
    assert case[6] == (TEX, T_MIXED)
    s, (w, h), n = avr.case_scene(case), case[1:3], avr.n_views(case)
    set_a, set_b = avr.case_surface(case), tex_ref.texture_set(s, T_ALBEDO)
    cams, sh, seeds = avr.case_cameras(case), avr.case_shutters(case), avr.case_seeds(case)
    ctx = pyrt.Context(s)
    busy = Busy()
    acc_a = busy.out((n, h, w, 4), zeroed=True)
    acc_b = busy.out((n, h, w, 4), zeroed=True)
    ctx.set_textures(*tex_ref.set_args(set_a))
    busy.start()
    ctx.render_views_shutter_albedo_device(avr.case_params(case), cams, sh, acc_a.ptr, albedo=TEXTURES, stream=busy.ptr, seeds=seeds)
    was_busy = busy.issued()
    ctx.set_textures(*tex_ref.set_args(set_b))
    ctx.render_views_shutter_albedo_device(avr.case_params(case), cams, sh, acc_b.ptr, albedo=TEXTURES, stream=busy.ptr, seeds=seeds)
    got_a, got_b = busy.fetch(acc_a), busy.fetch(acc_b)
    busy.finish()
    _, untextured, _ = plain(ctx, case)
    ctx.close()
    assert_frames_equal(got_a.numpy(), avr.case_reference(case)["accum"], "first set")
    assert_frames_equal(got_b.numpy(), untextured, "second set (X3)")
    assert (bits(got_a.numpy()) != bits(got_b.numpy())).any()
    assert was_busy, "the delay ended before the first call was issued (%.3f ms)" % busy.issue_ms


@pytest.mark.parametrize("surface", [TEX, COL])
def test_the_resident_data_stays_across_rt_update_and_rt_rebuild(surface):
    """New vertex positions refit the tree, rt_rebuild builds it again: uvs and colours are indexed by vertex id and stay."""
    case = next(c for c in avr.MIXED if c[6][0] == surface and c[3] is avr.SPP1)
    s = avr.case_scene(case)
    a = s.arrays()
    pos = (a["pos"] * F32(1.03) + F32(0.01)).astype(F32)
    moved = pyrt.ArrayScene(pos, a["nrm"], a["tri"], a["tri_begin"], a["vtx_begin"], a["materials"], a["lights"], a["camera"])
    exp = [avr.view_frame(moved, cam, rec, avr.view_params(case, j), avr.case_albedo_fn(case))
           for j, (cam, rec) in enumerate(zip(avr.case_cameras(case), avr.case_records(case)))]
    exp_acc = np.stack([v["accum"] for v in exp])
    ctx = pyrt.Context(s)
    try:
        avr.set_surface(ctx, case)
        ctx.update(pos=pos)
        _, acc, st = call(ctx, case)
        assert_frames_equal(acc, exp_acc, "after rt_update")
        assert (st.rays_closest, st.rays_shadow) == (sum(v["closest"] for v in exp), sum(v["shadow"] for v in exp))
        ctx.rebuild()
        _, acc, _ = call(ctx, case)
        assert_frames_equal(acc, exp_acc, "after rt_rebuild")
        assert (bits(exp_acc) != bits(avr.case_reference(case)["accum"])).any()
    finally:
        ctx.close()


def test_missing_data_is_a_state_error_and_writes_nothing():
    """A context without the data `albedo` names answers RT_ERR_STATE with the single-view forms' messages, after the
    release too, and neither the accumulator nor an AOV channel is touched; RT_ALBEDO_MATERIAL needs none."""
    import torch
    L = pyrt.amd()
    case = avr.MIXED[0]
    w, h, n, p = case[1], case[2], avr.n_views(case), avr.case_params(case)
    v, _keep = pyrt.make_views(avr.case_cameras(case), avr.case_seeds(case))
    sh = pyrt.make_shutters(avr.case_shutters(case), n)
    ptr = lambda x: x.ctypes.data_as(C.c_void_p)
    ctx = pyrt.Context(avr.case_scene(case))

    def calls(albedo):
        acc = np.full((n, h, w, 4), 3.0, F32)
        d = torch.full((n, h, w, 4), 3.0, dtype=torch.float32, device="cuda")
        alb = np.full((n, h, w, 3), 3.0, F32)
        a = pyrt.Aov()
        a.albedo = alb.ctypes.data
        da, dalb = pyrt.Aov(), torch.full((n, h, w, 3), 3.0, dtype=torch.float32, device="cuda")
        da.albedo = dalb.data_ptr()
        rcs, msgs = [], []
        for rc in (lambda: L.rt_render_views_shutter_albedo(ctx._h, C.byref(p), C.byref(v), sh, albedo, None, None, ptr(acc), None),
                   lambda: L.rt_render_views_shutter_albedo_device(ctx._h, C.byref(p), C.byref(v), sh, albedo, C.c_void_p(d.data_ptr()), None, None),
                   lambda: L.rt_render_aov_views_albedo(ctx._h, C.byref(p), C.byref(v), albedo, C.byref(a)),
                   lambda: L.rt_render_aov_views_albedo_device(ctx._h, C.byref(p), C.byref(v), albedo, C.byref(da), None)):
            rcs.append(rc())
            msgs.append(L.rt_last_error())
        torch.cuda.synchronize()
        return rcs, msgs, bool((acc == 3).all() and (d == 3).all() and (alb == 3).all() and (dalb == 3).all())

    try:
        for albedo, word in ((TEXTURES, b"rt_set_textures"), (COLORS, b"rt_set_vertex_colors")):
            rcs, msgs, untouched = calls(albedo)
            assert rcs == [STATE] * 4 and untouched and all(word in m for m in msgs), (rcs, msgs)
        rcs, _, untouched = calls(MATERIAL)
        assert rcs == [0] * 4 and not untouched
        rcs, _, _ = calls(3)
        assert rcs == [INVALID] * 4
        # each kind of data serves its own value only
        ctx.set_vertex_colors(vcol_ref.smooth_colors(avr.case_scene(case)))
        assert calls(TEXTURES)[0] == [STATE] * 4 and calls(COLORS)[0] == [0] * 4
        ctx.set_vertex_colors(None)
        avr.set_surface(ctx, case)
        assert calls(COLORS)[0] == [STATE] * 4
        _, got, _ = call(ctx, case)
        assert_frames_equal(got, avr.case_reference(case)["accum"], "after the rejected calls")
        ctx.set_textures(None)
        rcs, msgs, untouched = calls(TEXTURES)
        assert rcs == [STATE] * 4 and untouched and all(b"rt_set_textures" in m for m in msgs)
    finally:
        ctx.close()


@pytest.mark.parametrize("case", avr.MIXED[::2] + PER_FACE[:1], ids=avr.case_id)
def test_aov_views_albedo_slice_by_slice(case):
    """Slice j of every channel is the single-view coloured or textured AOV call on a context whose camera is cameras[j]
    (a camera-only rt_update), with seeds[j]; the albedo channel is also the reference's first-hit sums under the still
    records; RT_ALBEDO_MATERIAL is rt_render_aov_views; NULL channels are not written; the device form and the
    exhaustive loop give the same sums."""
    import torch
    ctx, p = context(case), avr.case_params(case)
    cams, seeds, alb = avr.case_cameras(case), avr.case_seeds(case), avr.albedo_of_case(case)
    n, w, h = avr.n_views(case), case[1], case[2]
    got = ctx.render_aov_views_albedo(p, cams, albedo=alb, seeds=seeds)
    other = pyrt.Context(avr.case_scene(case))
    try:
        avr.set_surface(other, case)
        for j in range(n):
            other.update(camera=cams[j])
            q = avr.view_params(case, j)
            exp = other.render_aov_textured(q, raw=True) if case[6][0] == TEX else other.render_aov_colors(q, raw=True)
            for k in exp:
                assert (bits(got[k][j]) == bits(exp[k])).all(), (k, j)
    finally:
        other.close()
    if case in avr.MIXED:
        assert_frames_equal(got["albedo"], avr.case_reference(case, still=True)["albedo"], "the reference's first-hit sums")
    mat = ctx.render_aov_views(p, cams, seeds=seeds)
    got_mat = ctx.render_aov_views_albedo(p, cams, albedo=MATERIAL, seeds=seeds)
    for k in mat:
        assert (bits(got_mat[k]) == bits(mat[k])).all(), k
        if k != "albedo":
            assert (bits(got[k]) == bits(mat[k])).all(), k
    assert (bits(got["albedo"]) != bits(mat["albedo"])).any()
    brute = ctx.render_aov_views_albedo(avr.case_params(case, accel=pyrt.ACCEL_BRUTE), cams, albedo=alb, seeds=seeds)
    for k in got:
        assert (bits(brute[k]) == bits(got[k])).all(), k
    # two channels only: the others are NULL and nothing else is written (the host form would stage them)
    some = ctx.render_aov_views_albedo(p, cams, albedo=alb, seeds=seeds, channels=("albedo", "hits"))
    assert set(some) == {"albedo", "hits"} and all((bits(some[k]) == bits(got[k])).all() for k in some)
    d = torch.full((n, h, w, 3), 3.0, dtype=torch.float32, device="cuda")
    dh = torch.full((n, h, w), 3, dtype=torch.int32, device="cuda")
    ctx.render_aov_views_albedo_device(p, cams, dict(albedo=d.data_ptr(), hits=dh.data_ptr()), albedo=alb,
                                       stream=torch.cuda.current_stream().cuda_stream, seeds=seeds)
    torch.cuda.synchronize()
    assert_frames_equal(d.cpu().numpy(), got["albedo"], "device form")
    assert (dh.cpu().numpy().view(np.uint32) == got["hits"]).all()
