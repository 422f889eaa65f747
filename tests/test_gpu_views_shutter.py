"""rt_render_views_shutter: many views of one scene, each under its own open shutter, in one launch — bit for bit against
tests/views_shutter_ref.py (the numpy generator of rt_render_shutter and one oracle row per pixel and sample, per view) on
accumulator, image and ray counts under six schedules; then the header's guarantees on the library itself: V1 against
rt_render_shutter_device on a second context after rt_update(camera), V2 against rt_render_views, V4 against
rt_render_shutter, chained ranges and host against device form, permuted records, the padding a far camera_close needs, Q8
contexts, the per-view rejections that read the cameras, and two calls back to back on a busy non-blocking stream."""
import ctypes as C

import numpy as np
import pytest
import torch

import pyrt
import shutter_ref
import views_shutter_ref as vs
from busystream import Busy

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = 1, 4
F32 = np.float32
_ctx = {}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_frames_equal(got, exp, what=""):
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    diff = (bits(got) != bits(exp)).any(axis=-1)
    first = np.unravel_index(int(np.argmax(diff)), diff.shape)
    assert not diff.any(), "%s: %d of %d pixels differ, first %s: got %s, expected %s" % (
        what, int(diff.sum()), diff.size, first, got[first], exp[first])


@pytest.fixture(scope="module", autouse=True)
def contexts():
    yield
    for c in _ctx.values():
        c.close()
    _ctx.clear()


def context(c, **kw):
    """One context per scene, frame aspect and option set, shared by the cases (the cases need no refit)."""
    key = (c[0], c[1], c[2], c[3], tuple(sorted(kw.items())))
    if key not in _ctx:
        _ctx[key] = pyrt.Context(vs.case_scene(c), **kw)
    return _ctx[key]


def with_seed(p, seed):
    q = pyrt.Params.from_buffer_copy(p)
    q.seed = int(seed)
    return q


def per_view_shutter_frames(ref, p, cams, shutters, seeds):
    """V1's right-hand side: rt_render_shutter_device on `ref` after a camera-only rt_update to each camera, with the view's
    seed and record: (accumulators [n][h][w][4], summed (closest, shadow) counts)."""
    accs, rays = [], [0, 0]
    stream = torch.cuda.current_stream()
    for j, cam in enumerate(cams):
        ref.update(camera=cam)
        acc = torch.zeros((p.height, p.width, 4), dtype=torch.float32, device="cuda")
        st = ref.render_shutter_device(p if seeds is None else with_seed(p, seeds[j]), shutters[j], acc.data_ptr(),
                                       stream=stream.cuda_stream, stats=True)
        stream.synchronize()
        accs.append(acc.cpu().numpy())
        rays = [rays[0] + st.rays_closest, rays[1] + st.rays_shadow]
    return np.stack(accs), rays


# ---- the CPU expectation under six schedules ---------------------------------------------------------------------------
def schedules(c):
    """(name, params keywords, brute) of a case: default, no pool, one and 64 lanes per pixel, the counted instances, and
    the exhaustive loop.  A brute case runs all of them on the exhaustive loop, which has no pool to switch off; a BVH
    case takes the loop as its sixth schedule where the table gives it a brute expectation of its own (BRUTE_TOO)."""
    out = [("default", dict(), None), ("lanes 1", dict(lanes_per_pixel=1), None), ("lanes 64", dict(lanes_per_pixel=64), None),
           ("counted", dict(collect_stats=1), None)]
    if not c[7]:
        out.append(("no pool", dict(no_pool=True), None))
        if c in BRUTE_TOO:
            out.append(("brute", dict(accel=pyrt.ACCEL_BRUTE), True))
    return out


BRUTE_TOO = [c for c in vs.CASES if not c[7]][:2]


@pytest.mark.parametrize("case", vs.CASES, ids=vs.case_id)
def test_views_shutter_bit_exact(case):
    ctx, bg = context(case), vs.case_background(case)
    cams, shutters, seeds = vs.case_cameras(case), vs.case_shutters(case), vs.case_seeds(case)
    for name, kw, brute in schedules(case):
        ref = vs.case_reference(case, brute)
        what = "%s %s" % (vs.case_id(case), name)
        out, acc, st = ctx.render_views_shutter(vs.case_params(case, **kw), cams, shutters, bg=bg, seeds=seeds)
        for j in range(vs.N_VIEWS):
            assert_frames_equal(acc[j], ref["accum"][j], "accum view %d (%s) %s" % (j, case[8][j], what))
            assert_frames_equal(out[j], ref["out"][j], "out view %d (%s) %s" % (j, case[8][j], what))
        assert (st.rays_closest, st.rays_shadow) == (ref["closest"], ref["shadow"]), what
        assert st.samples == vs.samples_of(case) and st.kernel_ms > 0, what
        if kw.get("collect_stats"):
            assert st.tris_tested > 0 and (case[7] or st.nodes_visited > st.rays_closest), what


# ---- V1, V2, V4 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", vs.CASES, ids=vs.case_id)
def test_v1_slices_are_rt_render_shutter_device_after_an_update(case):
    ctx = context(case)
    cams, shutters, seeds = vs.case_cameras(case), vs.case_shutters(case), vs.case_seeds(case)
    other = pyrt.Context(vs.case_scene(case))
    try:
        for kw in (dict(), dict(no_pool=True), dict(lanes_per_pixel=1)):
            p = vs.case_params(case, **kw)
            _, acc, st = ctx.render_views_shutter(p, cams, shutters, seeds=seeds)
            eacc, rays = per_view_shutter_frames(other, p, cams, shutters, seeds)
            for j in range(vs.N_VIEWS):
                assert_frames_equal(acc[j], eacc[j], "view %d %s %s" % (j, vs.case_id(case), kw))
            assert [st.rays_closest, st.rays_shadow] == rays
    finally:
        other.close()


@pytest.mark.parametrize("case", vs.CASES[::2], ids=vs.case_id)
def test_v2_no_optics_is_rt_render_views(case):
    ctx, bg = context(case), vs.case_background(case)
    cams, seeds = vs.case_cameras(case), vs.case_seeds(case)
    none = [vs.shutter_of(vs.record("none", cam)) for cam in cams]
    for kw in (dict(), dict(no_pool=True), dict(lanes_per_pixel=64), dict(collect_stats=1)):
        p = vs.case_params(case, **kw)
        eout, eacc, est = ctx.render_views(p, cams, bg, seeds=seeds)
        out, acc, st = ctx.render_views_shutter(p, cams, none, bg=bg, seeds=seeds)
        assert_frames_equal(acc, eacc, "accum %s %s" % (vs.case_id(case), kw))
        assert_frames_equal(out, eout, "out %s %s" % (vs.case_id(case), kw))
        assert (st.rays_closest, st.rays_shadow, st.samples) == (est.rays_closest, est.rays_shadow, est.samples)


@pytest.mark.parametrize("case", vs.CASES[1::2], ids=vs.case_id)
def test_v4_one_view_at_the_contexts_camera_is_rt_render_shutter(case):
    ctx, bg = context(case), vs.case_background(case)
    cam = vs.case_cameras(case)[0]  # (the scene's own camera, which the shared context still has)
    for kind in ("move_lens", "turn", "lens", "none"):
        sh = vs.shutter_of(vs.record(kind, cam, case[9], case[10]))
        for kw in (dict(), dict(no_pool=True)):
            p = vs.case_params(case, **kw)
            eout, eacc, est = ctx.render_shutter(p, sh, bg=bg)
            out, acc, st = ctx.render_views_shutter(p, cam[None], [sh], bg=bg)
            assert_frames_equal(acc[0], eacc, "accum %s %s %s" % (vs.case_id(case), kind, kw))
            assert_frames_equal(out[0], eout, "out %s %s %s" % (vs.case_id(case), kind, kw))
            assert (st.rays_closest, st.rays_shadow, st.samples) == (est.rays_closest, est.rays_shadow, est.samples)


# ---- forms and ranges ----------------------------------------------------------------------------------------------------
def test_sample_ranges_chain_and_host_equals_device():
    """[0, 3) then [3, 7) into one device accumulator is [0, 7), which is the host form's frame; the images are
    rt_resolve_device of the slices."""
    case = next(c for c in vs.CASES if c[4] is vs.SPP7_34)
    w, h, n = case[2], case[3], vs.N_VIEWS
    ctx, bg = context(case), vs.case_background(case)
    cams, shutters, seeds = vs.case_cameras(case), vs.case_shutters(case), vs.case_seeds(case)
    whole_p = vs.case_params(case, spp_begin=0, spp_count=0)
    hout, hacc, hst = ctx.render_views_shutter(whole_p, cams, shutters, bg=bg, seeds=seeds)
    stream = torch.cuda.current_stream()
    acc = torch.zeros((n, h, w, 4), dtype=torch.float32, device="cuda")
    whole = torch.zeros_like(acc)
    for b, cnt in ((0, 3), (3, 4)):
        ctx.render_views_shutter_device(vs.case_params(case, spp_begin=b, spp_count=cnt), cams, shutters, acc.data_ptr(),
                                        stream=stream.cuda_stream, seeds=seeds)
    st = ctx.render_views_shutter_device(whole_p, cams, shutters, whole.data_ptr(), stream=stream.cuda_stream, seeds=seeds, stats=True)
    stream.synchronize()
    assert_frames_equal(whole.cpu().numpy(), hacc, "device form against host form")
    assert (st.rays_closest, st.rays_shadow, st.samples) == (hst.rays_closest, hst.rays_shadow, hst.samples)
    assert_frames_equal(acc.cpu().numpy(), hacc, "[0, 3) then [3, 7)")
    d_bg = torch.from_numpy(bg).cuda()
    d_out = torch.empty((n, h, w, 3), dtype=torch.float32, device="cuda")
    for j in range(n):
        ctx.resolve_device(w, h, 7, acc[j].data_ptr(), d_bg.data_ptr(), d_out[j].data_ptr())
    torch.cuda.synchronize()
    assert_frames_equal(d_out.cpu().numpy(), hout, "rt_resolve_device of the slices")
    # the tail alone is the case's own reference
    _, tail, _ = ctx.render_views_shutter(vs.case_params(case), cams, shutters, seeds=seeds)
    assert_frames_equal(tail, vs.case_reference(case)["accum"], "[3, 7) alone")


def test_permuted_records_give_the_permuted_slices():
    """Five views, all four kinds among them, then the same views in another order: slice k of the second call is slice
    perm[k] of the first.  An index taken from the tile and not from the view, or a record read from another view's row,
    would break it."""
    case = vs.CASES[0]
    ctx = context(case)
    cams = vs.orbit(vs.case_scene(case).arrays()["camera"], (0.0, 14.0, -18.0, 30.0, -9.0), (1.0, 0.9, 1.15, 1.05, 0.95))
    kinds = ("none", "lens", "move_lens", "turn", "move_lens")
    recs = [vs.shutter_of(vs.record(k, cam, (j % 2, 0), shutter_ref.LARGE if j == 4 else shutter_ref.SMALL))
            for j, (k, cam) in enumerate(zip(kinds, cams))]
    seeds = [3, 1, 4, 1, 5]
    p = vs.case_params(case)
    _, acc, st = ctx.render_views_shutter(p, cams, recs, seeds=seeds)
    for a in range(5):
        for b in range(a + 1, 5):
            assert (bits(acc[a]) != bits(acc[b])).mean() > 0.25, "views %d and %d hardly differ" % (a, b)
    perm = [3, 0, 4, 2, 1]
    _, acc2, st2 = ctx.render_views_shutter(p, cams[perm], [recs[k] for k in perm], seeds=[seeds[k] for k in perm])
    for k in range(5):
        assert_frames_equal(acc2[k], acc[perm[k]], "slice %d of the permuted call" % k)
    assert (st2.rays_closest, st2.rays_shadow) == (st.rays_closest, st.rays_shadow)
    # and the unpermuted call equals the per-view frames of a second context (V1 over five views)
    other = pyrt.Context(vs.case_scene(case))
    try:
        eacc, rays = per_view_shutter_frames(other, p, cams, recs, seeds)
    finally:
        other.close()
    assert_frames_equal(acc, eacc, "five views against rt_render_shutter_device per view")
    assert [st.rays_closest, st.rays_shadow] == rays


# ---- the camera rule -------------------------------------------------------------------------------------------------------
def far_close(a, cam):
    """cam moved along x until its position lies at twice the padding reference of the scene: beyond what the context's
    padding covers, well inside its origin bound (16 times the reference)."""
    far = F32(2) * vs.pad_reference(a)
    return shutter_ref.translated(cam, (far - cam[0, 0], 0.0, 0.0))


def test_a_far_camera_close_refits_and_the_frames_still_match():
    case = vs.CASES[0]
    s = vs.case_scene(case)
    a = s.arrays()
    ctx, other = pyrt.Context(s), pyrt.Context(s)
    try:
        cams, seeds = vs.case_cameras(case), [5, 6, 7]
        pad0 = ctx.bvh_info().pad
        assert pad0 == F32(6e-5) * vs.pad_reference(a, cams[:1])
        recs = [vs.record(k, cam) for k, cam in zip(("none", "turn", "move_lens"), cams)]
        recs[2]["camera_close"] = far_close(a, cams[2])
        assert np.abs(recs[2]["camera_close"][0]).max() > max(np.abs(c[0]).max() for c in cams)
        shutters = [vs.shutter_of(r) for r in recs]
        p = vs.case_params(case)
        _, before, _ = ctx.render(p)
        _, acc, st = ctx.render_views_shutter(p, cams, shutters, seeds=seeds)
        assert ctx.bvh_info().pad == F32(6e-5) * vs.pad_reference(a, [recs[2]["camera_close"]]) > pad0
        eacc, rays = per_view_shutter_frames(other, p, cams, shutters, seeds)
        assert other.bvh_info().pad == pad0  # (rt_render_shutter never refits; the frames do not depend on the padding)
        assert_frames_equal(acc, eacc, "after the refit")
        assert [st.rays_closest, st.rays_shadow] == rays
        _, after, _ = ctx.render(p)
        assert_frames_equal(after, before, "the context's own camera did not move")
    finally:
        ctx.close(), other.close()


def test_q8_context_renders_covered_views_and_refuses_a_refit():
    case = next(c for c in vs.CASES if c[0] == "lowres" and not c[7])
    s = vs.case_scene(case)
    q8 = pyrt.Context(s, node_format=pyrt.NODES_Q8)
    try:
        assert q8.bvh_info().node_format == pyrt.NODES_Q8
        cams, shutters, seeds = vs.case_cameras(case), vs.case_shutters(case), vs.case_seeds(case)
        ref = vs.case_reference(case)
        for no_pool in (False, True):
            _, acc, st = q8.render_views_shutter(vs.case_params(case, no_pool=no_pool), cams, shutters, seeds=seeds)
            assert_frames_equal(acc, ref["accum"], "Q8 context")
            assert (st.rays_closest, st.rays_shadow) == (ref["closest"], ref["shadow"])
        far = vs.record("none", cams[1])
        far["camera_close"], far["close"] = far_close(s.arrays(), cams[1]), 1.0
        got = np.full((vs.N_VIEWS, case[3], case[2], 4), 3.0, F32)
        v, _keep = pyrt.make_views(cams)
        p = vs.case_params(case)
        sh = pyrt.make_shutters([shutters[0], vs.shutter_of(far), shutters[2]], vs.N_VIEWS)
        rc = pyrt.amd().rt_render_views_shutter(q8._h, C.byref(p), C.byref(v), sh, None, None, got.ctypes.data_as(C.c_void_p), None)
        assert rc == UNSUPPORTED and b"Q8" in pyrt.amd().rt_last_error() and (got == 3).all()
    finally:
        q8.close()


def test_rejections_that_read_the_cameras_name_the_view():
    """The origin bound, the axis rule and the fs rule fire per view, with cameras[j] in the place of the context's camera,
    at the first and at the last view alone; a rejected call writes nothing and leaves the padding alone."""
    L = pyrt.amd()
    case = vs.CASES[0]
    w, h, n = case[2], case[3], vs.N_VIEWS
    s = vs.case_scene(case)
    ctx = pyrt.Context(s)
    try:
        cams, good = vs.case_cameras(case), vs.case_shutters(case)
        p = vs.case_params(case)
        acc = np.full((n, h, w, 4), 3.0, F32)
        v, _keep = pyrt.make_views(cams)
        pad0 = ctx.bvh_info().pad

        def call(j, bad):
            sh = pyrt.make_shutters([bad if k == j else good[k] for k in range(n)], n)
            return L.rt_render_views_shutter(ctx._h, C.byref(p), C.byref(v), sh, None, None, acc.ctypes.data_as(C.c_void_p), None)

        def scaled(A, f):  # the image plane f times as far away, the same view
            c = A.copy()
            c[1] = A[0] + (A[1] - A[0]) * F32(f)
            c[2], c[3] = A[2] * F32(f), A[3] * F32(f)
            return c

        closes = [r["camera_close"] for r in vs.case_records(case)]
        for j in (0, n - 1):
            A = cams[j]
            who = b"view %d: " % j
            near = shutter_ref.translated(A, shutter_ref.SMALL)
            # (the bound the frame would run under: 16 times the padding reference over every end camera of the call)
            bound = 16.0 * float(vs.pad_reference(s.arrays(), list(cams) + closes + [near]))
            room = (bound - float(np.abs(near[0]).max())) / 2
            pad0 = ctx.bvh_info().pad
            flip, flat = A.copy(), A.copy()
            flip[3], flat[3] = -A[3], 0
            bad = [(pyrt.make_shutter(near, 0.0, 1.0, room * 1.01, 1.0), b"origin bound"),
                   (pyrt.make_shutter(shutter_ref.turned(A, 91.0)), b"90 degrees"),
                   (pyrt.make_shutter(shutter_ref.turned(A, 180.0), 0.0, 1.0, 0.1, 1.0), b"90 degrees"),
                   (pyrt.make_shutter(flip), b"90 degrees"), (pyrt.make_shutter(flat), b"normalised"),
                   (pyrt.make_shutter(scaled(A, 1e-15), 0.0, 1.0, 0.1, 1e25), b"focus_distance"),
                   (pyrt.make_shutter(scaled(A, 1e15), 0.0, 1.0, 0.1, 1e-44), b"focus_distance")]
            for rec, word in bad:
                rc = call(j, rec)
                msg = L.rt_last_error()
                assert rc == INVALID and word in msg and who in msg, (j, word, msg)
            assert (acc == 3).all() and ctx.bvh_info().pad == pad0
            # just inside the rules the same views render
            for rec in (pyrt.make_shutter(near, 0.0, 1.0, room * 0.98, 1.0), pyrt.make_shutter(shutter_ref.turned(A, 80.0)),
                        pyrt.make_shutter(scaled(A, 1e-15), 0.0, 1.0, 0.0, 1e25)):
                assert call(j, rec) == pyrt.RT_OK, L.rt_last_error()
                acc[:] = 3.0
        # the view camera itself: an axis of cameras[j] that cannot be normalised is the same rejection
        flatcams = cams.copy()
        flatcams[n - 1, 2] = 0
        vf, _k = pyrt.make_views(flatcams)
        sh = pyrt.make_shutters(good, n)
        rc = L.rt_render_views_shutter(ctx._h, C.byref(p), C.byref(vf), sh, None, None, acc.ctypes.data_as(C.c_void_p), None)
        assert rc == INVALID and b"view %d: " % (n - 1) in L.rt_last_error() and (acc == 3).all()
    finally:
        ctx.close()


# ---- stream order ----------------------------------------------------------------------------------------------------------
def test_two_calls_back_to_back_on_a_busy_non_blocking_stream():
    """Two calls with different records on a non-blocking stream that is still busy return without waiting — each takes a
    slot of the ring of pinned view and shutter records — and the accumulators, zeroed behind the delay, hold the frames
    the host form gives for the same arguments."""
    case = vs.CASES[0]
    n, h, w = vs.N_VIEWS, case[3], case[2]
    cams, first, seeds = vs.case_cameras(case), vs.case_shutters(case), vs.case_seeds(case)
    second = [vs.shutter_of(vs.record(k, cam, (1, 1), shutter_ref.LARGE)) for k, cam in zip(("turn", "move_lens", "lens"), cams)]
    p = vs.case_params(case)
    ctx = pyrt.Context(vs.case_scene(case))
    try:
        for _ in range(4):  # (every slot of the ring has its pinned copies before the stream is busy)
            _, exp2, _ = ctx.render_views_shutter(p, cams, second, seeds=seeds[::-1])
        b = Busy()
        acc1, acc2 = b.out((n, h, w, 4), zeroed=True), b.out((n, h, w, 4), zeroed=True)
        b.start()
        ctx.render_views_shutter_device(p, cams, first, acc1.ptr, stream=b.ptr, seeds=seeds)
        ctx.render_views_shutter_device(p, cams, second, acc2.ptr, stream=b.ptr, seeds=seeds[::-1])
        busy = b.issued()
        got1, got2 = b.fetch(acc1), b.fetch(acc2)
        b.finish()
    finally:
        ctx.close()
    assert_frames_equal(got1.numpy(), vs.case_reference(case)["accum"], "first call on the busy stream")
    assert_frames_equal(got2.numpy(), exp2, "second call on the busy stream")
    assert (bits(got1.numpy()) != bits(got2.numpy())).mean() > 0.25
    assert busy, "the delay ended before the calls were issued (%.3f ms)" % b.issue_ms
