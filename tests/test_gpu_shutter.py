"""rt_render_shutter: the frame under an open shutter while the camera moves, bit for bit against tests/shutter_ref.py —
the numpy generator and one oracle row per (pixel, sample) — on shutter_ref.CASES: accumulator, resolved image and ray
counts under all six schedules (reserved[0] in {1, 4, 64}, pool or no pool), and the change condition; then a still
shutter against rt_render on a context updated to the camera of that time (G2), a lens at rest against rt_render_lens
(G3), a camera that does not move, chained ranges, host against device form, the chained rt_render_rays_device calls the
header states the frame to be (G1), a Q8 context, a busy non-blocking stream, and the rejections that read the
context's camera."""
import ctypes as C

import numpy as np
import pytest

import lens_ref
import pyrt
import shutter_ref
from busystream import Busy

pytestmark = pytest.mark.gpu

INVALID = 1
LANES = (1, 4, 64)
F32 = np.float32
_ctx = {}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_frames_equal(got, exp, what=""):
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    diff = (bits(got) != bits(exp)).any(axis=-1)
    first = np.unravel_index(int(np.argmax(diff)), diff.shape)
    assert not diff.any(), "%s: %d of %d pixels differ, first (y, x) = %s: got %s, expected %s" % (
        what, int(diff.sum()), diff.size, first, got[first], exp[first])


@pytest.fixture(scope="module", autouse=True)
def contexts():
    yield
    for c in _ctx.values():
        c.close()
    _ctx.clear()


def context(c, **kw):
    """One context per scene, frame aspect and option set, shared by the cases (the call changes nothing in it)."""
    key = (c[0], c[1], c[2], c[3], tuple(sorted(kw.items())))
    if key not in _ctx:
        _ctx[key] = pyrt.Context(shutter_ref.case_scene(c), **kw)
    return _ctx[key]


def shutter_of(c, **kw):
    args = shutter_ref.case_shutter_args(c)
    args.update(kw)
    return pyrt.make_shutter(shutter_ref.case_cameras(c)[1], **args)


def samples_of(c):
    s0, s1 = lens_ref.sample_range(shutter_ref.case_params(c))
    return c[2] * c[3] * (s1 - s0)


def schedules(c):
    """(lanes per pixel, no_pool) of a case: all six; the exhaustive loop has no pool to switch off."""
    return [(l, n) for l in LANES for n in ((False,) if c[7] else (False, True))]


@pytest.mark.parametrize("case", shutter_ref.CASES, ids=shutter_ref.case_id)
def test_shutter_bit_exact(case):
    """Accumulator, resolved image and the counts of closest-hit and shadow rays, whatever the schedule; and the frame is
    neither the still frame at A nor the one at B."""
    ref, ctx, bg = shutter_ref.case_reference(case), context(case), shutter_ref.case_background(case)
    for lanes, no_pool in schedules(case):
        what = "%s lanes %d%s" % (shutter_ref.case_id(case), lanes, " no pool" if no_pool else "")
        out, acc, st = ctx.render_shutter(shutter_ref.case_params(case, lanes_per_pixel=lanes, no_pool=no_pool), shutter_of(case), bg=bg)
        assert_frames_equal(acc, ref["accum"], "accum " + what)
        assert_frames_equal(out, ref["out"], "out " + what)
        assert (st.rays_closest, st.rays_shadow) == (ref["closest"], ref["shadow"]), what
        assert st.samples == samples_of(case) and st.kernel_ms > 0, what
    for still in shutter_ref.case_stills(case):
        share = shutter_ref.changed_words(acc, still)
        assert share >= shutter_ref.case_threshold(case), "the moving camera changes only %.3f of the accumulator words" % share


STILL_CASES = [c for c in shutter_ref.CASES if c[10] is None and c[0] != "hires"][::2]


@pytest.mark.parametrize("case", STILL_CASES, ids=shutter_ref.case_id)
def test_a_still_shutter_is_rt_render_under_the_camera_of_that_time(case):
    """G2: open == close == s at aperture 0 is rt_render on a context whose camera rt_update set to C(s): accumulator,
    image and both ray counts, under every schedule."""
    A, B = shutter_ref.case_cameras(case)
    ctx, bg = context(case), shutter_ref.case_background(case)
    moved = pyrt.Context(shutter_ref.case_scene(case))
    try:
        for s in (0.0, 0.5, 1.0):
            moved.update(camera=shutter_ref.camera_at(A, B, s))
            eout, eacc, est = moved.render(shutter_ref.case_params(case), bg)
            for lanes, no_pool in schedules(case):
                what = "%s s %g lanes %d%s" % (shutter_ref.case_id(case), s, lanes, " no pool" if no_pool else "")
                out, acc, st = ctx.render_shutter(shutter_ref.case_params(case, lanes_per_pixel=lanes, no_pool=no_pool),
                                                  shutter_of(case, open=s, close=s), bg=bg)
                assert_frames_equal(acc, eacc, "accum " + what)
                assert_frames_equal(out, eout, "out " + what)
                assert (st.rays_closest, st.rays_shadow, st.samples) == (est.rays_closest, est.rays_shadow, est.samples), what
    finally:
        moved.close()


@pytest.mark.parametrize("case", [c for c in shutter_ref.CASES if c[10] is not None], ids=shutter_ref.case_id)
def test_a_lens_at_rest_is_rt_render_lens(case):
    """G3: open == close == 0 with an aperture is rt_render_lens with the same aperture and focus on the same context."""
    ctx, bg = context(case), shutter_ref.case_background(case)
    k = shutter_ref.case_shutter_args(case)
    eout, eacc, est = ctx.render_lens(shutter_ref.case_params(case), pyrt.make_lens(k["aperture"], k["focus_distance"]), bg=bg)
    for lanes, no_pool in schedules(case):
        what = "%s lanes %d%s" % (shutter_ref.case_id(case), lanes, " no pool" if no_pool else "")
        out, acc, st = ctx.render_shutter(shutter_ref.case_params(case, lanes_per_pixel=lanes, no_pool=no_pool),
                                          shutter_of(case, open=0.0, close=0.0), bg=bg)
        assert_frames_equal(acc, eacc, "accum " + what)
        assert_frames_equal(out, eout, "out " + what)
        assert (st.rays_closest, st.rays_shadow, st.samples) == (est.rays_closest, est.rays_shadow, est.samples), what


@pytest.mark.parametrize("case", shutter_ref.CASES[::3], ids=shutter_ref.case_id)
def test_a_camera_that_does_not_move_is_rt_render(case):
    """B == A at aperture 0: rt_render's frame whatever the exposure, under every schedule."""
    A, _ = shutter_ref.case_cameras(case)
    ctx, bg = context(case), shutter_ref.case_background(case)
    eout, eacc, est = ctx.render(shutter_ref.case_params(case), bg)
    for lanes, no_pool in schedules(case):
        what = "%s lanes %d%s" % (shutter_ref.case_id(case), lanes, " no pool" if no_pool else "")
        out, acc, st = ctx.render_shutter(shutter_ref.case_params(case, lanes_per_pixel=lanes, no_pool=no_pool),
                                          pyrt.make_shutter(A, *shutter_ref.EXPOSURES[case[9]]), bg=bg)
        assert_frames_equal(acc, eacc, "accum " + what)
        assert_frames_equal(out, eout, "out " + what)
        assert (st.rays_closest, st.rays_shadow, st.samples) == (est.rays_closest, est.rays_shadow, est.samples), what


def test_collect_stats_counts_nodes_and_triangles():
    case = shutter_ref.CASES[0]
    ref = shutter_ref.case_reference(case)
    for no_pool in (False, True):
        _, acc, st = context(case).render_shutter(shutter_ref.case_params(case, collect_stats=1, no_pool=no_pool), shutter_of(case))
        assert_frames_equal(acc, ref["accum"], "counted instance")
        assert (st.rays_closest, st.rays_shadow) == (ref["closest"], ref["shadow"])
        assert st.nodes_visited > st.rays_closest and st.tris_tested > 0
    brute = next(c for c in shutter_ref.CASES if c[7])
    _, acc, st = context(brute).render_shutter(shutter_ref.case_params(brute, collect_stats=1), shutter_of(brute))
    assert_frames_equal(acc, shutter_ref.case_reference(brute)["accum"], "counted exhaustive instance")
    assert st.tris_tested > 0


@pytest.mark.parametrize("with_lens", [False, True])
def test_sample_ranges_chain_and_host_equals_device(with_lens):
    """[0, 3) then [3, 7) into one device accumulator is [0, 7), which is the host form's frame; the tail alone is the
    [3, 7) case's own reference."""
    import torch
    tail = next(c for c in shutter_ref.CASES if c[4] is shutter_ref.SPP7_34 and not c[7])
    w, h = tail[2], tail[3]
    ctx = context(tail)
    sh = shutter_of(tail) if with_lens else shutter_of(tail, aperture=0.0)
    acc = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    whole = torch.zeros_like(acc)
    stream = torch.cuda.current_stream()
    for b, cnt in ((0, 3), (3, 4)):
        ctx.render_shutter_device(shutter_ref.case_params(tail, spp_begin=b, spp_count=cnt), sh, acc.data_ptr(), stream=stream.cuda_stream)
        if b == 0:
            stream.synchronize()
            head = acc.cpu().numpy().copy()
    st = ctx.render_shutter_device(shutter_ref.case_params(tail, spp_begin=0, spp_count=0), sh, whole.data_ptr(), stream=stream.cuda_stream, stats=True)
    stream.synchronize()
    _, host, hst = ctx.render_shutter(shutter_ref.case_params(tail, spp_begin=0, spp_count=0), sh)
    assert_frames_equal(whole.cpu().numpy(), host, "device form against host form")
    assert (st.rays_closest, st.rays_shadow, st.samples) == (hst.rays_closest, hst.rays_shadow, hst.samples)
    assert_frames_equal(acc.cpu().numpy(), host, "[0, 3) then [3, 7)")
    assert head[..., 3].max() == 3 and (bits(head) != bits(host)).any()
    if with_lens:
        _, alone, _ = ctx.render_shutter(shutter_ref.case_params(tail), sh)
        assert_frames_equal(alone, shutter_ref.case_reference(tail)["accum"], "[3, 7) alone")


def test_frame_equals_the_chained_render_rays_calls():
    """G1 on the library's own rows: sample i of every pixel is one rt_render_rays_device call over the rays (o, F - o)
    with stream_index = pix and the one-sample range i; the calls into one accumulator are the frame."""
    import torch
    case = next(c for c in shutter_ref.CASES if c[4] is shutter_ref.SPP7 and not c[7])
    w, h = case[2], case[3]
    p = shutter_ref.case_params(case)
    A, B = shutter_ref.case_cameras(case)
    k = shutter_ref.case_shutter_args(case)
    o, F = shutter_ref.shutter_rays(A, B, p, k["open"], k["close"], k["aperture"], k["focus_distance"])
    ctx = context(case)
    acc = torch.zeros((h * w, 4), dtype=torch.float32, device="cuda")
    idx = torch.arange(h * w, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream()
    keep = []
    s0, s1 = lens_ref.sample_range(p)
    for i in range(s0, s1):
        rays = np.zeros(h * w, pyrt.RAY_DTYPE)
        rays["origin"], rays["direction"] = o[:, :, i - s0].reshape(-1, 3), (F[:, :, i - s0] - o[:, :, i - s0]).astype(F32).reshape(-1, 3)
        keep.append(torch.from_numpy(rays.view(F32).reshape(-1, 6).copy()).cuda())
        ctx.render_rays_device(shutter_ref.case_params(case, spp_begin=i, spp_count=1), keep[-1].data_ptr(), h * w, acc.data_ptr(),
                               d_stream_index=idx.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    _, frame, _ = ctx.render_shutter(p, shutter_of(case))
    assert_frames_equal(frame, acc.cpu().numpy().reshape(h, w, 4), "rt_render_shutter against chained rt_render_rays_device calls")
    assert_frames_equal(frame, shutter_ref.case_reference(case)["accum"], "and both against the reference")


def test_q8_context_gives_the_same_bits():
    """An RT_NODES_Q8 context walks its resident 32-byte records: the same frame."""
    case = next(c for c in shutter_ref.CASES if c[0] == "hires")
    ctx = context(case, bvh_builder=pyrt.BVH_HOST, node_format=pyrt.NODES_Q8)
    assert ctx.bvh_info().node_format == pyrt.NODES_Q8
    ref = shutter_ref.case_reference(case)
    for no_pool in (False, True):
        _, acc, st = ctx.render_shutter(shutter_ref.case_params(case, no_pool=no_pool), shutter_of(case))
        assert_frames_equal(acc, ref["accum"], "Q8 context")
        assert (st.rays_closest, st.rays_shadow) == (ref["closest"], ref["shadow"])


def test_on_a_busy_non_blocking_stream():
    """One call on a non-blocking stream that is still busy returns without waiting; the accumulator, zeroed behind the
    delay, holds the reference's bits once the stream has run."""
    case = shutter_ref.CASES[0]
    ref = shutter_ref.case_reference(case)
    ctx = pyrt.Context(shutter_ref.case_scene(case))
    b = Busy()
    acc = b.out((case[3], case[2], 4), zeroed=True)
    b.start()
    ctx.render_shutter_device(shutter_ref.case_params(case), shutter_of(case), acc.ptr, stream=b.ptr)
    busy = b.issued()
    got = b.fetch(acc)
    b.finish()
    ctx.close()
    assert_frames_equal(got.numpy(), ref["accum"], "busy stream")
    assert busy, "the delay ended before the call was issued (%.3f ms)" % b.issue_ms


def test_context_untouched():
    case = shutter_ref.CASES[0]
    ctx = pyrt.Context(shutter_ref.case_scene(case))
    fp = pyrt.make_params(case[2], case[3], 4, seed=3)
    _, frame0, _ = ctx.render(fp)
    info0 = ctx.bvh_info()
    ctx.render_shutter(shutter_ref.case_params(case), shutter_of(case))
    _, frame1, _ = ctx.render(fp)
    assert (ctx.bvh_info().pad, ctx.bvh_info().n_nodes) == (info0.pad, info0.n_nodes)
    ctx.close()
    assert (bits(frame0) == bits(frame1)).all()


def test_rejections_that_read_the_camera():
    """The origin bound (one float above the larger end of the move, plus 2 aperture, against 16 x the padding
    reference), an axis that turns by 90 degrees or more or cannot be normalised, and an fs1 that is not a finite positive
    float are RT_ERR_INVALID and write nothing."""
    L = pyrt.amd()
    case = shutter_ref.CASES[4]
    w, h = case[2], case[3]
    s = shutter_ref.case_scene(case)
    p = shutter_ref.case_params(case)
    acc = np.full((h, w, 4), 3.0, F32)
    ctx = context(case)

    def call(sh):
        return L.rt_render_shutter(ctx._h, C.byref(p), C.byref(sh), None, None, acc.ctypes.data_as(C.c_void_p), None)

    a = s.arrays()
    A = np.asarray(a["camera"], F32).reshape(4, 3)
    ref = max(1.0, float(np.abs(a["pos"][a["tri"].reshape(-1)]).max()), float(np.abs(A[0]).max()), float(np.abs(a["lights"][:, :3]).max()))
    bound = 16.0 * ref
    # the far end of the move beyond the bound, in either direction and even where the exposure never reaches it; just
    # inside, the move renders
    far = A.copy()
    far[0, 0] = bound * 1.01
    assert call(pyrt.make_shutter(far)) == INVALID and b"origin bound" in L.rt_last_error(), L.rt_last_error()
    far[0, 0] = -bound * 1.01
    assert call(pyrt.make_shutter(far, 0.0, 0.0)) == INVALID and b"origin bound" in L.rt_last_error(), L.rt_last_error()
    near = shutter_ref.translated(A, shutter_ref.SMALL)
    room = (bound - float(np.abs(near[0]).max())) / 2
    assert call(pyrt.make_shutter(near, 0.0, 1.0, room * 1.01, 1.0)) == INVALID and b"origin bound" in L.rt_last_error()
    assert (acc == 3).all()
    far[0, 0] = -bound * 0.98
    assert call(pyrt.make_shutter(far)) == pyrt.RT_OK, L.rt_last_error()
    assert call(pyrt.make_shutter(near, 0.0, 1.0, room * 0.98, 1.0)) == pyrt.RT_OK, L.rt_last_error()
    acc[:] = 3.0
    # axes: H turned past a right angle (by 91 degrees: the rounded rotation of exactly 90 may land on either side) and
    # by 180 degrees, a V turned upside down, a null V at the close
    quarter, back, flip, flat = (shutter_ref.turned(A, 91.0), shutter_ref.turned(A, 180.0), A.copy(), A.copy())
    flip[3] = -A[3]
    flat[3] = 0
    for B, word in ((quarter, b"90 degrees"), (back, b"90 degrees"), (flip, b"90 degrees"), (flat, b"normalised")):
        for ap in (0.0, 0.1):
            assert call(pyrt.make_shutter(B, 0.0, 1.0, ap, 1.0)) == INVALID and word in L.rt_last_error(), L.rt_last_error()
    assert (acc == 3).all()
    assert call(pyrt.make_shutter(shutter_ref.turned(A, 80.0))) == pyrt.RT_OK, L.rt_last_error()
    acc[:] = 3.0

    def scaled(f):  # the image plane f times as far away, the same view
        c = A.copy()
        c[1] = A[0] + (A[1] - A[0]) * F32(f)
        c[2], c[3] = A[2] * F32(f), A[3] * F32(f)
        return c

    # (fs0 is a finite positive float in both; the close's plane 1e-15 away and a focus distance of 1e25: fs1 overflows;
    # 1e15 away and a denormal focus distance: fs1 is 0, not positive)
    for B, focus in ((scaled(1e-15), 1e25), (scaled(1e15), 1e-44)):
        assert call(pyrt.make_shutter(A, 0.0, 1.0, 0.1, focus)) == pyrt.RT_OK, L.rt_last_error()
        acc[:] = 3.0
        assert call(pyrt.make_shutter(B, 0.0, 1.0, 0.1, focus)) == INVALID and b"focus_distance" in L.rt_last_error(), L.rt_last_error()
        assert (acc == 3).all()
        assert call(pyrt.make_shutter(B, 0.0, 1.0, 0.0, focus)) == pyrt.RT_OK, L.rt_last_error()
        acc[:] = 3.0
