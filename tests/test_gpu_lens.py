"""rt_render_lens: the frame through a thin lens, bit for bit against tests/lens_ref.py — the numpy generator and one
oracle row per (pixel, sample) — on lens_ref.CASES: accumulator, resolved image and ray counts under all six schedules
(reserved[0] in {1, 4, 64}, pool or no pool); then aperture 0 against rt_render, chained ranges, host against device form,
the chained rt_render_rays_device calls the header states the frame to be, a Q8 context, a busy non-blocking stream, and
the rejections that read the context's camera."""
import ctypes as C

import numpy as np
import pytest

import lens_ref
import pyrt
from busystream import Busy

pytestmark = pytest.mark.gpu

INVALID = 1
LANES = (1, 4, 64)
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
        _ctx[key] = pyrt.Context(lens_ref.case_scene(c), **kw)
    return _ctx[key]


def lens_of(c):
    return pyrt.make_lens(*lens_ref.case_lens(c))


def samples_of(c):
    s0, s1 = lens_ref.sample_range(lens_ref.case_params(c))
    return c[2] * c[3] * (s1 - s0)


def schedules(c):
    """(lanes per pixel, no_pool) of a case: all six; the exhaustive loop has no pool to switch off."""
    return [(l, n) for l in LANES for n in ((False,) if c[7] else (False, True))]


@pytest.mark.parametrize("case", lens_ref.CASES, ids=lens_ref.case_id)
def test_lens_bit_exact(case):
    """Accumulator, resolved image and the counts of closest-hit and shadow rays, whatever the schedule; and the frame is
    not the pinhole's."""
    ref, ctx, bg = lens_ref.case_reference(case), context(case), lens_ref.case_background(case)
    for lanes, no_pool in schedules(case):
        what = "%s lanes %d%s" % (lens_ref.case_id(case), lanes, " no pool" if no_pool else "")
        out, acc, st = ctx.render_lens(lens_ref.case_params(case, lanes_per_pixel=lanes, no_pool=no_pool), lens_of(case), bg=bg)
        assert_frames_equal(acc, ref["accum"], "accum " + what)
        assert_frames_equal(out, ref["out"], "out " + what)
        assert (st.rays_closest, st.rays_shadow) == (ref["closest"], ref["shadow"]), what
        assert st.samples == samples_of(case) and st.kernel_ms > 0, what
    _, pin, _ = ctx.render(lens_ref.case_params(case))
    assert lens_ref.changed_words(acc, pin) >= 0.5, "the lens changes less than half of the accumulator words"


@pytest.mark.parametrize("case", lens_ref.CASES, ids=lens_ref.case_id)
def test_aperture_zero_is_rt_render(case):
    """aperture == 0: accum, out and the ray counts of rt_render for the same params, bit for bit, under every schedule —
    and with a focus distance that would be refused at any other aperture."""
    ctx, bg = context(case), lens_ref.case_background(case)
    eout, eacc, est = ctx.render(lens_ref.case_params(case), bg)
    pin, pst = lens_ref.pinhole_reference(case)
    assert_frames_equal(eacc, pin, "rt_render against the oracle " + lens_ref.case_id(case))
    for lanes, no_pool in schedules(case):
        what = "%s lanes %d%s" % (lens_ref.case_id(case), lanes, " no pool" if no_pool else "")
        out, acc, st = ctx.render_lens(lens_ref.case_params(case, lanes_per_pixel=lanes, no_pool=no_pool), pyrt.make_lens(0.0, -1.0), bg=bg)
        assert_frames_equal(acc, eacc, "accum " + what)
        assert_frames_equal(out, eout, "out " + what)
        assert (st.rays_closest, st.rays_shadow, st.samples) == (est.rays_closest, est.rays_shadow, est.samples), what
        assert (st.rays_closest, st.rays_shadow) == (pst.rays_closest, pst.rays_shadow), what


def test_collect_stats_counts_nodes_and_triangles():
    case = lens_ref.CASES[0]
    ref = lens_ref.case_reference(case)
    for no_pool in (False, True):
        _, acc, st = context(case).render_lens(lens_ref.case_params(case, collect_stats=1, no_pool=no_pool), lens_of(case))
        assert_frames_equal(acc, ref["accum"], "counted instance")
        assert (st.rays_closest, st.rays_shadow) == (ref["closest"], ref["shadow"])
        assert st.nodes_visited > st.rays_closest and st.tris_tested > 0
    brute = next(c for c in lens_ref.CASES if c[7])
    _, acc, st = context(brute).render_lens(lens_ref.case_params(brute, collect_stats=1), lens_of(brute))
    assert_frames_equal(acc, lens_ref.case_reference(brute)["accum"], "counted exhaustive instance")
    assert st.tris_tested > 0


@pytest.mark.parametrize("aperture", [0.0, lens_ref.APERTURES[1]])
def test_sample_ranges_chain_and_host_equals_device(aperture):
    """[0, 3) then [3, 7) into one device accumulator is [0, 7), which is the host form's frame; the tail alone is the
    [3, 7) case's own reference."""
    import torch
    tail = next(c for c in lens_ref.CASES if c[4] is lens_ref.SPP7_34 and not c[7] and c[:2] == ("cubes", False))
    w, h = tail[2], tail[3]
    ctx, lens = context(tail), pyrt.make_lens(aperture, lens_ref.case_lens(tail)[1])
    acc = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    whole = torch.zeros_like(acc)
    stream = torch.cuda.current_stream()
    for b, cnt in ((0, 3), (3, 4)):
        ctx.render_lens_device(lens_ref.case_params(tail, spp_begin=b, spp_count=cnt), lens, acc.data_ptr(), stream=stream.cuda_stream)
        if b == 0:
            stream.synchronize()
            head = acc.cpu().numpy().copy()
    st = ctx.render_lens_device(lens_ref.case_params(tail, spp_begin=0, spp_count=0), lens, whole.data_ptr(), stream=stream.cuda_stream, stats=True)
    stream.synchronize()
    _, host, hst = ctx.render_lens(lens_ref.case_params(tail, spp_begin=0, spp_count=0), lens)
    assert_frames_equal(whole.cpu().numpy(), host, "device form against host form")
    assert (st.rays_closest, st.rays_shadow, st.samples) == (hst.rays_closest, hst.rays_shadow, hst.samples)
    assert_frames_equal(acc.cpu().numpy(), host, "[0, 3) then [3, 7)")
    assert head[..., 3].max() == 3 and (bits(head) != bits(host)).any()
    if aperture == lens_ref.case_lens(tail)[0]:
        _, alone, _ = ctx.render_lens(lens_ref.case_params(tail), lens)
        assert_frames_equal(alone, lens_ref.case_reference(tail)["accum"], "[3, 7) alone")


def test_frame_equals_the_chained_render_rays_calls():
    """The stated equivalence on the device itself: sample i of every pixel is one rt_render_rays_device call over the
    rays (o', F - o') with stream_index = pix and the one-sample range i; seven calls into one accumulator are the frame."""
    import torch
    case = next(c for c in lens_ref.CASES if c[4] is lens_ref.SPP7 and not c[7])
    w, h = case[2], case[3]
    p = lens_ref.case_params(case)
    o, F = lens_ref.lens_rays(lens_ref.case_scene(case).arrays()["camera"], p, *lens_ref.case_lens(case))
    ctx = context(case)
    acc = torch.zeros((h * w, 4), dtype=torch.float32, device="cuda")
    idx = torch.arange(h * w, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream()
    keep = []
    for i in range(7):
        rays = np.zeros(h * w, pyrt.RAY_DTYPE)
        rays["origin"], rays["direction"] = o[:, :, i].reshape(-1, 3), (F[:, :, i] - o[:, :, i]).astype(np.float32).reshape(-1, 3)
        keep.append(torch.from_numpy(rays.view(np.float32).reshape(-1, 6).copy()).cuda())
        ctx.render_rays_device(lens_ref.case_params(case, spp_begin=i, spp_count=1), keep[-1].data_ptr(), h * w, acc.data_ptr(),
                               d_stream_index=idx.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    _, frame, _ = ctx.render_lens(p, lens_of(case))
    assert_frames_equal(frame, acc.cpu().numpy().reshape(h, w, 4), "rt_render_lens against seven rt_render_rays_device calls")
    assert_frames_equal(frame, lens_ref.case_reference(case)["accum"], "and both against the reference")


def test_q8_context_gives_the_same_bits():
    """An RT_NODES_Q8 context walks its resident 32-byte records: the same frame."""
    case = next(c for c in lens_ref.CASES if c[0] == "hires")
    ctx = context(case, bvh_builder=pyrt.BVH_HOST, node_format=pyrt.NODES_Q8)
    assert ctx.bvh_info().node_format == pyrt.NODES_Q8
    ref = lens_ref.case_reference(case)
    for no_pool in (False, True):
        _, acc, st = ctx.render_lens(lens_ref.case_params(case, no_pool=no_pool), lens_of(case))
        assert_frames_equal(acc, ref["accum"], "Q8 context")
        assert (st.rays_closest, st.rays_shadow) == (ref["closest"], ref["shadow"])


def test_on_a_busy_non_blocking_stream():
    """One call on a non-blocking stream that is still busy returns without waiting; the accumulator, zeroed behind the
    delay, holds the reference's bits once the stream has run."""
    case = lens_ref.CASES[0]
    ref = lens_ref.case_reference(case)
    ctx = pyrt.Context(lens_ref.case_scene(case))
    b = Busy()
    acc = b.out((case[3], case[2], 4), zeroed=True)
    b.start()
    ctx.render_lens_device(lens_ref.case_params(case), lens_of(case), acc.ptr, stream=b.ptr)
    busy = b.issued()
    got = b.fetch(acc)
    b.finish()
    ctx.close()
    assert_frames_equal(got.numpy(), ref["accum"], "busy stream")
    assert busy, "the delay ended before the call was issued (%.3f ms)" % b.issue_ms


def test_context_untouched():
    case = lens_ref.CASES[0]
    ctx = pyrt.Context(lens_ref.case_scene(case))
    fp = pyrt.make_params(case[2], case[3], 4, seed=3)
    _, frame0, _ = ctx.render(fp)
    info0 = ctx.bvh_info()
    ctx.render_lens(lens_ref.case_params(case), lens_of(case))
    _, frame1, _ = ctx.render(fp)
    assert (ctx.bvh_info().pad, ctx.bvh_info().n_nodes) == (info0.pad, info0.n_nodes)
    ctx.close()
    assert (bits(frame0) == bits(frame1)).all()


def _with_camera(s, cam):
    a = s.arrays()
    return pyrt.ArrayScene(a["pos"], a["nrm"], a["tri"], a["tri_begin"], a["vtx_begin"], a["materials"], a["lights"],
                           np.asarray(cam, np.float32).reshape(4, 3))


def test_rejections_that_read_the_camera():
    """The origin bound (max |pos| + 2 aperture against 16 x the padding reference) and the fs rule — a null H or V, an fs
    that overflows or underflows float32 — are RT_ERR_INVALID with aperture > 0 and write nothing; at aperture 0 the same
    contexts render."""
    L = pyrt.amd()
    case = lens_ref.CASES[4]
    w, h = case[2], case[3]
    s = lens_ref.case_scene(case)
    p = lens_ref.case_params(case)
    acc = np.full((h, w, 4), 3.0, np.float32)

    def call(ctx, lens):
        return L.rt_render_lens(ctx._h, C.byref(p), C.byref(lens), None, None, acc.ctypes.data_as(C.c_void_p), None)

    ctx = context(case)
    a = s.arrays()
    ref = max(1.0, float(np.abs(a["pos"][a["tri"].reshape(-1)]).max()), float(np.abs(a["camera"][0]).max()),
              float(np.abs(a["lights"][:, :3]).max()))
    bound = 16.0 * ref
    room = (bound - float(np.abs(a["camera"][0]).max())) / 2
    assert call(ctx, pyrt.make_lens(room * 1.01, 1.0)) == INVALID and b"origin bound" in L.rt_last_error()
    assert call(ctx, pyrt.make_lens(1e30, 1.0)) == INVALID and b"origin bound" in L.rt_last_error()
    assert (acc == 3).all()
    assert call(ctx, pyrt.make_lens(room * 0.99, 1.0)) == pyrt.RT_OK, L.rt_last_error()  # (just inside: it renders)
    acc[:] = 3.0
    cam = np.asarray(a["camera"], np.float32).reshape(4, 3).copy()

    def scaled(f):  # the image plane f times as far away, the same view
        c = cam.copy()
        c[1] = cam[0] + (cam[1] - cam[0]) * np.float32(f)
        c[2], c[3] = cam[2] * np.float32(f), cam[3] * np.float32(f)
        return c

    flat = cam.copy()
    flat[2] = 0  # a null horizontal axis
    # (the plane 1e-15 away and a focus distance of 1e25: fs overflows; 1e15 away and 1e-44: fs underflows to 0)
    for bad, lens, word in ((flat, pyrt.make_lens(0.1, 1.0), b"normalised"), (scaled(1e-15), pyrt.make_lens(0.1, 1e25), b"focus_distance"),
                            (scaled(1e15), pyrt.make_lens(0.1, 1e-44), b"focus_distance")):
        c2 = pyrt.Context(_with_camera(s, bad))
        assert call(c2, lens) == INVALID and word in L.rt_last_error(), L.rt_last_error()
        assert (acc == 3).all()
        assert call(c2, pyrt.make_lens(0.0, 1.0)) == pyrt.RT_OK, L.rt_last_error()
        acc[:] = 3.0
        c2.close()
