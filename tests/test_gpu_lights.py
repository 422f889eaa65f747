"""rt_render_lights: the frame split by light group, bit for bit against tests/lights_ref.py — the oracle's frame of the
scene with the other lights' colours zeroed — on lights_ref.CASES: every slice's accumulator and resolved image and both
ray counts, which are ONE frame's whatever the number of groups (L3), under six schedules (default, no pool, 1 and 64
lanes per pixel, the counted instances, the exhaustive loop) and two crossings of them; then L1 against a second context after rt_update, L2
against rt_render, chained ranges, host against device form, a Q8 context, two calls with different tables back to back
on a busy non-blocking stream, and the rejection that reads the context's lights."""
import ctypes as C

import numpy as np
import pytest

import lights_ref
import pyrt
from busystream import Busy

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = 1, 4
F32 = np.float32
_ctx = {}

# (name, params keywords, the reference over the oracle's exhaustive loop)
SCHEDULES = [("default", dict(), False), ("no pool", dict(no_pool=True), False), ("1 lane", dict(lanes_per_pixel=1), False),
             ("64 lanes", dict(lanes_per_pixel=64), False), ("counted", dict(collect_stats=1), False),
             ("counted, no pool", dict(collect_stats=1, no_pool=True), False),
             ("exhaustive", dict(accel=pyrt.ACCEL_BRUTE), True), ("exhaustive, counted, 4 lanes", dict(accel=pyrt.ACCEL_BRUTE, collect_stats=1, lanes_per_pixel=4), True)]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_frames_equal(got, exp, what=""):
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    diff = (bits(got) != bits(exp)).any(axis=-1)
    first = np.unravel_index(int(np.argmax(diff)), diff.shape)
    assert not diff.any(), "%s: %d of %d pixels differ, first (slice, y, x) = %s: got %s, expected %s" % (
        what, int(diff.sum()), diff.size, first, got[first], exp[first])


@pytest.fixture(scope="module", autouse=True)
def contexts():
    yield
    for c in _ctx.values():
        c.close()
    _ctx.clear()


def context(c, **kw):
    """One context per scene, frame aspect and option set, shared by the cases (the call changes nothing in it)."""
    key = (c[0], c[1], c[2], tuple(sorted(kw.items())))
    if key not in _ctx:
        _ctx[key] = pyrt.Context(lights_ref.case_scene(c), **kw)
    return _ctx[key]


def samples_of(c):
    p = lights_ref.case_params(c)
    return c[1] * c[2] * (p.spp_count if p.spp_count else p.spp)


@pytest.mark.parametrize("case", lights_ref.CASES, ids=lights_ref.case_id)
def test_lights_bit_exact(case):
    """Every slice's accumulator and resolved image, and one frame's samples and ray counts, whatever the schedule."""
    ctx, bg, masks = context(case), lights_ref.case_background(case), lights_ref.case_masks(case)
    for name, kw, brute in SCHEDULES:
        ref = lights_ref.case_reference(case, brute)
        what = "%s, %s" % (lights_ref.case_id(case), name)
        out, acc, st = ctx.render_lights(lights_ref.case_params(case, **kw), masks, bg=bg)
        assert_frames_equal(acc, ref["accum"], "accum " + what)
        assert_frames_equal(out, ref["out"], "out " + what)
        assert (st.rays_closest, st.rays_shadow) == (ref["closest"], ref["shadow"]), what
        assert st.samples == samples_of(case) and st.kernel_ms > 0, what
        if kw.get("collect_stats"):
            assert st.tris_tested > 0 and (brute or st.nodes_visited > st.rays_closest), what


L1_CASES = [c for c in lights_ref.CASES if c[0][0] != "sweep" or c[0][2] != 1][::2]


@pytest.mark.parametrize("case", L1_CASES, ids=lights_ref.case_id)
def test_a_slice_is_rt_render_after_rt_update_zeroed_the_other_lights(case):
    """L1 on the library's own frames: a second context whose lights outside masks[g] rt_update gave the colour (0, 0, 0)
    renders slice g with rt_render_device — accumulator and both ray counts."""
    import torch
    ctx, s, masks = context(case), lights_ref.case_scene(case), lights_ref.case_masks(case)
    w, h, p = case[1], case[2], lights_ref.case_params(case)
    _, acc, st = ctx.render_lights(p, masks)
    other = pyrt.Context(s)
    try:
        for g, m in enumerate(masks):
            other.update(lights=lights_ref.lights_only(s, m))
            d = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
            est = other.render_device(p, d.data_ptr(), stats=True)
            assert_frames_equal(acc[g], d.cpu().numpy(), "slice %d (mask %s)" % (g, bin(m)))
            assert (st.rays_closest, st.rays_shadow, st.samples) == (est.rays_closest, est.rays_shadow, est.samples)
    finally:
        other.close()


@pytest.mark.parametrize("case", lights_ref.CASES[::3], ids=lights_ref.case_id)
def test_the_mask_of_all_lights_is_rt_render(case):
    """L2: one group of all lights is rt_render's frame — accumulator, image, samples and both ray counts — under every
    schedule; and the same mask as one of several groups is that frame too."""
    ctx, bg = context(case), lights_ref.case_background(case)
    full = lights_ref.all_mask(lights_ref.case_scene(case))
    for name, kw, _ in SCHEDULES:
        p = lights_ref.case_params(case, **kw)
        eout, eacc, est = ctx.render(p, bg)
        out, acc, st = ctx.render_lights(p, [full], bg=bg)
        assert_frames_equal(acc[0], eacc, "accum " + name)
        assert_frames_equal(out[0], eout, "out " + name)
        assert (st.rays_closest, st.rays_shadow, st.samples) == (est.rays_closest, est.rays_shadow, est.samples), name
        _, acc, st = ctx.render_lights(p, [0, full, 1, full])
        assert_frames_equal(acc[1], eacc, "slice 1 of four, " + name)
        assert_frames_equal(acc[3], eacc, "slice 3 of four, " + name)
        assert (bits(acc[0][..., :3]) == 0).all() and (bits(acc[0][..., 3]) == bits(eacc[..., 3])).all()
        assert (st.rays_closest, st.rays_shadow, st.samples) == (est.rays_closest, est.rays_shadow, est.samples), name


def test_the_same_masks_in_two_orders_give_the_same_slices_permuted():
    a, b = lights_ref.CASES[0], lights_ref.CASES[1]
    ctx = context(a)
    _, fa, sa = ctx.render_lights(lights_ref.case_params(a), a[6])
    _, fb, sb = ctx.render_lights(lights_ref.case_params(b), b[6])
    for j, m in enumerate(b[6]):
        assert_frames_equal(fb[j], fa[a[6].index(m)], "mask %s" % bin(m))
    assert (bits(fa[0]) != bits(fa[1])).any() and (bits(fa[1]) != bits(fa[2])).any()
    assert (sa.rays_closest, sa.rays_shadow) == (sb.rays_closest, sb.rays_shadow)


@pytest.mark.parametrize("pooled", [True, False])
def test_sample_ranges_chain_and_host_equals_device(pooled):
    """[0, 3) then [3, 7) into one device accumulator is [0, 7) in every slice, which is the host form's frame; the tail
    alone is the [3, 7) case's own reference; each slice resolves with rt_resolve_device to the host form's image."""
    import torch
    tail = next(c for c in lights_ref.CASES if c[3] is lights_ref.SPP7_34 and (lights_ref.n_lights(lights_ref.case_scene(c)) <= 3) == pooled)
    w, h, masks = tail[1], tail[2], lights_ref.case_masks(tail)
    G = len(masks)
    ctx, bg = context(tail), lights_ref.case_background(tail)
    acc = torch.zeros((G, h, w, 4), dtype=torch.float32, device="cuda")
    whole = torch.zeros_like(acc)
    stream = torch.cuda.current_stream()
    for b, cnt in ((0, 3), (3, 4)):
        ctx.render_lights_device(lights_ref.case_params(tail, spp_begin=b, spp_count=cnt), masks, acc.data_ptr(), stream=stream.cuda_stream)
        if b == 0:
            stream.synchronize()
            head = acc.cpu().numpy().copy()
    full = lights_ref.case_params(tail, spp_begin=0, spp_count=0)
    st = ctx.render_lights_device(full, masks, whole.data_ptr(), stream=stream.cuda_stream, stats=True)
    dbg = torch.from_numpy(bg).cuda()
    dout = torch.zeros((G, h, w, 3), dtype=torch.float32, device="cuda")
    for g in range(G):
        ctx.resolve_device(w, h, full.spp, whole[g].data_ptr(), dbg.data_ptr(), dout[g].data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    hout, host, hst = ctx.render_lights(full, masks, bg=bg)
    assert_frames_equal(whole.cpu().numpy(), host, "device form against host form")
    assert_frames_equal(dout.cpu().numpy(), hout, "rt_resolve_device per slice against the host form's image")
    assert (st.rays_closest, st.rays_shadow, st.samples) == (hst.rays_closest, hst.rays_shadow, hst.samples)
    assert_frames_equal(acc.cpu().numpy(), host, "[0, 3) then [3, 7)")
    assert head[..., 3].max() == 3 and (bits(head) != bits(host)).any()
    _, alone, _ = ctx.render_lights(lights_ref.case_params(tail), masks)
    assert_frames_equal(alone, lights_ref.case_reference(tail)["accum"], "[3, 7) alone")
    only, _, _ = ctx.render_lights(full, masks, bg=bg, want_accum=False)
    assert_frames_equal(only, hout, "the image alone")


def test_q8_context_gives_the_same_bits():
    """An RT_NODES_Q8 context walks its resident 32-byte records: the same slices."""
    case = next(c for c in lights_ref.CASES if c[0] == ("lowres", True))
    ctx = context(case, bvh_builder=pyrt.BVH_HOST, node_format=pyrt.NODES_Q8)
    assert ctx.bvh_info().node_format == pyrt.NODES_Q8
    ref = lights_ref.case_reference(case)
    for no_pool in (False, True):
        _, acc, st = ctx.render_lights(lights_ref.case_params(case, no_pool=no_pool), lights_ref.case_masks(case))
        assert_frames_equal(acc, ref["accum"], "Q8 context")
        assert (st.rays_closest, st.rays_shadow) == (ref["closest"], ref["shadow"])


def test_two_tables_back_to_back_on_a_busy_non_blocking_stream():
    """Two calls with different group tables on a non-blocking stream that is still busy return without waiting: each
    table was copied before its call returned, and the accumulators, zeroed behind the delay, hold the references' bits
    once the stream has run."""
    a, b = lights_ref.CASES[0], lights_ref.CASES[1]
    ctx = pyrt.Context(lights_ref.case_scene(a))
    busy = Busy()
    acc_a = busy.out((len(a[6]), a[2], a[1], 4), zeroed=True)
    acc_b = busy.out((len(b[6]), b[2], b[1], 4), zeroed=True)
    busy.start()
    table = pyrt.make_light_groups(a[6])
    ctx.render_lights_device(lights_ref.case_params(a), table, acc_a.ptr, stream=busy.ptr)
    for j, m in enumerate(b[6]):  # (the caller's record is its own again)
        table.masks[j] = m
    ctx.render_lights_device(lights_ref.case_params(b), table, acc_b.ptr, stream=busy.ptr)
    was_busy = busy.issued()
    got_a, got_b = busy.fetch(acc_a), busy.fetch(acc_b)
    busy.finish()
    ctx.close()
    assert_frames_equal(got_a.numpy(), lights_ref.case_reference(a)["accum"], "first table")
    assert_frames_equal(got_b.numpy(), lights_ref.case_reference(b)["accum"], "second table")
    assert was_busy, "the delay ended before the calls were issued (%.3f ms)" % busy.issue_ms


def test_context_untouched():
    case = lights_ref.CASES[0]
    ctx = pyrt.Context(lights_ref.case_scene(case))
    fp = pyrt.make_params(case[1], case[2], 4, seed=3)
    _, frame0, _ = ctx.render(fp)
    info0 = ctx.bvh_info()
    ctx.render_lights(lights_ref.case_params(case), lights_ref.case_masks(case))
    _, frame1, _ = ctx.render(fp)
    assert (ctx.bvh_info().pad, ctx.bvh_info().n_nodes) == (info0.pad, info0.n_nodes)
    ctx.close()
    assert (bits(frame0) == bits(frame1)).all()


def test_a_context_with_more_than_32_lights_is_unsupported():
    """A mask holds 32 lights: a context with 33 is RT_ERR_UNSUPPORTED whatever the masks say, and nothing is written;
    with 32 the top bit is a light like any other."""
    L = pyrt.amd()
    a = pyrt.Scene("cubes", 8, 8).arrays()
    p = pyrt.make_params(8, 8, 1, mode=pyrt.MODE_RAY, max_depth=1, seed=lights_ref.SEED)
    for n, want in ((33, UNSUPPORTED), (32, pyrt.RT_OK)):
        lights = np.tile(np.asarray(a["lights"], F32).reshape(-1, 21), (11, 1))[:n]
        s = pyrt.ArrayScene(a["pos"], a["nrm"], a["tri"], a["tri_begin"], a["vtx_begin"], a["materials"], lights, a["camera"])
        ctx = pyrt.Context(s)
        try:
            acc = np.full((2, 8, 8, 4), 3.0, F32)
            g = pyrt.make_light_groups([1 << 31, 1])
            rc = L.rt_render_lights(ctx._h, C.byref(p), C.byref(g), None, None, acc.ctypes.data_as(C.c_void_p), None)
            assert rc == want, L.rt_last_error()
            if want == UNSUPPORTED:
                assert b"33 lights" in L.rt_last_error() and (acc == 3).all()
            else:
                _, full, _ = ctx.render(p)
                assert (bits(acc[..., 3]) == bits(np.stack([full[..., 3]] * 2))).all() and np.isfinite(acc).all()
                assert (bits(acc[0]) != bits(acc[1])).any()
        finally:
            ctx.close()


def test_a_mask_beyond_the_contexts_lights_is_refused_and_named():
    """A mask bit at or above n_lights is RT_ERR_INVALID, names the group and the mask, and writes nothing; the same
    table is valid on a context that has the light."""
    L = pyrt.amd()
    three = next(c for c in lights_ref.CASES if c[0] == ("cubes", False))
    four = next(c for c in lights_ref.CASES if c[0] == ("sweep", "cubes", 3))
    w, h = three[1], three[2]
    p = lights_ref.case_params(three)
    acc = np.full((4, h, w, 4), 3.0, F32)
    out = np.full((4, h, w, 3), 3.0, F32)
    bg = lights_ref.case_background(three)

    def call(ctx, masks, params=p):
        g = pyrt.make_light_groups(masks)
        return L.rt_render_lights(ctx._h, C.byref(params), C.byref(g), bg.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p),
                                  acc.ctypes.data_as(C.c_void_p), None)

    ctx = context(three)
    for masks, group, word in (([0b1000], 0, b"0x8"), ([0b001, 0b111, 0b1001], 2, b"0x9"), ([7, 7, 7, 1 << 31], 3, b"0x80000000"),
                               ([0xffffffff, 1], 0, b"0xffffffff")):
        assert call(ctx, masks) == INVALID, masks
        err = L.rt_last_error()
        assert b"group %d" % group in err and word in err and b"n_lights 3" in err, err
    assert (acc == 3).all() and (out == 3).all()
    assert call(ctx, [0b111, 0b100]) == pyrt.RT_OK, L.rt_last_error()
    acc[:], out[:] = 3.0, 3.0
    ctx4 = context(four)  # (a smaller frame: the buffers are large enough)
    assert four[1] <= w and four[2] <= h
    assert call(ctx4, [0b1000, 0b1001], lights_ref.case_params(four)) == pyrt.RT_OK, L.rt_last_error()
    assert call(ctx4, [0b10000], lights_ref.case_params(four)) == INVALID and b"n_lights 4" in L.rt_last_error()
