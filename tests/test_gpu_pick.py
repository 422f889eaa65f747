"""rt_render_pick: sampled direct lighting, bit for bit against tests/pick_ref.py — per pixel and sample the oracle's
one-sample frame under that sample's tuple of scaled lights — on pick_ref.CASES: accumulator, resolved image and both ray
counts under the eight schedules of test_gpu_lights.SCHEDULES (P1); then P1 against second contexts given a tuple's
lights by rt_update, P2 against rt_render, P3 against rt_render with m arbitrary lights, chained ranges, host against
device form, a Q8 context (P4), two calls with different importance arrays back to back on a busy non-blocking stream,
the untouched context, and the rejections that read the context's lights."""
import ctypes as C

import numpy as np
import pytest

import pick_ref
import pyrt
from busystream import Busy
from test_gpu_lights import SCHEDULES, assert_frames_equal, bits

pytestmark = pytest.mark.gpu

INVALID = 1
F32 = np.float32
_ctx = {}


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
        _ctx[key] = pyrt.Context(pick_ref.case_scene(c), **kw)
    return _ctx[key]


def samples_of(c):
    p = pick_ref.case_params(c)
    return c[1] * c[2] * (p.spp_count if p.spp_count else p.spp)


@pytest.mark.parametrize("case", pick_ref.CASES, ids=pick_ref.case_id)
def test_pick_bit_exact(case):
    """P1 against the oracle: accumulator, resolved image, samples and both ray counts, whatever the schedule."""
    ctx, bg = context(case), pick_ref.case_background(case)
    for name, kw, brute in SCHEDULES:
        ref = pick_ref.case_reference(case, brute)
        what = "%s, %s" % (pick_ref.case_id(case), name)
        out, acc, st = ctx.render_pick(pick_ref.case_params(case, **kw), pick_ref.case_pick(case), bg=bg)
        assert_frames_equal(acc, ref["accum"], "accum " + what)
        assert_frames_equal(out, ref["out"], "out " + what)
        assert (st.rays_closest, st.rays_shadow) == (ref["closest"], ref["shadow"]), what
        assert st.samples == samples_of(case) and st.kernel_ms > 0, what
        if kw.get("collect_stats"):
            assert st.tris_tested > 0 and (brute or st.nodes_visited > st.rays_closest), what


def test_a_sample_is_rt_render_on_a_context_with_its_tuples_lights():
    """P1 on the library's own frames: per distinct tuple a second context, given that tuple's scaled lights by
    rt_update, renders every one-sample range with rt_render_device; each pixel's row comes from its own tuple's frame."""
    import torch
    case = next(c for c in pick_ref.CASES if c[0] == ("lowres", False, 4))
    ctx, s = context(case), pick_ref.case_scene(case)
    w, h, p = case[1], case[2], pick_ref.case_params(case)
    s0, s1 = pick_ref.sample_range(p)
    table, k = pick_ref.case_table(case), pick_ref.case_picks(case).reshape(h * w, s1 - s0, -1)
    _, acc, st = ctx.render_pick(p, pick_ref.case_pick(case))
    rows = np.zeros((s1 - s0, h * w, 4), F32)
    closest = shadow = 0
    tuples = np.unique(k.reshape(-1, k.shape[-1]), axis=0)
    other = pyrt.Context(pick_ref.with_lights(s, table["lights"][list(tuples[0])]))
    try:
        for t, tup in enumerate(tuples):
            other.update(lights=np.ascontiguousarray(table["lights"][list(tup)]))
            for i in range(s0, s1):
                sel = (k[:, i - s0] == tup).all(axis=1)
                if not sel.any() and t != 0:
                    continue
                d = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
                est = other.render_device(pick_ref.case_params(case, spp_begin=i, spp_count=1), d.data_ptr(), stats=True)
                rows[i - s0][sel] = d.cpu().numpy().reshape(-1, 4)[sel]
                if t == 0:  # (P3: any one tuple's counts)
                    closest, shadow = closest + est.rays_closest, shadow + est.rays_shadow
    finally:
        other.close()
    exp = np.zeros((h * w, 4), F32)
    for r in rows:
        exp = (exp + r).astype(F32)
    assert_frames_equal(acc, exp.reshape(h, w, 4), "gathered from rt_render_device's frames")
    assert (st.rays_closest, st.rays_shadow) == (closest, shadow)


def test_one_light_and_one_slot_is_rt_render():
    """P2: n = 1, m = 1 — the weight is 1 — gives rt_render's frame, image and stats under every schedule."""
    case = next(c for c in pick_ref.CASES if c[0][2] == 1)
    assert pick_ref.case_slots(case) == 1 and pick_ref.case_table(case)["weights"][0] == 1
    ctx, bg = context(case), pick_ref.case_background(case)
    for name, kw, _ in SCHEDULES:
        p = pick_ref.case_params(case, **kw)
        eout, eacc, est = ctx.render(p, bg)
        out, acc, st = ctx.render_pick(p, 1, bg=bg)
        assert_frames_equal(acc, eacc, "accum " + name)
        assert_frames_equal(out, eout, "out " + name)
        assert (st.rays_closest, st.rays_shadow, st.samples) == (est.rays_closest, est.rays_shadow, est.samples), name


@pytest.mark.parametrize("case", pick_ref.CASES[:3], ids=pick_ref.case_id)
def test_hits_and_counts_do_not_depend_on_the_picks(case):
    """P3: .w, samples and both ray counts are rt_render's on the same geometry with any m lights — here the first m of
    the scene's — and the same under another importance."""
    s, m = pick_ref.case_scene(case), pick_ref.case_slots(case)
    p = pick_ref.case_params(case)
    _, acc, st = context(case).render_pick(p, pick_ref.case_pick(case))
    other = pyrt.Context(pick_ref.with_lights(s, pick_ref.scene_lights(s)[:m]))
    try:
        _, eacc, est = other.render(p)
    finally:
        other.close()
    assert (bits(acc[..., 3]) == bits(eacc[..., 3])).all()
    assert (st.rays_closest, st.rays_shadow, st.samples) == (est.rays_closest, est.rays_shadow, est.samples)
    q = np.arange(1, len(pick_ref.scene_lights(s)) + 1, dtype=F32)
    _, acc2, st2 = context(case).render_pick(p, m, importance=q)
    assert (bits(acc2[..., 3]) == bits(acc[..., 3])).all() and (bits(acc2) != bits(acc)).any()
    assert (st2.rays_closest, st2.rays_shadow, st2.samples) == (st.rays_closest, st.rays_shadow, st.samples)


@pytest.mark.parametrize("pooled", [True, False])
def test_sample_ranges_chain_and_host_equals_device(pooled):
    """P4: [0, 3) then [3, 7) into one device accumulator is [0, 7), which is the host form's frame; the tail alone is
    the [3, 7) case's own reference; the accumulator resolves with rt_resolve_device to the host form's image."""
    import torch
    tail = next(c for c in pick_ref.CASES if c[3] is pick_ref.SPP7_34 and c[0][2] > 3)
    w, h, pk = tail[1], tail[2], pick_ref.case_pick(tail)
    kw = dict() if pooled else dict(no_pool=True)
    ctx, bg = context(tail), pick_ref.case_background(tail)
    acc = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    whole = torch.zeros_like(acc)
    stream = torch.cuda.current_stream()
    for b, cnt in ((0, 3), (3, 4)):
        ctx.render_pick_device(pick_ref.case_params(tail, spp_begin=b, spp_count=cnt, **kw), pk, acc.data_ptr(), stream=stream.cuda_stream)
        if b == 0:
            stream.synchronize()
            head = acc.cpu().numpy().copy()
    full = pick_ref.case_params(tail, spp_begin=0, spp_count=0, **kw)
    st = ctx.render_pick_device(full, pk, whole.data_ptr(), stream=stream.cuda_stream, stats=True)
    dbg = torch.from_numpy(bg).cuda()
    dout = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
    ctx.resolve_device(w, h, full.spp, whole.data_ptr(), dbg.data_ptr(), dout.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    hout, host, hst = ctx.render_pick(full, pk, bg=bg)
    assert_frames_equal(whole.cpu().numpy(), host, "device form against host form")
    assert_frames_equal(dout.cpu().numpy(), hout, "rt_resolve_device against the host form's image")
    assert (st.rays_closest, st.rays_shadow, st.samples) == (hst.rays_closest, hst.rays_shadow, hst.samples)
    assert_frames_equal(acc.cpu().numpy(), host, "[0, 3) then [3, 7)")
    assert head[..., 3].max() == 3 and (bits(head) != bits(host)).any()
    _, alone, _ = ctx.render_pick(pick_ref.case_params(tail, **kw), pk)
    assert_frames_equal(alone, pick_ref.case_reference(tail)["accum"], "[3, 7) alone")
    only, _, _ = ctx.render_pick(full, pk, bg=bg, want_accum=False)
    assert_frames_equal(only, hout, "the image alone")


def test_q8_context_gives_the_same_bits():
    """An RT_NODES_Q8 context walks its resident 32-byte records: the same frame."""
    case = next(c for c in pick_ref.CASES if c[0] == ("lowres", True, 2))
    ctx = context(case, bvh_builder=pyrt.BVH_HOST, node_format=pyrt.NODES_Q8)
    assert ctx.bvh_info().node_format == pyrt.NODES_Q8
    ref = pick_ref.case_reference(case)
    for no_pool in (False, True):
        _, acc, st = ctx.render_pick(pick_ref.case_params(case, no_pool=no_pool), pick_ref.case_pick(case))
        assert_frames_equal(acc, ref["accum"], "Q8 context")
        assert (st.rays_closest, st.rays_shadow) == (ref["closest"], ref["shadow"])


def test_two_importance_arrays_back_to_back_on_a_busy_non_blocking_stream():
    """Two calls with different importance arrays on a non-blocking stream that is still busy return without waiting: each
    table was staged before its call returned — the caller overwrites its array between them — and the accumulators,
    zeroed behind the delay, hold the references' bits once the stream has run."""
    a, b = [c for c in pick_ref.CASES if c[0] == ("lowres", False, 6)]
    if a[7] is None:
        a, b = b, a
    assert a[7] is not None and b[7] is None
    ctx = pyrt.Context(pick_ref.case_scene(a))
    busy = Busy()
    acc_a = busy.out((a[2], a[1], 4), zeroed=True)
    acc_b = busy.out((b[2], b[1], 4), zeroed=True)
    busy.start()
    q = np.array(a[7], F32)
    pk = pyrt.LightPick()
    pk.slots, pk.n_importance, pk.importance = pick_ref.case_slots(a), len(q), q.ctypes.data
    ctx.render_pick_device(pick_ref.case_params(a), pk, acc_a.ptr, stream=busy.ptr)
    q[:] = pick_ref.case_table(b)["q"].astype(F32)  # (the caller's array is its own again: b's default, given explicitly)
    ctx.render_pick_device(pick_ref.case_params(b), pk, acc_b.ptr, stream=busy.ptr)
    was_busy = busy.issued()
    got_a, got_b = busy.fetch(acc_a), busy.fetch(acc_b)
    busy.finish()
    ctx.close()
    assert_frames_equal(got_a.numpy(), pick_ref.case_reference(a)["accum"], "first array")
    # (the float32 copy of the default q_k: its own table, restated)
    tb = pick_ref.table(pick_ref.scene_lights(pick_ref.case_scene(b)), pick_ref.case_slots(b), q)
    exp = pick_ref.build(b, tb["lights"], pick_ref.picks(pick_ref.case_params(b), tb["thresholds"], pick_ref.case_slots(b)), tag="f32 q")
    assert_frames_equal(got_b.numpy(), exp["accum"], "second array")
    assert (bits(got_a.numpy()) != bits(got_b.numpy())).any()
    assert was_busy, "the delay ended before the calls were issued (%.3f ms)" % busy.issue_ms


def test_context_untouched():
    case = pick_ref.CASES[0]
    ctx = pyrt.Context(pick_ref.case_scene(case))
    fp = pyrt.make_params(case[1], case[2], 4, seed=3)
    _, frame0, _ = ctx.render(fp)
    info0 = ctx.bvh_info()
    ctx.render_pick(pick_ref.case_params(case), pick_ref.case_pick(case))
    ctx.render_pick(pick_ref.case_params(case), 3, importance=np.arange(1, 6, dtype=F32))
    _, frame1, _ = ctx.render(fp)
    assert (ctx.bvh_info().pad, ctx.bvh_info().n_nodes) == (info0.pad, info0.n_nodes)
    ctx.close()
    assert (bits(frame0) == bits(frame1)).all()


def test_rejections_that_read_the_context():
    """No lights, an n_importance that is not n_lights and a weight that is not finite are RT_ERR_INVALID, name their
    numbers and write nothing."""
    L = pyrt.amd()
    case = pick_ref.CASES[0]
    w, h, p = case[1], case[2], pick_ref.case_params(case)
    acc = np.full((h, w, 4), 3.0, F32)
    out = np.full((h, w, 3), 3.0, F32)
    bg = pick_ref.case_background(case)

    def call(ctx, pk):
        return L.rt_render_pick(ctx._h, C.byref(p), C.byref(pk), bg.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p),
                                acc.ctypes.data_as(C.c_void_p), None)

    ctx = context(case)
    for n in (4, 6, 1):
        assert call(ctx, pyrt.make_light_pick(2, np.ones(n, F32))) == INVALID
        assert b"n_importance %d" % n in L.rt_last_error() and b"n_lights 5" in L.rt_last_error(), L.rt_last_error()
    # p_1 = 1e-45 / 3e38 underflows 1 / (m p) past float32: named
    assert call(ctx, pyrt.make_light_pick(1, np.array([3e38, 1e-45, 0, 0, 0], F32))) == INVALID
    assert b"light 1" in L.rt_last_error() and b"not finite" in L.rt_last_error(), L.rt_last_error()
    dark = pyrt.Context(pick_ref.with_lights(pick_ref.case_scene(case), np.zeros((0, 21), F32)))
    try:
        assert call(dark, pyrt.make_light_pick(1)) == INVALID and b"no lights" in L.rt_last_error()
    finally:
        dark.close()
    assert (acc == 3).all() and (out == 3).all()
    assert call(ctx, pyrt.make_light_pick(2, np.ones(5, F32))) == pyrt.RT_OK, L.rt_last_error()
