"""rt_set_material_maps and rt_render_material, bit for bit against tests/mat_ref.py — the oracle's rays, hits, BSDF and
light evaluation under the sampled material — on mat_ref.CASES: accumulator, resolved image, samples and both ray counts
under the eight schedules of test_gpu_lights.SCHEDULES; then the change floors against the library's own
rt_render_textured, M1 against rt_render_textured and rt_render, M2 against rt_render on a second context of the
per-triangle-mesh scene, chained ranges, host against device form, a Q8 context, two map sets with frames between them back
to back on a busy non-blocking stream, the maps kept across rt_update and rt_rebuild, stale maps after rt_set_textures, the
release and the rejections that read the context, and a context whose other frames resident maps leave untouched."""
import ctypes as C

import numpy as np
import pytest

import mat_ref
import pyrt
import tex_ref
from busystream import Busy
from mat_ref import map_args, set_args
from test_gpu_lights import SCHEDULES, assert_frames_equal, bits
from tex_ref import T_ALBEDO, T_FACES, T_MIXED, T_NONE

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


def resident(ctx, mset):
    ctx.set_textures(*set_args(mset))
    ctx.set_material_maps(*map_args(mset))
    return ctx


def context(c, **kw):
    """One context per case's scene and map set and option set, with the case's textures and maps resident."""
    key = (mat_ref.case_id(c) if c[6] == T_MIXED else (c[0], c[1], c[2], c[6]), tuple(sorted(kw.items())))
    if key not in _ctx:
        _ctx[key] = resident(pyrt.Context(mat_ref.case_scene(c), **kw), mat_ref.case_maps(c))
    return _ctx[key]


def samples_of(c):
    p = mat_ref.case_params(c)
    return c[1] * c[2] * (p.spp_count if p.spp_count else p.spp)


def first(kind, field, value):
    """The first case of a kind whose field (an index into the case) is value."""
    return next(c for c in mat_ref.CASES if c[6] == kind and c[field] == value)


def check(got, ref, what):
    out, acc, st = got
    assert_frames_equal(acc, ref["accum"], "accum " + what)
    assert_frames_equal(out, ref["out"], "out " + what)
    assert (st.rays_closest, st.rays_shadow) == (ref["closest"], ref["shadow"]), what


def as_ref(frame):
    out, acc, st = frame
    return dict(accum=acc, out=out, closest=st.rays_closest, shadow=st.rays_shadow)


@pytest.mark.parametrize("case", mat_ref.CASES, ids=mat_ref.case_id)
def test_material_bit_exact(case):
    """Accumulator, resolved image, samples and both ray counts, whatever the schedule (M4)."""
    ctx, bg = context(case), mat_ref.case_background(case)
    for name, kw, brute in SCHEDULES:
        ref = mat_ref.case_reference(case, brute)
        what = "%s, %s" % (mat_ref.case_id(case), name)
        out, acc, st = ctx.render_material(mat_ref.case_params(case, **kw), bg=bg)
        check((out, acc, st), ref, what)
        assert st.samples == samples_of(case) and st.kernel_ms > 0, what
        if kw.get("collect_stats"):
            assert st.tris_tested > 0 and (brute or st.nodes_visited > st.rays_closest), what


def test_the_mixed_maps_show():
    """The frames the cases compare are not the textured ones (mat_ref.MIN_CHANGED*, from the reference alone): with all
    maps, with the f0 maps alone and with the (kd, alpha) maps alone, against the library's own rt_render_textured."""
    for case in mat_ref.CASES:
        if case[6] != T_MIXED:
            continue
        ctx, p, mset = context(case), mat_ref.case_params(case), mat_ref.case_maps(case)
        _, tex, _ = ctx.render_textured(p)
        try:
            for name, floor, args in (("all", mat_ref.MIN_CHANGED, map_args(mset)), ("f0", mat_ref.MIN_CHANGED_F0, (mset["mesh_f0"], None)),
                                      ("kda", mat_ref.MIN_CHANGED_KDA, (None, mset["mesh_kd_alpha"]))):
                ctx.set_material_maps(*args)
                _, acc, _ = ctx.render_material(p)
                share = mat_ref.changed_rgb_words(acc, tex)
                print("%-48s %-3s %.4f" % (mat_ref.case_id(case), name, share))
                assert share > floor, (mat_ref.case_id(case), name)
                assert (bits(acc[..., 3]) == bits(tex[..., 3])).all()
        finally:
            ctx.set_material_maps(*map_args(mset))


@pytest.mark.parametrize("kind", [T_NONE, T_ALBEDO, T_MIXED])
@pytest.mark.parametrize("case", mat_ref.CASES[::2], ids=mat_ref.case_id)
def test_m1_no_maps_and_own_field_maps_are_rt_render_textured(case, kind):
    """M1 on the library's own frames, under every schedule: T_NONE — the T1 set without textures and both tables NULL;
    T_ALBEDO — T1's albedo set with maps of the meshes' own f0 and (kd, alpha, 9): rt_render_textured's frame and, with T1,
    rt_render's; T_MIXED — the mixed albedo set under tables that are RT_TEX_NONE everywhere: rt_render_textured's."""
    s, bg = mat_ref.case_scene(case), mat_ref.case_background(case)
    mset = dict(mat_ref.map_set(s, kind))
    if kind == T_MIXED:
        nm = len(mset["mesh_texture"])
        mset["mesh_f0"] = mset["mesh_kd_alpha"] = np.full(nm, pyrt.TEX_NONE, np.uint32)
    ctx = pyrt.Context(s)
    try:
        resident(ctx, mset)
        for name, kw, _ in SCHEDULES:
            p = mat_ref.case_params(case, **kw)
            got = ctx.render_material(p, bg=bg)
            exp = ctx.render_textured(p, bg=bg)
            check(got, as_ref(exp), "rt_render_textured, %s, %s" % (kind, name))
            assert got[2].samples == exp[2].samples, name
            if kind != T_MIXED:
                check(got, as_ref(ctx.render(p, bg)), "rt_render, %s, %s" % (kind, name))
    finally:
        ctx.close()


@pytest.mark.parametrize("case", [c for c in mat_ref.CASES if c[6] == T_FACES], ids=mat_ref.case_id)
def test_m2_the_strips_are_rt_render_of_one_mesh_per_triangle(case):
    ctx, bg = context(case), mat_ref.case_background(case)
    other = pyrt.Context(mat_ref.per_triangle_scene(mat_ref.case_scene(case)))
    try:
        for name, kw, _ in SCHEDULES[:2] + SCHEDULES[6:7]:
            p = mat_ref.case_params(case, **kw)
            got, exp = ctx.render_material(p, bg=bg), other.render(p, bg)
            check(got, as_ref(exp), "rt_render, %s" % name)
            assert got[2].samples == exp[2].samples, name
    finally:
        other.close()


@pytest.mark.parametrize("pooled", [True, False])
def test_sample_ranges_chain_and_host_equals_device(pooled):
    """M3: [0, 3) then [3, 7) into one device accumulator is [0, 7), which is the host form's frame; the tail alone is the
    [3, 7) case's own reference; the accumulator resolves with rt_resolve_device to the host form's image."""
    import torch
    tail = first(T_MIXED, 3, tex_ref.SPP7_34)
    w, h = tail[1], tail[2]
    kw = dict() if pooled else dict(no_pool=True)
    ctx, bg = context(tail), mat_ref.case_background(tail)
    acc = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    whole = torch.zeros_like(acc)
    stream = torch.cuda.current_stream()
    for b, cnt in ((0, 3), (3, 4)):
        ctx.render_material_device(mat_ref.case_params(tail, spp_begin=b, spp_count=cnt, **kw), acc.data_ptr(), stream=stream.cuda_stream)
        if b == 0:
            stream.synchronize()
            head = acc.cpu().numpy().copy()
    full = mat_ref.case_params(tail, spp_begin=0, spp_count=0, **kw)
    st = ctx.render_material_device(full, whole.data_ptr(), stream=stream.cuda_stream, stats=True)
    dbg = torch.from_numpy(bg).cuda()
    dout = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
    ctx.resolve_device(w, h, full.spp, whole.data_ptr(), dbg.data_ptr(), dout.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    hout, host, hst = ctx.render_material(full, bg=bg)
    assert_frames_equal(whole.cpu().numpy(), host, "device form against host form")
    assert_frames_equal(dout.cpu().numpy(), hout, "rt_resolve_device against the host form's image")
    assert (st.rays_closest, st.rays_shadow, st.samples) == (hst.rays_closest, hst.rays_shadow, hst.samples)
    assert_frames_equal(acc.cpu().numpy(), host, "[0, 3) then [3, 7)")
    assert head[..., 3].max() == 3 and (bits(head) != bits(host)).any()
    _, alone, _ = ctx.render_material(mat_ref.case_params(tail, **kw))
    assert_frames_equal(alone, mat_ref.case_reference(tail)["accum"], "[3, 7) alone")
    only, _, _ = ctx.render_material(full, bg=bg, want_accum=False)
    assert_frames_equal(only, hout, "the image alone")


def test_q8_context_gives_the_same_bits():
    """An RT_NODES_Q8 context walks its resident 32-byte records: the same frame."""
    case = first(T_MIXED, 0, ("lowres", True))
    ctx = context(case, bvh_builder=pyrt.BVH_HOST, node_format=pyrt.NODES_Q8)
    assert ctx.bvh_info().node_format == pyrt.NODES_Q8
    ref = mat_ref.case_reference(case)
    for no_pool in (False, True):
        _, acc, st = ctx.render_material(mat_ref.case_params(case, no_pool=no_pool))
        assert_frames_equal(acc, ref["accum"], "Q8 context")
        assert (st.rays_closest, st.rays_shadow) == (ref["closest"], ref["shadow"])


def test_two_map_sets_with_frames_between_them_on_a_busy_non_blocking_stream():
    """maps A, a frame, maps B, a frame, on a non-blocking stream that is still busy: the first frame reads A — the tables
    it replaces are freed only once the launches that read them have run — and the second B (the f0 maps moved on by one
    mesh, no (kd, alpha) maps)."""
    case = first(T_MIXED, 0, ("cubes", False))
    s, (w, h) = mat_ref.case_scene(case), case[1:3]
    mset = mat_ref.case_maps(case)
    other = mat_ref.without(mset, "mesh_kd_alpha")
    other["mesh_f0"] = np.roll(mset["mesh_f0"], 1)
    exp_b = mat_ref.frame(s, mat_ref.case_params(case), other)
    ctx = pyrt.Context(s)
    busy = Busy()
    acc_a = busy.out((h, w, 4), zeroed=True)
    acc_b = busy.out((h, w, 4), zeroed=True)
    resident(ctx, mset)
    busy.start()
    ctx.render_material_device(mat_ref.case_params(case), acc_a.ptr, stream=busy.ptr)
    was_busy = busy.issued()
    ctx.set_material_maps(*map_args(other))
    ctx.render_material_device(mat_ref.case_params(case), acc_b.ptr, stream=busy.ptr)
    got_a, got_b = busy.fetch(acc_a), busy.fetch(acc_b)
    busy.finish()
    ctx.close()
    assert_frames_equal(got_a.numpy(), mat_ref.case_reference(case)["accum"], "first maps")
    assert_frames_equal(got_b.numpy(), exp_b["accum"], "second maps")
    assert (bits(got_a.numpy()) != bits(got_b.numpy())).any()
    assert was_busy, "the delay ended before the first call was issued (%.3f ms)" % busy.issue_ms


def test_the_maps_stay_across_rt_update_and_rt_rebuild():
    """New vertex positions refit the tree, rt_rebuild builds it again: the tables are indexed by mesh and stay."""
    case = first(T_MIXED, 0, ("cubes", True))
    s = mat_ref.case_scene(case)
    a = s.arrays()
    pos = (a["pos"] * F32(1.03) + F32(0.01)).astype(F32)
    moved = pyrt.ArrayScene(pos, a["nrm"], a["tri"], a["tri_begin"], a["vtx_begin"], a["materials"], a["lights"], a["camera"])
    p = mat_ref.case_params(case)
    exp = mat_ref.frame(moved, p, mat_ref.case_maps(case))
    ctx = pyrt.Context(s)
    try:
        resident(ctx, mat_ref.case_maps(case))
        ctx.update(pos=pos)
        _, acc, st = ctx.render_material(p)
        assert_frames_equal(acc, exp["accum"], "after rt_update")
        assert (st.rays_closest, st.rays_shadow) == (exp["closest"], exp["shadow"])
        ctx.rebuild()
        _, acc, st = ctx.render_material(p)
        assert_frames_equal(acc, exp["accum"], "after rt_rebuild")
        assert (bits(exp["accum"]) != bits(mat_ref.case_reference(case)["accum"])).any()
    finally:
        ctx.close()


def test_stale_maps_release_and_the_rejections_that_read_the_context():
    """Without textures, without maps or with maps set for another texture set the render calls answer RT_ERR_STATE and
    write nothing; rt_set_material_maps refuses another mesh count, a context without textures and an index beyond the
    resident set, naming the table and the mesh; a new rt_set_material_maps makes stale maps valid again; NULL releases."""
    import torch
    L = pyrt.amd()
    case = mat_ref.CASES[0]
    w, h, p = case[1], case[2], mat_ref.case_params(case)
    s, mset = mat_ref.case_scene(case), mat_ref.case_maps(case)
    nm, nt = len(mset["mesh_texture"]), len(mset["textures"])
    acc = np.full((h, w, 4), 3.0, F32)
    ptr = lambda x: x.ctypes.data_as(C.c_void_p)
    ref = mat_ref.case_reference(case)["accum"]
    ctx = pyrt.Context(s)

    def frame_calls(word):
        d = torch.full((h, w, 4), 3.0, dtype=torch.float32, device="cuda")
        rcs = [L.rt_render_material(ctx._h, C.byref(p), None, None, ptr(acc), None)]
        said = word in L.rt_last_error()
        rcs.append(L.rt_render_material_device(ctx._h, C.byref(p), C.c_void_p(d.data_ptr()), None, None))
        said = said and word in L.rt_last_error()
        torch.cuda.synchronize()
        return rcs == [STATE] * 2 and said and bool((acc == 3).all()) and bool((d == 3).all())

    def set_refused(code, n, f0, kda, *words):
        m, keep = pyrt.material_maps(n, f0, kda)
        assert L.rt_set_material_maps(ctx._h, C.byref(m)) == code
        for word in words:
            assert word in L.rt_last_error(), (word, L.rt_last_error())

    try:
        # no textures: the frame and the maps both say so; the mesh count comes first
        assert frame_calls(b"rt_set_textures")
        set_refused(INVALID, nm + 1, None, None, b"%d meshes" % (nm + 1), b"of %d" % nm)
        set_refused(STATE, nm, None, None, b"rt_set_textures")
        ctx.set_textures(*set_args(mset))
        assert frame_calls(b"rt_set_material_maps")  # textures, no maps
        # the first entry that is neither an index nor RT_TEX_NONE, mesh_f0 before mesh_kd_alpha
        good = np.full(nm, pyrt.TEX_NONE, np.uint32)
        bad = good.copy()
        bad[nm - 2], bad[nm - 1] = nt, 0xfffffffe
        set_refused(INVALID, nm, good, bad, b"mesh_kd_alpha[%d]" % (nm - 2), b"is %d" % nt, b"%d textures" % nt)
        set_refused(INVALID, nm, bad, bad, b"mesh_f0[%d]" % (nm - 2))
        set_refused(INVALID, nm - 1, good[:-1], None, b"%d meshes" % (nm - 1))
        assert frame_calls(b"rt_set_material_maps")  # (a refused call sets nothing)
        ctx.set_material_maps(*map_args(mset))
        _, got, _ = ctx.render_material(p)
        assert_frames_equal(got, ref, "after the rejected calls")
        set_refused(INVALID, nm, bad, None, b"mesh_f0")  # a refused call leaves the resident maps in place
        _, got, _ = ctx.render_material(p)
        assert_frames_equal(got, ref, "after a refused call")
        # another texture set — even the same one again — makes the maps stale, and leaves rt_render_textured as it is
        ctx.set_textures(*set_args(mset))
        assert frame_calls(b"another texture set")
        _, tex, _ = ctx.render_textured(p)
        assert_frames_equal(tex, mat_ref.case_textured_reference(case)["accum"], "rt_render_textured under stale maps")
        ctx.set_material_maps(*map_args(mset))
        _, got, _ = ctx.render_material(p)
        assert_frames_equal(got, ref, "valid again")
        # a release of the textures: stale; of the maps: none
        ctx.set_textures(None)
        assert frame_calls(b"rt_set_textures")
        ctx.set_textures(*set_args(mset))
        assert frame_calls(b"another texture set")
        ctx.set_material_maps(release=True)
        assert frame_calls(b"rt_set_material_maps")
        ctx.set_material_maps(release=True)  # (releasing nothing is not an error)
    finally:
        ctx.close()


def test_resident_maps_change_no_other_frame():
    """rt_render, rt_render_textured and rt_render_aov_textured of a context are the same with and without resident maps."""
    case = mat_ref.CASES[0]
    s, mset = mat_ref.case_scene(case), mat_ref.case_maps(case)
    ctx = pyrt.Context(s)
    fp = pyrt.make_params(case[1], case[2], 4, seed=3)
    try:
        ctx.set_textures(*set_args(mset))
        _, frame0, st0 = ctx.render(fp)
        _, tex0, _ = ctx.render_textured(fp)
        aov0 = ctx.render_aov_textured(fp, raw=True)
        info0 = ctx.bvh_info()
        ctx.set_material_maps(*map_args(mset))
        _, mat1, _ = ctx.render_material(mat_ref.case_params(case))
        _, frame1, st1 = ctx.render(fp)
        _, tex1, _ = ctx.render_textured(fp)
        aov1 = ctx.render_aov_textured(fp, raw=True)
        assert (ctx.bvh_info().pad, ctx.bvh_info().n_nodes) == (info0.pad, info0.n_nodes)
    finally:
        ctx.close()
    assert_frames_equal(mat1, mat_ref.case_reference(case)["accum"], "the material frame between them")
    assert (bits(frame0) == bits(frame1)).all() and (bits(tex0) == bits(tex1)).all()
    assert (st0.rays_closest, st0.rays_shadow) == (st1.rays_closest, st1.rays_shadow)
    for k in aov0:
        assert (bits(aov0[k]) == bits(aov1[k])).all(), k
