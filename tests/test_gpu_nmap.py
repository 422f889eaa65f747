"""rt_set_normal_maps and rt_render_normal_mapped, bit for bit against tests/nmap_ref.py — a path walked vertex by vertex
from the oracle's trace, BSDF and light evaluation under the perturbed normal — on nmap_ref.CASES: accumulator, resolved
image, samples and both ray counts under the eight schedules of test_gpu_lights.SCHEDULES; then the change floor against
the library's own rt_render_material, N1 against rt_render_material and rt_render, N2 after rt_update of moved vertices and
after rt_update_transforms against a second context, chained ranges and host against device form, a Q8 context, the order
of rt_set_material_maps and rt_set_normal_maps and none of the former, the maps kept across rt_rebuild, stale maps after
rt_set_textures, the release and the rejections that read the context, and a context whose other frames resident normal
maps leave untouched."""
import ctypes as C

import numpy as np
import pytest

import mat_ref
import nmap_ref
import pyrt
import tex_ref
import transform_ref
from nmap_ref import map_args, set_args
from test_gpu_lights import SCHEDULES, assert_frames_equal, bits
from tex_ref import T_ALBEDO, T_MIXED, T_NONE

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
    ctx.set_normal_maps(mset["mesh_normal"])
    return ctx


def context(c, **kw):
    """One context per case's scene and map set and option set, with the case's textures and maps resident."""
    key = (nmap_ref.case_id(c) if c[6] == T_MIXED else (c[0], c[1], c[2], c[6]), tuple(sorted(kw.items())))
    if key not in _ctx:
        _ctx[key] = resident(pyrt.Context(nmap_ref.case_scene(c), **kw), nmap_ref.case_maps(c))
    return _ctx[key]


def samples_of(c):
    p = nmap_ref.case_params(c)
    return c[1] * c[2] * (p.spp_count if p.spp_count else p.spp)


def first(kind, field, value):
    """The first case of a kind whose field (an index into the case) is value."""
    return next(c for c in nmap_ref.CASES if c[6] == kind and c[field] == value)


def check(got, ref, what):
    out, acc, st = got
    assert_frames_equal(acc, ref["accum"], "accum " + what)
    assert_frames_equal(out, ref["out"], "out " + what)
    assert (st.rays_closest, st.rays_shadow) == (ref["closest"], ref["shadow"]), what


def as_ref(frame):
    out, acc, st = frame
    return dict(accum=acc, out=out, closest=st.rays_closest, shadow=st.rays_shadow)


@pytest.mark.parametrize("case", nmap_ref.CASES, ids=nmap_ref.case_id)
def test_normal_mapped_bit_exact(case):
    """Accumulator, resolved image, samples and both ray counts, whatever the schedule (N4)."""
    ctx, bg = context(case), nmap_ref.case_background(case)
    for name, kw, brute in SCHEDULES:
        ref = nmap_ref.case_reference(case, brute)
        what = "%s, %s" % (nmap_ref.case_id(case), name)
        out, acc, st = ctx.render_normal_mapped(nmap_ref.case_params(case, **kw), bg=bg)
        check((out, acc, st), ref, what)
        assert st.samples == samples_of(case) and st.kernel_ms > 0, what
        if kw.get("collect_stats"):
            assert st.tris_tested > 0 and (brute or st.nodes_visited > st.rays_closest), what


def test_the_mixed_maps_show():
    """The frames the cases compare are not the material ones (nmap_ref.MIN_CHANGED_N, from the reference alone), against
    the library's own rt_render_material."""
    for case in nmap_ref.CASES:
        if case[6] != T_MIXED:
            continue
        ctx, p = context(case), nmap_ref.case_params(case)
        _, mat, _ = ctx.render_material(p)
        _, acc, _ = ctx.render_normal_mapped(p)
        share = nmap_ref.changed_rgb_words(acc, mat)
        print("%-48s %.4f" % (nmap_ref.case_id(case), share))
        assert share > nmap_ref.MIN_CHANGED_N, nmap_ref.case_id(case)


@pytest.mark.parametrize("kind", ["null", "none", "flat"])
@pytest.mark.parametrize("case", nmap_ref.CASES[::2], ids=nmap_ref.case_id)
def test_n1_no_maps_and_flat_maps_are_rt_render_material(case, kind):
    """N1 on the library's own frames, under every schedule: a NULL table, a table of RT_TEX_NONE, and flat maps
    (0.5, 0.5, b) of every shape, filter and wrap on every mesh.  On the T1 / M1 sets the frame is rt_render's too."""
    s, bg = nmap_ref.case_scene(case), nmap_ref.case_background(case)
    i = nmap_ref.CASES.index(case)
    base = mat_ref.case_maps(case) if i % 4 == 0 else mat_ref.map_set(s, T_ALBEDO if i % 8 == 2 else T_NONE)
    plain = i % 4 != 0
    mset = nmap_ref.flat_set(base, s, i) if kind == "flat" else dict(base)
    if kind == "null":
        mset["mesh_normal"] = None
    elif kind == "none":
        mset["mesh_normal"] = np.full(len(base["mesh_texture"]), pyrt.TEX_NONE, np.uint32)
    ctx = pyrt.Context(s)
    try:
        resident(ctx, mset)
        for name, kw, _ in SCHEDULES:
            p = nmap_ref.case_params(case, **kw)
            got = ctx.render_normal_mapped(p, bg=bg)
            exp = ctx.render_material(p, bg=bg)
            check(got, as_ref(exp), "rt_render_material, %s, %s" % (kind, name))
            assert got[2].samples == exp[2].samples, name
            if plain:
                check(got, as_ref(ctx.render(p, bg)), "rt_render, %s, %s" % (kind, name))
    finally:
        ctx.close()


def moved_scene(s, pos, nrm=None):
    a = s.arrays()
    return pyrt.ArrayScene(pos, a["nrm"] if nrm is None else nrm, a["tri"], a["tri_begin"], a["vtx_begin"], a["materials"], a["lights"], a["camera"])


def test_n2_the_frame_follows_rt_update_and_rt_rebuild_keeps_the_maps():
    """Moved vertices (a shear, so that every tangent frame turns): the frame is the reference's on the moved scene and a
    fresh context's created on it, before and after rt_rebuild; it is not the frame before the move."""
    case = first(T_MIXED, 0, ("cubes", True))
    s, mset, p = nmap_ref.case_scene(case), nmap_ref.case_maps(case), nmap_ref.case_params(case)
    a = s.arrays()
    pos = a["pos"].copy()
    pos[:, 0] = (pos[:, 0] + F32(0.15) * pos[:, 1]).astype(F32)
    pos = (pos * F32(1.03) + F32(0.01)).astype(F32)
    moved = moved_scene(s, pos)
    exp = nmap_ref.frame(moved, p, mset)
    ctx, other = pyrt.Context(s), pyrt.Context(moved)
    try:
        resident(ctx, mset), resident(other, mset)
        ctx.update(pos=pos)
        _, acc, st = ctx.render_normal_mapped(p)
        assert_frames_equal(acc, exp["accum"], "after rt_update")
        assert (st.rays_closest, st.rays_shadow) == (exp["closest"], exp["shadow"])
        _, fresh, fst = other.render_normal_mapped(p)
        assert_frames_equal(acc, fresh, "against a fresh context")
        assert (st.rays_closest, st.rays_shadow) == (fst.rays_closest, fst.rays_shadow)
        ctx.rebuild()
        _, acc, st = ctx.render_normal_mapped(p)
        assert_frames_equal(acc, exp["accum"], "after rt_rebuild")
        assert (st.rays_closest, st.rays_shadow) == (exp["closest"], exp["shadow"])
        assert (bits(exp["accum"]) != bits(nmap_ref.case_reference(case)["accum"])).any()
    finally:
        ctx.close(), other.close()


def test_n2_the_frame_follows_rt_update_transforms():
    case = first(T_MIXED, 0, ("lowres", True))
    s, mset, p = nmap_ref.case_scene(case), nmap_ref.case_maps(case), nmap_ref.case_params(case)
    a = s.arrays()
    nm = len(a["tri_begin"]) - 1
    t = pyrt.make_transforms(nm)
    for j in range(nm):
        transform_ref.set_mesh(t, j, transform_ref.rotation_y(7.0 + 11.0 * j), translate=(0.02 * j, -0.01, 0.03))
    pos, nrm = transform_ref.apply(a, t)
    moved = moved_scene(s, pos, nrm)
    exp = nmap_ref.frame(moved, p, mset)
    ctx, other = pyrt.Context(s), pyrt.Context(moved)
    try:
        resident(ctx, mset), resident(other, mset)
        ctx.update_transforms(t)
        for no_pool in (False, True):
            q = nmap_ref.case_params(case, no_pool=no_pool)
            _, acc, st = ctx.render_normal_mapped(q)
            assert_frames_equal(acc, exp["accum"], "after rt_update_transforms")
            assert (st.rays_closest, st.rays_shadow) == (exp["closest"], exp["shadow"])
            _, fresh, _ = other.render_normal_mapped(q)
            assert_frames_equal(acc, fresh, "against a fresh context")
        assert (bits(exp["accum"]) != bits(nmap_ref.case_reference(case)["accum"])).any()
    finally:
        ctx.close(), other.close()


@pytest.mark.parametrize("pooled", [True, False])
def test_sample_ranges_chain_and_host_equals_device(pooled):
    """N3: [0, 3) then [3, 7) into one device accumulator is [0, 7), which is the host form's frame; the tail alone is the
    [3, 7) case's own reference; the accumulator resolves with rt_resolve_device to the host form's image."""
    import torch
    tail = first(T_MIXED, 3, tex_ref.SPP7_34)
    w, h = tail[1], tail[2]
    kw = dict() if pooled else dict(no_pool=True)
    ctx, bg = context(tail), nmap_ref.case_background(tail)
    acc = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    whole = torch.zeros_like(acc)
    stream = torch.cuda.current_stream()
    for b, cnt in ((0, 3), (3, 4)):
        ctx.render_normal_mapped_device(nmap_ref.case_params(tail, spp_begin=b, spp_count=cnt, **kw), acc.data_ptr(), stream=stream.cuda_stream)
        if b == 0:
            stream.synchronize()
            head = acc.cpu().numpy().copy()
    full = nmap_ref.case_params(tail, spp_begin=0, spp_count=0, **kw)
    st = ctx.render_normal_mapped_device(full, whole.data_ptr(), stream=stream.cuda_stream, stats=True)
    dbg = torch.from_numpy(bg).cuda()
    dout = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
    ctx.resolve_device(w, h, full.spp, whole.data_ptr(), dbg.data_ptr(), dout.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    hout, host, hst = ctx.render_normal_mapped(full, bg=bg)
    assert_frames_equal(whole.cpu().numpy(), host, "device form against host form")
    assert_frames_equal(dout.cpu().numpy(), hout, "rt_resolve_device against the host form's image")
    assert (st.rays_closest, st.rays_shadow, st.samples) == (hst.rays_closest, hst.rays_shadow, hst.samples)
    assert_frames_equal(acc.cpu().numpy(), host, "[0, 3) then [3, 7)")
    assert head[..., 3].max() == 3 and (bits(head) != bits(host)).any()
    _, alone, _ = ctx.render_normal_mapped(nmap_ref.case_params(tail, **kw))
    assert_frames_equal(alone, nmap_ref.case_reference(tail)["accum"], "[3, 7) alone")
    only, _, _ = ctx.render_normal_mapped(full, bg=bg, want_accum=False)
    assert_frames_equal(only, hout, "the image alone")


def test_q8_context_gives_the_same_bits():
    """An RT_NODES_Q8 context walks its resident 32-byte records: the same frame."""
    case = first(T_MIXED, 0, ("lowres", True))
    ctx = context(case, bvh_builder=pyrt.BVH_HOST, node_format=pyrt.NODES_Q8)
    assert ctx.bvh_info().node_format == pyrt.NODES_Q8
    ref = nmap_ref.case_reference(case)
    for no_pool in (False, True):
        _, acc, st = ctx.render_normal_mapped(nmap_ref.case_params(case, no_pool=no_pool))
        assert_frames_equal(acc, ref["accum"], "Q8 context")
        assert (st.rays_closest, st.rays_shadow) == (ref["closest"], ref["shadow"])


def test_either_order_of_the_two_map_calls_and_no_material_maps():
    """rt_set_normal_maps before rt_set_material_maps gives the frame of the other order; without material maps — never
    set, or released — the frame is the one under material tables that are RT_TEX_NONE everywhere."""
    case = first(T_MIXED, 0, ("cubes", False))
    s, mset, p = nmap_ref.case_scene(case), nmap_ref.case_maps(case), nmap_ref.case_params(case)
    bare = dict(mset)
    bare["mesh_f0"] = bare["mesh_kd_alpha"] = None
    exp_bare = nmap_ref.frame(s, p, bare)
    ref = nmap_ref.case_reference(case)
    ctx = pyrt.Context(s)
    try:
        ctx.set_textures(*set_args(mset))
        ctx.set_normal_maps(mset["mesh_normal"])
        for no_pool in (False, True):
            _, acc, st = ctx.render_normal_mapped(nmap_ref.case_params(case, no_pool=no_pool))
            assert_frames_equal(acc, exp_bare["accum"], "no material maps")
            assert (st.rays_closest, st.rays_shadow) == (exp_bare["closest"], exp_bare["shadow"])
        ctx.set_material_maps(*map_args(mset))  # (after the normal maps)
        _, acc, st = ctx.render_normal_mapped(p)
        assert_frames_equal(acc, ref["accum"], "normal maps first")
        assert (st.rays_closest, st.rays_shadow) == (ref["closest"], ref["shadow"])
        ctx.set_material_maps(release=True)
        _, acc, _ = ctx.render_normal_mapped(p)
        assert_frames_equal(acc, exp_bare["accum"], "material maps released")
        assert (bits(exp_bare["accum"]) != bits(ref["accum"])).any()
    finally:
        ctx.close()


def test_stale_maps_release_and_the_rejections_that_read_the_context():
    """Without textures, without normal maps, with normal maps or material maps set for another texture set the render
    calls answer RT_ERR_STATE, in that order, and write nothing; rt_set_normal_maps refuses another mesh count, a context
    without textures and an index beyond the resident set, naming the mesh; a new rt_set_normal_maps makes stale maps valid
    again; NULL releases."""
    import torch
    L = pyrt.amd()
    case = nmap_ref.CASES[0]
    w, h, p = case[1], case[2], nmap_ref.case_params(case)
    s, mset = nmap_ref.case_scene(case), nmap_ref.case_maps(case)
    nm, nt = len(mset["mesh_texture"]), len(mset["textures"])
    acc = np.full((h, w, 4), 3.0, F32)
    ptr = lambda x: x.ctypes.data_as(C.c_void_p)
    ref = nmap_ref.case_reference(case)["accum"]
    ctx = pyrt.Context(s)

    def frame_calls(word):
        d = torch.full((h, w, 4), 3.0, dtype=torch.float32, device="cuda")
        rcs = [L.rt_render_normal_mapped(ctx._h, C.byref(p), None, None, ptr(acc), None)]
        said = word in L.rt_last_error()
        rcs.append(L.rt_render_normal_mapped_device(ctx._h, C.byref(p), C.c_void_p(d.data_ptr()), None, None))
        said = said and word in L.rt_last_error()
        torch.cuda.synchronize()
        return rcs == [STATE] * 2 and said and bool((acc == 3).all()) and bool((d == 3).all())

    def set_refused(code, n, table, *words):
        m, keep = pyrt.normal_maps(n, table)
        assert L.rt_set_normal_maps(ctx._h, C.byref(m)) == code
        for word in words:
            assert word in L.rt_last_error(), (word, L.rt_last_error())

    try:
        # no textures: the frame and the maps both say so; the mesh count comes first
        assert frame_calls(b"rt_set_textures")
        set_refused(INVALID, nm + 1, None, b"normal maps: %d meshes" % (nm + 1), b"of %d" % nm)
        set_refused(STATE, nm, None, b"rt_set_textures")
        ctx.set_textures(*set_args(mset))
        assert frame_calls(b"rt_set_normal_maps")  # textures, no normal maps
        ctx.set_material_maps(*map_args(mset))
        assert frame_calls(b"rt_set_normal_maps")  # (material maps do not stand in for them)
        # the first entry that is neither an index nor RT_TEX_NONE
        good = np.full(nm, pyrt.TEX_NONE, np.uint32)
        bad = good.copy()
        bad[nm - 2], bad[nm - 1] = nt, 0xfffffffe
        set_refused(INVALID, nm, bad, b"mesh_normal[%d]" % (nm - 2), b"is %d" % nt, b"%d textures" % nt)
        set_refused(INVALID, nm - 1, good[:-1], b"%d meshes" % (nm - 1))
        assert frame_calls(b"rt_set_normal_maps")  # (a refused call sets nothing)
        ctx.set_normal_maps(mset["mesh_normal"])
        _, got, _ = ctx.render_normal_mapped(p)
        assert_frames_equal(got, ref, "after the rejected calls")
        set_refused(INVALID, nm, bad, b"mesh_normal")  # a refused call leaves the resident maps in place
        _, got, _ = ctx.render_normal_mapped(p)
        assert_frames_equal(got, ref, "after a refused call")
        # another texture set — even the same one again — makes both tables stale: the normal maps are named first, then
        # the material maps; rt_render_textured stays as it is
        ctx.set_textures(*set_args(mset))
        assert frame_calls(b"the normal maps were set for another texture set")
        ctx.set_normal_maps(mset["mesh_normal"])
        assert frame_calls(b"the material maps were set for another texture set")
        _, tex, _ = ctx.render_textured(p)
        assert_frames_equal(tex, mat_ref.case_textured_reference(case)["accum"], "rt_render_textured under stale maps")
        ctx.set_material_maps(*map_args(mset))
        _, got, _ = ctx.render_normal_mapped(p)
        assert_frames_equal(got, ref, "valid again")
        # a release of the textures: stale; of the normal maps: none
        ctx.set_textures(None)
        assert frame_calls(b"rt_set_textures")
        ctx.set_textures(*set_args(mset))
        assert frame_calls(b"another texture set")
        ctx.set_normal_maps(release=True)
        assert frame_calls(b"rt_set_normal_maps")
        ctx.set_normal_maps(release=True)  # (releasing nothing is not an error)
    finally:
        ctx.close()


def test_resident_normal_maps_change_no_other_frame():
    """rt_render, rt_render_textured and rt_render_material of a context are the same with and without resident normal
    maps."""
    case = nmap_ref.CASES[0]
    s, mset = nmap_ref.case_scene(case), nmap_ref.case_maps(case)
    ctx = pyrt.Context(s)
    fp = pyrt.make_params(case[1], case[2], 4, seed=3)
    try:
        ctx.set_textures(*set_args(mset))
        ctx.set_material_maps(*map_args(mset))
        _, frame0, st0 = ctx.render(fp)
        _, tex0, _ = ctx.render_textured(fp)
        _, mat0, mst0 = ctx.render_material(fp)
        info0 = ctx.bvh_info()
        ctx.set_normal_maps(mset["mesh_normal"])
        _, nrm1, _ = ctx.render_normal_mapped(nmap_ref.case_params(case))
        _, frame1, st1 = ctx.render(fp)
        _, tex1, _ = ctx.render_textured(fp)
        _, mat1, mst1 = ctx.render_material(fp)
        assert (ctx.bvh_info().pad, ctx.bvh_info().n_nodes) == (info0.pad, info0.n_nodes)
    finally:
        ctx.close()
    assert_frames_equal(nrm1, nmap_ref.case_reference(case)["accum"], "the normal-mapped frame between them")
    assert (bits(frame0) == bits(frame1)).all() and (bits(tex0) == bits(tex1)).all() and (bits(mat0) == bits(mat1)).all()
    assert (st0.rays_closest, st0.rays_shadow) == (st1.rays_closest, st1.rays_shadow)
    assert (mst0.rays_closest, mst0.rays_shadow) == (mst1.rays_closest, mst1.rays_shadow)
