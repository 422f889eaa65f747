"""rt_render_rays: the integrator over caller-given ray batches, bit for bit against the oracle's frames of the
degenerate cameras (tests/rays_ref.py) — accumulator, resolved rows and ray counts on rays_ref.CASES (1 to 130 rays:
partial waves and wave boundaries; the four sample ranges; ray mode and path mode at depths 1 to 3; both accelerators;
closed and open scenes), then the tree forms, stream_index, chained ranges, a far origin, the device form with
degenerate directions, a refit scene, the untouched context, four lights, and today's route through rt_render_views."""
import numpy as np
import pytest

import pyrt
import rays_ref

pytestmark = pytest.mark.gpu

_ctx = {}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_rows_equal(got, exp, what=""):
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    diff = (bits(got) != bits(exp)).any(axis=1)
    assert not diff.any(), "%s: %d of %d rows differ, first %d: got %s, expected %s" % (
        what, int(diff.sum()), len(diff), int(np.argmax(diff)), got[np.argmax(diff)], exp[np.argmax(diff)])


@pytest.fixture(scope="module", autouse=True)
def contexts():
    yield
    for c in _ctx.values():
        c.close()
    _ctx.clear()


def context(name, opened, **kw):
    """One context per scene and option set, shared by the cases (the call changes nothing in it)."""
    key = (name, opened, tuple(sorted(kw.items())))
    if key not in _ctx:
        _ctx[key] = pyrt.Context(rays_ref.scene(name, opened), **kw)
    return _ctx[key]


@pytest.mark.parametrize("case", rays_ref.CASES, ids=rays_ref.case_id)
def test_rays_bit_exact(case):
    """Accumulator, resolved rows and the counts of closest-hit and shadow rays."""
    name, opened, n = case[:3]
    rays, _ = rays_ref.batch(name, opened, n)
    ref = rays_ref.case_reference(case)
    out, acc, st = context(name, opened).render_rays(rays_ref.case_params(case), rays, bg=rays_ref.case_background(n))
    assert_rows_equal(acc, ref["accum"], "accum " + rays_ref.case_id(case))
    assert_rows_equal(out, ref["out"], "out " + rays_ref.case_id(case))
    rng = case[3]
    assert st.samples == n * rng.get("spp_count", rng["spp"])
    assert (st.rays_closest, st.rays_shadow) == (ref["closest"], ref["shadow"])
    assert st.kernel_ms > 0


def test_collect_stats_counts_nodes_and_triangles():
    case = rays_ref.CASES[0]
    name, opened, n = case[:3]
    rays, _ = rays_ref.batch(name, opened, n)
    ref = rays_ref.case_reference(case)
    _, acc, st = context(name, opened).render_rays(rays_ref.case_params(case, collect_stats=1), rays)
    assert_rows_equal(acc, ref["accum"], "counted instance")
    assert (st.rays_closest, st.rays_shadow) == (ref["closest"], ref["shadow"])
    assert st.nodes_visited > st.rays_closest and st.tris_tested > 0


@pytest.mark.parametrize("case", [rays_ref.CASES[0], rays_ref.CASES[12], rays_ref.CASES[7]], ids=rays_ref.case_id)
def test_sequential_shading_gives_the_same_rows(case):
    """rt_params.reserved[1] bit 0 changes the schedule only: every vertex shaded by its own lane, one light after the other,
    instead of through the wave's ray pool — the body that also serves scenes of more than three lights."""
    name, opened, n = case[:3]
    assert not case[6]
    rays, _ = rays_ref.batch(name, opened, n)
    ref = rays_ref.case_reference(case)
    _, acc, st = context(name, opened).render_rays(rays_ref.case_params(case, no_pool=True), rays)
    assert_rows_equal(acc, ref["accum"], "sequential " + rays_ref.case_id(case))
    assert (st.rays_closest, st.rays_shadow) == (ref["closest"], ref["shadow"])


HIRES = [c for c in rays_ref.CASES if c[0] == "hires" and not c[6]]


@pytest.mark.parametrize("builder,node_format,expect", [
    (pyrt.BVH_HOST, pyrt.NODES_AUTO, pyrt.BVH_HOST), (pyrt.BVH_DEVICE, pyrt.NODES_AUTO, pyrt.BVH_DEVICE),
    (pyrt.BVH_HOST, pyrt.NODES_Q8, pyrt.BVH_HOST)], ids=["host", "device", "host_q8"])
def test_tree_forms(builder, node_format, expect):
    """Host-built, device-built and RT_NODES_Q8 contexts (which walk their resident 32-byte records) give the same rows."""
    assert len(HIRES) == 1
    c = HIRES[0]
    ctx = context(c[0], c[1], bvh_builder=builder, node_format=node_format)
    info = ctx.bvh_info()
    assert info.builder == expect
    if node_format == pyrt.NODES_Q8:
        assert info.node_format == pyrt.NODES_Q8
    rays, _ = rays_ref.batch(c[0], c[1], c[2])
    _, acc, st = ctx.render_rays(rays_ref.case_params(c), rays)
    ref = rays_ref.case_reference(c)
    assert_rows_equal(acc, ref["accum"], "builder %d format %d" % (builder, node_format))
    assert (st.rays_closest, st.rays_shadow) == (ref["closest"], ref["shadow"])


def test_stream_index():
    """NULL is arange; an explicit permutation keys every row by its entry, row by row."""
    case = next(c for c in rays_ref.CASES if c[:3] == ("lowres", True, 65) and not c[6])
    name, opened, n = case[:3]
    rays, ll = rays_ref.batch(name, opened, n)
    p, ctx = rays_ref.case_params(case), context(name, opened)
    ref = rays_ref.case_reference(case)
    _, explicit, _ = ctx.render_rays(p, rays, stream_index=np.arange(n, dtype=np.uint32))
    assert_rows_equal(explicit, ref["accum"], "arange")
    perm = np.random.default_rng(4).permutation(n).astype(np.uint32)
    assert (perm != np.arange(n)).sum() > n // 2
    exp = rays_ref.rows(rays_ref.scene(name, opened), rays, ll, p, stream_index=perm)
    _, got, st = ctx.render_rays(p, rays, stream_index=perm)
    assert_rows_equal(got, exp["accum"], "permutation")
    assert (st.rays_closest, st.rays_shadow) == (exp["closest"], exp["shadow"])
    lit = ref["accum"][:, :3].any(axis=1) & (perm != np.arange(n))
    # (another key is another stream: the lit rows change — but for one whose every sample clamps to the same sum)
    assert lit.sum() > 10 and (bits(got[lit]) != bits(ref["accum"][lit])).any(axis=1).mean() > 0.8


def test_sample_ranges_chain():
    """[0, 3) then [3, 7) into one device accumulator is [0, 7); the tail alone is its own reference."""
    import torch
    full = next(c for c in rays_ref.CASES if c[:3] == ("cubes", False, 65))
    assert full[3] is rays_ref.SPP7_34
    name, opened, n = full[:3]
    rays, ll = rays_ref.batch(name, opened, n)
    ctx = context(name, opened)
    d_rays = torch.from_numpy(rays.view(np.float32).reshape(n, 6).copy()).cuda()
    acc = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
    whole = torch.zeros_like(acc)
    stream = torch.cuda.current_stream()
    for b, cnt in ((0, 3), (3, 4)):
        ctx.render_rays_device(rays_ref.case_params(full, spp_begin=b, spp_count=cnt), d_rays.data_ptr(), n, acc.data_ptr(),
                               stream=stream.cuda_stream)
        if b == 0:
            stream.synchronize()
            head = acc.cpu().numpy().copy()
    ctx.render_rays_device(rays_ref.case_params(full, spp_begin=0, spp_count=0), d_rays.data_ptr(), n, whole.data_ptr(),
                           stream=stream.cuda_stream)
    stream.synchronize()
    exp = rays_ref.rows(rays_ref.scene(name, opened), rays, ll, rays_ref.case_params(full, spp_begin=0, spp_count=0), counts=False)
    assert_rows_equal(whole.cpu().numpy(), exp["accum"], "[0, 7)")
    assert_rows_equal(acc.cpu().numpy(), exp["accum"], "[0, 3) then [3, 7)")
    assert head[:, 3].max() == 3 and (bits(head) != bits(exp["accum"])).any()
    _, tail, _ = ctx.render_rays(rays_ref.case_params(full), rays)
    assert_rows_equal(tail, rays_ref.case_reference(full)["accum"], "[3, 7) alone")


def test_far_origin_takes_the_exhaustive_loop():
    """One ray from 100 times the scene's extent, aimed at the scene, among 63 near ones: beyond the context's origin bound
    (16 times the largest coordinate of geometry, camera and lights) its primary cast is the exhaustive loop."""
    name, opened, n = "cubes", False, 64
    s = rays_ref.scene(name, opened)
    a = s.arrays()
    rays, ll = rays_ref.batch(name, opened, n)
    reach = max(1.0, float(np.abs(a["pos"]).max()), float(np.abs(a["camera"][0]).max()), float(np.abs(a["lights"][:, :3]).max()))
    centre = ((a["pos"].max(axis=0) + a["pos"].min(axis=0)) / 2).astype(np.float32)
    o = (centre + np.float32(100 * reach) * np.array([0.6, 0.5, 0.62], np.float32)).astype(np.float32)
    assert np.abs(o).max() > 16 * reach
    far, far_ll = rays_ref.library_rays(o[None], (centre - o)[None] * np.float32(0.01))
    k = 29
    rays[k], ll[k] = far[0], far_ll[0]
    p = pyrt.make_params(1, 1, 4, seed=rays_ref.SEED, collect_stats=1)
    exp = rays_ref.rows(s, rays, ll, p)
    assert exp["accum"][k, 3] == 4 and exp["accum"][k, :3].any(), "the far ray hits the scene and carries light"
    _, acc, st = context(name, opened).render_rays(p, rays)
    assert_rows_equal(acc, exp["accum"], "far origin")
    assert (st.rays_closest, st.rays_shadow) == (exp["closest"], exp["shadow"])
    assert st.tris_tested >= 4 * s.desc.n_triangles, "four exhaustive primary casts"
    p.collect_stats = 0
    _, acc, _ = context(name, opened).render_rays(p, rays)
    assert_rows_equal(acc, exp["accum"], "far origin, timed instance")


def test_device_form_on_torch_buffers_with_degenerate_directions():
    """rt_render_rays_device on torch tensors and torch's stream; rows whose direction is null or NaN stay zero (the kernel
    tests the value) and cast nothing, the other 62 rows are the reference's; rt_resolve_device(n, 1) resolves the batch."""
    import torch
    name, opened, n = "lowres", True, 64
    s = rays_ref.scene(name, opened)
    rays, ll = rays_ref.batch(name, opened, n)
    p = pyrt.make_params(1, 1, 4, seed=rays_ref.SEED)
    exp = rays_ref.rows(s, rays, ll, p, bg=rays_ref.case_background(n))
    bad = (7, 52)
    assert exp["accum"][list(bad), 3].all(), "the replaced rays would have hit"
    dropped = rays_ref.rows(s, rays[list(bad)], ll[list(bad)], p, stream_index=bad)
    rays["direction"][bad[0]] = 0
    rays["direction"][bad[1]] = [np.nan, 1, 0]
    d_rays = torch.from_numpy(rays.view(np.float32).reshape(n, 6).copy()).cuda()
    acc = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
    bg = torch.from_numpy(rays_ref.case_background(n)).cuda()
    out = torch.full((n, 3), -7.0, dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream()
    ctx = context(name, opened)
    st = ctx.render_rays_device(p, d_rays.data_ptr(), n, acc.data_ptr(), stream=stream.cuda_stream, stats=True)
    ctx.resolve_device(n, 1, p.spp, acc.data_ptr(), bg.data_ptr(), out.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    got, res = acc.cpu().numpy(), out.cpu().numpy()
    keep = np.ones(n, bool)
    keep[list(bad)] = False
    assert keep.sum() == 62 and not got[~keep].any()
    assert_rows_equal(got[keep], exp["accum"][keep], "device form")
    assert_rows_equal(res[keep], exp["out"][keep], "resolved")
    assert (bits(res[~keep]) == bits(rays_ref.case_background(n)[~keep])).all(), "a row without a hit resolves to its background"
    assert (st.rays_closest, st.rays_shadow) == (exp["closest"] - dropped["closest"], exp["shadow"] - dropped["shadow"])
    # an index tensor too: the reversed keys
    idx = torch.arange(n - 1, -1, -1, dtype=torch.int32, device="cuda")
    acc.zero_()
    ctx.render_rays_device(p, d_rays.data_ptr(), n, acc.data_ptr(), d_stream_index=idx.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    rev = rays_ref.rows(s, rays[keep], ll[keep], p, stream_index=np.arange(n - 1, -1, -1)[keep], counts=False)
    assert_rows_equal(acc.cpu().numpy()[keep], rev["accum"], "device stream_index")


def test_after_update_the_moved_scenes_reference():
    """After rt_update turns a mesh the rows follow the moved scene (the refit tree)."""
    name, opened, n = "lowres", False, 65
    s = pyrt.Scene(name, rays_ref.FRAME_W, rays_ref.FRAME_H)
    a = s.arrays()
    rays, ll = rays_ref.batch(name, True, n)
    p = pyrt.make_params(1, 1, 4, seed=rays_ref.SEED)
    ctx = pyrt.Context(s)
    _, before, _ = ctx.render_rays(p, rays)
    phi = np.float32(np.deg2rad(30.0))
    c, sn = np.cos(phi, dtype=np.float32), np.sin(phi, dtype=np.float32)
    R = np.array([[c, 0, sn], [0, 1, 0], [-sn, 0, c]], np.float32)
    b, e = a["vtx_begin"][3], a["vtx_begin"][4]
    pos, nrm = a["pos"].copy(), a["nrm"].copy()
    pos[b:e] = (pos[b:e] @ R.T).astype(np.float32)
    nrm[b:e] = (nrm[b:e] @ R.T).astype(np.float32)
    ctx.update(pos=pos, nrm=nrm)
    moved = pyrt.ArrayScene(pos, nrm, a["tri"], a["tri_begin"], a["vtx_begin"], a["materials"], a["lights"], a["camera"])
    _, got, st = ctx.render_rays(p, rays)
    ctx.close()
    exp = rays_ref.rows(moved, rays, ll, p)
    assert (bits(got) != bits(before)).any(), "the move changes rows"
    assert_rows_equal(got, exp["accum"], "after rt_update")
    assert (st.rays_closest, st.rays_shadow) == (exp["closest"], exp["shadow"])


def test_context_untouched():
    """A frame rendered before and after a render_rays call — with rays from far outside — is bit-identical, and the box
    padding is the same."""
    name, opened, n = "cubes", False, 64
    s = rays_ref.scene(name, opened)
    ctx = pyrt.Context(s)
    fp = pyrt.make_params(rays_ref.FRAME_W, rays_ref.FRAME_H, 4, seed=3)
    _, frame0, _ = ctx.render(fp)
    pad0 = ctx.bvh_info().pad
    rays, _ = rays_ref.batch(name, opened, n)
    rays["origin"][7] = [900.0, -700.0, 800.0]
    ctx.render_rays(pyrt.make_params(1, 1, 2, seed=rays_ref.SEED), rays, stream_index=np.full(n, 5, np.uint32))
    _, frame1, _ = ctx.render(fp)
    assert ctx.bvh_info().pad == pad0
    ctx.close()
    assert (bits(frame0) == bits(frame1)).all()


def test_more_lights_than_the_pool_holds():
    """Four lights: more than the vertex pool's three, the sequential shading whichever schedule serves the others."""
    name, opened, n = "cubes", True, 65
    a = rays_ref.scene(name, opened).arrays()
    extra = a["lights"][:1].copy()
    extra[0, :3] += np.array([0.3, -0.2, 0.25], np.float32)
    lights = np.concatenate([a["lights"], extra])
    assert len(lights) == 4
    s4 = pyrt.ArrayScene(a["pos"], a["nrm"], a["tri"], a["tri_begin"], a["vtx_begin"], a["materials"], lights, a["camera"])
    rays, ll = rays_ref.batch(name, opened, n)
    p = pyrt.make_params(1, 1, 4, seed=rays_ref.SEED)
    exp = rays_ref.rows(s4, rays, ll, p)
    three = rays_ref.rows(rays_ref.scene(name, opened), rays, ll, p, counts=False)
    assert (bits(exp["accum"]) != bits(three["accum"])).any(), "the fourth light shows"
    ctx = pyrt.Context(s4)
    _, acc, st = ctx.render_rays(p, rays)
    ctx.close()
    assert_rows_equal(acc, exp["accum"], "four lights")
    assert (st.rays_closest, st.rays_shadow) == (exp["closest"], exp["shadow"]) and st.rays_shadow % 4 == 0


def test_equals_todays_route_through_render_views():
    """What a caller could do before: rt_render_views at 1x1 with one degenerate camera per ray.  View j is row j with
    every stream index 0."""
    name, opened, n = "lowres", True, 65
    rays, ll = rays_ref.batch(name, opened, n)
    cams = np.zeros((n, 4, 3), np.float32)
    cams[:, 0], cams[:, 1] = rays["origin"], ll
    p = pyrt.make_params(1, 1, 4, seed=rays_ref.SEED)
    ctx = context(name, opened)
    _, views, vst = ctx.render_views(p, cams)
    _, acc, st = ctx.render_rays(p, rays, stream_index=np.zeros(n, np.uint32))
    assert views[:, 0, 0, 3].any() and not views[:, 0, 0, 3].all()
    assert_rows_equal(acc, views.reshape(n, 4), "rt_render_views at 1x1")
    assert (st.rays_closest, st.rays_shadow, st.samples) == (vst.rays_closest, vst.rays_shadow, vst.samples)
