"""rt_render_ao: ambient occlusion and bent normals at the first hit, all three channels bit for bit against the CPU
restatement (tests/ao_ref.py: aov_ref's vertices, a numpy sampler pinned to the oracle, the oracle's trace) on the cases
ao_ref.CASES lists — every preset closed and without its room, 64x48, 37x23 and 1x1, the sample ranges, 1 to 256 rays,
both accelerators, both biases, the three distance forms — then the tree builders and Q8, a refit scene, ranges that
chain, NULL channels, the device form, and RT_UNIT_HEMISPHERE against the numpy sampler."""
import numpy as np
import pytest

import ao_ref
import orc
import pyrt

pytestmark = pytest.mark.gpu

CHANNELS = pyrt.AO_CHANNELS
_ctx = {}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_ao_equal(got, exp, what=""):
    for k in CHANNELS:
        assert got[k].shape == exp[k].shape, (what, k)
        diff = (bits(got[k]) != bits(exp[k])).reshape(got[k].shape[0], got[k].shape[1], -1).any(axis=2)
        assert not diff.any(), "%s: channel %s differs at %d pixels, first %s" % (what, k, int(diff.sum()), np.argwhere(diff)[0])


@pytest.fixture(scope="module", autouse=True)
def contexts():
    yield
    for c in _ctx.values():
        c.close()
    _ctx.clear()


def context(name, opened, w, h, **kw):
    """One context per scene and option set, shared by the cases (the pass changes nothing in it)."""
    key = (name, opened, w, h, tuple(sorted(kw.items())))
    if key not in _ctx:
        _ctx[key] = pyrt.Context(ao_ref.case_scene(name, opened, w, h), **kw)
    return _ctx[key]


def render_case(ctx, c, **kw):
    name, opened, w, h, rng, n_rays, brute, bias, dist = c
    s = ao_ref.case_scene(name, opened, w, h)
    return ctx.render_ao(ao_ref.case_params(c), n_rays, bias=bias, max_distance=ao_ref.case_distance(s, dist), **kw)


@pytest.mark.parametrize("case", ao_ref.CASES, ids=ao_ref.case_id)
def test_ao_bit_exact(case):
    name, opened, w, h = case[:4]
    assert_ao_equal(render_case(context(name, opened, w, h), case), ao_ref.case_reference(case), ao_ref.case_id(case))


HIRES = [c for c in ao_ref.CASES if c[0] == "hires" and c[2] == 37 and not c[6]]


@pytest.mark.parametrize("builder,node_format,expect", [
    (pyrt.BVH_HOST, pyrt.NODES_AUTO, pyrt.BVH_HOST), (pyrt.BVH_DEVICE, pyrt.NODES_AUTO, pyrt.BVH_DEVICE),
    (pyrt.BVH_HOST, pyrt.NODES_Q8, pyrt.BVH_HOST)], ids=["host", "device", "host_q8"])
def test_ao_tree_builders_and_q8(builder, node_format, expect):
    """Host- and device-built trees give the restatement's sums, unbounded and bounded, closed and open; RT_NODES_Q8
    contexts run the pass on their resident 32-byte records with the same result."""
    assert len(HIRES) == 2 and {c[1] for c in HIRES} == {False, True} and {c[8] > 0 for c in HIRES} == {False, True}
    for c in HIRES:
        ctx = context(c[0], c[1], c[2], c[3], bvh_builder=builder, node_format=node_format)
        info = ctx.bvh_info()
        assert info.builder == expect
        if node_format == pyrt.NODES_Q8:
            assert info.node_format == pyrt.NODES_Q8
        assert_ao_equal(render_case(ctx, c), ao_ref.case_reference(c), "builder %d format %d %s" % (builder, node_format, ao_ref.case_id(c)))


def turned(a, deg, slot=3):
    """Positions and normals with mesh `slot` turned about the y axis by `deg` degrees."""
    phi = np.float32(np.deg2rad(deg))
    c, s = np.cos(phi, dtype=np.float32), np.sin(phi, dtype=np.float32)
    R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], np.float32)
    b, e = a["vtx_begin"][slot], a["vtx_begin"][slot + 1]
    pos, nrm = a["pos"].copy(), a["nrm"].copy()
    pos[b:e] = (pos[b:e] @ R.T).astype(np.float32)
    nrm[b:e] = (nrm[b:e] @ R.T).astype(np.float32)
    return pos, nrm


def test_after_update_the_moved_scenes_reference():
    """After rt_update turns a mesh the sums are the restatement's for the turned scene (the refit tree, and the default
    bias from the moved vertices' box)."""
    w, h, n_rays = 37, 23, 3
    s = pyrt.Scene("lowres", w, h)
    a = s.arrays()
    ctx = pyrt.Context(s)
    p = pyrt.make_params(w, h, 4, seed=ao_ref.SEED)
    before = ctx.render_ao(p, n_rays)
    pos, nrm = turned(a, 30.0)
    ctx.update(pos=pos, nrm=nrm)
    moved = pyrt.ArrayScene(pos, nrm, a["tri"], a["tri_begin"], a["vtx_begin"], a["materials"], a["lights"], a["camera"])
    got = ctx.render_ao(p, n_rays)
    assert not np.array_equal(got["unoccluded"], before["unoccluded"])
    assert_ao_equal(got, ao_ref.ao_sums(moved, p, n_rays, accel=orc.ACCEL_OBVH), "after rt_update")
    dist = 0.1 * ao_ref.diagonal(moved)
    assert_ao_equal(ctx.render_ao(p, n_rays, max_distance=dist), ao_ref.ao_sums(moved, p, n_rays, max_distance=dist, accel=orc.ACCEL_OBVH),
                    "after rt_update, bounded")
    ctx.close()


def test_sample_ranges_chain_exactly():
    """The counts of [0, 3) plus those of [3, 7) are the counts of [0, 7) (the streams are keyed by the sample, not by the
    range), and each range is its own reference."""
    full = next(c for c in ao_ref.CASES if c[:4] == ("cubes", True, 37, 23) and c[4] is ao_ref.SPP7)
    tail = next(c for c in ao_ref.CASES if c[:4] == ("cubes", True, 37, 23) and c[4] is ao_ref.SPP7_34)
    assert full[5:] == tail[5:]
    head = full[:4] + (dict(spp=7, spp_begin=0, spp_count=3),) + full[5:]
    ctx = context(*full[:4])
    a, b, whole = render_case(ctx, head), render_case(ctx, tail), render_case(ctx, full)
    assert_ao_equal(a, ao_ref.case_reference(head), "head")
    for k in ("unoccluded", "hits"):
        assert np.array_equal(a[k] + b[k], whole[k]), k
    assert whole["unoccluded"].any() and a["unoccluded"].any() and b["unoccluded"].any()


def test_null_channels_shift_nothing():
    case = next(c for c in ao_ref.CASES if c[:4] == ("lowres", True, 37, 23) and not c[6])
    ctx, ref = context(*case[:4]), ao_ref.case_reference(case)
    for chans in (("unoccluded",), ("hits",), ("bent",), ("hits", "bent"), ("unoccluded", "bent")):
        got = render_case(ctx, case, channels=chans)
        assert sorted(got) == sorted(chans)
        for k in chans:
            assert np.array_equal(bits(got[k]), bits(ref[k])), (chans, k)


def test_device_form_on_torch_buffers():
    """rt_render_ao_device into torch tensors on torch's stream equals the reference; channels not given stay as they were."""
    import torch
    case = next(c for c in ao_ref.CASES if c[:4] == ("lowres", False, 37, 23))
    name, opened, w, h, rng, n_rays, brute, bias, dist = case
    ctx, ref = context(name, opened, w, h), ao_ref.case_reference(case)
    d = ao_ref.case_distance(ao_ref.case_scene(name, opened, w, h), dist)
    dev = {k: torch.full((h, w, 3) if k == "bent" else (h, w), -7, dtype=torch.float32 if k == "bent" else torch.int32, device="cuda")
           for k in CHANNELS}
    stream = torch.cuda.current_stream()
    ctx.render_ao_device(ao_ref.case_params(case), n_rays, {k: v.data_ptr() for k, v in dev.items()}, bias=bias, max_distance=d,
                         stream=stream.cuda_stream)
    stream.synchronize()
    assert_ao_equal({k: v.cpu().numpy().view(ref[k].dtype) for k, v in dev.items()}, ref, "device form")
    part = {k: torch.full_like(v, 3) for k, v in dev.items()}
    torch.cuda.synchronize()
    ctx.render_ao_device(ao_ref.case_params(case), n_rays, {"bent": part["bent"].data_ptr()}, bias=bias, max_distance=d)
    torch.cuda.synchronize()
    assert np.array_equal(bits(part["bent"].cpu().numpy()), bits(ref["bent"]))
    assert bool((part["hits"] == 3).all()) and bool((part["unoccluded"] == 3).all())


def test_means():
    """ao_means is the stated formula in float32, on frames whose means are proper fractions (4 spp x 3 rays closed, and
    an open frame for the pixels without a hit)."""
    f = np.float32
    for case in (next(c for c in ao_ref.CASES if c[:6] == ("cubes", False, 37, 23, ao_ref.SPP4, 3)),
                 next(c for c in ao_ref.CASES if c[:6] == ("cubes", True, 64, 48, ao_ref.SPP4, 3))):
        n_rays = case[5]
        sums = render_case(context(*case[:4]), case)
        m = pyrt.ao_means(sums, n_rays)
        ref = ao_ref.case_reference(case)
        un, hits = ref["unoccluded"], ref["hits"]
        ao = np.where(hits > 0, un.astype(f) / np.maximum(hits.astype(f) * f(n_rays), f(1)), f(1))
        assert m["ao"].dtype == f and np.array_equal(bits(m["ao"]), bits(ao.astype(f)))
        assert ((ao > 0) & (ao < 1)).sum() > 100 and (case[1] is False or (hits == 0).any())
        assert m["bent"].dtype == f and np.array_equal(bits(m["bent"]), bits(ref["bent"] / np.maximum(un, 1).astype(f)[..., None]))
    empty = pyrt.ao_means(dict(unoccluded=np.zeros((2, 2), np.uint32), hits=np.zeros((2, 2), np.uint32)), 4)
    assert (empty["ao"] == 1).all() and "bent" not in empty


def test_unit_hemisphere_equals_the_numpy_sampler():
    """RT_UNIT_HEMISPHERE on 4,096 engine states: direction and end state bit for bit.  The normals: the axes and their
    negatives, equal absolute components (every tie of two_orthogonals), -0 components, the null vector, unnormalised and
    random ones."""
    rng = np.random.default_rng(13)
    special = [[1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0], [0, -1, 0], [0, 0, -1], [1, 1, 1], [-1, 1, 1], [1, -1, -1], [1, 1, 0],
               [0, 1, 1], [1, 0, 1], [-1, 0, 1], [2, 2, 0.5], [0.5, 2, 2], [2, 0.5, 2], [-0.0, 1, 0], [0, -0.0, 1], [1, 0, -0.0],
               [-0.0, -0.0, 1], [-0.0, -0.0, -0.0], [0, 0, 0], [1e-20, 0, 0], [3, 4, 12]]
    n = 4096
    normals = rng.normal(size=(n, 3)).astype(np.float32)
    for i in range(0, n // 2, len(special)):  # (the special ones many times over: each meets many engine states)
        k = min(len(special), n // 2 - i)
        normals[i:i + k] = np.asarray(special[:k], np.float32)
    states = ao_ref.stream_seed(5, ao_ref.STREAM_AO, np.arange(n), rng.integers(0, 2 ** 32, n, dtype=np.uint64))
    rows = np.empty((n, 4), np.uint32)
    rows[:, 0], rows[:, 1:] = states, normals.view(np.uint32)
    got = pyrt.unit(pyrt.UNIT_HEMISPHERE, rows)
    d, end = ao_ref.hemisphere_sample(states, normals)
    assert np.array_equal(got[:, :3], bits(d)) and np.array_equal(got[:, 3], end)
