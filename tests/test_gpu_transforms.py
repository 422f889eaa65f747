"""rt_update_transforms: one matrix per mesh, applied to a resident rest pose on the device.  After every call the context
is compared with a second context that got rt_update with the arrays of tests/transform_ref.py (tree export, rt_bvh_info,
report) and its frames with the CPU oracle's of the transformed scene."""
import ctypes as C

import numpy as np
import pytest

import pyrt
import transform_ref as xf
from test_gpu_update import BUILDERS, assert_frames_equal_oracle, bits, scene_of

pytestmark = pytest.mark.gpu

SHIFT = (-0.1, 0.05, 0.1)  # slot 4's translation (it stays inside the room)


def preset_transforms(deg):
    """Slot 3 turned by deg about the y axis, slot 4 translated, the three walls static."""
    t = pyrt.make_transforms(5)
    xf.set_mesh(t, 3, xf.rotation_y(deg))
    return xf.set_mesh(t, 4, translate=SHIFT)


def info_of(ctx):
    """rt_bvh_info without build_ms (the wall time of each context's own rt_create)."""
    bi = ctx.bvh_info()
    return {n: getattr(bi, n) for n, _ in bi._fields_ if n != "build_ms"}


def assert_same_context(ctx, other):
    for got, ref in zip(ctx.bvh_export(), other.bvh_export()):
        assert np.array_equal(got, ref)
    assert info_of(ctx) == info_of(other)


def assert_equivalent(ctx, other, a, t, seed=5, spp=3, **kw):
    """ctx.update_transforms(t, **kw) leaves what other.update(apply(a, t), **kw) leaves; the frames are the oracle's."""
    pos, nrm = xf.apply(a, t)
    rep = ctx.update_transforms(t, **kw)
    ref = other.update(pos=pos, nrm=nrm, **kw)
    assert (rep["refitted"], rep["photons_dropped"]) == (ref["refitted"], ref["photons_dropped"]) == (1, 0)
    assert rep["refit_ms"] > 0 and rep["total_ms"] >= rep["refit_ms"]
    assert_same_context(ctx, other)
    assert_frames_equal_oracle(ctx, scene_of(a, pos=pos, nrm=nrm, **kw), spp=spp, seed=seed, fresh=False)
    return pos, nrm


@pytest.mark.parametrize("kind,builder,expect", BUILDERS)
def test_equivalence(kind, builder, expect):
    s = pyrt.Scene(kind, 24, 24)
    a = s.arrays()
    ctx, other = pyrt.Context(s, bvh_builder=builder), pyrt.Context(s, bvh_builder=builder)
    assert ctx.bvh_info().builder == expect
    for deg in (5.0, 20.0, 90.0):
        pos, _ = assert_equivalent(ctx, other, a, preset_transforms(deg), seed=int(deg))
        assert not np.array_equal(pos, a["pos"])
    ctx.close()
    other.close()


def test_absolute_not_cumulative():
    s = pyrt.Scene("hires", 24, 24)
    ctx = pyrt.Context(s)
    exports = []
    for deg in (5.0, 20.0, 5.0):
        ctx.update_transforms(preset_transforms(deg))
        exports.append(ctx.bvh_export())
    assert np.array_equal(exports[0][0], exports[2][0]) and np.array_equal(exports[0][1], exports[2][1])
    assert not np.array_equal(exports[0][1], exports[1][1])
    ctx.close()


def test_update_with_arrays_sets_the_rest_pose():
    """update(pos=P2) after a transforms call: the rest pose becomes {P2, the live (transformed) normals}."""
    s = pyrt.Scene("lowres", 24, 24)
    a = s.arrays()
    ctx, other = pyrt.Context(s), pyrt.Context(s)
    _, nrm5 = assert_equivalent(ctx, other, a, preset_transforms(5.0))
    p2 = a["pos"].copy()
    b, e = a["vtx_begin"][3], a["vtx_begin"][4]
    p2[b:e] = p2[b:e] * np.float32(0.75) + np.float32(0.125)
    ctx.update(pos=p2)
    rest = dict(a, pos=p2, nrm=nrm5)
    pos, nrm = assert_equivalent(ctx, other, rest, preset_transforms(20.0), seed=20)
    assert not np.array_equal(bits(nrm), bits(xf.apply(a, preset_transforms(20.0))[1]))
    # ... and the device form that gives normals alone
    torch = pytest.importorskip("torch")
    n3 = torch.from_numpy(np.ascontiguousarray(a["nrm"][:, ::-1])).cuda()
    ctx.update_vertices_device(0, n3.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert_equivalent(ctx, other, dict(a, pos=pos, nrm=n3.cpu().numpy()), preset_transforms(5.0), seed=6)
    ctx.close()
    other.close()


def triangle_meshes(counts, seed):
    """A scene of len(counts) meshes inside the lowres room's walls: mesh j has counts[j] vertices and counts[j] - 2
    triangles over consecutive vertices, scattered in a slab facing the camera; materials cycle through lowres's."""
    base = pyrt.Scene("lowres", 24, 24).arrays()
    rng = np.random.default_rng(seed)
    nv = int(np.sum(counts))
    vb = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    centre = np.repeat(np.stack([rng.uniform(-1.2, 1.2, len(counts)), rng.uniform(-0.8, 1.2, len(counts)),
                                 rng.uniform(-1.2, 0.4, len(counts))], 1), counts, axis=0)
    pos = (centre + rng.uniform(-0.12, 0.12, (nv, 3))).astype(np.float32)
    nrm = rng.normal(size=(nv, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    pos[rng.integers(0, nv, 7), rng.integers(0, 3, 7)] = np.float32(-0.0)
    tri = np.concatenate([np.arange(c - 2)[:, None] + np.arange(3)[None, :] + vb[j] for j, c in enumerate(counts)]).astype(np.uint32)
    tb = np.concatenate([[0], np.cumsum(np.asarray(counts) - 2)]).astype(np.uint32)
    mats = base["materials"][np.arange(len(counts)) % len(base["materials"])]
    return dict(pos=pos, nrm=nrm, tri=tri, tri_begin=tb, vtx_begin=vb, materials=mats, lights=base["lights"], camera=base["camera"])


def own_matrices(a, seed, every_third_static=True):
    """Every mesh its own rotation about y, scale and small translation; every third one static."""
    n = len(a["vtx_begin"]) - 1
    rng = np.random.default_rng(seed)
    t = pyrt.make_transforms(n)
    for j in range(n):
        if every_third_static and j % 3 == 2:
            continue
        R = xf.rotation_y(rng.uniform(-180, 180)) * np.float32(rng.uniform(0.8, 1.1))
        xf.set_mesh(t, j, R, translate=rng.uniform(-0.05, 0.05, 3), normal=xf.rotation_y(rng.uniform(-180, 180)))
    return t


BOUNDARY_SCENES = [("70 one-triangle meshes", [3] * 70), ("1 triangle, 63, 64, 65, 257 vertices", [3, 63, 64, 65, 257]),
                   ("5,000 one-triangle meshes", [3] * 5000)]


@pytest.mark.parametrize("name,counts", BOUNDARY_SCENES, ids=[c[0] for c in BOUNDARY_SCENES])
def test_mesh_boundaries(name, counts):
    """Meshes that end inside a wave, at a wave's and a workgroup tile's edge, and more meshes than any table holds."""
    a = triangle_meshes(counts, len(counts))
    s = scene_of(a)
    ctx, other = pyrt.Context(s), pyrt.Context(s)
    t = own_matrices(a, 9)
    pos, nrm = assert_equivalent(ctx, other, a, t, spp=1)
    static = np.repeat(t["flags"] == pyrt.XF_STATIC, counts)
    assert static.any() and np.array_equal(bits(pos[static]), bits(a["pos"][static])) and not (pos[~static] == a["pos"][~static]).all()
    # all meshes moving under the identity: in value the rest pose, every -0 of it now +0
    ident = pyrt.make_transforms(len(counts))
    ident["flags"] = 0
    pos, _ = assert_equivalent(ctx, other, a, ident, spp=1, seed=2)
    assert (np.signbit(a["pos"]) & (a["pos"] == 0)).any() and np.array_equal(pos, a["pos"]) and not np.signbit(pos[pos == 0]).any()
    ctx.close()
    other.close()


def test_prev_positions_feed_the_motion_pass():
    torch = pytest.importorskip("torch")
    w = h = 32
    s = pyrt.Scene("lowres", w, h)
    a = s.arrays()
    ctx = pyrt.Context(s)
    stream = torch.cuda.current_stream()
    prev = torch.full((len(a["pos"]), 3), -7.0, device="cuda")
    torch.cuda.synchronize()
    ctx.update_transforms(preset_transforms(5.0), d_prev_pos=prev.data_ptr(), stream=stream.cuda_stream)
    assert np.array_equal(bits(prev.cpu().numpy()), bits(a["pos"]))
    pos5, _ = xf.apply(a, preset_transforms(5.0))
    ctx.update_transforms(preset_transforms(20.0), d_prev_pos=prev.data_ptr(), stream=stream.cuda_stream)
    assert np.array_equal(bits(prev.cpu().numpy()), bits(pos5))
    p = pyrt.make_params(w, h, 4, seed=11, mode=pyrt.MODE_PATH)
    host = ctx.render_motion(p, prev_pos=pos5)
    dev = {k: torch.full(host[k].shape, -7, dtype=torch.int32 if k == "mesh" else torch.float32, device="cuda") for k in pyrt.MOTION_CHANNELS}
    torch.cuda.synchronize()
    ctx.render_motion_device(p, {k: v.data_ptr() for k, v in dev.items()}, d_prev_pos=prev.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    for k in pyrt.MOTION_CHANNELS:
        assert np.array_equal(bits(dev[k].cpu().numpy()), bits(host[k])), k
    wall, moved = host["mesh"] <= 2, (host["mesh"] == 3) | (host["mesh"] == 4)
    assert wall.sum() > 100 and not host["motion"][wall].any()
    assert moved.sum() > 20 and (host["motion"][moved] != 0).any()
    ctx.close()


def test_rejections_leave_the_context_as_it_was():
    torch = pytest.importorskip("torch")
    s = pyrt.Scene("lowres", 24, 24)
    a = s.arrays()
    ctx = pyrt.Context(s)
    ctx.update_transforms(preset_transforms(5.0))
    p = pyrt.make_params(24, 24, 2, seed=9)
    _, before, _ = ctx.render(p)
    state = (ctx.bvh_export(), info_of(ctx))
    prev = torch.full((len(a["pos"]), 3), -7.0, device="cuda")
    torch.cuda.synchronize()

    def rejected(code, word, t, n_meshes=None, reserved=None):
        u = pyrt.TransformUpdate()
        u.transforms = C.cast(t.ctypes.data, C.POINTER(pyrt.MeshTransform))
        u.n_meshes = len(t) if n_meshes is None else n_meshes
        u.d_prev_pos = prev.data_ptr()
        if reserved is not None:
            u.reserved[reserved] = 1
        rep = pyrt.UpdateReport()
        assert pyrt.amd().rt_update_transforms(ctx._h, C.byref(u), None, C.byref(rep)) == code
        assert word in pyrt.amd().rt_last_error().decode() and rep.refitted == 0
        _, after, _ = ctx.render(p)
        assert np.array_equal(bits(before), bits(after))
        assert np.array_equal(state[0][0], ctx.bvh_export()[0]) and np.array_equal(state[0][1], ctx.bvh_export()[1]) and state[1] == info_of(ctx)
        assert bool((prev == -7).all())

    t = preset_transforms(20.0)
    t["m"][3, 1, 2] = np.nan
    rejected(1, "mesh 3", t)
    t = preset_transforms(20.0)
    t["n"][4, 0, 0] = np.inf
    rejected(1, "mesh 4", t)
    t = preset_transforms(20.0)
    xf.set_mesh(t, 0, np.eye(3, dtype=np.float32) * np.float32(3e38))  # (finite entries; the walls' 1.51 overflows)
    rejected(1, "non-finite vertex position", t)
    t = preset_transforms(20.0)
    t["flags"][0] = 4
    rejected(1, "flags", t)
    rejected(1, "meshes", preset_transforms(20.0), n_meshes=4)
    rejected(1, "meshes", pyrt.make_transforms(6))
    rejected(1, "reserved", preset_transforms(20.0), reserved=3)
    with pytest.raises(pyrt.RtError) as e:  # lights NULL with n_lights > 0
        u = pyrt.TransformUpdate()
        t = preset_transforms(20.0)
        u.transforms, u.n_meshes, u.n_lights = C.cast(t.ctypes.data, C.POINTER(pyrt.MeshTransform)), 5, 2
        pyrt._check(pyrt.amd().rt_update_transforms(ctx._h, C.byref(u), None, None))
    assert e.value.code == 1
    # a NaN in a static mesh's record is not read: accepted, and the result is the clean record's
    other = pyrt.Context(s)
    t = preset_transforms(20.0)
    t["m"][1, 0, 0] = t["n"][2, 2, 2] = np.nan
    assert_equivalent(ctx, other, a, t, seed=20)
    other.close()
    ctx.close()
    q8 = pyrt.Context(s, node_format=pyrt.NODES_Q8)
    with pytest.raises(pyrt.RtError) as e:
        q8.update_transforms(preset_transforms(20.0))
    assert e.value.code == 4
    q8.close()


def test_photon_map_is_released():
    s = pyrt.Scene("cubes", 48, 40)
    ctx = pyrt.Context(s)
    ctx.build_photon_map(5000, seed=4)
    p = pyrt.make_params(48, 40, 2, mode=pyrt.MODE_RAY, seed=3, use_photons=1, k=10, photons_requested=5000)
    ctx.render(p)
    rep = ctx.update_transforms(preset_transforms(20.0))
    assert rep["photons_dropped"] == 1 and rep["refitted"] == 1
    with pytest.raises(pyrt.RtError) as e:
        ctx.render(p)
    assert e.value.code == 5
    ctx.close()


def test_camera_and_lights_ride_along():
    s = pyrt.Scene("lowres", 24, 24)
    a = s.arrays()
    ctx, other = pyrt.Context(s), pyrt.Context(s)
    cam = a["camera"].copy()
    cam[0:2, 2] += np.float32(60.0)  # (far enough to enlarge the padding)
    lights = np.concatenate([a["lights"][1:], a["lights"][:1]])
    lights[-1, 0:3] = [0.0, 0.9, 0.5]
    pad0 = ctx.bvh_info().pad
    assert_equivalent(ctx, other, a, preset_transforms(20.0), camera=cam, lights=lights)
    assert ctx.bvh_info().pad > pad0
    fewer = a["lights"][:1].copy()
    assert_equivalent(ctx, other, a, preset_transforms(90.0), camera=a["camera"], lights=fewer, seed=90)
    ctx.close()
    other.close()
