"""rt_set_skin / rt_update_skin: linear blend skinning of a resident rest pose on the device.  After every call the context
is compared with a second context that got rt_update with the arrays of tests/skin_ref.py (tree export, rt_bvh_info,
report) and its frames with the CPU oracle's of the deformed scene.  tests/test_skin_ref_cpu.py has vetted every pose used
here: none of them is passed by a kernel that copies, takes one bone for the blend or pairs weights and slots wrongly."""
import ctypes as C

import numpy as np
import pytest

import pyrt
import skin_ref as sk
import transform_ref as xf
from busystream import Busy
from test_gpu_update import BUILDERS, assert_frames_equal_oracle, bits, scene_of

pytestmark = pytest.mark.gpu


def info_of(ctx):
    """rt_bvh_info without build_ms (the wall time of each context's own build)."""
    bi = ctx.bvh_info()
    return {n: getattr(bi, n) for n, _ in bi._fields_ if n != "build_ms"}


def same_exports(e1, e2):
    return np.array_equal(e1[0], e2[0]) and np.array_equal(e1[1], e2[1])


def assert_same_context(ctx, other):
    assert same_exports(ctx.bvh_export(), other.bvh_export())
    assert info_of(ctx) == info_of(other)


def assert_equivalent(ctx, other, a, skin, bones, seed=5, spp=3, **kw):
    """ctx.update_skin(bones, **kw) leaves what other.update(apply(a, skin, bones), **kw) leaves; the frames are the
    oracle's of that scene."""
    pos, nrm = sk.apply(a, skin[0], skin[1], bones)
    rep = ctx.update_skin(bones, **kw)
    ref = other.update(pos=pos, nrm=nrm, **kw)
    assert (rep["refitted"], rep["photons_dropped"]) == (ref["refitted"], ref["photons_dropped"]) == (1, 0)
    assert rep["refit_ms"] > 0 and rep["total_ms"] >= rep["refit_ms"]
    assert_same_context(ctx, other)
    assert_frames_equal_oracle(ctx, scene_of(a, pos=pos, nrm=nrm, **kw), spp=spp, seed=seed, fresh=False)
    return pos, nrm


def skinned_pair(kind, builder=pyrt.BVH_AUTO):
    """(arrays, the bend's skin, a context with it resident, a second context without)."""
    s = pyrt.Scene(kind, 24, 24)
    a = s.arrays()
    ctx, other = pyrt.Context(s, bvh_builder=builder), pyrt.Context(s, bvh_builder=builder)
    skin = sk.bend_skin(a)
    ctx.set_skin(skin[0], skin[1], sk.BEND_BONES)
    return a, skin, ctx, other


@pytest.mark.parametrize("kind,builder,expect", BUILDERS)
def test_equivalence(kind, builder, expect):
    a, skin, ctx, other = skinned_pair(kind, builder)
    assert ctx.bvh_info().builder == expect
    for deg in sk.BEND_DEGS:
        pos, _ = assert_equivalent(ctx, other, a, skin, sk.bend_bones(deg), seed=int(deg))
        assert not np.array_equal(pos, a["pos"])
    ctx.close()
    other.close()


def test_absolute_not_cumulative():
    a, skin, ctx, other = skinned_pair("hires")
    exports = []
    for deg in (10.0, 30.0, 10.0):
        ctx.update_skin(sk.bend_bones(deg))
        exports.append(ctx.bvh_export())
    assert same_exports(exports[0], exports[2]) and not same_exports(exports[0], exports[1])
    ctx.close()
    other.close()


def test_the_rest_pose_is_shared_with_update_transforms():
    """A transforms call between two identical skin calls changes nothing about the second; update(pos=...) sets a new
    rest pose and keeps the skin; rt_rebuild keeps both."""
    a, skin, ctx, other = skinned_pair("lowres")
    _, nrm10 = assert_equivalent(ctx, other, a, skin, sk.bend_bones(10.0))
    first = ctx.bvh_export()
    t = pyrt.make_transforms(5)
    xf.set_mesh(t, 3, xf.rotation_y(20.0))
    ctx.update_transforms(xf.set_mesh(t, 4, translate=(-0.1, 0.05, 0.1)))
    assert not same_exports(first, ctx.bvh_export())
    ctx.update_skin(sk.bend_bones(10.0))
    assert same_exports(first, ctx.bvh_export())
    # new positions: the rest pose becomes {p2, the live (skinned) normals}, the skin stays
    p2 = a["pos"].copy()
    b, e = a["vtx_begin"][3], a["vtx_begin"][4]
    p2[b:e] = p2[b:e] * np.float32(0.75) + np.float32(0.125)
    ctx.update(pos=p2)
    other.update(pos=p2)
    rest = dict(a, pos=p2, nrm=nrm10)
    pos30, nrm30 = assert_equivalent(ctx, other, rest, skin, sk.bend_bones(30.0), seed=30)
    assert not np.array_equal(bits(nrm30), bits(sk.apply(a, skin[0], skin[1], sk.bend_bones(30.0))[1]))
    # a rebuild keeps the rest pose and the skin: the next pose is still taken from `rest`
    assert ctx.rebuild()["rebuilt"] == 1 and other.rebuild()["rebuilt"] == 1
    assert_equivalent(ctx, other, rest, skin, sk.bend_bones(60.0), seed=60)
    # ... and a released skin is gone
    ctx.clear_skin()
    with pytest.raises(pyrt.RtError) as e:
        ctx.update_skin(sk.bend_bones(10.0))
    assert e.value.code == 5
    ctx.clear_skin()  # (releasing nothing is fine)
    ctx.close()
    other.close()


@pytest.mark.parametrize("counts,n_bones", sk.BOUNDARY, ids=["%s-%d" % ("+".join(map(str, c)), n) for c, n in sk.BOUNDARY])
def test_boundaries(counts, n_bones):
    """Vertex counts at a wave's and a workgroup tile's edges under the random rig: the lanes of a wave take 0 to 4 slots,
    vertices of four zero weights sit between skinned ones and keep their bits, the last bone of the table is used."""
    a, bone, weight, bones = sk.boundary_case(counts, n_bones)
    s = scene_of(a)
    ctx, other = pyrt.Context(s), pyrt.Context(s)
    ctx.set_skin(bone, weight, n_bones)
    pos, nrm = assert_equivalent(ctx, other, a, (bone, weight), bones, spp=1)
    still = ~sk.skinned_rows(weight)
    assert still.any() and (~still).any() and int(bone[weight != 0].max()) == n_bones - 1
    assert np.array_equal(bits(pos[still]), bits(a["pos"][still])) and np.array_equal(bits(nrm[still]), bits(a["nrm"][still]))
    assert (np.signbit(pos[still]) & (pos[still] == 0)).any()
    # a second skin replaces the first: other slots, other bones
    bone2, weight2 = sk.random_skin(len(pos), n_bones, seed=77)
    ctx.set_skin(bone2, weight2, n_bones)
    assert_equivalent(ctx, other, a, (bone2, weight2), sk.random_bones(n_bones, 78), spp=1, seed=2)
    ctx.close()
    other.close()


def test_prev_positions_feed_the_motion_pass():
    torch = pytest.importorskip("torch")
    w = h = 32
    s = pyrt.Scene("lowres", w, h)
    a = s.arrays()
    ctx = pyrt.Context(s)
    skin = sk.bend_skin(a)
    ctx.set_skin(skin[0], skin[1], sk.BEND_BONES)
    stream = torch.cuda.current_stream()
    prev = torch.full((len(a["pos"]), 3), -7.0, device="cuda")
    torch.cuda.synchronize()
    ctx.update_skin(sk.bend_bones(10.0), d_prev_pos=prev.data_ptr(), stream=stream.cuda_stream)
    assert np.array_equal(bits(prev.cpu().numpy()), bits(a["pos"]))
    pos10, _ = sk.apply(a, skin[0], skin[1], sk.bend_bones(10.0))
    ctx.update_skin(sk.bend_bones(30.0), d_prev_pos=prev.data_ptr(), stream=stream.cuda_stream)
    assert np.array_equal(bits(prev.cpu().numpy()), bits(pos10))
    p = pyrt.make_params(w, h, 3, seed=11, mode=pyrt.MODE_PATH)
    host = ctx.render_motion(p, prev_pos=pos10)
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


def test_camera_and_lights_ride_along():
    a, skin, ctx, other = skinned_pair("lowres")
    cam = a["camera"].copy()
    cam[0:2, 2] += np.float32(60.0)  # (far enough to enlarge the padding)
    lights = np.concatenate([a["lights"][1:], a["lights"][:1]])
    lights[-1, 0:3] = [0.0, 0.9, 0.5]
    pad0 = ctx.bvh_info().pad
    assert_equivalent(ctx, other, a, skin, sk.bend_bones(30.0), camera=cam, lights=lights)
    assert ctx.bvh_info().pad > pad0
    fewer = a["lights"][:1].copy()
    assert_equivalent(ctx, other, a, skin, sk.bend_bones(60.0), camera=a["camera"], lights=fewer, seed=60)
    ctx.close()
    other.close()


def test_set_skin_keeps_the_photon_map_and_update_skin_releases_it():
    s = pyrt.Scene("cubes", 24, 24)
    a = s.arrays()
    ctx = pyrt.Context(s)
    ctx.build_photon_map(5000, seed=4)
    p = pyrt.make_params(24, 24, 2, mode=pyrt.MODE_RAY, seed=3, use_photons=1, k=10, photons_requested=5000)
    _, before, _ = ctx.render(p)
    state = (ctx.bvh_export(), info_of(ctx))
    n_bones = 3
    bone, weight = sk.random_skin(len(a["pos"]), n_bones, 1)
    ctx.set_skin(bone, weight, n_bones)
    _, after, _ = ctx.render(p)
    assert np.array_equal(bits(before), bits(after)) and same_exports(state[0], ctx.bvh_export()) and state[1] == info_of(ctx)
    rep = ctx.update_skin(sk.random_bones(n_bones, 2))
    assert rep["photons_dropped"] == 1 and rep["refitted"] == 1
    with pytest.raises(pyrt.RtError) as e:
        ctx.render(p)
    assert e.value.code == 5
    ctx.close()


def test_on_a_busy_stream():
    """One call on a non-blocking stream that is still busy: the positions it replaces, the tree and the next frame on
    that stream are the host form's.  (The call synchronises its stream, so the delay has run out when it returns.)"""
    w, h = 37, 29
    a, skin, ctx, ref = skinned_pair("lowres")
    # the first pose comes before the delay, so that the call under test replaces positions that are not rt_create's
    pos10, _ = sk.apply(a, skin[0], skin[1], sk.bend_bones(10.0))
    ctx.update_skin(sk.bend_bones(10.0))
    pos, nrm = sk.apply(a, skin[0], skin[1], sk.bend_bones(30.0))
    erep = ref.update(pos=pos, nrm=nrm)
    p = pyrt.make_params(w, h, 2, seed=5)
    exp = ref.render(p)[1]
    b = Busy()
    d_prev = b.out((len(pos), 3))
    acc = b.out((h, w, 4), zeroed=True)
    b.start()
    rep = ctx.update_skin(sk.bend_bones(30.0), d_prev_pos=d_prev.ptr, stream=b.ptr)
    assert b.issued() is False
    ctx.render_device(p, acc.ptr, stream=b.ptr)
    got, prev = b.fetch(acc), b.fetch(d_prev)
    b.finish()
    assert (rep["refitted"], rep["photons_dropped"]) == (erep["refitted"], erep["photons_dropped"]) == (1, 0)
    assert_same_context(ctx, ref)
    assert np.array_equal(bits(got.numpy()), bits(exp)) and np.array_equal(bits(prev.numpy()), bits(pos10))
    ctx.close()
    ref.close()


def test_rejections_leave_the_context_as_it_was():
    torch = pytest.importorskip("torch")
    s = pyrt.Scene("lowres", 24, 24)
    a = s.arrays()
    ctx = pyrt.Context(s)
    skin = sk.bend_skin(a)
    prev = torch.full((len(a["pos"]), 3), -7.0, device="cuda")
    torch.cuda.synchronize()
    p = pyrt.make_params(24, 24, 2, seed=9)
    L = pyrt.amd()

    def snapshot():
        return ctx.render(p)[1], ctx.bvh_export(), info_of(ctx)

    def unchanged(state):
        acc, export, info = snapshot()
        assert np.array_equal(bits(state[0]), bits(acc)) and same_exports(state[1], export) and state[2] == info
        assert bool((prev == -7).all())

    def rejected(code, word, t, n_bones=None, reserved=None):
        u = pyrt.SkinUpdate()
        u.bones = C.cast(t.ctypes.data, C.POINTER(pyrt.MeshTransform))
        u.n_bones = len(t) if n_bones is None else n_bones
        u.d_prev_pos = prev.data_ptr()
        if reserved is not None:
            u.reserved[reserved] = 1
        rep = pyrt.UpdateReport()
        rep.refitted = 7
        assert L.rt_update_skin(ctx._h, C.byref(u), None, C.byref(rep)) == code
        assert word in L.rt_last_error().decode() and rep.refitted == 0
        unchanged(state)

    # no resident skin
    state = snapshot()
    rejected(5, "no resident skin", sk.bend_bones(30.0))
    ctx.set_skin(skin[0], skin[1], sk.BEND_BONES)
    ctx.update_skin(sk.bend_bones(10.0))
    state = snapshot()
    t = sk.bend_bones(30.0)
    t["m"][3, 1, 2] = np.nan
    rejected(1, "bone 3", t)
    t = sk.bend_bones(30.0)
    t["n"][2, 0, 0] = np.inf
    rejected(1, "bone 2", t)
    t = sk.bend_bones(30.0)
    t["flags"][1] = pyrt.XF_STATIC
    rejected(1, "bone 1", t)
    rejected(1, "bones", sk.bend_bones(30.0), n_bones=sk.BEND_BONES - 1)
    rejected(1, "bones", sk.bend_bones(30.0, n_bones=sk.BEND_BONES + 1))
    rejected(1, "reserved", sk.bend_bones(30.0), reserved=3)
    t = sk.bend_bones(30.0)
    t["m"][:, :, :3], t["m"][:, :, 3] = np.eye(3, dtype=np.float32) * np.float32(3e38), np.float32(3e38)  # (finite entries)
    assert not np.isfinite(sk.apply(a, skin[0], skin[1], t)[0][a["tri"].reshape(-1)]).all()
    rejected(1, "non-finite vertex position", t)
    with pytest.raises(pyrt.RtError) as e:  # lights NULL with n_lights > 0
        u = pyrt.SkinUpdate()
        t = sk.bend_bones(30.0)
        u.bones, u.n_bones, u.n_lights = C.cast(t.ctypes.data, C.POINTER(pyrt.MeshTransform)), len(t), 2
        pyrt._check(L.rt_update_skin(ctx._h, C.byref(u), None, None))
    assert e.value.code == 1
    unchanged(state)

    # rt_set_skin: a rejected skin leaves the resident one in force
    def skin_rejected(word, bone, weight, n_bones):
        with pytest.raises(pyrt.RtError) as e:
            ctx.set_skin(bone, weight, n_bones)
        assert e.value.code == 1 and word in str(e.value)
        unchanged(state)

    bad = skin[0].copy()
    bad[5, 3] = sk.BEND_BONES  # (a slot of zero weight)
    skin_rejected("vertex 5 slot 3", bad, skin[1], sk.BEND_BONES)
    skin_rejected("vertices", skin[0][:-1], skin[1][:-1], sk.BEND_BONES)
    skin_rejected("vertices", np.concatenate([skin[0], skin[0][:1]]), np.concatenate([skin[1], skin[1][:1]]), sk.BEND_BONES)
    ctx.update_skin(sk.bend_bones(10.0))  # the bend's skin still: the bytes of the pose before
    unchanged(state)
    ctx.close()
    q8 = pyrt.Context(s, node_format=pyrt.NODES_Q8)
    with pytest.raises(pyrt.RtError) as e:
        q8.set_skin(skin[0], skin[1], sk.BEND_BONES)
    assert e.value.code == 4
    with pytest.raises(pyrt.RtError) as e:
        q8.update_skin(sk.bend_bones(30.0))
    assert e.value.code == 5  # (no skin can be resident there: that is answered first)
    q8.close()
