"""rt_update: a resident scene follows its description between frames (positions, normals, camera, lights,
materials), with the tree refit in place.  Every frame after an update is compared bit for bit with the CPU oracle's
frame of the updated scene, with a fresh context of it and with the exhaustive loop; the refit boxes with a numpy refit
of the tree's own topology."""
import ctypes as C

import numpy as np
import pytest

import orc
import pyrt
from raybatch import ray_batch

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def turned(a, deg, slot=3):
    """Positions and normals with mesh `slot` turned about the y axis by `deg` degrees (ScenePresets rotationY's matrix)."""
    phi = np.float32(np.deg2rad(deg))
    c, s = np.cos(phi, dtype=np.float32), np.sin(phi, dtype=np.float32)
    R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], np.float32)
    b, e = a["vtx_begin"][slot], a["vtx_begin"][slot + 1]
    pos, nrm = a["pos"].copy(), a["nrm"].copy()
    pos[b:e] = (pos[b:e] @ R.T).astype(np.float32)
    nrm[b:e] = (nrm[b:e] @ R.T).astype(np.float32)
    return pos, nrm


def scene_of(a, **kw):
    d = dict(a)
    d.update(kw)
    return pyrt.ArrayScene(d["pos"], d["nrm"], d["tri"], d["tri_begin"], d["vtx_begin"], d["materials"], d["lights"], d["camera"])


def pad_rule(a):
    """bvh_build.cpp paddingRule in float32: the padding of a scene description."""
    ref = np.abs(a["pos"][a["tri"].reshape(-1)]).max()
    pr = np.float32(max(np.float32(1), ref))
    for v in list(a["camera"][0]) + list(a["lights"][:, 0:3].reshape(-1)):
        if np.isfinite(v):
            pr = max(pr, np.float32(abs(v)))
    return np.float32(np.float32(6e-5) * pr)


def assert_frames_equal_oracle(ctx, s, w=24, h=24, spp=3, seed=5, modes=(pyrt.MODE_PATH, pyrt.MODE_RAY), fresh=True,
                               accel=orc.ACCEL_OBVH, **kw):
    """ctx's path and ray frames equal the oracle's frame of s (accumulators, image, ray counts), the exhaustive loop's
    and (fresh=True) a new context's of s."""
    bg = pyrt.background(w, h)
    other = pyrt.Context(s) if fresh else None
    for mode in modes:
        p = pyrt.make_params(w, h, spp, mode=mode, seed=seed, **kw)
        out, acc, st = ctx.render(p, bg)
        ref_out, ref_acc, ref_st = orc.render(s, p, math_mode=orc.MATH_DET, bg=bg, accel=accel)
        assert np.array_equal(bits(acc), bits(ref_acc)), "mode %d: accumulators differ from the oracle" % mode
        assert np.array_equal(bits(out), bits(ref_out))
        assert (st.rays_closest, st.rays_shadow) == (ref_st.rays_closest, ref_st.rays_shadow)
        _, brute, _ = ctx.render(pyrt.make_params(w, h, spp, mode=mode, seed=seed, accel=pyrt.ACCEL_BRUTE))
        assert np.array_equal(bits(acc), bits(brute))
        if other is not None:
            _, facc, _ = other.render(p)
            assert np.array_equal(bits(acc), bits(facc))
    if other is not None:
        other.close()


BUILDERS = [("lowres", pyrt.BVH_AUTO, pyrt.BVH_HOST), ("hires", pyrt.BVH_AUTO, pyrt.BVH_DEVICE),
            ("hires", pyrt.BVH_HYBRID, pyrt.BVH_HYBRID)]


@pytest.mark.parametrize("kind,builder,expect", BUILDERS)
def test_turntable_frames_equal_oracle(kind, builder, expect):
    """Slot 3 turned three times (Main.cpp:88-99 rotationY): after each update the frames are the oracle's of the turned
    scene, a fresh context's and the exhaustive loop's; the host builder's case also on the wavefront integrator."""
    s = pyrt.Scene(kind, 24, 24)
    a = s.arrays()
    ctx = pyrt.Context(s, bvh_builder=builder)
    assert ctx.bvh_info().builder == expect
    for deg in (5.0, 20.0, 90.0):
        pos, nrm = turned(a, deg)
        rep = ctx.update(pos=pos, nrm=nrm)
        assert rep["refitted"] == 1 and rep["photons_dropped"] == 0 and rep["refit_ms"] > 0 and rep["total_ms"] >= rep["refit_ms"]
        t = scene_of(a, pos=pos, nrm=nrm)
        assert_frames_equal_oracle(ctx, t, seed=int(deg))
        if expect == pyrt.BVH_HOST:
            p = pyrt.make_params(24, 24, 3, mode=pyrt.MODE_PATH, seed=int(deg), wavefront=True)
            _, acc, _ = ctx.render(p)
            _, ref, _ = orc.render(t, p, math_mode=orc.MATH_DET, accel=orc.ACCEL_OBVH)
            assert np.array_equal(bits(acc), bits(ref))
    ctx.close()


def numpy_refit(nodes, tris, pos, tri, pad):
    """The pre-update export's topology over new positions: leaf slots = float32 min / max of their triangles' vertices,
    lo - pad, hi + pad; inner slots = the union of the child's two slots.  Returns the expected (nodes, tris) exports."""
    nodes = nodes.copy()
    f = nodes.view(np.float32)
    child = nodes[:, 12:14].view(np.int32)
    depth = np.full(len(nodes), -1, np.int64)
    depth[0] = 0
    order = [0]
    for i in order:  # breadth first: parents before children
        for c in child[i]:
            if c >= 0:
                depth[c] = depth[i] + 1
                order.append(int(c))
    assert (depth >= 0).all()
    ids = tris[:, 9]
    for i in reversed(order):
        for k in range(2):
            c = int(child[i, k])
            if c >= 0:
                lo = np.minimum(f[c, 0:3], f[c, 6:9])
                hi = np.maximum(f[c, 3:6], f[c, 9:12])
            else:
                code = ~c
                first, cnt = code >> 3, (code & 7) + 1
                v = pos[tri[ids[first:first + cnt]].reshape(-1)]
                lo = (v.min(0) - pad).astype(np.float32)
                hi = (v.max(0) + pad).astype(np.float32)
            f[i, 6 * k:6 * k + 3], f[i, 6 * k + 3:6 * k + 6] = lo, hi
    t = tris.copy()
    tf = t.view(np.float32)
    v = tri[ids]
    p0, p1, p2 = pos[v[:, 0]], pos[v[:, 1]], pos[v[:, 2]]
    tf[:, 0:3], tf[:, 3:6], tf[:, 6:9] = p0, (p1 - p0).astype(np.float32), (p2 - p0).astype(np.float32)
    return nodes, t


@pytest.mark.parametrize("kind,builder,expect", BUILDERS)
def test_refit_boxes_exact(kind, builder, expect):
    """The refit export is the numpy refit of the pre-update export's topology, with the shared padding rule's pad; an
    update with the unchanged arrays leaves the export and rt_bvh_info byte-identical."""
    s = pyrt.Scene(kind, 24, 24)
    a = s.arrays()
    ctx = pyrt.Context(s, bvh_builder=builder)
    n0, t0 = ctx.bvh_export()
    info0 = bytes(ctx.bvh_info())
    assert ctx.bvh_info().pad == pad_rule(a)
    rep = ctx.update(pos=a["pos"], nrm=a["nrm"])
    assert rep["refitted"] == 1
    n1, t1 = ctx.bvh_export()
    assert np.array_equal(n0, n1) and np.array_equal(t0, t1) and bytes(ctx.bvh_info()) == info0
    pos, nrm = turned(a, 20.0)
    pos[a["vtx_begin"][3]:a["vtx_begin"][4]] *= np.float32(1.5)  # (and grown)
    ctx.update(pos=pos, nrm=nrm)
    pad = pad_rule(dict(a, pos=pos))
    assert ctx.bvh_info().pad == pad
    en, et = numpy_refit(n0, t0, pos, a["tri"], pad)
    n2, t2 = ctx.bvh_export()
    assert np.array_equal(n2, en) and np.array_equal(t2, et)
    assert_frames_equal_oracle(ctx, scene_of(a, pos=pos, nrm=nrm), modes=(pyrt.MODE_PATH,))
    ctx.close()


def scaled(a, f):
    f = np.float32(f)
    lights = a["lights"].copy()
    lights[:, 0:3] *= f
    lights[:, 16] *= f
    return dict(a, pos=a["pos"] * f, lights=lights, camera=a["camera"] * f)


def test_derived_state_follows_scale():
    """lowres updated to x 1e15, x 1e10 and back: rt_bvh_info's pad and flags (short reciprocal forms) are rt_create's for
    each scale and the frames are the oracle's."""
    s = pyrt.Scene("lowres", 24, 24)
    a = s.arrays()
    ctx = pyrt.Context(s)
    flags = set()
    for f in (1e15, 1e10, 1.0):
        b = scaled(a, f) if f != 1.0 else a
        ctx.update(pos=b["pos"], camera=b["camera"], lights=b["lights"])
        t = scene_of(b)
        fresh = pyrt.Context(t)
        assert (ctx.bvh_info().pad, ctx.bvh_info().flags) == (fresh.bvh_info().pad, fresh.bvh_info().flags)
        flags.add(ctx.bvh_info().flags & 1)
        fresh.close()
        assert_frames_equal_oracle(ctx, t, w=16, h=16, spp=2, seed=13, modes=(pyrt.MODE_PATH,), fresh=False, accel=orc.ACCEL_LOOP)
    assert flags == {0, 1}
    ctx.close()


def test_camera_moves():
    """A camera move that enlarges the padding reference refits the boxes, one that does not only moves the camera; rays
    from origins between the old and the new origin bound go through the tree and equal the exhaustive loop."""
    s = pyrt.Scene("lowres", 24, 24)
    a = s.arrays()
    ctx = pyrt.Context(s)
    pad0 = ctx.bvh_info().pad
    near = a["camera"].copy()
    near[0:2] += np.float32(0.1)  # (position and lower-left corner: the whole camera shifts)
    rep = ctx.update(camera=near)
    assert rep["refitted"] == 0 and ctx.bvh_info().pad == pad0
    assert_frames_equal_oracle(ctx, scene_of(a, camera=near), modes=(pyrt.MODE_RAY,))
    far = a["camera"].copy()
    far[0:2, 2] += np.float32(60.0)
    rep = ctx.update(camera=far)
    t = scene_of(a, camera=far)
    assert rep["refitted"] == 1 and ctx.bvh_info().pad == pad_rule(dict(a, camera=far)) > pad0
    assert_frames_equal_oracle(ctx, t, modes=(pyrt.MODE_RAY,))
    # origins beyond rt_create's bound (16 x 2.9) and within the new one (16 x 62.3): towards the scene
    rng = np.random.default_rng(3)
    rays = np.zeros(20000, pyrt.RAY_DTYPE)
    o = rng.normal(size=(len(rays), 3)).astype(np.float32)
    o *= (rng.uniform(60, 900, len(rays)) / np.linalg.norm(o, axis=1)).astype(np.float32)[:, None]
    tgt = rng.uniform(-1, 1, (len(rays), 3)).astype(np.float32)
    rays["origin"], rays["direction"] = o, (tgt - o).astype(np.float32)
    bvh = ctx.trace(rays, pyrt.ACCEL_BVH)
    assert np.array_equal(bvh.view(np.uint8), ctx.trace(rays, pyrt.ACCEL_BRUTE).view(np.uint8))
    assert np.array_equal(bvh[:2000].view(np.uint8), orc.trace(t, rays[:2000]).view(np.uint8))
    assert 0.2 < bvh["hit"].mean()
    ctx.close()


def photon_frame_vs_oracle(ctx, t, nph, seed, w=48, h=40, k=10):
    p = pyrt.make_params(w, h, 2, mode=pyrt.MODE_RAY, seed=3, use_photons=1, k=k, photons_requested=nph)
    _, acc, st = ctx.render(p)
    ref, _, _ = orc.emit_photons(t, nph, pyrt.RNG_PIXEL, seed=seed, math_mode=orc.MATH_DET)
    kd = orc.kd_build(ref)
    _, ref_acc, ref_st = orc.render(t, p, math_mode=orc.MATH_DET, ext_photons=kd, accel=orc.ACCEL_OBVH)
    assert np.array_equal(bits(acc), bits(ref_acc)) and st.knn_queries == ref_st.knn_queries


def test_photon_map_dropped_by_geometry_kept_by_camera():
    s = pyrt.Scene("cubes", 48, 40)
    a = s.arrays()
    ctx = pyrt.Context(s)
    nph = 5000
    ctx.build_photon_map(nph, seed=4)
    photon_frame_vs_oracle(ctx, s, nph, 4)
    pos, nrm = turned(a, 20.0)
    rep = ctx.update(pos=pos, nrm=nrm)
    assert rep["photons_dropped"] == 1
    p = pyrt.make_params(48, 40, 2, mode=pyrt.MODE_RAY, seed=3, use_photons=1, k=10, photons_requested=nph)
    with pytest.raises(pyrt.RtError) as e:
        ctx.render(p)
    assert e.value.code == 5
    t = scene_of(a, pos=pos, nrm=nrm)
    ctx.build_photon_map(nph, seed=4)
    photon_frame_vs_oracle(ctx, t, nph, 4)
    cam = a["camera"].copy()
    cam[0:2, 0] += np.float32(0.15)
    rep = ctx.update(camera=cam)
    assert rep["photons_dropped"] == 0 and rep["refitted"] == 0
    photon_frame_vs_oracle(ctx, scene_of(a, pos=pos, nrm=nrm, camera=cam), nph, 4)
    ctx.close()


def test_materials_and_lights():
    """Changed albedo, a light added and a light removed: the frames are the oracle's."""
    s = pyrt.Scene("lowres", 24, 24)
    a = s.arrays()
    ctx = pyrt.Context(s)
    mats = a["materials"].copy()
    mats[3, 2:5] = [0.9, 0.2, 0.1]  # (rt_material: kd, alpha, albedo[3], f0[3])
    ctx.update(materials=mats)
    assert_frames_equal_oracle(ctx, scene_of(a, materials=mats), fresh=False)
    more = np.concatenate([a["lights"], a["lights"][:1]])
    more[-1, 0:3] = [0.0, 0.9, 0.5]
    ctx.update(lights=more)
    assert_frames_equal_oracle(ctx, scene_of(a, materials=mats, lights=more), fresh=False)
    fewer = a["lights"][1:].copy()
    ctx.update(lights=fewer)
    assert_frames_equal_oracle(ctx, scene_of(a, materials=mats, lights=fewer), fresh=False)
    ctx.close()


def test_rejected_updates_leave_the_context_as_it_was():
    s = pyrt.Scene("lowres", 24, 24)
    a = s.arrays()
    ctx = pyrt.Context(s)
    p = pyrt.make_params(24, 24, 2, seed=9)
    _, before, _ = ctx.render(p)
    n0, t0 = ctx.bvh_export()
    info0 = bytes(ctx.bvh_info())
    pos, nrm = turned(a, 20.0)
    pos[a["tri"][7, 1], 2] = np.nan
    with pytest.raises(pyrt.RtError) as e:
        ctx.update(pos=pos, nrm=nrm, camera=a["camera"] * np.float32(2))
    assert e.value.code == 1 and "non-finite" in str(e.value)
    _, after, _ = ctx.render(p)
    assert np.array_equal(bits(before), bits(after))
    n1, t1 = ctx.bvh_export()
    assert np.array_equal(n0, n1) and np.array_equal(t0, t1) and bytes(ctx.bvh_info()) == info0
    # null arguments
    L = pyrt.amd()
    rep = pyrt.UpdateReport()
    assert L.rt_update(ctx._h, None, C.byref(rep)) == 1
    assert L.rt_update(None, C.byref(pyrt.SceneUpdate()), None) == 1
    u = pyrt.SceneUpdate()
    u.n_lights = 2
    assert L.rt_update(ctx._h, C.byref(u), None) == 1
    assert L.rt_update_vertices_device(None, None, None, None, None) == 1
    assert L.rt_group_update(None, C.byref(pyrt.SceneUpdate()), None) == 1
    _, after, _ = ctx.render(p)
    assert np.array_equal(bits(before), bits(after))
    ctx.close()
    q8 = pyrt.Context(s, node_format=pyrt.NODES_Q8)
    with pytest.raises(pyrt.RtError) as e:
        q8.update(camera=a["camera"])
    assert e.value.code == 4
    q8.close()


def test_device_form_equals_host_form():
    torch = pytest.importorskip("torch")
    s = pyrt.Scene("hires", 24, 24)
    a = s.arrays()
    dev, host = pyrt.Context(s), pyrt.Context(s)
    p = pyrt.make_params(24, 24, 2, seed=17)
    _, before, _ = dev.render(p)
    phi = torch.tensor(np.deg2rad(20.0), dtype=torch.float32, device="cuda:0")
    c, sn = torch.cos(phi), torch.sin(phi)
    pos = torch.from_numpy(a["pos"]).to("cuda:0")
    nrm = torch.from_numpy(a["nrm"]).to("cuda:0")
    b, e = int(a["vtx_begin"][3]), int(a["vtx_begin"][4])
    for t in (pos, nrm):
        x, z = t[b:e, 0].clone(), t[b:e, 2].clone()
        t[b:e, 0], t[b:e, 2] = c * x + sn * z, c * z - sn * x
    stream = torch.cuda.current_stream().cuda_stream
    rep = dev.update_vertices_device(pos.data_ptr(), nrm.data_ptr(), stream)
    assert rep["refitted"] == 1
    hp, hn = pos.cpu().numpy(), nrm.cpu().numpy()
    host.update(pos=hp, nrm=hn)
    _, fd, _ = dev.render(p)
    _, fh, _ = host.render(p)
    assert np.array_equal(bits(fd), bits(fh)) and np.array_equal(dev.bvh_export()[0], host.bvh_export()[0])
    _, ref, _ = orc.render(scene_of(a, pos=hp, nrm=hn), p, math_mode=orc.MATH_DET, accel=orc.ACCEL_OBVH)
    assert np.array_equal(bits(fd), bits(ref))
    # a NaN in the device array is rejected and the frame stays
    bad = pos.clone()
    bad[int(a["tri"][5, 0]), 1] = float("nan")
    with pytest.raises(pyrt.RtError) as err:
        dev.update_vertices_device(bad.data_ptr(), 0, stream)
    assert err.value.code == 1 and "non-finite" in str(err.value)
    _, again, _ = dev.render(p)
    assert np.array_equal(bits(again), bits(fd)) and not np.array_equal(bits(again), bits(before))
    dev.close()
    host.close()


def test_stress_turned_bvh_equals_brute():
    """1 M triangles, slot 3 (the lattice) turned 20 degrees: 200 k rays through the refit tree equal the oracle's (through
    its own CPU BVH of the turned scene), closest and any hit; 20 k of them the exhaustive loop's; a 64 x 64 frame the
    exhaustive loop's."""
    s = pyrt.Scene("stress", 64, 64)
    a = s.arrays()
    ctx = pyrt.Context(s)
    pos, nrm = turned(a, 20.0)
    rep = ctx.update(pos=pos, nrm=nrm)
    assert rep["refitted"] == 1
    print("stress refit: %.2f ms device, %.2f ms in all (build %.1f ms)" % (rep["refit_ms"], rep["total_ms"], ctx.bvh_info().build_ms))
    t = scene_of(a, pos=pos, nrm=nrm)
    rays = ray_batch(t, 200000, 99)
    b = ctx.trace(rays, pyrt.ACCEL_BVH)
    assert np.array_equal(b.view(np.uint8), orc.trace(t, rays, orc.ACCEL_OBVH).view(np.uint8))
    ba = ctx.trace(rays, pyrt.ACCEL_BVH, pyrt.TRACE_ANY)
    assert np.array_equal(ba["hit"], orc.trace(t, rays, orc.ACCEL_OBVH, pyrt.TRACE_ANY)["hit"])
    sub = rays[::10]
    assert np.array_equal(np.ascontiguousarray(b[::10]).view(np.uint8), ctx.trace(sub, pyrt.ACCEL_BRUTE).view(np.uint8))
    assert np.array_equal(ba[::10]["hit"], ctx.trace(sub, pyrt.ACCEL_BRUTE, pyrt.TRACE_ANY)["hit"])
    p = pyrt.make_params(64, 64, 1, mode=pyrt.MODE_PATH, seed=2)
    _, acc, _ = ctx.render(p)
    _, brute, _ = ctx.render(pyrt.make_params(64, 64, 1, mode=pyrt.MODE_PATH, seed=2, accel=pyrt.ACCEL_BRUTE))
    assert np.array_equal(bits(acc), bits(brute))
    ctx.close()


def test_group_update_equals_single_context():
    s = pyrt.Scene("lowres", 32, 32)
    a = s.arrays()
    g = pyrt.Group(s, [0, 0])
    one = pyrt.Context(s)
    pos, nrm = turned(a, 20.0)
    cam = a["camera"].copy()
    cam[0:2, 1] += np.float32(0.05)
    rep = g.update(pos=pos, nrm=nrm, camera=cam)
    assert rep["refitted"] == 1
    one.update(pos=pos, nrm=nrm, camera=cam)
    p = pyrt.make_params(32, 32, 3, seed=21)
    bg = pyrt.background(32, 32)
    go, ga, _ = g.render(p, bg)
    oo, oa, _ = one.render(p, bg)
    assert np.array_equal(bits(ga), bits(oa)) and np.array_equal(bits(go), bits(oo))
    _, ref, _ = orc.render(scene_of(a, pos=pos, nrm=nrm, camera=cam), p, math_mode=orc.MATH_DET)
    assert np.array_equal(bits(ga), bits(ref))
    g.close()
    one.close()


def test_tune_after_update_keeps_oracle_frames():
    s = pyrt.Scene("lowres", 32, 32)
    a = s.arrays()
    ctx = pyrt.Context(s)
    pos, nrm = turned(a, 20.0)
    ctx.update(pos=pos, nrm=nrm)
    ctx.tune(pyrt.make_params(64, 64, 1, mode=pyrt.MODE_PATH, seed=1), 30.0, max_probes=40)
    assert_frames_equal_oracle(ctx, scene_of(a, pos=pos, nrm=nrm), fresh=False)
    # ... and a refit of the tuned tree
    pos2, nrm2 = turned(a, 90.0)
    ctx.update(pos=pos2, nrm=nrm2)
    assert_frames_equal_oracle(ctx, scene_of(a, pos=pos2, nrm=nrm2), fresh=False)
    ctx.close()
