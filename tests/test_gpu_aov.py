"""rt_render_aov: the first-hit AOVs of a frame's primary rays, bit for bit against the CPU restatement (tests/aov_ref.py:
the oracle's own primary rays and hits, Renderer.cpp:42-43 in float32, float32 sums in sample order) on every scene,
size, sample range, accelerator and tree builder; hits against the frame's own primary-hit count; mesh and tri against
rt_trace; the device form, NULL channels, a refit scene and the error codes."""
import ctypes as C

import numpy as np
import pytest

import aov_ref
import orc
import pyrt

pytestmark = pytest.mark.gpu

CHANNELS = pyrt.AOV_CHANNELS
RANGES = [dict(spp=1), dict(spp=4), dict(spp=7), dict(spp=7, spp_begin=3, spp_count=4)]
_ref_cache = {}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_aov_equal(got, exp, what=""):
    for k in CHANNELS:
        assert got[k].shape == exp[k].shape, (what, k)
        assert np.array_equal(bits(got[k]), bits(exp[k])), "%s: channel %s differs at %d pixels" % (
            what, k, int(np.any((bits(got[k]) != bits(exp[k])).reshape(got[k].shape[0], got[k].shape[1], -1), axis=2).sum()))


def oracle_accel(kind):
    return orc.ACCEL_OBVH if kind in ("hires", "stress") else orc.ACCEL_LOOP


def reference(kind, w, h, rng):
    key = (kind, w, h, tuple(sorted(rng.items())))
    if key not in _ref_cache:
        s = pyrt.Scene(kind, w, h)
        _ref_cache[key] = aov_ref.aov_sums(s, pyrt.make_params(w, h, seed=11, mode=pyrt.MODE_PATH, **rng), accel=oracle_accel(kind))
    return _ref_cache[key]


@pytest.mark.parametrize("accel", [pyrt.ACCEL_BVH, pyrt.ACCEL_BRUTE], ids=["bvh", "brute"])
@pytest.mark.parametrize("rng", RANGES, ids=["spp1", "spp4", "spp7", "spp7_3+4"])
@pytest.mark.parametrize("w,h", [(64, 48), (37, 23)])
@pytest.mark.parametrize("kind", ["cubes", "lowres", "hires"])
def test_aov_bit_exact(kind, w, h, rng, accel):
    s = pyrt.Scene(kind, w, h)
    ctx = pyrt.Context(s)
    got = ctx.render_aov(pyrt.make_params(w, h, seed=11, mode=pyrt.MODE_PATH, accel=accel, **rng), raw=True)
    assert_aov_equal(got, reference(kind, w, h, rng), "%s %dx%d %s accel %d" % (kind, w, h, rng, accel))
    ctx.close()


@pytest.mark.parametrize("builder,node_format,expect", [
    (pyrt.BVH_HOST, pyrt.NODES_AUTO, pyrt.BVH_HOST), (pyrt.BVH_DEVICE, pyrt.NODES_AUTO, pyrt.BVH_DEVICE),
    (pyrt.BVH_HOST, pyrt.NODES_Q8, pyrt.BVH_HOST)], ids=["host", "device", "host_q8"])
def test_aov_tree_builders_and_q8(builder, node_format, expect):
    """Host- and device-built trees give the restatement's AOVs; RT_NODES_Q8 contexts run the pass (on their resident
    32-byte records) with the same result."""
    rng = dict(spp=4)
    s = pyrt.Scene("hires", 64, 48)
    ctx = pyrt.Context(s, bvh_builder=builder, node_format=node_format)
    info = ctx.bvh_info()
    assert info.builder == expect
    if node_format == pyrt.NODES_Q8:
        assert info.node_format == pyrt.NODES_Q8
    got = ctx.render_aov(pyrt.make_params(64, 48, seed=11, mode=pyrt.MODE_PATH, **rng), raw=True)
    assert_aov_equal(got, reference("hires", 64, 48, rng), "builder %d" % builder)
    ctx.close()


def test_hits_equal_the_frames_primary_hit_count():
    """The pass casts the frame's own primary rays: hits == the w channel of rt_render's accumulator (C1: cubes 256x256,
    8 spp, path mode)."""
    s = pyrt.Scene("cubes", 256, 256)
    ctx = pyrt.Context(s)
    p = pyrt.make_params(256, 256, 8, mode=pyrt.MODE_PATH, seed=1)
    _, acc, _ = ctx.render(p)
    a = ctx.render_aov(p)
    assert np.array_equal(a["hits"].astype(np.float32), acc[..., 3])
    ctx.close()


@pytest.mark.parametrize("kind", ["cubes", "lowres", "hires"])
def test_mesh_and_tri_equal_rt_trace(kind):
    """mesh / tri are rt_trace's answer for the rays of sample spp_begin."""
    w, h = 37, 23
    s = pyrt.Scene(kind, w, h)
    ctx = pyrt.Context(s)
    p = pyrt.make_params(w, h, 7, mode=pyrt.MODE_PATH, seed=5, spp_begin=3, spp_count=4)
    rays = aov_ref.primary_rays(s, p)[:, :, 0]
    th = ctx.trace(rays.reshape(-1)).reshape(h, w)
    a = ctx.render_aov(p, channels=("mesh", "tri"))
    assert np.array_equal(a["mesh"], np.where(th["hit"] != 0, th["mesh"], aov_ref.MISS))
    assert np.array_equal(a["tri"], np.where(th["hit"] != 0, th["tri"], aov_ref.MISS))
    ctx.close()


def test_device_form_and_null_channels():
    """rt_render_aov_device into torch tensors equals the host form bit for bit; NULL channels are skipped and leave the
    others unchanged."""
    import torch
    w, h = 64, 48
    s = pyrt.Scene("lowres", w, h)
    ctx = pyrt.Context(s)
    p = pyrt.make_params(w, h, 7, mode=pyrt.MODE_PATH, seed=2, spp_begin=1, spp_count=5)
    host = ctx.render_aov(p, raw=True)
    dev = {k: torch.full((h, w, 3) if k in pyrt.AOV_FLOAT3 else (h, w), -7,
                         dtype=torch.float32 if k in pyrt.AOV_FLOAT3 + ("depth",) else torch.int32, device="cuda")
           for k in CHANNELS}
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream()
    ctx.render_aov_device(p, {k: v.data_ptr() for k, v in dev.items()}, stream.cuda_stream)
    stream.synchronize()
    got = {k: v.cpu().numpy() for k, v in dev.items()}
    assert_aov_equal({k: v.view(host[k].dtype) for k, v in got.items()}, host, "device form")
    # only some channels: the others untouched on the device, the given ones unchanged
    part = {k: torch.full_like(v, 3) for k, v in dev.items()}
    torch.cuda.synchronize()
    ctx.render_aov_device(p, {"normal": part["normal"].data_ptr(), "tri": part["tri"].data_ptr()}, 0)
    torch.cuda.synchronize()
    for k, v in part.items():
        if k in ("normal", "tri"):
            assert np.array_equal(bits(v.cpu().numpy()), bits(host[k]))
        else:
            assert bool((v == 3).all()), k
    sub = ctx.render_aov(p, raw=True, channels=("albedo", "hits"))
    assert sorted(sub) == ["albedo", "hits"]
    for k in sub:
        assert np.array_equal(bits(sub[k]), bits(host[k]))
    ctx.close()


def test_means_are_sums_over_hits():
    s = pyrt.Scene("cubes", 37, 23)
    ctx = pyrt.Context(s)
    p = pyrt.make_params(37, 23, 4, seed=3)
    raw, mean = ctx.render_aov(p, raw=True), ctx.render_aov(p)
    assert np.array_equal(raw["hits"], mean["hits"]) and np.array_equal(raw["mesh"], mean["mesh"])
    hit = raw["hits"] > 0
    n = raw["hits"][hit].astype(np.float32)
    assert np.array_equal(mean["albedo"][hit], raw["albedo"][hit] / n[:, None])
    assert np.array_equal(mean["depth"][hit], raw["depth"][hit] / n)
    assert not mean["normal"][~hit].any()
    ctx.close()


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


@pytest.mark.parametrize("kind", ["lowres", "hires"])
def test_after_update_equals_a_fresh_context(kind):
    """After rt_update turns slot 3, the AOVs are those of a fresh context of the turned scene (and the restatement's)."""
    w, h = 64, 48
    s = pyrt.Scene(kind, w, h)
    a = s.arrays()
    ctx = pyrt.Context(s)
    p = pyrt.make_params(w, h, 4, mode=pyrt.MODE_PATH, seed=9)
    before = ctx.render_aov(p, raw=True)
    pos, nrm = turned(a, 30.0)
    ctx.update(pos=pos, nrm=nrm)
    moved = pyrt.ArrayScene(pos, nrm, a["tri"], a["tri_begin"], a["vtx_begin"], a["materials"], a["lights"], a["camera"])
    fresh = pyrt.Context(moved)
    got, exp = ctx.render_aov(p, raw=True), fresh.render_aov(p, raw=True)
    assert_aov_equal(got, exp, "after rt_update")
    assert not np.array_equal(bits(got["position"]), bits(before["position"]))
    assert_aov_equal(got, aov_ref.aov_sums(moved, p, accel=oracle_accel(kind)), "after rt_update vs restatement")
    fresh.close()
    ctx.close()


def test_error_codes():
    L = pyrt.amd()
    s = pyrt.Scene("cubes", 16, 16)
    ctx = pyrt.Context(s)
    hits = np.zeros((16, 16), np.uint32)
    a = pyrt.Aov()
    a.hits = hits.ctypes.data

    def rc(ctx_h, **kw):
        p = pyrt.make_params(16, 16, 4)
        for k, v in kw.items():
            setattr(p, k, v)
        return L.rt_render_aov(ctx_h, C.byref(p), C.byref(a))
    assert rc(None) == 1
    assert rc(ctx._h, world=2) == 4
    assert rc(ctx._h, world=2, rank=3) == 1
    assert rc(ctx._h, width=0) == 1
    assert rc(ctx._h, spp_begin=2, spp_count=3) == 1
    assert rc(ctx._h, spp=0) == 1
    assert L.rt_render_aov(ctx._h, None, C.byref(a)) == 1
    assert L.rt_render_aov(ctx._h, C.byref(pyrt.make_params(16, 16, 4)), None) == 1
    assert L.rt_render_aov_device(None, C.byref(pyrt.make_params(16, 16, 4)), C.byref(a), None) == 1
    # the fields that do not affect the pass: photon shading without a photon map, any mode and depth
    assert rc(ctx._h, use_photons=1, k=5, photons_requested=100, mode=7, max_depth=9) == 0
    assert rc(ctx._h) == 0 and hits.max() > 0
    ctx.close()


def test_stress_scene_deep_tree():
    """The 1 M-triangle stress scene (the deep tree's stack) at 128x128, 1 spp, against the restatement over the oracle's
    own BVH."""
    w = h = 128
    s = pyrt.Scene("stress", w, h)
    ctx = pyrt.Context(s)
    p = pyrt.make_params(w, h, 1, mode=pyrt.MODE_PATH, seed=4)
    assert_aov_equal(ctx.render_aov(p, raw=True), aov_ref.aov_sums(s, p, accel=orc.ACCEL_OBVH), "stress")
    ctx.close()
