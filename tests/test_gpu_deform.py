"""rt_update, rt_bvh_quality_get and rt_rebuild under real deformation (tests/deform.py): one context per (size, leaf size,
builder) walks the whole pose list, so every refit works on a tree that has been through the poses before it.  After each
update the context must be what rt_create makes of the pose except for the topology: the derived state a fresh context's,
the export the numpy refit of the topology it had (byte for byte), hits and frames the exhaustive loop's and the CPU
oracle's (bit for bit), the cost tests/sah_ref.py's; a rebuild must give a fresh context's tree and keep every frame.  The
sizes are the builders' special cases: n <= leaf_max (two real leaves, or the one triangle twice), 16 (below it the host
builder is forced), 1,024 (up to it the device builder makes one part, above it the hybrid builder has a top)."""
import os

import numpy as np
import pytest

import deform
import orc
import pyrt
import treedigest
from test_gpu_rebuild import assert_quality_is_reference, dbits, info_of
from test_gpu_update import bits, numpy_refit, pad_rule

pytestmark = pytest.mark.gpu

if os.environ.get("RT_NODES") == "q8":
    pytest.skip("RT_NODES=q8 forces one-request node records, and such contexts refuse updates and rebuilds", allow_module_level=True)

N_RAYS = 2048
W = H = 16
SPP = 2
REBUILD_AFTER = ("shuffle", "point", "stray")
DERIVED = ("pad", "flags", "leaf_max", "node_format", "n_tri_records")

CASES = [(n, leaf, b) for n in deform.SIZES for leaf in (1, 2, 3, 8)
         for b in (pyrt.BVH_HOST, pyrt.BVH_DEVICE, pyrt.BVH_HYBRID)
         if b == pyrt.BVH_HOST or (b == pyrt.BVH_DEVICE and n >= 16) or (b == pyrt.BVH_HYBRID and n >= 1025)]
NAMES = {pyrt.BVH_HOST: "host", pyrt.BVH_DEVICE: "device", pyrt.BVH_HYBRID: "hybrid"}


def expected_builder(option, n):
    """rt_create's builder rule (RT_BVH_GPU overrides the option; below 16 triangles the host builder, up to 1,024 the
    hybrid builder has no top and the device builder's own path runs)."""
    want = int(os.environ.get("RT_BVH_GPU", option))
    if want in (pyrt.BVH_DEVICE, pyrt.BVH_HYBRID) and n >= 16:
        return pyrt.BVH_HYBRID if want == pyrt.BVH_HYBRID and n > 1024 else pyrt.BVH_DEVICE
    return pyrt.BVH_HOST


def frame(ctx, mode=pyrt.MODE_PATH, **kw):
    out, acc, st = ctx.render(pyrt.make_params(W, H, SPP, mode=mode, seed=5, **kw), pyrt.background(W, H))
    return out, acc, (st.rays_closest, st.rays_shadow)


def assert_same_frame(got, want, what):
    assert np.array_equal(bits(got[1]), bits(want[1])), "%s: accumulators differ" % what
    assert np.array_equal(bits(got[0]), bits(want[0])), "%s: images differ" % what
    assert got[2] == want[2], "%s: ray counts differ" % what


def assert_frames_are_the_oracles(ctx, s, name):
    """Check 4: the pooled, the sequential and the wavefront schedule against the oracle's exhaustive loop."""
    bg = pyrt.background(W, H)
    modes = (pyrt.MODE_PATH, pyrt.MODE_RAY) if name == "shuffle" else (pyrt.MODE_PATH,)
    first = None
    for mode in modes:
        p = pyrt.make_params(W, H, SPP, mode=mode, seed=5)
        out, acc, st = orc.render(s, p, math_mode=orc.MATH_DET, bg=bg, accel=orc.ACCEL_LOOP)
        ref = (out, acc, (st.rays_closest, st.rays_shadow))
        for kw in (({}, dict(no_pool=True), dict(wavefront=True)) if mode == pyrt.MODE_PATH else ({},)):
            got = frame(ctx, mode, **kw)
            assert_same_frame(got, ref, "%s mode %d %s" % (name, mode, kw))
            first = first or got
    if name in deform.DEGENERATE:
        assert np.array_equal(bits(first[0]), bits(bg))
    return first


def assert_hits_are_exact(ctx, s, a, name):
    """Check 3: closest and any hits through the tree, the exhaustive loop and the oracle; the stream form on the same rays."""
    import torch
    r = deform.rays(a, N_RAYS, 11)
    ref = orc.trace(s, r)
    hc = ctx.trace(r, pyrt.ACCEL_BVH)
    assert np.array_equal(hc.view(np.uint8), ref.view(np.uint8)), "%s: closest hits through the tree differ from the oracle's" % name
    assert np.array_equal(ctx.trace(r, pyrt.ACCEL_BRUTE).view(np.uint8), ref.view(np.uint8)), name
    ref_any = orc.trace(s, r, orc.ACCEL_LOOP, pyrt.TRACE_ANY)["hit"]
    ha = ctx.trace(r, pyrt.ACCEL_BVH, pyrt.TRACE_ANY)
    assert np.array_equal(ha["hit"], ref_any) and np.array_equal(ctx.trace(r, pyrt.ACCEL_BRUTE, pyrt.TRACE_ANY)["hit"], ref_any), name
    assert np.array_equal(ref_any, ref["hit"])
    frac = hc["hit"].mean()
    if name in deform.DEGENERATE:
        assert frac == 0, name
    else:
        assert frac >= 0.5, (name, frac)
    # rt_trace_stream_device, mixed kinds (tests/test_gpu_parity_big.py test_ray_stream_kernel_equals_rt_trace)
    n = len(r)
    anyk = (np.arange(n) % 4) != 3
    O = np.zeros((n, 4), np.float32)
    D = np.zeros((n, 4), np.float32)
    O[:, 0:3], D[:, 0:3] = r["origin"], r["direction"]
    O[:, 3] = anyk.astype(np.uint32).view(np.float32)
    dO, dD = torch.from_numpy(O).cuda(), torch.from_numpy(D).cuda()
    res = torch.full((n, 2), 7, dtype=torch.int32, device="cuda")
    ctx.trace_stream_device(dO.data_ptr(), dD.data_ptr(), n, res.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = res.cpu().numpy().view(np.uint32)
    assert np.array_equal(got[anyk, 0], ha["hit"][anyk].astype(np.uint32)) and (got[anyk, 1] == 0).all(), name
    c = ~anyk
    hit = hc["hit"] == 1
    gid = a["tri_begin"][np.where(hit, hc["mesh"], 0)] + hc["tri"]
    assert np.array_equal(got[c & hit, 0], hc["d"][c & hit].view(np.uint32)) and np.array_equal(got[c & hit, 1], gid[c & hit]), name
    assert (got[c & ~hit] == 0xFFFFFFFF).all(), name
    return frac


def assert_no_zero_plane(nodes):
    planes = nodes[:, 0:12]
    assert ((planes & 0x7FFFFFFF) != 0).all(), "a box plane is a zero"


@pytest.mark.parametrize("n,leaf,builder", CASES, ids=["n%d-leaf%d-%s" % (n, leaf, NAMES[b]) for n, leaf, b in CASES])
def test_pose_walk(n, leaf, builder):
    a = deform.scene(n, 100 + n)
    opts = dict(bvh_leaf_max=leaf, bvh_builder=builder)
    want_builder = expected_builder(builder, n)
    ctx = pyrt.Context(deform.array_scene(a), **opts)
    bi = ctx.bvh_info()
    assert bi.builder == want_builder and bi.leaf_max == leaf and bi.n_tri_records == n
    E0 = ctx.bvh_export()
    shape0 = (bi.n_nodes, bi.max_depth)
    cnt = ((~E0[0][:, 12:14].view(np.int32)) & 7) + 1
    assert cnt[E0[0][:, 12:14].view(np.int32) < 0].max() <= leaf
    cost0 = ctx.bvh_quality()["cost"]
    refits = 0
    for name, pose in deform.poses(a, 7):
        b = dict(a, **pose)
        s = deform.array_scene(b)
        rep = ctx.update(**pose)
        refits += 1
        # 1. the report and the derived state
        assert rep["refitted"] == 1 and rep["photons_dropped"] == 0, name
        fresh = pyrt.Context(s, **opts)
        got, ref = info_of(ctx), info_of(fresh)
        assert {k: got[k] for k in DERIVED} == {k: ref[k] for k in DERIVED}, name
        assert got["builder"] == ref["builder"] == want_builder, name
        fresh.close()
        pad = pad_rule(b)
        assert ctx.bvh_info().pad == pad and (got["n_nodes"], got["max_depth"]) == shape0, name
        # 2. boxes and records
        want_n, want_t = numpy_refit(E0[0], E0[1], b["pos"], b["tri"], pad)
        got_n, got_t = ctx.bvh_export()
        assert np.array_equal(got_t, want_t), "%s: triangle records differ from the numpy refit" % name
        assert np.array_equal(got_n, want_n), "%s: boxes differ from the numpy refit" % name
        if name == "origin":
            assert_no_zero_plane(got_n)
        # 3. hits, 4. frames
        assert_hits_are_exact(ctx, s, b, name)
        shown = assert_frames_are_the_oracles(ctx, s, name)
        # 5. quality
        q = assert_quality_is_reference(ctx)
        assert q["refits"] == refits and dbits(q["cost_built"]) == dbits(cost0), name
        assert q["ratio"] == q["cost"] / q["cost_built"], name
        # 6. the finiteness rule's other side: the same NaN in a vertex a triangle references
        if name == "stray":
            bad = pose["pos"].copy()
            bad[b["tri"][n // 2, 1]] = pose["pos"][-2]
            info0 = bytes(ctx.bvh_info())
            with pytest.raises(pyrt.RtError) as e:
                ctx.update(**dict(pose, pos=bad))
            assert e.value.code == 1 and "non-finite" in str(e.value)
            n1, t1 = ctx.bvh_export()
            assert np.array_equal(n1, got_n) and np.array_equal(t1, got_t) and bytes(ctx.bvh_info()) == info0
            assert_same_frame(frame(ctx), shown, "after the rejected update")
            assert ctx.bvh_quality()["refits"] == refits
        if name in REBUILD_AFTER:
            rr = ctx.rebuild()
            fresh = pyrt.Context(s, **opts)
            assert rr["rebuilt"] == 1 and rr["builder"] == want_builder == fresh.bvh_info().builder, name
            assert treedigest.context_digest(ctx) == treedigest.context_digest(fresh), "%s: the rebuilt tree is not rt_create's" % name
            assert info_of(ctx) == info_of(fresh) and ctx.bvh_info().pad == pad, name
            q, qf = ctx.bvh_quality(), fresh.bvh_quality()
            assert dbits(rr["cost_after"]) == dbits(q["cost"]) == dbits(qf["cost"]) == dbits(q["cost_built"]), name
            assert q["ratio"] == 1.0 and q["refits"] == 0, name
            fresh.close()
            assert_same_frame(frame(ctx), shown, "%s: after the rebuild" % name)
            # the poses after this one refit the rebuilt tree
            E0 = ctx.bvh_export()
            bi = ctx.bvh_info()
            shape0 = (bi.n_nodes, bi.max_depth)
            cost0, refits = q["cost"], 0
    ctx.close()


@pytest.mark.parametrize("n,builder", [(17, pyrt.BVH_DEVICE), (1025, pyrt.BVH_HYBRID)])
def test_long_chain(n, builder):
    """48 updates, each the previous pose plus N(0, 0.05) noise: the refit depends on the last pose only and the baseline
    cost stays the built tree's."""
    a = deform.scene(n, 100 + n)
    opts = dict(bvh_leaf_max=2, bvh_builder=builder)
    ctx, once = pyrt.Context(deform.array_scene(a), **opts), pyrt.Context(deform.array_scene(a), **opts)
    assert ctx.bvh_info().builder == expected_builder(builder, n)
    E0 = ctx.bvh_export()
    cost0 = ctx.bvh_quality()["cost"]
    rng = np.random.default_rng(48)
    pos = a["pos"]
    for _ in range(48):
        pos = (pos + rng.normal(0.0, 0.05, pos.shape).astype(np.float32)).astype(np.float32)
        assert ctx.update(pos=pos)["refitted"] == 1
    final = dict(a, pos=pos)
    want_n, want_t = numpy_refit(E0[0], E0[1], pos, a["tri"], pad_rule(final))
    got_n, got_t = ctx.bvh_export()
    assert np.array_equal(got_t, want_t) and np.array_equal(got_n, want_n)
    assert once.update(pos=pos)["refitted"] == 1
    n1, t1 = once.bvh_export()
    assert np.array_equal(n1, got_n) and np.array_equal(t1, got_t)
    q, q1 = assert_quality_is_reference(ctx), once.bvh_quality()
    assert dbits(q["cost"]) == dbits(q1["cost"]) and info_of(ctx) == info_of(once)
    assert q["refits"] == 48 and q1["refits"] == 1 and dbits(q["cost_built"]) == dbits(cost0) == dbits(q1["cost_built"])
    ctx.close()
    once.close()
