"""rt_bvh_quality_get and rt_rebuild: the surface-area cost of the resident tree against tests/sah_ref.py, and the tree built
again in place — a rebuilt context is compared with a freshly created one of the same description (tree digest, rt_bvh_info,
cost, frames against the CPU oracle), and with itself before the rebuild for everything a rebuild must keep."""
import ctypes as C

import numpy as np
import pytest

import pyrt
import sah_ref
import transform_ref as xf
import treedigest
from test_gpu_update import BUILDERS, assert_frames_equal_oracle, bits, numpy_refit, pad_rule, scene_of, turned

pytestmark = pytest.mark.gpu


def dbits(x):
    return np.float64(x).view(np.uint64)


def grown(a, deg=20.0):
    """Slot 3 turned by deg about y and scaled by 1.5 (test_refit_boxes_exact's pose)."""
    pos, nrm = turned(a, deg)
    pos[a["vtx_begin"][3]:a["vtx_begin"][4]] *= np.float32(1.5)
    return pos, nrm


def info_of(ctx):
    bi = ctx.bvh_info()
    return {n: getattr(bi, n) for n, _ in bi._fields_ if n != "build_ms"}


def assert_quality_is_reference(ctx):
    """cost, nodes and tris against sah_ref over the export, within 2 * n_slots * 2^-53 relative: the worst case of a
    float64 sum of n_slots non-negative terms in any order against the exact sum.  Returns the quality dict."""
    q = ctx.bvh_quality()
    ref = sah_ref.cost(ctx.bvh_export()[0])
    tol = 2.0 * ref["n_slots"] * 2.0 ** -53
    for k in ("cost", "nodes", "tris"):
        err = abs(q[k] - ref[k]) / ref[k]
        print("%s: device %.17g reference %.17g relative error %.3g (allowed %.3g)" % (k, q[k], ref[k], err, tol))
        assert err <= tol, k
    assert q["n_nodes"] == ref["n_slots"] // 2 == ctx.bvh_info().n_nodes
    again = ctx.bvh_quality()
    assert all(dbits(q[k]) == dbits(again[k]) for k in ("cost", "nodes", "tris", "cost_built", "ratio"))
    return q


@pytest.mark.parametrize("kind,builder,expect", BUILDERS)
def test_quality_equals_reference(kind, builder, expect):
    s = pyrt.Scene(kind, 24, 24)
    a = s.arrays()
    ctx = pyrt.Context(s, bvh_builder=builder)
    assert ctx.bvh_info().builder == expect
    q0 = assert_quality_is_reference(ctx)
    assert q0["ratio"] == 1.0 and q0["refits"] == 0 and dbits(q0["cost_built"]) == dbits(q0["cost"])
    pos, nrm = grown(a)
    ctx.update(pos=pos, nrm=nrm)
    q1 = assert_quality_is_reference(ctx)
    assert q1["refits"] == 1 and dbits(q1["cost_built"]) == dbits(q0["cost"])
    assert q1["ratio"] == q1["cost"] / q1["cost_built"] and q1["cost"] != q0["cost"]
    ctx.close()
    # the baseline taken by the update itself (no quality call before it), and an update with the unchanged arrays
    ctx = pyrt.Context(s, bvh_builder=builder)
    ctx.update(pos=a["pos"], nrm=a["nrm"])
    q = ctx.bvh_quality()
    assert q["refits"] == 1 and dbits(q["cost"]) == dbits(q["cost_built"]) == dbits(q0["cost"]) and q["ratio"] == 1.0
    ctx.close()


@pytest.mark.parametrize("kind,builder,expect", BUILDERS)
def test_rebuilt_context_is_a_created_one(kind, builder, expect):
    s = pyrt.Scene(kind, 24, 24)
    a = s.arrays()
    ctx = pyrt.Context(s, bvh_builder=builder)
    pos, nrm = grown(a)
    ctx.update(pos=pos, nrm=nrm)
    refit_digest = treedigest.context_digest(ctx)
    rep = ctx.rebuild()
    t = scene_of(a, pos=pos, nrm=nrm)
    fresh = pyrt.Context(t, bvh_builder=builder)
    assert rep["rebuilt"] == 1 and rep["builder"] == expect == fresh.bvh_info().builder
    assert rep["ratio_before"] > 0 and rep["build_ms"] > 0 and rep["total_ms"] >= rep["build_ms"]
    digest = treedigest.context_digest(ctx)
    assert digest == treedigest.context_digest(fresh)
    assert digest != refit_digest, "the rebuild kept the refit tree's topology"
    assert info_of(ctx) == info_of(fresh) and ctx.bvh_info().pad == pad_rule(dict(a, pos=pos))
    q, qf = ctx.bvh_quality(), fresh.bvh_quality()
    assert dbits(rep["cost_after"]) == dbits(q["cost"]) == dbits(qf["cost"])
    assert q["ratio"] == 1.0 and q["refits"] == 0 and dbits(q["cost_built"]) == dbits(q["cost"])
    if expect == pyrt.BVH_HOST:
        for got, ref in zip(ctx.bvh_export(), fresh.bvh_export()):
            assert np.array_equal(got, ref)
    p = pyrt.make_params(24, 24, 3, mode=pyrt.MODE_PATH, seed=5)
    assert np.array_equal(bits(ctx.render(p)[1]), bits(fresh.render(p)[1]))
    fresh.close()
    assert_frames_equal_oracle(ctx, t)
    ctx.close()


@pytest.mark.parametrize("kind,builder,expect", BUILDERS)
def test_frames_do_not_move(kind, builder, expect):
    s = pyrt.Scene(kind, 24, 24)
    a = s.arrays()
    ctx = pyrt.Context(s, bvh_builder=builder)
    pos, nrm = grown(a)
    ctx.update(pos=pos, nrm=nrm)
    p = pyrt.make_params(24, 24, 3, mode=pyrt.MODE_PATH, seed=11)
    bg = pyrt.background(24, 24)
    frames = [ctx.render(p, bg)]
    for _ in range(2):
        assert ctx.rebuild()["rebuilt"] == 1
        frames.append(ctx.render(p, bg))
    for out, acc, st in frames[1:]:
        assert np.array_equal(bits(acc), bits(frames[0][1])) and np.array_equal(bits(out), bits(frames[0][0]))
        assert (st.rays_closest, st.rays_shadow) == (frames[0][2].rays_closest, frames[0][2].rays_shadow)
    ctx.close()


@pytest.mark.parametrize("kind,builder,expect", BUILDERS)
def test_threshold(kind, builder, expect):
    """min_ratio is a float32 field compared with the float64 ratio r, so the two sharpest thresholds are float32
    neighbours: the largest float32 <= max(r, 1) must rebuild (ratio_before == r), the next float32 above it — the least
    representable threshold > r — must not.  No ratio is assumed for these scenes; r is printed."""
    s = pyrt.Scene(kind, 24, 24)
    a = s.arrays()
    ctx = pyrt.Context(s, bvh_builder=builder)
    pos, nrm = turned(a, 20.0)
    ctx.update(pos=pos, nrm=nrm)
    r = ctx.bvh_quality()["ratio"]
    print("%s builder %d: ratio after the 20 degree refit %.17g" % (kind, expect, r))
    at = np.float32(max(r, 1.0))
    if float(at) > max(r, 1.0):
        at = np.nextafter(at, np.float32(-np.inf))
    above = np.nextafter(at, np.float32(np.inf))
    assert float(at) <= max(r, 1.0) < float(above)
    n0, t0 = ctx.bvh_export()
    if r >= 1.0:
        rep = ctx.rebuild(min_ratio=float(above))
        assert rep["rebuilt"] == 0 and rep["ratio_before"] == r and rep["builder"] == 0 and rep["cost_after"] == 0.0
        n1, t1 = ctx.bvh_export()
        assert np.array_equal(n0, n1) and np.array_equal(t0, t1)
        q = ctx.bvh_quality()
        assert q["ratio"] == r and q["refits"] == 1
        rep = ctx.rebuild(min_ratio=float(at))
    else:
        rep = ctx.rebuild(min_ratio=0.0)
    assert rep["rebuilt"] == 1 and rep["ratio_before"] == r and rep["builder"] == expect
    q = ctx.bvh_quality()
    assert q["ratio"] == 1.0 and q["refits"] == 0
    ctx.close()


def test_rebuild_keeps_the_photon_map():
    s = pyrt.Scene("cubes", 48, 40)
    a = s.arrays()
    ctx = pyrt.Context(s)
    nph = 5000
    n, _ = ctx.build_photon_map(nph, seed=4)
    cam = a["camera"].copy()
    cam[0:2, 0] += np.float32(0.15)
    assert ctx.update(camera=cam)["photons_dropped"] == 0
    p = pyrt.make_params(48, 40, 2, mode=pyrt.MODE_RAY, seed=3, use_photons=1, k=10, photons_requested=nph)
    _, before, st0 = ctx.render(p)
    ph0 = ctx.get_photons(n)
    assert ctx.rebuild()["rebuilt"] == 1
    _, after, st1 = ctx.render(p)
    assert np.array_equal(bits(before), bits(after)) and st0.knn_queries == st1.knn_queries > 0
    for x, y in zip(ph0, ctx.get_photons(n)):
        assert len(x) == n and np.array_equal(bits(x), bits(y))
    ctx.close()


def records_by_id(ctx):
    """The triangle records (p0, e1, e2, id, mesh) in id order: the context's positions as its triangles see them,
    whatever the tree."""
    t = ctx.bvh_export()[1]
    return t[np.argsort(t[:, 9], kind="stable")]


@pytest.mark.parametrize("kind,builder,expect", BUILDERS)
def test_rebuild_keeps_the_rest_pose(kind, builder, expect):
    s = pyrt.Scene(kind, 24, 24)
    a = s.arrays()
    ctx, other = pyrt.Context(s, bvh_builder=builder), pyrt.Context(s, bvh_builder=builder)
    t1 = xf.set_mesh(pyrt.make_transforms(5), 3, xf.rotation_y(20.0))
    t2 = xf.set_mesh(pyrt.make_transforms(5), 3, xf.rotation_y(65.0))
    ctx.update_transforms(t1)
    other.update_transforms(t1)
    assert ctx.rebuild()["rebuilt"] == 1
    ctx.update_transforms(t2)
    other.update_transforms(t2)
    assert np.array_equal(records_by_id(ctx), records_by_id(other))
    pos, nrm = xf.apply(a, t2)  # (from the ORIGINAL rest pose: a rest pose retaken after the rebuild would compound the turns)
    fresh = pyrt.Context(scene_of(a, pos=pos, nrm=nrm), bvh_builder=builder)
    assert np.array_equal(records_by_id(ctx), records_by_id(fresh))
    fresh.close()
    for mode in (pyrt.MODE_PATH, pyrt.MODE_RAY):
        p = pyrt.make_params(24, 24, 3, mode=mode, seed=7)
        assert np.array_equal(bits(ctx.render(p)[1]), bits(other.render(p)[1]))
    assert ctx.bvh_quality()["refits"] == 1 and other.bvh_quality()["refits"] == 2
    ctx.close()
    other.close()


@pytest.mark.parametrize("kind,builder,expect", BUILDERS)
def test_refit_of_the_rebuilt_tree(kind, builder, expect):
    s = pyrt.Scene(kind, 24, 24)
    a = s.arrays()
    ctx = pyrt.Context(s, bvh_builder=builder)
    pos, nrm = grown(a)
    ctx.update(pos=pos, nrm=nrm)
    rep = ctx.rebuild()
    n0, t0 = ctx.bvh_export()
    pos2, nrm2 = turned(a, 90.0)
    assert ctx.update(pos=pos2, nrm=nrm2)["refitted"] == 1
    en, et = numpy_refit(n0, t0, pos2, a["tri"], pad_rule(dict(a, pos=pos2)))
    n1, t1 = ctx.bvh_export()
    assert np.array_equal(n1, en) and np.array_equal(t1, et)
    q = ctx.bvh_quality()
    assert q["refits"] == 1 and dbits(q["cost_built"]) == dbits(rep["cost_after"])
    assert_frames_equal_oracle(ctx, scene_of(a, pos=pos2, nrm=nrm2), seed=90)
    ctx.close()


def test_refusals():
    s = pyrt.Scene("lowres", 24, 24)
    a = s.arrays()
    L = pyrt.amd()
    q8 = pyrt.Context(s, node_format=pyrt.NODES_Q8)
    for call in (q8.bvh_quality, q8.rebuild):
        with pytest.raises(pyrt.RtError) as e:
            call()
        assert e.value.code == 4
    q8.close()
    ctx = pyrt.Context(s)
    pos, nrm = turned(a, 20.0)
    ctx.update(pos=pos, nrm=nrm)
    n0, t0 = ctx.bvh_export()
    info0 = bytes(ctx.bvh_info())
    for bad in (0.5, float("nan"), float("inf"), -2.0):
        with pytest.raises(pyrt.RtError) as e:
            ctx.rebuild(min_ratio=bad)
        assert e.value.code == 1 and "min_ratio" in str(e.value)
    p = pyrt.RebuildParams()
    p.reserved[3] = 1
    assert L.rt_rebuild(ctx._h, C.byref(p), None) == 1
    assert L.rt_bvh_quality_get(ctx._h, None) == 1
    n1, t1 = ctx.bvh_export()
    assert np.array_equal(n0, n1) and np.array_equal(t0, t1) and bytes(ctx.bvh_info()) == info0
    # NULL parameters = always, no report
    assert L.rt_rebuild(ctx._h, None, None) == 0
    assert ctx.bvh_quality()["refits"] == 0
    ctx.close()
