"""What produces the photon map on the device — k_emit, k_photon_compact, k_photon_gather and the host code around
them in rt_emit_photons / rt_build_photon_map — against the oracle, bit for bit, on the cases of
tests/photon_cases.py: every light count from 1 to 5, slot counts from 0 and 1 across the wave and the compaction's
1,024-thread chunk edges, each of emission's exits on a scene known to reach it (tests/test_photon_cases_cpu.py),
maps of one, two and three photons built by the device and rendered, the other tree forms, and the ABI's edges.

A one-line slip each test is there to catch: the light taken from j % perLight or the weight from a fixed light
count (emission over light counts); per = n / 1024, a dropped last chunk or an exclusive scan off by one thread
(compaction); a photon stored at the 20-cast cap, or a dropped miss-after-bounce photon (exits); a gather that
reads slot i instead of the item's source slot (any map whose kd order is not the emission order)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import orc
import photon_cases as pc
import pyrt

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@functools.lru_cache(maxsize=None)
def scene(name, w=40, h=32):
    return pc.scene(name, w, h)


@functools.lru_cache(maxsize=None)
def oracle(name, n, seed):
    """(photons [m][7] in emission order, the same in kd order, emission rays) — computed once, shared, read-only."""
    ph, _, rays = orc.emit_photons(scene(name), n, pyrt.RNG_PIXEL, seed=seed, math_mode=orc.MATH_DET)
    kd = orc.kd_build(ph)
    ph.setflags(write=False)
    kd.setflags(write=False)
    return ph, kd, rays


@pytest.fixture(scope="module")
def ctxs():
    """One context per scene name (and form), created on first use and reused across requests."""
    made = {}

    def get(name, **form):
        key = (name,) + tuple(sorted(form.items()))
        if key not in made:
            made[key] = pyrt.Context(scene(name), **form)
        return made[key]
    yield get
    for c in made.values():
        c.close()


def assert_emission(ctx, name, n, seed):
    """ctx.emit_photons == the oracle's list: count, order, positions, directions, weights."""
    ref, _, _ = oracle(name, n, seed)
    pos, dir_, wt = ctx.emit_photons(n, seed=seed)
    what = (name, n, seed)
    assert len(pos) == len(dir_) == len(wt) == len(ref), (what, len(pos), len(ref))
    assert np.array_equal(bits(pos), bits(ref[:, 0:3])), what
    assert np.array_equal(bits(dir_), bits(ref[:, 3:6])), what
    assert np.array_equal(bits(wt), bits(ref[:, 6])), what
    return pos, dir_, wt


def assert_device_map(ctx, name, n, seed, emitted=None):
    """rt_build_photon_map + rt_get_photons == the oracle's emission in the oracle's kd order, and == the host's
    std::nth_element order of the device's own emission."""
    _, kd, _ = oracle(name, n, seed)
    what = (name, n, seed)
    stored, _ = ctx.build_photon_map(n, seed=seed)
    assert stored == len(kd), (what, stored, len(kd))
    gp, gd, gw = ctx.get_photons(stored)
    assert len(gp) == len(gd) == len(gw) == stored, what
    assert np.array_equal(bits(gp), bits(kd[:, 0:3])), what
    assert np.array_equal(bits(gd), bits(kd[:, 3:6])), what
    assert np.array_equal(bits(gw), bits(kd[:, 6])), what
    pos, dir_, wt = emitted if emitted is not None else ctx.emit_photons(n, seed=seed)
    if len(pos):
        hp, hd, hw = pyrt.kd_order(pos, dir_, wt)
        assert np.array_equal(bits(gp), bits(hp)) and np.array_equal(bits(gd), bits(hd)) and np.array_equal(bits(gw), bits(hw)), what
    else:
        assert stored == 0, what
    return gp, gd, gw


@pytest.mark.parametrize("n_lights", pc.LIGHT_COUNTS)
def test_emission_over_light_counts(n_lights, ctxs):
    """rt_emit_photons for every request of the list and two seeds: the oracle's photons in the oracle's order.
    Requests below the light count give zero slots: no photons and no error."""
    name = "lights%d" % n_lights
    ctx = ctxs(name)
    stored = {}
    for _, n, seed in pc.emission_cases(n_lights):
        pos, _, _ = assert_emission(ctx, name, n, seed)
        stored[(n, seed)] = len(pos)
        if pc.slots(n, n_lights) == 0:
            assert len(pos) == 0
    # the sweep is not hollow: zero-slot requests exist beyond one light, and the large requests store hundreds
    assert n_lights == 1 or any(pc.slots(n, n_lights) == 0 for n, _ in stored)
    assert all(v > 256 for (n, _), v in stored.items() if n >= 1023), stored
    print("lights %d, stored per (request, seed): %s" % (n_lights, sorted(stored.items())))


@pytest.mark.parametrize("n_lights", pc.LIGHT_COUNTS)
def test_device_compaction_equals_host_compaction(n_lights, ctxs):
    """rt_build_photon_map (compaction by k_photon_compact, one workgroup) against rt_emit_photons (compaction on the
    host) + std::nth_element, and against the oracle: n_stored and all three arrays.  With one light the slot count
    is the request, so 1,024 m - 1, 1,024 m, 1,024 m + 1 for m = 1, 2, 3 and 1, 2, 3, 63, 64, 65 slots all occur."""
    name = "lights%d" % n_lights
    ctx = ctxs(name)
    seen = set()
    for _, n, seed in pc.emission_cases(n_lights):
        assert_device_map(ctx, name, n, seed)
        seen.add(pc.slots(n, n_lights))
    if n_lights == 1:
        assert set(pc.COMPACT_EDGES) | {1, 2, 3, 63, 64, 65} <= seen
    else:
        assert 0 in seen  # a non-zero request with perLight == 0: no launch, no map, no error
    assert ctx.build_photon_map(0)[0] == 0


@pytest.mark.parametrize("name", pc.EXIT_SCENES)
def test_exits(name, ctxs):
    """The 20-cast cap (box_bright: most slots store nothing), the roulette exit (box_dark: every slot stores, a
    full map) and the miss on the first cast (aimed_away: an empty map from a non-zero request).  (The emission's
    cast count is not compared: no entry point returns the counters of an emission.)"""
    ctx = ctxs(name)
    for n in pc.EXIT_SLOTS:
        seed = pc.SEEDS[0]
        ref, _, rays = oracle(name, n, seed)
        # the regime, restated from tests/test_photon_cases_cpu.py so that this test cannot pass hollow
        if name == "aimed_away":
            assert len(ref) == 0 and rays == n
        elif name == "box_dark":
            assert len(ref) == n
        else:
            assert 0 < len(ref) <= 3 * n // 4 and rays > 10 * n
        emitted = assert_emission(ctx, name, n, seed)
        assert_device_map(ctx, name, n, seed, emitted)
    if name != "aimed_away":
        return
    # m == 0 with n > 0: the build succeeded and left NO map
    n = pc.EXIT_SLOTS[0]
    assert ctx.build_photon_map(n, seed=pc.SEEDS[0])[0] == 0
    gp, gd, gw = ctx.get_photons(4)
    assert len(gp) == len(gd) == len(gw) == 0
    p = pyrt.make_params(16, 12, 2, mode=pyrt.MODE_RAY, seed=3, use_photons=1, k=1, photons_requested=n)
    with pytest.raises(pyrt.RtError) as e:
        ctx.render(p)
    assert e.value.code == 5
    with pytest.raises(pyrt.RtError) as e:
        ctx.knn(np.zeros((3, 3), np.float32), 1)
    assert e.value.code == 5
    # ... and the same context builds a map again once its light looks at the room (same geometry as "lights1")
    if ctx.bvh_info().node_format == pyrt.NODES_Q8:  # (forced by RT_NODES=q8: such contexts refuse updates)
        return
    ctx.update(lights=pc.light_rows(1))
    try:
        assert_device_map(ctx, "lights1", n, pc.SEEDS[0])
        assert oracle("lights1", n, pc.SEEDS[0])[0].shape[0] > 256
        ctx.knn(np.zeros((3, 3), np.float32), 1)
    finally:
        ctx.update(lights=scene(name).arrays()["lights"])  # (the fixture's context is the aimed-away scene again)
    assert ctx.build_photon_map(n, seed=pc.SEEDS[0])[0] == 0


@pytest.mark.parametrize("n_stored", sorted(pc.TINY))
def test_tiny_device_built_maps_rendered(n_stored):
    """Maps of one, two and three photons built by rt_build_photon_map, then 16x12 photon frames at 2 spp in both
    modes with k = 1 and k = n_stored against the oracle's frames over the same map; k = n_stored + 1 is refused
    (kdtree.h:182-183) and leaves the context rendering the k = 1 frame as before."""
    w, h, spp = 16, 12, 2
    req, seed = pc.TINY[n_stored]
    s = pc.lights_scene(1, w, h)
    ctx = pyrt.Context(s)
    n, _ = ctx.build_photon_map(req, seed=seed)
    assert n == n_stored
    gp, gd, gw = ctx.get_photons(n)
    ref, _, _ = orc.emit_photons(s, req, pyrt.RNG_PIXEL, seed=seed, math_mode=orc.MATH_DET)
    kd = orc.kd_build(ref)
    ext = np.concatenate([gp, gd, gw[:, None]], 1)
    assert np.array_equal(bits(ext), bits(kd))
    first = {}
    for mode in (pyrt.MODE_RAY, pyrt.MODE_PATH):
        for k in sorted({1, n_stored}):
            p = pyrt.make_params(w, h, spp, mode=mode, seed=9, use_photons=1, k=k, photons_requested=req)
            _, acc, st = ctx.render(p)
            _, ref_acc, ref_st = orc.render(s, p, math_mode=orc.MATH_DET, ext_photons=kd)
            assert np.array_equal(bits(acc), bits(ref_acc)), (n_stored, mode, k)
            assert st.knn_queries == ref_st.knn_queries > 0 and st.rays_closest == ref_st.rays_closest, (n_stored, mode, k)
            if k == 1:
                first[mode] = acc
        p = pyrt.make_params(w, h, spp, mode=mode, seed=9, use_photons=1, k=n_stored + 1, photons_requested=req)
        with pytest.raises(pyrt.RtError) as e:
            ctx.render(p)
        assert e.value.code == 5
        p.k = 1
        _, again, _ = ctx.render(p)
        assert np.array_equal(bits(again), bits(first[mode])), (n_stored, mode)
    assert first[pyrt.MODE_RAY][..., 0:3].any()  # the photons are seen: the frames are not black
    ctx.close()


def _three_five_one(base_lights):
    """Light lists of 3 and 5 lights around a one-light scene's own light (for rt_update and back)."""
    L = np.repeat(np.asarray(base_lights, np.float32)[:1], 5, axis=0).copy()
    L[1:, 0] += np.linspace(-0.5, 0.5, 4).astype(np.float32)
    return L[:3], L


@pytest.mark.parametrize("form", ["q8", "device", "updated"])
@pytest.mark.parametrize("name", ["lights5", "box_bright"])
def test_tree_forms(name, form):
    """Emission traverses the 32-byte records whatever the context's render kernels use: an RT_NODES_Q8 context, a
    device-built tree and a context whose lights went 3 -> 5 -> 1 through rt_update, on the five-light room and the
    bright closed box, 1,025 slots each."""
    n, seed = 1025, pc.SEEDS[0]
    assert pc.slots(n, 5) == pc.slots(n, 1) == n
    if form == "q8":
        ctx = pyrt.Context(scene(name), node_format=pyrt.NODES_Q8)
        assert ctx.bvh_info().node_format == pyrt.NODES_Q8
    elif form == "device":
        ctx = pyrt.Context(scene(name), bvh_builder=pyrt.BVH_DEVICE)
        if name == "lights5" and "RT_BVH_GPU" not in os.environ:  # (below 16 triangles rt_create takes the host builder)
            assert ctx.bvh_info().builder == pyrt.BVH_DEVICE
    else:
        a = scene(name).arrays()
        if name == "lights5":
            three, five, one, one_name = pc.light_rows(3), pc.light_rows(5), pc.light_rows(1), "lights1"
        else:
            (three, five), one, one_name = _three_five_one(a["lights"]), a["lights"], name
        start = pc._array_scene(a, three)
        ctx = pyrt.Context(start)
        if ctx.bvh_info().node_format == pyrt.NODES_Q8:
            ctx.close()
            pytest.skip("one-request node records were forced, and such contexts refuse updates")
        assert ctx.build_photon_map(n, seed=seed)[0] > 0
        rep = ctx.update(lights=five)
        assert rep["photons_dropped"] == 1
        if name == "lights5":
            assert_device_map(ctx, "lights5", n, seed, assert_emission(ctx, "lights5", n, seed))
        else:
            assert ctx.build_photon_map(n, seed=seed)[0] > 0
        rep = ctx.update(lights=one)
        assert rep["photons_dropped"] == 1
        name = one_name
    assert_device_map(ctx, name, n, seed, assert_emission(ctx, name, n, seed))
    ctx.close()


def test_abi_edges(ctxs):
    """rt_get_photons with too small a capacity: RT_ERR_INVALID, *n_out = n, the arrays untouched.  rt_emit_photons
    without a weight array: the same positions and directions."""
    L = pyrt.amd()
    name, req, seed = "lights1", 65, pc.SEEDS[0]
    ctx = ctxs(name)
    n, _ = ctx.build_photon_map(req, seed=seed)
    assert n == len(oracle(name, req, seed)[0]) > 8
    pattern = np.float32(-123.25)
    for cap in (0, 1, n - 1):
        pos, dir_, wt = np.full((n, 3), pattern), np.full((n, 3), pattern), np.full(n, pattern)
        got = C.c_uint32(0xdead)
        rc = L.rt_get_photons(ctx._h, pos.ctypes.data, dir_.ctypes.data, wt.ctypes.data, cap, C.byref(got))
        assert rc == 1 and got.value == n, (cap, rc, got.value)
        assert (pos == pattern).all() and (dir_ == pattern).all() and (wt == pattern).all(), cap
    gp, gd, gw = ctx.get_photons(n)  # exactly enough room
    _, kd, _ = oracle(name, req, seed)
    assert np.array_equal(bits(np.concatenate([gp, gd, gw[:, None]], 1)), bits(kd))
    # NULL weight
    ref, _, _ = oracle(name, req, seed)
    pos, dir_ = np.full((req, 3), pattern), np.full((req, 3), pattern)
    got = C.c_uint32(0xdead)
    assert L.rt_emit_photons(ctx._h, req, seed, pos.ctypes.data, dir_.ctypes.data, None, C.byref(got)) == 0
    assert got.value == len(ref)
    assert np.array_equal(bits(pos[:got.value]), bits(ref[:, 0:3])) and np.array_equal(bits(dir_[:got.value]), bits(ref[:, 3:6]))
    assert (pos[got.value:] == pattern).all() and (dir_[got.value:] == pattern).all()  # nothing past the count
    # a zero-slot request writes nothing and reports 0
    five = ctxs("lights5")
    got = C.c_uint32(0xdead)
    assert L.rt_emit_photons(five._h, 4, seed, pos.ctypes.data, dir_.ctypes.data, None, C.byref(got)) == 0 and got.value == 0
