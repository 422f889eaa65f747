"""The leaf phase of Trav::round: the LT_LEAF2 instances the launcher picks for trees whose leaves hold at most two
records (their leaf phase is test_pair alone; RT_LEAF2=0 forces the general instances and is read at every launch) — on
every leaf size, on scenes whose last record is a one-record leaf, across a rebuild and under eager stealing.  Frames are
compared bit for bit."""
import os

import numpy as np
import pytest

import orc
import pyrt
import soups
import tiescenes

pytestmark = pytest.mark.gpu

W = H = 48
SPP = 4
SEED = 29
# (name, mode, max_depth): a path frame with bounce pools and a shadow-only last pool, and a direct-lighting frame
FRAMES = (("path3", pyrt.MODE_PATH, 3), ("direct", pyrt.MODE_RAY, 1))
LEAVES = (1, 2, 3, 8)  # bvh_leaf_max: 2 is the default; 1 and 2 take the LT_LEAF2 instances, 3 and 8 the general ones


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def params(mode, depth, **kw):
    return pyrt.make_params(W, H, SPP, mode=mode, max_depth=depth, seed=SEED, **kw)


class general_instances:
    """RT_LEAF2=0 for the launches inside the block."""

    def __enter__(self):
        self.old = os.environ.get("RT_LEAF2")
        os.environ["RT_LEAF2"] = "0"

    def __exit__(self, *exc):
        if self.old is None:
            del os.environ["RT_LEAF2"]
        else:
            os.environ["RT_LEAF2"] = self.old


@pytest.fixture(scope="module")
def presets():
    """The two preset scenes with the oracle's frames (which do not depend on the tree): computed once, read-only."""
    out = {}
    for kind in ("cubes", "lowres"):
        s = pyrt.Scene(kind, W, H)
        ref = {}
        for name, mode, depth in FRAMES:
            _, acc, st = orc.render(s, params(mode, depth), math_mode=orc.MATH_DET)
            acc.setflags(write=False)
            ref[name] = (acc, (st.rays_closest, st.rays_shadow))
        out[kind] = (s, ref)
    return out


@pytest.mark.parametrize("leaf", LEAVES)
@pytest.mark.parametrize("kind", ("cubes", "lowres"))
def test_every_leaf_size_renders_the_oracle_s_frame(presets, kind, leaf):
    s, ref = presets[kind]
    ctx = pyrt.Context(s, bvh_leaf_max=leaf)
    try:
        assert ctx.bvh_info().leaf_max <= max(leaf, 1)
        for name, mode, depth in FRAMES:
            want, rays = ref[name]
            _, timed, st = ctx.render(params(mode, depth))
            _, counted, sc = ctx.render(params(mode, depth, collect_stats=1))
            with general_instances():
                _, general, sg = ctx.render(params(mode, depth))
                _, gcounted, sgc = ctx.render(params(mode, depth, collect_stats=1))
            assert np.array_equal(bits(timed), bits(want)), (name, "timed")
            assert np.array_equal(bits(counted), bits(want)), (name, "counted")
            assert np.array_equal(bits(general), bits(want)), (name, "RT_LEAF2=0")
            assert np.array_equal(bits(gcounted), bits(want)), (name, "RT_LEAF2=0, counted")
            assert (st.rays_closest, st.rays_shadow) == rays == (sg.rays_closest, sg.rays_shadow)
            # the counted totals do not depend on the knob
            totals = [(x.rays_closest, x.rays_shadow, x.nodes_visited, x.tris_tested) for x in (sc, sgc)]
            print(kind, leaf, name, totals[0])
            assert totals[0] == totals[1], name
            assert totals[0][:2] == rays and totals[0][3] > 0
    finally:
        ctx.close()


@pytest.mark.parametrize("leaf", (1, 2, 3))
@pytest.mark.parametrize("name", ("tiny1", "tiny2", "tiny3"))
def test_one_record_leaf_at_the_end_of_the_array(name, leaf):
    """Scenes of 1, 2 and 3 triangles: with an odd count (or leaf size 1) the LAST record of the array is a one-record
    leaf, whose second request re-reads it instead of the 48 bytes behind the array.  Closest-hit and any-hit rt_trace and
    a frame against the exhaustive loop."""
    s = tiescenes.scene(name)
    rays = soups.soup_rays(s, 512, seed=3)
    ctx = pyrt.Context(s, bvh_leaf_max=leaf)
    try:
        want = ctx.trace(rays, pyrt.ACCEL_BRUTE)
        assert want["hit"].any()
        assert np.array_equal(ctx.trace(rays, pyrt.ACCEL_BVH).view(np.uint8), want.view(np.uint8))
        assert np.array_equal(ctx.trace(rays, pyrt.ACCEL_BVH, pyrt.TRACE_ANY)["hit"], want["hit"])
        for fname, mode, depth in FRAMES:
            _, brute, sb = ctx.render(params(mode, depth, accel=pyrt.ACCEL_BRUTE))
            _, acc, st = ctx.render(params(mode, depth))
            with general_instances():
                _, general, _ = ctx.render(params(mode, depth))
            assert np.array_equal(bits(acc), bits(brute)), fname
            assert np.array_equal(bits(general), bits(brute)), (fname, "RT_LEAF2=0")
            assert (st.rays_closest, st.rays_shadow) == (sb.rays_closest, sb.rays_shadow)
    finally:
        ctx.close()


def test_the_instance_follows_the_resident_tree(presets):
    """The choice is made per launch from the tree the context holds: contexts of leaf size 2 and 3 render in turn in one
    process, each is rebuilt (rt_rebuild builds with the leaf size the context was created with) and renders again, and
    every frame is the oracle's — so the two-record instance never ran on the three-record tree."""
    s, ref = presets["lowres"]
    want, _ = ref["path3"]
    p = params(pyrt.MODE_PATH, 3)
    two, three = pyrt.Context(s, bvh_leaf_max=2), pyrt.Context(s, bvh_leaf_max=3)
    try:
        assert two.bvh_info().leaf_max == 2 and three.bvh_info().leaf_max == 3
        for step in ("fresh", "rebuilt", "rebuilt again"):
            for ctx in (two, three, two):
                _, acc, _ = ctx.render(p)
                assert np.array_equal(bits(acc), bits(want)), (step, ctx.bvh_info().leaf_max)
            assert three.rebuild()["rebuilt"] == 1 and two.rebuild()["rebuilt"] == 1
            assert two.bvh_info().leaf_max == 2 and three.bvh_info().leaf_max == 3
    finally:
        two.close()
        three.close()


def test_eager_stealing_keeps_the_frame(presets):
    """Thieves rewrite rows of their victims' stacks between rounds; with the steal threshold at two free lanes nearly
    every round is followed by a steal pass, so the entry a finished leaf pops meets as many rewritten stacks as it can —
    in the two-record instance and in the counted, general one.  (RT_STEALT / RT_REFILLT are read when a tree is
    installed.)"""
    s, ref = presets["lowres"]
    old = {k: os.environ.get(k) for k in ("RT_STEALT", "RT_REFILLT")}
    os.environ["RT_STEALT"], os.environ["RT_REFILLT"] = "2", "40"
    try:
        ctx = pyrt.Context(s)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    try:
        for name, mode, depth in FRAMES:
            want, rays = ref[name]
            _, acc, st = ctx.render(params(mode, depth))
            _, counted, _ = ctx.render(params(mode, depth, collect_stats=1))
            assert np.array_equal(bits(acc), bits(want)), name
            assert np.array_equal(bits(counted), bits(want)), (name, "counted")
            assert (st.rays_closest, st.rays_shadow) == rays
    finally:
        ctx.close()
