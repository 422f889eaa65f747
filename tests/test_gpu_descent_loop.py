"""The descent loop of Trav::round in the timed whole-tree-in-LDS, two-record-leaf instance (Trav::DESCENT, descent_asm:
one assembly block that narrows exec step by step and restores it once) against its twin with the compiler's loop
(RT_DESCENT=0, read at every launch), the counted instances (which keep the compiler's loop) and the oracle — on the
presets, at both ends of the exit rule, on trees whose root is a leaf, on frames with lanes that never hold a ray, under
eager stealing, at every stack-row count the shallow scene builders give and on a chain-shaped tree at the depth cap that
still fits the LDS whole.  The loop leaves when fewer than
exitBelow = max(1, min(RT_LEAFT, live * RT_LEAFMUL >> 6)) lanes still descend, in both forms: the schedule is the
same, and every comparison is bit for bit on the accumulator."""
import os

import numpy as np
import pytest

import depth_scenes
import orc
import pyrt
import tiescenes

pytestmark = pytest.mark.gpu

W = H = 48
SPP = 4
SEED = 29
# (name, mode, max_depth): a path frame with bounce pools and a shadow-only last pool (the mixed and the any-hit walker),
# and a direct-lighting frame (the any-hit walker alone); both cast their primary rays through the closest-hit walker
FRAMES = (("path3", pyrt.MODE_PATH, 3), ("direct", pyrt.MODE_RAY, 1))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def params(mode, depth, w=W, h=H, **kw):
    return pyrt.make_params(w, h, SPP, mode=mode, max_depth=depth, seed=SEED, **kw)


class env:
    """Environment knobs for the block; None unsets."""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kw}
        for k, v in self.kw.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def rays(st):
    return (st.rays_closest, st.rays_shadow)


def totals(st):
    return (st.rays_closest, st.rays_shadow, st.nodes_visited, st.tris_tested)


def four_frames(ctx, p, pc):
    """The default frame, the RT_DESCENT=0 frame and the counted frame with and without the knob: the three frames that
    must equal the first, the ray counts of the timed ones and the counted totals."""
    _, timed, st = ctx.render(p)
    _, counted, sc = ctx.render(pc)
    with env(RT_DESCENT="0"):
        _, twin, sw = ctx.render(p)
        _, tcounted, swc = ctx.render(pc)
    return timed, (("RT_DESCENT=0", twin), ("counted", counted), ("RT_DESCENT=0, counted", tcounted)), (rays(st), rays(sw)), (totals(sc), totals(swc))


def check(ctx, what, want=None, want_rays=None, w=W, h=H):
    for name, mode, depth in FRAMES:
        timed, others, rr, tt = four_frames(ctx, params(mode, depth, w, h), params(mode, depth, w, h, collect_stats=1))
        print(what, name, tt[0])
        for label, frame in others:
            assert np.array_equal(bits(frame), bits(timed)), (what, name, label)
        if want is not None:
            assert np.array_equal(bits(timed), bits(want[name][0])), (what, name, "reference")
            assert rr[0] == want[name][1], (what, name)
        assert rr[0] == rr[1] == tt[0][:2], (what, name)
        assert tt[0] == tt[1], (what, name, "the counted totals do not depend on the knob")


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


def brute_frames(ctx, w=W, h=H):
    """The exhaustive loop's frames of a context's scene (no tree is walked)."""
    ref = {}
    for name, mode, depth in FRAMES:
        _, acc, st = ctx.render(params(mode, depth, w, h, accel=pyrt.ACCEL_BRUTE))
        ref[name] = (acc, rays(st))
    return ref


@pytest.mark.parametrize("leaf", (1, 2))
@pytest.mark.parametrize("kind", ("cubes", "lowres"))
def test_presets_equal_the_twin_the_counted_frame_and_the_oracle(presets, kind, leaf):
    s, ref = presets[kind]
    ctx = pyrt.Context(s, bvh_leaf_max=leaf)
    try:
        check(ctx, "%s leaf %d" % (kind, leaf), ref)
    finally:
        ctx.close()


@pytest.mark.parametrize("leaft,leafmul", ((1, 64), (64, 64), (64, 1), (None, None)))
def test_the_exit_rule_at_its_ends(presets, leaft, leafmul):
    """(1, 64): the loop runs until no lane descends; (64, 64): it leaves as soon as one live lane holds a leaf, after
    one step at the earliest; (64, 1): live * 1 >> 6 is 0 or 1, the clamp exitBelow = 1; and the defaults.  (RT_LEAFT /
    RT_LEAFMUL are read when a tree is installed.)"""
    s, ref = presets["lowres"]
    with env(RT_LEAFT=None if leaft is None else str(leaft), RT_LEAFMUL=None if leafmul is None else str(leafmul)):
        ctx = pyrt.Context(s)
    try:
        check(ctx, "RT_LEAFT %s RT_LEAFMUL %s" % (leaft, leafmul), ref)
    finally:
        ctx.close()


@pytest.mark.parametrize("name", ("tiny1", "tiny2", "tiny3"))
def test_the_root_is_a_leaf(name):
    """One-leaf trees (one record above the leaf): every ray's descent is one step, the later rounds of a wave enter the
    block with an empty mask and fall through."""
    ctx = pyrt.Context(tiescenes.scene(name))
    try:
        print(name, "nodes", ctx.bvh_info().n_nodes, "max_depth", ctx.bvh_info().max_depth)
        check(ctx, name, brute_frames(ctx))
    finally:
        ctx.close()


@pytest.mark.parametrize("kind", ("cubes", "lowres"))
def test_edge_tiles_hold_lanes_without_a_ray(kind):
    """50x46: the wave tiles of the right and the bottom edge hold lanes that have no ray from the first step on, and
    waves whose first step is entered by a few lanes."""
    w, h = 50, 46
    s = pyrt.Scene(kind, w, h)
    ref = {}
    for name, mode, depth in FRAMES:
        _, acc, st = orc.render(s, params(mode, depth, w, h), math_mode=orc.MATH_DET)
        ref[name] = (acc, (st.rays_closest, st.rays_shadow))
    ctx = pyrt.Context(s)
    try:
        check(ctx, "%s 50x46" % kind, ref, w=w, h=h)
    finally:
        ctx.close()


def test_thieves_start_below_the_root(presets):
    """With the steal threshold at two free lanes nearly every round is followed by a steal pass: thieves enter the loop at
    nodes below the root, with one-entry stacks.  lowres against the oracle, the tie scenes against the exhaustive loop.
    (RT_STEALT / RT_REFILLT are read when a tree is installed.)"""
    s, ref = presets["lowres"]
    with env(RT_STEALT="2", RT_REFILLT="40"):
        ctx = pyrt.Context(s)
        ties = [(name, pyrt.Context(tiescenes.scene(name))) for name in tiescenes.SCENES]
    try:
        check(ctx, "lowres, eager stealing", ref)
        for name, c in ties:
            check(c, "%s, eager stealing" % name, brute_frames(c))
    finally:
        ctx.close()
        for _, c in ties:
            c.close()


@pytest.mark.parametrize("name", depth_scenes.NAMES + ("hires",))
def test_every_stack_row_count(name):
    """depth_scenes' shallow scenes (2 to 5 stack rows; B, D and F have two-record leaves and take the instance under
    test, the others the general one) and the 17 rows of hires, whose tree stays partly outside the LDS; a launch that
    takes another instance ignores the knob (lowres, in the tests above, is the deepest preset that fits the LDS whole).  Against the exhaustive loop where that is quick (the shallow scenes)."""
    shallow = name in depth_scenes.SHALLOW
    preset = depth_scenes.PREFIX + name if shallow else name
    s = depth_scenes.preset(preset, W, H)
    ctx = pyrt.Context(s, **depth_scenes.context_options(preset))
    try:
        assert ctx.bvh_info().max_depth == depth_scenes.max_depth(preset)
        check(ctx, preset, brute_frames(ctx) if shallow else None)
    finally:
        ctx.close()


# plan_persist's LDS budget (rt_kernels.hip, bvh_build.h): words per CU, per stack row, of a wave's ray pool, per node
LDS_WORDS, ROW_WORDS, POOL_WORDS, NODE_WORDS, DEPTH_CAP = 160 * 1024 // 4, 64, 1128, 8, 31


def resident_waves(max_depth, n_nodes):
    """The waves per CU plan_persist keeps for a tree of this depth if the whole tree fits in LDS beside their stacks
    (the LT_ALL class), else 0."""
    wave = (max_depth + 1) * ROW_WORDS + POOL_WORDS
    w = 16
    while w > 1 and w * wave > LDS_WORDS:
        w -= 1
    return w if w * wave <= LDS_WORDS and (LDS_WORDS - w * wave) // NODE_WORDS >= n_nodes else 0


def chain_scene(cells=34, ratio=2.0):
    """A strip of `cells` rectangles in the front plane of tiescenes' stack view whose widths double from left to right,
    over the stack scene's back sheet, under its camera and lights: the surface-area splits peel the strip off cell by
    cell, so with spare levels to use (RT_BVH_SLACK) the tree is a chain down to the builder's depth cap."""
    a = tiescenes.arrays("stack")
    z = np.float32(tiescenes.FRONT_Z) / np.float32(tiescenes.L)
    x = np.concatenate([[0.0], np.cumsum(ratio ** np.arange(cells))])
    x = -1.25 + 2.5 * x / x[-1]
    pos, tri = [], []
    for i in range(cells):
        b = len(pos)
        pos += [(x[i], -1, z), (x[i + 1], -1, z), (x[i], 1, z), (x[i + 1], 1, z)]
        tri += [(b, b + 1, b + 2), (b + 3, b + 2, b + 1)]
    bp, bt = tiescenes._sheet(tiescenes.BACK_Z)
    allpos = np.concatenate([np.array(pos, np.float32), bp.astype(np.float32) / np.float32(tiescenes.L)])
    alltri = np.concatenate([np.array(tri), bt + len(pos)]).astype(np.uint32)
    nrm = np.tile(np.array((0, 0, 1), np.float32), (len(allpos), 1))
    return pyrt.ArrayScene(allpos, nrm, alltri, np.array([0, len(tri), len(alltri)], np.uint32),
                           np.array([0, len(pos), len(allpos)], np.uint32), a["materials"][:2], a["lights"], a["camera"])


def test_the_deepest_tree_the_lds_resident_class_allows():
    """A tree at the builder's depth cap — 31 levels, 32 stack rows, the deepest any tree can be — of few enough nodes
    that plan_persist still keeps it whole in LDS (twelve waves per CU instead of sixteen): the longest descents and the
    tallest stacks the block can meet.  Against the exhaustive loop.  (RT_BVH_SLACK is read when a tree is built.)"""
    with env(RT_BVH_SLACK="40"):
        ctx = pyrt.Context(chain_scene())
    try:
        info = ctx.bvh_info()
        print("chain: %d nodes, max_depth %d, leaf_max %d, %d waves" % (info.n_nodes, info.max_depth, info.leaf_max, resident_waves(info.max_depth, info.n_nodes)))
        assert info.max_depth == DEPTH_CAP and info.leaf_max <= 2
        assert resident_waves(info.max_depth, info.n_nodes) == 12
        check(ctx, "chain", brute_frames(ctx))
    finally:
        ctx.close()


@pytest.mark.parametrize("kind,leaf,want", (("cubes", 1, True), ("cubes", 2, True), ("lowres", 2, True), ("lowres", 1, False), ("hires", 2, False)))
def test_which_presets_are_lds_resident(kind, leaf, want):
    """What the tests above rest on: the trees of cubes and of lowres at leaf size 2 fit the LDS whole (they take the
    instance under test), lowres at leaf size 1 and hires do not (their launches ignore the knob)."""
    ctx = pyrt.Context(pyrt.Scene(kind, W, H), bvh_leaf_max=leaf)
    try:
        info = ctx.bvh_info()
        print(kind, leaf, info.n_nodes, info.max_depth)
        assert (resident_waves(info.max_depth, info.n_nodes) == 16) == want
    finally:
        ctx.close()


def test_the_instance_follows_the_launch(presets):
    """RT_DESCENT is read at every launch: one context renders with the knob unset, at 0, at 1 and unset again, and every
    frame is the oracle's."""
    s, ref = presets["lowres"]
    want, want_rays = ref["path3"]
    p = params(pyrt.MODE_PATH, 3)
    ctx = pyrt.Context(s)
    try:
        for knob in (None, "0", None, "0", "1", "0", None):
            with env(RT_DESCENT=knob):
                _, acc, st = ctx.render(p)
            assert np.array_equal(bits(acc), bits(want)), knob
            assert rays(st) == want_rays, knob
    finally:
        ctx.close()
