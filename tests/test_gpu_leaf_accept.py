"""Trav::test_pair's acceptance as one 64-bit key compare and the triangle test's predicate as masks (rt_kernels.hip,
rt_device.h), on the smallest scenes where the rule decides: tests/tiescenes.py's exact ties between meshes, hits on shared
edges and axis-parallel rays, one-leaf trees, and the cubes preset.  Each through rt_trace (closest and any-hit), the pooled
frame with bounce pools (path depth 3: the mixed body, shadow-only last pool) and without (depth 1: the shadow-only body
alone), timed and counted instance, RT_LEAF2=0, bvh_leaf_max 1, 2 and 3, and eager stealing, where `shared` rays publish
from inside test_pair.  Everything is compared bit for bit with the oracle."""
import os

import numpy as np
import pytest

import orc
import pyrt
import soups
import tiescenes as ts

pytestmark = pytest.mark.gpu

SEED = 5
SCENES = ("stack", "stack_shuffled", "fan", "tiny1", "tiny2", "cubes")  # (tiny1 / tiny2: the tree is one leaf)
FRAMES = (("path3", pyrt.MODE_PATH, 3), ("path1", pyrt.MODE_PATH, 1))
_ref = {}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def size(name):
    return (32, 32, 4) if name == "cubes" else (32, 24, 4)


def params(name, mode, depth, **kw):
    w, h, spp = size(name)
    return pyrt.make_params(w, h, spp, mode=mode, max_depth=depth, seed=SEED, **kw)


def reference(name):
    """The scene, its rays with the oracle's closest hits and any-hit flags, and the oracle's frames: computed once per
    scene, read-only (none depends on the tree)."""
    if name not in _ref:
        w, h, _ = size(name)
        s = pyrt.Scene("cubes", w, h) if name == "cubes" else ts.scene(name)
        rays = soups.soup_rays(s, 512, seed=3) if name == "cubes" else np.concatenate([f.rays for f in ts.families(name)])
        want, want_any = orc.trace(s, rays), orc.trace(s, rays, orc.ACCEL_LOOP, pyrt.TRACE_ANY)["hit"]
        assert want["hit"].any()
        frames = {}
        for fname, mode, depth in FRAMES:
            _, acc, st = orc.render(s, params(name, mode, depth), math_mode=orc.MATH_DET, accel=orc.ACCEL_OBVH)
            acc.setflags(write=False)
            assert (acc[..., 3] > 0).any() and st.rays_shadow > 0
            frames[fname] = (acc, (st.rays_closest, st.rays_shadow))
        _ref[name] = (s, rays, want, want_any, frames)
    return _ref[name]


class env:
    """Environment knobs for the block."""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kw}
        os.environ.update(self.kw)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def check_frames(name, ctx, what):
    """Timed and counted frame, with the two-record instances and with the general ones (RT_LEAF2 is read at every
    launch): the oracle's accumulators and ray counts, and counted totals that do not depend on the knob."""
    _, _, _, _, frames = reference(name)
    for fname, mode, depth in FRAMES:
        want, rays = frames[fname]
        _, timed, st = ctx.render(params(name, mode, depth))
        _, counted, sc = ctx.render(params(name, mode, depth, collect_stats=1))
        with env(RT_LEAF2="0"):
            _, general, sg = ctx.render(params(name, mode, depth))
            _, gcounted, sgc = ctx.render(params(name, mode, depth, collect_stats=1))
        for acc, which in ((timed, "timed"), (counted, "counted"), (general, "RT_LEAF2=0"), (gcounted, "RT_LEAF2=0, counted")):
            diff = (bits(acc) != bits(want)).any(axis=2)
            assert not diff.any(), "%s %s %s %s: %d of %d pixels differ" % (name, what, fname, which, diff.sum(), diff.size)
        assert (st.rays_closest, st.rays_shadow) == rays == (sg.rays_closest, sg.rays_shadow), (name, what, fname)
        totals = [(x.rays_closest, x.rays_shadow, x.nodes_visited, x.tris_tested) for x in (sc, sgc)]
        print(name, what, fname, totals[0])
        assert totals[0] == totals[1], (name, what, fname)
        assert totals[0][:2] == rays and totals[0][3] > 0


@pytest.mark.parametrize("leaf", (1, 2, 3))
@pytest.mark.parametrize("name", SCENES)
def test_hits_and_frames_are_the_oracle_s(name, leaf):
    s, rays, want, want_any, _ = reference(name)
    ctx = pyrt.Context(s, bvh_leaf_max=leaf)
    try:
        got = ctx.trace(rays, pyrt.ACCEL_BVH)
        diff = (got.view(np.uint8).reshape(len(got), -1) != want.view(np.uint8).reshape(len(got), -1)).any(axis=1)
        assert not diff.any(), "closest: %d of %d rays, first %d: ray %s got %s expected %s" % (
            diff.sum(), len(diff), np.argmax(diff), rays[np.argmax(diff)], got[np.argmax(diff)], want[np.argmax(diff)])
        diff = ctx.trace(rays, pyrt.ACCEL_BVH, pyrt.TRACE_ANY)["hit"] != want_any
        assert not diff.any(), "any-hit: %d of %d rays, first ray %s" % (diff.sum(), len(diff), rays[np.argmax(diff)])
        check_frames(name, ctx, "leaf %d" % leaf)
    finally:
        ctx.close()


@pytest.mark.parametrize("name", SCENES)
def test_eager_stealing(name):
    """With the steal threshold at two free lanes nearly every round is followed by a steal pass: many lanes walk parts of
    one ray, and each publishes its improvements from inside test_pair, so the shared key decides the ties.  (RT_STEALT /
    RT_REFILLT are read when a tree is installed.)"""
    s = reference(name)[0]
    with env(RT_STEALT="2", RT_REFILLT="40"):
        ctx = pyrt.Context(s)
    try:
        check_frames(name, ctx, "eager stealing")
    finally:
        ctx.close()
