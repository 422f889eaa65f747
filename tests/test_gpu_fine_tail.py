"""The fine tail of a plain frame's wave-tile list (rt_api.cpp wave_tiles, rt_kernels.hip render_tile): the last coarse
tiles of the list rendered as items of more samples and fewer pixels per wave.  The frame must not depend on it: the
accumulator of every RT_FINE_TAIL setting ('1': one coarse tile split, 'all': every tile, unset: the default, which on
frames this small is the whole list too) equals RT_FINE_TAIL=0's bit for bit, timed and counted instance, and the counted
pass counts the same rays and samples.  Frame sizes: 8x8 (one granule), 33x19 (the edges cut the coarse and the fine
footprint), 64x64 (more items than one workgroup's waves).

A list has a tail only where the fine shift min(6, sshift + 2), clamped to the launch's sample count, is above the coarse
one, and on frames this small the automatic coarse shift already is the sample limit.  So the cases set the coarse shift
(lanes_per_pixel): 5 samples at 2 per wave (coarse 8x4 x 2 -> fine 4x4 x 4: the fine shift clamps to the count), 16 at 8
(4x2 x 8 -> 2x2 x 16, clamped too), 64 and 128 at 16 (2x2 x 16 -> 1x1 x 64; 128: two sample groups per fine item); and 64
samples at the automatic shift (1x1 x 64 coarse: the fine shift clamps onto the coarse one, no tail).  That a tail was
really rendered shows in the counted pass: its items put other lanes into a wave, so the wave-level node steps and leaf
phases (rt_stats.reserved[0..1]) and the per-lane node and triangle visits differ from RT_FINE_TAIL=0's wherever a tail
exists ('all' and the default), and are equal where none does.  RT_FINE_TAIL is read at every launch."""
import os
import subprocess
import sys

import numpy as np
import pytest

import pyrt

pytestmark = pytest.mark.gpu

SEED = 11
SIZES = ((8, 8), (33, 19), (64, 64))
# (samples, lanes_per_pixel, a tail exists)
CASES = ((5, 2, True), (16, 8, True), (64, 16, True), (128, 16, True), (64, 0, False))
TAILS = ("1", "all", None)  # (None: the default)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


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


def counts(st):
    return (st.rays_closest, st.rays_shadow, st.samples)


def schedule(st):
    """What depends on which lanes share a wave (counted pass)."""
    return (st.nodes_visited, st.tris_tested, st.reserved[0], st.reserved[1])


def check(ctx, what, w, h, spp, lpp, tail_exists, **kw):
    """Timed and counted frame at every setting against RT_FINE_TAIL=0; the counted pass's schedule figures say whether
    the launch had a tail."""
    def frames():
        _, timed, st = ctx.render(pyrt.make_params(w, h, spp, seed=SEED, lanes_per_pixel=lpp, **kw))
        _, counted, sc = ctx.render(pyrt.make_params(w, h, spp, seed=SEED, lanes_per_pixel=lpp, collect_stats=1, **kw))
        return timed, counted, counts(st), counts(sc), schedule(sc)

    with env(RT_FINE_TAIL="0"):
        want = frames()
    assert (want[0][..., 3] > 0).any() and want[3][1] > 0 and want[4][2] > 0, what
    assert not (bits(want[0]) != bits(want[1])).any(), (what, "RT_FINE_TAIL=0: timed and counted frame differ")
    for tail in TAILS:
        with env(RT_FINE_TAIL=tail):
            got = frames()
        print(what, "RT_FINE_TAIL =", tail, "schedule", got[4], "without", want[4])
        for k, which in ((0, "timed"), (1, "counted")):
            diff = (bits(got[k]) != bits(want[k])).any(axis=2)
            assert not diff.any(), "%s RT_FINE_TAIL=%s %s: %d of %d pixels differ, first (y, x) %s" % (
                what, tail, which, diff.sum(), diff.size, np.argwhere(diff)[0])
        assert got[2] == want[2] and got[3] == want[3], (what, tail, got[2:], want[2:])
        if not tail_exists:
            assert got[4] == want[4], (what, tail, "no tail, but another schedule", got[4], want[4])
        elif tail != "1":
            assert got[4] != want[4], (what, tail, "the launch rendered no fine item", got[4])


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("kind", ("cubes", "lowres"))
def test_frame_does_not_depend_on_the_fine_tail(kind, size):
    w, h = size
    ctx = pyrt.Context(pyrt.Scene(kind, w, h))
    try:
        for spp, lpp, tail in CASES:
            check(ctx, "%s %dx%d x %d at %d" % (kind, w, h, spp, lpp), w, h, spp, lpp, tail)
    finally:
        ctx.close()


@pytest.mark.parametrize("kind", ("cubes", "lowres"))
def test_shards_take_the_tail_of_their_own_list(kind):
    """world = 2: each rank's list ends in its own fine items."""
    w, h = 33, 19
    ctx = pyrt.Context(pyrt.Scene(kind, w, h))
    try:
        for rank in (0, 1):
            for spp, lpp in ((5, 2), (64, 16)):
                check(ctx, "%s rank %d of 2, %d spp" % (kind, rank, spp), w, h, spp, lpp, True, rank=rank, world=2)
    finally:
        ctx.close()


@pytest.mark.parametrize("kind", ("cubes", "lowres"))
def test_sample_ranges(kind):
    """A frame of 128 samples as the ranges [0, 37) and [37, 128) through rt_render_passes: the fine shift follows each
    range's count (coarse 2x2 x 16; 37 samples: 32 per fine item, 91: 64), and the sum is the one-launch frame."""
    w, h, spp = 33, 19, 128
    ctx = pyrt.Context(pyrt.Scene(kind, w, h))
    bg = np.zeros((h, w, 3), np.float32)
    try:
        for b, n in ((0, 37), (37, 91)):  # (each range alone: same frame, and a tail was rendered)
            check(ctx, "%s samples [%d, %d)" % (kind, b, b + n), w, h, spp, 16, True, spp_begin=b, spp_count=n)
        with env(RT_FINE_TAIL="0"):
            _, want, _ = ctx.render(pyrt.make_params(w, h, spp, seed=SEED, lanes_per_pixel=16))
        for tail in ("0",) + TAILS:
            with env(RT_FINE_TAIL=tail):
                acc = np.zeros((h, w, 4), np.float32)
                for b, n in ((0, 37), (37, 91)):
                    ctx.render_passes(pyrt.make_params(w, h, spp, seed=SEED, spp_begin=b, spp_count=n, lanes_per_pixel=16), bg, acc)
            diff = (bits(acc) != bits(want)).any(axis=2)
            assert not diff.any(), "%s RT_FINE_TAIL=%s: %d of %d pixels differ" % (kind, tail, diff.sum(), diff.size)
    finally:
        ctx.close()


@pytest.mark.parametrize("kind", ("cubes", "lowres"))
def test_eager_stealing(kind):
    """(RT_STEALT / RT_REFILLT are read when a tree is installed.)"""
    w, h = 33, 19
    with env(RT_STEALT="2", RT_REFILLT="40"):
        ctx = pyrt.Context(pyrt.Scene(kind, w, h))
    try:
        for spp, lpp in ((5, 2), (64, 16)):
            check(ctx, "%s eager stealing, %d spp" % (kind, spp), w, h, spp, lpp, True)
    finally:
        ctx.close()


_LAYOUT_SCRIPT = '''
import os, sys, numpy as np
sys.path.insert(0, sys.argv[1] + "/ray-tracing-engine_amd")
import pyrt
out = {}
for kind in ("cubes", "lowres"):
    ctx = pyrt.Context(pyrt.Scene(kind, 33, 19))
    for spp, lpp in ((5, 2), (64, 16)):
        for tail in ("0", "1", "all", ""):
            os.environ["RT_FINE_TAIL"] = tail
            if not tail: del os.environ["RT_FINE_TAIL"]
            for stats in (0, 1):
                _, acc, st = ctx.render(pyrt.make_params(33, 19, spp, seed=11, collect_stats=stats, lanes_per_pixel=lpp))
                key = "%s_%d_%s_%d" % (kind, spp, tail or "default", stats)
                out[key] = acc; out[key + "_n"] = np.array([st.rays_closest, st.rays_shadow, st.samples])
                out[key + "_s"] = np.array([st.nodes_visited, st.tris_tested, st.reserved[0], st.reserved[1]])
    ctx.close()
np.savez(sys.argv[2], **out)
'''


@pytest.mark.parametrize("topk", ("0", "37"))
def test_partial_top_and_tree_from_l2(topk, tmp_path):
    """RT_TOPK=37: a partial top of the tree in LDS (the LT_TOP instances); RT_TOPK=0: none (the tree from L2).  The knob is
    read once per process, so each layout renders in a process of its own."""
    script, out = tmp_path / "layout.py", tmp_path / "layout.npz"
    script.write_text(_LAYOUT_SCRIPT)
    r = subprocess.run([sys.executable, str(script), pyrt.ROOT, str(out)], env=dict(os.environ, RT_TOPK=topk), capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.load(out)
    for kind in ("cubes", "lowres"):
        for spp in (5, 64):
            for stats in (0, 1):
                want = "%s_%d_0_%d" % (kind, spp, stats)
                assert (got[want][..., 3] > 0).any()
                for tail in ("1", "all", "default"):
                    key = "%s_%d_%s_%d" % (kind, spp, tail, stats)
                    assert np.array_equal(bits(got[key]), bits(got[want])), (topk, key)
                    assert np.array_equal(got[key + "_n"], got[want + "_n"]), (topk, key)
                    if stats and tail != "1":  # (a tail was rendered: another schedule in the counted pass)
                        assert not np.array_equal(got[key + "_s"], got[want + "_s"]), (topk, key, got[key + "_s"])
