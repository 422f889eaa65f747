"""rt_render_adaptive where its device-built work list can go wrong without test_gpu_adaptive.py noticing: every wave
footprint of k_adapt_expand (csrc/adaptive.hip kTileW / kTileH) over partial edge granules, frames of more than 1,024
granules (the second iteration of both list kernels' chunk loops, with a carried offset), more than 64 passes, frames
smaller than a granule, the device form on those shapes, and a small frame after a large one on the same scratch.

Everything is bit for bit against the chain of rt_render_passes calls and the numpy rule (adaptive_cases.check_frame);
there is no tolerance in this file.  The conditions the inputs must meet (which passes cross a chunk, which footprint a
pass selects) are asserted from the rule's output and from the frame's geometry, never from the kernels' results."""
import ctypes as C

import numpy as np
import pytest

import adaptive_ref
import pyrt
from adaptive_cases import (CHUNK, bits, chain_of, check_frame, check_result, chunk_conditions, pick_chunk_threshold,
                            pick_threshold)

gpu = pytest.mark.gpu  # (the footprint arithmetic below needs no device)

SEED = 17
PASSES = 6

# wave footprints by sshift (rt_api.cpp wave_tile_shape; adaptive.hip kTileW / kTileH)
FOOTPRINT = [(8, 8), (8, 4), (4, 4), (4, 2), (2, 2), (2, 1), (1, 1)]

# The sshift of every case below, from choose_sshift_px (rt_api.cpp) and not from a run.  lanes_per_pixel L > 0 returns
# floor(log2 L) (at most 6) at once.  Otherwise three loops raise s from 0, each only while (2 << s) <= P:
#   first   while (pixels << s) / 64 < 131,072.  The largest pass here has 520 x 264 = 137,280 pixels, and
#           137,280 * 32 / 64 = 68,640, so this holds for every s <= 5 on every frame of this file: the loop stops
#           only when 2^(s+1) > P or s = 6, that is at s = min(6, floor(log2 P)).  (An adaptive pass passes its
#           active pixels, which are fewer.)
#   pooled  (BVH, no photons, <= 3 lights; both scenes have 3 lights and far fewer than 65,536 nodes): up to 4,
#           under the same (2 << s) <= P — already exhausted by the first loop, so s does not move
#   photon  (use_photons on the BVH): up to 6 under the same condition — does not move either
# ACCEL_BRUTE takes the first loop alone, the photon map the first and the third, everything else the first and the
# second.
#
#      P   lanes_per_pixel   sshift   footprint
#      1         0             0        8x8
#      2         0             1        8x4
#      3         0             1        8x4     (3 samples in rounds of 2: the last round is half empty)
#      4         0             2        4x4     (test_gpu_adaptive.py; the chunk frames below)
#      5         0             2        4x4     (rounds of 4: 4 + 1)
#      6         0             2        4x4     (4 + 2)
#      8         0             3        4x2
#     16         0             4        2x2     (also ACCEL_BRUTE and the photon map)
#     32         0             5        2x1
#     64         0             6        1x1
#     64         1             0        8x8
#     64         8             3        4x2
#     64        64             6        1x1
SSHIFT = {1: 0, 2: 1, 3: 1, 4: 2, 5: 2, 6: 2, 8: 3, 16: 4, 32: 5, 64: 6}
LANES_SSHIFT = {1: 0, 8: 3, 64: 6}


def sshift_rule(pixels, P, lanes=0, pooled=True, photons=False):
    """choose_sshift_px restated (the table above is its value on this file's cases)."""
    s = 0
    if lanes:
        while (1 << (s + 1)) <= lanes and s < 6:
            s += 1
        return s
    while s < 6 and (pixels << s) // 64 < 32 * 256 * 16 and (2 << s) <= P:
        s += 1
    if pooled:
        while s < 4 and (2 << s) <= P:
            s += 1
    if photons:
        while s < 6 and (2 << s) <= P:
            s += 1
    return s


def edge_tiles(w, h, sshift):
    """(partly outside, wholly outside) wave tiles of the frame's granules at this footprint: the tiles
    k_adapt_expand clips (it lists the first kind and skips the second)."""
    tw, th = FOOTPRINT[sshift]
    gx, gy = adaptive_ref.granule_grid(w, h)
    part = skipped = 0
    for y8 in range(gy):
        for x8 in range(gx):
            cw, ch = min(8, w - 8 * x8), min(8, h - 8 * y8)
            ntx, nty = -(-cw // tw), -(-ch // th)
            skipped += (8 // tw) * (8 // th) - ntx * nty
            part += ntx * nty - (cw // tw) * (ch // th)
    return part, skipped


def bg_of(w, h):
    # (a 1-pixel-high image has no background gradient: Image::fillBackground divides by h - 1)
    return pyrt.background(w, h) if h > 1 else np.full((h, w, 3), 0.5, np.float32)


class Frames:
    """Contexts and reference chains, made once and shared by the tests of this file (never modified)."""

    def __init__(self):
        self.ctxs, self.chains = {}, {}

    def ctx(self, kind, w, h, photons=False):
        key = (kind, w, h, photons)
        if key not in self.ctxs:
            c = pyrt.Context(pyrt.Scene(kind, w, h))
            if photons:
                pos, dir_, wt = c.emit_photons(3000, seed=2)
                kp, kd_, _ = pyrt.kd_order(pos, dir_, wt)
                c.set_photons(kp, kd_)
            assert c.bvh_info().n_nodes <= 65536  # the sshift table's premise
            self.ctxs[key] = c
        return self.ctxs[key]

    def chain(self, kind, w, h, P, passes=PASSES, scene_wh=None, photons=False, **kw):
        """(ctx, params, bg, chain) of a w x h frame through the context of kind at scene_wh (default w x h)."""
        sw, sh = scene_wh or (w, h)
        key = (kind, sw, sh, photons, w, h, P, passes, tuple(sorted(kw.items())))
        c = self.ctx(kind, sw, sh, photons)
        if key not in self.chains:
            kw.setdefault("mode", pyrt.MODE_PATH)
            p = pyrt.make_params(w, h, P, seed=SEED, **kw)
            bg = bg_of(w, h)
            ch = chain_of(c, p, bg, passes)
            for a in ch:
                a.flags.writeable = False
            bg.flags.writeable = False
            self.chains[key] = (p, bg, ch)
        p, bg, ch = self.chains[key]
        return c, p, bg, ch

    def close(self):
        for c in self.ctxs.values():
            c.close()


@pytest.fixture(scope="module")
def frames():
    f = Frames()
    yield f
    f.close()


# ---- 1. every footprint, with partial edge granules ---------------------------------------------------------------------
# 70 = 8 * 8 + 6, 45 = 5 * 8 + 5; 61 = 7 * 8 + 5, 59 = 7 * 8 + 3: the last granule column and row are 6 and 5, 5 and 3
# pixels, no multiple of 8, 4 or 2.
EDGE_FRAMES = [("cubes", 70, 45), ("lowres", 70, 45), ("cubes", 61, 59), ("lowres", 61, 59)]


def _footprint_case(frames, kind, w, h, P, lanes, sshift, **kw):
    photons = bool(kw.get("use_photons"))
    pooled = not photons and kw.get("accel", pyrt.ACCEL_BVH) != pyrt.ACCEL_BRUTE
    assert sshift_rule(w * h, P, lanes, pooled, photons) == sshift
    assert sshift_rule(1, P, lanes, pooled, photons) == sshift  # a pass over fewer active pixels picks the same
    part, skipped = edge_tiles(w, h, sshift)
    assert part or skipped, "the frame has no clipped tile at this footprint"
    # the chain is rendered with the automatic samples-per-wave whatever the case forces: the image does not depend on it
    ctx, p0, bg, chain = frames.chain(kind, w, h, P, photons=photons, **kw)
    p = pyrt.Params.from_buffer_copy(p0)
    p.reserved[0] = lanes
    t, _ = pick_threshold(chain, bg, PASSES, P)
    K, *_ = check_frame(ctx, p, bg, chain, t, PASSES)
    assert len(np.unique(K)) >= 3


@gpu
@pytest.mark.parametrize("P", [1, 2, 8, 16, 32, 64, 3, 5, 6])
@pytest.mark.parametrize("kind,w,h", EDGE_FRAMES, ids=["%s%dx%d" % f for f in EDGE_FRAMES])
def test_every_footprint(frames, kind, w, h, P):
    _footprint_case(frames, kind, w, h, P, 0, SSHIFT[P])


def test_footprint_table_covers_all_seven():
    """The parametrisation reaches every kTileW / kTileH entry, and the two frame sizes clip every footprint both ways:
    tiles partly outside the image at all but 1x1, tiles wholly outside (skipped) at all but 8x8.  (partly, wholly) per
    sshift 0..6 — the 8x4 .. 4x4 tiles of 70x45's 6x5 edge granules are all at least partly inside:
        70x45   (14, 0) (20, 0) (29, 0) (40, 18) (35, 59) (0, 153) (0, 306)
        61x59   (15, 0) (22, 8) (30, 16) (45, 32) (60, 94) (59, 219) (0, 497)"""
    reached = {SSHIFT[P] for P in (1, 2, 8, 16, 32, 64, 3, 5, 6)} | {SSHIFT[4]}
    assert reached == set(range(7))
    assert [edge_tiles(70, 45, s) for s in range(7)] == [(14, 0), (20, 0), (29, 0), (40, 18), (35, 59), (0, 153), (0, 306)]
    assert [edge_tiles(61, 59, s) for s in range(7)] == [(15, 0), (22, 8), (30, 16), (45, 32), (60, 94), (59, 219), (0, 497)]
    for s in range(7):
        part, skipped = edge_tiles(61, 59, s)
        assert (part > 0 or s == 6) and (skipped > 0 or s == 0)
        assert sum(edge_tiles(70, 45, s)) > 0
    # what k_adapt_compact counts for the host: the tiles listed are the full grid's minus the skipped ones
    for w, h in ((70, 45), (61, 59), (197, 323)):
        gx, gy = adaptive_ref.granule_grid(w, h)
        for s, (tw, th) in enumerate(FOOTPRINT):
            listed = gx * gy * (8 // tw) * (8 // th) - edge_tiles(w, h, s)[1]
            assert listed == sum(-(-min(8, w - x) // tw) * -(-min(8, h - y) // th)
                                 for y in range(0, h, 8) for x in range(0, w, 8))
            assert listed <= 64 * gx * gy  # the tiles allocation


@gpu
@pytest.mark.parametrize("lanes", [1, 8, 64])
@pytest.mark.parametrize("kind,w,h", [("cubes", 70, 45), ("lowres", 61, 59)], ids=["cubes70x45", "lowres61x59"])
def test_forced_footprint_at_64_samples(frames, kind, w, h, lanes):
    """lanes_per_pixel on P = 64 (check_params accepts every value): 8x8, 4x2 and 1x1 tiles under the same chain."""
    _footprint_case(frames, kind, w, h, 64, lanes, LANES_SSHIFT[lanes])


@gpu
@pytest.mark.parametrize("case", ["brute", "photon"])
def test_footprint_2x2_on_the_other_branches(frames, case):
    """P = 16 through the branches of choose_sshift_px that the BVH path frames do not take."""
    if case == "brute":
        _footprint_case(frames, "cubes", 70, 45, 16, 0, 4, accel=pyrt.ACCEL_BRUTE)
    else:
        _footprint_case(frames, "cubes", 61, 59, 16, 0, 4, use_photons=1, k=10, photons_requested=3000)


# ---- 2. past 1,024 granules ---------------------------------------------------------------------------------------------
@gpu
def test_1024_granules_one_full_chunk(frames):
    ctx, p, bg, chain = frames.chain("cubes", 256, 256, 4)
    assert adaptive_ref.granule_grid(256, 256) == (32, 32) and 32 * 32 == CHUNK
    t, _ = pick_threshold(chain, bg, PASSES, 4)
    K, *_ = check_frame(ctx, p, bg, chain, t, PASSES)
    assert K.size == CHUNK and len(np.unique(K)) >= 3


@gpu
def test_1023_granules(frames):
    ctx, p, bg, chain = frames.chain("cubes", 248, 264, 4)
    assert adaptive_ref.granule_grid(248, 264) == (31, 33)
    t, _ = pick_threshold(chain, bg, PASSES, 4)
    K, *_ = check_frame(ctx, p, bg, chain, t, PASSES)
    assert K.size == CHUNK - 1 and len(np.unique(K)) >= 3


@gpu
def test_1025_granules_second_chunk_of_one(frames):
    """25 x 41 granules, both edges partial; the second chunk of k_adapt_compact holds granule 1,024 alone.

    Asserted from the rule before the device runs:
    (a) a pass in which granule 1,024 is active while one of the first 1,024 is retired: k_adapt_compact enters its
        second iteration with a base that is neither 0 nor 1,024 and writes the granule to list[base].  (On 1,025
        granules no pass can have MORE than 1,024 active ones with one retired; k_adapt_expand's second iteration
        runs in the passes before anything retires, with all 1,025 listed, which (c) asserts.)
    (b) a later pass with 1..1,023 active granules: one iteration, and a list shorter than the last pass's.
    (c) the first pass lists all 1,025 granules."""
    w, h = 197, 323
    assert adaptive_ref.granule_grid(w, h) == (25, 41) and (w % 8, h % 8) == (5, 3)
    ctx, p, bg, chain = frames.chain("cubes", w, h, 4)
    t, K, active = pick_chunk_threshold(chain, bg, PASSES, 4, need_full=False)
    mid, _, short = chunk_conditions(K, active)
    assert mid and K.reshape(-1)[CHUNK] > mid[0] and (K.reshape(-1)[:CHUNK] <= mid[0]).any()  # (a)
    assert short and short[-1] > mid[0] and 1 <= active[short[-1]] < CHUNK  # (b)
    assert active[0] == CHUNK + 1  # (c)
    Kg, *_ = check_frame(ctx, p, bg, chain, t, PASSES)
    assert np.array_equal(Kg, K)


@gpu
@pytest.mark.parametrize("P", [4, 1, 64])
def test_2145_granules_three_chunks(frames, P):
    """65 x 33 granules.  Asserted from the rule before the device runs:
    (a) a pass with more than 1,024 active granules of which one of the first 1,024 (row-major) is retired: both list
        kernels run a second iteration, k_adapt_compact with a base that is neither 0 nor 1,024;
    (b) a later pass with 1..1,023 active granules.
    P = 1 lists 8x8 tiles (one per granule), P = 64 1x1 tiles: 64 per full granule, the whole tiles allocation."""
    w, h = 520, 264
    assert adaptive_ref.granule_grid(w, h) == (65, 33) and 65 * 33 == 2145 and 2145 > 2 * CHUNK
    assert sshift_rule(w * h, P) == SSHIFT[P] == {4: 2, 1: 0, 64: 6}[P]
    ctx, p, bg, chain = frames.chain("cubes", w, h, P)
    t, K, active = pick_chunk_threshold(chain, bg, PASSES, P, need_full=True)
    _, full, short = chunk_conditions(K, active)
    Kf = K.reshape(-1)
    assert full and active[full[0]] > CHUNK and (Kf[:CHUNK] <= full[0]).any()  # (a)
    assert short and short[-1] > full[0] and 1 <= active[short[-1]] < CHUNK  # (b)
    Kg, *_ = check_frame(ctx, p, bg, chain, t, PASSES)
    assert np.array_equal(Kg, K)


# ---- 3. small edges -----------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("w,h", [(1, 1), (7, 3), (9, 1)], ids=["1x1", "7x3", "9x1"])
def test_frames_smaller_than_a_granule(frames, w, h):
    ctx, p, bg, chain = frames.chain("cubes", w, h, 4)
    n = (w + 7) // 8
    K, out, acc, spp, rep = check_frame(ctx, p, bg, chain, 0., PASSES)
    assert K.shape == (1, n) and (K == PASSES).all() and list(rep.active)[:PASSES] == [n] * PASSES
    assert np.array_equal(bits(acc), bits(chain[PASSES - 1]))
    # a huge threshold: every granule retires at max(min_passes, 2), min_passes = min(4, max_passes)
    K, *_ = check_frame(ctx, p, bg, chain, 1e30, PASSES)
    assert (K == 4).all()
    K, *_ = check_frame(ctx, p, bg, chain, 1e30, 3)
    assert (K == 3).all()
    K, *_ = check_frame(ctx, p, bg, chain, 1e30, PASSES, min_passes=2)
    assert (K == 2).all()


@gpu
def test_more_passes_than_the_report_stores(frames):
    """max_passes 70: the report keeps the first 64 active counts (the k < 64 guard of the pass loop) and counts all."""
    w, h, n = 24, 16, 70
    ctx, p, bg, chain = frames.chain("cubes", w, h, 1, passes=n)
    K, out, acc, spp, rep = check_frame(ctx, p, bg, chain, 0., n)
    assert (K == n).all() and rep.passes == n and rep.granules == 6
    assert list(rep.active) == [6] * 64
    assert rep.pixel_samples == n * w * h and (spp == n).all()
    assert np.array_equal(bits(acc), bits(chain[n - 1]))


@gpu
@pytest.mark.parametrize("kind,w,h,P", [("cubes", 197, 323, 4), ("cubes", 70, 45, 32)], ids=["197x323", "70x45P32"])
def test_device_form_on_these_shapes(frames, kind, w, h, P):
    torch = pytest.importorskip("torch")
    ctx, p, bg, chain = frames.chain(kind, w, h, P)
    if adaptive_ref.granule_grid(w, h)[0] * adaptive_ref.granule_grid(w, h)[1] > CHUNK:
        t, K, active = pick_chunk_threshold(chain, bg, PASSES, P, need_full=False)
    else:
        t, K = pick_threshold(chain, bg, PASSES, P)
        _, active = adaptive_ref.run_rule(chain, bg, P, t, PASSES)
    out, acc, spp, rep, st = ctx.render_adaptive(p, bg, t, PASSES)
    dev = torch.device("cuda:0")
    d_bg = torch.from_numpy(np.array(bg)).to(dev)
    d_acc = torch.full((h, w, 4), 7.0, dtype=torch.float32, device=dev)  # overwritten
    d_out = torch.empty((h, w, 3), dtype=torch.float32, device=dev)
    d_spp = torch.empty((h, w), dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    rep2, st2 = ctx.render_adaptive_device(p, d_bg.data_ptr(), d_acc.data_ptr(), d_out.data_ptr(), t, PASSES,
                                           d_spp=d_spp.data_ptr(), stream=stream, stats=True)
    torch.cuda.synchronize()
    got = (d_out.cpu().numpy(), d_acc.cpu().numpy(), d_spp.cpu().numpy().view(np.uint32), rep2, st2)
    check_result(p, bg, chain, K, active, got)  # the device form against the rule ...
    assert np.array_equal(bits(got[0]), bits(out)) and np.array_equal(bits(got[1]), bits(acc))  # ... and the host form
    assert np.array_equal(got[2], spp)
    assert rep2.passes == rep.passes and list(rep2.active) == list(rep.active)
    assert rep2.pixel_samples == rep.pixel_samples == st2.samples == st.samples
    # without report, stats or spp: the same accumulator and image once the stream has run
    d_acc2 = torch.full((h, w, 4), -3.0, dtype=torch.float32, device=dev)
    d_out2 = torch.empty_like(d_out)
    a = pyrt.make_adaptive(t, PASSES)
    rc = pyrt.amd().rt_render_adaptive_device(ctx._h, C.byref(p), C.byref(a), C.c_void_p(d_bg.data_ptr()),
                                              C.c_void_p(d_acc2.data_ptr()), C.c_void_p(d_out2.data_ptr()), None,
                                              C.c_void_p(stream), None, None)
    assert rc == 0
    torch.cuda.synchronize()
    assert np.array_equal(bits(d_out2.cpu().numpy()), bits(out))
    assert np.array_equal(bits(d_acc2.cpu().numpy()), bits(acc))


@gpu
def test_small_frame_after_a_large_one_on_the_same_scratch(frames):
    """520x264 and then 70x45 on one context: the second frame runs in the first one's scratch, whose list and tiles
    are not cleared between frames (2,145 stale granule indices and their tiles, all outside the small frame)."""
    big = (520, 264)
    ctx, p1, bg1, chain1 = frames.chain("cubes", 520, 264, 4)
    ctx2, p2, bg2, chain2 = frames.chain("cubes", 70, 45, 4, scene_wh=big)
    assert ctx2 is ctx
    t1, K1, _ = pick_chunk_threshold(chain1, bg1, PASSES, 4, need_full=True)
    t2, K2 = pick_threshold(chain2, bg2, PASSES, 4)
    Kg, *_ = check_frame(ctx, p1, bg1, chain1, t1, PASSES)
    assert np.array_equal(Kg, K1)
    Kg, *_ = check_frame(ctx, p2, bg2, chain2, t2, PASSES)
    assert np.array_equal(Kg, K2) and len(np.unique(K2)) >= 3
    # ... and the large one again after the small one
    Kg, *_ = check_frame(ctx, p1, bg1, chain1, t1, PASSES)
    assert np.array_equal(Kg, K1)
