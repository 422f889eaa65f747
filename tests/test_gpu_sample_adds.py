"""The ordered sample adds of the render kernels (render_tile): a wave runs 1..64 samples of a pixel side by side and
hands them through LDS to the lanes that add, whose running sums are loaded from the accumulator at the tile's start and
stored at its end.  However the adds are split over lanes, every channel of every pixel must be the float32 sum of its
samples in sample order, on top of what the accumulator held — the oracle's bits — at every samples-per-wave setting,
for sample counts around a group's size, on tiles that overhang the image, over two passes and on a pre-filled
accumulator."""
import numpy as np
import pytest

import orc
import pyrt

pytestmark = pytest.mark.gpu

SIZES = ((20, 12), (5, 3))  # (at 5 x 3 the one wave tile is mostly outside the image)
LPPS = (1, 2, 4, 8, 16, 32, 64)
SPPS = (1, 15, 16, 17, 33)
SEED = 5


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def wide_scene(w, h):
    """The cubes scene through a camera three times as wide and high about the same axis: the box fills the middle of
    the frame and the border sees background, so the channel that counts primary hits gets 0 and 1 increments."""
    a = pyrt.Scene("cubes", w, h).arrays()
    cam = a["camera"].copy()
    centre = cam[1] + np.float32(0.5) * cam[2] + np.float32(0.5) * cam[3]
    cam[2] *= np.float32(3)
    cam[3] *= np.float32(3)
    cam[1] = centre - np.float32(0.5) * cam[2] - np.float32(0.5) * cam[3]
    return pyrt.ArrayScene(a["pos"], a["nrm"], a["tri"], a["tri_begin"], a["vtx_begin"], a["materials"], a["lights"], cam)


@pytest.fixture(scope="module")
def frames():
    """Per size: the scene, its context, and the oracle's accumulators by sample count (computed once, never changed)."""
    out = {}
    for (w, h) in SIZES:
        s = wide_scene(w, h)
        out[(w, h)] = dict(scene=s, ctx=pyrt.Context(s), ref={})
    yield out
    for f in out.values():
        f["ctx"].close()


def oracle(f, w, h, spp):
    if spp not in f["ref"]:
        _, acc, _ = orc.render(f["scene"], pyrt.make_params(w, h, spp, seed=SEED), math_mode=orc.MATH_DET)
        acc.setflags(write=False)
        f["ref"][spp] = acc
    return f["ref"][spp]


def test_the_camera_sees_background_in_part_of_the_frame(frames):
    for (w, h) in SIZES:
        hits = oracle(frames[(w, h)], w, h, 33)[..., 3]
        assert (hits == 33).any() and (hits < 33).any() and ((hits > 0) & (hits < 33)).any(), (w, h)


@pytest.mark.parametrize("spp", SPPS)
@pytest.mark.parametrize("lpp", LPPS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_accumulator_equals_the_oracle(frames, size, lpp, spp):
    w, h = size
    f = frames[size]
    _, acc, st = f["ctx"].render(pyrt.make_params(w, h, spp, seed=SEED, lanes_per_pixel=lpp))
    assert st.samples == w * h * spp
    ref = oracle(f, w, h, spp)
    for c in range(4):
        assert np.array_equal(bits(acc[..., c]), bits(ref[..., c])), ("channel", c)


@pytest.mark.parametrize("lpp", LPPS)
def test_two_passes_equal_one(frames, lpp):
    """Samples 0-7, then 8-18, into the same accumulator: the second pass must go on from what the first one stored."""
    w, h = SIZES[0]
    f = frames[SIZES[0]]
    bg = pyrt.background(w, h)
    acc = np.zeros((h, w, 4), np.float32)
    for (b, c) in ((0, 8), (8, 11)):
        f["ctx"].render_passes(pyrt.make_params(w, h, 19, seed=SEED, spp_begin=b, spp_count=c, lanes_per_pixel=lpp), bg, acc)
    _, one, _ = f["ctx"].render(pyrt.make_params(w, h, 19, seed=SEED, lanes_per_pixel=lpp))
    assert np.array_equal(bits(acc), bits(one))
    _, ref, _ = orc.render(f["scene"], pyrt.make_params(w, h, 19, seed=SEED), math_mode=orc.MATH_DET)
    assert np.array_equal(bits(acc), bits(ref))


@pytest.fixture(scope="module")
def prefilled(frames):
    """A non-zero accumulator plus 17 samples, added one by one in float32: the oracle renders every sample alone
    (spp_begin = i, spp_count = 1: 0 + v is v exactly), numpy adds them in sample order."""
    w, h = SIZES[0]
    f = frames[SIZES[0]]
    rng = np.random.default_rng(11)
    pattern = rng.uniform(0.25, 3.0, (h, w, 4)).astype(np.float32)
    want = pattern.copy()
    for i in range(17):
        _, one, _ = orc.render(f["scene"], pyrt.make_params(w, h, 17, seed=SEED, spp_begin=i, spp_count=1), math_mode=orc.MATH_DET)
        want = (want + one).astype(np.float32)
    pattern.setflags(write=False)
    want.setflags(write=False)
    return pattern, want


@pytest.mark.parametrize("lpp", LPPS)
def test_prefilled_accumulator_is_added_to(frames, prefilled, lpp):
    import torch
    w, h = SIZES[0]
    pattern, want = prefilled
    acc = torch.from_numpy(pattern.copy()).cuda()
    frames[SIZES[0]]["ctx"].render_device(pyrt.make_params(w, h, 17, seed=SEED, lanes_per_pixel=lpp), acc.data_ptr(),
                                          torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = acc.cpu().numpy()
    assert not np.array_equal(bits(want), bits(pattern))
    assert np.array_equal(bits(got), bits(want))
