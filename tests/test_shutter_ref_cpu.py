"""shutter_ref.py against the oracle and against itself, without a GPU: a still shutter's construction is the oracle's frame
under the camera of that time, a camera that does not move gives the oracle's own frame, the times lie in the exposure
and fill it, and every case test_gpu_shutter.py runs meets its change condition on the oracle alone."""
import numpy as np
import pytest

import lens_ref
import orc
import pyrt
import shutter_ref

F32 = np.float32


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


STILL = [("cubes", False, lens_ref.SPP4, lens_ref.PATH, 3, "large"), ("cubes", True, lens_ref.SPP7_34, lens_ref.PATH, 2, "turn"),
         ("lowres", True, lens_ref.SPP1, lens_ref.RAY, 1, "small")]


@pytest.mark.parametrize("s", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("name,opened,rng,mode,depth,move", STILL)
def test_a_still_shutter_is_the_oracles_frame_under_the_camera_of_that_time(name, opened, rng, mode, depth, move, s):
    """(a) open == close == s: every t is s, and the chained rows are orc.render's frame of the scene with camera C(s), bit
    for bit, ray counts included."""
    scene = lens_ref.scene(name, opened, 13, 9)
    args = dict(rng)
    p = pyrt.make_params(13, 9, args.pop("spp"), mode=mode, max_depth=depth, seed=shutter_ref.SEED, **args)
    A = np.asarray(scene.arrays()["camera"], F32).reshape(4, 3)
    B = shutter_ref.MOVES[move](A)
    assert (shutter_ref.times(p, s, s) == F32(s)).all()
    got = shutter_ref.expected(scene, B, p, s, s)
    acc, st = shutter_ref.still_reference(scene, shutter_ref.camera_at(A, B, s), p, False)
    assert np.array_equal(bits(acc), bits(got["accum"]))
    assert (got["closest"], got["shadow"]) == (st.rays_closest, st.rays_shadow)


def test_a_camera_that_does_not_move_gives_the_oracles_own_frame():
    """(b) B == A: D is zero, every sample's camera is A whatever its time, and the frame is the oracle's."""
    scene = lens_ref.scene("cubes", True, 13, 9)
    p = pyrt.make_params(13, 9, 4, mode=lens_ref.PATH, max_depth=3, seed=shutter_ref.SEED)
    A = np.asarray(scene.arrays()["camera"], F32).reshape(4, 3)
    got = shutter_ref.expected(scene, A, p, 0.0, 1.0)
    _, acc, st = orc.render(scene, p, math_mode=orc.MATH_DET, accel=orc.ACCEL_OBVH)
    assert np.array_equal(bits(acc), bits(got["accum"]))
    assert (got["closest"], got["shadow"]) == (st.rays_closest, st.rays_shadow)


@pytest.mark.parametrize("op,cl", [(0.0, 1.0), (0.25, 0.5), (0.0, 0.0), (1.0, 1.0), (0.3, 0.3)])
def test_times_lie_in_the_exposure_and_fill_it(op, cl):
    """(c) t in [open, close]; over 16 x 16 x 7 draws both tenths at the ends of the interval are reached and the mean is
    the middle (a uniform draw: the standard error of the mean of 1,792 draws is 0.7 % of the width); a sample range
    draws the whole frame's values."""
    p = pyrt.make_params(16, 16, 7, seed=shutter_ref.SEED)
    t = shutter_ref.times(p, op, cl)
    assert t.dtype == F32 and (t >= F32(op)).all() and (t <= F32(cl)).all()
    wd = cl - op
    if wd > 0:
        assert t.min() < op + 0.1 * wd and t.max() > cl - 0.1 * wd
        assert abs(float(t.mean()) - (op + cl) / 2) < 0.05 * wd
        assert len(np.unique(t)) > 0.99 * t.size
    q = pyrt.make_params(16, 16, 7, seed=shutter_ref.SEED, spp_begin=3, spp_count=4)
    assert np.array_equal(shutter_ref.times(q, op, cl), t[:, :, 3:7])


def test_the_interpolated_camera_is_stated_component_by_component():
    A = np.arange(1, 13, dtype=F32).reshape(4, 3) / F32(7)
    B = (A * F32(1.5) + F32(0.25)).astype(F32)
    t = F32(0.37)
    C = shutter_ref.camera_at(A, B, t)
    for r in range(4):
        for k in range(3):
            assert C[r, k] == F32(A[r, k] + F32(t * F32(B[r, k] - A[r, k])))
    assert np.array_equal(shutter_ref.camera_at(A, B, 0.0), A)
    many = shutter_ref.camera_at(A, B, np.array([[0.0, 0.37]], F32))
    assert many.shape == (1, 2, 4, 3) and np.array_equal(many[0, 1], C) and np.array_equal(many[0, 0], A)


def test_a_lens_at_rest_is_the_lens_references_rays():
    """open == close == 0 with an aperture: the rays are lens_ref.lens_rays' (G3 on the references)."""
    scene = lens_ref.scene("cubes", False, 13, 9)
    p = pyrt.make_params(13, 9, 4, seed=shutter_ref.SEED)
    A = np.asarray(scene.arrays()["camera"], F32).reshape(4, 3)
    B = shutter_ref.MOVES["turn"](A)
    o, F = shutter_ref.shutter_rays(A, B, p, 0.0, 0.0, lens_ref.APERTURES[0], lens_ref.FOCUS[1])
    lo, lF = lens_ref.lens_rays(A, p, lens_ref.APERTURES[0], lens_ref.FOCUS[1])
    assert np.array_equal(bits(o), bits(lo)) and np.array_equal(bits(F), bits(lF))


def test_the_turned_camera_keeps_its_shape():
    A = np.asarray(lens_ref.scene("cubes", False, 13, 9).arrays()["camera"], F32).reshape(4, 3)
    B = shutter_ref.turned(A, shutter_ref.TURN_DEGREES)
    assert np.array_equal(B[0], A[0]) and np.allclose(B[3], A[3], atol=1e-6)
    for k in (1, 2):
        a, b = (A[k] - (A[0] if k == 1 else 0)).astype(np.float64), (B[k] - (B[0] if k == 1 else 0)).astype(np.float64)
        assert abs(np.linalg.norm(a) - np.linalg.norm(b)) < 1e-5
    h = float(A[2].astype(np.float64) @ B[2].astype(np.float64)) / float(np.linalg.norm(A[2]) * np.linalg.norm(B[2]))
    assert abs(np.degrees(np.arccos(h)) - shutter_ref.TURN_DEGREES) < 1e-2


@pytest.mark.parametrize("c", shutter_ref.CASES, ids=shutter_ref.case_id)
def test_every_case_meets_its_change_condition(c):
    """(d) The condition test_gpu_shutter.py holds the library to, on the oracle alone: the frame differs from the still
    frames at A and at B in at least half of the accumulator words (a quarter for one-sample open frames)."""
    ref, (fa, fb) = shutter_ref.case_reference(c), shutter_ref.case_stills(c)
    sa, sb = shutter_ref.changed_words(ref["accum"], fa), shutter_ref.changed_words(ref["accum"], fb)
    print("%s: differs from the still frame at A in %.3f, at B in %.3f of the words" % (shutter_ref.case_id(c), sa, sb))
    assert sa >= shutter_ref.case_threshold(c) and sb >= shutter_ref.case_threshold(c)
    s0, s1 = lens_ref.sample_range(shutter_ref.case_params(c))
    assert ref["closest"] >= fa.shape[0] * fa.shape[1] * (s1 - s0)  # (every sample casts its primary ray)
