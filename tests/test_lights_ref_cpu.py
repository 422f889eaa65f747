"""tests/lights_ref.py on the oracle alone (no GPU): for every case of the table the frame "with only these lights lit" —
the other lights' colours zeroed — is finite, casts the full frame's rays, counts the full frame's hits, IS the full
frame for the mask of all lights and is black for the empty mask; and any two different masks of a case differ in more
than a fifth of their rgb words, which is what keeps a kernel that ignores or swaps masks from passing
tests/test_gpu_lights.py.  The oracle's exhaustive loop gives the same frames as its BVH."""
import itertools

import numpy as np
import pytest

import lights_ref
import orc


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def masks_of(c):
    """The case's masks, the empty one and the one of all lights."""
    return sorted(set(lights_ref.case_masks(c)) | {0, lights_ref.all_mask(lights_ref.case_scene(c))})


@pytest.mark.parametrize("case", lights_ref.CASES, ids=lights_ref.case_id)
def test_masked_frames_share_the_full_frames_rays(case):
    s = lights_ref.case_scene(case)
    _, facc, fst = orc.render(s, lights_ref.case_params(case), math_mode=orc.MATH_DET, accel=orc.ACCEL_OBVH)
    for m in masks_of(case):
        f = lights_ref.masked_frame(case, m)
        assert np.isfinite(f["accum"]).all() and np.isfinite(f["out"]).all(), bin(m)
        assert (f["closest"], f["shadow"]) == (fst.rays_closest, fst.rays_shadow), bin(m)
        assert (bits(f["accum"][..., 3]) == bits(facc[..., 3])).all(), bin(m)
    assert fst.rays_closest > 0 and fst.rays_shadow > 0 and fst.rays_shadow % lights_ref.n_lights(s) == 0
    assert (bits(lights_ref.masked_frame(case, lights_ref.all_mask(s))["accum"]) == bits(facc)).all()
    assert (bits(lights_ref.masked_frame(case, 0)["accum"][..., :3]) == 0).all()


@pytest.mark.parametrize("case", lights_ref.CASES, ids=lights_ref.case_id)
def test_different_masks_give_different_frames(case):
    for a, b in itertools.combinations(masks_of(case), 2):
        share = lights_ref.changed_rgb_words(lights_ref.masked_frame(case, a)["accum"], lights_ref.masked_frame(case, b)["accum"])
        print("%s: masks %s and %s differ in %.3f of their rgb words" % (lights_ref.case_id(case), bin(a), bin(b), share))
        assert share > lights_ref.MIN_CHANGED, (bin(a), bin(b), share)


@pytest.mark.parametrize("case", lights_ref.CASES[2::4], ids=lights_ref.case_id)
def test_the_exhaustive_loop_gives_the_same_frames(case):
    for m in lights_ref.case_masks(case):
        a, b = lights_ref.masked_frame(case, m), lights_ref.masked_frame(case, m, brute=True)
        assert (bits(a["accum"]) == bits(b["accum"])).all() and (bits(a["out"]) == bits(b["out"])).all()
        assert (a["closest"], a["shadow"]) == (b["closest"], b["shadow"])


def test_the_reference_stacks_the_masks_in_table_order():
    a, b = lights_ref.CASES[0], lights_ref.CASES[1]
    assert a[:6] == b[:6] and sorted(a[6]) == sorted(b[6]) and a[6] != b[6]
    ra, rb = lights_ref.case_reference(a), lights_ref.case_reference(b)
    for j, m in enumerate(b[6]):
        assert (bits(rb["accum"][j]) == bits(ra["accum"][a[6].index(m)])).all()
    assert ra["accum"].shape == (3, 16, 16, 4) and ra["out"].shape == (3, 16, 16, 3)
    assert (ra["closest"], ra["shadow"]) == (rb["closest"], rb["shadow"])
