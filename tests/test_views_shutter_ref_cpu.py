"""The case table of rt_render_views_shutter on the CPU oracle alone (tests/views_shutter_ref.py): the condition that keeps
tests/test_gpu_views_shutter.py from passing on a kernel that ignores the per-view table, or reads another view's row of it.
Every view's expectation differs from the same view rendered with each other view's shutter record in more than a quarter
of its accumulator words; the no-optics view is the oracle's own still frame of its camera; and the table has the shape
the GPU tests rely on."""
import numpy as np
import pytest

import lens_ref
import orc
import views_shutter_ref as vs

SHARE = 0.25


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_the_table_has_the_shape_the_gpu_tests_rely_on():
    assert len(vs.CASES) >= 6
    assert {(c[2], c[3]) for c in vs.CASES} == {(13, 9), (16, 16)}
    assert {tuple(c[4].values()) for c in vs.CASES} == {(1,), (4,), (7,), (7, 3, 4)}
    assert {(c[5], c[6]) for c in vs.CASES} >= {(vs.RAY, 1), (vs.PATH, 1), (vs.PATH, 2), (vs.PATH, 3)}
    assert {c[7] for c in vs.CASES} == {False, True}
    assert {(c[0], c[1]) for c in vs.CASES} >= {("cubes", False), ("lowres", False), ("lowres", True)}
    assert sum(c[11] is not None for c in vs.CASES) * 2 == len(vs.CASES)
    kinds = set()
    for c in vs.CASES:
        assert len(c[8]) == vs.N_VIEWS and "none" in c[8] and len(set(c[8])) == vs.N_VIEWS
        kinds |= set(c[8])
        if c[11] is not None:
            assert len(set(c[11])) == vs.N_VIEWS
        recs = vs.case_records(c)
        for a in range(vs.N_VIEWS):
            for b in range(a + 1, vs.N_VIEWS):
                assert bytes(vs.shutter_of(recs[a])) != bytes(vs.shutter_of(recs[b])), "two views share a record"
        cams = vs.case_cameras(c)
        assert np.array_equal(bits(cams[0]), bits(np.asarray(vs.case_scene(c).arrays()["camera"], np.float32).reshape(4, 3)))
    assert kinds == {"none", "lens", "move_lens", "turn"}


@pytest.mark.parametrize("case", vs.CASES, ids=vs.case_id)
def test_every_view_needs_its_own_record(case):
    for j in range(vs.N_VIEWS):
        own = vs.view_expected(case, j)["accum"]
        for r in range(vs.N_VIEWS):
            if r == j:
                continue
            share = vs.changed_words(own, vs.view_expected(case, j, r)["accum"])
            assert share > SHARE, "view %d (%s) under view %d's record (%s) changes only %.3f of its accumulator words" % (
                j, case[8][j], r, case[8][r], share)


@pytest.mark.parametrize("case", vs.CASES, ids=vs.case_id)
def test_the_no_optics_view_is_the_oracles_still_frame(case):
    j = vs.none_view(case)
    ref = vs.view_expected(case, j)
    bg = vs.case_background(case)
    out, acc, st = orc.render(vs.with_camera(vs.case_scene(case), vs.case_cameras(case)[j]), vs.view_params(case, j),
                              math_mode=orc.MATH_DET, accel=vs.case_accel(case), bg=bg)
    assert np.array_equal(bits(ref["accum"]), bits(acc))
    assert (ref["closest"], ref["shadow"]) == (st.rays_closest, st.rays_shadow)
    if lens_ref.sample_range(vs.view_params(case, j)) == (0, case[4]["spp"]):
        assert np.array_equal(bits(ref["out"]), bits(out))
