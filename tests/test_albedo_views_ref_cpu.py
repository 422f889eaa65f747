"""tests/albedo_views_ref.py against the oracle alone (no GPU), before it judges anything: with X3's data — texels or
colours equal to each mesh's albedo, or no texture at all — it is views_shutter_ref's construction (shutter_ref.expected:
one oracle row per pixel and sample) bit for bit, and with X4's per-face data that construction on the scene with every
triangle a mesh of its own; with a still record and one view it is tex_ref.frame / vcol_ref.frame.  Then the conditions
that keep a kernel which ignores the surface, or the optics, from passing: every mixed case differs from the untextured
multi-view shutter frame and from the still textured frame in measured shares of its rgb words (printed), whose halves
are the floors the GPU test uses; and the mixed cases between them sample every texture of tex_ref.MIXED_TEXTURES."""
import numpy as np
import pytest

import albedo_views_ref as avr
import tex_ref
import vcol_ref
from albedo_views_ref import COL, TEX
from tex_ref import T_MIXED

EXACT = [c for c in avr.CASES if c not in avr.MIXED]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(ref, exp, what):
    assert np.array_equal(bits(ref["accum"]), bits(exp["accum"])), "accum " + what
    assert np.array_equal(bits(ref["out"]), bits(exp["out"])), "out " + what
    assert (ref["closest"], ref["shadow"]) == (exp["closest"], exp["shadow"]), what


@pytest.mark.parametrize("case", EXACT, ids=avr.case_id)
def test_albedo_data_and_per_face_data_are_the_multi_view_shutter_expectation(case):
    """X3's and X4's data: the oracle's rows under the same views and records, whatever the surface's form."""
    brute = avr.CASES.index(case) % 2 == 1
    same(avr.case_reference(case, brute), avr.plain_reference(case, brute), avr.case_id(case))


@pytest.mark.parametrize("case", avr.MIXED, ids=avr.case_id)
def test_a_still_record_and_one_view_are_the_single_view_references(case):
    """View 0 is the scene's own camera: under its "none" record and its seed the construction is tex_ref.frame /
    vcol_ref.frame of the scene — accumulator, both ray counts and the first-hit albedo sums."""
    s, p = avr.case_scene(case), avr.view_params(case, 0)
    cam = avr.case_cameras(case)[0]
    assert np.array_equal(bits(cam), bits(np.asarray(s.arrays()["camera"], np.float32).reshape(4, 3)))
    got = avr.view_frame(s, cam, avr.record("none", cam, case[8]), p, avr.case_albedo_fn(case))
    if case[6][0] == TEX:
        exp = tex_ref.frame(s, p, avr.case_surface(case), touched=False)
    else:
        exp = vcol_ref.frame(s, p, avr.case_surface(case), touched=False)
    for k in ("accum", "albedo"):
        assert np.array_equal(bits(got[k]), bits(exp[k])), (k, avr.case_id(case))
    assert (got["closest"], got["shadow"]) == (exp["closest"], exp["shadow"])


def test_every_mixed_case_shows_its_surface_and_its_optics():
    """The shares of rgb words by which a mixed case differs from the untextured frame of the same views and records,
    and from the still frame of the same surface; the floors are half the smallest of each."""
    surface, optics = {}, {}
    for case in avr.MIXED:
        ref = avr.case_reference(case)
        surface[avr.case_id(case)] = avr.changed_rgb_words(ref["accum"], avr.plain_reference(case)["accum"])
        optics[avr.case_id(case)] = avr.changed_rgb_words(ref["accum"], avr.case_reference(case, still=True)["accum"])
        print("%-72s surface %.3f  optics %.3f" % (avr.case_id(case), surface[avr.case_id(case)], optics[avr.case_id(case)]))
        # the hit counts are the generator's alone
        assert np.array_equal(bits(ref["accum"][..., 3]), bits(avr.plain_reference(case)["accum"][..., 3]))
    for name, shares, floor in (("surface", surface, avr.MIN_CHANGED_SURFACE), ("optics", optics, avr.MIN_CHANGED_OPTICS)):
        low = min(shares, key=shares.get)
        print("smallest %s share: %.4f (%s); floor %.4f" % (name, shares[low], low, floor))
        assert shares[low] > 0, low
        assert 0.95 * shares[low] / 2 <= floor <= shares[low] / 2, (name, shares[low], floor)


def test_the_mixed_cases_cover_every_texture_both_filters_every_wrap_pair_and_the_untextured_mesh():
    used, none = set(), False
    for case in avr.MIXED:
        if case[6] == (TEX, T_MIXED):
            which = avr.case_surface(case)["mesh_texture"]
            used |= {int(k) for k in which if k != tex_ref.NONE}
            none |= bool((which == tex_ref.NONE).any())
    assert used == set(range(len(tex_ref.MIXED_TEXTURES))) and none
    specs = [tex_ref.MIXED_TEXTURES[k] for k in used]
    assert {s[3] for s in specs} == {tex_ref.NEAREST, tex_ref.BILINEAR}
    assert {(s[1], s[2]) for s in specs} == {(a, b) for a in (tex_ref.REPEAT, tex_ref.CLAMP) for b in (tex_ref.REPEAT, tex_ref.CLAMP)}
    assert any(c[6][0] == COL for c in avr.MIXED)


def test_the_case_table_covers_what_it_says():
    assert {avr.n_views(c) for c in avr.CASES} == {1, 2, 3}
    assert {(c[1], c[2]) for c in avr.CASES} == {(13, 9), (16, 16)}
    assert {k for c in avr.CASES for k in c[7]} == {"none", "lens", "turn_lens"}
    assert {(c[4], c[5]) for c in avr.MIXED} >= {(avr.RAY, 1), (avr.PATH, 1), (avr.PATH, 2), (avr.PATH, 3)}
    assert {tuple(c[3].values()) for c in avr.MIXED} == {(1,), (4,), (7,), (7, 3, 4)}
    assert any(c[9] is None for c in avr.MIXED) and any(c[9] is not None for c in avr.MIXED)
    for c in avr.CASES:  # (the turned end differs from the open end, and every lens is one)
        for kind, rec, cam in zip(c[7], avr.case_records(c), avr.case_cameras(c)):
            assert (rec["aperture"] > 0) == (kind != "none")
            assert np.array_equal(rec["camera_close"], cam) == (kind != "turn_lens")
