"""tests/vcol_ref.py against the oracle alone (no GPU): the reference restates the colour, the products and the sums, so
its summation orders are pinned to the oracle's own frames by the two guarantees that need no coloured oracle — C1, the
mesh's albedo on every vertex, is orc.render of the plain scene, and C2, one colour per triangle on the vertex-split
scene, is orc.render of the scene with every triangle a mesh of its own — bit for bit, over both accelerators.  Then the
conditions that keep a kernel which ignores the colours, or interpolates them wrongly, from passing: the smooth colouring
changes more than vcol_ref.MIN_CHANGED of the rgb words, and a colouring with c1 != c0 on one triangle changes only
pixels whose paths touch that triangle."""
import numpy as np
import pytest

import vcol_ref
from vcol_ref import ALBEDO, FACES, SMOOTH

F32 = np.float32


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(ref, exp, what):
    assert np.array_equal(bits(ref["accum"]), bits(exp["accum"])), "accum " + what
    assert np.array_equal(bits(ref["out"]), bits(exp["out"])), "out " + what
    assert (ref["closest"], ref["shadow"]) == (exp["closest"], exp["shadow"]), what


@pytest.mark.parametrize("case", vcol_ref.CASES, ids=vcol_ref.case_id)
@pytest.mark.parametrize("brute", [False, True], ids=["bvh", "loop"])
def test_c1_the_materials_albedo_is_the_plain_frame(case, brute):
    """C1 on every case's scene, whatever its own colouring."""
    s = vcol_ref.case_scene(case)
    ref = vcol_ref.case_reference(case, brute) if case[6] == ALBEDO else vcol_ref.frame(
        s, vcol_ref.case_params(case), vcol_ref.albedo_colors(s), vcol_ref.case_background(case), brute)
    same(ref, vcol_ref.plain_frame(s, case, brute), vcol_ref.case_id(case))


@pytest.mark.parametrize("case", [c for c in vcol_ref.CASES if c[6] == FACES], ids=vcol_ref.case_id)
@pytest.mark.parametrize("brute", [False, True], ids=["bvh", "loop"])
def test_c2_one_colour_per_triangle_is_the_frame_of_one_mesh_per_triangle(case, brute):
    same(vcol_ref.case_reference(case, brute), vcol_ref.plain_frame(vcol_ref.case_triangle_scene(case), case, brute),
         vcol_ref.case_id(case))


def test_three_equal_colours_give_c0_exactly():
    rng = np.random.default_rng(5)
    col = rng.uniform(0, 2, (64, 3)).astype(F32)
    tv = np.stack([np.arange(64)] * 3, axis=1)
    u, v = rng.uniform(0, 1, 64).astype(F32), rng.uniform(0, 1, 64).astype(F32)
    assert np.array_equal(bits(vcol_ref.interpolate(col, tv, u, v)), bits(col))
    # ... and the weighted form the definition rules out does not
    w = (F32(1) - u - v)[:, None]
    other = (w * col + u[:, None] * col + v[:, None] * col).astype(F32)
    assert not np.array_equal(bits(other), bits(col))


def test_the_smooth_colouring_changes_the_frame():
    """The discrimination floor: the share of rgb words a SMOOTH case changes against the uncoloured frame (the mesh's
    albedo on every vertex, which is the plain frame by C1); MIN_CHANGED is half the smallest share."""
    shares = {}
    for case in vcol_ref.CASES:
        if case[6] != SMOOTH:
            continue
        s = vcol_ref.case_scene(case)
        plain = vcol_ref.plain_frame(s, case)
        shares[vcol_ref.case_id(case)] = vcol_ref.changed_rgb_words(vcol_ref.case_reference(case)["accum"], plain["accum"])
        # the rays, hence .w and both counts, are the plain frame's
        ref = vcol_ref.case_reference(case)
        assert np.array_equal(bits(ref["accum"][..., 3]), bits(plain["accum"][..., 3]))
        assert (ref["closest"], ref["shadow"]) == (plain["closest"], plain["shadow"])
    for k, v in shares.items():
        print("%-48s %.4f" % (k, v))
    assert min(shares.values()) > vcol_ref.MIN_CHANGED, shares
    assert vcol_ref.MIN_CHANGED >= 0.45 * min(shares.values()), "the floor is half the smallest share: %r" % shares


def test_some_colours_are_zero_and_some_above_one():
    for case in vcol_ref.CASES:
        if case[6] == SMOOTH:
            c = vcol_ref.case_colors(case)
            assert (c == 0).all(axis=1).any() and (c > 1).any() and np.isfinite(c).all(), vcol_ref.case_id(case)


@pytest.mark.parametrize("case", [c for c in vcol_ref.CASES if c[6] == ALBEDO][:2], ids=vcol_ref.case_id)
def test_a_gradient_on_one_triangle_changes_only_pixels_that_touch_it(case):
    """From C1's colouring, one vertex of the most-touched triangle takes another colour in a split copy of the scene
    (so that no other triangle shares the vertex): c1 != c0 there.  Pixels none of whose paths shade a vertex on that
    triangle keep their bits; some pixel that touches it changes."""
    s = vcol_ref.split_scene(vcol_ref.case_scene(case))
    p, bg = vcol_ref.case_params(case), vcol_ref.case_background(case)
    col = vcol_ref.albedo_colors(s)
    base = vcol_ref.frame(s, p, col, bg)
    t = int(np.argmax(base["touched"].sum(axis=(0, 1))))
    assert base["touched"][..., t].any()
    col = col.copy()
    col[3 * t + 1] = (col[3 * t + 1] * F32(0.25) + F32(0.6)).astype(F32)
    got = vcol_ref.frame(s, p, col, bg)
    assert np.array_equal(got["touched"], base["touched"]) and (got["closest"], got["shadow"]) == (base["closest"], base["shadow"])
    changed = (bits(got["accum"]) != bits(base["accum"])).any(axis=-1)
    assert not (changed & ~base["touched"][..., t]).any()
    assert changed.any()
