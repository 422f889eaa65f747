"""tests/tex_ref.py against the oracle alone (no GPU): the reference restates the sampler, the products and the sums, so
its summation orders are pinned to the oracle's own frames by the two guarantees that need no textured oracle — T1, no
texture at all or texels equal to the mesh's albedo, is orc.render of the plain scene, and T2, the 3n x 1 texture of one
colour per triangle on the vertex-split scene, is orc.render of the scene with every triangle a mesh of its own — bit for
bit, over both accelerators.  Then the sampler's exact points, and the conditions that keep a kernel which ignores the
textures, or samples them wrongly, from passing: the mixed texturing changes more than tex_ref.MIN_CHANGED of the rgb
words, and other texels on one mesh change only pixels whose paths touch that mesh."""
import numpy as np
import pytest

import tex_ref
from tex_ref import BILINEAR, CLAMP, NEAREST, REPEAT, T_ALBEDO, T_FACES, T_MIXED, T_NONE

F32 = np.float32
FILTERS = (NEAREST, BILINEAR)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(ref, exp, what):
    assert np.array_equal(bits(ref["accum"]), bits(exp["accum"])), "accum " + what
    assert np.array_equal(bits(ref["out"]), bits(exp["out"])), "out " + what
    assert (ref["closest"], ref["shadow"]) == (exp["closest"], exp["shadow"]), what


# ---- T1 and T2 against the oracle's frames ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", tex_ref.CASES, ids=tex_ref.case_id)
@pytest.mark.parametrize("brute", [False, True], ids=["bvh", "loop"])
def test_t1_no_texture_and_albedo_texels_are_the_plain_frame(case, brute):
    """T1 on every case's scene, whatever its own texturing: every mesh RT_TEX_NONE (even cases) or textured with its
    albedo (odd cases, and the T_ALBEDO cases themselves)."""
    s = tex_ref.case_scene(case)
    if case[6] in (T_NONE, T_ALBEDO):
        ref = tex_ref.case_reference(case, brute)
    else:
        kind = T_NONE if tex_ref.CASES.index(case) % 2 == 0 else T_ALBEDO
        ref = tex_ref.frame(s, tex_ref.case_params(case), tex_ref.texture_set(s, kind), tex_ref.case_background(case), brute)
    same(ref, tex_ref.plain_frame(s, case, brute), tex_ref.case_id(case))


@pytest.mark.parametrize("case", [c for c in tex_ref.CASES if c[6] == T_FACES], ids=tex_ref.case_id)
@pytest.mark.parametrize("brute", [False, True], ids=["bvh", "loop"])
def test_t2_the_strip_texture_is_the_frame_of_one_mesh_per_triangle(case, brute):
    same(tex_ref.case_reference(case, brute), tex_ref.plain_frame(tex_ref.case_face_colors(case)[1], case, brute),
         tex_ref.case_id(case))


def test_t2_sets_use_both_filters_and_sample_only_the_triangles_own_texels():
    """The T_FACES sets hold the strip under both filters, and whichever texel the rounding of x picks holds the colour."""
    for case in tex_ref.CASES:
        if case[6] != T_FACES:
            continue
        t = tex_ref.case_textures(case)
        assert {x[3] for x in t["textures"]} == set(FILTERS)
        nt = len(t["uv"]) // 3
        face = t["textures"][0][0].reshape(nt, 3, 3)[:, 0]
        for tex in t["textures"]:
            got = tex_ref.sample(tex, t["uv"][::3, 0], t["uv"][::3, 1])
            assert np.array_equal(bits(got), bits(face)), tex_ref.case_id(case)


# ---- the sampler's exact points --------------------------------------------------------------------------------------------
def ramp(w, h):
    """Distinct dyadic texels: texel (j, i) is (i, j, 8 j + i) / 4."""
    j, i = np.mgrid[0:h, 0:w]
    return np.stack([i, j, 8 * j + i], axis=-1).astype(F32) / F32(4)


def at(tex, s, t):
    return tex_ref.sample(tex, np.array([s], F32), np.array([t], F32))[0]


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("wrap", (REPEAT, CLAMP))
def test_a_texel_centre_returns_that_texel(filt, wrap):
    """Power-of-two sizes, dyadic centres (i + 0.5) / W: x is exact, fx = fy = 0."""
    texels = ramp(8, 4)
    tex = (texels, wrap, wrap, filt)
    for j in range(4):
        for i in range(8):
            assert np.array_equal(at(tex, (i + 0.5) / 8, (j + 0.5) / 4), texels[j, i]), (i, j)


def test_the_midpoint_of_two_texels_is_t0_plus_half_the_difference():
    texels = np.random.default_rng(3).uniform(0, 1, (4, 8, 3)).astype(F32)
    tex = (texels, REPEAT, REPEAT, BILINEAR)
    for i in range(7):  # between columns i and i + 1 of row 2: s = (i + 1) / 8, t = 2.5 / 4
        exp = (texels[2, i] + F32(0.5) * (texels[2, i + 1] - texels[2, i])).astype(F32)
        assert np.array_equal(bits(at(tex, (i + 1) / 8, 2.5 / 4)), bits(exp)), i
    for j in range(3):  # between rows j and j + 1 of column 5
        exp = (texels[j, 5] + F32(0.5) * (texels[j + 1, 5] - texels[j, 5])).astype(F32)
        assert np.array_equal(bits(at(tex, 5.5 / 8, (j + 1) / 4)), bits(exp)), j
    # ... and the nearest filter at the same points takes the texel the edge opens
    near = (texels, REPEAT, REPEAT, NEAREST)
    assert np.array_equal(at(near, 3 / 8, 2.5 / 4), texels[2, 3])


@pytest.mark.parametrize("filt", FILTERS)
def test_repeat_is_periodic_in_whole_units_at_dyadic_points(filt):
    texels = np.random.default_rng(4).uniform(0, 1, (4, 8, 3)).astype(F32)
    tex = (texels, REPEAT, REPEAT, filt)
    for s, t in ((0.3125, 0.625), (0.0, 0.0), (0.96875, 0.125), (0.0625, 0.9375)):
        base = at(tex, s, t)
        for ds, dt in ((1, 0), (-1, 0), (0, 3), (-7, 5), (1023, -1024), (-1024, 1023)):
            assert np.array_equal(bits(at(tex, s + ds, t + dt)), bits(base)), (s, t, ds, dt)
    # the bilinear filter wraps across the seam: at s = 0 it is the midpoint of the last and the first column
    if filt == BILINEAR:
        exp = (texels[1, 7] + F32(0.5) * (texels[1, 0] - texels[1, 7])).astype(F32)
        assert np.array_equal(bits(at(tex, 0.0, 1.5 / 4)), bits(exp))
        assert np.array_equal(bits(at(tex, 1.0, 1.5 / 4)), bits(exp))


@pytest.mark.parametrize("filt", FILTERS)
def test_clamp_below_0_and_above_1_returns_the_edge_texel(filt):
    texels = ramp(8, 4)
    tex = (texels, CLAMP, CLAMP, filt)
    for t, j in ((0.375, 1), (0.875, 3)):
        for s in (-0.001, -0.5, -3.25, -1024.0):
            assert np.array_equal(at(tex, s, t), texels[j, 0]), s
        for s in (1.001, 1.5, 7.75, 1024.0):
            assert np.array_equal(at(tex, s, t), texels[j, 7]), s
    for s, i in ((0.4375, 3),):
        assert np.array_equal(at(tex, s, -2.0), texels[0, i]) and np.array_equal(at(tex, s, 2.0), texels[3, i])


def test_s_0_and_s_1_exactly():
    texels = ramp(8, 4)
    t = 2.5 / 4
    # nearest: s = 0 is texel 0; s = 1 is texel W, which REPEAT wraps to 0 and CLAMP holds at W - 1
    assert np.array_equal(at((texels, REPEAT, REPEAT, NEAREST), 0.0, t), texels[2, 0])
    assert np.array_equal(at((texels, REPEAT, REPEAT, NEAREST), 1.0, t), texels[2, 0])
    assert np.array_equal(at((texels, CLAMP, CLAMP, NEAREST), 0.0, t), texels[2, 0])
    assert np.array_equal(at((texels, CLAMP, CLAMP, NEAREST), 1.0, t), texels[2, 7])
    # bilinear: x = -0.5 and W - 0.5, fx = 0.5 between texels -1 | 0 and W - 1 | W: CLAMP folds both onto the edge texel
    assert np.array_equal(at((texels, CLAMP, CLAMP, BILINEAR), 0.0, t), texels[2, 0])
    assert np.array_equal(at((texels, CLAMP, CLAMP, BILINEAR), 1.0, t), texels[2, 7])
    seam = (texels[2, 7] + F32(0.5) * (texels[2, 0] - texels[2, 7])).astype(F32)
    assert np.array_equal(at((texels, REPEAT, CLAMP, BILINEAR), 0.0, t), seam)
    assert np.array_equal(at((texels, REPEAT, CLAMP, BILINEAR), 1.0, t), seam)


@pytest.mark.parametrize("filt", FILTERS)
def test_a_non_square_texture_distinguishes_the_axes_and_row_0_is_t_0(filt):
    """8 x 2: s runs over the 8 columns, t over the 2 rows; row 0 covers t in [0, 1/2)."""
    texels = ramp(8, 2)
    tex = (texels, CLAMP, CLAMP, filt)
    assert np.array_equal(at(tex, 6.5 / 8, 0.25), texels[0, 6])
    assert np.array_equal(at(tex, 2.5 / 8, 6.5 / 8), texels[1, 2])
    assert np.array_equal(at(tex, 0.5 / 8, 0.25), texels[0, 0]) and np.array_equal(at(tex, 0.5 / 8, 0.75), texels[1, 0])
    assert not np.array_equal(at(tex, 6.5 / 8, 0.25), at(tex, 0.25, 6.5 / 8))  # (s and t swapped)
    # the wraps are per axis too: REPEAT on s, CLAMP on t
    mixed = (texels, REPEAT, CLAMP, filt)
    assert np.array_equal(at(mixed, 1 + 2.5 / 8, 1.75), texels[1, 2])
    assert np.array_equal(at((texels, CLAMP, REPEAT, filt), 1 + 2.5 / 8, 1.75), texels[1, 7])
    assert np.array_equal(at((texels, CLAMP, REPEAT, filt), 2.5 / 8, 1.25), texels[0, 2])


def test_three_equal_uvs_give_s0_and_four_equal_texels_that_texel():
    rng = np.random.default_rng(5)
    s0 = rng.uniform(-3, 3, 64).astype(F32)
    u, v = rng.uniform(0, 1, 64).astype(F32), rng.uniform(0, 1, 64).astype(F32)
    assert np.array_equal(bits(tex_ref.coord(s0, s0, s0, u, v)), bits(s0))
    colour = np.array([0.3, 0.7, 1.9], F32)
    for (w, h), ws, wt, f in tex_ref.MIXED_TEXTURES:
        tex = (np.broadcast_to(colour, (h, w, 3)).copy(), ws, wt, f)
        got = tex_ref.sample(tex, rng.uniform(-4, 4, 64).astype(F32), rng.uniform(-4, 4, 64).astype(F32))
        assert np.array_equal(bits(got), bits(np.broadcast_to(colour, (64, 3))))


def test_the_mixed_set_covers_what_it_claims():
    sizes = {x[0] for x in tex_ref.MIXED_TEXTURES}
    assert sizes == {(1, 1), (1, 5), (5, 3), (2, 2), (64, 32)}
    assert {x[3] for x in tex_ref.MIXED_TEXTURES} == set(FILTERS)
    assert {(x[1], x[2]) for x in tex_ref.MIXED_TEXTURES} == {(REPEAT, REPEAT), (REPEAT, CLAMP), (CLAMP, REPEAT), (CLAMP, CLAMP)}
    used = set()
    for case in tex_ref.CASES:
        if case[6] == T_MIXED:
            t = tex_ref.case_textures(case)
            used |= set(t["mesh_texture"].tolist())
            uv, which = t["uv"], t["mesh_texture"]
            assert (which == tex_ref.NONE).sum() == 1 and len(set(which.tolist())) >= 3, tex_ref.case_id(case)
            assert (uv < 0).any() and (uv > 1).any() and ((uv > 0) & (uv < 1)).any() and np.abs(uv).max() <= 1024
            assert (uv[2::3] * 4 == np.round(uv[2::3] * 4)).all()  # (on texel edges of the 2x2 and 64x32 textures)
            flat = np.concatenate([x[0].reshape(-1, 3) for x in t["textures"]])
            assert np.isfinite(flat).all() and (flat == 0).all(axis=1).any() and (flat > 1).any()
    assert used == set(range(len(tex_ref.MIXED_TEXTURES))) | {tex_ref.NONE}  # (every texture is sampled by some case)


# ---- the discrimination floor ----------------------------------------------------------------------------------------------
def test_the_mixed_texturing_changes_the_frame():
    """The share of rgb words a T_MIXED case changes against the plain frame; MIN_CHANGED is half the smallest share."""
    shares = {}
    for case in tex_ref.CASES:
        if case[6] != T_MIXED:
            continue
        s = tex_ref.case_scene(case)
        plain = tex_ref.plain_frame(s, case)
        ref = tex_ref.case_reference(case)
        shares[tex_ref.case_id(case)] = tex_ref.changed_rgb_words(ref["accum"], plain["accum"])
        # the rays, hence .w and both counts, are the plain frame's
        assert np.array_equal(bits(ref["accum"][..., 3]), bits(plain["accum"][..., 3]))
        assert (ref["closest"], ref["shadow"]) == (plain["closest"], plain["shadow"])
    for k, v in shares.items():
        print("%-48s %.4f" % (k, v))
    assert min(shares.values()) > tex_ref.MIN_CHANGED, shares
    assert tex_ref.MIN_CHANGED >= 0.45 * min(shares.values()), "the floor is half the smallest share: %r" % shares


@pytest.mark.parametrize("case", [c for c in tex_ref.CASES if c[6] == T_ALBEDO], ids=tex_ref.case_id)
def test_other_texels_on_one_mesh_change_only_pixels_that_touch_it(case):
    """From T1's set, the most-touched mesh takes a texture of other texels: pixels none of whose paths shade a vertex on
    that mesh keep their bits; some pixel that touches it changes."""
    s = tex_ref.case_scene(case)
    p, bg = tex_ref.case_params(case), tex_ref.case_background(case)
    tset = tex_ref.texture_set(s, T_ALBEDO)
    base = tex_ref.frame(s, p, tset, bg)
    m = int(np.argmax(base["touched"].sum(axis=(0, 1))))
    assert base["touched"][..., m].any()
    texels, ws, wt, f = tset["textures"][m]
    tset["textures"][m] = (tex_ref.random_texels(texels.shape[1], texels.shape[0], 99), ws, wt, f)
    got = tex_ref.frame(s, p, tset, bg)
    assert np.array_equal(got["touched"], base["touched"]) and (got["closest"], got["shadow"]) == (base["closest"], base["shadow"])
    changed = (bits(got["accum"]) != bits(base["accum"])).any(axis=-1)
    assert not (changed & ~base["touched"][..., m]).any()
    assert changed.any()
