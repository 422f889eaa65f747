"""tests/mat_ref.py against the oracle and tex_ref alone (no GPU): the reference fills two more columns of orc.bsdf_rows per
vertex, so it is pinned by the two guarantees that need no oracle of its own — M1, no maps at all or maps whose texels
are the mesh's own fields, is tex_ref.frame of the same set (and so, with T1, orc.render of the plain scene), and M2, the
strips of per-triangle values on the vertex-split scene, is orc.render of the scene with every triangle a mesh of its own
— bit for bit, M2 over both accelerators.  Then the conditions on the test data: every reference frame is finite, and the
mixed maps change more than mat_ref.MIN_CHANGED* of the rgb words against the albedo-only textured frame, so that a kernel
which ignores a map, or reads the wrong channel, cannot pass."""
import numpy as np
import pytest

import mat_ref
import tex_ref
from tex_ref import T_ALBEDO, T_FACES, T_MIXED, T_NONE


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(ref, exp, what):
    assert np.array_equal(bits(ref["accum"]), bits(exp["accum"])), "accum " + what
    assert np.array_equal(bits(ref["out"]), bits(exp["out"])), "out " + what
    assert (ref["closest"], ref["shadow"]) == (exp["closest"], exp["shadow"]), what


MIXED = [c for c in mat_ref.CASES if c[6] == T_MIXED]
FACES = [c for c in mat_ref.CASES if c[6] == T_FACES]


# ---- M1 and M2 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", mat_ref.CASES, ids=mat_ref.case_id)
def test_m1_no_maps_and_own_field_maps_are_the_textured_frame(case):
    """M1 on every case's scene, whatever its own maps: no maps at all (even cases: both tables None or RT_TEX_NONE
    everywhere, over the case's own texture set) or maps of the meshes' own fields over T1's albedo set (odd cases)."""
    s = mat_ref.case_scene(case)
    p, bg = mat_ref.case_params(case), mat_ref.case_background(case)
    i = mat_ref.CASES.index(case)
    if case[6] == T_NONE:
        mset = mat_ref.case_maps(case)
    elif i % 2 == 0:
        mset = dict(mat_ref.case_maps(case))
        nm = len(mset["mesh_texture"])
        mset["mesh_f0"] = None if i % 4 == 0 else np.full(nm, mat_ref.NONE, np.uint32)
        mset["mesh_kd_alpha"] = np.full(nm, mat_ref.NONE, np.uint32) if i % 4 == 0 else None
    else:
        mset = mat_ref.map_set(s, T_ALBEDO)
    got = mat_ref.frame(s, p, mset, bg)
    same(got, tex_ref.frame(s, p, mset, bg, touched=False), mat_ref.case_id(case))
    if case[6] in (T_NONE, T_ALBEDO) or i % 2 == 1:
        same(got, tex_ref.plain_frame(s, case), "against the plain frame " + mat_ref.case_id(case))  # (with T1)


@pytest.mark.parametrize("case", FACES, ids=mat_ref.case_id)
@pytest.mark.parametrize("brute", [False, True], ids=["bvh", "loop"])
def test_m2_the_strips_are_the_frame_of_one_mesh_per_triangle(case, brute):
    same(mat_ref.case_reference(case, brute), tex_ref.plain_frame(mat_ref.per_triangle_scene(mat_ref.case_scene(case)), case, brute),
         mat_ref.case_id(case))


def test_m2_sets_hold_every_strip_under_both_filters_and_b_is_9():
    for case in FACES:
        t = mat_ref.case_maps(case)
        assert len(t["textures"]) == 6
        albedo, f0, kd, alpha = mat_ref.face_fields(mat_ref.case_scene(case))
        assert kd.min() >= 0 and kd.max() < 1 and alpha.min() >= 0.05 and alpha.max() < 1 and f0.min() >= 0 and f0.max() < 1
        for k, exp in ((0, albedo), (2, f0), (4, np.stack([kd, alpha, np.full(len(kd), 9.0, np.float32)], axis=1))):
            assert {t["textures"][k][3], t["textures"][k + 1][3]} == {tex_ref.NEAREST, tex_ref.BILINEAR}
            for tex in t["textures"][k:k + 2]:
                got = tex_ref.sample(tex, t["uv"][::3, 0], t["uv"][::3, 1])
                assert np.array_equal(bits(got), bits(exp)), mat_ref.case_id(case)
        assert set(t["mesh_f0"].tolist()) == {2, 3} and set(t["mesh_kd_alpha"].tolist()) <= {4, 5}


# ---- the test data ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", mat_ref.CASES, ids=mat_ref.case_id)
def test_every_reference_frame_is_finite(case):
    ref = mat_ref.case_reference(case)
    assert np.isfinite(ref["accum"]).all() and np.isfinite(ref["out"]).all()


def test_the_mixed_maps_cover_what_they_claim():
    for case in MIXED:
        t = mat_ref.case_maps(case)
        nx = len(tex_ref.MIXED_TEXTURES)
        assert len(t["textures"]) == 3 * nx
        f0, kda = t["mesh_f0"], t["mesh_kd_alpha"]
        assert (f0 == mat_ref.NONE).sum() == 1 and (kda == mat_ref.NONE).sum() == 1
        assert int(np.argmax(f0 == mat_ref.NONE)) != int(np.argmax(kda == mat_ref.NONE))
        assert all(nx <= x < 2 * nx for x in f0.tolist() if x != mat_ref.NONE)
        assert all(2 * nx <= x < 3 * nx for x in kda.tolist() if x != mat_ref.NONE)
        for k in range(nx):
            shape = tuple(reversed(tex_ref.MIXED_TEXTURES[k][0])) + (3,)
            assert t["textures"][nx + k][0].shape == shape and t["textures"][2 * nx + k][0].shape == shape
            x = t["textures"][2 * nx + k][0]
            assert 0 <= x[..., 0].min() and x[..., 0].max() < 1 and 0.05 <= x[..., 1].min() and x[..., 1].max() < 1
            assert -5 <= x[..., 2].min() and x[..., 2].max() < 5
        flat = np.concatenate([x[0].reshape(-1, 3) for x in t["textures"]])
        assert np.isfinite(flat).all()
    used_f0 = set().union(*(set(mat_ref.case_maps(c)["mesh_f0"].tolist()) for c in MIXED))
    used_kda = set().union(*(set(mat_ref.case_maps(c)["mesh_kd_alpha"].tolist()) for c in MIXED))
    nx = len(tex_ref.MIXED_TEXTURES)
    assert used_f0 == set(range(nx, 2 * nx)) | {mat_ref.NONE} and used_kda == set(range(2 * nx, 3 * nx)) | {mat_ref.NONE}


def test_the_mixed_maps_change_the_textured_frame():
    """The share of rgb words a T_MIXED case changes against the albedo-only textured frame of the same set: with all maps,
    with the f0 maps alone and with the (kd, alpha) maps alone.  Each MIN_CHANGED* is half the smallest share."""
    shares = {"all": {}, "f0": {}, "kda": {}}
    for case in MIXED:
        s, p, bg = mat_ref.case_scene(case), mat_ref.case_params(case), mat_ref.case_background(case)
        mset = mat_ref.case_maps(case)
        base = mat_ref.case_textured_reference(case)
        frames = {"all": mat_ref.case_reference(case), "f0": mat_ref.frame(s, p, mat_ref.without(mset, "mesh_kd_alpha"), bg),
                  "kda": mat_ref.frame(s, p, mat_ref.without(mset, "mesh_f0"), bg)}
        for k, ref in frames.items():
            shares[k][mat_ref.case_id(case)] = mat_ref.changed_rgb_words(ref["accum"], base["accum"])
            # the rays, hence .w and both counts, are the textured frame's
            assert np.array_equal(bits(ref["accum"][..., 3]), bits(base["accum"][..., 3]))
            assert (ref["closest"], ref["shadow"]) == (base["closest"], base["shadow"])
    for cid in shares["all"]:
        print("%-48s all %.4f  f0 %.4f  kda %.4f" % (cid, shares["all"][cid], shares["f0"][cid], shares["kda"][cid]))
    for k, floor in (("all", mat_ref.MIN_CHANGED), ("f0", mat_ref.MIN_CHANGED_F0), ("kda", mat_ref.MIN_CHANGED_KDA)):
        low = min(shares[k].values())
        print("smallest share, %s: %.4f (floor %.4f)" % (k, low, floor))
        assert low > floor, (k, shares[k])
        assert floor >= 0.45 * low, "the floor is half the smallest share: %s %r" % (k, shares[k])
