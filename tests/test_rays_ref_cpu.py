"""The reference of rt_render_rays (tests/rays_ref.py) on its own, without a GPU: the conditions that keep the GPU
comparison from being vacuous — the open scenes' ray sets both hit and miss, most hit rays carry light, every expected
accumulator is finite — and the one property the construction rests on: a wider frame of the degenerate camera changes
the stream's pixel index and nothing else."""
import numpy as np
import pytest

import orc
import pyrt
import rays_ref

SETS = [("cubes", False), ("cubes", True), ("lowres", True)]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def full_set_rows(name, opened, **kw):
    rays, ll = rays_ref.ray_set(name, opened)
    p = pyrt.make_params(1, 1, 4, seed=rays_ref.SEED, **kw)
    keys = np.zeros(len(rays), np.uint32)
    return rays, rays_ref.rows(rays_ref.scene(name, opened), rays, ll, p, stream_index=keys, counts=False)["accum"]


@pytest.mark.parametrize("name,opened", SETS, ids=["cubes", "cubes_open", "lowres_open"])
def test_ray_sets_hit_miss_and_carry_light(name, opened):
    rays, acc = full_set_rows(name, opened)
    assert np.isfinite(acc).all()
    n_dir = np.sqrt((rays["direction"].astype(np.float64) ** 2).sum(axis=1))
    assert (np.abs(n_dir[:rays_ref.FRAME_W * rays_ref.FRAME_H] - 2.5) < 1e-3).all(), "the frame's rays are not unit length"
    hit = acc[:, 3] > 0
    share = hit.mean()
    print("%s%s: %d / %d rays hit (%.1f %%), %d with light" % (name, "_open" if opened else "", hit.sum(), len(hit), 100 * share,
                                                             acc[hit, :3].any(axis=1).sum()))
    if opened:
        assert 0.2 <= share <= 0.8
    else:
        assert share > 0.8
    assert acc[hit, :3].any(axis=1).mean() >= 0.8
    assert not acc[~hit].any(), "a primary miss adds nothing"
    # a sample either hits or misses as a whole ray does: .w is 0 or the sample count
    assert set(np.unique(acc[:, 3])) <= {0.0, 4.0}


def test_library_direction_is_the_oracles_primary_direction():
    """orc.dump_rays of the degenerate camera shows the primary ray (o, unit3(ll - o)) for every sample, and fl32(ll - o)
    normalises to the same bits in numpy's float32 (Vec3.h:170-178: sum of squares left to right, sqrt, 1 / length)."""
    import aov_ref
    name, opened = "cubes", True
    rays, ll = rays_ref.ray_set(name, opened)
    s = rays_ref.scene(name, opened)
    for r in (0, 17, 47, 48, len(rays) - 1):
        cs = rays_ref._with_camera(s, rays["origin"][r], ll[r])
        prim = aov_ref.primary_rays(cs, pyrt.make_params(1, 1, 3, seed=5)).reshape(-1)
        assert (bits(prim["origin"]) == bits(rays["origin"][r])).all()
        want = aov_ref._unit(rays["direction"][r][None])[0]
        assert (bits(prim["direction"]) == bits(want)).all(), r


def test_a_wider_frame_changes_the_stream_index_only():
    """Pixel 0 of the (k + 1) x 1 frame is the 1 x 1 frame's pixel; pixel k differs from it where the ray carries light
    (another stream), and the rays of pixel k are the difference of the two frames' counts."""
    name, opened = "lowres", True
    rays, ll = rays_ref.ray_set(name, opened)
    s = rays_ref.scene(name, opened)
    p = pyrt.make_params(1, 1, 4, seed=rays_ref.SEED)
    differ = lit = 0
    for r in range(1, len(rays), 3):
        cs = rays_ref._with_camera(s, rays["origin"][r], ll[r])
        _, one, st1 = orc.render(cs, rays_ref._frame_params(p, 1), math_mode=orc.MATH_DET, accel=orc.ACCEL_OBVH)
        for k in (1, 5):
            _, wide, stw = orc.render(cs, rays_ref._frame_params(p, k + 1), math_mode=orc.MATH_DET, accel=orc.ACCEL_OBVH)
            assert (bits(wide[0, 0]) == bits(one[0, 0])).all(), (r, k)
            assert (wide[0, :, 3] == one[0, 0, 3]).all(), "every pixel casts the same primary ray"
            lit += int(one[0, 0, :3].any())
            differ += int((bits(wide[0, k]) != bits(one[0, 0])).any())
            a, _, (c, sh) = rays_ref.row(s, rays["origin"][r], ll[r], k, p, orc.ACCEL_OBVH)
            assert (bits(a) == bits(wide[0, k])).all()
            assert c >= 4 and c <= 12 and sh % s.desc.n_lights == 0 and c <= stw.rays_closest
    assert differ == lit and lit > 10, (differ, lit)


def test_cases_cover_what_the_issue_lists():
    ns = {c[2] for c in rays_ref.CASES}
    assert ns == {1, 37, 63, 64, 65, 130} and max(ns) <= 130
    rngs = {tuple(sorted(c[3].items())) for c in rays_ref.CASES}
    assert len(rngs) == 4
    assert {(c[4], c[5]) for c in rays_ref.CASES if c[4] == pyrt.MODE_PATH} >= {(pyrt.MODE_PATH, d) for d in (1, 2, 3)}
    assert any(c[4] == pyrt.MODE_RAY for c in rays_ref.CASES)
    assert {c[6] for c in rays_ref.CASES} == {False, True}
    assert {(c[0], c[1]) for c in rays_ref.CASES} == {("cubes", False), ("cubes", True), ("lowres", True), ("hires", False)}
    for c in rays_ref.CASES:
        ref = rays_ref.case_reference(c)
        assert np.isfinite(ref["accum"]).all() and np.isfinite(ref["out"]).all()
        assert ref["closest"] >= (ref["accum"][:, 3] > 0).sum() and ref["shadow"] > 0
