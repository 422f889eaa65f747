"""lens_ref.py against the oracle and against itself, without a GPU: the restated screen samples give the oracle's own
primary rays, the chained-rows construction of a frame gives the oracle's frame, and the lens generator has the
properties a thin lens must have."""
import numpy as np
import pytest

import aov_ref
import lens_ref
import orc
import pyrt

F32, F64 = np.float32, np.float64
PRESETS = [("cubes", 13, 9), ("cubes", 16, 16), ("lowres", 13, 9), ("hires", 16, 16)]


@pytest.mark.parametrize("rng", [lens_ref.SPP1, lens_ref.SPP4, lens_ref.SPP7, lens_ref.SPP7_34], ids=lambda r: "+".join(map(str, r.values())))
def test_restated_pinhole_rays_are_the_oracles(rng):
    """At aperture 0 the ray of the restated (cu, cv) is aov_ref.primary_rays' — the oracle's ray dump — bit for bit."""
    for w, h in ((13, 9), (16, 16)):
        s = lens_ref.scene("cubes", False, w, h)
        args = dict(rng)
        p = pyrt.make_params(w, h, args.pop("spp"), seed=lens_ref.SEED, **args)
        o, d = lens_ref.pinhole_rays(s.arrays()["camera"], p)
        ref = aov_ref.primary_rays(s, p)
        assert np.array_equal(ref["origin"].view(np.uint32), o.view(np.uint32))
        assert np.array_equal(ref["direction"].view(np.uint32), d.view(np.uint32))


@pytest.mark.parametrize("name,opened,rng,mode,depth", [("cubes", False, lens_ref.SPP4, lens_ref.PATH, 3),
                                                        ("cubes", True, lens_ref.SPP7_34, lens_ref.PATH, 2),
                                                        ("lowres", True, lens_ref.SPP1, lens_ref.RAY, 1)])
def test_chained_rows_of_a_pinhole_frame_are_the_oracles_frame(name, opened, rng, mode, depth):
    """The construction of the expectation itself: one oracle row per (pixel, sample), added in float32 in sample order,
    is orc.render's accumulator, and the rows' ray counts add up to the frame's."""
    s = lens_ref.scene(name, opened, 13, 9)
    args = dict(rng)
    p = pyrt.make_params(13, 9, args.pop("spp"), mode=mode, max_depth=depth, seed=lens_ref.SEED, **args)
    got = lens_ref.expected_pinhole(s, p)
    _, acc, st = orc.render(s, p, math_mode=orc.MATH_DET, accel=orc.ACCEL_OBVH)
    assert np.array_equal(acc.view(np.uint32), got["accum"].view(np.uint32))
    assert (got["closest"], got["shadow"]) == (st.rays_closest, st.rays_shadow)


def test_resolve_restated_is_the_oracles():
    s = lens_ref.scene("cubes", True, 13, 9)
    p = pyrt.make_params(13, 9, 4, seed=lens_ref.SEED)
    bg = np.random.default_rng(1).uniform(0, 1, (9, 13, 3)).astype(F32)
    out, acc, _ = orc.render(s, p, math_mode=orc.MATH_DET, bg=bg, accel=orc.ACCEL_OBVH)
    assert np.array_equal(out.view(np.uint32), lens_ref.resolve(acc, bg, 4).view(np.uint32))


def test_lens_points_lie_on_the_unit_disc_and_fill_it():
    p = pyrt.make_params(16, 16, 7, seed=lens_ref.SEED)
    lx, ly = lens_ref.lens_points(p)
    r2 = (lx * lx).astype(F32) + (ly * ly).astype(F32)
    assert (r2 <= F32(1)).all()
    assert ((lx != 0) | (ly != 0)).all()  # (32 rejections in a row: (1 - pi / 4)^32 = 4e-22)
    # all four quadrants and the rim are reached; the mean radius^2 of a uniform disc is 1 / 2
    assert (lx > 0).any() and (lx < 0).any() and (ly > 0).any() and (ly < 0).any() and r2.max() > 0.95
    assert abs(float(r2.mean()) - 0.5) < 0.05
    # a sample range draws the samples of the whole frame
    q = pyrt.make_params(16, 16, 7, seed=lens_ref.SEED, spp_begin=3, spp_count=4)
    mx, my = lens_ref.lens_points(q)
    assert np.array_equal(mx, lx[:, :, 3:7]) and np.array_equal(my, ly[:, :, 3:7])


@pytest.mark.parametrize("name,w,h", PRESETS)
def test_constants_of_the_preset_cameras_are_finite(name, w, h):
    cam = np.asarray(pyrt.Scene(name, w, h).arrays()["camera"], F32).reshape(4, 3)
    for f in lens_ref.FOCUS:
        hu, vu, fs = lens_ref.constants(cam, f)
        assert np.isfinite(hu).all() and np.isfinite(vu).all() and np.isfinite(fs) and fs > 0
        assert abs(float(np.dot(hu.astype(F64), hu.astype(F64))) - 1) < 1e-6 and abs(float(np.dot(vu.astype(F64), vu.astype(F64))) - 1) < 1e-6
    assert lens_ref.plane_distance(cam) > 0


@pytest.mark.parametrize("name,w,h", PRESETS)
def test_a_point_of_the_focus_plane_projects_to_the_same_screen_point_from_every_lens_sample(name, w, h):
    """The rays of all lens samples of one (cu, cv) meet in F, F lies at focus_distance along the axis, and seen from the
    camera position F projects to (cu, cv) again.  The bounds are float32 roundings of the stated formulas: F = pos + fs q
    carries a few ulps of |pos| + |fs q| (< 16 here: 2^-20), the focus distance two more roundings, and the projection
    divides by a determinant of O(1) components."""
    cam = np.asarray(pyrt.Scene(name, w, h).arrays()["camera"], F32).reshape(4, 3)
    p = pyrt.make_params(w, h, 4, seed=lens_ref.SEED)
    cu, cv = lens_ref.screen_samples(p)
    pos, ll, H, V = (cam[k].astype(F64) for k in range(4))
    n = lens_ref._cross64(H, V)
    n = n / np.sqrt(lens_ref._dot64(n, n))
    for a in lens_ref.APERTURES:
        for f in lens_ref.FOCUS:
            o, F = lens_ref.lens_rays(cam, p, a, f)
            o, F = o.astype(F64), F.astype(F64)
            # the lens points lie on the disc of radius a around pos, in the plane through pos parallel to the image plane
            r = o - pos
            assert (np.sqrt((r * r).sum(-1)) <= a * (1 + 1e-6)).all() and np.abs(r @ n).max() < 1e-6 * max(a, 1)
            # F at the focus distance along the axis
            assert np.abs(np.abs((F - pos) @ n) - f).max() < 1e-5 * max(f, 1)
            # F seen from pos: Cramer's rule for F - pos = lambda (ll - pos + s H + t V)
            q, c = F - pos, ll - pos
            hv = lens_ref._cross64(H, V)
            s_ = (np.cross(q, V) * c).sum(-1) / (q @ hv)
            t_ = (np.cross(H, q) * c).sum(-1) / (q @ hv)
            assert np.abs(s_ - cu).max() < 1e-5 and np.abs(t_ - cv).max() < 1e-5


@pytest.mark.parametrize("c", lens_ref.CASES, ids=lens_ref.case_id)
def test_every_case_changes_half_of_the_accumulator_words(c):
    """The condition test_gpu_lens.py holds the library to, on the oracle alone: at least half of the accumulator words of
    an aperture > 0 frame differ from the pinhole frame of the same params."""
    ref, (pin, _) = lens_ref.case_reference(c), lens_ref.pinhole_reference(c)
    assert lens_ref.changed_words(ref["accum"], pin) >= 0.5
    s0, s1 = lens_ref.sample_range(lens_ref.case_params(c))
    assert ref["closest"] >= pin.shape[0] * pin.shape[1] * (s1 - s0)  # (every sample casts its primary ray)
