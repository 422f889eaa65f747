"""The numpy restatement of rt_svgf (tests/svgf_ref.py) against things that do not share its formulas: a running mean and
a population variance, a fixed point, the a-trous restatement of rt_denoise, and the analytic variance reduction of the
a-trous kernel; and the float32 evaluation against the float64 one on the frames of the GPU test (the tolerance that test
uses)."""
import numpy as np
import pytest

import aov_ref
import svgf_ref as sv

W, H = 24, 20


def static_inputs(rng, albedo=None, flat=False, size=(W, H)):
    """A static synthetic frame of `size`: every pixel hit once, one mesh, no motion; guides random (or constant: flat)."""
    W, H = size
    one = lambda *s: np.ones(s, np.float32)
    alb = (rng.uniform(0.2, 0.9, (H, W, 3)) if albedo is None else np.broadcast_to(albedo, (H, W, 3))).astype(np.float32)
    nrm = np.broadcast_to(np.float32([0, 0, 1]), (H, W, 3)).copy()
    pos = np.zeros((H, W, 3), np.float32)
    if not flat:
        ys, xs = np.mgrid[0:H, 0:W]
        pos[..., 0], pos[..., 1] = 0.01 * xs, 0.01 * ys
    sums = dict(albedo=alb, normal=nrm, position=pos, hits=np.ones((H, W), np.uint32))
    cur = dict(motion=np.zeros((H, W, 2), np.float32), position=pos, prev_position=pos, mesh=np.ones((H, W), np.uint32))
    return sums, cur


def test_static_scene_is_a_running_mean_and_a_population_variance():
    rng = np.random.default_rng(1)
    sums, cur = static_inputs(rng)
    hist, ds = sv.empty_history(W, H), []
    for k in range(6):
        rgb = rng.uniform(0.0, 1.0, (H, W, 3)).astype(np.float32)
        o = sv.svgf_ref(rgb, sums, cur, hist, max_history=64, sigma_position=1.0, sigma_reproject=1.0)
        ds.append((rgb / np.maximum(sums["albedo"], np.float32(1e-3))).astype(np.float64))
        hist = sv.next_history(dict(o, color=o["accum"]), cur)  # (the unfiltered colour fed back: the mean of the frames)
        assert (o["length"] == k + 1).all()
        mean = np.mean(ds, axis=0)
        assert np.allclose(o["accum"], mean, rtol=1e-5, atol=1e-6)
        lum = [0.2126 * d[..., 0] + 0.7152 * d[..., 1] + 0.0722 * d[..., 2] for d in ds]
        m1, m2 = o["moments"][..., 0].astype(np.float64), o["moments"][..., 1].astype(np.float64)
        assert np.allclose(m1, np.mean(lum, axis=0), rtol=1e-5) and np.allclose(m2 - m1 * m1, np.var(lum, axis=0), rtol=1e-3, atol=1e-5)
    assert o["info"]["long_history"] == W * H and o["info"]["history"] == W * H


@pytest.mark.parametrize("f32", (False, True))
def test_a_constant_frame_is_a_fixed_point_with_variance_zero(f32):
    sums, cur = static_inputs(np.random.default_rng(2), albedo=np.float32([0.5, 0.25, 0.75]), flat=True)
    rgb = np.broadcast_to(np.float32([0.3, 0.2, 0.6]), (H, W, 3)).copy()
    hist = sv.empty_history(W, H)
    # (zero to the rounding of the two moments, which are kept in float32: a few eps of l^2, times 4 / length)
    bound = 4 * 8 * np.finfo(np.float32).eps * float(sv.luminance((rgb / sums["albedo"]).astype(np.float64)).max()) ** 2
    for k in range(5):
        o = sv.svgf_ref(rgb, sums, cur, hist, sigma_position=1.0, sigma_reproject=1.0, f32=f32)
        assert np.allclose(o["rgb"], rgb, rtol=1e-6, atol=0) and np.allclose(o["color"], rgb / sums["albedo"], rtol=1e-6)
        assert np.abs(o["variance"]).max() <= bound and np.abs(o["variance0"]).max() <= bound
        hist = sv.next_history(o, cur)


def test_one_iteration_without_luminance_weight_is_the_denoisers():
    rng = np.random.default_rng(3)
    sums, cur = static_inputs(rng)
    sums["normal"] = rng.normal(size=(H, W, 3)).astype(np.float32)
    sums["hits"][3:6, 4:9] = 0  # invalid pixels pass through and weigh 0
    rgb = rng.uniform(0.1, 1.0, (H, W, 3)).astype(np.float32)
    o = sv.svgf_ref(rgb, sums, cur, sv.empty_history(W, H), iterations=1, sigma_luminance=1e30, sigma_normal=0.7,
                    sigma_position=0.05, sigma_reproject=1.0)
    ref = aov_ref.atrous(rgb, sums, iterations=1, sigma_color=1e15, sigma_normal=0.7, sigma_position=0.05)
    assert (o["variance0"][sums["hits"] > 0] > 0).all()
    assert np.allclose(o["rgb"], ref, rtol=2e-6, atol=1e-7)
    assert np.array_equal(o["rgb"][3:6, 4:9], rgb[3:6, 4:9])


def test_equal_weights_reduce_the_variance_by_the_kernels_sum_of_squares():
    """Constant guides and no luminance weight: w = h[dx] h[dy], so var' = (sum h^2)^2 var away from the border, and the
    variance of filtered i.i.d. noise falls by that factor."""
    W, H = 96, 96
    rng = np.random.default_rng(4)
    sums, cur = static_inputs(rng, albedo=np.float32([1, 1, 1]), flat=True, size=(W, H))
    v = 0.37
    hist = sv.empty_history(W, H)
    hist.update(mesh=cur["mesh"], length=np.full((H, W), 9.0, np.float32))
    hist["moments"][..., 0], hist["moments"][..., 1] = 0.0, v / 0.9  # with l = 0 now and alpha = 1 / 10: m1 = 0, m2 = v
    noise = rng.normal(size=(H, W, 3)).astype(np.float32)
    zero = np.zeros((H, W, 3), np.float32)
    o = sv.svgf_ref(zero, sums, cur, hist, iterations=1, max_history=10, sigma_luminance=1e30, sigma_position=1.0,
                    sigma_reproject=1.0)
    k2 = sum(h * h for h in aov_ref.H5) ** 2
    assert abs(k2 - (70.0 / 256) ** 2) < 1e-15
    assert np.allclose(o["variance0"], v, rtol=1e-6)
    assert np.allclose(o["variance"][2:-2, 2:-2], k2 * v, rtol=1e-5)
    # empirically: unit-variance noise as the colour, accumulated onto nothing
    o = sv.svgf_ref(noise, sums, cur, sv.empty_history(W, H), iterations=1, sigma_luminance=1e30, sigma_position=1.0,
                    sigma_reproject=1.0)
    got = o["color"][2:-2, 2:-2].astype(np.float64).var()
    assert abs(got / k2 - 1) < 0.1, (got, k2)


def test_float32_evaluation_stays_within_the_recorded_tolerance():
    """T_CPU (svgf_ref.py) is what this measures on the frames of tests/test_gpu_svgf.py, per size and setting; at each
    size the sequence reaches the 7x7 window, the long-history path and every reprojection branch."""
    for w, h in sv.SEQ_SIZES:
        seq = sv.sequence_inputs(w, h)
        seen = {}
        for si, kw in enumerate(sv.SEQ_SETTINGS):
            t, info = sv.measure_tolerance(seq, **kw)
            rec = sv.tolerance((w, h), si)
            print(w, h, kw, "measured:", t, "recorded:", rec)
            for k in t:
                assert 0.9 * rec[k] <= t[k] <= rec[k], (w, h, kw, k, t[k], rec[k])
            for k, v in info.items():
                seen[k] = seen.get(k, 0) + v
        for name in sv.BRANCHES:
            assert seen[name] > 0, "the %dx%d sequence never takes the branch %r" % (w, h, name)
