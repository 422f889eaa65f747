"""rt_denoise: the edge-avoiding a-trous filter on the GPU against its numpy restatement (tests/aov_ref.py atrous), the
pass-through and constant-image identities, the in-place and device forms, and its quality on a 4-spp frame.

Tolerance: 1e-4 absolute.  The kernel forms each tap weight as one float32 expf of the summed exponent (expf: within
2 ulp, the exponent's own float32 rounding a few ulp more); the restatement takes the three exponentials in float64.
A weight's relative error is then below ~1e-6, the weighted mean moves by that fraction of the spread of the taps'
colours (demodulated values up to ~1 / albedo), and the colour differences of the next iteration feed it back through
exp(-d^2 / sigma_i^2) with sigma_i down to sigma_color / 16: a few 1e-6 relative over five iterations, two orders
below the 1e-4 the tests allow (measured on the MI355X: at most 6.0e-7 over these cases; the first test prints it)."""
import ctypes as C

import numpy as np
import pytest

import aov_ref
import pyrt

pytestmark = pytest.mark.gpu

TOL = 1e-4


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def wide_view(scene):
    """The scene with a camera whose field of view is three times as wide: background pixels around the box."""
    a = scene.arrays()
    cam = a["camera"].copy()
    ll, hz, vt = cam[1], cam[2], cam[3]
    c = ll + hz / 2 + vt / 2
    cam[1], cam[2], cam[3] = c - 1.5 * hz - 1.5 * vt, 3 * hz, 3 * vt
    return pyrt.ArrayScene(a["pos"], a["nrm"], a["tri"], a["tri_begin"], a["vtx_begin"], a["materials"], a["lights"], cam)


def frame(scene, w, h, spp, seed=1):
    ctx = pyrt.Context(scene)
    p = pyrt.make_params(w, h, spp, mode=pyrt.MODE_PATH, seed=seed)
    # (a 1-pixel-high image has no background gradient: Image::fillBackground divides by h - 1)
    out, _, _ = ctx.render(p, pyrt.background(w, h) if h > 1 else np.full((h, w, 3), 0.5, np.float32))
    return ctx, out, ctx.render_aov(p, raw=True)


CASES = [("cubes", 64, 48, 1), ("cubes", 64, 48, 5), ("cubes", 37, 23, 1), ("lowres", 37, 23, 5), ("hires", 64, 48, 5),
         ("wide", 64, 48, 5), ("wide", 37, 23, 1), ("cubes", 1, 1, 5)]


@pytest.mark.parametrize("kind,w,h,iters", CASES)
@pytest.mark.parametrize("sig", [(0.0, 0.0, 0.0), (0.25, 0.3, 0.1)], ids=["defaults", "explicit"])
def test_denoise_matches_restatement(kind, w, h, iters, sig):
    scene = wide_view(pyrt.Scene("cubes", w, h)) if kind == "wide" else pyrt.Scene(kind, w, h)
    ctx, rgb, sums = frame(scene, w, h, 4)
    if kind == "wide":
        assert (sums["hits"] == 0).any() and (sums["hits"] > 0).any()
    got = ctx.denoise(rgb, sums, iterations=iters, sigma_color=sig[0], sigma_normal=sig[1], sigma_position=sig[2])
    exp = aov_ref.atrous(rgb, sums, iters, *sig, scene=scene)
    err = float(np.abs(got - exp).max())
    print("%s %dx%d it %d sig %s: max |gpu - numpy| = %.3g" % (kind, w, h, iters, sig, err))
    assert err <= TOL
    miss = sums["hits"] == 0
    assert np.array_equal(bits(got[miss]), bits(rgb[miss]))  # pixels without a hit pass through unchanged
    if w * h > 1 and iters > 1 and not miss.all():
        assert not np.array_equal(got[~miss], rgb[~miss])
    ctx.close()


def test_constant_image_and_passthrough():
    """A constant colour over constant guides comes back unchanged (within the tolerance); pixels with hits == 0 come
    back exactly, whatever their neighbours."""
    w, h = 40, 30
    scene = pyrt.Scene("cubes", w, h)
    ctx = pyrt.Context(scene)
    rng = np.random.default_rng(3)
    hits = np.full((h, w), 4, np.uint32)
    sums = dict(hits=hits, albedo=np.full((h, w, 3), 4 * 0.6, np.float32), normal=np.tile(np.float32([0, 0, 4]), (h, w, 1)),
                position=np.tile(np.float32([0.4, 1.2, -2.0]), (h, w, 1)))
    rgb = np.tile(np.float32([0.3, 0.5, 0.7]), (h, w, 1))
    for it in (1, 5, 8):
        out = ctx.denoise(rgb, sums, iterations=it)
        assert np.abs(out - rgb).max() <= TOL
    hits[rng.random((h, w)) < 0.3] = 0
    rgb2 = rgb.copy()
    rgb2[hits == 0] = rng.random(((hits == 0).sum(), 3), dtype=np.float32)
    out = ctx.denoise(rgb2, sums)
    assert np.array_equal(bits(out[hits == 0]), bits(rgb2[hits == 0]))
    assert np.abs(out[hits > 0] - rgb2[hits > 0]).max() <= TOL  # (the hit pixels are still constant)
    ctx.close()


def test_in_place_and_device_form():
    """rgb == out gives the same image; rt_denoise_device on torch tensors equals the host form bit for bit."""
    import torch
    w, h = 64, 48
    scene = wide_view(pyrt.Scene("lowres", w, h))
    ctx, rgb, sums = frame(scene, w, h, 4, seed=6)
    ref = ctx.denoise(rgb, sums, iterations=4, sigma_color=0.7)
    buf = rgb.copy()
    ctx.denoise(buf, sums, iterations=4, sigma_color=0.7, out=buf)
    assert np.array_equal(bits(buf), bits(ref))
    t = {k: torch.from_numpy(np.ascontiguousarray(v).view(np.int32) if k == "hits" else v).cuda() for k, v in sums.items()
         if k in ("albedo", "normal", "position", "hits")}
    d_rgb = torch.from_numpy(rgb).cuda()
    d_out = torch.zeros_like(d_rgb)
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream()
    ctx.denoise_device(w, h, d_rgb.data_ptr(), {k: v.data_ptr() for k, v in t.items()}, d_out.data_ptr(), stream.cuda_stream,
                       iterations=4, sigma_color=0.7)
    stream.synchronize()
    assert np.array_equal(bits(d_out.cpu().numpy()), bits(ref))
    # in place on the device
    ctx.denoise_device(w, h, d_rgb.data_ptr(), {k: v.data_ptr() for k, v in t.items()}, d_rgb.data_ptr(), 0, iterations=4,
                       sigma_color=0.7)
    torch.cuda.synchronize()
    assert np.array_equal(bits(d_rgb.cpu().numpy()), bits(ref))
    ctx.close()


# F: the denoised 4-spp frame's MSE against a 1024-spp frame, as a fraction of the raw 4-spp frame's.  Measured on the
# CPU first (oracle frames of the same streams + the numpy restatement, DESIGN.md "AOVs and the a-trous denoiser"):
# 0.0627 with the defaults; F leaves about twice that as margin.
QUALITY_F = 0.12


def test_quality_on_a_4spp_frame():
    w = h = 128
    scene = pyrt.Scene("cubes", w, h)
    ctx, noisy, sums = frame(scene, w, h, 4, seed=1)
    ref, _, _ = ctx.render(pyrt.make_params(w, h, 1024, mode=pyrt.MODE_PATH, seed=2), pyrt.background(w, h))
    den = ctx.denoise(noisy, sums)
    raw_mse, den_mse = aov_ref.mse(noisy, ref), aov_ref.mse(den, ref)
    print("cubes 128x128 4 spp: raw MSE %.4g, denoised %.4g (ratio %.4f)" % (raw_mse, den_mse, den_mse / raw_mse))
    assert den_mse <= QUALITY_F * raw_mse
    ctx.close()


def test_error_codes():
    L = pyrt.amd()
    w, h = 8, 8
    scene = pyrt.Scene("cubes", w, h)
    ctx = pyrt.Context(scene)
    rgb = np.zeros((h, w, 3), np.float32)
    out = np.zeros_like(rgb)
    keep = dict(albedo=np.ones((h, w, 3), np.float32), normal=np.ones((h, w, 3), np.float32),
                position=np.ones((h, w, 3), np.float32), hits=np.ones((h, w), np.uint32))

    def rc(ctx_h=ctx._h, drop=None, **kw):
        a = pyrt.Aov()
        for k, v in keep.items():
            if k != drop:
                setattr(a, k, v.ctypes.data)
        d = pyrt.DenoiseParams()
        d.width, d.height = w, h
        for k, v in kw.items():
            setattr(d, k, v)
        return L.rt_denoise(ctx_h, C.byref(d), rgb.ctypes.data, C.byref(a), out.ctypes.data)
    assert rc() == 0
    assert rc(None) == 1
    for k in keep:
        assert rc(drop=k) == 1, k
    assert rc(iterations=9) == 1 and rc(iterations=8) == 0
    assert rc(width=0) == 1 and rc(height=70000) == 1
    assert rc(sigma_color=-1.0) == 1 and rc(sigma_position=float("inf")) == 1 and rc(sigma_normal=float("nan")) == 1
    ctx.close()
