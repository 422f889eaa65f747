"""The CPU reference of rt_render_lens (test infrastructure).

The generator of include/rt_amd.h restated in numpy, in the header's operation order: the frame's jitter_sample and (cu,
cv) from the pixel stream, the host-derived constants (Hu, Vu in float32, fs in float64), the lens point by rejection
from the lens stream, o' and F in float32.  No restatement of the integrator: what sample i adds to pixel pix is row pix of
rt_render_rays for the ray (o', F - o') with spp_begin = i, spp_count = 1 — rays_ref.row, i.e. the oracle under the
degenerate camera (o', F, 0, 0) — and the frame's accumulator is the float32 sum of those rows in sample order.

The oracle forms F + u 0 + v 0, which turns a -0 into +0, and so does the lens point's 0 * Hu: the cameras used here
have no position component that is +-0 (scene() asserts it)."""
import ctypes as C

import numpy as np

import ao_ref
import aov_ref
import depth_scenes
import orc
import pyrt
import rays_ref

F32, F64 = np.float32, np.float64
STREAM_PIXEL, STREAM_LENS = 0, 3
SEED = 13
MAX_TRIES = 32
_cache = {}


# ---- rt_device.h, elementwise over arrays --------------------------------------------------------------------------------
def canon_f(s):
    """Rng::canonF: (value float32, end states)."""
    s = ao_ref.engine_next(np.asarray(s, np.uint32))
    r = (s - np.uint32(1)).astype(F32) / F32(2147483648.0)
    return np.where(r >= F32(1), F32(0.99999994), r).astype(F32), s


def uniform_f(s, a, b):
    """Rng::uniformF(a, b) = canonF() * (b - a) + a in float32."""
    c, s = canon_f(s)
    return (c * (F32(b) - F32(a)) + F32(a)).astype(F32), s


def jitter_sample(s, idx, n):
    """jitter_sample(g, idx, n) over arrays of states and sample indices: (x, y float32, end states)."""
    d = int(np.sqrt(F32(n)))
    idx = np.asarray(idx, np.int64)
    j2, i2 = idx // d, idx % d
    c, s = ao_ref.canon_d(np.asarray(s, np.uint32))
    x = ((i2.astype(F32).astype(F64) + (c * (1.0 - 0.0) + 0.0)) / F64(F32(d))).astype(F32)
    c, s = ao_ref.canon_d(s)
    y = ((j2.astype(F32).astype(F64) + (c * (1.0 - 0.0) + 0.0)) / F64(F32(d))).astype(F32)
    return x, y, s


# ---- the host-derived constants ------------------------------------------------------------------------------------------
def _cross64(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], F64)


def _dot64(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def plane_distance(camera):
    """The distance of the image plane along the optical axis, in float64 from the float32 camera [4][3]."""
    pos, ll, H, V = (np.asarray(camera, F32).reshape(4, 3)[k].astype(F64) for k in range(4))
    c = ((ll + 0.5 * H) + 0.5 * V) - pos
    n = _cross64(H, V)
    return abs(_dot64(c, n)) / np.sqrt(_dot64(n, n))


def constants(camera, focus_distance):
    """(Hu, Vu float32 [3], fs float32) of rt_amd.h for a camera [4][3] and a focus distance (a float32 value)."""
    cam = np.asarray(camera, F32).reshape(4, 3)
    with np.errstate(divide="ignore", invalid="ignore"):
        fs = F32(F64(F32(focus_distance)) / plane_distance(cam))
    return aov_ref._unit(cam[2]), aov_ref._unit(cam[3]), fs


# ---- the generator -------------------------------------------------------------------------------------------------------
def sample_range(params):
    return (params.spp_begin, params.spp_begin + params.spp_count) if params.spp_count else (0, params.spp)


def screen_samples(params):
    """(cu, cv) float32 [h][w][ns] of the frame's sample range, formed exactly as the frame forms them."""
    w, h = params.width, params.height
    s0, s1 = sample_range(params)
    py, px, smp = np.meshgrid(np.arange(h), np.arange(w), np.arange(s0, s1), indexing="ij")
    g = ao_ref.stream_seed(params.seed, STREAM_PIXEL, py * w + px, smp)
    sx, sy, _ = jitter_sample(g, smp, params.spp)
    cu = ((px.astype(F32) + sx) / F32(w)).astype(F32)
    cv = (F32(1) - ((py.astype(F32) + sy) / F32(h)).astype(F32)).astype(F32)
    return cu, cv


def pinhole_corner(camera, cu, cv):
    """t = (ll + cu H) + cv V in float32: the point of the image plane a sample looks through."""
    _, ll, H, V = np.asarray(camera, F32).reshape(4, 3)
    return ((ll + cu[..., None] * H).astype(F32) + (cv[..., None] * V).astype(F32)).astype(F32)


def pinhole_operand(camera, cu, cv):
    """q = ((ll + cu H) + cv V) - pos in float32: camera_ray's operand before unit3."""
    return (pinhole_corner(camera, cu, cv) - np.asarray(camera, F32).reshape(4, 3)[0]).astype(F32)


def lens_points(params):
    """(lx, ly) float32 [h][w][ns]: the first of up to 32 pairs of the lens stream inside the unit disc, else (0, 0)."""
    w, h = params.width, params.height
    s0, s1 = sample_range(params)
    py, px, smp = np.meshgrid(np.arange(h), np.arange(w), np.arange(s0, s1), indexing="ij")
    e = ao_ref.stream_seed(params.seed, STREAM_LENS, py * w + px, smp)
    lx, ly = np.zeros(e.shape, F32), np.zeros(e.shape, F32)
    done = np.zeros(e.shape, bool)
    for _ in range(MAX_TRIES):
        x, e = uniform_f(e, -1, 1)
        y, e = uniform_f(e, -1, 1)
        ok = ~done & (((x * x).astype(F32) + (y * y).astype(F32)).astype(F32) <= F32(1))
        lx, ly = np.where(ok, x, lx), np.where(ok, y, ly)
        done |= ok
    return lx, ly


def lens_rays(camera, params, aperture, focus_distance):
    """The primary rays of an aperture > 0 frame: (o' [h][w][ns][3], F [h][w][ns][3]) float32; the ray is (o', unit3(F - o'))."""
    cam = np.asarray(camera, F32).reshape(4, 3)
    pos = cam[0]
    Hu, Vu, fs = constants(cam, focus_distance)
    cu, cv = screen_samples(params)
    q = pinhole_operand(cam, cu, cv)
    F = (pos + (fs * q).astype(F32)).astype(F32)
    lx, ly = lens_points(params)
    a = F32(aperture)
    o = ((pos + ((a * lx).astype(F32)[..., None] * Hu).astype(F32)).astype(F32) + ((a * ly).astype(F32)[..., None] * Vu).astype(F32)).astype(F32)
    return o, F


def pinhole_rays(camera, params):
    """The aperture == 0 rays, (origin, unit direction) [h][w][ns][3]: camera_ray on the restated (cu, cv)."""
    cam = np.asarray(camera, F32).reshape(4, 3)
    cu, cv = screen_samples(params)
    d = aov_ref._unit(pinhole_operand(cam, cu, cv))
    return np.broadcast_to(cam[0], d.shape).copy(), d


# ---- the expected frame --------------------------------------------------------------------------------------------------
def _one_sample(params, i):
    q = pyrt.Params()
    C.memmove(C.byref(q), C.byref(params), C.sizeof(pyrt.Params))
    q.spp_begin, q.spp_count = i, 1
    return q


def chained_rows(scene, params, o, F, accel=orc.ACCEL_OBVH):
    """The frame as rt_amd.h's row equivalence gives it: per pixel the float32 sum, in sample order, of rays_ref.row for
    (o'[pix][i], F[pix][i]) with stream index pix and the one-sample range i.  dict(accum [h][w][4], closest, shadow)."""
    w, h = params.width, params.height
    s0, s1 = sample_range(params)
    acc = np.zeros((h, w, 4), F32)
    nc = ns = 0
    for y in range(h):
        for x in range(w):
            for i in range(s0, s1):
                a, _, (c, sh) = rays_ref.row(scene, o[y, x, i - s0], F[y, x, i - s0], y * w + x, _one_sample(params, i), accel)
                acc[y, x] = (acc[y, x] + a).astype(F32)
                nc, ns = nc + c, ns + sh
    return dict(accum=acc, closest=nc, shadow=ns)


def resolve(accum, bg, spp):
    """k_resolve in float32: sum / N + bg * (N - count) / N."""
    n = F32(spp)
    miss = (np.int64(spp) - accum[..., 3].astype(np.int64)).astype(F32)[..., None]
    return (accum[..., :3] / n + (bg * miss).astype(F32) / n).astype(F32)


def expected(scene, params, aperture, focus_distance, accel=orc.ACCEL_OBVH, bg=None):
    """rt_render_lens' expectation for aperture > 0: dict(accum, out (None without bg), closest, shadow)."""
    o, F = lens_rays(scene.arrays()["camera"], params, aperture, focus_distance)
    ref = chained_rows(scene, params, o, F, accel)
    ref["out"] = None if bg is None else resolve(ref["accum"], np.asarray(bg, F32), params.spp)
    return ref


def expected_pinhole(scene, params, accel=orc.ACCEL_OBVH):
    """The same construction for aperture == 0: the row of sample i is the degenerate camera (pos, t, 0, 0) with t the
    point of the image plane the sample looks through, so that the oracle's t - pos is camera_ray's own operand."""
    cam = np.asarray(scene.arrays()["camera"], F32).reshape(4, 3)
    cu, cv = screen_samples(params)
    t = pinhole_corner(cam, cu, cv)
    return chained_rows(scene, params, np.broadcast_to(cam[0], t.shape), t, accel)


# ---- scenes, cameras and the cases test_gpu_lens.py compares bit for bit ---------------------------------------------------
def scene(name, opened, w, h):
    """The preset at the frame's aspect, or (opened) without its enclosing room: primary rays then miss.  name: a
    preset's, or "depth:X" for depth_scenes' shallow scene X."""
    key = ("scene", name, opened, w, h)
    if key not in _cache:
        s = depth_scenes.preset(name, w, h)
        s = ao_ref.without_mesh0(s) if opened else s
        pos = np.asarray(s.arrays()["camera"], F32).reshape(4, 3)[0]
        assert (pos != 0).all(), "a camera position component is +-0: the oracle's F + u 0 would lose a -0"
        _cache[key] = s
    return _cache[key]


# Two lens radii and two focus distances, in scene units.  Wide and near on purpose: in every case below at least half of
# the frame's accumulator words differ from the pinhole frame's, on the oracle alone (test_lens_ref_cpu.py), although the
# hit count of a closed scene never changes and the open scenes' pinhole frames miss in 35 to 60 % of their pixels.  The
# open frames with one sample take the widest lens at the nearest focus for it (a scan over 0.1 .. 0.6 x 0.5 .. 6).
APERTURES = (0.3, 0.6)
FOCUS = (0.5, 1.5)
SPP1, SPP4, SPP7, SPP7_34 = dict(spp=1), dict(spp=4), dict(spp=7), dict(spp=7, spp_begin=3, spp_count=4)
RAY, PATH = pyrt.MODE_RAY, pyrt.MODE_PATH
# (preset, open = without mesh 0, w, h, sample range, mode, max_depth, brute, aperture, focus).  13x9: partial 8x8 wave
# tiles at both edges; 16x16: whole ones.  Every size, range, shading form (ray mode; path mode at depths 1, 2, 3),
# accelerator, scene (closed and open), aperture and focus distance appears several times, each pair of them at least
# once where the kernel's paths could interact (partial tiles x ranges, brute x depth, open scenes x depth).  The
# schedule words — reserved[0] in {1, 4, 64}, pool or no pool — do not change the expectation: test_gpu_lens.py runs all six
# on every case.
CASES = [
    ("cubes", False, 16, 16, SPP4, PATH, 3, False, 0, 0),
    ("cubes", False, 13, 9, SPP7, RAY, 1, True, 1, 1),
    ("cubes", False, 13, 9, SPP7_34, PATH, 3, False, 1, 0),
    ("cubes", False, 16, 16, SPP1, PATH, 2, True, 0, 1),
    ("cubes", False, 13, 9, SPP4, PATH, 1, False, 0, 1),
    ("cubes", True, 13, 9, SPP7, PATH, 1, False, 0, 1),
    ("cubes", True, 16, 16, SPP1, PATH, 2, False, 1, 0),
    ("cubes", True, 13, 9, SPP7_34, PATH, 3, True, 1, 1),
    ("cubes", True, 13, 9, SPP4, RAY, 3, False, 0, 0),
    ("lowres", False, 13, 9, SPP4, PATH, 3, False, 1, 1),
    ("lowres", False, 16, 16, SPP1, RAY, 1, False, 0, 0),
    ("lowres", False, 13, 9, SPP1, PATH, 1, True, 0, 0),
    ("lowres", True, 13, 9, SPP7_34, PATH, 2, False, 0, 1),
    ("lowres", True, 13, 9, SPP1, PATH, 3, True, 1, 0),
    ("lowres", True, 16, 16, SPP4, PATH, 2, False, 1, 1),
    ("hires", False, 13, 9, SPP1, PATH, 3, False, 1, 0),
]


def case_id(c):
    name, opened, w, h, rng, mode, depth, brute, ai, fi = c
    return "%s%s-%dx%d-%s-%s%d-%s-a%g-f%g" % (name, "_open" if opened else "", w, h, "+".join(str(v) for v in rng.values()),
                                               "path" if mode == PATH else "ray", depth, "brute" if brute else "bvh",
                                               APERTURES[ai], FOCUS[fi])


def case_scene(c):
    return scene(c[0], c[1], c[2], c[3])


def case_lens(c):
    return APERTURES[c[8]], FOCUS[c[9]]


def case_params(c, **kw):
    name, opened, w, h, rng, mode, depth, brute, ai, fi = c
    args = dict(mode=mode, max_depth=depth, seed=SEED, accel=pyrt.ACCEL_BRUTE if brute else pyrt.ACCEL_BVH)
    args.update(rng)
    args.update(kw)
    spp = args.pop("spp")
    return pyrt.make_params(w, h, spp, **args)


def case_background(c):
    return np.random.default_rng(c[2] * 100 + c[3]).uniform(0, 1, (c[3], c[2], 3)).astype(F32)


def case_reference(c):
    """The expectation of a case (computed once, shared, never written to)."""
    key = ("ref", case_id(c))
    if key not in _cache:
        a, f = case_lens(c)
        ref = expected(case_scene(c), case_params(c), a, f, accel=orc.ACCEL_LOOP if c[7] else orc.ACCEL_OBVH, bg=case_background(c))
        for v in ref.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cache[key] = ref
    return _cache[key]


def pinhole_reference(c):
    """The oracle's pinhole frame of a case's params: (accum, stats), shared."""
    key = ("pin", case_id(c))
    if key not in _cache:
        _, acc, st = orc.render(case_scene(c), case_params(c), math_mode=orc.MATH_DET,
                                accel=orc.ACCEL_LOOP if c[7] else orc.ACCEL_OBVH)
        acc.setflags(write=False)
        _cache[key] = (acc, st)
    return _cache[key]


def changed_words(a, b):
    """The share of the accumulator words that differ between the frames a and b [h][w][4]."""
    return float((a.view(np.uint32) != b.view(np.uint32)).mean())
