"""The CPU reference of rt_render_shutter (test infrastructure).

The generator of include/rt_amd.h restated in numpy, in the header's operation order: the time t of every sample from the
shutter stream, its camera C(t) = A + t D component by component in float32, the frame's (cu, cv) from the pixel stream
(lens_ref.screen_samples), then the corner of the image plane the sample looks through or, with an aperture, the lens ray
over that camera with the axes and the focus scale of its time.  No restatement of the integrator: the expectation is
lens_ref.chained_rows, one oracle row per pixel and sample added in float32 in sample order.

The oracle forms F + u 0 + v 0 for a row, which turns a -0 into +0, and so does A_c + t 0: no camera used here has a -0
component (no_negative_zero asserts it of A, B and every sample's camera)."""
import numpy as np

import ao_ref
import aov_ref
import lens_ref
import orc
import pyrt

F32, F64 = np.float32, np.float64
STREAM_SHUTTER = 4
SEED = lens_ref.SEED
_cache = {}


def no_negative_zero(cam):
    cam = np.asarray(cam, F32)
    assert not ((cam == 0) & np.signbit(cam)).any(), "a camera component is -0"
    return cam


# ---- the generator -------------------------------------------------------------------------------------------------------
def times(params, open_, close):
    """t float32 [h][w][ns]: one uniformF(open, close) draw of the shutter stream per pixel and sample."""
    w, h = params.width, params.height
    s0, s1 = lens_ref.sample_range(params)
    py, px, smp = np.meshgrid(np.arange(h), np.arange(w), np.arange(s0, s1), indexing="ij")
    e = ao_ref.stream_seed(params.seed, STREAM_SHUTTER, py * w + px, smp)
    t, _ = lens_ref.uniform_f(e, open_, close)
    return t


def camera_at(A, B, t):
    """C(t): A_c + (t D_c) with D = B - A, all float32; t a scalar or an array [...] -> [4][3] or [...][4][3]."""
    A, B = np.asarray(A, F32).reshape(4, 3), np.asarray(B, F32).reshape(4, 3)
    D = (B - A).astype(F32)
    t = np.asarray(t, F32)
    return no_negative_zero((A + (t[..., None, None] * D).astype(F32)).astype(F32))


def corner(cam, cu, cv):
    """((ll + cu H) + cv V) in float32 over per-sample cameras [...][4][3]."""
    ll, H, V = cam[..., 1, :], cam[..., 2, :], cam[..., 3, :]
    return ((ll + (cu[..., None] * H).astype(F32)).astype(F32) + (cv[..., None] * V).astype(F32)).astype(F32)


def shutter_rays(A, B, params, open_=0.0, close=1.0, aperture=0.0, focus_distance=0.0):
    """The primary rays of the frame as (o, F) float32 [h][w][ns][3]: the ray is (o, unit3(F - o)).  aperture == 0:
    (pos(t), corner); aperture > 0: the lens ray of rt_render_lens over C(t) with Hu, Vu and fs of that time."""
    A, B = no_negative_zero(np.asarray(A, F32).reshape(4, 3)), no_negative_zero(np.asarray(B, F32).reshape(4, 3))
    t = times(params, open_, close)
    cam = camera_at(A, B, t)
    cu, cv = lens_ref.screen_samples(params)
    pos = cam[..., 0, :]
    c = corner(cam, cu, cv)
    if not aperture > 0:
        return pos.copy(), c
    _, _, fs0 = lens_ref.constants(A, focus_distance)
    _, _, fs1 = lens_ref.constants(B, focus_distance)
    dfs = F32(fs1 - fs0)
    Hu, Vu = aov_ref._unit(cam[..., 2, :]), aov_ref._unit(cam[..., 3, :])
    fs = (fs0 + (t * dfs).astype(F32)).astype(F32)
    q = (c - pos).astype(F32)
    F = (pos + (fs[..., None] * q).astype(F32)).astype(F32)
    lx, ly = lens_ref.lens_points(params)
    a = F32(aperture)
    o = ((pos + ((a * lx).astype(F32)[..., None] * Hu).astype(F32)).astype(F32) + ((a * ly).astype(F32)[..., None] * Vu).astype(F32)).astype(F32)
    return o, F


def expected(scene, B, params, open_=0.0, close=1.0, aperture=0.0, focus_distance=0.0, accel=orc.ACCEL_OBVH, bg=None):
    """rt_render_shutter's expectation: dict(accum, out (None without bg), closest, shadow)."""
    o, F = shutter_rays(scene.arrays()["camera"], B, params, open_, close, aperture, focus_distance)
    ref = lens_ref.chained_rows(scene, params, o, F, accel)
    ref["out"] = None if bg is None else lens_ref.resolve(ref["accum"], np.asarray(bg, F32), params.spp)
    return ref


# ---- scenes, moves and the cases test_gpu_shutter.py compares bit for bit --------------------------------------------------
def with_camera(s, cam):
    a = s.arrays()
    return pyrt.ArrayScene(a["pos"], a["nrm"], a["tri"], a["tri_begin"], a["vtx_begin"], a["materials"], a["lights"],
                           np.asarray(cam, F32).reshape(4, 3))


def translated(A, move):
    """The camera moved by `move`: position and lower_left shifted in float32."""
    B = np.asarray(A, F32).reshape(4, 3).copy()
    m = np.asarray(move, F32)
    B[0], B[1] = (B[0] + m).astype(F32), (B[1] + m).astype(F32)
    return B


def turned(A, degrees):
    """The camera turned about its vertical axis through its position: lower_left - position, H and V rotated (Rodrigues,
    float64, rounded once)."""
    A = np.asarray(A, F32).reshape(4, 3)
    pos, ll, H, V = (A[k].astype(F64) for k in range(4))
    k = V / np.sqrt(V @ V)
    th = np.deg2rad(degrees)

    def rot(v):
        return v * np.cos(th) + np.cross(k, v) * np.sin(th) + k * (k @ v) * (1 - np.cos(th))

    B = np.stack([pos, pos + rot(ll - pos), rot(H), rot(V)]) + 0.0  # (+ 0.0: no -0)
    return B.astype(F32)


SMALL, LARGE = (0.2, 0.1, 0.0), (0.6, 0.3, 0.1)
TURN_DEGREES = 4.0
MOVES = {"small": lambda A: translated(A, SMALL), "large": lambda A: translated(A, LARGE),
         "turn": lambda A: turned(translated(A, SMALL), TURN_DEGREES)}
EXPOSURES = ((0.0, 1.0), (0.25, 0.5))
SPP1, SPP4, SPP7, SPP7_34 = lens_ref.SPP1, lens_ref.SPP4, lens_ref.SPP7, lens_ref.SPP7_34
RAY, PATH = lens_ref.RAY, lens_ref.PATH
# (preset, open = without mesh 0, w, h, sample range, mode, max_depth, brute, move, exposure, lens = None or (aperture,
# focus) as indices into lens_ref.APERTURES / lens_ref.FOCUS).  13x9: partial 8x8 wave tiles at both edges; 16x16: whole
# ones.  Every size, range, shading form, accelerator, scene, move and exposure appears several times, and a third of the
# cases carry the lens.  The schedule words do not change the expectation: test_gpu_shutter.py runs all six on every case.
CASES = [
    ("cubes", False, 16, 16, SPP4, PATH, 3, False, "small", 0, None),
    ("cubes", False, 13, 9, SPP7, RAY, 1, True, "large", 1, None),
    ("cubes", False, 13, 9, SPP7_34, PATH, 3, False, "turn", 0, (0, 1)),
    ("cubes", False, 16, 16, SPP1, PATH, 2, True, "large", 0, None),
    ("cubes", True, 13, 9, SPP4, PATH, 1, False, "small", 0, None),
    ("cubes", True, 16, 16, SPP1, PATH, 2, False, "large", 0, None),
    ("cubes", True, 13, 9, SPP7_34, PATH, 3, True, "turn", 1, (1, 0)),
    ("lowres", False, 13, 9, SPP7, PATH, 3, False, "small", 1, None),
    ("lowres", False, 16, 16, SPP1, RAY, 1, False, "turn", 0, None),
    ("lowres", True, 16, 16, SPP1, PATH, 3, False, "large", 0, (0, 0)),
    ("lowres", True, 13, 9, SPP4, PATH, 2, True, "small", 0, (1, 1)),
    ("hires", False, 13, 9, SPP1, PATH, 3, False, "large", 0, None),
]


def case_id(c):
    name, opened, w, h, rng, mode, depth, brute, move, ex, lens = c
    return "%s%s-%dx%d-%s-%s%d-%s-%s-%g..%g%s" % (
        name, "_open" if opened else "", w, h, "+".join(str(v) for v in rng.values()), "path" if mode == PATH else "ray", depth,
        "brute" if brute else "bvh", move, EXPOSURES[ex][0], EXPOSURES[ex][1],
        "" if lens is None else "-a%g-f%g" % (lens_ref.APERTURES[lens[0]], lens_ref.FOCUS[lens[1]]))


def case_scene(c):
    s = lens_ref.scene(c[0], c[1], c[2], c[3])
    no_negative_zero(s.arrays()["camera"])
    return s


def case_cameras(c):
    """(A, B) float32 [4][3]: the scene's camera and the case's camera_close."""
    A = np.asarray(case_scene(c).arrays()["camera"], F32).reshape(4, 3)
    return A, no_negative_zero(MOVES[c[8]](A))


def case_shutter_args(c):
    """dict(open, close, aperture, focus_distance) of a case."""
    op, cl = EXPOSURES[c[9]]
    a, f = (0.0, 0.0) if c[10] is None else (lens_ref.APERTURES[c[10][0]], lens_ref.FOCUS[c[10][1]])
    return dict(open=op, close=cl, aperture=a, focus_distance=f)


def case_params(c, **kw):
    return lens_ref.case_params(c[:8] + (0, 0), **kw)


def case_background(c):
    return lens_ref.case_background(c)


def case_threshold(c):
    """The change condition's share: half of the accumulator words for closed scenes and for open scenes with at least
    four samples in the range, a quarter for one-sample open frames."""
    s0, s1 = lens_ref.sample_range(case_params(c))
    return 0.5 if not c[1] or s1 - s0 >= 4 else 0.25


def _frozen(ref):
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


def case_reference(c):
    """The expectation of a case (computed once, shared, never written to)."""
    key = ("ref", case_id(c))
    if key not in _cache:
        k = case_shutter_args(c)
        _cache[key] = _frozen(expected(case_scene(c), case_cameras(c)[1], case_params(c), k["open"], k["close"], k["aperture"],
                                       k["focus_distance"], accel=orc.ACCEL_LOOP if c[7] else orc.ACCEL_OBVH, bg=case_background(c)))
    return _cache[key]


def still_reference(scene, cam, params, brute):
    """The oracle's still pinhole frame of `scene` seen by camera `cam`: (accum, stats)."""
    _, acc, st = orc.render(with_camera(scene, cam), params, math_mode=orc.MATH_DET, accel=orc.ACCEL_LOOP if brute else orc.ACCEL_OBVH)
    return acc, st


def case_stills(c):
    """The oracle's still frames of a case's params at A and at B (accumulators; shared)."""
    key = ("still", case_id(c))
    if key not in _cache:
        A, B = case_cameras(c)
        fa, fb = still_reference(case_scene(c), A, case_params(c), c[7])[0], still_reference(case_scene(c), B, case_params(c), c[7])[0]
        fa.setflags(write=False), fb.setflags(write=False)
        _cache[key] = (fa, fb)
    return _cache[key]


changed_words = lens_ref.changed_words
