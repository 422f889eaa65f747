"""The case table of rt_render_views_shutter and its CPU expectation (test infrastructure).

No new arithmetic: view j of a case is shutter_ref.expected — the numpy generator of rt_render_shutter and one oracle row
per pixel and sample — on the case's scene seen by cameras[j], with the params' seed replaced by seeds[j] and the view's own
record.  That is guarantee V1 of include/rt_amd.h stated on the CPU.

A case has three views on an orbit about the point the scene's camera looks at (view 0 is the scene's own camera) and three
shutter records, pairwise different.  The records are of four kinds; every case carries the no-optics view and two of the
three kinds with optics, and the table rotates through those so that each is rendered beside each other and in every
position of the launch:
  none       camera_close == cameras[j], open == close == 0, aperture 0: the still pinhole frame of cameras[j]
  lens       the same camera at both ends, open == close == 0, an aperture: depth of field alone
  move_lens  a translated camera_close over the whole exposure, with an aperture
  turn       a translated and turned camera_close, exposure (0.25, 0.5), no lens
tests/test_views_shutter_ref_cpu.py checks on the oracle alone that a kernel which took another view's record for a view
would be seen: every view's frame under each other view's record differs from its own in more than a quarter of its words.

No camera used here has a -0 component (shutter_ref.no_negative_zero)."""
import ctypes as C

import numpy as np

import lens_ref
import orc
import pyrt
import shutter_ref
from shutter_ref import no_negative_zero, translated, turned, with_camera

F32, F64 = np.float32, np.float64
SEED = lens_ref.SEED
N_VIEWS = 3
ORBIT_DEGREES, ORBIT_SCALES = (0.0, 14.0, -18.0), (1.0, 0.9, 1.15)
VIEW_SEEDS = (11, 12, 40000)
TURN_EXPOSURE = (0.25, 0.5)
SPP1, SPP4, SPP7, SPP7_34 = lens_ref.SPP1, lens_ref.SPP4, lens_ref.SPP7, lens_ref.SPP7_34
RAY, PATH = lens_ref.RAY, lens_ref.PATH
_cache = {}


# ---- cameras -------------------------------------------------------------------------------------------------------------
def look_at(eye, target, half_w, half_h):
    """The look-at camera with +y up, float32 [4][3]: position, lower_left, horizontal, vertical."""
    eye, target = np.asarray(eye, F64), np.asarray(target, F64)
    back = (eye - target) / np.linalg.norm(eye - target)
    right = np.cross([0.0, 1.0, 0.0], back)
    right /= np.linalg.norm(right)
    up = np.cross(back, right)
    cam = np.stack([eye, eye - half_w * right - half_h * up - back, 2 * half_w * right, 2 * half_h * up]) + 0.0  # (+ 0.0: no -0)
    return cam.astype(F32)


def orbit(cam, degrees, scales):
    """Cameras on orbits about the point `cam` looks at, at its own distance from the origin ahead of it: one per (angle
    about +y, scale of the distance to that point), with cam's field of view.  Angle 0 at scale 1 is cam itself."""
    cam = np.asarray(cam, F32).reshape(4, 3)
    eye0 = cam[0].astype(F64)
    centre = cam[1].astype(F64) + cam[2].astype(F64) / 2 + cam[3].astype(F64) / 2
    fwd = (centre - eye0) / np.linalg.norm(centre - eye0)
    target = eye0 + fwd * max(np.linalg.norm(eye0), 1.0)
    half_w, half_h = np.linalg.norm(cam[2].astype(F64)) / 2, np.linalg.norm(cam[3].astype(F64)) / 2
    plane = np.linalg.norm(centre - eye0)  # (look_at puts the image plane at distance 1: scale the frame to cam's)
    out = []
    for deg, f in zip(degrees, scales):
        if deg == 0.0 and f == 1.0:
            out.append(cam.copy())
            continue
        phi = np.deg2rad(deg)
        R = np.array([[np.cos(phi), 0, np.sin(phi)], [0, 1, 0], [-np.sin(phi), 0, np.cos(phi)]])
        out.append(look_at(target + R @ (eye0 - target) * f, target, half_w / plane, half_h / plane))
    return no_negative_zero(np.stack(out).astype(F32))


# ---- records -------------------------------------------------------------------------------------------------------------
def record(kind, cam, lens=(0, 0), move=shutter_ref.SMALL):
    """dict(camera_close, open, close, aperture, focus_distance) of a kind for the view camera `cam`."""
    cam = np.asarray(cam, F32).reshape(4, 3)
    a, f = lens_ref.APERTURES[lens[0]], lens_ref.FOCUS[lens[1]]
    if kind == "none":
        return dict(camera_close=cam.copy(), open=0.0, close=0.0, aperture=0.0, focus_distance=0.0)
    if kind == "lens":
        return dict(camera_close=cam.copy(), open=0.0, close=0.0, aperture=a, focus_distance=f)
    if kind == "move_lens":
        return dict(camera_close=no_negative_zero(translated(cam, move)), open=0.0, close=1.0, aperture=a, focus_distance=f)
    assert kind == "turn", kind
    B = no_negative_zero(turned(translated(cam, shutter_ref.SMALL), shutter_ref.TURN_DEGREES))
    return dict(camera_close=B, open=TURN_EXPOSURE[0], close=TURN_EXPOSURE[1], aperture=0.0, focus_distance=0.0)


def shutter_of(rec):
    return pyrt.make_shutter(rec["camera_close"], rec["open"], rec["close"], rec["aperture"], rec["focus_distance"])


# (preset, open = without mesh 0, w, h, sample range, mode, max_depth, brute, the three views' kinds, lens = (aperture,
# focus) as indices into lens_ref.APERTURES / lens_ref.FOCUS, the translation of move_lens, seeds per view or None).
# 13x9: partial 8x8 wave tiles at both edges; 16x16: whole ones.  Ranges 1, 4, 7 and 3..7 of 7; ray mode and path depths 1
# to 3; BVH and the exhaustive loop; cubes, and lowres closed and open.  The one-sample frames take the wide lens at the
# near focus.  Seeds differ per view in half of the cases.
CASES = [
    ("cubes", False, 16, 16, SPP4, PATH, 3, False, ("none", "lens", "move_lens"), (0, 0), shutter_ref.SMALL, VIEW_SEEDS),
    ("cubes", False, 13, 9, SPP7, RAY, 1, True, ("move_lens", "none", "turn"), (1, 1), shutter_ref.LARGE, None),
    ("cubes", True, 13, 9, SPP7_34, PATH, 3, False, ("turn", "lens", "none"), (1, 0), shutter_ref.SMALL, VIEW_SEEDS),
    ("lowres", False, 16, 16, SPP1, PATH, 2, False, ("lens", "none", "move_lens"), (1, 0), shutter_ref.LARGE, None),
    ("lowres", True, 13, 9, SPP4, PATH, 1, True, ("none", "turn", "lens"), (0, 1), shutter_ref.SMALL, VIEW_SEEDS),
    ("lowres", True, 16, 16, SPP7, PATH, 2, False, ("turn", "move_lens", "none"), (1, 0), shutter_ref.LARGE, None),
]


def case_id(c):
    name, opened, w, h, rng, mode, depth, brute, kinds, lens, move, seeds = c
    return "%s%s-%dx%d-%s-%s%d-%s-%s-%s" % (
        name, "_open" if opened else "", w, h, "+".join(str(v) for v in rng.values()), "path" if mode == PATH else "ray", depth,
        "brute" if brute else "bvh", "+".join(kinds), "seeds" if seeds else "oneseed")


def case_scene(c):
    s = lens_ref.scene(c[0], c[1], c[2], c[3])
    no_negative_zero(s.arrays()["camera"])
    return s


def case_cameras(c):
    """float32 [3][4][3]: the scene's camera and two more on its orbit."""
    return orbit(case_scene(c).arrays()["camera"], ORBIT_DEGREES, ORBIT_SCALES)


def case_seeds(c):
    return None if c[11] is None else list(c[11])


def case_records(c):
    """The three views' records (dicts)."""
    return [record(kind, cam, c[9], c[10]) for kind, cam in zip(c[8], case_cameras(c))]


def case_shutters(c):
    return [shutter_of(r) for r in case_records(c)]


def case_params(c, **kw):
    return lens_ref.case_params(c[:8] + (0, 0), **kw)


def case_background(c):
    return lens_ref.case_background(c)


def case_accel(c):
    return orc.ACCEL_LOOP if c[7] else orc.ACCEL_OBVH


def none_view(c):
    return c[8].index("none")


def samples_of(c):
    s0, s1 = lens_ref.sample_range(case_params(c))
    return N_VIEWS * c[2] * c[3] * (s1 - s0)


def _frozen(ref):
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


def view_params(c, j):
    """The case's params with view j's seed."""
    p = case_params(c)
    q = pyrt.Params()
    C.memmove(C.byref(q), C.byref(p), C.sizeof(pyrt.Params))
    if c[11] is not None:
        q.seed = c[11][j]
    return q


def view_expected(c, j, r=None, brute=None):
    """The expectation of view j under the record of view r (its own when None): dict(accum, out, closest, shadow);
    computed once, shared, never written to.  brute: the accelerator, the case's own when None."""
    r = j if r is None else r
    brute = c[7] if brute is None else brute
    key = ("view", case_id(c), j, r, brute)
    if key not in _cache:
        rec = case_records(c)[r]
        scene = with_camera(case_scene(c), case_cameras(c)[j])
        _cache[key] = _frozen(shutter_ref.expected(scene, rec["camera_close"], view_params(c, j), rec["open"], rec["close"], rec["aperture"],
                                                   rec["focus_distance"], accel=orc.ACCEL_LOOP if brute else orc.ACCEL_OBVH,
                                                   bg=case_background(c)))
    return _cache[key]


def case_reference(c, brute=None):
    """The expectation of the call: dict(accum [3][h][w][4], out [3][h][w][3], closest, shadow — sums over the views)."""
    key = ("ref", case_id(c), brute)
    if key not in _cache:
        views = [view_expected(c, j, brute=brute) for j in range(N_VIEWS)]
        _cache[key] = _frozen(dict(accum=np.stack([v["accum"] for v in views]), out=np.stack([v["out"] for v in views]),
                                   closest=sum(v["closest"] for v in views), shadow=sum(v["shadow"] for v in views)))
    return _cache[key]


def pad_reference(a, cameras=()):
    """The reference magnitude of the box padding rule for a scene description and further cameras [n][4][3]: the largest
    of 1, the referenced vertices', the camera positions' and the light positions' |coordinate|, float32.  The padding is
    6e-5 of it, the origin bound 16 times it."""
    ref = F32(max(F32(1), np.abs(a["pos"][a["tri"].reshape(-1)]).max()))
    for v in list(np.asarray(a["camera"], F32).reshape(4, 3)[0]) + list(a["lights"][:, 0:3].reshape(-1)) + \
            [x for c in cameras for x in np.asarray(c, F32).reshape(4, 3)[0]]:
        if np.isfinite(v):
            ref = max(ref, F32(abs(v)))
    return F32(ref)


changed_words = lens_ref.changed_words
