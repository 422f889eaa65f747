"""The CPU reference of rt_render_rays (test infrastructure).  No restatement of the integrator: row r is what rt_amd.h
says it is — pixel (0, k) of a frame whose camera returns the row's ray for every sample — rendered by the oracle.

For a ray (o, D) the scene gets the degenerate camera (o, ll, 0, 0) with ll = fl32(o + D): the oracle's camera_ray then
computes unit3((ll + u 0 + v 0) - o) whatever u and v are.  The ray handed to the library is (o, fl32(ll - o)), so the
library's unit3(d_r) is the oracle's primary direction by construction (no numpy square root is involved).  The stream's
pixel index k is the pixel's index in a (k + 1) x 1 frame; the rays a row casts are the difference between the counts of
the (k + 1) x 1 and the k x 1 frame, whose pixels 0..k-1 are the same pixels."""
import ctypes as C

import numpy as np

import ao_ref
import aov_ref
import depth_scenes
import orc
import pyrt

F32 = np.float32
FRAME_W, FRAME_H, FRAME_SEED, RNG_SEED = 8, 6, 9, 3
SEED = 11  # the stream key of the calls under test
_cache = {}


def scene(name, opened):
    """The preset scene, or (opened) the preset without its enclosing room: rays then miss.  name: a preset's, or
    "depth:X" for depth_scenes' shallow scene X."""
    key = ("scene", name, opened)
    if key not in _cache:
        s = depth_scenes.preset(name, FRAME_W, FRAME_H)
        _cache[key] = ao_ref.without_mesh0(s) if opened else s
    return _cache[key]


def library_rays(o, D):
    """(o, fl32(fl32(o + D) - o)) as RAY_DTYPE, and the camera corners ll = fl32(o + D)."""
    o, D = np.asarray(o, F32).reshape(-1, 3), np.asarray(D, F32).reshape(-1, 3)
    ll = (o + D).astype(F32)
    rays = np.zeros(len(o), pyrt.RAY_DTYPE)
    rays["origin"], rays["direction"] = o, (ll - o).astype(F32)
    return rays, ll


def ray_set(name, opened):
    """The rays of a scene's cases: the primary rays of an 8x6 frame with their directions scaled by 2.5 (not unit
    length), then one ray from every first-hit point of that frame, offset by 1e-3 n, towards n + U(-0.7, 0.7)^3.
    Returns (rays RAY_DTYPE [m], ll [m][3])."""
    key = ("rays", name, opened)
    if key not in _cache:
        s = scene(name, opened)
        p = pyrt.make_params(FRAME_W, FRAME_H, 1, seed=FRAME_SEED)
        prim = aov_ref.primary_rays(s, p).reshape(-1)
        hit, nrm, pt = ao_ref.vertices(s, p, accel=orc.ACCEL_OBVH)
        hit, nrm, pt = hit.reshape(-1), nrm.reshape(-1, 3), pt.reshape(-1, 3)
        g = np.random.default_rng(RNG_SEED)
        jig = g.uniform(-0.7, 0.7, (len(hit), 3)).astype(F32)
        o2 = (pt + F32(1e-3) * nrm).astype(F32)[hit]
        d2 = (nrm + jig).astype(F32)[hit]
        o = np.concatenate([prim["origin"], o2])
        D = np.concatenate([(prim["direction"] * F32(2.5)).astype(F32), d2])
        rays, ll = library_rays(o, D)
        rays.setflags(write=False), ll.setflags(write=False)
        _cache[key] = (rays, ll)
    return _cache[key]


def batch(name, opened, n):
    """n rays of the scene's set, repeated cyclically where n is larger (a repeated ray has another stream key)."""
    rays, ll = ray_set(name, opened)
    idx = np.arange(n) % len(rays)
    return rays[idx].copy(), ll[idx].copy()


def _with_camera(s, o, ll):
    a = s.arrays()
    cam = np.zeros((4, 3), F32)
    cam[0], cam[1] = o, ll
    return pyrt.ArrayScene(a["pos"], a["nrm"], a["tri"], a["tri_begin"], a["vtx_begin"], a["materials"], a["lights"], cam)


def _frame_params(params, w):
    q = pyrt.Params()
    C.memmove(C.byref(q), C.byref(params), C.sizeof(pyrt.Params))
    q.width, q.height = w, 1
    return q


def row(s, o, ll, k, params, accel, bg=None, counts=True):
    """The expected row of ray (o, fl32(ll - o)) with stream index k: (accum [4], out [3] or None, (closest, shadow))."""
    cs = _with_camera(s, o, ll)
    bgf = None
    if bg is not None:
        bgf = np.zeros((1, k + 1, 3), F32)
        bgf[0, k] = bg
    out, acc, st = orc.render(cs, _frame_params(params, k + 1), math_mode=orc.MATH_DET, bg=bgf, accel=accel)
    n = [st.rays_closest, st.rays_shadow]
    if counts and k > 0:
        _, _, lo = orc.render(cs, _frame_params(params, k), math_mode=orc.MATH_DET, accel=accel)
        n = [n[0] - lo.rays_closest, n[1] - lo.rays_shadow]
    return acc[0, k].copy(), None if out is None else out[0, k].copy(), tuple(n)


def rows(s, rays, ll, params, stream_index=None, accel=orc.ACCEL_OBVH, bg=None, counts=True):
    """rt_render_rays' expectation for a batch: dict(accum [n][4], out [n][3] or None, closest, shadow: totals of the
    batch — None without counts)."""
    n = len(rays)
    keys = np.arange(n) if stream_index is None else np.asarray(stream_index)
    acc = np.zeros((n, 4), F32)
    out = None if bg is None else np.zeros((n, 3), F32)
    nc = ns = 0
    for r in range(n):
        a, o, (c, sh) = row(s, rays["origin"][r], ll[r], int(keys[r]), params, accel, None if bg is None else bg[r], counts)
        acc[r] = a
        if out is not None:
            out[r] = o
        nc, ns = nc + c, ns + sh
    return dict(accum=acc, out=out, closest=nc if counts else None, shadow=ns if counts else None)


# ---- the cases test_gpu_rays.py compares bit for bit ---------------------------------------------------------------------
# (preset, open = without mesh 0, n, sample range, mode, max_depth, brute).  n: 1, a wave less one, a wave, a wave and
# one, two waves and two; every n, range, shading form (ray mode; path mode at depths 1, 2, 3), accelerator and scene
# appears several times, each pair of them at least once where the kernel's paths could interact (partial waves x
# ranges, brute x depth, open scenes x depth).
SPP1, SPP4, SPP7, SPP7_34 = dict(spp=1), dict(spp=4), dict(spp=7), dict(spp=7, spp_begin=3, spp_count=4)
RAY, PATH = pyrt.MODE_RAY, pyrt.MODE_PATH
CASES = [
    ("cubes", False, 130, SPP4, PATH, 3, False),
    ("cubes", False, 1, SPP7, RAY, 1, True),
    ("cubes", False, 65, SPP7_34, PATH, 3, False),
    ("cubes", False, 64, SPP1, PATH, 2, True),
    ("cubes", False, 63, SPP7, PATH, 1, False),
    ("cubes", True, 63, SPP1, PATH, 2, False),
    ("cubes", True, 64, SPP7_34, PATH, 3, True),
    ("cubes", True, 65, SPP7, PATH, 1, False),
    ("cubes", True, 130, SPP4, RAY, 3, False),
    ("cubes", True, 1, SPP4, PATH, 3, False),
    ("lowres", True, 65, SPP4, PATH, 3, False),
    ("lowres", True, 64, SPP7, RAY, 1, False),
    ("lowres", True, 130, SPP7_34, PATH, 2, False),
    ("lowres", True, 63, SPP1, PATH, 3, True),
    ("lowres", True, 1, SPP7, PATH, 3, False),
    ("lowres", True, 65, SPP7, PATH, 1, True),
    ("hires", False, 37, SPP4, PATH, 3, False),
    ("hires", False, 37, SPP1, RAY, 1, True),
]


def case_id(c):
    name, opened, n, rng, mode, depth, brute = c
    return "%s%s-n%d-%s-%s%d-%s" % (name, "_open" if opened else "", n, "+".join(str(v) for v in rng.values()),
                                    "path" if mode == PATH else "ray", depth, "brute" if brute else "bvh")


def case_params(c, **kw):
    name, opened, n, rng, mode, depth, brute = c
    args = dict(mode=mode, max_depth=depth, seed=SEED, accel=pyrt.ACCEL_BRUTE if brute else pyrt.ACCEL_BVH)
    args.update(rng)
    args.update(kw)
    spp = args.pop("spp")
    return pyrt.make_params(1, 1, spp, **args)


def case_background(n):
    return np.random.default_rng(n).uniform(0, 1, (n, 3)).astype(F32)


def case_reference(c):
    """The expectation of a case with stream_index NULL (computed once, shared, never written to)."""
    key = ("ref", case_id(c))
    if key not in _cache:
        name, opened, n, rng, mode, depth, brute = c
        rays, ll = batch(name, opened, n)
        ref = rows(scene(name, opened), rays, ll, case_params(c), accel=orc.ACCEL_LOOP if brute else orc.ACCEL_OBVH,
                   bg=case_background(n))
        for v in ref.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cache[key] = ref
    return _cache[key]
