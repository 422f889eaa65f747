"""CPU restatement of rt_render_ao (test infrastructure), vectorised numpy.

The primary hits, shading normals and points are formed as aov_ref.aov_sums forms them (the oracle's primary rays and
trace, Renderer.cpp:42-43 in float32).  The occlusion rays' directions come from a numpy restatement of the sampler in
the headers' operation order — rt_stream_seed, the minstd_rand0 engine, canonD, rt_asin, rt_sincosf, hemisphere_sample
(include/rt_pixelmode.h, csrc/rt_device.h) — and their answers from orc.trace (closest): occluded iff hit and
(max_distance == 0 or d < max_distance).  test_ao_ref_cpu.py pins the sampler to the oracle's own bounce rays."""
import numpy as np

import aov_ref
import orc
import pyrt

STREAM_PIXEL, STREAM_AO = 0, 2
BIAS_SCALE = 1e-4
U64, F32, F64 = np.uint64, np.float32, np.float64


# ---- rt_pixelmode.h / rt_device.h, elementwise over arrays ---------------------------------------------------------------
def _mix64(z):
    z = z ^ (z >> U64(30))
    z = z * U64(0xbf58476d1ce4e5b9)
    z = z ^ (z >> U64(27))
    z = z * U64(0x94d049bb133111eb)
    return z ^ (z >> U64(31))


def stream_seed(seed, domain, index, sub):
    """rt_stream_seed over arrays of index and sub (uint32 state in [1, 2147483646])."""
    index, sub = np.asarray(index, U64), np.asarray(sub, U64)
    with np.errstate(over="ignore"):
        h = _mix64(U64((int(seed) << 32) | int(domain)))
        h = _mix64(h + ((index << U64(32)) | sub))
    s = h >> U64(33)
    s = np.where(s >= U64(2147483646), s - U64(2147483646), s)
    return (s + U64(1)).astype(np.uint32)


def engine_next(s):
    """One minstd_rand0 step of the states s (uint32 array): the new states (also the value drawn)."""
    p = s.astype(U64) * U64(16807)
    x = (p & U64(0x7fffffff)) + (p >> U64(31))
    x = np.where(x >= U64(0x7fffffff), x - U64(0x7fffffff), x)
    return x.astype(np.uint32)


def canon_d(s):
    """Rng::canonD: (value float64, end states)."""
    R = F64(2147483646.0)
    R2 = R * R
    a = engine_next(s)
    b = engine_next(a)
    tot = (a - np.uint32(1)).astype(F64)
    tot = tot + (b - np.uint32(1)).astype(F64) * R
    r = tot / R2
    return np.where(r >= 1.0, F64(0.99999999999999988898), r), b


def _asin_poly(t):
    pS0, pS1, pS2 = 1.66666666666666657415e-01, -3.25565818622400915405e-01, 2.01212532134862925881e-01
    pS3, pS4, pS5 = -4.00555345006794114027e-02, 7.91534994289814532176e-04, 3.47933107596021167570e-05
    qS1, qS2, qS3, qS4 = -2.40339491173441421878e+00, 2.02094576023350569471e+00, -6.88283971605453293030e-01, 7.70381505559019352791e-02
    p = t * (pS0 + t * (pS1 + t * (pS2 + t * (pS3 + t * (pS4 + t * pS5)))))
    q = 1.0 + t * (qS1 + t * (qS2 + t * (qS3 + t * qS4)))
    return p / q


def rt_asin(x):
    """rt_asin on float64 arrays, every branch evaluated and selected."""
    x = np.asarray(x, F64)
    pio2_hi, pio2_lo, pio4_hi = 1.57079632679489655800e+00, 6.12323399573676603587e-17, 7.85398163397448278999e-01
    ax = np.where(x < 0.0, -x, x)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        small = x + x * _asin_poly(x * x)
        w = 1.0 - ax
        t = w * 0.5
        r = _asin_poly(t)
        s = np.sqrt(t)
        hi = pio2_hi - (2.0 * (s + s * r) - pio2_lo)
        sh = (s.view(U64) & U64(0xffffffff00000000)).view(F64)
        c = (t - sh * sh) / (s + sh)
        p = 2.0 * s * r - (pio2_lo - 2.0 * c)
        q = pio4_hi - 2.0 * sh
        mid = pio4_hi - (p - q)
        big = np.where(ax >= 0.975, hi, mid)
        big = np.where(x < 0.0, -big, big)
    res = np.where(ax < 0.5, np.where(ax < 7.450580596923828125e-09, x, small), big)
    res = np.where(ax == 1.0, x * pio2_hi + x * pio2_lo, res)
    return np.where(ax <= 1.0, res, np.nan)


def _ksin(r):
    S1, S2, S3 = -1.66666666666666324348e-01, 8.33333333332248946124e-03, -1.98412698298579493134e-04
    S4, S5, S6 = 2.75573137070700676789e-06, -2.50507602534068634195e-08, 1.58969099521155010221e-10
    z = r * r
    v = z * r
    p = S2 + z * (S3 + z * (S4 + z * (S5 + z * S6)))
    return r + v * (S1 + z * p)


def _kcos(r):
    C1, C2, C3 = 4.16666666666666019037e-02, -1.38888888888741095749e-03, 2.48015872894767294178e-05
    C4, C5, C6 = -2.75573143513906633035e-07, 2.08757232129817482790e-09, -1.13596475577881948265e-11
    z = r * r
    p = z * (C1 + z * (C2 + z * (C3 + z * (C4 + z * (C5 + z * C6)))))
    return 1.0 - (0.5 * z - z * p)


def rt_sincosf(xf):
    """rt_sincosf on a float32 array: (sin, cos) float32."""
    invpio2, pio2_1, pio2_1t = 6.36619772367581382433e-01, 1.57079632673412561417e+00, 6.07710050650619224932e-11
    x = np.asarray(xf, F32).astype(F64)
    with np.errstate(invalid="ignore"):
        fn = x * invpio2
        n = np.where(np.isfinite(fn), np.trunc(np.where(fn < 0.0, fn - 0.5, fn + 0.5)), 0.0).astype(np.int64)
        dn = n.astype(F64)
        r = (x - dn * pio2_1) - dn * pio2_1t
        q = n & 3
        ks, kc = _ksin(r), _kcos(r)
        sv = np.where(q & 1, kc, ks)
        cv = np.where(q & 1, ks, kc)
        sv = np.where(q & 2, -sv, sv)
        cv = np.where((q == 1) | (q == 2), -cv, cv)
        return sv.astype(F32), cv.astype(F32)


def _unit(a):
    return aov_ref._unit(np.asarray(a, F32))


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1).astype(F32)


def _two_orthogonals(n):
    x, y, z = n[..., 0], n[..., 1], n[..., 2]
    ax, ay, az = np.abs(x), np.abs(y), np.abs(z)
    zero = np.zeros_like(x)
    a = np.stack([zero, -z, y], -1)   # (0, -n.z, n.y)
    b = np.stack([-y, x, zero], -1)   # (-n.y, n.x, 0)
    c = np.stack([z, zero, -x], -1)   # (n.z, 0, -n.x)
    u = np.where((ax < ay)[..., None], np.where((ax < az)[..., None], a, b), np.where((ay < az)[..., None], c, b)).astype(F32)
    return u, _cross(n, u)


def hemisphere_sample(state, normal):
    """hemisphere_sample from the engine states `state` (uint32 [...]) about `normal` (float32 [..., 3]): (direction
    float32 [..., 3], end states)."""
    PI = F64(3.14159265358979323846)
    hi = F64(F32(2) * F32(1.57079637)) / PI
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        n = _unit(normal)
        v1, v2 = _two_orthogonals(n)
        v1, v2 = _unit(v1), _unit(v2)
        c1, state = canon_d(np.asarray(state, np.uint32))
        theta = rt_asin(c1 * (hi - 0.0) + 0.0).astype(F32)
        c2, state = canon_d(state)
        phi = (2 * PI * (c2 * (hi - 0.0) + 0.0)).astype(F32)
        sp, cp = rt_sincosf(phi)
        st, ct = rt_sincosf(theta)
        d = _unit((v1 * cp[..., None] + v2 * sp[..., None]).astype(F32))
        return _unit((n * ct[..., None] + d * st[..., None]).astype(F32)), state


# ---- the pass ------------------------------------------------------------------------------------------------------------
def default_bias(scene):
    """1e-4 of the diagonal of the bounding box of the vertices the triangles reference (float32), computed like
    aov_ref.default_sigma_position."""
    a = scene.arrays()
    p = a["pos"][a["tri"].reshape(-1)]
    d = (p.max(axis=0) - p.min(axis=0)).astype(F32)
    return float(F32(BIAS_SCALE) * np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))


def diagonal(scene):
    return default_bias(scene) / BIAS_SCALE


def without_mesh0(scene):
    """The scene without its first mesh (the presets' enclosing room): an open scene whose frames have misses."""
    a = scene.arrays()
    nv, nt = int(a["vtx_begin"][1]), int(a["tri_begin"][1])
    return pyrt.ArrayScene(a["pos"][nv:], a["nrm"][nv:], a["tri"][nt:] - np.uint32(nv), a["tri_begin"][1:] - np.uint32(nt),
                           a["vtx_begin"][1:] - np.uint32(nv), a["materials"][1:], a["lights"], a["camera"])


def vertices(scene, params, accel=orc.ACCEL_LOOP):
    """Per sample of the range the primary hit as aov_ref.aov_sums forms it: hit [h][w][ns] bool, normal and point
    [h][w][ns][3] float32."""
    a = scene.arrays()
    rays = aov_ref.primary_rays(scene, params)
    h, w, ns = rays.shape
    hits = orc.trace(scene, rays.reshape(-1), accel=accel).reshape(h, w, ns)
    hit = hits["hit"] != 0
    mesh = np.where(hit, hits["mesh"], 0).astype(np.int64)
    gid = a["tri_begin"][mesh].astype(np.int64) + np.where(hit, hits["tri"], 0)
    tv = a["tri"][gid].astype(np.int64)
    u, v = hits["u"][..., None], hits["v"][..., None]
    wgt = (F32(1) - u) - v
    p0, p1, p2 = (a["pos"][tv[..., k]] for k in range(3))
    n0, n1, n2 = (a["nrm"][tv[..., k]] for k in range(3))
    nrm = aov_ref._unit((wgt * n0 + u * n1) + v * n2)
    pt = ((wgt * p0 + u * p1) + v * p2).astype(F32)
    return hit, nrm, pt


def ao_sums(scene, params, n_rays, bias=0., max_distance=0., accel=orc.ACCEL_LOOP):
    """rt_render_ao's sums for the frame `params` describes: dict of unoccluded, hits [h][w] uint32, bent [h][w][3]
    float32, and `occluded_share` (of all occlusion rays; nan when there is none)."""
    hit, nrm, pt = vertices(scene, params, accel)
    h, w, ns = hit.shape
    s0 = params.spp_begin if params.spp_count else 0
    bias = F32(bias) if bias else F32(default_bias(scene))
    pix = (np.arange(h)[:, None] * w + np.arange(w)[None, :])[:, :, None, None]
    smp = (s0 + np.arange(ns))[None, None, :, None]
    j = np.arange(n_rays)[None, None, None, :]
    state = stream_seed(params.seed, STREAM_AO, np.broadcast_to(pix, (h, w, ns, n_rays)), smp * n_rays + j)
    d, _ = hemisphere_sample(state, np.broadcast_to(nrm[:, :, :, None, :], (h, w, ns, n_rays, 3)))
    o = (pt[:, :, :, None, :] + (bias * d).astype(F32)).astype(F32)
    on = np.broadcast_to(hit[..., None], (h, w, ns, n_rays))
    rays = np.zeros(int(on.sum()), pyrt.RAY_DTYPE)
    rays["origin"], rays["direction"] = o[on], d[on]
    res = orc.trace(scene, rays, accel=accel)
    occ = (res["hit"] != 0) & ((res["d"] < F32(max_distance)) if max_distance else True)
    esc = np.zeros((h, w, ns, n_rays), bool)
    esc[on] = ~occ
    fin = np.isfinite(d).all(axis=-1)
    bent = np.zeros((h, w, 3), F32)
    for s in range(ns):  # float32 adds in (sample, j) order; a direction that is not finite adds nothing
        for k in range(n_rays):
            m = esc[:, :, s, k] & fin[:, :, s, k]
            bent = np.where(m[..., None], bent + d[:, :, s, k], bent).astype(F32)
    n_on = int(on.sum())
    return dict(unoccluded=esc.sum(axis=(2, 3)).astype(np.uint32), hits=hit.sum(axis=2).astype(np.uint32), bent=bent,
                occluded_share=float(occ.sum()) / n_on if n_on else float("nan"))


# ---- the frames test_gpu_ao.py compares bit for bit, shared with test_ao_ref_cpu.py ---------------------------------------
# (preset, open = without mesh 0, w, h, sample range, n_rays, brute, bias (0 = default), max_distance: a share of the
# diagonal when below 1, else absolute).  The sizes: 64x48 (whole tiles), 37x23 (partial tiles at both edges), 1x1 (one
# lane; in the open scenes a lane whose samples hit and miss by turns), 16x8 with RT_AO_MAX_RAYS.  Every scene closed and open, both accelerators, both biases, the three distance
# forms and the four sample ranges appear at least once at each of the two frame sizes.
SPP1, SPP4, SPP7, SPP7_34 = dict(spp=1), dict(spp=4), dict(spp=7), dict(spp=7, spp_begin=3, spp_count=4)
FAR = 1e30
CASES = [
    ("cubes", False, 64, 48, SPP1, 1, False, 0., 0.),
    ("cubes", True, 64, 48, SPP4, 3, False, 1e-3, 0.1),
    ("cubes", True, 64, 48, SPP1, 8, True, 0., 0.),
    ("lowres", False, 64, 48, SPP7_34, 1, False, 0., 0.1),
    ("lowres", True, 64, 48, SPP1, 3, False, 0., FAR),
    ("lowres", True, 64, 48, SPP7, 1, True, 1e-3, 0.1),
    ("hires", False, 64, 48, SPP1, 3, False, 0., 0.),
    ("hires", True, 64, 48, SPP1, 1, True, 0., FAR),
    ("cubes", False, 37, 23, SPP4, 3, False, 0., 0.),
    ("cubes", True, 37, 23, SPP7, 8, False, 1e-3, 0.1),
    ("cubes", True, 37, 23, SPP7_34, 8, False, 1e-3, 0.1),
    ("cubes", False, 37, 23, SPP1, 8, True, 0., FAR),
    ("lowres", False, 37, 23, SPP4, 3, False, 0., 0.1),
    ("lowres", True, 37, 23, SPP7, 1, True, 0., 0.),
    ("lowres", True, 37, 23, SPP1, 8, False, 1e-3, FAR),
    ("hires", False, 37, 23, SPP4, 1, False, 1e-3, 0.1),
    ("hires", True, 37, 23, SPP1, 3, False, 0., 0.),
    ("hires", True, 37, 23, SPP7_34, 3, True, 0., 0.1),
    ("cubes", False, 16, 8, SPP1, 256, False, 0., 0.),
    ("cubes", False, 1, 1, SPP7, 8, False, 0., 0.),
    ("lowres", True, 1, 1, SPP4, 3, True, 0., 0.),
    ("hires", False, 1, 1, SPP7, 8, False, 1e-3, 0.1),
    ("hires", True, 1, 1, SPP7, 8, True, 1e-3, FAR),
]
SEED = 9
_cache = {}


def case_id(c):
    name, opened, w, h, rng, n_rays, brute, bias, dist = c
    return "%s%s-%dx%d-%s-n%d-%s-b%g-d%g" % (name, "_open" if opened else "", w, h, "+".join(str(v) for v in rng.values()), n_rays,
                                             "brute" if brute else "bvh", bias, dist)


def case_scene(name, opened, w, h):
    key = ("scene", name, opened, w, h)
    if key not in _cache:
        s = pyrt.Scene(name, w, h)
        _cache[key] = without_mesh0(s) if opened else s
    return _cache[key]


def case_distance(scene, dist):
    return dist * diagonal(scene) if dist < 1 else dist


def case_params(c, accel=None):
    name, opened, w, h, rng, n_rays, brute, bias, dist = c
    accel = (pyrt.ACCEL_BRUTE if brute else pyrt.ACCEL_BVH) if accel is None else accel
    return pyrt.make_params(w, h, seed=SEED, accel=accel, **rng)


def case_reference(c):
    """The restatement's sums for a case (computed once, shared, never written to)."""
    key = ("ref", case_id(c))
    if key not in _cache:
        name, opened, w, h, rng, n_rays, brute, bias, dist = c
        s = case_scene(name, opened, w, h)
        ref = ao_sums(s, case_params(c), n_rays, bias, case_distance(s, dist), accel=orc.ACCEL_OBVH)
        for v in ref.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cache[key] = ref
    return _cache[key]
