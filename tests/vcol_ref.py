"""The CPU reference of rt_render_colors and rt_render_aov_colors (test infrastructure), from the oracle's own parts.

Colours never move a ray, so every ray of a coloured frame is the plain frame's: orc.dump_rays lists them in casting
order, orc.trace on the closest rays gives each vertex's mesh, triangle, vertex ids, u and v, orc.trace(kind=ANY) on the
shadow rays the occlusions.  The point is the shadow rays' origin, the normal the interpolation ao_ref.vertices does,
orc.bsdf_rows (rows with albedo = c, MATH_DET) and orc.eval_light_rows the two factors of a term.  The only arithmetic
stated here is the colour c = (c0 + u (c1 - c0)) + v (c2 - c0), the products radiance * bsdf and the sums: lights from +0
in index order, vertices as the recursion adds them (c0 + (c1 + (c2 + 0))), the per-sample clamp, and the accumulation in
sample order.  tests/test_vcol_ref_cpu.py pins those orders to the oracle's own frames (C1 and C2 of include/rt_amd.h)."""
import numpy as np

import aov_ref
import lens_ref
import lights_ref
import orc
import pyrt

F32 = np.float32
SEED = 13
_cache = {}

SPP1, SPP4, SPP7, SPP7_34 = lens_ref.SPP1, lens_ref.SPP4, lens_ref.SPP7, lens_ref.SPP7_34
RAY, PATH = pyrt.MODE_RAY, pyrt.MODE_PATH
ALBEDO, FACES, SMOOTH = "albedo", "faces", "smooth"


# ---- scenes and colourings -------------------------------------------------------------------------------------------------
def mesh_of_vertex(a):
    """The mesh of every vertex, from the scene's vertex partition."""
    return np.repeat(np.arange(len(a["vtx_begin"]) - 1), np.diff(a["vtx_begin"].astype(np.int64)))


def mesh_of_triangle(a):
    return np.repeat(np.arange(len(a["tri_begin"]) - 1), np.diff(a["tri_begin"].astype(np.int64)))


def albedo_colors(s):
    """C1's colouring: every vertex carries its mesh's albedo (rt_material: floats 2..4 of a row)."""
    a = s.arrays()
    return np.ascontiguousarray(a["materials"][mesh_of_vertex(a), 2:5], F32)


def split_scene(s):
    """The scene with three vertices of its own per triangle (positions and normals copied, the mesh partition kept):
    triangle t owns vertices 3t .. 3t + 2."""
    a = s.arrays()
    tv = a["tri"].astype(np.int64).reshape(-1)
    nt = len(a["tri"])
    return pyrt.ArrayScene(a["pos"][tv], a["nrm"][tv], np.arange(3 * nt, dtype=np.uint32).reshape(nt, 3), a["tri_begin"],
                           3 * a["tri_begin"], a["materials"], a["lights"], a["camera"])


def face_colors(s):
    """C2's colouring of a split scene: one random colour per triangle on its three vertices; returns (rgb per vertex,
    rgb per triangle)."""
    nt = len(s.arrays()["tri"])
    face = np.random.default_rng(nt).uniform(0.05, 1.0, (nt, 3)).astype(F32)
    return np.repeat(face, 3, axis=0), face


def per_triangle_scene(s, face):
    """C2's other side: the split scene with every triangle a mesh of its own, in the same order, whose material is its
    mesh's with albedo = the triangle's colour."""
    a = s.arrays()
    nt = len(a["tri"])
    mats = a["materials"][mesh_of_triangle(a)].copy()
    mats[:, 2:5] = face
    one = np.arange(nt + 1, dtype=np.uint32)
    return pyrt.ArrayScene(a["pos"], a["nrm"], a["tri"], one, 3 * one, mats, a["lights"], a["camera"])


def smooth_colors(s):
    """A colouring that varies inside every triangle: a function of the vertex position plus a per-vertex hash, with
    every seventh vertex at 0 and every fifth above 1."""
    a = s.arrays()
    pos = a["pos"].astype(np.float64)
    ext = np.maximum(pos.max(axis=0) - pos.min(axis=0), 1e-9)
    q = (pos - pos.min(axis=0)) / ext
    n = len(pos)
    hsh = ((np.arange(n, dtype=np.uint64) * np.uint64(2654435761)) % np.uint64(1 << 32)).astype(np.float64) / float(1 << 32)
    c = np.stack([0.15 + 0.7 * q[:, 0], 0.15 + 0.7 * q[:, 1], 0.15 + 0.7 * q[:, 2]], axis=1) + 0.15 * (hsh[:, None] - 0.5)
    c = np.clip(c, 0.02, 1.0)
    c[np.arange(n) % 5 == 0] *= 1.7
    c[np.arange(n) % 7 == 0] = 0.0
    return np.ascontiguousarray(c, F32)


# ---- the frame -------------------------------------------------------------------------------------------------------------
def interpolate(colors, tv, u, v):
    """c = (c0 + u (c1 - c0)) + v (c2 - c0) in float32, every operation rounded on its own."""
    c0, c1, c2 = (np.asarray(colors, F32)[tv[:, k]] for k in range(3))
    u, v = u.astype(F32)[:, None], v.astype(F32)[:, None]
    return ((c0 + u * (c1 - c0)).astype(F32) + v * (c2 - c0)).astype(F32)


def clamp01(x):
    """Renderer.cpp:279-283: fmaxf(fminf(v, 1), 0)."""
    return np.fmax(np.fmin(x, F32(1)), F32(0)).astype(F32)


def frame(scene, params, colors, bg=None, brute=False, touched=True):
    """The coloured frame `params` describes: dict(accum [h][w][4], out [h][w][3] or None, closest, shadow, albedo
    [h][w][3] — the first-hit sums of c, rt_render_aov_colors' albedo channel — and touched [h][w][n_tris] bool: the
    triangles the pixel's paths shaded a vertex on (None with touched=False: at a million triangles it is 48 MB for an
    8x6 frame)."""
    a = scene.arrays()
    w, h = params.width, params.height
    ns = params.spp_count if params.spp_count else params.spp
    nl = len(a["lights"])
    accel = orc.ACCEL_LOOP if brute else orc.ACCEL_OBVH
    worst = w * h * ns * 3 * (1 + nl)
    d = orc.dump_rays(scene, params, cap=worst + 16)
    tag = np.ascontiguousarray(d[:, 3]).view(np.uint32)
    kind, depth = tag & 0xff, tag >> 8
    rays = np.zeros(len(d), pyrt.RAY_DTYPE)
    rays["origin"], rays["direction"] = d[:, 0:3], d[:, 4:7]
    closest, shadow = kind == 0, kind == 1
    sample = np.cumsum(closest & (depth == 0)) - 1  # (pixel-major, then the samples of the range in order)
    assert sample[-1] + 1 == w * h * ns, (sample[-1] + 1, w, h, ns)
    # the vertices: the closest rays that hit, in casting order
    cr, cs, cd = rays[closest], sample[closest], depth[closest].astype(np.int64)
    hits = orc.trace(scene, cr, accel=accel)
    hit = (hits["hit"] != 0) & (hits["d"] > 0)
    vr, vs, vd, vh = cr[hit], cs[hit], cd[hit], hits[hit]
    nv = len(vr)
    sr = rays[shadow]
    assert len(sr) == nv * nl, (len(sr), nv, nl)
    occluded = (orc.trace(scene, sr, accel=accel, kind=pyrt.TRACE_ANY)["hit"] != 0).reshape(nv, nl)
    to_light = sr["direction"].reshape(nv, nl, 3)
    mesh = vh["mesh"].astype(np.int64)
    gid = a["tri_begin"].astype(np.int64)[mesh] + vh["tri"]
    tv = a["tri"][gid].astype(np.int64)
    u, v = vh["u"], vh["v"]
    wgt = ((F32(1) - u) - v)[:, None]
    n0, n1, n2 = (a["nrm"][tv[:, k]] for k in range(3))
    nrm = aov_ref._unit((wgt * n0 + u[:, None] * n1) + v[:, None] * n2)
    point = sr["origin"].reshape(nv, nl, 3)[:, 0] if nl else np.zeros((nv, 3), F32)
    c = interpolate(colors, tv, u, v)
    rows = np.zeros((nv, 17), F32)
    rows[:, 0:2], rows[:, 2:5], rows[:, 5:8] = a["materials"][mesh, 0:2], c, a["materials"][mesh, 5:8]
    rows[:, 8:11], rows[:, 14:17] = nrm, -vr["direction"]
    color = np.zeros((nv, 3), F32)
    for l in range(nl):  # from +0 in index order; an occluded light adds nothing
        rows[:, 11:14] = to_light[:, l]
        bsdf = orc.bsdf_rows(rows, orc.MATH_DET)
        lrow = np.zeros((nv, 24), F32)
        lrow[:, :21], lrow[:, 21:] = a["lights"][l], point
        term = (orc.eval_light_rows(lrow) * bsdf).astype(F32)
        color = np.where(occluded[:, l, None], color, (color + term).astype(F32))
    # the samples: c0 + (c1 + (c2 + 0)) over the vertices the sample shaded
    nsmp = w * h * ns
    total = np.zeros((nsmp, 3), F32)
    for dd in (2, 1, 0):
        m = vd == dd
        total[vs[m]] = (color[m] + total[vs[m]]).astype(F32)
    total = clamp01(total).reshape(w * h, ns, 3)
    found = np.zeros(nsmp, bool)
    found[vs[vd == 0]] = True
    found = found.reshape(w * h, ns)
    first = np.zeros((nsmp, 3), F32)
    first[vs[vd == 0]] = c[vd == 0]
    first = first.reshape(w * h, ns, 3)
    acc = np.zeros((w * h, 4), F32)
    alb = np.zeros((w * h, 3), F32)
    for i in range(ns):  # float32 adds in sample order
        acc[:, :3] = (acc[:, :3] + total[:, i]).astype(F32)
        acc[:, 3] = np.where(found[:, i], acc[:, 3] + F32(1), acc[:, 3])
        alb = np.where(found[:, i, None], (alb + first[:, i]).astype(F32), alb)
    acc = acc.reshape(h, w, 4)
    seen = None
    if touched:
        seen = np.zeros((w * h, len(a["tri"])), bool)
        seen[vs // ns, gid] = True
        seen = seen.reshape(h, w, -1)
    out = None if bg is None else lens_ref.resolve(acc, np.asarray(bg, F32), params.spp)
    return dict(accum=acc, out=out, closest=int(closest.sum()), shadow=int(shadow.sum()), albedo=alb.reshape(h, w, 3),
                touched=seen)


# ---- the frames test_gpu_vcol.py compares bit for bit, shared with test_vcol_ref_cpu.py -----------------------------------
# (scene key as lights_ref.scene's, w, h, sample range, mode, max_depth, colouring).  13x9: partial 8x8 wave tiles at both
# edges; 16x16: whole ones.  Every size, range (1, 4, 7 and 3..7 of 7 samples), shading form (ray mode; path mode at depths
# 1, 2, 3), scene (cubes and lowres closed and open: three lights, the pooled body; sweep scenes 1, 2 and 5: one and two
# lights; sweep scene 3: four lights, the sequential body) and colouring appears several times.  FACES cases run on the
# vertex-split scene of their key.
CASES = [
    (("cubes", False), 16, 16, SPP4, PATH, 3, SMOOTH),
    (("cubes", False), 13, 9, SPP7, RAY, 1, FACES),
    (("cubes", False), 13, 9, SPP1, PATH, 2, ALBEDO),
    (("cubes", True), 13, 9, SPP7_34, PATH, 3, SMOOTH),
    (("cubes", True), 16, 16, SPP1, PATH, 2, FACES),
    (("lowres", False), 13, 9, SPP4, PATH, 3, FACES),
    (("lowres", False), 16, 16, SPP1, RAY, 1, SMOOTH),
    (("lowres", True), 13, 9, SPP7, PATH, 2, SMOOTH),
    (("lowres", True), 16, 16, SPP4, PATH, 1, ALBEDO),
    (("sweep", "cubes", 1), 13, 9, SPP4, PATH, 3, SMOOTH),
    (("sweep", "lowres", 2), 16, 16, SPP7_34, PATH, 2, FACES),
    (("sweep", "cubes", 5), 13, 9, SPP1, PATH, 3, SMOOTH),
    (("sweep", "lowres", 3), 16, 16, SPP1, PATH, 3, SMOOTH),
    (("sweep", "cubes", 3), 13, 9, SPP7, RAY, 1, FACES),
    (("sweep", "lowres", 3), 13, 9, SPP7_34, PATH, 2, ALBEDO),
]
# A SMOOTH case must differ from the uncoloured frame in more than this share of its rgb words: half the smallest share
# the reference itself shows over the SMOOTH cases (61.0 %, on the open cubes scene, whose misses change nothing;
# tests/test_vcol_ref_cpu.py measures and prints every share)
MIN_CHANGED = 0.3


def case_id(c):
    key, w, h, rng, mode, depth, colouring = c
    name = "sweep%d_%s" % (key[2], key[1]) if key[0] == "sweep" else key[0] + ("_open" if key[1] else "")
    return "%s-%dx%d-%s-%s%d-%s" % (name, w, h, "+".join(str(v) for v in rng.values()), "path" if mode == PATH else "ray", depth,
                                    colouring)


def case_scene(c):
    """The scene a case's context holds: the key's, vertex-split for FACES."""
    ck = ("vscene", c[0], c[1], c[2], c[6] == FACES)
    if ck not in _cache:
        s = lights_ref.scene(c[0], c[1], c[2])
        _cache[ck] = split_scene(s) if c[6] == FACES else s
    return _cache[ck]


def case_colors(c):
    ck = ("colors", c[0], c[1], c[2], c[6])
    if ck not in _cache:
        s = case_scene(c)
        rgb = albedo_colors(s) if c[6] == ALBEDO else face_colors(s)[0] if c[6] == FACES else smooth_colors(s)
        rgb.setflags(write=False)
        _cache[ck] = rgb
    return _cache[ck]


def case_triangle_scene(c):
    """C2's second scene of a FACES case."""
    s = case_scene(c)
    return per_triangle_scene(s, face_colors(s)[1])


def case_params(c, **kw):
    key, w, h, rng, mode, depth, colouring = c
    args = dict(mode=mode, max_depth=depth, seed=SEED)
    args.update(rng)
    args.update(kw)
    spp = args.pop("spp")
    return pyrt.make_params(w, h, spp, **args)


def case_background(c):
    return lights_ref.case_background(c)


def case_reference(c, brute=False):
    """The reference frame of a case (computed once, shared, never written to)."""
    key = ("ref", case_id(c), brute)
    if key not in _cache:
        ref = frame(case_scene(c), case_params(c), case_colors(c), case_background(c), brute)
        for v in ref.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cache[key] = ref
    return _cache[key]


def plain_frame(scene, c, brute=False):
    """The oracle's own frame of `scene` under a case's parameters: dict(accum, out, closest, shadow)."""
    out, acc, st = orc.render(scene, case_params(c), math_mode=orc.MATH_DET, bg=case_background(c),
                              accel=orc.ACCEL_LOOP if brute else orc.ACCEL_OBVH)
    return dict(accum=acc, out=out, closest=st.rays_closest, shadow=st.rays_shadow)


changed_rgb_words = lights_ref.changed_rgb_words
