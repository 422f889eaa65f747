"""The CPU reference of rt_render_views_shutter_albedo and rt_render_aov_views_albedo (test infrastructure), built only
from parts that exist; it restates nothing about the integrator or the generator.

  1. the primary rays (o, F) of every sample of view j are shutter_ref.shutter_rays with that view's camera, seed and
     record — what views_shutter_ref's expectation uses;
  2. each sample becomes rays_ref's degenerate-camera frame (rays_ref._with_camera, rays_ref._frame_params) with the
     sample's one-sample range and its pixel as the stream index: pixel k of a (k + 1) x 1 frame;
  3. that frame feeds the construction of tex_ref.frame / vcol_ref.frame — orc.dump_rays for the rays, orc.trace for the
     vertices and the occlusions, orc.bsdf_rows with albedo = c and orc.eval_light_rows for the two factors of a term —
     with c from tex_ref.vertex_albedo or vcol_ref.interpolate;
  4. only the last pixel's rays are kept (the others are the stream indices below the sample's);
  5. the samples add up per view in sample order.
The oracle renders k + 1 pixels for the sample of pixel k, so the cost grows with the square of the pixel count: the
frames are 13x9 and 16x16.  tests/test_albedo_views_ref_cpu.py pins this to views_shutter_ref's expectation (albedo texels
and per-mesh colours) and to tex_ref.frame / vcol_ref.frame (a still record, one view) before it judges anything."""
import ctypes as C

import numpy as np

import aov_ref
import lens_ref
import lights_ref
import orc
import pyrt
import rays_ref
import shutter_ref
import tex_ref
import vcol_ref
import views_shutter_ref
from shutter_ref import no_negative_zero, translated, turned
from tex_ref import T_ALBEDO, T_FACES, T_MIXED, T_NONE
from vcol_ref import ALBEDO, FACES, SMOOTH, clamp01

F32 = np.float32
SEED = 17
VIEW_SEEDS = (21, 22, 50000)
SPP1, SPP4, SPP7, SPP7_34 = lens_ref.SPP1, lens_ref.SPP4, lens_ref.SPP7, lens_ref.SPP7_34
RAY, PATH = pyrt.MODE_RAY, pyrt.MODE_PATH
TEX, COL = "tex", "col"
MATERIAL, COLORS, TEXTURES = pyrt.ALBEDO_MATERIAL, pyrt.ALBEDO_COLORS, pyrt.ALBEDO_TEXTURES
_cache = {}


# ---- the surface: what a vertex's albedo is ------------------------------------------------------------------------------
def texture_albedo(tset):
    """c of tex_ref.frame: the mesh's texture at the hit's uv, or the mesh's own albedo."""
    return lambda a, mesh, tv, u, v: tex_ref.vertex_albedo(a, tset, mesh, tv, u, v)


def color_albedo(colors):
    """c of vcol_ref.frame: the interpolated vertex colour."""
    return lambda a, mesh, tv, u, v: vcol_ref.interpolate(colors, tv, u, v)


# ---- one view ---------------------------------------------------------------------------------------------------------------
def _last_pixel_rays(scene, o, ll, k, p1):
    """Steps 2 and 4: the rays [n][8] (orc.dump_rays' rows) of pixel k of the (k + 1) x 1 degenerate-camera frame."""
    cs = rays_ref._with_camera(scene, o, ll)
    nl = len(scene.arrays()["lights"])
    d = orc.dump_rays(cs, rays_ref._frame_params(p1, k + 1), cap=(k + 1) * 3 * (1 + nl) + 16)
    tag = np.ascontiguousarray(d[:, 3]).view(np.uint32)
    pixel = np.cumsum(((tag & 0xff) == 0) & ((tag >> 8) == 0)) - 1  # (one sample per pixel: pixel-major)
    assert pixel[-1] == k, (pixel[-1], k)
    return d[pixel == k]


def view_frame(scene, cam, rec, params, albedo_of, brute=False):
    """View `cam` of `scene` under the record `rec` (views_shutter_ref.record's dict) with params (its seed the view's):
    dict(accum [h][w][4], closest, shadow, albedo [h][w][3]: the first-hit sums of c)."""
    a = scene.arrays()
    w, h = params.width, params.height
    s0, s1 = lens_ref.sample_range(params)
    ns, nl = s1 - s0, len(a["lights"])
    accel = orc.ACCEL_LOOP if brute else orc.ACCEL_OBVH
    o, F = shutter_ref.shutter_rays(cam, rec["camera_close"], params, rec["open"], rec["close"], rec["aperture"], rec["focus_distance"])
    chunks, owner = [], []
    for y in range(h):
        for x in range(w):
            for i in range(s0, s1):
                d = _last_pixel_rays(scene, o[y, x, i - s0], F[y, x, i - s0], y * w + x, lens_ref._one_sample(params, i))
                chunks.append(d)
                owner.append(np.full(len(d), (y * w + x) * ns + (i - s0), np.int64))
    d, sample_of = np.concatenate(chunks), np.concatenate(owner)
    # step 3: tex_ref.frame's construction over the kept rays (pixel-major, then the samples of the range in order)
    tag = np.ascontiguousarray(d[:, 3]).view(np.uint32)
    kind, depth = tag & 0xff, tag >> 8
    rays = np.zeros(len(d), pyrt.RAY_DTYPE)
    rays["origin"], rays["direction"] = d[:, 0:3], d[:, 4:7]
    closest, shadow = kind == 0, kind == 1
    cr, cs, cd = rays[closest], sample_of[closest], depth[closest].astype(np.int64)
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
    c = albedo_of(a, mesh, tv, u, v)
    rows = np.zeros((nv, 17), F32)
    rows[:, 0:2], rows[:, 2:5], rows[:, 5:8] = a["materials"][mesh, 0:2], c, a["materials"][mesh, 5:8]
    rows[:, 8:11], rows[:, 14:17] = nrm, -vr["direction"]
    color = np.zeros((nv, 3), F32)
    for l in range(nl):
        rows[:, 11:14] = to_light[:, l]
        bsdf = orc.bsdf_rows(rows, orc.MATH_DET)
        lrow = np.zeros((nv, 24), F32)
        lrow[:, :21], lrow[:, 21:] = a["lights"][l], point
        term = (orc.eval_light_rows(lrow) * bsdf).astype(F32)
        color = np.where(occluded[:, l, None], color, (color + term).astype(F32))
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
    # step 5
    acc = np.zeros((w * h, 4), F32)
    alb = np.zeros((w * h, 3), F32)
    for i in range(ns):
        acc[:, :3] = (acc[:, :3] + total[:, i]).astype(F32)
        acc[:, 3] = np.where(found[:, i], acc[:, 3] + F32(1), acc[:, 3])
        alb = np.where(found[:, i, None], (alb + first[:, i]).astype(F32), alb)
    return dict(accum=acc.reshape(h, w, 4), closest=int(closest.sum()), shadow=int(shadow.sum()), albedo=alb.reshape(h, w, 3))


# ---- records ----------------------------------------------------------------------------------------------------------------
def record(kind, cam, lens, move=shutter_ref.SMALL):
    """views_shutter_ref.record's kinds and "turn_lens": a moved and turned camera_close over (0.25, 0.5) with a lens."""
    if kind != "turn_lens":
        return views_shutter_ref.record(kind, cam, lens, move)
    r = views_shutter_ref.record("turn", cam, lens, move)
    r["aperture"], r["focus_distance"] = lens_ref.APERTURES[lens[0]], lens_ref.FOCUS[lens[1]]
    return r


# ---- the cases test_gpu_albedo_views.py compares bit for bit, shared with test_albedo_views_ref_cpu.py -------------------
# (scene key as lights_ref.scene's, w, h, sample range, mode, max_depth, surface, the views' kinds, lens = (aperture, focus)
# as indices into lens_ref.APERTURES / lens_ref.FOCUS, seeds per view or None).  surface: (TEX, one of tex_ref's sets) or
# (COL, one of vcol_ref's colourings).  One, two and three views; within a call a still pinhole view ("none"), a lens alone
# ("lens") and a moved and turned camera with a lens ("turn_lens"), in every position of the launch.  13x9: partial 8x8
# wave tiles at both edges; 16x16: whole ones; the views of one tile row share a launch.  Ranges 1, 4, 7 and 3..7 of 7; ray
# mode and path depths 1 to 3; cubes and lowres closed and open (three lights, the pooled body), sweep scenes of one, two
# and four lights (scene 3: the sequential body).  T_MIXED's shift is the case's index (tex_ref.texture_set): the seven
# cases below with T_MIXED sample between them every texture of MIXED_TEXTURES, the RT_TEX_NONE mesh beside them
# (test_albedo_views_ref_cpu.py checks that).  FACES / T_FACES cases run on the vertex-split scene of their key.
CASES = [
    (("cubes", False), 13, 9, SPP4, PATH, 3, (TEX, T_MIXED), ("none", "lens", "turn_lens"), (0, 0), VIEW_SEEDS),
    (("cubes", True), 16, 16, SPP1, PATH, 2, (TEX, T_MIXED), ("turn_lens", "none"), (1, 0), None),
    (("lowres", False), 13, 9, SPP7_34, PATH, 3, (COL, SMOOTH), ("lens", "turn_lens", "none"), (1, 1), VIEW_SEEDS),
    (("lowres", True), 13, 9, SPP7, RAY, 1, (TEX, T_MIXED), ("lens",), (0, 1), None),
    (("sweep", "cubes", 3), 13, 9, SPP4, PATH, 2, (TEX, T_MIXED), ("turn_lens", "lens"), (0, 0), VIEW_SEEDS[:2]),
    (("sweep", "lowres", 1), 16, 16, SPP1, PATH, 3, (COL, SMOOTH), ("none", "turn_lens"), (1, 0), None),
    (("sweep", "cubes", 2), 13, 9, SPP7, PATH, 1, (TEX, T_MIXED), ("turn_lens",), (0, 1), (VIEW_SEEDS[2],)),
    (("sweep", "lowres", 3), 13, 9, SPP1, PATH, 3, (COL, SMOOTH), ("lens", "none", "turn_lens"), (0, 0), VIEW_SEEDS),
    (("lowres", False), 16, 16, SPP1, RAY, 1, (TEX, T_MIXED), ("none", "lens"), (1, 1), None),
    (("cubes", True), 13, 9, SPP4, PATH, 3, (TEX, T_MIXED), ("lens", "turn_lens"), (1, 0), VIEW_SEEDS[1:]),
    # X3's and X4's data: compared with the library's own rt_render_views_shutter, and by the CPU test with the oracle
    (("cubes", False), 13, 9, SPP4, PATH, 3, (TEX, T_ALBEDO), ("turn_lens", "none", "lens"), (0, 0), VIEW_SEEDS),
    (("lowres", True), 13, 9, SPP1, PATH, 2, (TEX, T_NONE), ("lens", "turn_lens"), (1, 0), None),
    (("sweep", "cubes", 3), 13, 9, SPP4, RAY, 1, (COL, ALBEDO), ("none", "turn_lens"), (0, 1), None),
    (("cubes", False), 13, 9, SPP4, PATH, 2, (TEX, T_FACES), ("lens", "turn_lens"), (0, 0), VIEW_SEEDS[:2]),
    (("sweep", "lowres", 3), 13, 9, SPP1, PATH, 3, (COL, FACES), ("turn_lens", "none", "lens"), (1, 1), None),
]
MIXED = [c for c in CASES if c[6][1] in (T_MIXED, SMOOTH)]
# A mixed case must differ from the untextured rt_render_views_shutter frame in more than MIN_CHANGED_SURFACE of its rgb
# words, and from the still frame with the same surface (every record "none") in more than MIN_CHANGED_OPTICS of them:
# half the smallest shares the reference itself shows over MIXED (tests/test_albedo_views_ref_cpu.py measures and prints
# every share).  Measured: the surface 15.4 % at least (sweep2_cubes-13x9-7-path1-tex-mixed-turn_lens, one vertex per
# path on sweep scene 2's materials; the next is 29.2 %), the optics 29.4 % at least (cubes_open-16x16-1-path2-tex-mixed-
# turn_lens+none: an open scene, whose misses change nothing, with the still view as one of its two).
MIN_CHANGED_SURFACE = 0.075
MIN_CHANGED_OPTICS = 0.145


def case_id(c):
    key, w, h, rng, mode, depth, surface, kinds, lens, seeds = c
    name = "sweep%d_%s" % (key[2], key[1]) if key[0] == "sweep" else key[0] + ("_open" if key[1] else "")
    return "%s-%dx%d-%s-%s%d-%s-%s-%s" % (name, w, h, "+".join(str(v) for v in rng.values()), "path" if mode == PATH else "ray", depth,
                                          "-".join(surface), "+".join(kinds), "seeds" if seeds else "oneseed")


def albedo_of_case(c):
    """The `albedo` argument of a case."""
    return TEXTURES if c[6][0] == TEX else COLORS


def n_views(c):
    return len(c[7])


def case_scene(c):
    """The scene a case's context holds: the key's, vertex-split for the per-face surfaces."""
    ck = ("scene", c[0], c[1], c[2], c[6][1] in (T_FACES, FACES))
    if ck not in _cache:
        s = lights_ref.scene(c[0], c[1], c[2])
        no_negative_zero(s.arrays()["camera"])
        _cache[ck] = vcol_ref.split_scene(s) if ck[4] else s
    return _cache[ck]


def case_surface(c):
    """The resident data of a case: tex_ref.texture_set's dict, or the colours [n_vertices][3]."""
    ck = ("surface", c[0], c[1], c[2], c[6], CASES.index(c) if c[6][1] == T_MIXED else 0)
    if ck not in _cache:
        s = case_scene(c)
        if c[6][0] == TEX:
            x = tex_ref.texture_set(s, c[6][1], CASES.index(c))
            arrays = [x["mesh_texture"], x["uv"]] + [t[0] for t in x["textures"]]
        else:
            x = vcol_ref.albedo_colors(s) if c[6][1] == ALBEDO else vcol_ref.face_colors(s)[0] if c[6][1] == FACES else vcol_ref.smooth_colors(s)
            arrays = [x]
        for arr in arrays:
            arr.setflags(write=False)
        _cache[ck] = x
    return _cache[ck]


def set_surface(ctx, c):
    """Make the case's surface resident on a context."""
    if c[6][0] == TEX:
        ctx.set_textures(*tex_ref.set_args(case_surface(c)))
    else:
        ctx.set_vertex_colors(case_surface(c))


def case_albedo_fn(c):
    x = case_surface(c)
    return texture_albedo(x) if c[6][0] == TEX else color_albedo(x)


def case_triangle_scene(c):
    """X4's other side of a per-face case: the vertex-split scene with every triangle a mesh of its own."""
    s = case_scene(c)
    return vcol_ref.per_triangle_scene(s, vcol_ref.face_colors(s)[1])


def case_cameras(c):
    """float32 [n][4][3]: the scene's camera first, then others on its orbit."""
    return views_shutter_ref.orbit(case_scene(c).arrays()["camera"], views_shutter_ref.ORBIT_DEGREES, views_shutter_ref.ORBIT_SCALES)[:n_views(c)]


def case_seeds(c):
    return None if c[9] is None else list(c[9])


def case_records(c, still=False):
    """The views' records (dicts); still: every view's "none" record instead."""
    return [record("none" if still else kind, cam, c[8]) for kind, cam in zip(c[7], case_cameras(c))]


def case_shutters(c, still=False):
    return [views_shutter_ref.shutter_of(r) for r in case_records(c, still)]


def case_params(c, **kw):
    key, w, h, rng, mode, depth = c[:6]
    args = dict(mode=mode, max_depth=depth, seed=SEED)
    args.update(rng)
    args.update(kw)
    spp = args.pop("spp")
    return pyrt.make_params(w, h, spp, **args)


def case_background(c):
    return lights_ref.case_background(c)


def view_params(c, j, **kw):
    """The case's params with view j's seed."""
    q = case_params(c, **kw)
    if c[9] is not None:
        q.seed = c[9][j]
    return q


def samples_of(c):
    s0, s1 = lens_ref.sample_range(case_params(c))
    return n_views(c) * c[1] * c[2] * (s1 - s0)


def _frozen(ref):
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


def frames(c, albedo_fn, brute=False, still=False):
    """The expectation of the call on a case's scene, views and records under any surface: dict(accum [n][h][w][4], out
    [n][h][w][3], closest, shadow — sums over the views —, albedo [n][h][w][3])."""
    bg = case_background(c)
    views = [view_frame(case_scene(c), cam, rec, view_params(c, j), albedo_fn, brute)
             for j, (cam, rec) in enumerate(zip(case_cameras(c), case_records(c, still)))]
    acc = np.stack([v["accum"] for v in views])
    return dict(accum=acc, out=np.stack([lens_ref.resolve(v["accum"], bg, case_params(c).spp) for v in views]),
                closest=sum(v["closest"] for v in views), shadow=sum(v["shadow"] for v in views),
                albedo=np.stack([v["albedo"] for v in views]))


def case_reference(c, brute=False, still=False):
    """The expectation of a case (computed once, shared, never written to)."""
    key = ("ref", case_id(c), brute, still)
    if key not in _cache:
        _cache[key] = _frozen(frames(c, case_albedo_fn(c), brute, still))
    return _cache[key]


def plain_reference(c, brute=False):
    """views_shutter_ref's own construction of the case's call with the meshes' albedo — shutter_ref.expected per view,
    lens_ref.chained_rows' oracle rows: dict(accum, out, closest, shadow).  On the per-face cases: of the scene with
    every triangle a mesh of its own (X4)."""
    key = ("plain", case_id(c), brute)
    if key not in _cache:
        bg = case_background(c)
        s = case_triangle_scene(c) if c[6][1] in (T_FACES, FACES) else case_scene(c)
        views = []
        for j, (cam, rec) in enumerate(zip(case_cameras(c), case_records(c))):
            views.append(shutter_ref.expected(shutter_ref.with_camera(s, cam), rec["camera_close"], view_params(c, j), rec["open"],
                                              rec["close"], rec["aperture"], rec["focus_distance"],
                                              accel=orc.ACCEL_LOOP if brute else orc.ACCEL_OBVH, bg=bg))
        _cache[key] = _frozen(dict(accum=np.stack([v["accum"] for v in views]), out=np.stack([v["out"] for v in views]),
                                   closest=sum(v["closest"] for v in views), shadow=sum(v["shadow"] for v in views)))
    return _cache[key]


changed_rgb_words = lights_ref.changed_rgb_words
