"""The CPU reference of rt_render_textured and rt_render_aov_textured (test infrastructure), from the oracle's own parts.

It is vcol_ref.frame's construction — orc.dump_rays for the rays, orc.trace for the vertices and the occlusions,
orc.bsdf_rows with albedo = c and orc.eval_light_rows for the two factors of a term — with c from the sampler of
include/rt_amd.h, restated here in numpy float32 with every operation rounded on its own: the hit's uv per axis,
s = (s0 + u (s1 - s0)) + v (s2 - s0); the nearest texel or the bilinear combination a + fy (b - a) of two rows; REPEAT as
the non-negative remainder and CLAMP as min(max(i, 0), N - 1).  A mesh without a texture keeps its material's albedo.
Besides the sampler only the products radiance * bsdf and the sums are stated here, in vcol_ref.frame's orders.
tests/test_tex_ref_cpu.py pins them to the oracle's own frames (T1 and T2 of include/rt_amd.h)."""
import numpy as np

import aov_ref
import lens_ref
import lights_ref
import orc
import pyrt
from vcol_ref import (F32, PATH, RAY, SEED, SPP1, SPP4, SPP7, SPP7_34, clamp01, face_colors, per_triangle_scene,
                      plain_frame, split_scene)

_cache = {}
NONE = pyrt.TEX_NONE
REPEAT, CLAMP = pyrt.TEX_REPEAT, pyrt.TEX_CLAMP
NEAREST, BILINEAR = pyrt.TEX_NEAREST, pyrt.TEX_BILINEAR
T_NONE, T_ALBEDO, T_FACES, T_MIXED = "none", "albedo", "faces", "mixed"


# ---- the sampler -----------------------------------------------------------------------------------------------------------
def wrap(i, n, mode):
    """The texel index of the integer coordinate i on an axis of n texels."""
    i = np.asarray(i, np.int64)
    return np.clip(i, 0, n - 1) if mode == CLAMP else np.mod(i, n)


def coord(s0, s1, s2, u, v):
    """s = (s0 + u (s1 - s0)) + v (s2 - s0) in float32."""
    s0, s1, s2, u, v = (np.asarray(x, F32) for x in (s0, s1, s2, u, v))
    return ((s0 + (u * (s1 - s0)).astype(F32)).astype(F32) + (v * (s2 - s0)).astype(F32)).astype(F32)


def sample(tex, s, t, parts=False):
    """The sample [n][3] of tex = (texels [h][w][3], wrap_s, wrap_t, filter) at the float32 coordinates s, t [n].  parts:
    also a dict of what the sample went through, [n] each — sw, th: the float32 products s * W and t * H; xi, yj: the
    integer coordinates before the wrap (NEAREST: the texel's; BILINEAR: int(xf), int(yf)); i0, i1, j0, j1: the wrapped
    indices (NEAREST: i1 == i0, j1 == j0); fx, fy (NEAREST: 0) — and bilinear, a bool."""
    texels, wrap_s, wrap_t, filt = tex
    texels = np.asarray(texels, F32)
    h, w = texels.shape[:2]
    s, t = np.asarray(s, F32), np.asarray(t, F32)
    sw, th = (s * F32(w)).astype(F32), (t * F32(h)).astype(F32)
    if filt == NEAREST:
        xi, yj = np.floor(sw).astype(np.int64), np.floor(th).astype(np.int64)
        i = wrap(xi, w, wrap_s)
        j = wrap(yj, h, wrap_t)
        if parts:
            zero = np.zeros(s.shape, F32)
            return texels[j, i], dict(sw=sw, th=th, xi=xi, yj=yj, i0=i, i1=i, j0=j, j1=j, fx=zero, fy=zero, bilinear=False)
        return texels[j, i]
    x = (sw - F32(0.5)).astype(F32)
    y = (th - F32(0.5)).astype(F32)
    xf, yf = np.floor(x).astype(F32), np.floor(y).astype(F32)
    fx, fy = (x - xf).astype(F32)[..., None], (y - yf).astype(F32)[..., None]
    i0, i1 = wrap(xf, w, wrap_s), wrap(xf.astype(np.int64) + 1, w, wrap_s)
    j0, j1 = wrap(yf, h, wrap_t), wrap(yf.astype(np.int64) + 1, h, wrap_t)
    with np.errstate(over="ignore", invalid="ignore"):  # (texels near the float32 range: the sums may overflow, as they do on the device)
        a = (texels[j0, i0] + (fx * (texels[j0, i1] - texels[j0, i0]).astype(F32)).astype(F32)).astype(F32)
        b = (texels[j1, i0] + (fx * (texels[j1, i1] - texels[j1, i0]).astype(F32)).astype(F32)).astype(F32)
        c = (a + (fy * (b - a).astype(F32)).astype(F32)).astype(F32)
    if parts:
        return c, dict(sw=sw, th=th, xi=xf.astype(np.int64), yj=yf.astype(np.int64), i0=i0, i1=i1, j0=j0, j1=j1, fx=fx[..., 0],
                       fy=fy[..., 0], bilinear=True)
    return c


def vertex_albedo(a, tset, mesh, tv, u, v):
    """The albedo c [n][3] of the vertices (mesh, vertex ids tv, barycentrics u, v): the mesh's texture at the hit's uv,
    or the mesh's own albedo."""
    c = np.ascontiguousarray(a["materials"][mesh, 2:5], F32).copy()
    uv = np.asarray(tset["uv"], F32)
    which = np.asarray(tset["mesh_texture"], np.uint32)[mesh]
    for k, tex in enumerate(tset["textures"]):
        m = which == k
        if m.any():
            q = tv[m]
            s = coord(uv[q[:, 0], 0], uv[q[:, 1], 0], uv[q[:, 2], 0], u[m], v[m])
            t = coord(uv[q[:, 0], 1], uv[q[:, 1], 1], uv[q[:, 2], 1], u[m], v[m])
            c[m] = sample(tex, s, t)
    return c


# ---- the frame -------------------------------------------------------------------------------------------------------------
def frame(scene, params, tset, bg=None, brute=False, touched=True):
    """The textured frame `params` describes: dict(accum [h][w][4], out [h][w][3] or None, closest, shadow, albedo
    [h][w][3] — the first-hit sums of c, rt_render_aov_textured's albedo channel — and touched [h][w][n_meshes] bool: the
    meshes the pixel's paths shaded a vertex on)."""
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
    sample_of = np.cumsum(closest & (depth == 0)) - 1  # (pixel-major, then the samples of the range in order)
    assert sample_of[-1] + 1 == w * h * ns, (sample_of[-1] + 1, w, h, ns)
    # the vertices: the closest rays that hit, in casting order
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
    c = vertex_albedo(a, tset, mesh, tv, u, v)
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
        with np.errstate(over="ignore"):  # (texels near the float32 range sum to inf, here as on the device)
            alb = np.where(found[:, i, None], (alb + first[:, i]).astype(F32), alb)
    acc = acc.reshape(h, w, 4)
    seen = None
    if touched:
        seen = np.zeros((w * h, len(a["tri_begin"]) - 1), bool)
        seen[vs // ns, mesh] = True
        seen = seen.reshape(h, w, -1)
    out = None if bg is None else lens_ref.resolve(acc, np.asarray(bg, F32), params.spp)
    return dict(accum=acc, out=out, closest=int(closest.sum()), shadow=int(shadow.sum()), albedo=alb.reshape(h, w, 3),
                touched=seen)


# ---- texture sets ----------------------------------------------------------------------------------------------------------
# the sizes (w, h) of T_MIXED's textures with their wraps and filter: every size of the issue, both filters, both wraps on
# either axis, mixed
MIXED_TEXTURES = [((5, 3), REPEAT, CLAMP, BILINEAR), ((1, 1), CLAMP, CLAMP, BILINEAR), ((64, 32), CLAMP, REPEAT, NEAREST),
                  ((1, 5), REPEAT, REPEAT, BILINEAR), ((2, 2), REPEAT, REPEAT, NEAREST), ((5, 3), CLAMP, CLAMP, NEAREST),
                  ((64, 32), REPEAT, REPEAT, BILINEAR)]


def random_texels(w, h, seed):
    """Texels in [0.02, 1), every seventh 0 and every fifth above 1."""
    t = np.random.default_rng(seed).uniform(0.02, 1.0, (h, w, 3)).astype(F32)
    flat = t.reshape(-1, 3)
    flat[np.arange(len(flat)) % 5 == 0] *= F32(1.7)
    flat[np.arange(len(flat)) % 7 == 3] = 0
    return t


def spread_uv(s):
    """One uv per vertex from its position and a hash: inside [0, 1] for a third of the vertices, beyond it on both sides
    for a third (-2.5 .. 3.5), and on multiples of 1/4 — texel edges of the 2x2 texture, and of the 64x32 one — for the
    rest."""
    a = s.arrays()
    pos = a["pos"].astype(np.float64)
    ext = np.maximum(pos.max(axis=0) - pos.min(axis=0), 1e-9)
    q = (pos - pos.min(axis=0)) / ext
    n = len(pos)
    hsh = ((np.arange(n, dtype=np.uint64) * np.uint64(2654435761)) % np.uint64(1 << 32)).astype(np.float64) / float(1 << 32)
    uv = np.stack([0.6 * q[:, 0] + 0.4 * q[:, 2], 0.7 * q[:, 1] + 0.3 * hsh], axis=1)
    k = np.arange(n) % 3
    uv[k == 1] = uv[k == 1] * 6.0 - 2.5
    uv[k == 2] = np.round(uv[k == 2] * 12.0 - 4.0) / 4.0
    return np.ascontiguousarray(uv, F32)


def texture_set(s, kind, shift=0):
    """dict(textures=[(texels, wrap_s, wrap_t, filter)], mesh_texture [n_meshes] uint32, uv [n_vertices][2]) of a kind on
    the scene s (T_FACES: s is vertex-split).  shift (T_MIXED): mesh m takes texture (m + shift) mod the set's count, so
    that the cases between them sample every texture of the set from scenes of five meshes."""
    a = s.arrays()
    nm, nvtx = len(a["tri_begin"]) - 1, len(a["pos"])
    if kind == T_NONE:  # T1: no mesh has a texture (a set holds one texture at least)
        return dict(textures=[(random_texels(2, 2, 1), REPEAT, REPEAT, BILINEAR)], mesh_texture=np.full(nm, NONE, np.uint32),
                    uv=spread_uv(s))
    if kind == T_ALBEDO:  # T1: every textured mesh's texels equal its albedo, whatever the uvs, filter and wrap
        tex = []
        for m in range(nm):
            (w, h), ws, wt, f = MIXED_TEXTURES[m % len(MIXED_TEXTURES)]
            tex.append((np.broadcast_to(a["materials"][m, 2:5].astype(F32), (h, w, 3)).copy(), ws, wt, f))
        return dict(textures=tex, mesh_texture=np.arange(nm, dtype=np.uint32), uv=spread_uv(s))
    if kind == T_FACES:  # T2: triangle k of n at ((3k + 1.5) / (3n), 0.5) of a 3n x 1 texture, texels 3k .. 3k+2 its colour
        nt = len(a["tri"])
        assert nvtx == 3 * nt and 3 * nt <= pyrt.TEX_MAX_SIDE
        face = face_colors(s)[1]
        texels = np.repeat(face, 3, axis=0).reshape(1, 3 * nt, 3)
        uv = np.zeros((nvtx, 2), F32)
        uv[:, 0] = np.repeat(((3.0 * np.arange(nt) + 1.5) / (3.0 * nt)).astype(F32), 3)
        uv[:, 1] = F32(0.5)
        filt = BILINEAR if nt % 2 else NEAREST
        return dict(textures=[(texels, REPEAT if nt % 3 else CLAMP, CLAMP, filt), (texels, CLAMP, REPEAT, BILINEAR + NEAREST - filt)],
                    mesh_texture=(np.arange(nm) % 2).astype(np.uint32), uv=uv)
    assert kind == T_MIXED
    tex = [(random_texels(w, h, 10 + k), ws, wt, f) for k, ((w, h), ws, wt, f) in enumerate(MIXED_TEXTURES)]
    which = ((np.arange(nm) + shift) % len(tex)).astype(np.uint32)
    if nm > 1:
        which[nm - 1] = NONE  # one mesh without a texture beside them
    return dict(textures=tex, mesh_texture=which, uv=spread_uv(s))


# ---- the frames test_gpu_tex.py compares bit for bit, shared with test_tex_ref_cpu.py --------------------------------------
# (scene key as lights_ref.scene's, w, h, sample range, mode, max_depth, texturing): vcol_ref.CASES' frames, ranges, modes
# and scenes — cubes and lowres closed and open (three lights, the pooled body), sweep scenes of one, two and four lights
# (scene 3: the sequential body) — under the four texturings.  T_FACES cases run on the vertex-split scene of their key.
# (These scenes keep uvs within -2.5 .. 3.5 and textures within 64 x 32; the sampler at the header's bounds is run on the
# probe card of tests/probe_card.py, by tests/test_gpu_surface_limits.py.)
CASES = [
    (("cubes", False), 16, 16, SPP4, PATH, 3, T_MIXED),
    (("cubes", False), 13, 9, SPP7, RAY, 1, T_FACES),
    (("cubes", False), 13, 9, SPP1, PATH, 2, T_ALBEDO),
    (("cubes", True), 13, 9, SPP7_34, PATH, 3, T_MIXED),
    (("cubes", True), 16, 16, SPP1, PATH, 2, T_FACES),
    (("lowres", False), 13, 9, SPP4, PATH, 3, T_FACES),
    (("lowres", False), 16, 16, SPP1, RAY, 1, T_MIXED),
    (("lowres", True), 13, 9, SPP7, PATH, 2, T_MIXED),
    (("lowres", True), 16, 16, SPP4, PATH, 1, T_NONE),
    (("sweep", "cubes", 1), 13, 9, SPP4, PATH, 3, T_MIXED),
    (("sweep", "lowres", 2), 16, 16, SPP7_34, PATH, 2, T_FACES),
    (("sweep", "cubes", 5), 13, 9, SPP1, PATH, 3, T_MIXED),
    (("sweep", "lowres", 3), 16, 16, SPP1, PATH, 3, T_MIXED),
    (("sweep", "cubes", 3), 13, 9, SPP7, RAY, 1, T_FACES),
    (("sweep", "lowres", 3), 13, 9, SPP7_34, PATH, 2, T_ALBEDO),
]
# A T_MIXED case must differ from the plain frame in more than this share of its rgb words: half the smallest share the
# reference itself shows over the T_MIXED cases (55.6 %, on the open scenes at 13x9, whose misses change nothing;
# tests/test_tex_ref_cpu.py measures and prints every share)
MIN_CHANGED = 0.275


def case_id(c):
    key, w, h, rng, mode, depth, kind = c
    name = "sweep%d_%s" % (key[2], key[1]) if key[0] == "sweep" else key[0] + ("_open" if key[1] else "")
    return "%s-%dx%d-%s-%s%d-%s" % (name, w, h, "+".join(str(v) for v in rng.values()), "path" if mode == PATH else "ray", depth, kind)


def case_scene(c):
    """The scene a case's context holds: the key's, vertex-split for T_FACES."""
    ck = ("tscene", c[0], c[1], c[2], c[6] == T_FACES)
    if ck not in _cache:
        s = lights_ref.scene(c[0], c[1], c[2])
        _cache[ck] = split_scene(s) if c[6] == T_FACES else s
    return _cache[ck]


def case_textures(c):
    ck = ("tset", c[0], c[1], c[2], c[6])
    if ck not in _cache:
        t = texture_set(case_scene(c), c[6], CASES.index(c))
        for arr in [t["mesh_texture"], t["uv"]] + [x[0] for x in t["textures"]]:
            arr.setflags(write=False)
        _cache[ck] = t
    return _cache[ck]


def set_args(t):
    """Context.set_textures' arguments of a texture set."""
    return t["textures"], t["mesh_texture"], t["uv"]


def case_face_colors(c):
    """T2's other sides of a T_FACES case: (the colours per vertex for rt_render_colors, the per-triangle scene)."""
    s = case_scene(c)
    rgb, face = face_colors(s)
    return rgb, per_triangle_scene(s, face)


def case_params(c, **kw):
    key, w, h, rng, mode, depth, kind = c
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
        ref = frame(case_scene(c), case_params(c), case_textures(c), case_background(c), brute)
        for v in ref.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cache[key] = ref
    return _cache[key]


changed_rgb_words = lights_ref.changed_rgb_words
