"""The CPU reference of rt_render_material (test infrastructure), from the oracle's own parts.

It is tex_ref.frame's construction — orc.dump_rays for the rays, orc.trace for the vertices and the occlusions,
orc.bsdf_rows and orc.eval_light_rows for the two factors of a term, the products and the sums in tex_ref.frame's orders —
with two more columns of orc.bsdf_rows filled per vertex: rows[:, 5:8] (f0) from the rgb sample of the mesh's f0 texture and
rows[:, 0:2] (kd, alpha) from the r and g of the sample of its (kd, alpha) texture, through tex_ref.coord and
tex_ref.sample at the same hit coordinate as the albedo's; RT_TEX_NONE keeps the mesh's own.  The frame integrator draws
its bounce from the shading normal alone, so no material field moves a ray: the rays are orc.dump_rays' of the plain scene.
tests/test_mat_ref_cpu.py pins it to the oracle's own frames (M1 and M2 of include/rt_amd.h)."""
import numpy as np

import aov_ref
import lens_ref
import orc
import pyrt
import tex_ref
from tex_ref import (BILINEAR, CLAMP, F32, MIXED_TEXTURES, NEAREST, NONE, REPEAT, T_ALBEDO, T_FACES, T_MIXED, T_NONE, case_id,
                     case_params, case_background, case_scene, clamp01)

_cache = {}
CASES = tex_ref.CASES


def table(mset, name, nm):
    """A map table of the set as [n_meshes] uint32 (None: RT_TEX_NONE on every mesh)."""
    t = mset.get(name)
    return np.full(nm, NONE, np.uint32) if t is None else np.asarray(t, np.uint32)


def vertex_sample(mset, which, mesh, tv, u, v, own):
    """[n][3]: per vertex the sample of texture which[mesh] of the set at the hit's uv, or own[n][3] on RT_TEX_NONE."""
    c = np.ascontiguousarray(own, F32).copy()
    uv = np.asarray(mset["uv"], F32)
    idx = which[mesh]
    for k, tex in enumerate(mset["textures"]):
        m = idx == k
        if m.any():
            q = tv[m]
            s = tex_ref.coord(uv[q[:, 0], 0], uv[q[:, 1], 0], uv[q[:, 2], 0], u[m], v[m])
            t = tex_ref.coord(uv[q[:, 0], 1], uv[q[:, 1], 1], uv[q[:, 2], 1], u[m], v[m])
            c[m] = tex_ref.sample(tex, s, t)
    return c


def frame(scene, params, mset, bg=None, brute=False):
    """The material-map frame `params` describes: dict(accum [h][w][4], out [h][w][3] or None, closest, shadow, nonfinite —
    how many rgb words of the samples' sums were not finite before the clamp).  mset: a
    texture set of tex_ref's form with mesh_f0 and mesh_kd_alpha beside mesh_texture (either None)."""
    a = scene.arrays()
    w, h = params.width, params.height
    ns = params.spp_count if params.spp_count else params.spp
    nl = len(a["lights"])
    nm = len(a["tri_begin"]) - 1
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
    mats = a["materials"]
    kda_own = np.concatenate([mats[mesh, 0:2], np.zeros((nv, 1), F32)], axis=1)
    rows = np.zeros((nv, 17), F32)
    rows[:, 2:5] = tex_ref.vertex_albedo(a, mset, mesh, tv, u, v)
    rows[:, 5:8] = vertex_sample(mset, table(mset, "mesh_f0", nm), mesh, tv, u, v, mats[mesh, 5:8])
    rows[:, 0:2] = vertex_sample(mset, table(mset, "mesh_kd_alpha", nm), mesh, tv, u, v, kda_own)[:, 0:2]
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
    nonfinite = int((~np.isfinite(total)).sum())
    total = clamp01(total).reshape(w * h, ns, 3)
    found = np.zeros(nsmp, bool)
    found[vs[vd == 0]] = True
    found = found.reshape(w * h, ns)
    acc = np.zeros((w * h, 4), F32)
    for i in range(ns):  # float32 adds in sample order
        acc[:, :3] = (acc[:, :3] + total[:, i]).astype(F32)
        acc[:, 3] = np.where(found[:, i], acc[:, 3] + F32(1), acc[:, 3])
    acc = acc.reshape(h, w, 4)
    out = None if bg is None else lens_ref.resolve(acc, np.asarray(bg, F32), params.spp)
    return dict(accum=acc, out=out, closest=int(closest.sum()), shadow=int(shadow.sum()), nonfinite=nonfinite)


# ---- map sets --------------------------------------------------------------------------------------------------------------
def kd_alpha_texels(w, h, seed):
    """(kd, alpha, b) texels: r uniform in [0, 1), g uniform in [0.05, 1), b uniform in [-5, 5) — b is never read, and a
    read of it would show."""
    g = np.random.default_rng(seed)
    return np.stack([g.uniform(0.0, 1.0, (h, w)), g.uniform(0.05, 1.0, (h, w)), g.uniform(-5.0, 5.0, (h, w))], axis=-1).astype(F32)


def face_fields(s):
    """The strips' per-triangle values on a split scene: (albedo [nt][3], as tex_ref's T_FACES set holds it; f0 [nt][3] in
    [0, 1); kd [nt] in [0, 1); alpha [nt] in [0.05, 1))."""
    nt = len(s.arrays()["tri"])
    g = np.random.default_rng(1000 + nt)
    f0 = g.uniform(0.0, 1.0, (nt, 3)).astype(F32)
    kd = g.uniform(0.0, 1.0, nt).astype(F32)
    alpha = g.uniform(0.05, 1.0, nt).astype(F32)
    return tex_ref.face_colors(s)[1], f0, kd, alpha


def map_set(s, kind, shift=0):
    """tex_ref.texture_set(s, kind, shift) with the maps' textures appended and the two tables beside mesh_texture:
    T_NONE: no maps (both tables None); T_ALBEDO: per mesh an f0 texture and a (kd, alpha) texture whose texels are the
    mesh's own fields (b = 9), on MIXED_TEXTURES' shapes; T_FACES: 3n x 1 strips of per-triangle values under both filters
    (b = 9); T_MIXED: random maps on MIXED_TEXTURES' shapes, with RT_TEX_NONE on mesh 0 of mesh_f0 and on mesh 1 of
    mesh_kd_alpha where the scene has three meshes at least."""
    t = dict(tex_ref.texture_set(s, kind, shift))
    tex = list(t["textures"])
    a = s.arrays()
    nm = len(a["tri_begin"]) - 1
    n0 = len(tex)
    t["mesh_f0"] = t["mesh_kd_alpha"] = None
    if kind == T_ALBEDO:
        for m in range(nm):
            (w, h), ws, wt, f = MIXED_TEXTURES[(m + 2) % len(MIXED_TEXTURES)]
            tex.append((np.broadcast_to(a["materials"][m, 5:8].astype(F32), (h, w, 3)).copy(), ws, wt, f))
        for m in range(nm):
            (w, h), ws, wt, f = MIXED_TEXTURES[(m + 4) % len(MIXED_TEXTURES)]
            kda = np.array([a["materials"][m, 0], a["materials"][m, 1], 9.0], F32)
            tex.append((np.broadcast_to(kda, (h, w, 3)).copy(), ws, wt, f))
        t["mesh_f0"] = (n0 + np.arange(nm)).astype(np.uint32)
        t["mesh_kd_alpha"] = (n0 + nm + np.arange(nm)).astype(np.uint32)
    elif kind == T_FACES:
        nt = len(a["tri"])
        _, f0, kd, alpha = face_fields(s)
        kda = np.stack([kd, alpha, np.full(nt, 9.0, F32)], axis=1)
        (_, ws0, wt0, f0filt), (_, ws1, wt1, f1filt) = tex[0], tex[1]
        for vals in (f0, kda):
            texels = np.repeat(vals, 3, axis=0).reshape(1, 3 * nt, 3)
            tex += [(texels, ws0, wt0, f0filt), (texels, ws1, wt1, f1filt)]
        # (a mesh's three maps do not all sit under one filter)
        t["mesh_f0"] = (n0 + (np.arange(nm) + 1) % 2).astype(np.uint32)
        t["mesh_kd_alpha"] = (n0 + 2 + (np.arange(nm) // 2) % 2).astype(np.uint32)
    elif kind == T_MIXED:
        nx = len(MIXED_TEXTURES)
        tex += [(tex_ref.random_texels(w, h, 40 + k), ws, wt, f) for k, ((w, h), ws, wt, f) in enumerate(MIXED_TEXTURES)]
        tex += [(kd_alpha_texels(w, h, 70 + k), ws, wt, f) for k, ((w, h), ws, wt, f) in enumerate(MIXED_TEXTURES)]
        mf = (n0 + (np.arange(nm) + shift + 2) % nx).astype(np.uint32)
        mk = (n0 + nx + (np.arange(nm) + shift + 4) % nx).astype(np.uint32)
        if nm >= 3:  # (the cases' scenes have five meshes; the one- and two-mesh scenes of depth_scenes keep every map)
            mf[0], mk[1] = NONE, NONE
        t["mesh_f0"], t["mesh_kd_alpha"] = mf, mk
    else:
        assert kind == T_NONE
    t["textures"] = tex
    return t


def without(mset, name):
    """The set with one of its two tables None."""
    t = dict(mset)
    t[name] = None
    return t


def per_triangle_scene(s):
    """M2's other side: the split scene with every triangle a mesh of its own, in the same order, whose material holds
    the triangle's four fields."""
    a = s.arrays()
    nt = len(a["tri"])
    albedo, f0, kd, alpha = face_fields(s)
    mats = np.zeros((nt, 8), F32)
    mats[:, 0], mats[:, 1], mats[:, 2:5], mats[:, 5:8] = kd, alpha, albedo, f0
    one = np.arange(nt + 1, dtype=np.uint32)
    return pyrt.ArrayScene(a["pos"], a["nrm"], a["tri"], one, 3 * one, mats, a["lights"], a["camera"])


# A T_MIXED case must differ from the albedo-only textured frame of the same set (tex_ref.frame) in more than this share of
# its rgb words: half the smallest share the reference itself shows over the T_MIXED cases, with all maps, with the f0
# maps alone and with the (kd, alpha) maps alone (tests/test_mat_ref_cpu.py measures and prints every share; the smallest
# are 0.6068 and 0.5413 on the open cubes at 13x9, whose misses change nothing, and 0.2995 for f0 alone on lowres 16x16
# with one ray-mode sample per pixel)
MIN_CHANGED = 0.3034
MIN_CHANGED_F0 = 0.1497
MIN_CHANGED_KDA = 0.2706


# ---- the frames test_gpu_mat.py compares bit for bit, shared with test_mat_ref_cpu.py --------------------------------------
def case_maps(c):
    ck = ("mset", c[0], c[1], c[2], c[6])
    if ck not in _cache:
        t = map_set(case_scene(c), c[6], CASES.index(c))
        for arr in [t["mesh_texture"], t["uv"], t["mesh_f0"], t["mesh_kd_alpha"]] + [x[0] for x in t["textures"]]:
            if arr is not None:
                arr.setflags(write=False)
        _cache[ck] = t
    return _cache[ck]


def set_args(t):
    """Context.set_textures' arguments of a map set."""
    return t["textures"], t["mesh_texture"], t["uv"]


def map_args(t):
    """Context.set_material_maps' arguments of a map set."""
    return t["mesh_f0"], t["mesh_kd_alpha"]


def case_reference(c, brute=False):
    """The reference frame of a case (computed once, shared, never written to)."""
    key = ("ref", case_id(c), brute)
    if key not in _cache:
        ref = frame(case_scene(c), case_params(c), case_maps(c), case_background(c), brute)
        for v in ref.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cache[key] = ref
    return _cache[key]


def case_textured_reference(c):
    """The albedo-only textured frame of a case's set (tex_ref.frame: the maps are not read)."""
    key = ("texref", case_id(c))
    if key not in _cache:
        _cache[key] = tex_ref.frame(case_scene(c), case_params(c), case_maps(c), case_background(c), touched=False)
    return _cache[key]


changed_rgb_words = tex_ref.changed_rgb_words
