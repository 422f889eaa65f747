"""The CPU reference of rt_render_normal_mapped (test infrastructure): a path walked vertex by vertex.

A perturbed shading normal moves the bounce ray, so — unlike every other surface reference here — this one cannot take
its rays from orc.dump_rays of the plain scene.  It walks depth by depth over all samples at once, from the oracle's own
parts: aov_ref.primary_rays for the first rays, orc.trace for every closest and any-hit query, orc.bsdf_rows and
orc.eval_light_rows for the two factors of a term, ao_ref's stream_seed, engine_next, canon_d and hemisphere_sample for the
draws, tex_ref.sample / coord and mat_ref.vertex_sample for the maps, and the sums and the clamp in mat_ref.frame's order.
Newly restated here are three things only: the per-light sample (light_sample_params / light_point of csrc/rt_device.h),
the order of a sample's draws (the jitter's four engine calls; then per shaded vertex the lights' (rh, rv) in light order
and, where a bounce follows, the hemisphere sample), and the operations that form N' (include/rt_amd.h, `bend`).
tests/test_nmap_ref_cpu.py pins the first two to mat_ref.frame and orc.render (no normal maps: the same frame bit for
bit, with both ray counts) and the third to a float64 evaluation."""
import numpy as np

import ao_ref
import aov_ref
import lens_ref
import mat_ref
import orc
import pyrt
import tex_ref
from tex_ref import F32, MIXED_TEXTURES, NONE, T_FACES, T_MIXED, case_background, case_id, case_params, case_scene, clamp01

_cache = {}
CASES = mat_ref.CASES
BILINEAR, REPEAT = tex_ref.BILINEAR, tex_ref.REPEAT


# ---- N' (include/rt_amd.h), float32, every operation rounded on its own ----------------------------------------------------
def _dot(a, b):
    return ((a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]).astype(F32)


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1).astype(F32)


def bend(N, e1, e2, uv0, uv1, uv2, m, parts=False):
    """N' [n][3] of the unit normals N [n][3] for triangles of edges e1, e2 [n][3], vertex uvs uv0..2 [n][2] and the
    normal map's samples m [n][3] (a row of NaN in m stands for RT_TEX_NONE: it keeps N).  parts: also a dict of T, B and
    the five keep conditions (none, flat, r0, tp0, v0, and kept: any of them), with r, Tr (after the flip), Tp, xyz and vv."""
    N, e1, e2, m = (np.asarray(x, F32) for x in (N, e1, e2, m))
    uv0, uv1, uv2 = (np.asarray(x, F32) for x in (uv0, uv1, uv2))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        a1, a2 = uv1[:, 0] - uv0[:, 0], uv2[:, 0] - uv0[:, 0]
        b1, b2 = uv1[:, 1] - uv0[:, 1], uv2[:, 1] - uv0[:, 1]
        r = (a1 * b2 - a2 * b1).astype(F32)
        Tr = (b2[:, None] * e1 - b1[:, None] * e2).astype(F32)
        Br = (a1[:, None] * e2 - a2[:, None] * e1).astype(F32)
        neg = (r < 0)[:, None]
        Tr, Br = np.where(neg, -Tr, Tr), np.where(neg, -Br, Br)
        Tp = (Tr - _dot(N, Tr)[:, None] * N).astype(F32)
        T = aov_ref._unit(Tp)
        B = _cross(N, T)
        B = np.where((_dot(B, Br) < 0)[:, None], -B, B)
        x, y, z = (F32(2) * m[:, k] - F32(1) for k in range(3))
        V = (((x[:, None] * T).astype(F32) + (y[:, None] * B).astype(F32)).astype(F32) + (z[:, None] * N).astype(F32)).astype(F32)
        vv = _dot(V, V)
        keep = dict(none=np.isnan(m).any(axis=1), flat=(x == 0) & (y == 0), r0=~(r != 0), tp0=~(_dot(Tp, Tp) > 0),
                    v0=~((vv > 0) & np.isfinite(vv)))
        kept = keep["none"] | keep["flat"] | keep["r0"] | keep["tp0"] | keep["v0"]
        out = np.where(kept[:, None], N, aov_ref._unit(V)).astype(F32)
    if parts:
        keep.update(T=T, B=B, kept=kept, r=r, Tr=Tr, Tp=Tp, xyz=np.stack([x, y, z], axis=-1).astype(F32), vv=vv)
        return out, keep
    return out


# What frame() counts over its shaded vertices, all depths together (bend_events).  The keep conditions are counted on the
# vertices of meshes that have a normal map, each on its own: a vertex at which two of them hold counts under both, and
# under kept_two.
EVENTS = ("kept_flat", "kept_r0", "kept_tp0", "kept_v0", "kept_v0_inf", "kept_two", "r_neg", "r_subnormal", "tp_subnormal",
          "z_neg_moved")
TINY = np.finfo(F32).tiny


def bend_events(parts, N, N2):
    """name -> bool [n]: the events of EVENTS among the vertices bend(..., parts=True) was given (N, N2: the normals
    before and after).  kept_v0_inf: V's squared length overflowed; r_subnormal, tp_subnormal: r, dot3(Tp, Tp) are
    subnormal and not zero; z_neg_moved: the map's z is negative and N' is not N."""
    has = ~parts["none"]
    with np.errstate(invalid="ignore", over="ignore"):
        tt = _dot(parts["Tp"], parts["Tp"])
        r, vv = parts["r"], parts["vv"]
        conds = [parts[k] & has for k in ("flat", "r0", "tp0", "v0")]
        moved = (np.ascontiguousarray(N2).view(np.uint32) != np.ascontiguousarray(N).view(np.uint32)).any(axis=1)
        return dict(kept_flat=conds[0], kept_r0=conds[1], kept_tp0=conds[2], kept_v0=conds[3],
                    kept_v0_inf=conds[3] & np.isinf(vv), kept_two=np.sum(conds, axis=0) >= 2, r_neg=has & (r < 0),
                    r_subnormal=has & (r != 0) & (np.abs(r) < TINY), tp_subnormal=has & (tt > 0) & (tt < TINY),
                    z_neg_moved=has & (parts["xyz"][:, 2] < 0) & moved)


# ---- the two restated pieces of the integrator -----------------------------------------------------------------------------
def canon_f(state):
    """Rng::canonF: (value float32, end states)."""
    s = ao_ref.engine_next(state)
    r = ((s - np.uint32(1)).astype(F32) / F32(2147483648.0)).astype(F32)
    return np.where(r >= F32(1), F32(0.99999994), r).astype(F32), s


def light_sample(state, light):
    """light_sample of one rt_light (21 floats) from the engine states: (point on the light float32 [n][3], end states).
    uniformF(-side, side) = canonF() * (side - -side) + -side, the horizontal parameter first."""
    light = np.asarray(light, F32)
    pos, vert, hor, side = light[0:3], light[6:9], light[9:12], light[16]
    a, span = F32(-side), F32(side - F32(-side))
    c, state = canon_f(state)
    rh = ((c * span).astype(F32) + a).astype(F32)
    c, state = canon_f(state)
    rv = ((c * span).astype(F32) + a).astype(F32)
    return ((pos + (rv[:, None] * vert).astype(F32)).astype(F32) + (rh[:, None] * hor).astype(F32)).astype(F32), state


def frame(scene, params, mset, bg=None, brute=False):
    """The normal-mapped frame `params` describes: dict(accum [h][w][4], out [h][w][3] or None, closest, shadow, bent — the
    shaded vertices whose normal the maps moved —, kept_r0 — those a degenerate uv triangle kept — and events: EVENTS'
    counts).  mset: a map set of
    mat_ref's form with mesh_normal beside its tables (None: RT_TEX_NONE on every mesh)."""
    a = scene.arrays()
    w, h = params.width, params.height
    ns = params.spp_count if params.spp_count else params.spp
    s0 = params.spp_begin if params.spp_count else 0
    nl = len(a["lights"])
    nm = len(a["tri_begin"]) - 1
    accel = orc.ACCEL_LOOP if brute else orc.ACCEL_OBVH
    nvert = int(params.max_depth) if params.mode == pyrt.MODE_PATH else 1
    assert 1 <= nvert <= 3
    nsmp = w * h * ns
    prim = aov_ref.primary_rays(scene, params).reshape(-1)  # (pixel-major, then the samples of the range in order)
    o, d = prim["origin"].astype(F32).copy(), prim["direction"].astype(F32).copy()
    pix, smp = np.repeat(np.arange(w * h), ns), np.tile(s0 + np.arange(ns), w * h)
    state = ao_ref.stream_seed(params.seed, ao_ref.STREAM_PIXEL, pix, smp)
    for _ in range(4):  # jitter_sample: two double draws
        state = ao_ref.engine_next(state)
    uvs = np.asarray(mset["uv"], F32)
    which_n = mat_ref.table(mset, "mesh_normal", nm)
    mats = a["materials"]
    alive = np.ones(nsmp, bool)
    found = np.zeros(nsmp, bool)
    cols = np.zeros((3, nsmp, 3), F32)
    closest = shadow = bent = kept_r0 = 0
    events = dict.fromkeys(EVENTS, 0)
    for depth in range(nvert):
        idx = np.nonzero(alive)[0]
        if not len(idx):
            break
        rays = np.zeros(len(idx), pyrt.RAY_DTYPE)
        rays["origin"], rays["direction"] = o[idx], d[idx]
        closest += len(idx)
        hits = orc.trace(scene, rays, accel=accel)
        hit = (hits["hit"] != 0) & (hits["d"] > 0)
        alive[idx[~hit]] = False
        idx, vh, vdir = idx[hit], hits[hit], d[idx[hit]]
        nv = len(idx)
        if depth == 0:
            found[idx] = True
        if not nv:
            break
        mesh = vh["mesh"].astype(np.int64)
        gid = a["tri_begin"].astype(np.int64)[mesh] + vh["tri"]
        tv = a["tri"][gid].astype(np.int64)
        u, v = vh["u"], vh["v"]
        wgt = ((F32(1) - u) - v)[:, None]
        p0, p1, p2 = (a["pos"][tv[:, k]] for k in range(3))
        n0, n1, n2 = (a["nrm"][tv[:, k]] for k in range(3))
        nrm = aov_ref._unit((wgt * n0 + u[:, None] * n1) + v[:, None] * n2)
        point = ((wgt * p0 + u[:, None] * p1) + v[:, None] * p2).astype(F32)
        # N': the map's sample at the albedo's hit coordinate; NaN rows stand for RT_TEX_NONE
        m = mat_ref.vertex_sample(mset, which_n, mesh, tv, u, v, np.full((nv, 3), np.nan, F32))
        nrm2, parts = bend(nrm, (p1 - p0).astype(F32), (p2 - p0).astype(F32), uvs[tv[:, 0]], uvs[tv[:, 1]], uvs[tv[:, 2]], m, parts=True)
        bent += int((~parts["kept"]).sum())
        kept_r0 += int((parts["r0"] & ~parts["none"]).sum())
        for name, mask in bend_events(parts, nrm, nrm2).items():
            events[name] += int(mask.sum())
        nrm = nrm2
        kda_own = np.concatenate([mats[mesh, 0:2], np.zeros((nv, 1), F32)], axis=1)
        rows = np.zeros((nv, 17), F32)
        rows[:, 2:5] = tex_ref.vertex_albedo(a, mset, mesh, tv, u, v)
        rows[:, 5:8] = mat_ref.vertex_sample(mset, mat_ref.table(mset, "mesh_f0", nm), mesh, tv, u, v, mats[mesh, 5:8])
        rows[:, 0:2] = mat_ref.vertex_sample(mset, mat_ref.table(mset, "mesh_kd_alpha", nm), mesh, tv, u, v, kda_own)[:, 0:2]
        rows[:, 8:11], rows[:, 14:17] = nrm, -vdir
        color = np.zeros((nv, 3), F32)
        st = state[idx]
        for l in range(nl):  # the light samples in light order, drawn whether the light is occluded or not
            lp, st = light_sample(st, a["lights"][l])
            to_light = (lp - point).astype(F32)
            sr = np.zeros(nv, pyrt.RAY_DTYPE)
            sr["origin"], sr["direction"] = point, to_light
            shadow += nv
            occluded = orc.trace(scene, sr, accel=accel, kind=pyrt.TRACE_ANY)["hit"] != 0
            rows[:, 11:14] = to_light
            bsdf = orc.bsdf_rows(rows, orc.MATH_DET)
            lrow = np.zeros((nv, 24), F32)
            lrow[:, :21], lrow[:, 21:] = a["lights"][l], point
            term = (orc.eval_light_rows(lrow) * bsdf).astype(F32)
            color = np.where(occluded[:, None], color, (color + term).astype(F32))
        cols[depth, idx] = color
        if depth + 1 < nvert:  # the bounce: drawn after the lights, from the normal the vertex shaded with
            bd, st = ao_ref.hemisphere_sample(st, nrm)
            o[idx], d[idx] = point, bd
        state[idx] = st
    # the samples: c0 + (c1 + (c2 + 0)), clamped; then float32 adds in sample order
    total = (cols[0] + (cols[1] + (cols[2] + F32(0)).astype(F32)).astype(F32)).astype(F32)
    total = clamp01(total).reshape(w * h, ns, 3)
    found = found.reshape(w * h, ns)
    acc = np.zeros((w * h, 4), F32)
    for i in range(ns):
        acc[:, :3] = (acc[:, :3] + total[:, i]).astype(F32)
        acc[:, 3] = np.where(found[:, i], acc[:, 3] + F32(1), acc[:, 3])
    acc = acc.reshape(h, w, 4)
    out = None if bg is None else lens_ref.resolve(acc, np.asarray(bg, F32), params.spp)
    return dict(accum=acc, out=out, closest=closest, shadow=shadow, bent=bent, kept_r0=kept_r0, events=events)


# ---- normal-map sets -------------------------------------------------------------------------------------------------------
FLAT = (0.5, 0.5, 1.0)


def normal_texels(w, h, seed):
    """Texels with r, g uniform in [0, 1) and b uniform in [0.5, 1): x, y in [-1, 1), z in [0, 1)."""
    g = np.random.default_rng(seed)
    return np.stack([g.uniform(0.0, 1.0, (h, w)), g.uniform(0.0, 1.0, (h, w)), g.uniform(0.5, 1.0, (h, w))], axis=-1).astype(F32)


def flat_texels(w, h, b=1.0):
    return np.broadcast_to(np.array([0.5, 0.5, b], F32), (h, w, 3)).copy()


def nmap_set(base, s, shift=0):
    """The map set `base` (mat_ref.map_set's form) with normal maps appended and mesh_normal beside the other tables: one
    random map per MIXED_TEXTURES shape (both filters, both wraps) and a flat (0.5, 0.5, 1) one; mesh m takes map
    (m + shift + 1) mod the count, and where the scene has four meshes at least mesh 2 is RT_TEX_NONE and mesh 3 takes the
    flat map (the one- and two-mesh scenes of depth_scenes keep a random map on every mesh)."""
    t = dict(base)
    tex = list(t["textures"])
    nm = len(s.arrays()["tri_begin"]) - 1
    n0, nx = len(tex), len(MIXED_TEXTURES)
    tex += [(normal_texels(w, h, 100 + k), ws, wt, f) for k, ((w, h), ws, wt, f) in enumerate(MIXED_TEXTURES)]
    tex.append((flat_texels(2, 2), REPEAT, REPEAT, BILINEAR))
    mn = (n0 + (np.arange(nm) + shift + 1) % nx).astype(np.uint32)
    if nm >= 4:
        mn[2], mn[3] = NONE, n0 + nx
    t["textures"], t["mesh_normal"] = tex, mn
    return t


def flat_set(base, s, shift=0):
    """N1's second side: nmap_set's shapes, filters and wraps with every texel (0.5, 0.5, b), b differing per map (some
    below 0.5: z < 0), on every mesh."""
    t = dict(base)
    tex = list(t["textures"])
    nm = len(s.arrays()["tri_begin"]) - 1
    n0, nx = len(tex), len(MIXED_TEXTURES)
    tex += [(flat_texels(w, h, (-2.0, 0.0, 0.25, 0.5, 0.75, 1.0, 7.0)[k % 7]), ws, wt, f) for k, ((w, h), ws, wt, f) in enumerate(MIXED_TEXTURES)]
    t["textures"], t["mesh_normal"] = tex, (n0 + (np.arange(nm) + shift) % nx).astype(np.uint32)
    return t


def without_normals(mset):
    t = dict(mset)
    t["mesh_normal"] = None
    return t


def degenerate_triangles(s, mset):
    """How many triangles of meshes with a normal map have uvs that span no area (r == 0 in float32)."""
    a = s.arrays()
    uv = np.asarray(mset["uv"], F32)
    tri = a["tri"].astype(np.int64)
    q0, q1, q2 = uv[tri[:, 0]], uv[tri[:, 1]], uv[tri[:, 2]]
    r = ((q1[:, 0] - q0[:, 0]) * (q2[:, 1] - q0[:, 1]) - (q2[:, 0] - q0[:, 0]) * (q1[:, 1] - q0[:, 1])).astype(F32)
    mesh = np.searchsorted(a["tri_begin"], np.arange(len(tri)), side="right") - 1
    return int(((r == 0) & (mat_ref.table(mset, "mesh_normal", len(a["tri_begin"]) - 1)[mesh] != NONE)).sum())


# A T_MIXED case must differ from the material frame of the same set (mat_ref.frame) in more than this share of its rgb
# words: half the smallest share the reference itself shows over the T_MIXED cases (tests/test_nmap_ref_cpu.py measures
# and prints every share; the smallest is 0.4701, on cubes_open 13x9 [3, 7) path 3, whose misses change nothing)
MIN_CHANGED_N = 0.2350


# ---- the frames test_gpu_nmap.py compares bit for bit, shared with test_nmap_ref_cpu.py ------------------------------------
def case_maps(c):
    ck = ("nset", c[0], c[1], c[2], c[6])
    if ck not in _cache:
        t = nmap_set(mat_ref.case_maps(c), case_scene(c), CASES.index(c))
        for x in t["textures"]:
            x[0].setflags(write=False)
        t["mesh_normal"].setflags(write=False)
        _cache[ck] = t
    return _cache[ck]


set_args, map_args = mat_ref.set_args, mat_ref.map_args


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


def case_material_reference(c):
    """The material frame of a case's set (mat_ref.frame: the normal maps are not read)."""
    key = ("matref", case_id(c))
    if key not in _cache:
        _cache[key] = mat_ref.frame(case_scene(c), case_params(c), case_maps(c), case_background(c))
    return _cache[key]


changed_rgb_words = tex_ref.changed_rgb_words
