"""The probe card (test infrastructure): one small scene whose every mesh puts the sampler, the material maps or the
normal maps of include/rt_amd.h at a limit the header allows and the preset scenes never reach.

The card is a 6 x 4 grid of quads (one mesh of two triangles each, vertices 0..3 counter-clockwise from the lower left,
triangles (0, 1, 2) and (0, 2, 3)) in the plane z = 0, facing a camera whose image plane is that plane: at 48 x 32 pixels a
cell is 8 x 8 pixels and a quad about 7 x 7.  Behind it stand a back wall and below it a floor (meshes 24 and 25, no
textures), so that bounce and shadow rays have something to hit.  Vertex normals are given per quad, not derived from the
geometry.  scene(3) has the three lights of the cubes preset (the pooled body), scene(1) the one light of shading_sweep's
scene 1 (the sequential body).  map_set() is the one set all tests share: per quad an albedo texture and, where the
table says so, an f0, a (kd, alpha) and a normal map — 24 quads name 50-odd textures between them.

quad  probe   uvs                                 what it is there for
  0   S6      (0.05, 0.95)^2                      the ordinary quad every other one can be read against: random 8 x 8 maps
  1   S1      s in [1023, 1024]                   16384-wide maps: |s W| >= 2^23, x = s W - 0.5 loses its half, fx == 0
  2   S1 B5   s in [-1024, -1023]                 the same below zero; vertex normals within 1e-3 of unit3(Tr): Tp is residue
  3   S1      t in [1023, 1024]                   the same on t: 1 x 16384 and 2 x 16384 maps
  4   S1      t in [-1024, -1023]                 the same on t below zero
  5   S1 B7   s == 1024 on all four vertices      |s W| == 2^24, the largest product the set's bounds allow; r == 0 under
                                                  the 1e30 normal map of B2: two keep conditions at once
  6   S1      t == -1024 on all four vertices     |t H| == 2^24 below zero: int(floorf(.)) = -2^24 through i % n
  7   S2      corners (-1024, -1024)..(1024, 1024) 3 x 2 and 7 x 5 maps, REPEAT x CLAMP and CLAMP x REPEAT, both filters:
  8   S2      the same                            neighbouring pixels thousands of periods apart, negative remainders, the
                                                  clamp at both ends; quad 8: REPEAT x REPEAT and CLAMP x CLAMP
  9   S3      s == 3/8 on all four vertices       s W == 3 exactly: the NEAREST boundary, bilinear fx == 0.5 (r == 0)
 10   S3      s == 3.5/8                          s W - 0.5 == 3 exactly: fx == 0
 11   S3      t == 0                              k = 0: y = -0.5, j0 = -1 -> H - 1, j1 = 0, fy == 0.5
 12   S3      t == 1                              k = H: j0 = H - 1, j1 = H -> 0, fy == 0.5
 13   S3      t == -3/8, then s == -2.5/8 (f0 ..) a negative k on either axis (this quad's four uvs are one point of s, t)
 14   S4 B4   s in (-0.05, 0.05), t in (0.95, 1.05)  x in (-1, 0): i0 = -1 -> W - 1, i1 = 0; y in (H - 1, H): j1 = H -> 0; under
                                                  CLAMP i0 == i1 at both ends.  Normal map (NEAREST): x, y in {-7, 7}, z < 0
 15   S5      (-1.3, 2.2)^2                       1 x 1, 1 x 5 and 5 x 1 maps, both filters and wraps: i1 == i0
 16   S5      the same                            the same shapes under the other filter and wrap
 17   M       (0.05, 0.95)^2                      NEAREST: whole regions of alpha = 0 and 1e20, kd = 0, 1.5, -0.25; f0 = 0, 1,
                                                  2.5, -1; albedo 0, 1e30, -3, 3e38
 18   M       the same                            BILINEAR: the same texels blended
 19   B1      a quad in the plane x = -2.5        edge p1 - p0 along z, uv1.t == uv0.t, normals (0, 0, 1): Tr is parallel to
                                                  N and Tp is exactly 0
 20   B1 B7   a quad in the plane x = 2.5         the same under the flat texel: two keep conditions at once
 21   B2      (0.05, 0.95)^2                      normal texels (1e30, 0.5, 0.5): dot3(V, V) overflows; (0.5 + 2^-24, 0.5, 0.5):
                                                  the smallest x a texel encodes
 22   B3      triangle (0, 2, 3) mirrored         r > 0 on one triangle of the quad, r < 0 on the other
 23   B6      (0, 1e-22)^2                        r and dot3(Tp, Tp) are subnormal and not zero

(|uv| <= 1024 is the set's own bound, and barycentrics keep s inside the triangle's: |s W| cannot exceed 1024 * 16384 =
2^24.  The header's "|s W| < 2^27" is the bound for u and v anywhere in [0, 1].)"""
import numpy as np

import aov_ref
import mat_ref
import nmap_ref
import orc
import pyrt
import tex_ref
from tex_ref import BILINEAR, CLAMP, F32, NEAREST, NONE, REPEAT

W, H = 48, 32
COLS, ROWS = 6, 4
N_QUADS = COLS * ROWS
WALL, FLOOR = N_QUADS, N_QUADS + 1
HALF = 0.45  # a quad's half side, in cells
_cache = {}


def rect(s0, s1, t0, t1):
    """The uvs of a quad's four vertices over the rectangle [s0, s1] x [t0, t1]."""
    return [(s0, t0), (s1, t0), (s1, t1), (s0, t1)]


# ---- the textures ------------------------------------------------------------------------------------------------------
def _extreme(vals, w, h):
    """[h][w][3] texels whose texel k is vals[k] (a number: grey; a triple: itself), row-major."""
    t = np.zeros((h * w, 3), F32)
    for k, v in enumerate(vals):
        t[k] = v
    return t.reshape(h, w, 3)


def _textures():
    """name -> (texels, wrap_s, wrap_t, filter)."""
    rnd, kda, nrm = tex_ref.random_texels, mat_ref.kd_alpha_texels, nmap_ref.normal_texels
    R, Cl, N, B = REPEAT, CLAMP, NEAREST, BILINEAR
    t = {}
    # S6, S3, S4: 8 x 8 (k / 8 is exact)
    t["rand8"] = (rnd(8, 8, 201), R, R, B)
    t["rand8_nearest"] = (rnd(8, 8, 201), R, R, N)
    t["rand8_clamp"] = (rnd(8, 8, 202), Cl, Cl, B)
    t["rand5x3"] = (rnd(5, 3, 203), R, Cl, B)
    t["kda4"] = (kda(4, 4, 204), R, R, B)
    t["kda8_clamp_nearest"] = (kda(8, 8, 205), Cl, Cl, N)
    t["nrm8"] = (nrm(8, 8, 206), R, R, B)
    t["nrm8_clamp"] = (nrm(8, 8, 207), Cl, Cl, B)
    # S1: the widest and the tallest maps
    t["wide"] = (rnd(16384, 1, 210), R, R, B)
    t["wide2"] = (rnd(16384, 2, 211), R, R, B)
    t["tall"] = (rnd(1, 16384, 212), R, R, B)
    t["tall2"] = (rnd(2, 16384, 213), R, R, B)
    t["wide_kda"] = (kda(16384, 1, 214), R, R, B)
    t["tall_kda"] = (kda(1, 16384, 215), R, R, N)
    t["wide_nrm"] = (nrm(16384, 1, 216), R, R, B)
    t["tall_nrm"] = (nrm(1, 16384, 217), R, R, B)
    t["wide_nearest"] = (rnd(16384, 1, 218), R, R, N)
    # S2: small odd maps, every wrap pair, both filters
    s2 = [((3, 2), R, Cl, N, rnd), ((3, 2), Cl, R, B, rnd), ((7, 5), R, Cl, B, kda), ((7, 5), Cl, R, N, nrm),
          ((3, 2), R, R, B, rnd), ((3, 2), Cl, Cl, N, rnd), ((7, 5), Cl, Cl, B, kda), ((7, 5), R, R, N, nrm)]
    for k, ((w, h), ws, wt, f, make) in enumerate(s2):
        t["s2_%d" % k] = (make(w, h, 220 + k), ws, wt, f)
    # S5: one texel on an axis
    s5 = [("one", (1, 1), R, R, B, rnd), ("c1x5", (1, 5), Cl, Cl, B, rnd), ("k5x1", (5, 1), R, Cl, N, kda), ("n1x5", (1, 5), R, R, N, nrm),
          ("a5x1", (5, 1), Cl, R, B, rnd), ("one_nearest", (1, 1), Cl, Cl, N, rnd), ("k1x5", (1, 5), R, R, B, kda), ("n5x1", (5, 1), Cl, Cl, B, nrm)]
    for k, (name, (w, h), ws, wt, f, make) in enumerate(s5):
        t[name] = (make(w, h, 240 + k), ws, wt, f)
    # M: values the header allows and no other set holds.  (kd, alpha, b): b is never read
    # (alpha = 1e20: alpha * alpha overflows and the specular term is inf / inf; albedo 3e38 under kd = 1.5: the diffuse
    # term times a radiance above 2.4 overflows — the two ways these frames reach a sum that is not finite)
    mk = _extreme([(0.0, 0.3, 9.0), (1.5, 0.5, 9.0), (-0.25, 0.2, 9.0), (0.5, 0.0, 9.0), (0.5, 1e20, 9.0), (1.5, 0.6, 9.0)], 3, 2)
    mf = _extreme([0.0, 1.0, 2.5, -1.0], 2, 2)
    ma = _extreme([0.0, 1e30, -3.0, 3e38], 4, 1)
    for name, texels in (("m_kda", mk), ("m_f0", mf), ("m_alb", ma)):
        t[name + "_nearest"], t[name + "_bilinear"] = (texels, R, R, N), (texels, Cl, Cl, B)
    # B2, B4, B7
    t["b2"] = (_extreme([(1e30, 0.5, 0.5), (0.5 + 2.0 ** -24, 0.5, 0.5)], 2, 1), R, R, N)
    t["b4"] = (_extreme([(-3.0, 4.0, 0.25), (4.0, -3.0, 0.0), (4.0, 4.0, 0.125), (-3.0, -3.0, 0.375)], 2, 2), R, R, N)
    t["flat"] = (nmap_ref.flat_texels(2, 2), R, R, B)
    return t


# quad -> (probe, uvs, albedo, f0, (kd, alpha), normal map); None: RT_TEX_NONE
_UNIT = rect(0.05, 0.95, 0.05, 0.95)
_S2 = rect(-1024.0, 1024.0, -1024.0, 1024.0)
_S5 = rect(-1.3, 2.2, -1.3, 2.2)
QUADS = [
    ("S6", _UNIT, "rand8", "rand5x3", "kda4", "nrm8"),
    ("S1", rect(1023.0, 1024.0, 0.1, 0.9), "wide", "wide2", "wide_kda", "wide_nrm"),
    ("S1 B5", rect(-1024.0, -1023.0, 0.1, 0.9), "wide", "wide_nearest", None, "wide_nrm"),
    ("S1", rect(0.1, 0.9, 1023.0, 1024.0), "tall", "tall2", "tall_kda", "tall_nrm"),
    ("S1", rect(0.1, 0.9, -1024.0, -1023.0), "tall", "tall2", None, "tall_nrm"),
    ("S1 B7", rect(1024.0, 1024.0, 0.0, 1.0), "wide", "wide2", None, "b2"),
    ("S1", rect(0.0, 1.0, -1024.0, -1024.0), "tall", "tall2", "tall_kda", None),
    ("S2", _S2, "s2_0", "s2_1", "s2_2", "s2_3"),
    ("S2", _S2, "s2_4", "s2_5", "s2_6", "s2_7"),
    ("S3", rect(0.375, 0.375, 0.0, 1.0), "rand8", "rand8_nearest", "kda8_clamp_nearest", "nrm8"),
    ("S3", rect(0.4375, 0.4375, 0.0, 1.0), "rand8", "rand8_clamp", None, "nrm8"),
    ("S3", rect(0.0, 1.0, 0.0, 0.0), "rand8", "rand8_nearest", None, "nrm8_clamp"),
    ("S3", rect(0.0, 1.0, 1.0, 1.0), "rand8", "rand8_clamp", "kda8_clamp_nearest", None),
    ("S3", rect(-0.3125, -0.3125, -0.375, -0.375), "rand8", "rand8_nearest", "kda8_clamp_nearest", "nrm8"),
    ("S4 B4", rect(-0.05, 0.05, 0.95, 1.05), "rand8", "rand8_clamp", "kda4", "b4"),
    ("S5", _S5, "one", "c1x5", "k5x1", "n1x5"),
    ("S5", _S5, "a5x1", "one_nearest", "k1x5", "n5x1"),
    ("M", _UNIT, "m_alb_nearest", "m_f0_nearest", "m_kda_nearest", None),
    ("M", _UNIT, "m_alb_bilinear", "m_f0_bilinear", "m_kda_bilinear", None),
    ("B1", rect(0.1, 0.9, 0.1, 0.9), "rand8", None, None, "nrm8"),
    ("B1 B7", rect(0.1, 0.9, 0.1, 0.9), "rand8_clamp", None, None, "flat"),
    ("B2", _UNIT, "rand8", None, None, "b2"),
    ("B3", [(0.1, 0.1), (0.9, 0.1), (0.9, 0.9), (0.9, 0.5)], "rand8", None, None, "nrm8"),
    ("B6", rect(0.0, 1e-22, 0.0, 1e-22), "rand8", None, None, "nrm8"),
]
assert len(QUADS) == N_QUADS
B1_QUADS = {19: -2.5, 20: 2.5}  # quad -> the plane x = const it stands in
B5_QUAD, B6_QUAD = 2, 23


def probe_name(mesh):
    """What a failure says of a mesh: "quad 14 (S4 B4)", the wall, the floor."""
    mesh = int(mesh)
    return "quad %d (%s)" % (mesh, QUADS[mesh][0]) if mesh < N_QUADS else "the wall" if mesh == WALL else "the floor"


# ---- the scene ---------------------------------------------------------------------------------------------------------
def _geometry():
    """(pos, nrm) [4 * 26][3]."""
    pos, nrm = [], []
    for q in range(N_QUADS):
        cx, cy = -2.5 + (q % COLS), 1.5 - (q // COLS)
        x0, x1, y0, y1 = cx - HALF, cx + HALF, cy - HALF, cy + HALF
        if q in B1_QUADS:  # p1 - p0 along z; seen from the side by the camera's perspective
            x = B1_QUADS[q]
            pos += [(x, y0, -1.0), (x, y0, 0.9), (x, y1, 0.9), (x, y1, -1.0)]
        else:
            pos += [(x0, y0, 0.0), (x1, y0, 0.0), (x1, y1, 0.0), (x0, y1, 0.0)]
        if q == B5_QUAD:  # Tr is along +x on both triangles: normals a hair off it, another hair per vertex
            nrm += [(1.0, 6e-4, 2e-4), (1.0, -5e-4, 4e-4), (1.0, 3e-4, -7e-4), (1.0, -2e-4, -3e-4)]
        else:
            nrm += [(0.0, 0.0, 1.0)] * 4
    pos += [(-4.0, -2.4, -1.2), (4.0, -2.4, -1.2), (4.0, 3.0, -1.2), (-4.0, 3.0, -1.2)]  # the wall
    nrm += [(0.0, 0.0, 1.0)] * 4
    pos += [(-4.0, -2.3, 5.5), (4.0, -2.3, 5.5), (4.0, -2.3, -1.2), (-4.0, -2.3, -1.2)]  # the floor
    nrm += [(0.0, 1.0, 0.0)] * 4
    pos, nrm = np.array(pos, F32), np.array(nrm, np.float64)
    nrm = (nrm / np.linalg.norm(nrm, axis=1)[:, None]).astype(F32)
    return pos, nrm


def scene(n_lights=3):
    """The card under three lights (the cubes preset's) or one (shading_sweep's scene 1); shared, never written to."""
    key = ("scene", n_lights)
    if key not in _cache:
        assert n_lights in (1, 3)
        import shading_sweep
        pos, nrm = _geometry()
        nm = N_QUADS + 2
        tri = np.concatenate([np.array([(0, 1, 2), (0, 2, 3)], np.uint32) + 4 * m for m in range(nm)]).astype(np.uint32)
        begin = np.arange(nm + 1, dtype=np.uint32)
        g = np.random.default_rng(300)
        mats = np.zeros((nm, 8), F32)  # (kd, alpha, albedo, f0): every mesh its own
        mats[:, 0], mats[:, 1] = g.uniform(0.3, 0.8, nm), g.uniform(0.2, 0.8, nm)
        mats[:, 2:5], mats[:, 5:8] = g.uniform(0.3, 0.95, (nm, 3)), g.uniform(0.2, 0.9, (nm, 3))
        lights = (pyrt.Scene("cubes", W, H).arrays()["lights"] if n_lights == 3
                  else shading_sweep.build_scene("cubes", W, H, 1).arrays()["lights"])
        assert len(lights) == n_lights
        camera = np.array([(0.0, 0.0, 5.0), (-3.0, -2.0, 0.0), (6.0, 0.0, 0.0), (0.0, 4.0, 0.0)], F32)
        s = pyrt.ArrayScene(pos, nrm, tri, 2 * begin, 4 * begin, mats, lights.copy(), camera)
        for arr in s.arrays().values():
            arr.setflags(write=False)
        _cache[key] = s
    return _cache[key]


def map_set():
    """The card's set in nmap_ref's form: dict(textures, mesh_texture, mesh_f0, mesh_kd_alpha, mesh_normal, uv, names —
    the textures' names in index order); shared, never written to."""
    if "set" not in _cache:
        tex = _textures()
        names = list(tex)
        index = {n: k for k, n in enumerate(names)}
        nm = N_QUADS + 2
        tables = [np.full(nm, NONE, np.uint32) for _ in range(4)]
        uv = np.zeros((4 * nm, 2), F32)
        for q, (_, uvs, *maps) in enumerate(QUADS):
            uv[4 * q:4 * q + 4] = np.array(uvs, F32)
            for table, name in zip(tables, maps):
                if name is not None:
                    table[q] = index[name]
        uv[4 * N_QUADS:] = np.array(rect(0.0, 1.0, 0.0, 1.0) * 2, F32)
        t = dict(textures=[tex[n] for n in names], mesh_texture=tables[0], mesh_f0=tables[1], mesh_kd_alpha=tables[2],
                 mesh_normal=tables[3], uv=uv, names=names)
        assert set(np.concatenate(tables).tolist()) - {int(NONE)} == set(range(len(names))), "a texture no quad names"
        for arr in tables + [uv] + [x[0] for x in t["textures"]]:
            arr.setflags(write=False)
        _cache["set"] = t
    return _cache["set"]


TABLES = ("mesh_texture", "mesh_f0", "mesh_kd_alpha", "mesh_normal")


def albedo_set(table):
    """The card's set with mesh_texture replaced by another of its tables: every map texture read as an albedo, which is
    what rt_render_aov_textured's albedo channel shows."""
    t = dict(map_set())
    t["mesh_texture"] = t[table]
    return t


def params(spp=4, depth=3, **kw):
    args = dict(mode=pyrt.MODE_PATH, max_depth=depth, seed=tex_ref.SEED)
    args.update(kw)
    return pyrt.make_params(W, H, spp, **args)


def one_sample(**kw):
    """The first sample alone: spp_count 1."""
    return params(4, 1, spp_begin=0, spp_count=1, **kw)


# ---- first hits --------------------------------------------------------------------------------------------------------
def first_hits(s, p):
    """The first hits of the frame p of scene s, from the oracle's own primary rays and trace: dict(hit [n] bool, mesh, tv
    [n][3] vertex ids, u, v — of the hits only —, index: the hits' places among the n = w h samples (pixel-major))."""
    key = ("hits", id(s), p.spp, p.spp_begin, p.spp_count, p.seed)
    if key not in _cache:
        a = s.arrays()
        prim = aov_ref.primary_rays(s, p).reshape(-1)
        hits = orc.trace(s, prim, accel=orc.ACCEL_OBVH)
        hit = (hits["hit"] != 0) & (hits["d"] > 0)
        vh = hits[hit]
        mesh = vh["mesh"].astype(np.int64)
        tv = a["tri"][a["tri_begin"].astype(np.int64)[mesh] + vh["tri"]].astype(np.int64)
        _cache[key] = dict(hit=hit, mesh=mesh, tv=tv, u=vh["u"].astype(F32), v=vh["v"].astype(F32), index=np.nonzero(hit)[0],
                           scene=s)  # (the scene is kept alive: the key holds its id)
    return _cache[key]


def first_hit_mesh(s, p):
    """[h][w][samples] int64: the mesh of every sample's first hit, -1 for a miss."""
    fh = first_hits(s, p)
    out = np.full(len(fh["hit"]), -1, np.int64)
    out[fh["index"]] = fh["mesh"]
    return out.reshape(p.height, p.width, -1)


def table_samples(mset, table, fh):
    """Per texture k that `table` gives a first hit: k -> (rows into fh's hits, s, t [n] float32, the sample [n][3], its
    parts)."""
    uv = np.asarray(mset["uv"], F32)
    which = np.asarray(mset[table], np.uint32)[fh["mesh"]]
    out = {}
    for k, tex in enumerate(mset["textures"]):
        rows = np.nonzero(which == k)[0]
        if len(rows):
            q, u, v = fh["tv"][rows], fh["u"][rows], fh["v"][rows]
            s = tex_ref.coord(uv[q[:, 0], 0], uv[q[:, 1], 0], uv[q[:, 2], 0], u, v)
            t = tex_ref.coord(uv[q[:, 0], 1], uv[q[:, 1], 1], uv[q[:, 2], 1], u, v)
            c, parts = tex_ref.sample(tex, s, t, parts=True)
            out[k] = (rows, s, t, c, parts)
    return out


SAMPLER_EVENTS = ("repeat_below", "repeat_above", "clamp_low", "clamp_high", "seam", "f_zero", "f_half", "big", "same")


def sampler_events(mset, fh):
    """(counts, largest): counts[axis][event] over the first hits fh and all four tables of the set, axis "s" or "t";
    largest[axis] = max |s W| or |t H|.  The events: the integer coordinate before the wrap is below 0 / at or above N
    under REPEAT; the clamp moved an index at the low / the high end; seam: a bilinear pair (N - 1, 0) under REPEAT;
    f_zero, f_half: the bilinear weight is exactly 0 / 0.5; big: |s W| >= 2^24; same: a bilinear pair of one texel."""
    counts = {ax: dict.fromkeys(SAMPLER_EVENTS, 0) for ax in "st"}
    largest = dict(s=0.0, t=0.0)
    for table in TABLES:
        for k, (rows, s, t, c, parts) in table_samples(mset, table, fh).items():
            texels, ws, wt, filt = mset["textures"][k]
            bil = parts["bilinear"]
            for ax, n, mode, prod, lo, i0, i1, f in (("s", texels.shape[1], ws, parts["sw"], parts["xi"], parts["i0"], parts["i1"], parts["fx"]),
                                                       ("t", texels.shape[0], wt, parts["th"], parts["yj"], parts["j0"], parts["j1"], parts["fy"])):
                hi = lo + 1 if bil else lo  # the larger integer coordinate before the wrap
                ev = counts[ax]
                if mode == REPEAT:
                    ev["repeat_below"] += int((lo < 0).sum())
                    ev["repeat_above"] += int((hi >= n).sum())
                    if bil and n > 1:
                        ev["seam"] += int(((i0 == n - 1) & (i1 == 0)).sum())
                else:
                    ev["clamp_low"] += int((lo < 0).sum())
                    ev["clamp_high"] += int((hi > n - 1).sum())
                if bil:
                    ev["f_zero"] += int((f == 0).sum())
                    ev["f_half"] += int((f == F32(0.5)).sum())
                    ev["same"] += int((i0 == i1).sum())
                ev["big"] += int((np.abs(prod) >= F32(2.0 ** 24)).sum())
                largest[ax] = max(largest[ax], float(np.abs(prod).max()))
    return counts, largest


def sample64(tex, s, t):
    """The header's sampler in float64 on the float32 coordinates s, t: (the sample [n][3] float64, i0, i1, j0, j1)."""
    texels, ws, wt, filt = tex
    tx = np.asarray(texels, np.float64)
    h, w = tx.shape[:2]
    s, t = np.asarray(s, np.float64), np.asarray(t, np.float64)
    if filt == NEAREST:
        i, j = tex_ref.wrap(np.floor(s * w), w, ws), tex_ref.wrap(np.floor(t * h), h, wt)
        return tx[j, i], i, i, j, j
    x, y = s * w - 0.5, t * h - 0.5
    xf, yf = np.floor(x), np.floor(y)
    fx, fy = (x - xf)[:, None], (y - yf)[:, None]
    i0, i1 = tex_ref.wrap(xf, w, ws), tex_ref.wrap(xf + 1, w, ws)
    j0, j1 = tex_ref.wrap(yf, h, wt), tex_ref.wrap(yf + 1, h, wt)
    a = tx[j0, i0] + fx * (tx[j0, i1] - tx[j0, i0])
    b = tx[j1, i0] + fx * (tx[j1, i1] - tx[j1, i0])
    return a + fy * (b - a), i0, i1, j0, j1


# ---- a two-bone skin over the card (N2 under rt_update_skin) -----------------------------------------------------------
def skin():
    """(bone, weight, bones): every quad vertex hangs on bones 0 and 1 with weights (1 - w, w), w = 0.15 + 0.7 f, f its
    way across the card in x; the wall and the floor on none.  The bones turn about y by 4 and -6 degrees and shift."""
    import skin_ref
    pos = scene(3).arrays()["pos"]
    nv = len(pos)
    bone, weight = np.zeros((nv, skin_ref.SLOTS), np.uint16), np.zeros((nv, skin_ref.SLOTS), F32)
    rows = np.arange(4 * N_QUADS)
    w1 = (0.15 + 0.7 * (pos[rows, 0].astype(np.float64) + 3.0) / 6.0).astype(F32)
    bone[rows, 1] = 1
    weight[rows, 0], weight[rows, 1] = F32(1) - w1, w1
    bones = skin_ref.rotation_records([4.0, -6.0], translate=[(0.02, 0.01, -0.03), (-0.01, 0.03, 0.02)])
    return bone, weight, bones
