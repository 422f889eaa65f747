"""Scenes and ray families on which the rule "closest t > 0, then the lowest (mesh, triangle)" DECIDES the hit (tests of the
four restatements of RayTracer.h:27-53 in rt_kernels.hip — Trav::test_pair, Trav::test_record, the pool's publish /
refresh_best key and brute — and of k_ao's bounded walker, the slab test's `tnear <= best` and safe_inv): coincident
sheets in several meshes, a wall met edge-on, a fan around one vertex, trees that are one leaf; rays that are axis-parallel,
start in box planes, lie in the plane of the triangles, start on them, and straddle Ray.cpp's absolute |det| threshold.

Every vertex is on the 1/16 lattice with |coordinate| <= 4 and every triangle's doubled area is a power of two, so for a
ray whose origin is on the lattice and whose direction's component across the triangle is a power of two, every float32
operation of Ray.cpp:9-24 is exact.  exact_hits restates the rule in integers, independently of the oracle.
numpy only; materials and lights are the `cubes` preset's, each mesh with a material of its own.

The scenes: `stack` — four coincident copies of an 8 x 8-cell sheet at z = -2 in four meshes, a fifth sheet at z = -2.5, a
wall standing on the front sheets; `stack_shuffled` — the same surfaces with the meshes in reverse order and the triangles
of each permuted, the copy that wins the ties cut into 1/2 x 1/8 cells (equal areas, other boxes: the builders put
triangles of equal boxes in id order, which would hand every walker the winner first); `fan` — eight triangles around one
vertex in three meshes, a coincident copy in a fourth, the back sheet; `tiny1` / `tiny2` / `tiny3` — one triangle, two
coincident in two meshes, three coincident in one (the tree is one leaf or one pair)."""
import numpy as np

import pyrt

F32 = np.float32
L = 16  # lattice units per 1.0
SCENES = ("stack", "stack_shuffled", "fan", "tiny1", "tiny2", "tiny3")
FRAME = (24, 16)  # the small frame of the CPU tests (the GPU tests size theirs)
K_AXIAL = (-40, -17, -16, -15, -14, 0, 7, 60)
EPS = float(F32(0.000001))  # Ray.cpp's EPSILON as the float32 it is compared as
FRONT_Z, BACK_Z = -2 * L, -2 * L - L // 2
# lattice coordinates (x or y, in 1/16) of origins and targets: vertices (multiples of 4), cell edges, diagonals (fractions
# that sum to 4), interiors, the border (+-16) and past it
COORDS = np.array([-17, -16, -15, -12, -10, -8, -5, -3, -2, 0, 1, 3, 4, 8, 13, 16])
_cache = {}


# ---- geometry (integer lattice coordinates) ------------------------------------------------------------------------------
def _sheet(z, nx=8, ny=8, cx=4, cy=4, x0=-16, y0=-16):
    """nx x ny cells of cx x cy, two triangles each, in the plane z: (vertices [(nx+1)(ny+1)][3], triangles [2 nx ny][3])."""
    x, y = np.meshgrid(np.arange(nx + 1) * cx + x0, np.arange(ny + 1) * cy + y0, indexing="xy")
    pos = np.stack([x.reshape(-1), y.reshape(-1), np.full(x.size, z)], 1)
    i, j = np.meshgrid(np.arange(nx), np.arange(ny), indexing="xy")
    p00 = (j * (nx + 1) + i).reshape(-1)
    p10, p01, p11 = p00 + 1, p00 + nx + 1, p00 + nx + 2
    tri = np.stack([np.stack([p00, p10, p01], 1), np.stack([p11, p01, p10], 1)], 1).reshape(-1, 3)
    return pos, tri


def _wall():
    """2 x 2 cells of 1/2 in the plane x = 1/2, y in [-1/2, 1/2], z in [-2, -1]: it stands on the front sheets."""
    g = np.arange(3) * 8
    y, z = np.meshgrid(g - 8, g + FRONT_Z, indexing="xy")
    pos = np.stack([np.full(y.size, 8), y.reshape(-1), z.reshape(-1)], 1)
    i, j = np.meshgrid(np.arange(2), np.arange(2), indexing="xy")
    p00 = (j * 3 + i).reshape(-1)
    p10, p01, p11 = p00 + 1, p00 + 3, p00 + 4
    tri = np.stack([np.stack([p00, p10, p01], 1), np.stack([p11, p01, p10], 1)], 1).reshape(-1, 3)
    return pos, tri


def _fan():
    """Eight triangles around (0, 0, -2), the ring the eight lattice neighbours at distance 1/2 (doubled areas 1/4)."""
    ring = [(8, 0), (8, 8), (0, 8), (-8, 8), (-8, 0), (-8, -8), (0, -8), (8, -8)]
    pos = np.array([(0, 0, FRONT_Z)] + [(x, y, FRONT_Z) for x, y in ring])
    tri = np.array([(0, 1 + k, 1 + (k + 1) % 8) for k in range(8)])
    return pos, tri


def _meshes(name):
    """[(vertices, triangles, normal)] of a scene, in mesh order."""
    up, side = (0, 0, 1), (-1, 0, 0)
    if name in ("stack", "stack_shuffled", "stack_apart"):
        # stack_apart: the four copies 1/16 apart (what test_gpu_ties' refit moves into coincidence)
        zs = [FRONT_Z - k if name == "stack_apart" else FRONT_Z for k in range(4)]
        # stack_shuffled: the copy that wins the ties among the four (the last here, the first after the reversal) is the
        # same sheet from 4 x 16 cells of 1/2 x 1/8: triangles of the same area (the same determinants) in other boxes.
        # The builders order triangles of equal boxes by id, so among exact copies the winner is always met first
        m = [(_sheet(z, 4, 16, 8, 2) if name == "stack_shuffled" and k == 3 else _sheet(z)) + (up,) for k, z in enumerate(zs)]
        m += [_sheet(BACK_Z) + (up,), _wall() + (side,)]
        if name == "stack_shuffled":
            rng = np.random.default_rng(5)
            m = [(p, t[rng.permutation(len(t))], n) for p, t, n in m][::-1]
        return m
    if name == "fan":
        p, t = _fan()
        return [(p, t[0:3], up), (p, t[3:6], up), (p, t[6:8], up), (p, t, up), _sheet(BACK_Z) + (up,)]
    one = (np.array([(-16, -16, FRONT_Z), (16, -16, FRONT_Z), (-16, 16, FRONT_Z)]), np.array([(0, 1, 2)]))
    if name == "tiny1":
        return [one + (up,)]
    if name == "tiny2":
        return [one + (up,), one + (up,)]
    if name == "tiny3":
        return [(one[0], np.repeat(one[1], 3, axis=0), up)]
    raise ValueError(name)


# the window of the plane z = -2 each scene's camera sees: (camera position, window centre, half width, half height)
_VIEWS = {"stack": ((0, 0, 1), (0, 0), 1.25, 1.0), "fan": ((0, 0, 0), (0, 0), 0.625, 0.5),
          "tiny": ((-0.5, -0.5, 0), (-0.5, -0.5), 0.5, 0.375)}


def camera(name="stack"):
    """Faces the plane z = -2 squarely from a dyadic position: the frame is a window of that plane of which the front
    triangles fill 80 % (the stacks, the fan) or all (the tiny scenes: the window lies inside the triangle).  [4][3]:
    position, lower-left corner, horizontal, vertical."""
    pos, (cx, cy), hw, hh = _VIEWS["stack" if name.startswith("stack") else "tiny" if name.startswith("tiny") else name]
    return np.array([pos, (cx - hw, cy - hh, FRONT_Z / L), (2 * hw, 0, 0), (0, 2 * hh, 0)], F32)


def arrays(name, flip_normals=False):
    """The dict pyrt.ArrayScene takes apart.  Mesh i has material i of the preset's five, its albedo scaled by 3/4 per
    round through them: no two meshes share one, so the winner of a tie shows in colour."""
    base = pyrt.Scene("cubes", 16, 16).arrays()
    meshes = _meshes(name)
    pos, nrm, tri, tb, vb = [], [], [], [0], [0]
    for p, t, n in meshes:
        assert np.abs(p).max() <= 4 * L
        tri.append(t + vb[-1])
        pos.append(p.astype(F32) / F32(L))
        nrm.append(np.tile(np.array(n, F32) * F32(-1 if flip_normals else 1), (len(p), 1)))
        tb.append(tb[-1] + len(t))
        vb.append(vb[-1] + len(p))
    nm = len(meshes)
    assert len(base["materials"]) >= 5
    mats = base["materials"][np.arange(nm) % 5].copy()
    mats[:, 2:5] *= (F32(0.75) ** (np.arange(nm) // 5).astype(F32))[:, None]
    assert len(np.unique(mats, axis=0)) == nm
    return dict(pos=np.concatenate(pos), nrm=np.concatenate(nrm), tri=np.concatenate(tri).astype(np.uint32),
                tri_begin=np.array(tb, np.uint32), vtx_begin=np.array(vb, np.uint32), materials=mats,
                lights=base["lights"].copy(), camera=camera(name))


def array_scene(a, **kw):
    d = dict(a, **kw)
    return pyrt.ArrayScene(d["pos"], d["nrm"], d["tri"], d["tri_begin"], d["vtx_begin"], d["materials"], d["lights"], d["camera"])


def scene(name, flip_normals=False):
    """The scene (built once, shared, never written to)."""
    key = ("scene", name, flip_normals)
    if key not in _cache:
        _cache[key] = array_scene(arrays(name, flip_normals))
    return _cache[key]


def front_meshes(name):
    """The meshes whose triangles lie in z = -2 and coincide with another triangle there."""
    return {"stack": (0, 1, 2, 3), "stack_shuffled": (2, 3, 4, 5), "fan": (0, 1, 2, 3), "tiny2": (0, 1), "tiny3": (0,)}.get(name, ())


def min_tie(name):
    """How many triangles are tied at least at every hit of a front mesh."""
    return {"stack": 4, "stack_shuffled": 4, "fan": 2, "tiny2": 2, "tiny3": 3}.get(name, 1)


def origin_bound(a):
    """bvh_build.cpp paddingRule's originBound in float32: 16 x max(1, the largest referenced |coordinate|, the camera's and
    the lights' positions)."""
    reach = max(F32(1), np.abs(a["pos"][a["tri"].reshape(-1)]).max(), np.abs(a["camera"][0]).max(), np.abs(a["lights"][:, :3]).max())
    return F32(16) * F32(reach)


def box_scale(a):
    """bvh_build.cpp paddingRule's boxScale in float32: 32768 / max(maxAbs + pad, 1e-30) = m 2^e with m in [0.5, 1), boxScale =
    2^clamp(e - 1, -100, 100); pad = 6e-5 x the reach of origin_bound."""
    max_abs = F32(np.abs(a["pos"][a["tri"].reshape(-1)]).max())
    pad = F32(6e-5) * (origin_bound(a) / F32(16))
    _, e = np.frexp(F32(32768) / max(F32(max_abs + pad), F32(1e-30)))
    return np.ldexp(F32(1), min(max(int(e) - 1, -100), 100))


# ---- ray families ---------------------------------------------------------------------------------------------------------
class Family:
    """name, rays (RAY_DTYPE), exact (bool [n]: exact_hits covers the ray), k (int [n], axial: the direction is 2^k long)."""

    def __init__(self, name, o, d, exact=None, k=None):
        self.name = name
        self.rays = np.zeros(len(o), pyrt.RAY_DTYPE)
        self.rays["origin"], self.rays["direction"] = np.asarray(o, F32), np.asarray(d, F32)
        assert np.isfinite(self.rays["origin"]).all() and np.isfinite(self.rays["direction"]).all()
        self.exact = np.zeros(len(o), bool) if exact is None else np.asarray(exact, bool)
        self.k = None if k is None else np.asarray(k)
        self.rays.setflags(write=False)

    def __len__(self):
        return len(self.rays)


def _grid():
    x, y = np.meshgrid(COORDS, COORDS, indexing="xy")
    return x.reshape(-1), y.reshape(-1)


DENORMAL = (F32(1e-45), F32(-1e-45), F32(1.1e-38), F32(-3e-42))


def axial():
    """(0, 0, -+1) 2^k from z = -1 downwards and from z = -2.25 (between the sheets) upwards, over the 16 x 16 lattice
    origins, for every k of K_AXIAL.  The two zero components are +0, -0 or — every fourth ray, outside `exact` — denormal."""
    x, y = _grid()
    o, d, ex, ks = [], [], [], []
    for k in K_AXIAL:
        i = np.arange(len(x))
        down = i % 2 == 0
        oz = np.where(down, -L, FRONT_Z - L // 4)
        dz = np.where(down, -1.0, 1.0) * 2.0 ** k
        var = (i // 2) % 4  # the form of the zero components
        dx = np.select([var == 0, var == 1, var == 2], [F32(0), F32(-0.0), DENORMAL[0]], DENORMAL[2]).astype(F32)
        dy = np.select([var == 0, var == 1, var == 2], [F32(-0.0), F32(0), F32(-0.0)], DENORMAL[3]).astype(F32)
        dx[(var == 2) & (i % 3 == 0)] = DENORMAL[1]
        o.append(np.stack([x, y, oz], 1).astype(F32) / F32(L))
        d.append(np.stack([dx, dy, dz.astype(F32)], 1))
        ex.append(var < 2)
        ks.append(np.full(len(x), k))
    return Family("axial", np.concatenate(o), np.concatenate(d), np.concatenate(ex), np.concatenate(ks))


# (dx, dy, dz) in 1/16: dx is 0 or a power of two (the wall's determinant), dz a power of two (the sheets'), dy anything
_SLANTS = [(0, 3, -16), (4, -5, -16), (-8, 16, -32), (16, -23, -8), (-32, 28, -16), (1, 0, -16), (0, 0, 4), (2, 7, 2),
           (-16, -9, 4), (0, -32, -32), (8, 1, -64), (-4, 12, -4)]


def slanted():
    """Lattice origins, each direction the exact difference to a lattice point of the front sheets (a vertex, on an edge, on
    a diagonal, inside a cell, on the border, just outside), some scaled by 2^10 or 2^-10."""
    x, y = _grid()
    o, d = [], []
    for r in range(6):
        i = np.arange(len(x))
        s = np.array(_SLANTS)[(i * 5 + r * 7 + i // 16) % len(_SLANTS)]
        tgt = np.stack([x, y, np.full(len(x), FRONT_Z)], 1)
        scale = np.select([(i + r) % 3 == 1, (i + r) % 3 == 2], [2.0 ** 10, 2.0 ** -10], 1.0)
        o.append((tgt - s).astype(F32) / F32(L))
        d.append((s / L * scale[:, None]).astype(F32))
    return Family("slanted", np.concatenate(o), np.concatenate(d), np.ones(6 * len(x), bool))


def inplane():
    """Origins in the plane z = -2 inside and outside the sheets, directions in that plane along x, y and the diagonals: the
    sheets' determinant is 0 and the wall is met on its bottom edge."""
    c = COORDS[::2]
    c = np.concatenate([c, [-24, 24, 8]])
    x, y = (g.reshape(-1) for g in np.meshgrid(c, c, indexing="xy"))
    dirs = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (1, 1, 0), (-1, 1, 0), (1, -1, 0), (-0.5, -0.5, 0)], F32)
    o = np.repeat(np.stack([x, y, np.full(len(x), FRONT_Z)], 1).astype(F32) / F32(L), len(dirs), axis=0)
    d = np.tile(dirs, (len(x), 1))
    d[np.arange(len(d)) % 5 == 0, 2] = F32(-0.0)
    return Family("inplane", o, d)


def onsurface():
    """Origins ON the front sheets at lattice points, directions +-z: the origin's own triangles are at t = 0 and refused by
    t > 0; downwards the back sheet is hit, upwards nothing."""
    x, y = _grid()
    o = np.tile(np.stack([x, y, np.full(len(x), FRONT_Z)], 1).astype(F32) / F32(L), (2, 1))
    d = np.zeros_like(o)
    d[:len(x), 2], d[len(x):, 2] = -1, 0.5
    return Family("onsurface", o, d, np.ones(len(o), bool))


def bound(a):
    """Origins at, just inside and just outside the origin bound B (and at 4 B), on every axis and both sides, aimed at
    tied lattice points: along z axis-parallel, along x and y in the plane z = -1.5 through the wall.  Inside B the tree
    answers, beyond it the exhaustive loop."""
    B = origin_bound(a)
    steps = [np.nextafter(B, F32(0)), B, np.nextafter(B, F32(np.inf)), F32(4) * B]
    o, d = [], []
    pts = [(0, 0), (4, 4), (-16, 8), (1, 3), (5, -7), (16, 16), (-17, 0), (8, 0)]
    for b in steps:
        for sgn in (1, -1):
            for x, y in pts:
                o.append((x / L, y / L, sgn * b)), d.append((0, 0, -sgn))
                o.append((sgn * b, y / L, -1.5)), d.append((-sgn * 0.25, 0, 0))
                o.append((x / L, sgn * b, -1.5)), d.append((0, -sgn * 2, 0))
                # slanted from afar at the lattice point (x, y, -2): float32 rounds the direction, the oracle decides
                org = np.array((sgn * b, y / L + 3, 7), F32)
                o.append(org), d.append(np.array((x / L, y / L, -2), F32) - org)
    return Family("bound", np.array(o, F32), np.array(d, F32))


def inside_bound(a, rays):
    """The rays the tree answers (k_trace: beyond the bound is `>`)."""
    return np.abs(rays["origin"]).max(axis=1) <= origin_bound(a)


def families(name):
    """The families that need no tree, for a scene (built once, shared)."""
    key = ("families", name)
    if key not in _cache:
        _cache[key] = [axial(), slanted(), inplane(), onsurface(), bound(arrays(name))]
    return _cache[key]


def f16_planes(nodes, box_scale):
    """The binary16 planes the walker tests, as float32 coordinates: each exported float plane times boxScale rounded
    outwards to binary16 (lo down, hi up), divided by boxScale again.  nodes: [n][16] uint32 of Context.bvh_export()."""
    f = np.ascontiguousarray(nodes[:, 0:12]).view(F32).reshape(-1, 2, 2, 3)  # node, slot, lo / hi, axis
    s = f * F32(box_scale)
    h = s.astype(np.float16)
    lo = np.where(h[:, :, 0].astype(F32) > s[:, :, 0], np.nextafter(h[:, :, 0], np.float16(-np.inf)), h[:, :, 0])
    hi = np.where(h[:, :, 1].astype(F32) < s[:, :, 1], np.nextafter(h[:, :, 1], np.float16(np.inf)), h[:, :, 1])
    return np.stack([lo, hi], 2).astype(F32) / F32(box_scale)


def boxplanes(nodes, box_scale, max_nodes=24):
    """From the float boxes of the actual tree (Context.bvh_export) and their binary16 form: for a sample of nodes, both
    slots and each axis, rays whose origin coordinate is exactly a box plane and whose direction component on that axis is
    +-0 (they run inside the plane, across the box); rays along the twelve box edges; rays from the camera through the
    eight corners."""
    n = len(nodes)
    pick = np.unique(np.concatenate([np.arange(min(n, 8)), np.linspace(0, n - 1, min(n, max_nodes)).astype(int)]))
    f = np.ascontiguousarray(nodes[:, 0:12]).view(F32).reshape(-1, 2, 2, 3)
    o, d = [], []
    for boxes in (f[pick], f16_planes(nodes, box_scale)[pick]):
        for box in boxes.reshape(-1, 2, 3):
            if not np.isfinite(box).all() or (box[0] > box[1]).any():
                continue  # (an empty slot)
            mid = ((box[0] + box[1]) * F32(0.5)).astype(F32)
            for a in range(3):
                for side in range(2):
                    for b in ((a + 1) % 3, (a + 2) % 3):
                        org, dr = mid.copy(), np.zeros(3, F32)
                        org[a], org[b] = box[side, a], box[0, b] - F32(1)
                        dr[a], dr[b] = F32(-0.0) if side else F32(0), F32(2)
                        o.append(org), d.append(dr)
                        # ... and along the edge where two planes meet: two zero components, two coordinates in planes
                        c = 3 - a - b
                        org2, dr2 = org.copy(), dr.copy()
                        org2[c], dr2[c] = box[1 - side, c], F32(0) if side else F32(-0.0)
                        o.append(org2), d.append(dr2)
            cam = camera()[0]
            for corner in range(8):
                p = np.array([box[(corner >> a) & 1, a] for a in range(3)], F32)
                o.append(cam), d.append(p - cam)
    return Family("boxplanes", np.array(o, F32), np.array(d, F32))


# ---- the exact reference --------------------------------------------------------------------------------------------------
def _lattice(x, what):
    i = np.rint(np.asarray(x, np.float64) * L).astype(np.int64)
    assert np.array_equal(i / L, np.asarray(x, np.float64)), "%s off the 1/16 lattice" % what
    return i


def _int_directions(d):
    """d = D 2^e with D odd-reduced int64 [n][3] and e int [n] (float32 directions, not all zero, no component more than
    2^20 times another's lowest bit)."""
    d = np.asarray(d, np.float64)
    _, x = np.frexp(d)
    e = np.where(d != 0, x - 24, 10 ** 6).min(axis=1)
    D = np.ldexp(d, -e[:, None]).astype(np.int64)
    assert np.array_equal(np.ldexp(D.astype(np.float64), e[:, None]), d)
    low = D[:, 0] | D[:, 1] | D[:, 2]
    tz = np.zeros(len(D), np.int64)
    for _ in range(64):
        m = (low & 1) == 0
        if not m.any():
            break
        low = np.where(m, low >> 1, low)
        tz += m
    D >>= tz[:, None]
    assert np.abs(D).max() < 1 << 20, "direction components too far apart for the integer reference"
    return D, e + tz


def exact_hits(scene, rays, chunk=256, groups=False):
    """RayTracer.h:27-53 over Ray.cpp:9-24 in integers: |det| >= EPSILON, 0 <= u <= 1, v >= 0, u + v <= 1, t > 0, the closest
    t, then the lowest (mesh, triangle).  The rays' origins are on the lattice and their directions D 2^e with small
    integer D.  Returns a dict of arrays [n]: hit, mesh, tri (within the mesh), tied (triangles at the winning t that pass
    the test), edge (u == 0, v == 0 or u + v == 1 exactly), u, v, t (float64; exact where pow2) and pow2 (the winner's
    |det| is a power of two: every float32 operation of the test was exact).  groups: also `group`, per ray the global ids
    of the tied triangles (ascending; the first is the winner)."""
    a = scene.arrays()
    P = _lattice(a["pos"], "vertex")
    p0, p1, p2 = (P[a["tri"][:, k].astype(np.int64)] for k in range(3))
    e1, e2 = p1 - p0, p2 - p0
    mesh_of = np.searchsorted(a["tri_begin"].astype(np.int64), np.arange(len(e1)), side="right") - 1
    O = _lattice(rays["origin"], "origin")
    D, e = _int_directions(rays["direction"])
    n = len(O)
    out = dict(hit=np.zeros(n, bool), mesh=np.zeros(n, np.uint32), tri=np.zeros(n, np.uint32), tied=np.zeros(n, np.int64),
               edge=np.zeros(n, bool), u=np.zeros(n), v=np.zeros(n), t=np.zeros(n), pow2=np.zeros(n, bool))
    if groups:
        out["group"] = [np.zeros(0, np.int64)] * n
    for b in range(0, n, chunk):
        Dc, Oc, ec = D[b:b + chunk, None, :], O[b:b + chunk, None, :], e[b:b + chunk]
        pvec = np.cross(Dc, e2[None])
        det = (e1[None] * pvec).sum(-1)            # x 2^e / 256
        tv = Oc - p0[None]
        un = (tv * pvec).sum(-1)                   # u = un / det
        q = np.cross(tv, e1[None])
        vn = (Dc * q).sum(-1)                      # v = vn / det
        tn = (e2[None] * q).sum(-1)                # t = tn / (16 det 2^e)
        s, ad = np.sign(det), np.abs(det)
        ok = np.ldexp(ad.astype(np.float64), (ec - 8)[:, None]) >= EPS
        ok &= (un * s >= 0) & (un * s <= ad) & (vn * s >= 0) & ((un + vn) * s <= ad) & (tn * s > 0)
        ts = tn * s
        for r in np.nonzero(ok.any(axis=1))[0]:
            idx = np.nonzero(ok[r])[0]
            num, den = ts[r, idx], ad[r, idx]
            c = int(np.argmin(num / den))
            while True:
                less = num * den[c] < num[c] * den
                if not less.any():
                    break
                c = int(np.nonzero(less)[0][np.argmin((num / den)[less])])
            tie = idx[num * den[c] == num[c] * den]
            w = int(tie.min())  # (global triangle ids ascend in (mesh, triangle) order)
            g = b + r
            if groups:
                out["group"][g] = np.sort(tie)
            out["hit"][g], out["mesh"][g], out["tied"][g] = True, mesh_of[w], len(tie)
            out["tri"][g] = w - int(a["tri_begin"][mesh_of[w]])
            dw = int(det[r, w])
            out["edge"][g] = un[r, w] == 0 or vn[r, w] == 0 or un[r, w] + vn[r, w] == dw
            out["u"][g], out["v"][g] = un[r, w] / dw, vn[r, w] / dw
            out["t"][g] = np.ldexp(tn[r, w] / dw, -int(ec[r]) - 4)
            out["pow2"][g] = abs(dw) & (abs(dw) - 1) == 0
    return out


def exact_pairs(tri_pos, rays):
    """Ray.cpp:9-24 alone, in integers, on ray i against triangle i (tri_pos [n][3][3] on the lattice): dict of det_ok
    (|det| >= EPSILON: u, v and t get written), hit (the function's return value — it does not look at t), u, v, t (float64,
    exact where pow2) and pow2, arrays [n]."""
    P = _lattice(tri_pos, "vertex")
    p0, e1, e2 = P[:, 0], P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]
    O = _lattice(rays["origin"], "origin")
    D, e = _int_directions(rays["direction"])
    pvec = np.cross(D, e2)
    det = (e1 * pvec).sum(-1)
    tv = O - p0
    un = (tv * pvec).sum(-1)
    q = np.cross(tv, e1)
    vn, tn = (D * q).sum(-1), (e2 * q).sum(-1)
    s, ad = np.sign(det), np.abs(det)
    det_ok = np.ldexp(ad.astype(np.float64), e - 8) >= EPS
    hit = det_ok & (un * s >= 0) & (un * s <= ad) & (vn * s >= 0) & ((un + vn) * s <= ad)
    safe = np.where(det == 0, 1, det)
    return dict(det_ok=det_ok, hit=hit, u=un / safe, v=vn / safe, t=np.ldexp(tn / safe, (-e - 4).astype(np.int64)),
                pow2=(ad & (ad - 1)) == 0)


def gid(a, hits):
    """Global triangle ids of rt_hit records (0 where there is no hit)."""
    hit = hits["hit"] != 0
    return np.where(hit, a["tri_begin"][np.where(hit, hits["mesh"], 0)].astype(np.int64) + hits["tri"], 0)


def leaf_order(nodes, tris):
    """Triangle ids in the order a depth-first walk, child 0 first, meets the exported tree's leaf records: (position of each
    global id in that order [n_triangles])."""
    child = np.ascontiguousarray(nodes[:, 12:14]).view(np.int32)
    ids = tris[:, 9]
    order, stack = [], [0]
    if len(nodes) == 0:
        order = list(ids)
    while stack and len(nodes):
        ref = stack.pop()
        if ref < 0:
            code = (~ref) & 0xFFFFFFFF
            order.extend(ids[code >> 3:(code >> 3) + (code & 7) + 1])
        else:
            stack.append(int(child[ref, 1])), stack.append(int(child[ref, 0]))
    pos = np.full(int(ids.max()) + 1, -1, np.int64)
    pos[np.array(order, np.int64)] = np.arange(len(order))
    return pos


def layers(name):
    """The scene's triangles (global ids) split into sets within which no two coincide: tracing a layer alone shows whether it
    has a triangle at a given t, for rays off the lattice too."""
    a = arrays(name)
    tb = a["tri_begin"].astype(int)
    per_mesh = [np.arange(tb[m], tb[m + 1]) for m in range(len(tb) - 1)]
    if name == "fan":
        return [np.concatenate(per_mesh[0:3]), per_mesh[3], per_mesh[4]]
    if name == "tiny3":
        return [np.array([k]) for k in range(3)]
    return per_mesh


def tie_counts(name, rays, hits):
    """By the oracle alone: for each ray, in how many layers of the scene the closest hit of that layer alone has the
    distance bits of the scene's closest hit `hits` (0 where the ray misses)."""
    import orc
    a = arrays(name)
    n = np.zeros(len(rays), np.int64)
    for ids in layers(name):
        tri = a["tri"][ids]
        solo = pyrt.ArrayScene(a["pos"], a["nrm"], tri, [0, len(tri)], [0, len(a["pos"])], a["materials"][:1], a["lights"], a["camera"])
        h = orc.trace(solo, rays)
        n += (h["hit"] != 0) & (hits["hit"] != 0) & (h["d"].view(np.uint32) == hits["d"].view(np.uint32))
    return n
