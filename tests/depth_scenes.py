"""Scenes at both ends of the frame kernels' stack-row range (test infrastructure; DESIGN.md §6q, "Stack rows").

The frame kernels carve their per-wave LDS from RenderArgs::stackLevels = BVH max_depth + 1 rows, and every launcher
clamps that number in its own way.  The presets the suite runs give 7 (cubes), 14 (lowres), 17 (hires) and 25 (stress)
rows; the scenes here give 2, 3, 4 and 5 and still have occluded shadow rays and bounce rays that hit, which the flat
one-to-three-triangle scenes of tiescenes.py do not.  (The suite's other purpose-built scenes: tiescenes.py — exact ties
between hits; soups.py — triangle soups for the tree builders; probe_card.py — 24 textured quads, each at one limit of the
sampler, the material maps or the normal maps.)

Shallow family: sub-scenes of the cubes preset — a subset of its five meshes, in mesh order, with their materials, all
three lights and the camera (ao_ref.without_mesh0, generalised), each with the bvh_leaf_max to create the context with.
The numbers of SHALLOW are the host builder's (tests/test_depth_scenes_cpu.py pins them, together with the liveness of
every scene).  Rows 2, 3 and 4 each appear on both sides of leaf_max <= 2, which selects the two-record leaf phase; row 5
is the first above every clamp of 4.  A, C and G are closed (every primary ray hits); B, D, E and F have misses.

Deep family: the hires preset (device builder, max_depth 16) and the stress preset (max_depth 24), as they are.

Every scene has a name the reference modules' scene() helpers take in place of a preset's: "depth:A" .. "depth:G", and
"depth:B4", "depth:C4", "depth:D4", "depth:F4", "depth:G4" (rows 2, 3, 3, 4, 5) — that scene under the four lights of
shading_sweep's scene 3, which the pooled body refuses.  pick_ref.scene(("depth:C", False, 5), w, h) is the many-lights
version."""
import numpy as np

import pyrt

PREFIX = "depth:"
# name: (meshes kept, bvh_leaf_max, triangles, nodes, max_depth).  stack rows = max_depth + 1
SHALLOW = {
    "A": ((0, 1, 2), 8, 10, 1, 1),
    "B": ((1, 2), 2, 4, 1, 1),
    "C": ((0, 1, 2, 3), 8, 22, 2, 2),
    "D": ((0,), 2, 6, 2, 2),
    "E": ((1, 2, 3), 4, 16, 3, 3),
    "F": ((0, 1), 2, 8, 3, 3),
    "G": ((0, 1, 2, 3), 4, 22, 5, 4),
}
NAMES = tuple(SHALLOW)
FOUR_LIGHTS = ("B4", "C4", "D4", "F4", "G4")  # the sequential body (more than three lights)
# The scenes an RT_NODES_Q8 context can hold (its records keep leaves of at most two triangles, so C and G, leaf_max 8
# and 4, are refused by rt_create): rows 2, 3 and 4
Q8_NAMES = ("B", "D", "F")
CLOSED = ("A", "C", "G")
# the deep presets: name -> max_depth of the host builder (the device builder's tree of hires has the same depth)
DEEP = {"hires": 16, "stress": 24}
# The parameters the liveness and sensitivity conditions are measured under, and the shallow GPU frames run with
W, H, SEED, MAX_DEPTH = 13, 9, 11, 3
SPP7_34 = dict(spp=7, spp_begin=3, spp_count=4)
# Liveness floors (conditions, not tolerances): about half the smallest shares the host builder's scenes show
# (occluded 0.097 on D, bounce hits 0.427 on B; tests/test_depth_scenes_cpu.py prints every share)
MIN_OCCLUDED, MIN_UNOCCLUDED, MIN_BOUNCE_HIT = 0.05, 0.05, 0.25
# Sensitivity: the share of the rgb words of the oracle's frame of A, B and C that change when one of the scene's own
# meshes is dropped, every mesh in turn.  Measured (scene: mesh dropped share ...): A: 0 0.989, 1 0.741, 2 0.781; B: 0
# 0.402, 1 0.419 (41 % of B's pixels are hit at all); C: 0 0.983, 1 0.635, 2 0.724, 3 0.709.  The floor is half the
# smallest.
SENSITIVE = ("A", "B", "C")
MIN_CHANGED = 0.2
_cache = {}


def sub_scene(s, keep):
    """The scene with only the meshes `keep` (ascending), in mesh order, with their materials; lights and camera kept."""
    a = s.arrays()
    vb, tb = a["vtx_begin"].astype(np.int64), a["tri_begin"].astype(np.int64)
    assert list(keep) == sorted(set(keep)) and 0 <= keep[0] and keep[-1] < len(tb) - 1, keep
    pos, nrm, tri, nvb, ntb = [], [], [], [0], [0]
    for m in keep:
        pos.append(a["pos"][vb[m]:vb[m + 1]])
        nrm.append(a["nrm"][vb[m]:vb[m + 1]])
        tri.append(a["tri"][tb[m]:tb[m + 1]].astype(np.int64) - vb[m] + nvb[-1])
        nvb.append(nvb[-1] + int(vb[m + 1] - vb[m]))
        ntb.append(ntb[-1] + int(tb[m + 1] - tb[m]))
    return pyrt.ArrayScene(np.concatenate(pos), np.concatenate(nrm), np.concatenate(tri).astype(np.uint32), np.array(ntb, np.uint32),
                           np.array(nvb, np.uint32), a["materials"][list(keep)], a["lights"], a["camera"])


def with_lights(s, lights):
    a = s.arrays()
    return pyrt.ArrayScene(a["pos"], a["nrm"], a["tri"], a["tri_begin"], a["vtx_begin"], a["materials"],
                           np.ascontiguousarray(lights, np.float32).reshape(-1, 21), a["camera"])


def base(name):
    """"C4" -> "C": the shallow scene a name's geometry is."""
    return name[0]


def is_depth(preset):
    return isinstance(preset, str) and preset.startswith(PREFIX)


def scene(name, w, h):
    """Shallow scene `name` ("A" .. "G", or one of FOUR_LIGHTS) at the frame's aspect; shared, never written to."""
    key = (name, w, h)
    if key not in _cache:
        assert base(name) in SHALLOW and (len(name) == 1 or name in FOUR_LIGHTS), name
        s = sub_scene(pyrt.Scene("cubes", w, h), SHALLOW[base(name)][0])
        if name in FOUR_LIGHTS:
            import shading_sweep
            s = with_lights(s, shading_sweep.build_scene("cubes", w, h, 3).arrays()["lights"])
        _cache[key] = s
    return _cache[key]


def preset(name, w, h):
    """What the reference modules' scene() helpers build their scenes from: pyrt.Scene(name, w, h), or for "depth:X" the
    shallow scene X."""
    return scene(name[len(PREFIX):], w, h) if is_depth(name) else pyrt.Scene(name, w, h)


def without_mesh(name, w, h, mesh):
    """Shallow scene `name` without its mesh `mesh` (an index into the scene's own meshes)."""
    s = scene(name, w, h)
    n = len(s.arrays()["tri_begin"]) - 1
    return sub_scene(s, [m for m in range(n) if m != mesh])


def leaf_max(preset_name):
    """The bvh_leaf_max a context of a scene is created with (0, the library's default, for the presets)."""
    return SHALLOW[base(preset_name[len(PREFIX):])][1] if is_depth(preset_name) else 0


def max_depth(preset_name):
    """The max_depth a context of a scene must report."""
    return SHALLOW[base(preset_name[len(PREFIX):])][4] if is_depth(preset_name) else DEEP[preset_name]


def context_options(preset_name):
    lm = leaf_max(preset_name)
    return dict(bvh_leaf_max=lm) if lm else {}


def params(w=W, h=H, **kw):
    """The shallow frames' parameters: samples 3..6 of 7, path mode at max_depth 3, seed 11."""
    args = dict(mode=pyrt.MODE_PATH, max_depth=MAX_DEPTH, seed=SEED)
    args.update(SPP7_34)
    args.update(kw)
    return pyrt.make_params(w, h, args.pop("spp"), **args)


def liveness(s, p):
    """What the frame `p` of scene `s` casts, from the oracle's ray dump and its any-hit / closest trace on the dumped
    rays (the way vcol_ref.frame decides occlusion): dict(primary_hit, occluded, bounce_hit: shares; shadow, bounce:
    counts; depths: the path depths at which a vertex exists)."""
    import orc
    nl = len(s.arrays()["lights"])
    ns = p.spp_count if p.spp_count else p.spp
    d = orc.dump_rays(s, p, cap=p.width * p.height * ns * 3 * (1 + nl) + 16)
    tag = np.ascontiguousarray(d[:, 3]).view(np.uint32)
    kind, depth = tag & 0xff, tag >> 8
    rays = np.zeros(len(d), pyrt.RAY_DTYPE)
    rays["origin"], rays["direction"] = d[:, 0:3], d[:, 4:7]
    cr, cd = rays[kind == 0], depth[kind == 0]
    hits = orc.trace(s, cr, accel=orc.ACCEL_OBVH)
    hit = (hits["hit"] != 0) & (hits["d"] > 0)
    sr = rays[kind == 1]
    occ = orc.trace(s, sr, accel=orc.ACCEL_OBVH, kind=pyrt.TRACE_ANY)["hit"] != 0
    bounce = cd > 0
    return dict(primary_hit=float(hit[cd == 0].mean()), occluded=float(occ.mean()), bounce_hit=float(hit[bounce].mean()),
                shadow=len(sr), bounce=int(bounce.sum()), depths=sorted(set(int(v) for v in cd[hit])))
