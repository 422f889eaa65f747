"""The CPU reference of rt_render_lights (test infrastructure).

No restatement of anything: slice g of a frame split by light group is, by the contract of include/rt_amd.h (L1), the
oracle's own frame of the scene with the colours of the lights outside masks[g] set to (0, 0, 0) — the scene rebuilt as a
pyrt.ArrayScene, orc.render under MATH_DET.  The light samples are drawn and the shadow rays cast whether or not a light
is lit, so that frame shares every ray and every draw with the full frame; tests/test_lights_ref_cpu.py shows that on the
oracle alone, together with the condition that keeps a kernel which ignores or swaps masks from passing."""
import numpy as np

import ao_ref
import depth_scenes
import lens_ref
import orc
import pyrt
import shading_sweep

F32 = np.float32
SEED = 11
_cache = {}

SPP1, SPP4, SPP7, SPP7_34 = lens_ref.SPP1, lens_ref.SPP4, lens_ref.SPP7, lens_ref.SPP7_34
RAY, PATH = pyrt.MODE_RAY, pyrt.MODE_PATH


def scene(key, w, h):
    """key: (preset, opened) — the preset, or without its enclosing room, three lights — or ("sweep", preset, idx): the
    preset's geometry with the materials and the 1, 2 or 4 lights of shading_sweep's scene idx.  preset: a preset's name,
    or "depth:X" for depth_scenes' shallow scene X."""
    ck = ("scene", key, w, h)
    if ck not in _cache:
        if key[0] == "sweep":
            _cache[ck] = shading_sweep.build_scene(key[1], w, h, key[2])
        else:
            s = depth_scenes.preset(key[0], w, h)
            _cache[ck] = ao_ref.without_mesh0(s) if key[1] else s
    return _cache[ck]


def n_lights(s):
    return len(s.arrays()["lights"])


def all_mask(s):
    return (1 << n_lights(s)) - 1


def with_only(s, mask):
    """The scene with the colour of every light outside `mask` set to (0, 0, 0) (rt_light: floats 3..5 of a row)."""
    a = s.arrays()
    lights = np.array(a["lights"], F32).reshape(-1, 21).copy()
    for l in range(len(lights)):
        if not (mask >> l) & 1:
            lights[l, 3:6] = 0.0
    return pyrt.ArrayScene(a["pos"], a["nrm"], a["tri"], a["tri_begin"], a["vtx_begin"], a["materials"], lights, a["camera"])


def lights_only(s, mask):
    """The rt_light rows [n][21] of with_only(s, mask): what rt_update takes."""
    return with_only(s, mask).arrays()["lights"]


# (scene key, w, h, sample range, mode, max_depth, masks).  13x9: partial 8x8 wave tiles at both edges; 16x16: whole ones.
# Every size, range (1, 4, 7 and 3..7 of 7 samples), shading form (ray mode; path mode at depths 1, 2, 3), scene (cubes and
# lowres closed and open: three lights, the pooled body; sweep scenes 1, 2 and 5: one and two lights; sweep scene 3: four
# lights, the sequential body) and group count (1..4) appears several times.  The tables: singletons, overlapping pairs,
# all lights as one of several groups, an empty mask, and the same masks in two orders (the first two cases).  The
# schedule — default, no pool, 1 and 64 lanes per pixel, the counted instances, the exhaustive loop — does not change the
# expectation: test_gpu_lights.py runs all six on every case.
CASES = [
    (("cubes", False), 16, 16, SPP4, PATH, 3, (0b001, 0b010, 0b100)),
    (("cubes", False), 16, 16, SPP4, PATH, 3, (0b100, 0b001, 0b010)),
    (("cubes", False), 13, 9, SPP7, RAY, 1, (0b011, 0b110)),
    (("cubes", True), 13, 9, SPP7_34, PATH, 3, (0b111, 0b001, 0b000, 0b110)),
    (("cubes", True), 16, 16, SPP1, PATH, 2, (0b010, 0b101)),
    (("lowres", False), 13, 9, SPP4, PATH, 3, (0b111,)),
    (("lowres", False), 16, 16, SPP1, RAY, 1, (0b001, 0b010, 0b100)),
    (("lowres", True), 13, 9, SPP7, PATH, 2, (0b011, 0b110, 0b101, 0b111)),
    (("lowres", True), 16, 16, SPP4, PATH, 1, (0b000, 0b010)),
    (("sweep", "cubes", 1), 13, 9, SPP4, PATH, 3, (0b1, 0b0)),
    (("sweep", "lowres", 2), 16, 16, SPP7_34, PATH, 2, (0b01, 0b10, 0b11)),
    (("sweep", "cubes", 5), 13, 9, SPP1, PATH, 3, (0b10, 0b01)),
    (("sweep", "lowres", 3), 16, 16, SPP1, PATH, 3, (0b0001, 0b0010, 0b0100, 0b1000)),
    (("sweep", "cubes", 3), 13, 9, SPP7, RAY, 1, (0b0110, 0b1111, 0b1001)),
    (("sweep", "lowres", 3), 13, 9, SPP7_34, PATH, 2, (0b1000, 0b0011)),
]
# Two different masks of a case must differ in more than this share of their rgb words (the oracle's own minimum over
# every subset pair of these scenes is 25.7 %)
MIN_CHANGED = 0.2


def case_id(c):
    key, w, h, rng, mode, depth, masks = c
    name = "sweep%d_%s" % (key[2], key[1]) if key[0] == "sweep" else key[0] + ("_open" if key[1] else "")
    return "%s-%dx%d-%s-%s%d-%s" % (name, w, h, "+".join(str(v) for v in rng.values()), "path" if mode == PATH else "ray", depth,
                                    ".".join(format(m, "b") for m in masks))


def case_scene(c):
    return scene(c[0], c[1], c[2])


def case_masks(c):
    return c[6]


def case_params(c, **kw):
    key, w, h, rng, mode, depth, masks = c
    args = dict(mode=mode, max_depth=depth, seed=SEED)
    args.update(rng)
    args.update(kw)
    spp = args.pop("spp")
    return pyrt.make_params(w, h, spp, **args)


def case_background(c):
    return np.random.default_rng(c[1] * 100 + c[2]).uniform(0, 1, (c[2], c[1], 3)).astype(F32)


def masked_frame(c, mask, brute=False):
    """The oracle's frame of a case with only `mask` lit: dict(accum, out, closest, shadow); computed once, shared, never
    written to.  brute: over the oracle's exhaustive loop instead of its BVH."""
    key = ("frame", case_id(c[:6] + ((),)), mask, brute)
    if key not in _cache:
        s = case_scene(c)
        out, acc, st = orc.render(s if mask == all_mask(s) else with_only(s, mask), case_params(c), math_mode=orc.MATH_DET,
                                  bg=case_background(c), accel=orc.ACCEL_LOOP if brute else orc.ACCEL_OBVH)
        out.setflags(write=False), acc.setflags(write=False)
        _cache[key] = dict(accum=acc, out=out, closest=st.rays_closest, shadow=st.rays_shadow)
    return _cache[key]


def case_reference(c, brute=False):
    """rt_render_lights' expectation of a case: dict(accum [G][h][w][4], out [G][h][w][3], closest, shadow) — the counts
    are ONE frame's (L3)."""
    frames = [masked_frame(c, m, brute) for m in case_masks(c)]
    full = masked_frame(c, all_mask(case_scene(c)), brute)
    return dict(accum=np.stack([f["accum"] for f in frames]), out=np.stack([f["out"] for f in frames]),
                closest=full["closest"], shadow=full["shadow"])


def changed_rgb_words(a, b):
    """The share of the rgb words that differ between the accumulators a and b [h][w][4]."""
    return float((np.ascontiguousarray(a[..., :3]).view(np.uint32) != np.ascontiguousarray(b[..., :3]).view(np.uint32)).mean())
