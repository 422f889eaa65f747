"""Deterministic sweep of the shading inputs: materials, direction triples, lights and whole scenes, in named
classes.  Plain numpy, seeded; shared by the CPU tests (tests/test_oracle_shading.py), the GPU tests
(tests/test_gpu_shading.py) and the golden-fixture script (tests/golden/make_shading_golden.py).

Row layouts (float32):
  material   [8]   kd alpha albedo3 f03                                   (rt_material)
  triple     [9]   n3 wi3 wo3
  bsdf row   [17]  material, triple                                       (RT_UNIT_BSDF's input)
  light spec [16]  position3 color3 direction3 intensity side factor ac al aq 0
                   (the arguments of LightSource's constructor and its four coefficients)
  light      [21]  position3 color3 vertical3 horizontal3 normal3 intensity side factor ac al aq   (rt_light)
  eval row   [24]  light, point3                                          (RT_UNIT_LIGHT_EVAL's input)

Every vector a sweep draws is between 1e-3 and 1e3 long, so squared lengths stay far below the 2^100 up to which the
FAST flavour of the device code is promised."""
import numpy as np

MATERIAL_CLASSES = ("interior", "corner", "corner_albedo", "out_of_range")
REGULAR_CLASSES = ("regular_unit", "regular_scaled")
DEGENERATE_CLASSES = ("grazing", "back_wi", "back_wo", "opposite", "near_opposite", "mirror", "null_normal", "extreme_lengths")
DIRECTION_CLASSES = REGULAR_CLASSES + DEGENERATE_CLASSES
ATTENUATION_CLASSES = ("general", "al_aq_zero", "all_zero")
ORIENTATION_CLASSES = ("general", "axis", "null")


def _rng(seed, stream):
    return np.random.default_rng([int(seed), int(stream)])


# ------------------------------------------------------------------ materials
def materials(seed, n_interior):
    """(mats [n][8] float32, cls [n] index into MATERIAL_CLASSES)."""
    g = _rng(seed, 1)
    rows, cls = [], []
    inner = np.clip(g.uniform(0, 1, (n_interior, 8)), 1e-6, 1 - 1e-6)
    for r in inner:
        rows.append(r), cls.append(0)
    for kd in (0.0, 1.0):
        for alpha in (1e-4, 1e-2, 1.0):
            for f0 in (0.0, 1.0):
                rows.append([kd, alpha, *g.uniform(0.05, 0.95, 3), f0, f0, f0]), cls.append(1)
    rows.append([0.5, 0.3, 0.0, 0.0, 0.0, 0.5, 0.5, 0.5]), cls.append(2)
    rows.append([0.7, 0.2, 1.5, 2.0, 4.0, 0.3, 0.6, 0.9]), cls.append(2)
    # outside the model's range but legal for the reference
    rows.append([0.5, 0.0, 0.8, 0.5, 0.3, 0.4, 0.4, 0.4]), cls.append(3)
    rows.append([0.5, 1.5, 0.8, 0.5, 0.3, 0.4, 0.4, 0.4]), cls.append(3)
    rows.append([0.3, 3.0, 0.2, 0.9, 0.6, 0.9, 0.1, 0.5]), cls.append(3)
    rows.append([1.5, 0.4, 0.6, 0.6, 0.2, 0.2, 0.5, 0.8]), cls.append(3)
    # Material's default constructor: m_kd = M_PI (narrowed to float), alpha 0.5, albedo (0.9, 0.4, 0.4), F0 0.31
    rows.append([np.float32(np.pi), 0.5, 0.9, 0.4, 0.4, 0.31, 0.31, 0.31]), cls.append(3)
    return np.array(rows, np.float64).astype(np.float32), np.array(cls, np.int32)


# ------------------------------------------------------------------ direction triples
def _unit(g, n):
    v = g.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _front(g, nrm, margin, sign=1.0):
    """Unit vectors w with sign * (n . w) > margin for the unit normals nrm, by rejection."""
    out = np.zeros_like(nrm)
    todo = np.arange(len(nrm))
    while len(todo):
        w = _unit(g, len(todo))
        d = (w * nrm[todo]).sum(1)
        w[d < 0] *= -1
        ok = np.abs(d) > margin
        out[todo[ok]] = sign * w[ok]
        todo = todo[~ok]
    return out


def _cos32(a, b):
    """n . w of the float32 rows as the shading code sees them: both normalised, in float32."""
    a, b = a.astype(np.float32), b.astype(np.float32)
    with np.errstate(all="ignore"):
        a = a / np.sqrt((a * a).sum(1, dtype=np.float32), dtype=np.float32)[:, None]
        b = b / np.sqrt((b * b).sum(1, dtype=np.float32), dtype=np.float32)[:, None]
        return (a * b).sum(1, dtype=np.float32)


def _lengths(g, n):
    return 10.0 ** g.uniform(-3, 3, (n, 1))


def directions(seed, n_per_class):
    """(triples [n][9] float32, cls [n] index into DIRECTION_CLASSES): n_per_class rows of each class."""
    g = _rng(seed, 2)
    m = n_per_class
    out, cls = [], []

    def add(name, n, wi, wo):
        t = np.concatenate([n, wi, wo], 1).astype(np.float32)
        out.append(t), cls.append(np.full(len(t), DIRECTION_CLASSES.index(name), np.int32))

    n = _unit(g, m)
    add("regular_unit", n, _front(g, n, 0.06), _front(g, n, 0.06))
    n = _unit(g, m)
    add("regular_scaled", n * _lengths(g, m), _front(g, n, 0.06) * _lengths(g, m), _front(g, n, 0.06) * _lengths(g, m))
    # grazing: n . wi = 0 — exactly (an axis normal, wi in its plane) on the even rows, to rounding (a cross product) on the odd
    n = _unit(g, m)
    wi = np.cross(n, _unit(g, m))
    ax = np.arange(m) % 3
    ev = np.arange(m) % 2 == 0
    n[ev] = 0
    n[ev, ax[ev]] = np.where(g.uniform(size=ev.sum()) < 0.5, -1.0, 1.0)
    wi[ev] = g.uniform(-1, 1, (ev.sum(), 3))
    wi[ev, ax[ev]] = 0
    add("grazing", n, wi, _front(g, n, 0.06) * _lengths(g, m))
    n = _unit(g, m)
    add("back_wi", n, _front(g, n, 0.06, -1.0) * _lengths(g, m), _front(g, n, 0.06))
    n = _unit(g, m)
    add("back_wo", n, _front(g, n, 0.06), _front(g, n, 0.06, -1.0) * _lengths(g, m))
    n = _unit(g, m)
    wi = (_front(g, n, 0.06) * _lengths(g, m)).astype(np.float32)
    add("opposite", n, wi, -wi)  # wi + wo = 0 exactly: the half vector is null
    # wo = -wi up to rounding (a few ulps off, or rescaled by a factor that is no power of two): wi + wo is rounding noise
    # after the normalisations, the half vector its direction, and wi . wh takes either sign — the fmax(0, .) of the
    # Fresnel term decides
    n = _unit(g, m)
    wi = (_front(g, n, 0.06) * _lengths(g, m)).astype(np.float32)
    off = wi.view(np.int32) + g.integers(-3, 4, wi.shape).astype(np.int32)
    wo = np.where((np.arange(m) % 2 == 0)[:, None], -off.view(np.float32), -(wi * g.uniform(0.5, 2.0, (m, 1)).astype(np.float32)))
    add("near_opposite", n, wi, wo)
    n = (_unit(g, m) * np.where(np.arange(m)[:, None] % 2 == 0, 1.0, _lengths(g, m))).astype(np.float32)
    add("mirror", n, n, n)  # n . wh = 1
    n = _unit(g, m)
    add("null_normal", np.zeros((m, 3)), _front(g, n, 0.06), _front(g, n, 0.06) * _lengths(g, m))
    n = _unit(g, m)
    ends = np.array([1e-3, 1e3])
    pick = g.integers(0, 2, (m, 3))
    add("extreme_lengths", n * ends[pick[:, 0:1]], _front(g, n, 0.06) * ends[pick[:, 1:2]], _front(g, n, 0.06) * ends[pick[:, 2:3]])
    t, c = np.concatenate(out), np.concatenate(cls)
    reg = np.isin(c, [DIRECTION_CLASSES.index(k) for k in REGULAR_CLASSES + ("extreme_lengths",)])
    assert (_cos32(t[reg, 0:3], t[reg, 3:6]) > 0.05).all() and (_cos32(t[reg, 0:3], t[reg, 6:9]) > 0.05).all()
    return t, c


def bsdf_rows(mats, mat_cls, triples, dir_cls):
    """Every material with every triple: (rows [nm * nd][17], material class, direction class)."""
    nm, nd = len(mats), len(triples)
    rows = np.concatenate([np.repeat(mats, nd, 0), np.tile(triples, (nm, 1))], 1)
    return np.ascontiguousarray(rows, np.float32), np.repeat(mat_cls, nd), np.tile(dir_cls, nm)


def must_be_finite(rows, dir_cls):
    """The rows the model must answer with finite numbers: a regular direction class and alpha >= 1e-4."""
    reg = np.isin(dir_cls, [DIRECTION_CLASSES.index(k) for k in REGULAR_CLASSES])
    return reg & (rows[:, 1] >= np.float32(1e-4))


# ------------------------------------------------------------------ lights
def _grid(x):
    """Multiples of 1/64 (so that position +- a unit axis is exact in float32)."""
    return np.round(np.asarray(x) * 64) / 64


def light_specs(seed, n):
    """(specs [n][16] float32, attenuation class [n], orientation class [n]).  Orientation: the light looks from
    `position` towards `direction`; "axis" ones look exactly along +-x, +-y, +-z (on +-x the constructor's basis
    collapses to null vectors), "null" ones have direction == position."""
    g = _rng(seed, 3)
    spec = np.zeros((n, 16))
    spec[:, 0:3] = _grid(g.uniform([-1.4, 0.2, -1.4], [1.4, 1.4, 2.9], (n, 3)))
    spec[:, 3:6] = g.uniform(0, 1.5, (n, 3))
    spec[:, 6:9] = _grid(g.uniform([-1.2, -1.0, -1.2], [1.2, 0.5, 1.2], (n, 3)))
    spec[:, 9] = g.uniform(0.1, 3.0, n)
    spec[:, 10] = np.where(np.arange(n) % 5 == 4, 0.0, g.uniform(0.005, 0.3, n))
    spec[:, 11] = g.uniform(0.5, 8.0, n)
    spec[:, 12:15] = 10.0 ** g.uniform(-3, 1, (n, 3))
    att = np.zeros(n, np.int32)
    att[np.arange(n) % 4 == 2] = 1
    att[np.arange(n) % 8 == 7] = 2
    spec[att == 1, 13:15] = 0
    black = np.flatnonzero(np.arange(n) % 4 == 3)  # one colour channel exactly 0 (0 * inf where the attenuation vanishes)
    spec[black, 3 + black % 3] = 0
    spec[att == 2, 12:15] = 0
    ori = np.zeros(n, np.int32)
    for i in range(n):
        if i % 3 == 1:
            ori[i] = 1
            axis, sign = (i // 3) % 3, 1.0 if (i // 9) % 2 == 0 else -1.0
            spec[i, 6:9] = spec[i, 0:3]
            spec[i, 6 + axis] += sign
        elif i % 16 == 15:
            ori[i] = 2
            spec[i, 6:9] = spec[i, 0:3]
    return spec.astype(np.float32), att, ori


def light_rows(specs, basis):
    """rt_light rows [n][21] of the specs, with basis [n][9] = vertical, horizontal, normal (the host's
    pyrt.light_basis(specs[:, 0:3], specs[:, 6:9]), or the reference's recorded one)."""
    specs = np.asarray(specs, np.float32)
    return np.ascontiguousarray(np.concatenate([specs[:, 0:6], np.asarray(basis, np.float32), specs[:, 9:15]], 1), np.float32)


def eval_points(seed, specs, n_random):
    """Evaluation points for each light: n_random in the room, the light's own position (d = 0), one far away.
    Returns (light index [m], points [m][3])."""
    g = _rng(seed, 4)
    idx, pts = [], []
    for i, s in enumerate(np.asarray(specs, np.float32)):
        p = g.uniform([-1.5, -1.0, -1.5], [1.5, 1.5, 1.5], (n_random, 3)).astype(np.float32)
        far = (s[0:3] + np.float32(1e3) * g.uniform(-1, 1, 3).astype(np.float32)).astype(np.float32)
        pts.append(np.concatenate([p, s[None, 0:3], far[None]]))
        idx.append(np.full(n_random + 2, i, np.int32))
    return np.concatenate(idx), np.concatenate(pts).astype(np.float32)


# ------------------------------------------------------------------ scenes
# The preset room (cubes / lowres geometry, five meshes: walls, left, right, the two objects) with swept materials and
# lights.  What each scene stresses:
SCENE_NOTES = {
    0: "interior materials, three general lights",
    1: "interior materials, one light",
    2: "corner materials (kd 0 / 1, alpha 1e-2 / 1, F0 0 / 1), two lights, one without linear and quadratic terms",
    3: "rough and smooth interior materials, four lights (beyond the pooled kernel's three), one looking along -y",
    4: "out-of-range materials (alpha > 1, kd > 1, the default Material with kd = pi), three lights, one along -z",
    5: "albedo 0 and albedo > 1, alpha 1e-4 on one object, two lights of side 0 and a coloured one",
    6: "interior materials, a light looking along -x (null basis: a point light), one general",
    7: "interior materials, strong attenuation spread (1e-3 .. 10), three lights",
}
N_SCENES = len(SCENE_NOTES)


def scene_spec(idx, seed=77):
    """(materials [5][8], light specs [n][16]) of swept scene idx."""
    g = _rng(seed, 100 + idx)
    mats, mcls = materials(seed + idx, 12)
    inner = mats[mcls == 0]
    pick = inner[g.choice(len(inner), 5, replace=False)].copy()
    pick[:, 1] = np.maximum(pick[:, 1], np.float32(0.02))
    corner = mats[mcls == 1]
    oor = mats[mcls == 3]

    def light(pos, towards, att="general", **kw):
        s = np.zeros(16)
        s[0:3], s[6:9] = _grid(pos), _grid(towards)
        s[3:6] = kw.get("color", g.uniform(0.4, 1.2, 3))
        s[9], s[10], s[11] = kw.get("intensity", g.uniform(0.4, 1.5)), kw.get("side", g.uniform(0.01, 0.2)), g.uniform(2.0, 6.0)
        s[12:15] = 10.0 ** g.uniform(-1, 0.3, 3) if "coef" not in kw else kw["coef"]
        if att == "al_aq_zero":
            s[12], s[13], s[14] = g.uniform(1.0, 3.0), 0, 0
        return s

    def jitter(p, r=0.3):
        return np.asarray(p) + g.uniform(-r, r, 3)
    front_l, front_r, low = (-1.4, 1.0, 2.9), (1.4, 1.0, 2.9), (0.0, -0.3, 1.1)
    aim_l, aim_r, aim_c = (0.3, 0.0, -1.0), (-0.3, 0.0, -1.0), (0.0, 0.0, -1.0)
    if idx == 0:
        lights = [light(jitter(front_l), jitter(aim_l)), light(jitter(front_r), jitter(aim_r)), light(jitter(low), jitter(aim_c))]
    elif idx == 1:
        lights = [light(jitter((0.0, 1.0, 2.5)), jitter(aim_c), intensity=2.0)]
    elif idx == 2:
        pick = corner[[2, 3, 5, 8, 10]].copy()  # kd 0 / 1 with alpha 1e-2 and 1, F0 0 and 1
        lights = [light(jitter(front_l), jitter(aim_l)), light(jitter(low), jitter(aim_c), att="al_aq_zero")]
    elif idx == 3:
        pick[0, 1], pick[3, 1] = 0.95, 0.03
        top = _grid(jitter((0.0, 1.25, 0.5), 0.2))
        lights = [light(jitter(front_l), jitter(aim_l)), light(jitter(front_r), jitter(aim_r)), light(jitter(low), jitter(aim_c)),
                  light(top, top + np.array([0.0, -1.0, 0.0]))]
    elif idx == 4:
        pick[1], pick[2], pick[3], pick[4] = oor[1], oor[3], oor[4], oor[2]
        back = _grid(jitter((0.2, 0.5, 2.5), 0.2))
        lights = [light(jitter(front_l), jitter(aim_l)), light(jitter(front_r), jitter(aim_r)), light(back, back + np.array([0.0, 0.0, -1.0]))]
    elif idx == 5:
        pick[1], pick[2] = mats[mcls == 2][0], mats[mcls == 2][1]
        pick[3, 1] = 1e-4
        lights = [light(jitter(front_l), jitter(aim_l), side=0.0), light(jitter(low), jitter(aim_c), side=0.0, color=(1.4, 0.2, 0.6))]
    elif idx == 6:
        side = _grid(jitter((1.25, 0.5, 1.5), 0.15))
        lights = [light(side, side + np.array([-1.0, 0.0, 0.0]), intensity=1.5), light(jitter(front_l), jitter(aim_l))]
    else:
        lights = [light(jitter(front_l), jitter(aim_l), coef=(1e-3, 10.0, 0.1)), light(jitter(front_r), jitter(aim_r), coef=(10.0, 1e-3, 1e-3)),
                  light(jitter(low), jitter(aim_c), coef=(0.1, 0.01, 10.0), intensity=3.0)]
    return np.ascontiguousarray(pick, np.float32), np.array(lights, np.float64).astype(np.float32)


def build_scene(kind, w, h, idx, seed=77):
    """The preset geometry and camera of `kind` at w x h with the materials and lights of swept scene idx, as a
    pyrt.ArrayScene (the lights' basis from the host's own LightSource constructor)."""
    import pyrt
    mats, specs = scene_spec(idx, seed)
    a = pyrt.Scene(kind, w, h).arrays()
    lights = light_rows(specs, pyrt.light_basis(specs[:, 0:3], specs[:, 6:9]))
    return pyrt.ArrayScene(a["pos"], a["nrm"], a["tri"], a["tri_begin"], a["vtx_begin"], mats, lights, a["camera"])


# ------------------------------------------------------------------ the comparison rule
def assert_same_bits(got, want, what=""):
    """Every element as a 32-bit pattern.  A NaN in `want` must be met by a NaN (sign and payload free: x86 and
    gfx950 make different default NaNs); everything else, +-0 and +-inf included, bit for bit.  Nothing is left out."""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan = np.isnan(want)
    bad = np.where(nan, ~np.isnan(got), got.view(np.uint32) != want.view(np.uint32))
    if bad.any():
        at = np.argwhere(bad)
        first = tuple(at[0])
        raise AssertionError("%s: %d of %d elements differ (%d expected NaNs), first at %s: got %r (0x%08x), want %r (0x%08x)"
                             % (what, len(at), bad.size, int(nan.sum()), first, got[first], got.view(np.uint32)[first],
                                want[first], want.view(np.uint32)[first]))
