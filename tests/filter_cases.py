"""Synthetic inputs for the three image-space filters (rt_denoise, rt_temporal_accumulate, rt_svgf): numpy only, no
rendering (test infrastructure; tests/test_filter_cases_cpu.py and tests/test_gpu_filter_cases.py run them).

A case is a size, a list of overlays and the call's settings.  build(case) returns the current frame (rgb, AOV sums,
motion channels) and a history for both filters, seeded by the case's name.  The content is piecewise smooth: up to four
"meshes", each a region with its own normal, a plane of positions and an albedo, the region borders on x = 16, 64, 128 and
y = 16 (or the middle row of a lower image), colour noise on top.  Overlays place their feature on the multiples of 16 (64
among them) and on those +-1, +-2, +-3 (marks), so that it lies on the seams of the 64x4 stage-A footprint and on the edges
and corners of the 16x16 tiles of the LDS kernels.

Every case passes sigma_position and sigma_reproject explicitly (0.25 and 0.5, exact in float32), so the restatements need
no scene; the one case of each list named "default_sigmas" leaves them 0 and needs the cubes scene.

EXPECT names, per overlay and setting, the counters of the restatements that the case must drive; T_SVGF and T_DENOISE hold
per case the largest |float32 evaluation - float64 evaluation| of the filtered outputs, measured on the CPU by
measure_svgf / measure_denoise (python tests/filter_cases.py prints both tables)."""
import zlib

import numpy as np

import aov_ref
import svgf_ref as sv
import temporal_ref as tr

SIGMA_POSITION, SIGMA_REPROJECT = 0.25, 0.5
MESH_IDS = (0xfffffffe, 1, 2, 0)  # by region; 0xfffffffe is a valid id, one below the miss marker
NORMALS = ((0.0, 0.0, 1.0), (0.6, 0.0, 0.8), (0.0, 0.6, 0.8), (0.36, 0.48, 0.8))
HITS = (1, 4, 7)
F32 = np.float32
BELOW_LONG = float(np.nextafter(F32(3), F32(0)))  # stored length whose L + 1 is the largest float below 4


def marks(n):
    """The multiples of 16 and those +-1, +-2, +-3, inside [0, n)."""
    return sorted({b + d for b in range(0, n + 16, 16) for d in range(-3, 4) if 0 <= b + d < n})


def mark_points(w, h):
    """One pixel per mark of x, walking through the marks of y: single pixels on and around the tile corners."""
    my = marks(h)
    return [(x, my[i % len(my)]) for i, x in enumerate(marks(w))]


def corner(w, h):
    """The pixel (16, 16), which starts the tile diagonally next to the first; clamped into a smaller image."""
    return min(16, w - 1), min(16, h - 1)


def regions(w, h):
    ys, xs = np.mgrid[0:h, 0:w]
    by = 16 if h > 16 else (h // 2 if h > 2 else h)
    return ((xs >= 16).astype(int) + (xs >= 64) + (xs >= 128)) % 2 + 2 * (ys >= by)


def base(w, h, rng, spacing, low_albedo):
    ys, xs = np.mgrid[0:h, 0:w]
    reg = regions(w, h)
    alb = rng.uniform(0.2, 1.0, (4, 3))
    if low_albedo:
        alb[0] = (5e-4, 2e-4, 8e-4)  # below the 1e-3 floor of the demodulation
    hits = rng.choice(HITS, (h, w)).astype(np.uint32)
    fh = hits.astype(F32)[..., None]
    nrm = (np.asarray(NORMALS)[reg] + rng.normal(0, 0.02, (h, w, 3))).astype(F32)
    pos = np.stack([spacing * xs, spacing * ys, reg + 0.1 * spacing * xs * (reg + 1)], axis=-1).astype(F32)
    shade = 0.5 + 0.3 * np.sin(0.2 * xs + 0.3 * ys)
    rgb = np.clip(alb[reg] * shade[..., None] + rng.normal(0, 0.08, (h, w, 3)) * alb[reg], 0, 1).astype(F32)
    sums = dict(albedo=(alb[reg].astype(F32) * fh).astype(F32), normal=(nrm * fh).astype(F32), position=(pos * fh).astype(F32),
                hits=hits)
    mesh = np.asarray(MESH_IDS, np.uint32)[reg]
    cur = dict(motion=np.zeros((h, w, 2), F32), position=pos.copy(), prev_position=pos.copy(), mesh=mesh.copy())
    d = (rgb / np.maximum(alb[reg].astype(F32), F32(1e-3))).astype(F32)
    color = np.maximum(d + rng.normal(0, 0.1, (h, w, 3)).astype(F32) * d, 0).astype(F32)
    lum = sv.luminance(color)
    hist = dict(color=color, moments=np.stack([lum, lum * lum + rng.uniform(0, 0.02, (h, w)).astype(F32)], axis=-1).astype(F32),
                position=(pos + rng.uniform(-0.01, 0.01, (h, w, 3)) * min(1.0, spacing / 0.01)).astype(F32), mesh=mesh.copy(),
                length=np.full((h, w), 2, F32),
                rgb=np.clip(rgb + rng.normal(0, 0.05, (h, w, 3)), 0, 1).astype(F32))
    return rgb, sums, cur, hist


# ---- overlays: each a function of the case's arrays, placing its feature by (w, h) --------------------------------------
def _holes_corners(c, w, h):
    cs = lambda n: sorted({b + d for b in range(16, n + 1, 16) for d in (-1, 0) if b + d < n} | {0, n - 1})
    for y in cs(h):
        for x in cs(w):
            c["sums"]["hits"][y, x] = 0


def _holes_column(c, w, h):
    for x in (15, 16):
        if x < w:
            c["sums"]["hits"][:, x] = 0


def _holes_isolated(c, w, h):
    x, y = corner(w, h)
    keep = c["sums"]["hits"][y, x]
    c["sums"]["hits"][...] = 0
    c["sums"]["hits"][y, x] = keep


def _holes_all(c, w, h):
    c["sums"]["hits"][...] = 0


def _flat_grey(c, w, h):
    """Colour 0.5 over albedo 1: the luminance 0.5 and its square are exact, so every variance is exactly 0."""
    c["rgb"][...] = 0.5
    c["sums"]["albedo"][...] = c["sums"]["hits"].astype(F32)[..., None]
    c["hist"]["color"][...] = 0.5
    c["hist"]["rgb"][...] = 0.5
    c["hist"]["moments"][...] = (0.5, 0.25)


def _len_zero(c, w, h):
    c["hist"]["length"][...] = 0


def _len_long(c, w, h):
    c["hist"]["length"][...] = c["rng"].choice((4, 5, 8), (h, w))


def _len_one_short(c, w, h):
    _len_long(c, w, h)
    x, y = corner(w, h)
    c["hist"]["length"][y, x] = 1


def _len_checker(c, w, h):
    ys, xs = np.mgrid[0:h, 0:w]
    c["hist"]["length"][...] = np.where((xs + ys) % 2 == 0, 3, 5)


def _len_edge(c, w, h):
    """Stored lengths 3 and the float below it: L + 1 is exactly 4.0 and the largest float below 4."""
    ys, xs = np.mgrid[0:h, 0:w]
    c["hist"]["length"][...] = np.where((xs + ys) % 2 == 0, 3.0, BELOW_LONG)


def _len_tap0(c, w, h):
    for i, (x, y) in enumerate(mark_points(w, h)):
        c["hist"]["length"][y, x] = (0.0, -1.0)[i % 2]


def _shift(dx, dy):
    def f(c, w, h):
        c["cur"]["motion"][...] = (dx, dy)
    return f


def _r_edges(axis):
    """Motion that puts r = pixel + motion on the comparison edges along `axis`: -1, n - 1 and n, in turn with no motion;
    and nextafter(n, 0), which is exact only from pixel 0."""
    def f(c, w, h):
        n = (w, h)[axis]
        ys, xs = np.mgrid[0:h, 0:w]
        p = (xs, ys)[axis]
        k = (xs + 2 * ys) % 4
        m = np.select([k == 0, k == 1, k == 2], [-1 - p, n - 1 - p, n - p], 0).astype(F32)
        m = np.where(p == 0, np.where(k % 2 == 0, np.nextafter(F32(n), F32(0)), m), m)
        c["cur"]["motion"][..., axis] = m
    return f


def _nonfinite(c, w, h):
    vals = (np.nan, np.inf, -np.inf, 1e30, -1e30)
    for i, (x, y) in enumerate(mark_points(w, h)):
        c["cur"]["motion"][y, x, i % 2] = vals[i % 5]


def _pos_on_sigma(c, w, h):
    """(no motion) history points at distance exactly sigma_reproject from prev_position along one axis (accepted: the
    test is <=), and at the next float (rejected)."""
    far = (F32(SIGMA_REPROJECT), np.nextafter(F32(SIGMA_REPROJECT), F32(1)))
    for i, (x, y) in enumerate(mark_points(w, h)):
        a = (i // 2) % 3
        c["cur"]["prev_position"][y, x] = c["hist"]["position"][y, x]
        c["cur"]["prev_position"][y, x, a] = 0
        c["hist"]["position"][y, x, a] = far[i % 2] * (1, -1)[(i // 6) % 2]


def _mesh_one_tap(c, w, h):
    for x, y in mark_points(w, h):
        m = c["hist"]["mesh"][y, x]
        c["hist"]["mesh"][y, x] = MESH_IDS[1] if m == MESH_IDS[0] else MESH_IDS[0]


def _miss(c, w, h):
    """Misses of the motion pass at single pixels."""
    for x, y in mark_points(w, h)[::3]:
        c["cur"]["mesh"][y, x] = 0xffffffff


# in the order they are applied: the motion first (prev_position follows it), then the history's features
OVERLAYS = dict(
    flat_grey=_flat_grey, holes_corners=_holes_corners, holes_column=_holes_column, holes_isolated=_holes_isolated,
    holes_all=_holes_all, shift_px=_shift(1, 0), shift_nx=_shift(-1, 0), shift_py=_shift(0, 1), shift_ny=_shift(0, -1),
    shift_p64=_shift(64, 0), shift_n64=_shift(-64, 0), half_p=_shift(0.5, 0.5), half_n=_shift(-0.5, -0.5), half_x=_shift(0.5, 0),
    rx_edges=_r_edges(0), ry_edges=_r_edges(1), nonfinite=_nonfinite, miss=_miss, FOLLOW=None, len_zero=_len_zero, len_long=_len_long,
    len_one_short=_len_one_short, len_checker=_len_checker, len_edge=_len_edge, len_tap0=_len_tap0, pos_on_sigma=_pos_on_sigma,
    mesh_one_tap=_mesh_one_tap)

# counters a case must drive: name -> (where, test); where: "a" stage A / accumulate_ref's info, "f" filter_info
GT0 = lambda name: (name, lambda v, n: v > 0)
EXPECT = dict(
    holes_corners=[("a", GT0("invalid"))], holes_column=[("a", GT0("invalid"))],
    holes_isolated=[("a", GT0("invalid")), ("f", ("isolated_valid", lambda v, n: v == 1))],
    holes_all=[("a", ("invalid", lambda v, n: v == n))],
    flat_grey=[("f", GT0("zero_variance_centre"))],
    shift_px=[("t", GT0("single_tap"))], shift_nx=[("t", GT0("single_tap"))], shift_py=[("t", GT0("single_tap"))],
    shift_ny=[("t", GT0("single_tap"))], shift_p64=[("t", GT0("single_tap")), ("t", GT0("outside"))],
    shift_n64=[("t", GT0("single_tap")), ("t", GT0("outside"))],
    half_p=[("t", GT0("history"))], half_n=[("t", GT0("history"))], half_x=[("t", GT0("history"))],
    rx_edges=[("t", GT0("rx_minus_one")), ("t", GT0("last_column_tap_outside")), ("t", GT0("single_tap")), ("t", GT0("outside")),
              ("t", GT0("no_weight"))],
    ry_edges=[("t", GT0("single_tap")), ("t", GT0("outside")), ("t", GT0("no_weight"))],
    nonfinite=[("t", GT0("nonfinite")), ("t", GT0("outside"))], miss=[("t", GT0("miss"))],
    len_zero=[("t", GT0("tap_nolength")), ("t", ("history", lambda v, n: v == 0))],
    len_long=[("a", GT0("long_history")), ("a", ("window", lambda v, n: v == 0))],
    len_one_short=[("a", GT0("long_history")), ("a", ("window", lambda v, n: v == 1))],
    len_checker=[("a", GT0("long_history"))], len_edge=[("a", GT0("length_exactly_long")), ("a", GT0("length_just_short"))],
    len_tap0=[("t", GT0("tap_nolength"))], pos_on_sigma=[("t", GT0("position_on_sigma")), ("t", GT0("tap_position"))],
    mesh_one_tap=[("t", GT0("tap_mesh"))],
    max_history_1=[("t", GT0("saturated"))], alpha_min=[("t", GT0("alpha_bound"))], alpha_min_moments=[("a", GT0("alpha_moments_bound"))],
    far_128=[("f", ("far_tap_in_range", lambda v, n: v.get(128, 0) > 0))])


def case(name, size, *overlays, spacing=0.01, low_albedo=False, **kw):
    return dict(name=name, size=size, overlays=overlays, spacing=spacing, low_albedo=low_albedo, kw=kw)


def expectations(c, filt):
    """The (where, (counter, test)) list of case c for filter `filt` ("svgf", "temporal" or "denoise"): "t" entries apply to
    both reprojecting filters, "a" and "f" to rt_svgf alone."""
    names = list(c["overlays"])
    kw = c["kw"]
    if kw.get("max_history") == 1:
        names.append("max_history_1")
    if kw.get("alpha_min", 0) >= 0.4 and kw.get("max_history") != 1 and "len_zero" not in names:  # (1 / 1 is no bound)
        names.append("alpha_min")
    if kw.get("alpha_min_moments", 0) == 1:
        names.append("alpha_min_moments")
    if c["size"] == (513, 3) and kw.get("iterations") == 8 and filt == "svgf":
        names.append("far_128")
    out = [e for n in names for e in EXPECT.get(n, [])]
    return [e for e in out if filt == "svgf" or (filt == "temporal" and e[0] == "t")]


def cubes_scene(c):
    import pyrt
    return pyrt.Scene("cubes", *c["size"])


def build(c):
    """The arrays of case c: dict of rgb, sums (albedo, normal, position, hits), cur (motion, position, prev_position,
    mesh), svgf_hist and temporal_hist (sharing position, mesh and length), scene (None unless the case leaves the sigmas
    0), and the keyword arguments of the three calls: svgf_kw, temporal_kw, denoise_kw."""
    w, h = c["size"]
    rng = np.random.default_rng(zlib.crc32(c["name"].encode()))
    default = c["name"].startswith("default_sigmas")
    scene = cubes_scene(c) if default else None
    spacing = c["spacing"] * (float(tr.default_sigma_position(scene)) / SIGMA_POSITION if default else 1.0)
    rgb, sums, cur, hist = base(w, h, rng, spacing, c["low_albedo"])
    a = dict(rgb=rgb, sums=sums, cur=cur, hist=hist, rng=rng)
    for name, f in OVERLAYS.items():
        if name == "FOLLOW":  # the previous-frame surface point is the history's at the nearest pixel the motion points to
            m = cur["motion"].astype(np.float64)
            ok = np.isfinite(m).all(-1) & (np.abs(np.nan_to_num(m)) < 1e6).all(-1)
            m = np.where(ok[..., None], m, 0.0)
            ys, xs = np.mgrid[0:h, 0:w]
            tx = np.clip(np.floor(xs + m[..., 0] + 0.5), 0, w - 1).astype(int)
            ty = np.clip(np.floor(ys + m[..., 1] + 0.5), 0, h - 1).astype(int)
            cur["prev_position"][...] = hist["position"][ty, tx]
        elif name in c["overlays"]:
            f(a, w, h)
    assert set(c["overlays"]) <= set(OVERLAYS), c["overlays"]
    # as the renderer's passes relate: no sample of the pixel hit, so the motion pass's first sample missed too
    hole = sums["hits"] == 0
    cur["mesh"][hole] = 0xffffffff
    for k in ("motion", "position", "prev_position"):
        cur[k][hole] = 0
    kw = dict(c["kw"])
    it, dit = kw.pop("iterations", 0), kw.pop("denoise_iterations", 0)
    sig = {} if default else dict(sigma_position=SIGMA_POSITION)
    rep = {} if default else dict(sigma_reproject=SIGMA_REPROJECT)
    return dict(rgb=rgb, sums=sums, cur=cur, scene=scene,
                svgf_hist={k: hist[k] for k in sv.HISTORY_CHANNELS}, temporal_hist={k: hist[k] for k in ("rgb", "position", "mesh", "length")},
                svgf_kw=dict(kw, iterations=it, **sig, **rep),
                temporal_kw=dict({k: v for k, v in kw.items() if k in ("max_history", "alpha_min")},
                                 **({} if default else dict(sigma_position=SIGMA_REPROJECT))),
                denoise_kw=dict(iterations=dit, **sig))


S = dict(s1=(1, 1), col=(1, 70), row=(70, 1), t16=(16, 16), t17=(17, 17), t33=(33, 16), a63=(63, 4), a64=(64, 4), a65=(65, 5),
         a129=(129, 9), m130=(130, 21), far=(513, 3))

SVGF_CASES = [
    case("1x1", S["s1"]),
    case("1x1_no_hit", S["s1"], "holes_all"),
    case("1x70_first_frame_8", S["col"], "len_zero", iterations=8),
    case("1x70_ry_edges", S["col"], "ry_edges", max_history=4),
    case("70x1_half", S["row"], "half_x", iterations=2),
    case("70x1_rx_edges", S["row"], "rx_edges", max_history=1000),
    case("16x16_long", S["t16"], "len_long", max_history=1000),
    case("16x16_nonfinite", S["t16"], "nonfinite", "miss"),
    case("17x17_one_short", S["t17"], "len_one_short", max_history=1000),
    case("17x17_holes_corners", S["t17"], "holes_corners"),
    case("17x17_pos_on_sigma", S["t17"], "pos_on_sigma", max_history=4),
    case("33x16_holes_column_1", S["t33"], "holes_column", iterations=1),
    case("33x16_checker", S["t33"], "len_checker", max_history=1000),
    case("63x4_shift_px", S["a63"], "shift_px"),
    case("63x4_checker_half", S["a63"], "len_checker", "half_x", max_history=1000),
    case("64x4_shift_nx", S["a64"], "shift_nx", max_history=4, alpha_min=0.4),
    case("64x4_holes_column_8", S["a64"], "holes_column", iterations=8),
    case("65x5_shift_py", S["a65"], "shift_py"),
    case("65x5_shift_ny", S["a65"], "shift_ny", max_history=4, alpha_min=0.4, alpha_min_moments=1.0, iterations=2),
    case("65x5_rx_edges", S["a65"], "rx_edges"),
    case("129x9_shift_p64", S["a129"], "shift_p64"),
    case("129x9_shift_n64", S["a129"], "shift_n64", alpha_min_moments=1.0),
    case("129x9_ry_edges", S["a129"], "ry_edges"),
    case("129x9_one_short", S["a129"], "len_one_short", max_history=4),
    case("130x21", S["m130"]),
    case("130x21_holes_corners", S["m130"], "holes_corners"),
    case("130x21_one_short", S["m130"], "len_one_short", max_history=1000),
    case("130x21_isolated", S["m130"], "holes_isolated"),
    case("130x21_no_hit", S["m130"], "holes_all"),
    case("130x21_long_4", S["m130"], "len_long", max_history=4),
    case("130x21_len_edge_4", S["m130"], "len_edge", max_history=4),
    case("130x21_len_edge_8", S["m130"], "len_edge", max_history=1000, iterations=8),
    case("130x21_half_mesh_tap", S["m130"], "half_n", "mesh_one_tap"),
    case("130x21_pos_on_sigma", S["m130"], "pos_on_sigma"),
    case("130x21_nonfinite", S["m130"], "nonfinite", "miss", "holes_column"),
    case("130x21_half_tap0", S["m130"], "half_p", "len_tap0", max_history=1000),
    case("130x21_rx_edges", S["m130"], "rx_edges", max_history=4),
    case("130x21_low_albedo", S["m130"], low_albedo=True),
    case("130x21_flat_first", S["m130"], "flat_grey", "len_zero"),
    case("130x21_flat_long", S["m130"], "flat_grey", "len_long", max_history=1000, alpha_min=0.4),
    case("130x21_alpha_1", S["m130"], max_history=1, alpha_min=1.0, iterations=1),
    case("default_sigmas_130x21", S["m130"], "holes_corners"),
    case("513x3_8_long", S["far"], "len_long", spacing=0.001, max_history=1000, iterations=8),
    case("513x3_8_shift_p64", S["far"], "shift_p64", "holes_corners", spacing=0.001, iterations=8),
]

TEMPORAL_CASES = [
    case("1x1", S["s1"]),
    case("1x70_ry_edges", S["col"], "ry_edges", max_history=4),
    case("70x1_rx_edges", S["row"], "rx_edges", max_history=1000),
    case("16x16_nonfinite", S["t16"], "nonfinite", "miss"),
    case("17x17_pos_on_sigma", S["t17"], "pos_on_sigma", max_history=4),
    case("33x16_half_tap0", S["t33"], "half_p", "len_tap0"),
    case("63x4_shift_px", S["a63"], "shift_px", max_history=1),
    case("64x4_shift_nx", S["a64"], "shift_nx", alpha_min=0.4),
    case("64x4_first_frame", S["a64"], "len_zero", alpha_min=1.0),
    case("65x5_shift_py", S["a65"], "shift_py", max_history=1000),
    case("65x5_shift_ny", S["a65"], "shift_ny", max_history=4, alpha_min=0.4),
    case("65x5_rx_edges", S["a65"], "rx_edges"),
    case("129x9_shift_p64", S["a129"], "shift_p64"),
    case("129x9_shift_n64", S["a129"], "shift_n64", alpha_min=1.0),
    case("129x9_ry_edges", S["a129"], "ry_edges"),
    case("129x9_half_mesh_tap", S["a129"], "half_x", "mesh_one_tap"),
    case("130x21", S["m130"]),
    case("130x21_first_frame", S["m130"], "len_zero"),
    case("130x21_len_edge", S["m130"], "len_edge", max_history=4),
    case("130x21_half_mesh_tap", S["m130"], "half_n", "mesh_one_tap", max_history=1000),
    case("130x21_pos_on_sigma", S["m130"], "pos_on_sigma"),
    case("130x21_nonfinite", S["m130"], "nonfinite", "miss", max_history=4),
    case("130x21_rx_edges", S["m130"], "rx_edges", max_history=1, alpha_min=0.4),
    case("default_sigmas_130x21", S["m130"], "half_p"),
    case("513x3_shift_n64", S["far"], "shift_n64", spacing=0.001),
]

DENOISE_CASES = [
    case("1x1", S["s1"], denoise_iterations=5),
    case("1x70_8", S["col"], denoise_iterations=8),
    case("70x1_8", S["row"], "holes_corners", denoise_iterations=8),
    case("16x16_1", S["t16"], denoise_iterations=1),
    case("17x17_5", S["t17"], "holes_corners", denoise_iterations=5),
    case("33x16_5", S["t33"], "holes_column", denoise_iterations=5),
    case("64x4_8", S["a64"], denoise_iterations=8),
    case("65x5_1", S["a65"], "holes_column", denoise_iterations=1),
    case("129x9_5", S["a129"], "holes_corners", denoise_iterations=5),
    case("130x21_8", S["m130"], denoise_iterations=8),
    case("130x21_isolated", S["m130"], "holes_isolated", denoise_iterations=5),
    case("130x21_no_hit", S["m130"], "holes_all", denoise_iterations=5),
    case("130x21_low_albedo", S["m130"], "holes_corners", low_albedo=True, denoise_iterations=5),
    case("default_sigmas_130x21", S["m130"], "holes_column", denoise_iterations=5),
    case("513x3_8", S["far"], "holes_corners", spacing=0.001, denoise_iterations=8),
]

DEVICE_FORM_CASES = ("130x21_holes_corners", "65x5_rx_edges")  # of SVGF_CASES; the denoiser's: DENOISE_DEVICE_FORM_CASES
DENOISE_DEVICE_FORM_CASES = ("130x21_8", "65x5_1")
ONE_CONTEXT_ORDER = ("513x3_8_long", "1x1", "130x21_one_short", "130x21_one_short")  # of SVGF_CASES; DENOISE: below
DENOISE_ONE_CONTEXT_ORDER = ("513x3_8", "1x1", "130x21_8", "130x21_8")


def by_name(cases, name):
    return next(c for c in cases if c["name"] == name)


def svgf_refs(b):
    """Stage A and both evaluations of stages B and C on build()'s arrays: (A, float64 outputs, float32 outputs)."""
    kw = b["svgf_kw"]
    akw = {k: kw[k] for k in ("max_history", "alpha_min", "alpha_min_moments", "sigma_reproject") if k in kw}
    fkw = {k: v for k, v in kw.items() if k not in akw}
    A = sv.stage_a(b["rgb"], b["sums"], b["cur"], b["svgf_hist"], scene=b["scene"], **akw)
    return A, sv.filter_stages(A, b["sums"], scene=b["scene"], **fkw), sv.filter_stages(A, b["sums"], scene=b["scene"], f32=True, **fkw)


def measure_svgf(b):
    """(A, float64 outputs, T): T per filtered output, max |float32 evaluation - float64 evaluation|."""
    A, o64, o32 = svgf_refs(b)
    return A, o64, tuple(float(np.abs(o32[k].astype(np.float64) - o64[k].astype(np.float64)).max()) for k in sv.FILTERED)


def measure_denoise(b):
    """(float64 output, T)."""
    o64 = aov_ref.atrous(b["rgb"], b["sums"], scene=b["scene"], **b["denoise_kw"])
    o32 = aov_ref.atrous(b["rgb"], b["sums"], scene=b["scene"], f32=True, **b["denoise_kw"])
    return o64, float(np.abs(o32.astype(np.float64) - o64.astype(np.float64)).max())


# T per case: (colour, rgb, variance) of rt_svgf and the output of rt_denoise; from the restatements alone, rounded up to
# two digits.  tests/test_filter_cases_cpu.py re-measures every entry; the GPU test allows svgf_ref.TOLERANCE_FACTOR times
# the entry (and never more than 1e-4 for rt_denoise).
T_SVGF = {
    "1x1": (0.0, 0.0, 1.5e-08),
    "1x1_no_hit": (0.0, 0.0, 0.0),
    "1x70_first_frame_8": (1.8e-07, 2.4e-07, 2.6e-08),
    "1x70_ry_edges": (1.2e-07, 2.4e-07, 7.5e-09),
    "70x1_half": (1.2e-07, 1.2e-07, 2.7e-08),
    "70x1_rx_edges": (2.4e-07, 2.4e-07, 2.2e-08),
    "16x16_long": (3e-07, 3e-07, 1.9e-09),
    "16x16_nonfinite": (2.4e-07, 2.4e-07, 2.3e-09),
    "17x17_one_short": (3e-07, 1.8e-07, 4.3e-08),
    "17x17_holes_corners": (1.8e-07, 3e-07, 1.1e-08),
    "17x17_pos_on_sigma": (2.4e-07, 3e-07, 9.4e-09),
    "33x16_holes_column_1": (2.4e-07, 2.4e-07, 3.2e-08),
    "33x16_checker": (3.6e-07, 2.4e-07, 1.3e-09),
    "63x4_shift_px": (1.8e-07, 2.4e-07, 1.1e-08),
    "63x4_checker_half": (1.8e-07, 2.7e-07, 4.7e-09),
    "64x4_shift_nx": (1.8e-07, 2.4e-07, 4.5e-09),
    "64x4_holes_column_8": (1.8e-07, 2.7e-07, 5.4e-09),
    "65x5_shift_py": (1.8e-07, 3e-07, 4.2e-08),
    "65x5_shift_ny": (1.8e-07, 1.8e-07, 6e-08),
    "65x5_rx_edges": (1.8e-07, 3.6e-07, 8.9e-08),
    "129x9_shift_p64": (2.4e-07, 3e-07, 1.1e-07),
    "129x9_shift_n64": (3e-07, 3.6e-07, 8.8e-08),
    "129x9_ry_edges": (2.4e-07, 2.4e-07, 2.9e-08),
    "129x9_one_short": (3.6e-07, 3.6e-07, 6.8e-09),
    "130x21": (3e-07, 3e-07, 4.9e-09),
    "130x21_holes_corners": (3e-07, 4.2e-07, 7e-09),
    "130x21_one_short": (3e-07, 7.2e-07, 1.6e-09),
    "130x21_isolated": (6e-08, 0.0, 1.2e-08),
    "130x21_no_hit": (0.0, 0.0, 0.0),
    "130x21_long_4": (3e-07, 3.6e-07, 1.9e-09),
    "130x21_len_edge_4": (3.6e-07, 6.6e-07, 3e-09),
    "130x21_len_edge_8": (3.6e-07, 4.8e-07, 3.5e-09),
    "130x21_half_mesh_tap": (3e-07, 5.4e-07, 4.2e-09),
    "130x21_pos_on_sigma": (2.4e-07, 3.6e-07, 5.2e-09),
    "130x21_nonfinite": (3.6e-07, 3.6e-07, 3.8e-09),
    "130x21_half_tap0": (3.6e-07, 3.6e-07, 4.9e-09),
    "130x21_rx_edges": (3e-07, 3.3e-07, 4.7e-09),
    "130x21_low_albedo": (3e-07, 2.7e-07, 5.2e-09),
    "130x21_flat_first": (0.0, 0.0, 0.0),
    "130x21_flat_long": (0.0, 0.0, 0.0),
    "130x21_alpha_1": (3.6e-07, 3e-07, 9.1e-08),
    "default_sigmas_130x21": (3e-07, 3.9e-07, 6.7e-09),
    "513x3_8_long": (2.4e-07, 4.2e-07, 3.2e-09),
    "513x3_8_shift_p64": (4.2e-07, 4.2e-07, 4.6e-09),
}
T_DENOISE = {
    "1x1": 3e-08,
    "1x70_8": 1.2e-07,
    "70x1_8": 1.8e-07,
    "16x16_1": 3e-07,
    "17x17_5": 3e-07,
    "33x16_5": 1.8e-07,
    "64x4_8": 2.4e-07,
    "65x5_1": 1.8e-07,
    "129x9_5": 2.7e-07,
    "130x21_8": 3.6e-07,
    "130x21_isolated": 0.0,
    "130x21_no_hit": 0.0,
    "130x21_low_albedo": 2.7e-07,
    "default_sigmas_130x21": 3e-07,
    "513x3_8": 2.4e-07,
}


def _up(v):
    """v rounded up to two significant digits."""
    if v == 0:
        return 0.0
    e = int(np.floor(np.log10(v))) - 1
    return float("%.1e" % (np.ceil(v / 10.0 ** e * (1 - 1e-12)) * 10.0 ** e))


if __name__ == "__main__":
    print("T_SVGF = {")
    for c in SVGF_CASES:
        print('    "%s": (%s),' % (c["name"], ", ".join(repr(_up(t)) for t in measure_svgf(build(c))[2])))
    print("}\nT_DENOISE = {")
    for c in DENOISE_CASES:
        print('    "%s": %r,' % (c["name"], _up(measure_denoise(build(c))[1])))
    print("}")
