"""CPU restatement of rt_svgf (test infrastructure), built like temporal_ref.py and aov_ref.py.

stage_a: demodulation in float32 as the denoiser forms it, then the reprojection of rt_temporal_accumulate (tap by tap in
the stated order, float64) over the demodulated colour, the two luminance moments and the length, with a count of every
branch the frame took.

filter_stages: the variance estimate (stage B) and the a-trous iterations (stage C) in float64, or — f32=True — with
every operation in float32 in the device's order (taps row by row, the sums running in that order)."""
import numpy as np

import aov_ref
import temporal_ref as tr

MISS = aov_ref.MISS
H5 = aov_ref.H5
G3 = (0.25, 0.5, 0.25)  # the 3x3 Gaussian of the variance is G3[dx] G3[dy]: 1/4, 1/8, 1/16
LUM = (0.2126, 0.7152, 0.0722)
# the defaults of rt_svgf_params (rt_amd.h; tools/svgf_sweep.py chose them)
ITERATIONS, MAX_HISTORY, SIGMA_LUMINANCE, SIGMA_NORMAL, SIGMA_POSITION_SCALE = 5, 2, 2.0, 0.5, 0.02
HISTORY_CHANNELS = ("color", "moments", "position", "mesh", "length")
LONG_HISTORY = 4.0  # from this length on the temporal moments alone give the variance


def demodulate(rgb, sums):
    """(factor, demodulated colour, valid): float32, as rt_denoise forms them; hits == 0: factor 1, colour rgb."""
    rgb = np.asarray(rgb, np.float32)
    hits = np.asarray(sums["hits"])
    valid = hits > 0
    fh = np.maximum(hits, 1).astype(np.float32)[..., None]
    fac = np.where(valid[..., None], np.maximum(np.asarray(sums["albedo"], np.float32) / fh, np.float32(1e-3)), np.float32(1))
    fac = fac.astype(np.float32)
    return fac, (rgb / fac).astype(np.float32), valid


def luminance(c):
    """(0.2126 r + 0.7152 g) + 0.0722 b in c's own precision."""
    t = c.dtype.type
    return (t(LUM[0]) * c[..., 0] + t(LUM[1]) * c[..., 1]) + t(LUM[2]) * c[..., 2]


def stage_a(cur_rgb, sums, cur, prev, max_history=0, alpha_min=0., alpha_min_moments=0., sigma_reproject=0., scene=None):
    """Stage A: dict of fac, valid, accum [h][w][3], moments [h][w][2], length [h][w] (float32) and info (branch counts).
    cur: motion, prev_position, mesh; prev: color, moments, position, mesh, length."""
    maxh = float(max_history or MAX_HISTORY)
    amin, aminm = float(np.float32(alpha_min)), float(np.float32(alpha_min_moments))
    sig = float(np.float32(sigma_reproject) if sigma_reproject else tr.default_sigma_position(scene))
    s2 = sig * sig
    fac, d32, valid = demodulate(cur_rgb, sums)
    d = d32.astype(np.float64)
    l = luminance(d)
    cur5 = np.concatenate([d, l[..., None], (l * l)[..., None]], axis=-1)
    mesh = np.asarray(cur["mesh"], np.uint32)
    h, w = mesh.shape
    mx, my = cur["motion"][..., 0], cur["motion"][..., 1]
    X = np.asarray(cur["prev_position"], np.float32).astype(np.float64)
    ys, xs = np.mgrid[0:h, 0:w]
    miss = mesh == MISS
    nonfinite = ~miss & ~(np.isfinite(mx) & np.isfinite(my))
    with np.errstate(invalid="ignore"):
        rx, ry = xs + mx.astype(np.float64), ys + my.astype(np.float64)
        outside = ~miss & ~nonfinite & ((rx < -1) | (rx >= w) | (ry < -1) | (ry >= h))
    cand = ~(miss | nonfinite | outside)
    rx, ry = np.where(cand, rx, 0.0), np.where(cand, ry, 0.0)
    fx, fy = np.floor(rx), np.floor(ry)
    ax, ay = rx - fx, ry - fy
    x0, y0 = fx.astype(np.int64), fy.astype(np.int64)
    wxs, wys = (1.0 - ax, ax), (1.0 - ay, ay)
    W, SL, S = np.zeros((h, w)), np.zeros((h, w)), np.zeros((h, w, 5))
    info = dict(miss=int(miss.sum()), nonfinite=int(nonfinite.sum()), outside=int(outside.sum()), tap_mesh=0, tap_position=0,
                tap_nolength=0)
    info.update(tr.edge_counts(cand, rx, x0, ax, ay, w))
    h5 = np.concatenate([np.asarray(prev["color"], np.float32), np.asarray(prev["moments"], np.float32)], axis=-1)
    hpos = np.asarray(prev["position"], np.float32)
    hmesh, hlen = np.asarray(prev["mesh"], np.uint32), np.asarray(prev["length"], np.float32)
    for i, j in tr.TAPS:
        wt = wxs[i] * wys[j]
        x, y = x0 + i, y0 + j
        base = cand & (wt > 0) & (x >= 0) & (x < w) & (y >= 0) & (y < h)
        xc, yc = np.clip(x, 0, w - 1), np.clip(y, 0, h - 1)
        tl = hlen[yc, xc]
        with np.errstate(invalid="ignore"):
            haslen = tl > 0
        meshok = hmesh[yc, xc] == mesh
        dd = hpos[yc, xc].astype(np.float64) - X
        with np.errstate(invalid="ignore", over="ignore"):
            d2 = (dd[..., 0] * dd[..., 0] + dd[..., 1] * dd[..., 1]) + dd[..., 2] * dd[..., 2]
            posok = d2 <= s2
        ok = base & haslen & meshok & posok
        info["position_on_sigma"] += int((ok & (d2 == s2)).sum())
        info["tap_nolength"] += int((base & ~haslen).sum())
        info["tap_mesh"] += int((base & haslen & ~meshok).sum())
        info["tap_position"] += int((base & haslen & meshok & ~posok).sum())
        W = np.where(ok, W + wt, W)
        S = np.where(ok[..., None], S + wt[..., None] * h5[yc, xc].astype(np.float64), S)
        SL = np.where(ok, SL + wt * tl.astype(np.float64), SL)
    hist = cand & (W > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        hh, L = S / W[..., None], SL / W
        Ln = np.minimum(L + 1.0, maxh)
        alpha, alpham = np.maximum(1.0 / Ln, amin), np.maximum(1.0 / Ln, aminm)
        al = np.stack([alpha] * 3 + [alpham] * 2, axis=-1)
        out5 = np.where(hist[..., None], hh + al * (cur5 - hh), cur5).astype(np.float32)
        length = np.where(hist, Ln, 1.0).astype(np.float32)
        info.update(no_weight=int((cand & ~hist).sum()), history=int(hist.sum()), saturated=int((hist & (L + 1.0 > maxh)).sum()),
                    alpha_bound=int((hist & (amin > 1.0 / Ln)).sum()), alpha_moments_bound=int((hist & (aminm > 1.0 / Ln)).sum()))
    info.update(invalid=int((~valid).sum()), window=int((valid & (length < LONG_HISTORY)).sum()),
                long_history=int((valid & (length >= LONG_HISTORY)).sum()),
                length_exactly_long=int((valid & hist & (length == np.float32(LONG_HISTORY))).sum()),
                length_just_short=int((valid & hist & (length == np.nextafter(np.float32(LONG_HISTORY), np.float32(0)))).sum()))
    return dict(fac=fac, valid=valid, accum=np.ascontiguousarray(out5[..., :3]), moments=np.ascontiguousarray(out5[..., 3:]),
                length=length, info=info)


def _sq3(a, b):
    d = a - b
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def _shift(a, qy, qx):
    return a[qy][:, qx]


def filter_stages(A, sums, iterations=0, sigma_luminance=0., sigma_normal=0., sigma_position=0., scene=None, f32=False):
    """Stages B and C on stage_a's result A: dict of rgb, color [h][w][3], variance [h][w] (float32) and variance0 (stage
    B's).  f32: every operation in float32 in the device's order; otherwise float64.  filter_info counts the edges the
    frame met: isolated_valid (valid pixels whose 3x3 neighbourhood holds no other valid pixel: gk == 0.25),
    zero_variance_centre (valid pixels whose pre-filtered variance is 0 in the first iteration: den == 1e-4) and
    far_tap_in_range[step] (the taps other than the centre that are accepted at that step)."""
    ft = np.float32 if f32 else np.float64
    iterations = iterations or ITERATIONS
    sl = ft(np.float32(sigma_luminance or SIGMA_LUMINANCE))
    sn = ft(np.float32(sigma_normal or SIGMA_NORMAL))
    sx = ft(np.float32(sigma_position or aov_ref.default_sigma_position(scene)))
    isn, isx = ft(1) / (sn * sn), ft(1) / (sx * sx)
    valid = A["valid"]
    hits = np.asarray(sums["hits"])
    fh = np.maximum(hits, 1).astype(np.float32)[..., None]
    n = (np.asarray(sums["normal"], np.float32) / fh).astype(np.float32).astype(ft)
    x = (np.asarray(sums["position"], np.float32) / fh).astype(np.float32).astype(ft)
    h, w = valid.shape
    ys, xs = np.arange(h), np.arange(w)
    zero = ft(0)

    def taps(r, s):
        for dy in range(-r, r + 1):
            qy = ys + dy * s
            iny = (qy >= 0) & (qy < h)
            qy = np.clip(qy, 0, h - 1)
            for dx in range(-r, r + 1):
                qx = xs + dx * s
                inx = (qx >= 0) & (qx < w)
                qx = np.clip(qx, 0, w - 1)
                yield dy, dx, qy, qx, iny[:, None] & inx[None, :] & _shift(valid, qy, qx)

    # stage B
    m = A["moments"].astype(ft)
    Ln = A["length"].astype(ft)
    m1, m2 = m[..., 0], m[..., 1]
    temporal = np.maximum(zero, m2 - m1 * m1)
    sw, s1, s2 = np.zeros((h, w), ft), np.zeros((h, w), ft), np.zeros((h, w), ft)
    for dy, dx, qy, qx, ok in taps(3, 1):
        wt = np.where(ok, np.exp(-(_sq3(n, _shift(n, qy, qx)) * isn + _sq3(x, _shift(x, qy, qx)) * isx)), zero).astype(ft)
        sw += wt
        s1 += wt * _shift(m1, qy, qx)
        s2 += wt * _shift(m2, qy, qx)
    with np.errstate(divide="ignore", invalid="ignore"):
        M1, M2 = s1 / sw, s2 / sw
        spatial = np.maximum(zero, M2 - M1 * M1) * (ft(4) / Ln)
    var = np.where(Ln >= ft(LONG_HISTORY), temporal, spatial)
    var = np.where(valid, var, zero).astype(ft)
    variance0 = var.astype(np.float32)

    # stage C
    c = A["accum"].astype(ft)
    color = None
    finfo = dict(isolated_valid=0, zero_variance_centre=0, far_tap_in_range={})
    for it in range(iterations):
        s = 1 << it
        sg, sk = np.zeros((h, w), ft), np.zeros((h, w), ft)
        for dy, dx, qy, qx, ok in taps(1, 1):
            k = ft(G3[dx + 1] * G3[dy + 1])
            sg += np.where(ok, k * _shift(var, qy, qx), zero)
            sk += np.where(ok, k, zero)
        with np.errstate(divide="ignore", invalid="ignore"):
            den = sl * np.sqrt(sg / sk) + ft(1e-4)
        if it == 0:
            finfo.update(isolated_valid=int((valid & (sk == ft(0.25))).sum()), zero_variance_centre=int((valid & (sg == zero)).sum()))
        far = 0
        lp = luminance(c)
        num, nv, sw = np.zeros((h, w, 3), ft), np.zeros((h, w), ft), np.zeros((h, w), ft)
        for dy, dx, qy, qx, ok in taps(2, s):
            cq = _shift(c, qy, qx)
            with np.errstate(over="ignore", invalid="ignore"):
                e = (_sq3(n, _shift(n, qy, qx)) * isn + _sq3(x, _shift(x, qy, qx)) * isx) + np.abs(lp - luminance(cq)) / den
                wt = np.where(ok, ft(H5[dx + 2] * H5[dy + 2]) * np.exp(-e), zero).astype(ft)
            far += int((ok & valid).sum()) if (dy or dx) else 0
            num += wt[..., None] * cq
            nv += (wt * wt) * _shift(var, qy, qx)
            sw += wt
        with np.errstate(divide="ignore", invalid="ignore"):
            c = np.where(valid[..., None], num / sw[..., None], c).astype(ft)
            var = np.where(valid, nv / (sw * sw), var).astype(ft)
        finfo["far_tap_in_range"][s] = far
        if it == 0:
            color = c.astype(np.float32)
    rgb = (c * A["fac"].astype(ft)).astype(np.float32)
    return dict(rgb=rgb, color=color, variance=var.astype(np.float32), variance0=variance0, filter_info=finfo)


def svgf_ref(cur_rgb, sums, cur, prev, iterations=0, max_history=0, alpha_min=0., alpha_min_moments=0., sigma_luminance=0.,
             sigma_normal=0., sigma_position=0., sigma_reproject=0., scene=None, f32=False):
    """rt_svgf: dict of rgb, color, moments, length, accum, variance and info (0 = the defaults; the default sigmas need
    the CURRENT scene)."""
    A = stage_a(cur_rgb, sums, cur, prev, max_history, alpha_min, alpha_min_moments, sigma_reproject, scene)
    out = filter_stages(A, sums, iterations, sigma_luminance, sigma_normal, sigma_position, scene, f32)
    out.update(moments=A["moments"], length=A["length"], accum=A["accum"], info=A["info"])
    return out


def empty_history(width, height):
    """The history the first frame of a sequence passes: length 0 everywhere."""
    z = lambda *s: np.zeros(s, np.float32)
    return dict(color=z(height, width, 3), moments=z(height, width, 2), position=z(height, width, 3),
                mesh=np.full((height, width), 0xffffffff, np.uint32), length=z(height, width))


def next_history(out, cur):
    """The history the next frame reads."""
    return dict(color=out["color"], moments=out["moments"], position=cur["position"], mesh=cur["mesh"], length=out["length"])


# ---- the animated sequence of the GPU test and its tolerance ------------------------------------------------------------
SEQ_SIZES = ((40, 56), (37, 23))  # (the second is not a multiple of 16 either way)
SEQ_SETTINGS = (dict(), dict(max_history=3, alpha_min=0.4, iterations=1),
                dict(max_history=8, alpha_min_moments=0.5, sigma_luminance=1.0, sigma_normal=0.3, iterations=2))
TOLERANCE_FACTOR = 4.0  # the device's expf and square root differ from numpy's float32 ones by a few ulp; same summation order
FILTERED = ("color", "rgb", "variance")
# T_CPU[size][setting]: per filtered output (colour, rgb, variance), the largest absolute difference between the float32
# and the float64 evaluation of stages B and C over the sequence at that size with that setting (measure_tolerance below;
# tests/test_svgf_ref_cpu.py holds the restatement to these figures).  The GPU test allows TOLERANCE_FACTOR times the
# figure of its own size and setting.  measure_tolerance feeds the float64 outputs forward as the history, the GPU test
# the GPU's: the frames, guides and motion are exactly the same, the histories differ by what the tolerance allows, and
# both evaluations of a frame always start from the same history, so T is the rounding of stages B and C on inputs of
# the same kind, not on bit-identical ones.  Largest differences seen on the MI355X over all sizes and settings:
# 1.67e-6, 1.55e-6, 1.34e-5 (40x56: 1.67e-6, 1.55e-6, 6.97e-6; 37x23: 1.19e-6, 5.4e-7, 1.34e-5).
T_CPU = {
    (40, 56): ((9.6e-7, 7.2e-7, 5.8e-6), (9.6e-7, 7.2e-7, 6.1e-6), (1.55e-6, 1.50e-6, 7.1e-6)),
    (37, 23): ((1.32e-6, 4.8e-7, 1.09e-5), (1.32e-6, 4.2e-7, 1.34e-5), (9.6e-7, 5.4e-7, 7.8e-6)),
}


def tolerance(size, setting):
    """T_CPU of SEQ_SETTINGS[setting] at `size`, as a dict over FILTERED."""
    return dict(zip(FILTERED, T_CPU[tuple(size)][setting]))


def sequence_inputs(w, h):
    """The seven-frame sequence of temporal_ref.animated_sequence at w x h, 4 spp, path mode, from the oracle: list of
    dict(frame, scene, params, rgb, sums, cur)."""
    import orc
    import pyrt
    a = pyrt.Scene("lowres", w, h).arrays()
    frames = tr.animated_sequence(a)
    bg = pyrt.background(w, h)
    out = []
    for k, f in enumerate(frames):
        s = tr.scene_of(a, pos=f["pos"], nrm=f["nrm"], camera=f["camera"])
        p = pyrt.make_params(w, h, 4, mode=pyrt.MODE_PATH, seed=f["seed"])
        prev = frames[k - 1] if k else f
        out.append(dict(frame=f, prev=prev, scene=s, params=p, rgb=orc.render(s, p, math_mode=orc.MATH_DET, bg=bg)[0],
                        sums=aov_sums_of(s, p), cur=tr.motion_ref(s, p, prev_pos=prev["pos"], prev_camera=prev["camera"])))
    return out


def aov_sums_of(scene, params):
    return aov_ref.aov_sums(scene, params)


def measure_tolerance(seq, **kw):
    """Per filtered output, max |float32 evaluation - float64 evaluation| over the sequence (the float64 outputs are the
    history fed forward); and the summed branch counts."""
    w, h = seq[0]["rgb"].shape[1], seq[0]["rgb"].shape[0]
    hist, T, seen = empty_history(w, h), dict.fromkeys(FILTERED, 0.0), {}
    skw = {k: v for k, v in kw.items() if k in ("max_history", "alpha_min", "alpha_min_moments", "sigma_reproject")}
    fkw = {k: v for k, v in kw.items() if k not in skw}
    for q in seq:
        A = stage_a(q["rgb"], q["sums"], q["cur"], hist, scene=q["scene"], **skw)
        o64 = filter_stages(A, q["sums"], scene=q["scene"], **fkw)
        o32 = filter_stages(A, q["sums"], scene=q["scene"], f32=True, **fkw)
        for k in FILTERED:
            T[k] = max(T[k], float(np.abs(o32[k].astype(np.float64) - o64[k].astype(np.float64)).max()))
        for k, v in A["info"].items():
            seen[k] = seen.get(k, 0) + v
        o64.update(moments=A["moments"], length=A["length"])
        hist = next_history(o64, q["cur"])
    return T, seen


# the exact comparison edges of the rule, counted by stage_a (EDGES) and by filter_stages (FILTER_EDGES, in filter_info);
# tests/filter_cases.py constructs every one of them
EDGES = tr.EDGES + ("length_exactly_long", "length_just_short")
FILTER_EDGES = ("isolated_valid", "zero_variance_centre", "far_tap_in_range")
BRANCHES = ("miss", "nonfinite", "outside", "no_weight", "tap_mesh", "tap_position", "tap_nolength", "history", "saturated",
            "alpha_bound", "alpha_moments_bound", "invalid", "window", "long_history")
