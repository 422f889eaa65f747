"""CPU restatements of rt_render_motion and rt_temporal_accumulate (test infrastructure), built like aov_ref.py.

motion_ref: the primary ray of sample spp_begin of every pixel from the oracle's ray dump, its hit from the oracle's
trace; the hit point over the current and over last frame's positions in float32 in the stated order
(w = (1 - u) - v; (w P0 + u P1) + v P2), the two screen positions and their difference in float64 in the stated order.

accumulate_ref: the blend rule of rt_amd.h in float64, tap by tap in the stated order, with a count of every branch the
frame took (what the GPU test asserts its sequence exercises)."""
import numpy as np

import aov_ref
import orc
import pyrt

MISS = aov_ref.MISS
# the defaults of rt_temporal_params (rt_amd.h)
MAX_HISTORY, SIGMA_POSITION_SCALE = 16, 0.02
TAPS = ((0, 0), (1, 0), (0, 1), (1, 1))


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def screen_pos(camera, Y, width, height):
    """(sx, sy, front, lam): the screen position in pixels of the points Y [..][3] (float32) under camera [4][3] (float32),
    float64 in rt_amd.h's order; front = in front of the camera; lam = qn / den (the point is lam times the ray's
    unnormalised direction away)."""
    cam = np.asarray(camera, np.float32).astype(np.float64)
    q = np.asarray(Y, np.float32).astype(np.float64) - cam[0]
    a, H, V = cam[1] - cam[0], cam[2], cam[3]
    a, H, V = (np.broadcast_to(x, q.shape) for x in (a, H, V))
    hv = _cross(H, V)
    qn, den = _dot(q, hv), _dot(a, hv)
    with np.errstate(divide="ignore", invalid="ignore"):
        s, t = _dot(a, _cross(q, V)) / qn, _dot(a, _cross(H, q)) / qn
        lam = qn / den
        return s * float(width), (1.0 - t) * float(height), lam > 0, lam


def motion_ref(scene, params, prev_pos=None, prev_camera=None, accel=orc.ACCEL_LOOP):
    """rt_render_motion for the frame `params` describes on `scene` (the CURRENT frame's scene); prev_pos
    [n_vertices][3] / prev_camera [4][3] last frame's (None = the scene's own).  dict of motion [h][w][2], position,
    prev_position [h][w][3] (float32), mesh [h][w] (uint32); and, for the tests, sx, sy (float64 screen position of the
    hit point under the current camera), hit, and lam_prev (depth factor of X' under the previous camera)."""
    a = scene.arrays()
    s0 = params.spp_begin if params.spp_count else 0
    rays = aov_ref.primary_rays(scene, aov_ref._copy_params(params, spp_begin=s0, spp_count=1))[:, :, 0]
    h, w = rays.shape
    hits = orc.trace(scene, rays.reshape(-1), accel=accel).reshape(h, w)
    hit = hits["hit"] != 0
    mesh = np.where(hit, hits["mesh"], 0).astype(np.int64)
    gid = a["tri_begin"][mesh].astype(np.int64) + np.where(hit, hits["tri"], 0)
    tv = a["tri"][gid].astype(np.int64)
    u, v = hits["u"][..., None], hits["v"][..., None]
    wgt = (np.float32(1) - u) - v
    ppos = a["pos"] if prev_pos is None else np.ascontiguousarray(prev_pos, np.float32).reshape(-1, 3)
    pcam = a["camera"] if prev_camera is None else np.ascontiguousarray(prev_camera, np.float32).reshape(4, 3)

    def interp(pos):
        p0, p1, p2 = (pos[tv[..., k]] for k in range(3))
        return ((wgt * p0 + u * p1) + v * p2).astype(np.float32)
    X, Xp = interp(a["pos"]), interp(ppos)
    cx, cy, fc, _ = screen_pos(a["camera"], X, w, h)
    qx, qy, fp, lam = screen_pos(pcam, Xp, w, h)
    ok = fc & fp & np.isfinite(cx) & np.isfinite(cy) & np.isfinite(qx) & np.isfinite(qy)
    with np.errstate(invalid="ignore", over="ignore"):
        m = np.stack([(qx - cx).astype(np.float32), (qy - cy).astype(np.float32)], axis=-1)
    m = np.where(ok[..., None], m, np.float32(np.inf))
    z3 = np.zeros((h, w, 3), np.float32)
    return dict(motion=np.where(hit[..., None], m, np.float32(0)).astype(np.float32),
                position=np.where(hit[..., None], X, z3), prev_position=np.where(hit[..., None], Xp, z3),
                mesh=np.where(hit, hits["mesh"], MISS).astype(np.uint32), sx=cx, sy=cy, hit=hit, lam_prev=lam)


def default_sigma_position(scene):
    """SIGMA_POSITION_SCALE of the diagonal of the bounding box of the vertices the triangles reference (float32)."""
    a = scene.arrays()
    p = a["pos"][a["tri"].reshape(-1)]
    d = (p.max(axis=0) - p.min(axis=0)).astype(np.float32)
    return np.float32(SIGMA_POSITION_SCALE) * np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])


# the exact comparison edges of the reprojection (rt_svgf's stage A counts the same ones)
EDGES = ("rx_minus_one", "last_column_tap_outside", "single_tap", "position_on_sigma")


def edge_counts(cand, rx, x0, ax, ay, w):
    """Counts of the reprojected pixels on the rule's edges: rx == -1 (the tap of weight 1 lies outside: no weight),
    x0 == w - 1 with a fraction (the right-hand taps lie outside, rx == nextafter(w, 0) among them), and a whole-pixel
    position (one tap of weight 1, rx == w - 1 among them); position_on_sigma counts the taps at d^2 == sigma^2."""
    return dict(rx_minus_one=int((cand & (rx == -1.0)).sum()), last_column_tap_outside=int((cand & (x0 == w - 1) & (ax > 0)).sum()),
                single_tap=int((cand & (ax == 0) & (ay == 0)).sum()), position_on_sigma=0)


def accumulate_ref(cur_rgb, cur, prev, max_history=0, alpha_min=0., sigma_position=0., scene=None):
    """rt_temporal_accumulate: (out_rgb [h][w][3], out_length [h][w], info).  cur: motion, prev_position, mesh; prev: rgb,
    position, mesh, length; 0 = the defaults (the default sigma_position needs the CURRENT scene).  info counts the
    pixels / taps of every branch."""
    maxh = float(max_history or MAX_HISTORY)
    amin = float(np.float32(alpha_min))
    sig = float(np.float32(sigma_position) if sigma_position else default_sigma_position(scene))
    s2 = sig * sig
    c = np.asarray(cur_rgb, np.float32).astype(np.float64)
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
    W, SL, S = np.zeros((h, w)), np.zeros((h, w)), np.zeros((h, w, 3))
    info = dict(miss=int(miss.sum()), nonfinite=int(nonfinite.sum()), outside=int(outside.sum()), tap_mesh=0, tap_position=0,
                tap_nolength=0)
    info.update(edge_counts(cand, rx, x0, ax, ay, w))
    hrgb, hpos = np.asarray(prev["rgb"], np.float32), np.asarray(prev["position"], np.float32)
    hmesh, hlen = np.asarray(prev["mesh"], np.uint32), np.asarray(prev["length"], np.float32)
    for i, j in TAPS:
        wt = wxs[i] * wys[j]
        x, y = x0 + i, y0 + j
        base = cand & (wt > 0) & (x >= 0) & (x < w) & (y >= 0) & (y < h)
        xc, yc = np.clip(x, 0, w - 1), np.clip(y, 0, h - 1)
        tl = hlen[yc, xc]
        with np.errstate(invalid="ignore"):
            haslen = tl > 0
        meshok = hmesh[yc, xc] == mesh
        d = hpos[yc, xc].astype(np.float64) - X
        with np.errstate(invalid="ignore", over="ignore"):
            d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
            posok = d2 <= s2
        ok = base & haslen & meshok & posok
        info["position_on_sigma"] += int((ok & (d2 == s2)).sum())
        info["tap_nolength"] += int((base & ~haslen).sum())
        info["tap_mesh"] += int((base & haslen & ~meshok).sum())
        info["tap_position"] += int((base & haslen & meshok & ~posok).sum())
        W = np.where(ok, W + wt, W)
        S = np.where(ok[..., None], S + wt[..., None] * hrgb[yc, xc].astype(np.float64), S)
        SL = np.where(ok, SL + wt * tl.astype(np.float64), SL)
    hist = cand & (W > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        hh, L = S / W[..., None], SL / W
        Ln = np.minimum(L + 1.0, maxh)
        alpha = np.maximum(1.0 / Ln, amin)
        out = np.where(hist[..., None], hh + alpha[..., None] * (c - hh), c).astype(np.float32)
        length = np.where(hist, Ln, 1.0).astype(np.float32)
        info.update(no_weight=int((cand & ~hist).sum()), history=int(hist.sum()), saturated=int((hist & (L + 1.0 > maxh)).sum()),
                    alpha_bound=int((hist & (amin > 1.0 / Ln)).sum()))
    return out, length, info


def next_history(out_rgb, out_length, cur):
    """The history the next frame reads."""
    return dict(rgb=out_rgb, position=cur["position"], mesh=cur["mesh"], length=out_length)


# ---- the animated scenes of the tests -------------------------------------------------------------------------------
def turned(a, deg, slot=3):
    """Positions and normals with mesh `slot` turned about the y axis by `deg` degrees (tests/test_gpu_update.py's)."""
    phi = np.float32(np.deg2rad(deg))
    c, s = np.cos(phi, dtype=np.float32), np.sin(phi, dtype=np.float32)
    R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], np.float32)
    b, e = a["vtx_begin"][slot], a["vtx_begin"][slot + 1]
    pos, nrm = a["pos"].copy(), a["nrm"].copy()
    pos[b:e] = (pos[b:e] @ R.T).astype(np.float32)
    nrm[b:e] = (nrm[b:e] @ R.T).astype(np.float32)
    return pos, nrm


def scene_of(a, **kw):
    """An ArrayScene of the arrays a with some replaced."""
    d = dict(a)
    d.update(kw)
    return pyrt.ArrayScene(d["pos"], d["nrm"], d["tri"], d["tri_begin"], d["vtx_begin"], d["materials"], d["lights"], d["camera"])


def moved_camera(cam, delta):
    """The camera translated by delta (its position and the lower left corner of its image plane)."""
    c = np.array(cam, np.float32)
    c[0] += np.asarray(delta, np.float32)
    c[1] += np.asarray(delta, np.float32)
    return c


def panned_camera(cam, f):
    """The camera looking f image widths to the side (f = 1.5 looks past the preset room's wall: some rays miss)."""
    c = np.array(cam, np.float32)
    c[1] += np.float32(f) * c[2]
    return c


def animated_sequence(a, n=7):
    """The animated sequence of the accumulation tests over the preset arrays a: frame k has slot 3 turned by 5 k degrees
    and its own camera and seed — a small move, a pan past the room's wall (misses; most of the history leaves the image),
    a jump into the room (so that in the next frame, seen from outside again, points lie behind the previous camera),
    then small moves.  List of dict(pos, nrm, camera, seed)."""
    cam = a["camera"]
    cams = [cam, moved_camera(cam, (0.05, 0.0, 0.0)), panned_camera(cam, 2.5), moved_camera(cam, (0.0, 0.0, -3.0)), cam,
            moved_camera(cam, (0.04, 0.02, 0.0)), moved_camera(cam, (0.08, 0.04, 0.0)), moved_camera(cam, (0.1, 0.05, 0.02))]
    frames = []
    for k in range(n):
        pos, nrm = turned(a, 5.0 * k) if k else (a["pos"], a["nrm"])
        frames.append(dict(pos=pos, nrm=nrm, camera=cams[k % len(cams)], seed=20 + k))
    return frames


def run_sequence_ref(a, frames, rgbs, params_of, accel=orc.ACCEL_LOOP, **kw):
    """The sequence through motion_ref and accumulate_ref, the history fed forward: list of (cur, out_rgb, out_length,
    info) per frame.  rgbs: the frames' images; params_of(k): frame k's rt_params."""
    h, w = rgbs[0].shape[:2]
    hist, out = pyrt.empty_history(w, h), []
    for k, f in enumerate(frames):
        s = scene_of(a, pos=f["pos"], nrm=f["nrm"], camera=f["camera"])
        prev = frames[k - 1] if k else f
        cur = motion_ref(s, params_of(k), prev_pos=prev["pos"], prev_camera=prev["camera"], accel=accel)
        o, l, info = accumulate_ref(rgbs[k], cur, hist, scene=s, **kw)
        out.append((cur, o, l, info))
        hist = next_history(o, l, cur)
    return out
