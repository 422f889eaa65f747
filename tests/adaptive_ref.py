"""numpy restatement of rt_render_adaptive (include/rt_amd.h, DESIGN.md "Adaptive sampling"): the retirement rule over a
chain of pass accumulators, and the resolve with per-pixel sample counts.

A granule that is active in pass k has run passes 0..k, so its accumulator after pass k is the chain's k-th entry
(rt_render_passes with seed + j, j = 0..k, on a zero accumulator).  The rule is float64 in the order the header writes
it; numpy does not contract, so the bits are the device's."""
import numpy as np

DEFAULT_MIN_PASSES = 4
DEFAULT_FLOOR = 0.01


def granule_grid(w, h):
    return (w + 7) // 8, (h + 7) // 8


def per_pixel(gran, w, h):
    """[gy][gx] -> [h][w]: the value of each pixel's 8x8 granule."""
    return np.repeat(np.repeat(gran, 8, axis=0), 8, axis=1)[:h, :w]


def run_rule(chain, bg, P, threshold, max_passes, min_passes=0, floor=0.):
    """chain[k]: float32 [h][w][4] accumulator after passes 0..k (at least max_passes entries).  Returns (K [gy][gx]
    passes per granule, active: granules rendered by each pass run)."""
    h, w = chain[0].shape[:2]
    gx, gy = granule_grid(w, h)
    minp = min_passes if min_passes else min(DEFAULT_MIN_PASSES, max_passes)
    minp = max(minp, 2)
    thr = np.float64(np.float32(threshold))
    fl = np.float64(np.float32(floor if floor else DEFAULT_FLOOR))
    bg = np.asarray(bg, np.float32).astype(np.float64)
    prev = np.zeros((h, w, 4), np.float32)
    s1 = np.zeros((h, w), np.float64)
    s2 = np.zeros((h, w), np.float64)
    K = np.zeros((gy, gx), np.int64)
    retired = np.zeros((gy, gx), bool)
    active = []
    Pd = np.float64(P)
    for k in range(max_passes):
        act = ~retired
        if not act.any():
            break
        active.append(int(act.sum()))
        K[act] += 1
        m = per_pixel(act, w, h)
        d = (chain[k] - prev).astype(np.float32)
        prev = np.where(m[..., None], chain[k], prev)
        dd = d.astype(np.float64)
        miss = Pd - dd[..., 3]
        y = (0.2126 * (dd[..., 0] + bg[..., 0] * miss) + 0.7152 * (dd[..., 1] + bg[..., 1] * miss)
             + 0.0722 * (dd[..., 2] + bg[..., 2] * miss)) / Pd
        s1 = np.where(m, s1 + y, s1)
        s2 = np.where(m, s2 + y * y, s2)
        Kp = per_pixel(K, w, h).astype(np.float64)
        if thr > 0:
            with np.errstate(divide="ignore", invalid="ignore"):
                mean = s1 / Kp
                v = (s2 - s1 * mean) / (Kp - 1.0)
                v = np.where(v < 0.0, 0.0, v)
                lim = thr * (mean + fl)
                conv = (v / Kp <= lim * lim) & (Kp >= minp)
        else:
            conv = np.zeros((h, w), bool)
        # a granule retires when all its in-image pixels converged (pad with True outside the image)
        full = np.ones((gy * 8, gx * 8), bool)
        full[:h, :w] = conv
        gconv = full.reshape(gy, 8, gx, 8).all(axis=(1, 3))
        retired |= act & gconv
    return K, active


def resolve(accum, bg, spp):
    """k_resolve in float32 with a per-pixel spp ([h][w] integers)."""
    a = np.asarray(accum, np.float32)
    bg = np.asarray(bg, np.float32)
    sppf = np.asarray(spp).astype(np.float32)
    miss = (sppf.astype(np.int64) - a[..., 3].astype(np.int64)).astype(np.float32)
    out = a[..., :3] / sppf[..., None] + bg * miss[..., None] / sppf[..., None]
    return out.astype(np.float32)


def assemble(chain, K, w, h):
    """The accumulator an adaptive frame leaves: chain[K - 1] per granule."""
    Kp = per_pixel(K, w, h)
    out = np.zeros_like(chain[0])
    for k in np.unique(Kp):
        sel = Kp == k
        out[sel] = chain[k - 1][sel]
    return out
