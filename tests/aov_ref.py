"""CPU restatements of rt_render_aov and rt_denoise (test infrastructure).

aov_sums: the frame's primary rays are the tag-0 rows of the oracle's ray dump (pixel-major, in sample order), their hits
come from the oracle's trace; the shading normal and the hit point are Renderer.cpp:42-43 on the hit's (u, v) in float32
in the reference's operation order, and every sum is a float32 add in sample order.

atrous: the edge-avoiding a-trous filter exactly as DESIGN.md "AOVs and the a-trous denoiser" defines it, in numpy."""
import ctypes as C

import numpy as np

import orc
import pyrt

MISS = np.uint32(0xffffffff)
H5 = (1.0 / 16, 1.0 / 4, 3.0 / 8, 1.0 / 4, 1.0 / 16)
# the defaults of rt_denoise_params (rt_amd.h)
ITERATIONS, SIGMA_COLOR, SIGMA_NORMAL, SIGMA_POSITION_SCALE = 5, 2.0, 0.5, 0.02


def _copy_params(params, **kw):
    q = pyrt.Params()
    C.memmove(C.byref(q), C.byref(params), C.sizeof(pyrt.Params))
    for k, v in kw.items():
        setattr(q, k, v)
    return q


def primary_rays(scene, params):
    """The frame's primary rays [h][w][samples] (RAY_DTYPE), from the oracle's ray dump of a ray-mode frame of the same
    stream key, size and sample range."""
    q = _copy_params(params, mode=pyrt.MODE_RAY, max_depth=1, use_photons=0, k=0, photons_requested=0)
    d = orc.dump_rays(scene, q)
    tag = np.ascontiguousarray(d[:, 3]).view(np.uint32)
    prim = d[tag == 0]
    ns = params.spp_count if params.spp_count else params.spp
    w, h = params.width, params.height
    assert len(prim) == w * h * ns, (len(prim), w, h, ns)
    rays = np.zeros(len(prim), pyrt.RAY_DTYPE)
    rays["origin"], rays["direction"] = prim[:, 0:3], prim[:, 4:7]
    return rays.reshape(h, w, ns)


def _unit(a):
    """Vec3.h:170-178 in float32: null vectors stay null, otherwise times 1 / length."""
    x, y, z = a[..., 0], a[..., 1], a[..., 2]
    ln = np.sqrt((x * x + y * y) + z * z)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = np.float32(1) / ln
        r = a * inv[..., None]
    return np.where((ln == 0)[..., None], a, r).astype(np.float32)


def aov_sums(scene, params, accel=orc.ACCEL_LOOP, rays=None):
    """rt_render_aov's sums for the frame `params` describes: dict of albedo, normal, position [h][w][3] float32, depth
    [h][w] float32, hits, mesh, tri [h][w] uint32."""
    a = scene.arrays()
    if rays is None:
        rays = primary_rays(scene, params)
    h, w, ns = rays.shape
    hits = orc.trace(scene, rays.reshape(-1), accel=accel).reshape(h, w, ns)
    hit = hits["hit"] != 0
    mesh = np.where(hit, hits["mesh"], 0).astype(np.int64)
    gid = a["tri_begin"][mesh].astype(np.int64) + np.where(hit, hits["tri"], 0)
    tv = a["tri"][gid].astype(np.int64)  # global vertex ids
    u, v = hits["u"][..., None], hits["v"][..., None]
    wgt = (np.float32(1) - u) - v
    p0, p1, p2 = (a["pos"][tv[..., k]] for k in range(3))
    n0, n1, n2 = (a["nrm"][tv[..., k]] for k in range(3))
    nrm = _unit((wgt * n0 + u * n1) + v * n2)
    pt = ((wgt * p0 + u * p1) + v * p2).astype(np.float32)
    alb = a["materials"][mesh][..., 2:5]
    out = dict(albedo=np.zeros((h, w, 3), np.float32), normal=np.zeros((h, w, 3), np.float32),
               position=np.zeros((h, w, 3), np.float32), depth=np.zeros((h, w), np.float32))
    for s in range(ns):  # float32 adds in sample order; a miss adds nothing
        m = hit[:, :, s]
        for k, val in (("albedo", alb), ("normal", nrm), ("position", pt)):
            out[k] = np.where(m[..., None], out[k] + val[:, :, s], out[k]).astype(np.float32)
        out["depth"] = np.where(m, out["depth"] + hits["d"][:, :, s], out["depth"]).astype(np.float32)
    out["hits"] = hit.sum(axis=2).astype(np.uint32)
    out["mesh"] = np.where(hit[:, :, 0], hits["mesh"][:, :, 0], MISS).astype(np.uint32)
    out["tri"] = np.where(hit[:, :, 0], hits["tri"][:, :, 0], MISS).astype(np.uint32)
    return out


def default_sigma_position(scene):
    """2 % of the diagonal of the bounding box of the vertices the triangles reference (float32)."""
    a = scene.arrays()
    p = a["pos"][a["tri"].reshape(-1)]
    d = (p.max(axis=0) - p.min(axis=0)).astype(np.float32)
    return float(np.float32(SIGMA_POSITION_SCALE) * np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))


def _sq3(a, b):
    d = a - b
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def _atrous_f32(rgb, sums, iterations, sigma_color, sigma_normal, sigma_position):
    """atrous with every operation in float32 in k_dn_iter's order: the taps row by row, the three terms of the exponent
    summed left to right, one exp per tap, the sums running in tap order."""
    f = np.float32
    rgb = np.asarray(rgb, f)
    hits = np.asarray(sums["hits"])
    valid = hits > 0
    fh = np.maximum(hits, 1).astype(f)[..., None]
    n = (np.asarray(sums["normal"], f) / fh).astype(f)
    x = (np.asarray(sums["position"], f) / fh).astype(f)
    fac = np.maximum(np.asarray(sums["albedo"], f) / fh, f(1e-3)).astype(f)
    c = np.where(valid[..., None], rgb / fac, rgb).astype(f)
    h, w = hits.shape
    ys, xs = np.arange(h), np.arange(w)
    isn, isx = f(1) / (f(sigma_normal) * f(sigma_normal)), f(1) / (f(sigma_position) * f(sigma_position))
    for i in range(iterations):
        s = 1 << i
        sc = f(sigma_color) * f(2.0 ** -i)
        isc = f(1) / (sc * sc)
        num, den = np.zeros((h, w, 3), f), np.zeros((h, w), f)
        for dy in range(-2, 3):
            qy = ys + dy * s
            iny = (qy >= 0) & (qy < h)
            qy = np.clip(qy, 0, h - 1)
            for dx in range(-2, 3):
                qx = xs + dx * s
                inx = (qx >= 0) & (qx < w)
                qx = np.clip(qx, 0, w - 1)
                ok = iny[:, None] & inx[None, :] & valid[qy][:, qx]
                cq = c[qy][:, qx]
                with np.errstate(over="ignore", invalid="ignore"):
                    e = (_sq3(c, cq) * isc + _sq3(n, n[qy][:, qx]) * isn) + _sq3(x, x[qy][:, qx]) * isx
                    wt = np.where(ok, (f(H5[dx + 2]) * f(H5[dy + 2])) * np.exp(-e), f(0)).astype(f)
                num += wt[..., None] * cq
                den += wt
        with np.errstate(divide="ignore", invalid="ignore"):
            c = np.where(valid[..., None], num / den[..., None], c).astype(f)
    return np.where(valid[..., None], c * fac, rgb).astype(f)


def atrous(rgb, sums, iterations=0, sigma_color=0., sigma_normal=0., sigma_position=0., scene=None, f32=False):
    """The filter of rt_denoise on a resolved frame rgb [h][w][3] and rt_render_aov's sums (0 = the defaults; the default
    sigma_position needs the scene).  f32: every operation in float32 in k_dn_iter's order, the exponent summed as the
    kernel sums it, with one exp; otherwise float64 with the three exponentials apart."""
    iterations = iterations or ITERATIONS
    if f32:
        return _atrous_f32(rgb, sums, iterations, sigma_color or SIGMA_COLOR, sigma_normal or SIGMA_NORMAL,
                           sigma_position or default_sigma_position(scene))
    sc, sn = sigma_color or SIGMA_COLOR, sigma_normal or SIGMA_NORMAL
    sx = sigma_position or default_sigma_position(scene)
    rgb = np.asarray(rgb, np.float32)
    hits = np.asarray(sums["hits"])
    valid = hits > 0
    fh = np.maximum(hits, 1).astype(np.float32)[..., None]
    a = sums["albedo"] / fh
    n = (sums["normal"] / fh).astype(np.float64)
    x = (sums["position"] / fh).astype(np.float64)
    fac = np.maximum(a, np.float32(1e-3)).astype(np.float32)
    c = np.where(valid[..., None], rgb / fac, rgb).astype(np.float32)
    h, w = hits.shape
    ys, xs = np.arange(h), np.arange(w)
    for i in range(iterations):
        s = 1 << i
        sci = sc * 2.0 ** -i
        cd = c.astype(np.float64)
        num = np.zeros((h, w, 3))
        den = np.zeros((h, w))
        for dy in range(-2, 3):
            qy = ys + dy * s
            iny = (qy >= 0) & (qy < h)
            qy = np.clip(qy, 0, h - 1)
            for dx in range(-2, 3):
                qx = xs + dx * s
                inx = (qx >= 0) & (qx < w)
                qx = np.clip(qx, 0, w - 1)
                ok = iny[:, None] & inx[None, :] & valid[qy][:, qx]
                cq, nq, xq = cd[qy][:, qx], n[qy][:, qx], x[qy][:, qx]
                wt = (H5[dx + 2] * H5[dy + 2] * np.exp(-((cd - cq) ** 2).sum(-1) / sci ** 2)
                      * np.exp(-((n - nq) ** 2).sum(-1) / sn ** 2) * np.exp(-((x - xq) ** 2).sum(-1) / sx ** 2))
                wt = np.where(ok, wt, 0.0)
                num += wt[..., None] * cq
                den += wt
        with np.errstate(divide="ignore", invalid="ignore"):
            c = np.where(valid[..., None], num / den[..., None], c).astype(np.float32)
    return np.where(valid[..., None], c * fac, rgb).astype(np.float32)


def mse(a, b):
    return float(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2))
