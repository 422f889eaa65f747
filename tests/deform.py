"""Deformations for the refit / rebuild tests (tests/test_deform_cpu.py, tests/test_gpu_deform.py): a small triangle soup
and an ordered list of poses of it that a rigid turn never reaches — triangles thrown anywhere in the tree, collapsed onto a
plane, a point or signed zeros, scaled across the steps of the derived state, with non-finite vertices nobody references —
and a ray batch aimed at each pose.  numpy only; materials, lights and camera are the `lowres` preset's."""
import numpy as np

import pyrt
from soups import soup_rays
from test_gpu_update import pad_rule, scaled

SIZES = (1, 2, 3, 8, 9, 15, 16, 17, 1024, 1025, 2500)
DEGENERATE = ("point", "origin")  # poses on which nothing can be hit


def scene(n, seed):
    """n triangles over 3 n own vertices (centroids uniform in +-1.2, vertex offsets in +-0.15) and two more vertices that
    no triangle references; two meshes from n = 2 (split at n // 2).  Returns the dict pyrt.ArrayScene takes apart."""
    rng = np.random.default_rng(seed)
    base = pyrt.Scene("lowres", 16, 16).arrays()
    c = rng.uniform(-1.2, 1.2, (n, 1, 3))
    off = rng.uniform(-0.15, 0.15, (n, 3, 3))
    pos = np.concatenate([(c + off).reshape(-1, 3), rng.uniform(-1.0, 1.0, (2, 3))]).astype(np.float32)
    tri = np.arange(3 * n, dtype=np.uint32).reshape(n, 3)
    p = pos[tri].astype(np.float64)
    g = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    nrm = np.concatenate([np.repeat(g, 3, axis=0), [[0, 0, 1], [0, 0, 1]]]).astype(np.float32)
    if n >= 2:
        tri_begin, vtx_begin = [0, n // 2, n], [0, 3 * (n // 2), len(pos)]
    else:
        tri_begin, vtx_begin = [0, n], [0, len(pos)]
    nm = len(tri_begin) - 1
    return dict(pos=pos, nrm=nrm, tri=tri, tri_begin=np.array(tri_begin, np.uint32), vtx_begin=np.array(vtx_begin, np.uint32),
                materials=base["materials"][:nm].copy(), lights=base["lights"].copy(), camera=base["camera"].copy())


def array_scene(a, **kw):
    d = dict(a, **kw)
    return pyrt.ArrayScene(d["pos"], d["nrm"], d["tri"], d["tri_begin"], d["vtx_begin"], d["materials"], d["lights"], d["camera"])


def referenced(a):
    """The vertex ids the triangles reference, ascending."""
    return np.unique(a["tri"])


def pad_ref(a):
    """bvh_build.cpp paddingRule's padRef in float32: max(1, largest referenced |coordinate|, the finite |coordinates| of the
    camera position and the light positions)."""
    pr = max(np.float32(1), np.abs(a["pos"][a["tri"].reshape(-1)]).max())
    for v in list(a["camera"][0]) + list(a["lights"][:, 0:3].reshape(-1)):
        if np.isfinite(v):
            pr = max(pr, np.float32(abs(v)))
    return np.float32(pr)


def box_scale(a):
    """bvh_build.cpp paddingRule's boxScale in float32: 32768 / max(maxAbs + pad, 1e-30) = m 2^e with m in [0.5, 1) (frexp),
    boxScale = 2^clamp(e - 1, -100, 100) (ldexp)."""
    max_abs = np.float32(np.abs(a["pos"][a["tri"].reshape(-1)]).max())
    x = np.float32(32768) / max(np.float32(max_abs + pad_rule(a)), np.float32(1e-30))
    _, e = np.frexp(np.float32(x))
    return np.ldexp(np.float32(1), min(max(int(e) - 1, -100), 100))


def step_factors(a):
    """Two neighbouring float32 factors f0 < f1 about the scale at which maxAbs + pad of the scaled scene passes 2: the
    restated boxScale of scaled(a, f0) is twice that of scaled(a, f1).  Found by bisection on the restatement, which is
    monotone in the factor (every product and sum in it is)."""
    v = np.float32(np.abs(a["pos"][a["tri"].reshape(-1)]).max()) + pad_rule(a)
    mid = np.float32(2.0) / np.float32(v)
    lo, hi = np.float32(mid * np.float32(0.996)), np.float32(mid * np.float32(1.004))
    s_lo, s_hi = box_scale(scaled(a, lo)), box_scale(scaled(a, hi))
    assert s_lo == 2 * s_hi, (s_lo, s_hi)
    while np.nextafter(lo, np.float32(np.inf)) < hi:
        m = np.float32((np.float64(lo) + np.float64(hi)) / 2)
        if box_scale(scaled(a, m)) == s_lo:
            lo = m
        else:
            hi = m
    return lo, hi


def poses(a, seed):
    """The ordered list of (name, dict(pos, nrm, camera, lights)): every pose gives all four, so each one replaces the
    previous whole.  Normals stay the rest pose's."""
    rng = np.random.default_rng(seed)
    ref = referenced(a)
    rest = dict(pos=a["pos"], nrm=a["nrm"], camera=a["camera"], lights=a["lights"])

    def posed(pos=None, src=None):
        b = src if src is not None else a
        return dict(pos=np.ascontiguousarray(pos if pos is not None else b["pos"], np.float32), nrm=a["nrm"], camera=b["camera"],
                    lights=b["lights"])

    out = []
    # every triangle anywhere: the topology means nothing any more
    p = a["pos"].copy()
    p[ref] = a["pos"][rng.permutation(ref)]
    out.append(("shuffle", posed(p)))
    # one axis without extent
    p = a["pos"].copy()
    p[ref, 2] = np.float32(-0.5)
    out.append(("flat", posed(p)))
    # no extent at all, away from zero ...
    p = a["pos"].copy()
    p[ref] = a["pos"][0]
    out.append(("point", posed(p)))
    # ... and at zero, both signs
    p = a["pos"].copy()
    z = np.zeros((len(ref), 3), np.float32)
    z[rng.random(z.shape) < 0.5] = np.float32(-0.0)
    if not np.signbit(z).any():
        z[0, 0] = np.float32(-0.0)
    if np.signbit(z).all():
        z[0, 1] = np.float32(0.0)
    p[ref] = z
    out.append(("origin", posed(p)))
    # the scale: far from 1 both ways, then either side of a step of the plane scale
    out.append(("big", posed(src=scaled(a, 4096.0))))
    out.append(("small", posed(src=scaled(a, 0.125))))
    f0, f1 = step_factors(a)
    out.append(("step_below", posed(src=scaled(a, f0))))
    out.append(("step_at", posed(src=scaled(a, f1))))
    # non-finite vertices that no triangle references
    p = a["pos"].copy()
    p[-2] = np.float32(np.nan)
    p[-1] = np.float32(np.inf)
    out.append(("stray", posed(p)))
    out.append(("rest", rest))
    return out


class _Arrays:
    def __init__(self, a):
        self._a = a

    def arrays(self):
        return self._a


AXES = np.array([[1, 0, 0], [0, -1, 0], [0, 0, 1], [0, 1, 1], [-1, 0, 1]], np.float32)


def rays(a, m, seed):
    """m rays at the pose `a` (the scene dict with the pose's arrays): soups.soup_rays' — origins around the referenced
    geometry, nine in ten aimed at a point inside a random triangle —, the last m // 16 + 1 of them replaced by raybatch's
    axis-parallel directions and one NaN direction.  Every origin lies within 16 padRef, the bound up to which the tree is
    walked, so the stream form (which has no exhaustive fallback beyond it) may take the same rays."""
    pos = a["pos"].copy()
    stray = np.ones(len(pos), bool)
    stray[referenced(a)] = False
    pos[stray] = pos[a["tri"][0, 0]]  # (the unreferenced vertices, NaN on one pose, stay out of the bounds)
    r = soup_rays(_Arrays(dict(a, pos=pos)), m, seed)
    rng = np.random.default_rng(seed + 1)
    lo, hi = pos.min(0), pos.max(0)
    ext = np.maximum(hi - lo, 0.25 * (hi - lo).max() + 1e-3)
    q = m // 16
    r["origin"][m - 1 - q:m - 1] = rng.uniform(lo - ext, hi + ext, (q, 3)).astype(np.float32)
    r["direction"][m - 1 - q:m - 1] = rng.choice(AXES, q)
    r["direction"][m - 1] = np.nan
    assert np.abs(r["origin"]).max() < np.float32(16) * pad_ref(a)
    return r
