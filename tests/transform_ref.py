"""rt_update_transforms in numpy: the header's per-vertex expression spelt out column by column in float32 — no `@`, no
einsum (BLAS may fuse or reorder) — over the rest arrays of a scene description."""
import numpy as np

import pyrt


def rotation_y(deg):
    """ScenePresets rotationY's matrix (as test_gpu_update.turned builds it)."""
    phi = np.float32(np.deg2rad(deg))
    c, s = np.cos(phi, dtype=np.float32), np.sin(phi, dtype=np.float32)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], np.float32)


def set_mesh(t, j, R=None, translate=(0, 0, 0), normal=None):
    """Mesh j of t (pyrt.make_transforms) moves: m = (R | translate), n = `normal` (None = R)."""
    R = np.eye(3, dtype=np.float32) if R is None else np.asarray(R, np.float32)
    t["m"][j, :, :3], t["m"][j, :, 3] = R, np.asarray(translate, np.float32)
    t["n"][j] = R if normal is None else np.asarray(normal, np.float32)
    t["flags"][j] = 0
    return t


def apply(a, transforms):
    """(pos, nrm) of the arrays a["pos"], a["nrm"] (meshes by a["vtx_begin"]) under `transforms`:
    X'_i = ((m[i][0] x + m[i][1] y) + m[i][2] z) + m[i][3], N'_i = (n[i][0] a + n[i][1] b) + n[i][2] c, every product and
    sum rounded to float32; XF_STATIC meshes are copied."""
    pos, nrm = np.array(a["pos"], np.float32), np.array(a["nrm"], np.float32)
    rest_p, rest_n = pos.copy(), nrm.copy()
    assert len(transforms) == len(a["vtx_begin"]) - 1
    with np.errstate(over="ignore", invalid="ignore"):
        for j, t in enumerate(transforms):
            if t["flags"] & pyrt.XF_STATIC:
                continue
            b, e = int(a["vtx_begin"][j]), int(a["vtx_begin"][j + 1])
            m, n = t["m"].astype(np.float32), t["n"].astype(np.float32)
            x, y, z = rest_p[b:e, 0], rest_p[b:e, 1], rest_p[b:e, 2]
            u, v, w = rest_n[b:e, 0], rest_n[b:e, 1], rest_n[b:e, 2]
            for i in range(3):
                pos[b:e, i] = ((m[i, 0] * x + m[i, 1] * y) + m[i, 2] * z) + m[i, 3]
                nrm[b:e, i] = (n[i, 0] * u + n[i, 1] * v) + n[i, 2] * w
    assert pos.dtype == np.float32 and nrm.dtype == np.float32
    return pos, nrm
