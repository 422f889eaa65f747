"""rt_update_skin in numpy: the header's per-vertex blend spelt out column by column in float32 — no `@`, no einsum (BLAS
may fuse or reorder) — over the rest arrays of a scene description, the rigs the skinning tests pose, and the table of
cases that tests/test_gpu_skin.py runs on the device and tests/test_skin_ref_cpu.py vets on this restatement first."""
import numpy as np

import pyrt

SLOTS = 4


def apply(a, bone, weight, bones):
    """(pos, nrm) of the arrays a["pos"], a["nrm"] under the skin (bone [n][4] indices, weight [n][4]) and the records
    `bones` (make_transforms' layout): X' = N' = +0, then for every slot k in slot order whose weight is not zero
    P_i = ((m[i][0] x + m[i][1] y) + m[i][2] z) + m[i][3], Q_i = (n[i][0] a + n[i][1] b) + n[i][2] c, X'_i = X'_i + (w P_i),
    N'_i = N'_i + (w Q_i), every product and sum rounded to float32; a vertex of four zero weights is copied."""
    rest_p, rest_n = np.array(a["pos"], np.float32), np.array(a["nrm"], np.float32)
    bone, weight = np.asarray(bone), np.asarray(weight, np.float32)
    assert bone.shape == weight.shape == (len(rest_p), SLOTS) and bone.max() < len(bones)
    M, N = np.asarray(bones["m"], np.float32), np.asarray(bones["n"], np.float32)
    X, Y = np.zeros_like(rest_p), np.zeros_like(rest_n)
    with np.errstate(over="ignore", invalid="ignore"):
        for k in range(SLOTS):
            on = weight[:, k] != 0  # (-0.0 != 0 is False: a zero of either sign is skipped)
            w, m, n = weight[on, k], M[bone[on, k]], N[bone[on, k]]
            x, y, z = rest_p[on, 0], rest_p[on, 1], rest_p[on, 2]
            u, v, t = rest_n[on, 0], rest_n[on, 1], rest_n[on, 2]
            for i in range(3):
                p = ((m[:, i, 0] * x + m[:, i, 1] * y) + m[:, i, 2] * z) + m[:, i, 3]
                q = (n[:, i, 0] * u + n[:, i, 1] * v) + n[:, i, 2] * t
                X[on, i] = X[on, i] + (w * p)
                Y[on, i] = Y[on, i] + (w * q)
    skinned = (weight != 0).any(axis=1)
    pos, nrm = rest_p.copy(), rest_n.copy()
    pos[skinned], nrm[skinned] = X[skinned], Y[skinned]
    assert pos.dtype == np.float32 and nrm.dtype == np.float32
    return pos, nrm


def skinned_rows(weight):
    return (np.asarray(weight) != 0).any(axis=1)


def rotation_records(deg, scale=None, translate=None, normal_deg=None):
    """One record per entry of `deg`: m = (scale rotationY(deg) | translate), n = rotationY(normal_deg, default deg);
    flags 0."""
    deg = np.asarray(deg, np.float64)
    t = pyrt.make_transforms(len(deg))
    t["flags"] = 0

    def fill(dst, d, s):
        phi = np.deg2rad(d).astype(np.float32)
        c, sn = np.cos(phi, dtype=np.float32) * s, np.sin(phi, dtype=np.float32) * s
        dst[:, 0, 0], dst[:, 0, 2], dst[:, 2, 0], dst[:, 2, 2], dst[:, 1, 1] = c, sn, -sn, c, s
    fill(t["m"], deg, np.float32(1) if scale is None else np.asarray(scale, np.float32))
    fill(t["n"], deg if normal_deg is None else np.asarray(normal_deg, np.float64), np.float32(1))
    if translate is not None:
        t["m"][:, :, 3] = np.asarray(translate, np.float32)
    return t


# ---- the bend: bones stacked along y --------------------------------------------------------------------------------
BEND_BONES = 4
BEND_SLOTS = (3, 4)  # the two objects of the preset scenes; the walls keep four zero weights


def bend_skin(a, n_bones=BEND_BONES, meshes=BEND_SLOTS):
    """(bone, weight): the vertices of `meshes` hang on the two bones nearest to their height — bone j0 in slot 0 with
    1 - w and j0 + 1 in slot 1 with w = 0.15 + 0.7 f, f the fraction of the way up from j0 — the rest on none."""
    nv = len(a["pos"])
    bone, weight = np.zeros((nv, SLOTS), np.uint16), np.zeros((nv, SLOTS), np.float32)
    rows = np.concatenate([np.arange(a["vtx_begin"][m], a["vtx_begin"][m + 1]) for m in meshes]).astype(np.int64)
    y = a["pos"][rows, 1].astype(np.float64)
    t = (y - y.min()) / (y.max() - y.min()) * (n_bones - 1)
    j0 = np.minimum(np.floor(t), n_bones - 2)
    w1 = (0.15 + 0.7 * (t - j0)).astype(np.float32)
    bone[rows, 0], bone[rows, 1] = j0, j0 + 1
    weight[rows, 0], weight[rows, 1] = np.float32(1) - w1, w1
    assert (weight[rows, :2] > 0.1).all() and (weight[rows, :2] < 0.9).all()
    return bone, weight


def bend_bones(deg, n_bones=BEND_BONES):
    """Bone j turned about y by (j + 1) deg and moved by (j + 1) (0.01, 0.015, -0.01)."""
    j = np.arange(1, n_bones + 1)
    return rotation_records(j * float(deg), translate=j[:, None] * np.array([0.01, 0.015, -0.01]))


# ---- the random rig ---------------------------------------------------------------------------------------------------
def random_skin(nv, n_bones, seed):
    """(bone, weight): every vertex 0 to 4 non-zero slots anywhere among its four (so (w, 0, w, 0) occurs), weights in
    (0.1, 0.9) — half of the one-slot vertices exactly 1 —, about half of the zeros -0.0, indices over the whole table
    under zero and non-zero weights alike, and the last index on a non-zero slot of the first skinned vertex."""
    rng = np.random.default_rng(seed)
    count = rng.integers(0, SLOTS + 1, nv)
    count[:min(nv, 5)] = np.arange(5)[:min(nv, 5)][::-1]  # (every count occurs in the smallest scene too)
    on = rng.permuted(np.arange(SLOTS)[None, :] < count[:, None], axis=1)
    weight = np.where(on, rng.uniform(0.1, 0.9, (nv, SLOTS)), 0.0).astype(np.float32)
    ones = (count == 1) & (rng.random(nv) < 0.5)
    weight[ones[:, None] & on] = 1.0
    weight[~on & (rng.random((nv, SLOTS)) < 0.5)] = np.float32(-0.0)
    bone = rng.integers(0, n_bones, (nv, SLOTS)).astype(np.uint16)
    first = int(np.flatnonzero(count > 0)[0])
    bone[first, int(np.flatnonzero(on[first])[0])] = n_bones - 1
    return bone, weight


def random_bones(n_bones, seed):
    """Every bone its own rotation about y, scale in (0.8, 1.1), small translation and normal matrix."""
    rng = np.random.default_rng(seed)
    return rotation_records(rng.uniform(-180, 180, n_bones), scale=rng.uniform(0.8, 1.1, n_bones),
                            translate=rng.uniform(-0.05, 0.05, (n_bones, 3)), normal_deg=rng.uniform(-180, 180, n_bones))


# ---- scenes of small meshes (the construction of test_gpu_transforms.triangle_meshes) ---------------------------------
def triangle_meshes(counts, seed):
    """A scene of len(counts) meshes inside the lowres room's walls: mesh j has counts[j] vertices and counts[j] - 2
    triangles over consecutive vertices, scattered in a slab facing the camera; some coordinates are -0."""
    base = pyrt.Scene("lowres", 24, 24).arrays()
    rng = np.random.default_rng(seed)
    nv = int(np.sum(counts))
    vb = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    centre = np.repeat(np.stack([rng.uniform(-1.2, 1.2, len(counts)), rng.uniform(-0.8, 1.2, len(counts)),
                                 rng.uniform(-1.2, 0.4, len(counts))], 1), counts, axis=0)
    pos = (centre + rng.uniform(-0.12, 0.12, (nv, 3))).astype(np.float32)
    nrm = rng.normal(size=(nv, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    pos[rng.integers(0, nv, 7), rng.integers(0, 3, 7)] = np.float32(-0.0)
    tri = np.concatenate([np.arange(c - 2)[:, None] + np.arange(3)[None, :] + vb[j] for j, c in enumerate(counts)]).astype(np.uint32)
    tb = np.concatenate([[0], np.cumsum(np.asarray(counts) - 2)]).astype(np.uint32)
    mats = base["materials"][np.arange(len(counts)) % len(base["materials"])]
    return dict(pos=pos, nrm=nrm, tri=tri, tri_begin=tb, vtx_begin=vb, materials=mats, lights=base["lights"], camera=base["camera"])


# ---- the cases of tests/test_gpu_skin.py --------------------------------------------------------------------------------
BEND_DEGS = (10.0, 30.0, 60.0)
BEND_KINDS = ("lowres", "hires")
# (vertex counts of the scene's meshes, n_bones): one mesh per wave / tile edge, then all edges in one scene under the
# smallest and the largest table
BOUNDARY = [([3], 1), ([63], 2), ([64], 65), ([65], 2), ([255], 65), ([256], 1), ([257], 65), ([513], 65536),
            ([3, 63, 64, 65, 255, 256, 257, 513], 65536)]


def boundary_case(counts, n_bones):
    """(arrays, bone, weight, bones) of a boundary case: the random rig over a scene of small meshes."""
    a = triangle_meshes(counts, 100 + len(counts) + counts[0])
    nv = len(a["pos"])
    bone, weight = random_skin(nv, n_bones, seed=nv + n_bones)
    # (a -0 in the rest pose of a vertex that keeps its bits, whatever the scene's own -0 fell on)
    a["pos"][int(np.flatnonzero(~skinned_rows(weight))[0]), 0] = np.float32(-0.0)
    return a, bone, weight, random_bones(n_bones, seed=n_bones)


def all_cases():
    """(name, arrays, bone, weight, bones) of every pose the device tests compare."""
    for kind in BEND_KINDS:
        a = pyrt.Scene(kind, 24, 24).arrays()
        bone, weight = bend_skin(a)
        for deg in BEND_DEGS:
            yield "bend %s %g" % (kind, deg), a, bone, weight, bend_bones(deg)
    for counts, n_bones in BOUNDARY:
        yield ("boundary %s %d" % (counts, n_bones),) + boundary_case(counts, n_bones)
