"""tests/tiescenes.py against the oracle, on the CPU: on every scene and ray family the oracle's exhaustive loop and its BVH
agree on every field; on the families with exact arithmetic the oracle's hits are those of the integer restatement
(tiescenes.exact_hits), u, v and t to the bit; the small frames agree; and the families do what they are for — the coverage
conditions below are asserted from the exact reference and the oracle alone, never measured on the code under test."""
import numpy as np
import pytest

import aov_ref
import orc
import pyrt
import tiescenes as ts

W, H = ts.FRAME


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def family(name, fam):
    return next(f for f in ts.families(name) if f.name == fam)


def exact_pair(name, fam):
    """(oracle hits, exact_hits) of the family's exact rays, and the family's k for them."""
    f = family(name, fam)
    rays = f.rays[f.exact]
    return orc.trace(ts.scene(name), rays), ts.exact_hits(ts.scene(name), rays), None if f.k is None else f.k[f.exact]


@pytest.mark.parametrize("name", ts.SCENES)
def test_oracle_loop_equals_oracle_bvh(name):
    s = ts.scene(name)
    for f in ts.families(name):
        loop = orc.trace(s, f.rays)
        tree = orc.trace(s, f.rays, orc.ACCEL_OBVH)
        diff = (loop.view(np.uint8).reshape(len(loop), -1) != tree.view(np.uint8).reshape(len(loop), -1)).any(axis=1)
        assert not diff.any(), "%s %s: %d rays differ, first %d" % (name, f.name, diff.sum(), np.argmax(diff))
        for accel in (orc.ACCEL_LOOP, orc.ACCEL_OBVH):
            assert np.array_equal(orc.trace(s, f.rays, accel, pyrt.TRACE_ANY)["hit"], loop["hit"]), (name, f.name, accel)


@pytest.mark.parametrize("fam", ["axial", "slanted", "onsurface"])
@pytest.mark.parametrize("name", ts.SCENES)
def test_oracle_equals_the_integer_restatement(name, fam):
    """hit, mesh and tri; u, v and t bit for bit wherever the winner's determinant is a power of two — all of `axial`, and by
    the choice of the directions the other two families as well."""
    o, ex, _ = exact_pair(name, fam)
    h = o["hit"] != 0
    assert np.array_equal(h, ex["hit"]), "%s %s: first ray %d" % (name, fam, np.argmax(h != ex["hit"]))
    assert np.array_equal(o["mesh"][h], ex["mesh"][h]) and np.array_equal(o["tri"][h], ex["tri"][h]), (name, fam)
    assert ex["pow2"][h].all()
    for k, e in (("u", "u"), ("v", "v"), ("d", "t")):
        assert np.array_equal(o[k][h].astype(np.float64), ex[e][h]), (name, fam, k)


@pytest.mark.parametrize("name", ts.SCENES)
def test_oracle_frames_agree(name):
    """The scene's small frame by the loop and by the oracle's BVH: accumulators and ray counts.  The frame is lit, and it
    shows who wins a tie: with the materials of the meshes reversed it is another frame."""
    s = ts.scene(name)
    p = pyrt.make_params(W, H, 2, seed=5)
    _, loop, sl = orc.render(s, p, math_mode=orc.MATH_DET)
    _, tree, st = orc.render(s, p, math_mode=orc.MATH_DET, accel=orc.ACCEL_OBVH)
    assert np.array_equal(bits(loop), bits(tree))
    assert (sl.rays_closest, sl.rays_shadow) == (st.rays_closest, st.rays_shadow)
    assert (loop[..., :3].sum(axis=2) > 0).mean() > 0.5, "most of the frame is lit"
    a = s.arrays()
    if len(a["materials"]) > 1:
        _, other, _ = orc.render(ts.array_scene(a, materials=a["materials"][::-1].copy()), p, math_mode=orc.MATH_DET)
        assert (bits(other) != bits(loop)).any(axis=2).mean() > 0.5


# ---- what the families are for -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["stack", "stack_shuffled"])
def test_most_rays_hit_a_tie_of_four(name):
    for fam in ("axial", "slanted"):
        _, ex, k = exact_pair(name, fam)
        sel = np.ones(len(ex["hit"]), bool) if k is None else k >= -15
        assert ex["hit"][sel].mean() >= 0.5, (name, fam, ex["hit"][sel].mean())
        front = ex["hit"] & np.isin(ex["mesh"], ts.front_meshes(name))
        assert front[sel].mean() >= 0.4 and (ex["tied"][front] >= 4).all(), (name, fam)
        assert (ex["mesh"][front] == min(ts.front_meshes(name))).all(), "the lowest mesh wins"


@pytest.mark.parametrize("name", ["fan", "tiny2", "tiny3"])
def test_front_hits_of_the_small_scenes_are_ties(name):
    for fam in ("axial", "slanted"):
        _, ex, _ = exact_pair(name, fam)
        front = ex["hit"] & np.isin(ex["mesh"], ts.front_meshes(name))
        assert front.mean() >= 0.2 and (ex["tied"][front] >= ts.min_tie(name)).all(), (name, fam, front.mean())
    if name == "fan":
        _, ex, _ = exact_pair(name, "axial")
        assert ex["tied"].max() >= 16, "the rays through the fan's centre meet all eight triangles of both copies"


@pytest.mark.parametrize("name", ["stack", "stack_shuffled", "fan"])
def test_many_hits_lie_on_an_edge_or_a_vertex(name):
    for fam in ("axial", "slanted"):
        o, ex, _ = exact_pair(name, fam)
        h = ex["hit"]
        assert ex["edge"][h].mean() >= 0.3, (name, fam)
        # ... in the oracle's floats too
        u, v = o["u"][h], o["v"][h]
        assert ((u == 0) | (v == 0) | (u + v == 1)).mean() >= 0.3


@pytest.mark.parametrize("name", ts.SCENES)
def test_the_determinant_threshold_is_straddled(name):
    """The same origins and signs at every k.  A triangle of doubled area 2^a has |det| = 2^(k + a): the sheets' 2^(k - 4) is
    below Ray.cpp's EPSILON (2^-20 < 1e-6 < 2^-19) at k = -16 and above it at k = -15.  Where every determinant is below,
    nothing is hit; from the first k at which every determinant is above, the hits are those of k = 0
    (on the rays whose zero components are zeros)."""
    f = family(name, "axial")
    hit = orc.trace(ts.scene(name), f.rays)["hit"] != 0
    a_max, a_min = {"stack": (-4, -4), "stack_shuffled": (-4, -4), "fan": (-2, -4)}.get(name, (2, 2))  # log2 of the doubled areas
    per_k = {k: hit[f.k == k] for k in ts.K_AXIAL}
    plain = f.exact[f.k == 0]  # (a denormal component moves an edge hit to one side or the other, by an amount that depends on k)
    dead = [k for k in ts.K_AXIAL if k + a_max < -19]
    alive = [k for k in ts.K_AXIAL if k + a_min >= -19]
    assert dead and len(alive) >= 4
    for k in dead:
        assert not per_k[k].any(), (name, k)
    for k in alive:
        assert np.array_equal(per_k[k][plain], per_k[0][plain]) and per_k[k].mean() > 0.4, (name, k)
    if name.startswith("stack"):  # (the wall is edge-on to these rays: its determinant is 0, or denormal)
        assert not per_k[-16].any() and not per_k[-17].any() and -15 in alive


@pytest.mark.parametrize("name", ts.SCENES)
def test_at_least_half_the_frame_sees_a_tie(name):
    s = ts.scene(name)
    rays = aov_ref.primary_rays(s, pyrt.make_params(W, H, 1, seed=5)).reshape(-1)
    hits = orc.trace(s, rays)
    if name == "tiny1":
        assert (hits["hit"] != 0).all()  # (one triangle: nothing to tie with)
        return
    tied = ts.tie_counts(name, rays, hits) >= ts.min_tie(name)
    assert tied.mean() >= 0.5, (name, tied.mean())


def test_onsurface_rays_leave_their_own_sheets():
    for name in ("stack", "stack_shuffled"):
        f = family(name, "onsurface")
        o = orc.trace(ts.scene(name), f.rays)
        down = f.rays["direction"][:, 2] < 0
        inside = (np.abs(f.rays["origin"][:, :2]) <= 1).all(axis=1)
        back = 4 if name == "stack" else 1
        assert np.array_equal(o["hit"] != 0, down & inside) and (o["mesh"][down & inside] == back).all()
        assert (o["d"][down & inside] == 0.5).all()


def test_bound_family_sits_on_both_sides():
    for name in ts.SCENES:
        a = ts.arrays(name)
        f = family(name, "bound")
        ins = ts.inside_bound(a, f.rays)
        B = ts.origin_bound(a)
        assert 0.3 < ins.mean() < 0.7 and (np.abs(f.rays["origin"]).max(axis=1) == B).sum() >= 16
        hit = orc.trace(ts.scene(name), f.rays)["hit"] != 0
        assert hit[ins].any() and hit[~ins].any()


def test_inplane_rays_meet_the_wall_on_its_edge():
    f = family("stack", "inplane")
    o = orc.trace(ts.scene("stack"), f.rays)
    h = o["hit"] != 0
    assert h.any() and (o["mesh"][h] == 5).all(), "the sheets' determinant is 0"
    assert ((o["u"][h] == 0) | (o["v"][h] == 0) | (o["u"][h] + o["v"][h] == 1)).all()


def test_helpers_on_a_hand_made_tree():
    """f16_planes rounds outwards, boxplanes puts origins exactly on planes with a zero direction component there, leaf_order
    walks child 0 first."""
    nodes = np.zeros((2, 16), np.uint32)
    f = nodes[:, 0:12].view(np.float32)
    f[0] = [-1.00007, -1.00007, -2.5001, 1.00007, 1.00007, -2.4999, -1.0001, -1.0001, -2.0001, 1.0001, 1.0001, -0.9999]
    f[1] = [-1.0001, -1.0001, -2.0001, 0.1, 1.0001, -1.9999, 0.4999, -0.5001, -2.0001, 0.5001, 0.5001, -0.9999]
    code = lambda first, cnt: np.uint32(~((first << 3) | (cnt - 1)) & 0xFFFFFFFF)
    nodes[0, 12:14] = [code(0, 2), 1]
    nodes[1, 12:14] = [code(2, 1), code(3, 2)]
    tris = np.zeros((5, 12), np.uint32)
    tris[:, 9] = [4, 0, 3, 1, 2]
    assert list(ts.leaf_order(nodes, tris)) == [1, 3, 4, 2, 0]
    scale = np.float32(4096)
    q = ts.f16_planes(nodes, scale)
    box = f.reshape(2, 2, 2, 3)
    assert (q[:, :, 0] <= box[:, :, 0]).all() and (q[:, :, 1] >= box[:, :, 1]).all()
    assert np.array_equal((q * scale).astype(np.float16).astype(np.float32), q * scale) and np.abs(q - box).max() < 2e-3
    fam = ts.boxplanes(nodes, scale)
    planes = set(np.concatenate([box.reshape(-1), q.reshape(-1)]).tolist())
    o, d = fam.rays["origin"], fam.rays["direction"]
    zero = d == 0
    on_plane = np.array([[o[i, a] in planes for a in range(3)] for i in range(len(o))])
    assert (zero & on_plane).any(axis=1).sum() >= 2 * 4 * 24 and np.signbit(d[zero]).any() and not np.signbit(d[zero]).all()
    assert ((zero & on_plane).sum(axis=1) == 2).sum() >= 2 * 4 * 12, "the rays along the edges"
