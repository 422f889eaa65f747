"""tests/deform.py checked on the CPU, with the oracle alone: the poses are what their names say, the restated plane scale
steps where the poses claim it does, and the ray batch hits the deformed geometry (or provably nothing on the collapsed
poses) — so that tests/test_gpu_deform.py cannot pass on rays that miss everything.  Also numpy_refit itself, on a tree small
enough to work the boxes out by hand, with the leaf sizes 8 and 1 that no preset scene has."""
import numpy as np
import pytest

import deform
import orc
import pyrt
from test_gpu_update import numpy_refit, pad_rule

N_RAYS = 2048


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def posed(a, pose):
    return dict(a, **pose)


@pytest.mark.parametrize("n", deform.SIZES)
def test_scene_shape(n):
    a = deform.scene(n, 100 + n)
    assert a["tri"].shape == (n, 3) and a["pos"].shape == (3 * n + 2, 3) == a["nrm"].shape
    assert np.array_equal(deform.referenced(a), np.arange(3 * n))
    assert len(a["tri_begin"]) == (3 if n >= 2 else 2) and a["tri_begin"][-1] == n and a["vtx_begin"][-1] == 3 * n + 2
    if n >= 2:
        assert a["tri_begin"][1] == n // 2 and a["vtx_begin"][1] == 3 * (n // 2)
    assert len(a["materials"]) == len(a["tri_begin"]) - 1
    assert np.isfinite(a["pos"]).all() and np.abs(a["pos"]).max() <= 1.35 + 1e-6
    assert np.float32(np.float32(6e-5) * deform.pad_ref(a)) == pad_rule(a)


@pytest.mark.parametrize("n", deform.SIZES)
def test_poses_are_what_they_say(n):
    a = deform.scene(n, 100 + n)
    ref = deform.referenced(a)
    P = dict(deform.poses(a, 7))
    assert list(P) == ["shuffle", "flat", "point", "origin", "big", "small", "step_below", "step_at", "stray", "rest"]
    for name, pose in P.items():
        assert pose["pos"].dtype == np.float32 and pose["pos"].shape == a["pos"].shape, name
        assert np.array_equal(bits(pose["nrm"]), bits(a["nrm"])), name
        assert np.isfinite(pose["pos"][ref]).all(), name
    # shuffle: a permutation of the referenced rows, the others untouched
    s = P["shuffle"]["pos"]
    order = lambda x: x[np.lexsort(x.T)]
    assert np.array_equal(bits(order(s[ref])), bits(order(a["pos"][ref])))
    assert np.array_equal(bits(s[-2:]), bits(a["pos"][-2:]))
    if n >= 8:
        assert not np.array_equal(s[ref], a["pos"][ref])
    # extents
    ext = lambda name: np.ptp(P[name]["pos"][ref], axis=0)
    assert ext("flat")[2] == 0 and (P["flat"]["pos"][ref, 2] == np.float32(-0.5)).all() and (ext("flat")[:2] > 0).all()
    assert (ext("point") == 0).all() and np.array_equal(bits(P["point"]["pos"][ref[-1]]), bits(a["pos"][0]))
    o = P["origin"]["pos"][ref]
    assert (o == 0).all() and np.signbit(o).any() and not np.signbit(o).all()
    # the scaled poses take the camera and the lights along
    for name, f in (("big", 4096.0), ("small", 0.125)):
        assert np.array_equal(P[name]["pos"], a["pos"] * np.float32(f))
        assert np.array_equal(P[name]["camera"], a["camera"] * np.float32(f))
        assert np.array_equal(P[name]["lights"][:, 0:3], a["lights"][:, 0:3] * np.float32(f))
    for name in ("shuffle", "flat", "point", "origin", "stray", "rest"):
        assert P[name]["camera"] is a["camera"] and P[name]["lights"] is a["lights"]
    # stray: the rest pose, except two non-finite vertices nobody references
    st = P["stray"]["pos"]
    assert np.array_equal(bits(st[ref]), bits(a["pos"][ref])) and np.isnan(st[-2]).all() and (st[-1] == np.inf).all()
    assert P["rest"]["pos"] is a["pos"]


@pytest.mark.parametrize("n", deform.SIZES)
def test_plane_scale_steps(n):
    """step_below and step_at lie either side of a step of the restated boxScale, under 1 % apart; the scale of the other
    poses follows their size, and at maxAbs = 0 it stays finite."""
    a = deform.scene(n, 100 + n)
    P = dict(deform.poses(a, 7))
    below, at = posed(a, P["step_below"]), posed(a, P["step_at"])
    sb, sa = deform.box_scale(below), deform.box_scale(at)
    assert sb == 2 * sa and sb.dtype == np.float32
    ref = deform.referenced(a)
    rel = np.abs(at["pos"][ref] - below["pos"][ref]) / np.abs(below["pos"][ref])
    assert rel.max() < 0.01
    # ... and the sum that decides it lies at most at 2 on one side, above it on the other
    v = lambda b: np.float32(np.abs(b["pos"][ref]).max() + pad_rule(b))
    assert v(below) <= 2 < v(at) and v(at) / v(below) < 1.01
    s0 = deform.box_scale(posed(a, P["origin"]))
    assert np.isfinite(s0) and 0 < s0 <= np.float32(2.0) ** 29  # (pad >= 6e-5: 32768 / pad < 2^30)
    # (a power of two scales every term of the rule exactly; 1/8 does not, where padRef's floor of 1 binds)
    assert deform.box_scale(posed(a, P["big"])) * 4096 == deform.box_scale(a)
    assert deform.box_scale(posed(a, P["small"])) >= 4 * deform.box_scale(a)
    # every plane of the scaled scene fits binary16's range
    for name in P:
        b = posed(a, P[name])
        assert (np.abs(b["pos"][ref]).max() + pad_rule(b)) * deform.box_scale(b) <= 32768


FRACTIONS = {}


@pytest.mark.parametrize("n", deform.SIZES)
def test_rays_hit_the_deformed_geometry(n):
    """The non-vacuity condition: through the exhaustive loop at least half of the rays hit on every pose with extent, and
    none on the collapsed ones, whose frame is the background."""
    a = deform.scene(n, 100 + n)
    for name, pose in deform.poses(a, 7):
        b = posed(a, pose)
        r = deform.rays(b, N_RAYS, 11)
        assert len(r) == N_RAYS and np.isfinite(r["origin"]).all() and np.isnan(r["direction"][-1]).all()
        assert np.abs(r["origin"]).max() < 16 * deform.pad_ref(b)
        assert ((r["direction"][:-1] == 0).sum(1) >= 1).sum() >= N_RAYS // 16
        s = deform.array_scene(b)
        frac = orc.trace(s, r)["hit"].mean()
        FRACTIONS[(n, name)] = frac
        print("n %4d %-10s hit fraction %.3f" % (n, name, frac))
        if name in deform.DEGENERATE:
            assert frac == 0, name
            p = pyrt.make_params(16, 16, 2, mode=pyrt.MODE_PATH, seed=5)
            bg = orc.background(16, 16)
            out, acc, st = orc.render(s, p, math_mode=orc.MATH_DET, bg=bg)
            assert np.array_equal(bits(out), bits(bg)) and st.rays_shadow == 0
        else:
            assert frac >= 0.5, name


def test_numpy_refit_by_hand():
    """Three nodes, leaves of 8, 1, 2 and 3 records in a shuffled record order.  Triangle t = {(t, 10 t, -t),
    (t + 1/2, 10 t + 1, -t), (t, 10 t, -t - 1/4)}, pad 1/8: a leaf over the set S has
    lo = (min S - 1/8, 10 min S - 1/8, -max S - 3/8) and hi = (max S + 5/8, 10 max S + 9/8, -min S + 1/8)."""
    t = np.arange(14, dtype=np.float32)
    pos = np.stack([np.stack([t, 10 * t, -t], 1), np.stack([t + 0.5, 10 * t + 1, -t], 1), np.stack([t, 10 * t, -t - 0.25], 1)], 1)
    pos = np.ascontiguousarray(pos.reshape(-1, 3), np.float32)
    tri = np.arange(42, dtype=np.uint32).reshape(14, 3)
    ids = np.array([3, 7, 1, 12, 9, 4, 10, 6, 13, 0, 2, 5, 8, 11], np.uint32)
    leaf = lambda first, cnt: np.uint32(~((first << 3) | (cnt - 1)) & 0xFFFFFFFF)
    nodes = np.zeros((3, 16), np.uint32)
    nodes[:, 0:12] = np.float32(777).view(np.uint32)  # (stale boxes: every plane must be written)
    nodes[0, 12:14] = [1, 2]
    nodes[1, 12:14] = [leaf(0, 8), leaf(8, 1)]
    nodes[2, 12:14] = [leaf(9, 2), leaf(11, 3)]
    tris = np.zeros((14, 12), np.uint32)
    tris[:, 0:9] = np.float32(-5).view(np.uint32)
    tris[:, 9] = ids
    got_n, got_t = numpy_refit(nodes, tris, pos, tri, np.float32(0.125))
    A = [0.875, 9.875, -12.375, 12.625, 121.125, -0.875]      # {1 ... 12}
    B = [12.875, 129.875, -13.375, 13.625, 131.125, -12.875]  # {13}
    Cc = [-0.125, -0.125, -2.375, 2.625, 21.125, 0.125]       # {0, 2}
    D = [4.875, 49.875, -11.375, 11.625, 111.125, -4.875]     # {5, 8, 11}
    AB = [0.875, 9.875, -13.375, 13.625, 131.125, -0.875]
    CD = [-0.125, -0.125, -11.375, 11.625, 111.125, 0.125]
    want = np.array([AB + CD, A + B, Cc + D], np.float32)
    assert np.array_equal(got_n[:, 0:12].view(np.float32), want)
    assert np.array_equal(got_n[:, 12:], nodes[:, 12:])
    f = got_t.view(np.float32)
    idf = ids.astype(np.float32)
    assert np.array_equal(f[:, 0:3], np.stack([idf, 10 * idf, -idf], 1))
    assert (f[:, 3:6] == np.float32([0.5, 1, 0])).all() and (f[:, 6:9] == np.float32([0, 0, -0.25])).all()
    assert np.array_equal(got_t[:, 9:], tris[:, 9:])
