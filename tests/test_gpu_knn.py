"""rt_knn (the photon frames' k-NN walk, knn_query, on the frames' LDS layout) query by query:
against the reference's own kdtree::knearest on tie-heavy and scaled maps
(tests/golden/ref_knn_ties.npz), against the oracle on tie families across the 16-bit / 32-bit
stack-entry boundary (65,534 / 65,535 / 65,536 photons), at 2^-80 .. 2^64, on special queries
and launch edges; and photon frames whose k results tie exactly, against the oracle's frames.
Everything bit-exact; the GPU walk may visit fewer nodes than the reference, never more."""
import numpy as np
import pytest

import knn_ties
import orc
import pyrt

pytestmark = pytest.mark.gpu

RT_ERR_UNSUPPORTED, RT_ERR_STATE = 4, 5
G = 0.125  # grid spacing of the tie families (exact in float)
SMALL = list(range(1, 18))
BIG = [1000, 65534, 65535, 65536, 100003]
BIG_K = (1, 2, 7, 16)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def ctx():
    c = pyrt.Context(pyrt.Scene("cubes", 16, 16))
    yield c
    c.close()


def _family(rng, n, kind):
    """Tie-heavy positions: 0 a lattice of spacing 1/8, 1 every position repeated,
    2 axis-aligned walls (one coordinate shared), 3 a line (two coordinates shared)."""
    if kind == 0:
        return (rng.integers(-12, 13, (n, 3)) * G).astype(np.float32)
    if kind == 1:
        base = rng.uniform(-1.5, 1.5, (n // 3 + 1, 3)).astype(np.float32)
        return base[rng.integers(0, len(base), n)]
    pos = rng.uniform(-1.5, 1.5, (n, 3)).astype(np.float32)
    if kind == 2:
        wall = rng.integers(0, 5, n)
        pos[wall == 0, 1] = -1.0
        pos[wall == 1, 0] = -1.5
        pos[wall == 2, 0] = 1.5
        pos[wall == 3, 2] = -1.5
        return pos
    pos[:, 0], pos[:, 2] = 0.25, -0.5
    pos[:, 1] = rng.integers(-48, 48, n) * (G / 4)
    return pos


def _queries(rng, pos, nq):
    """Photon positions, cell centres and edge midpoints of the 1/8 grid around them (exact
    equal-distance ties on the lattice), points with one coordinate on a photon's (split planes),
    random points, and points 10^3 x the map's extent away (k = 1 walks record a far child at
    every level there: the deepest stacks)."""
    lo, hi = pos.min(0), pos.max(0)
    ext = max(float((hi - lo).max()), G)
    pick = pos[rng.integers(0, len(pos), nq)]
    q = rng.uniform(lo - G, hi + G, (nq, 3)).astype(np.float32)
    kind = np.arange(nq) % 6
    q[kind == 0] = pick[kind == 0]
    half = rng.choice([-G / 2, G / 2], (nq, 3)).astype(np.float32)
    q[kind == 1] = pick[kind == 1] + half[kind == 1]
    edge = half * (rng.integers(0, 3, nq)[:, None] == np.arange(3))
    q[kind == 2] = pick[kind == 2] + edge[kind == 2]
    ax = rng.integers(0, 3, nq)
    on = kind == 3
    q[on, ax[on]] = pick[on, ax[on]]
    far = np.array([[-1, -1, -1], [1, 1, 1], [-1, 1, -1], [1, -1, 0.5]], np.float32)
    f = kind == 5
    q[f] = ((lo + hi) / 2 + far[np.arange(nq)[f] % 4] * (1000 * ext)).astype(np.float32)
    return q


def _upload(ctx, pos):
    """The map in kdtree order (unique directions), installed; returns it as [n][7]."""
    n = len(pos)
    dirs = np.stack([np.arange(n), np.ones(n), -np.arange(n)], 1).astype(np.float32)
    kp, kd_, kw = pyrt.kd_order(pos, dirs, np.ones(n, np.float32))
    ctx.set_photons(kp, kd_)
    return np.concatenate([kp, kd_, kw[:, None]], 1)


def _check(ctx, ph7, q, ks, tag):
    for k in ks:
        idx, dist, vis = ctx.knn(q, k)
        ri, rd, rv = orc.knn(ph7, q, k)
        # distances bit for bit; a NaN distance (NaN query) only as NaN: its sign and payload are the ALU's
        # NaN propagation, which x86 and gfx950 do differently, and no result depends on them
        bad_i = (idx != ri).any(1)
        bad_d = ((bits(dist) != bits(rd)) & ~(np.isnan(dist) & np.isnan(rd))).any(1)
        bad = bad_i | bad_d
        assert not bad.any(), (tag, k, int(bad_i.sum()), int(bad_d.sum()), q[bad][:4])
        assert (vis <= rv).all(), (tag, k, q[vis > rv][:4])


def test_knn_equals_reference_on_ties(ctx):
    """The reference's own tree order uploaded as is; every result (position + direction of
    each of the k photons, in order) is the reference's, for every query and k."""
    for m in knn_ties.load():
        tree = m["tree"]
        ctx.set_photons(tree[:, 0:3], tree[:, 3:6])
        for k, (_, visited, slots) in m["by_k"].items():
            idx, dist, vis = ctx.knn(m["queries"], k)
            bad = (bits(tree[idx]) != bits(tree[slots])).any((1, 2))
            assert not bad.any(), (m["name"], k, int(bad.sum()), m["queries"][bad][:4])
            assert (vis <= visited).all(), (m["name"], k)


@pytest.mark.parametrize("kind", [0, 1, 2, 3])
def test_knn_equals_oracle_tie_families(ctx, kind):
    """Every k on maps of 1..17 photons (one-child nodes, the initial heap the whole map), and
    k in {1, 2, 7, 16} across the entry-width boundary: 65,534 photons walk with 16-bit stack
    entries, 65,535 and up with 32-bit ones (slot 0xffff would be the 16-bit sentinel)."""
    rng = np.random.default_rng(40 + kind)
    for n in SMALL + BIG:
        pos = _family(rng, n, kind)
        ph7 = _upload(ctx, pos)
        big = n > 17
        _check(ctx, ph7, _queries(rng, pos, 256 if big else 64), BIG_K if big else range(1, min(16, n) + 1), (kind, n))


@pytest.mark.parametrize("e", [-80, -72, -64, -40, 0, 40, 62, 64])
def test_knn_equals_oracle_scaled(ctx, e):
    """The tie families at 2^e, queries scaled with them: squared distances underflow to 0
    (the m_bestdist == 0 stop), go subnormal, approach FLT_MAX or overflow to inf (all ties)."""
    rng = np.random.default_rng(1000 + e)
    for kind in range(4):
        for n in SMALL + [1000, 65534]:
            pos = _family(rng, n, kind)
            q = _queries(rng, pos, 12 if n > 17 else 16)  # (below 2^-40 the reference visits every node)
            ph7 = _upload(ctx, np.ldexp(pos, e).astype(np.float32))
            big = n > 17
            _check(ctx, ph7, np.ldexp(q, e).astype(np.float32), BIG_K if big else range(1, min(16, n) + 1),
                   (e, kind, n))


def test_knn_special_queries_and_launch_edges(ctx):
    rng = np.random.default_rng(7)
    inf, nan = np.inf, np.nan
    special = np.array([[inf, 0, 0], [-inf, 0, 0], [0, inf, 0], [0, 0, -inf], [inf, inf, inf], [-inf, inf, -inf],
                        [nan, 0, 0], [0, nan, 0], [0, 0, nan], [nan, nan, nan], [nan, inf, 0], [inf, -inf, nan]],
                       np.float32)
    for n in (5, 1000, 65534, 65535):
        pos = _family(rng, n, 0)
        ph7 = _upload(ctx, pos)
        at = pos[rng.integers(0, n, 64)]  # exactly at a photon
        plane = rng.uniform(-1.5, 1.5, (64, 3)).astype(np.float32)  # on a photon's split coordinate
        plane[np.arange(64), np.arange(64) % 3] = ph7[rng.integers(0, n, 64), np.arange(64) % 3]
        _check(ctx, ph7, np.concatenate([special, at, plane]), (1, 2, 5) if n == 5 else BIG_K, n)
        for nq in (0, 1, 63, 65):  # partial workgroups
            _check(ctx, ph7, _queries(rng, pos, nq), (1, 5), (n, nq))
        q = _queries(rng, pos, 4)
        for k in (0, 17):
            with pytest.raises(pyrt.RtError) as err:
                ctx.knn(q, k)
            assert err.value.code == RT_ERR_UNSUPPORTED
        if n < 16:
            with pytest.raises(pyrt.RtError) as err:
                ctx.knn(q, n + 1)
            assert err.value.code == RT_ERR_STATE
    ctx.set_photons(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32))
    with pytest.raises(pyrt.RtError) as err:
        ctx.knn(np.zeros((4, 3), np.float32), 1)
    assert err.value.code == RT_ERR_STATE


def _frame(kind, mode, k, ph7, nreq):
    w, h = 32, 24
    s = pyrt.Scene(kind, w, h)
    c = pyrt.Context(s)
    c.set_photons(ph7[:, 0:3], ph7[:, 3:6])
    bg = pyrt.background(w, h)
    p = pyrt.make_params(w, h, 2, mode=mode, seed=5, use_photons=1, k=k, photons_requested=nreq, collect_stats=1)
    out, acc, st = c.render(p, bg)
    ref_out, ref_acc, ref_st = orc.render(s, p, math_mode=orc.MATH_DET, bg=bg, ext_photons=ph7)
    c.close()
    assert np.array_equal(bits(acc), bits(ref_acc)), (mode, k, len(ph7))
    assert np.array_equal(bits(out), bits(ref_out)), (mode, k, len(ph7))
    assert st.knn_queries == ref_st.knn_queries and 0 < st.kd_visited <= ref_st.kd_visited


@pytest.mark.parametrize("mode", [pyrt.MODE_RAY, pyrt.MODE_PATH])
def test_photon_frames_with_tied_results(ctx, mode):
    """Every photon position twice, the copy carrying another photon's direction: each query's
    k results tie exactly, and their order reaches the direction sum that shades the pixel.
    Then maps of 65,534 (16-bit entries) and 65,535 photons (32-bit)."""
    pos, dir_, w = ctx.emit_photons(4000, seed=3)
    n = len(pos)
    assert n > 1000
    other = np.roll(np.arange(n), 7)
    pos2, dir2 = np.concatenate([pos, pos]), np.concatenate([dir_, dir_[other]])
    kp, kd_, kw = pyrt.kd_order(pos2, dir2, np.concatenate([w, w]))
    ph7 = np.concatenate([kp, kd_, kw[:, None]], 1)
    for k in (1, 2, 16):
        _frame("cubes", mode, k, ph7, 4000)
    pos, dir_, w = ctx.emit_photons(140000, seed=4)
    assert len(pos) >= 65535
    for n in (65534, 65535):
        kp, kd_, kw = pyrt.kd_order(pos[:n], dir_[:n], w[:n])
        _frame("cubes", mode, 10, np.concatenate([kp, kd_, kw[:, None]], 1), n)
