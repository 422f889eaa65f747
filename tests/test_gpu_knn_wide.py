"""rt_knn_wide (the k-NN walk photon frames with 17 <= k <= 256 run, on their LDS layout) query by query
against the oracle's kdtree::knearest: the tie families and query mix of test_gpu_knn.py on maps across the
16-bit / 32-bit boundary (65,534 / 65,535 photons), at 2^-40 .. 2^62, k from 17 to 256 and k = n on small
maps.  Indices, distances and their order bit for bit; the GPU walk may visit fewer nodes, never more."""
import numpy as np
import pytest

import orc
import pyrt
from test_gpu_knn import _family, _queries, _upload

pytestmark = pytest.mark.gpu

RT_ERR_UNSUPPORTED, RT_ERR_STATE = 4, 5
KS = (17, 31, 32, 33, 64, 100, 128, 255, 256)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def ctx():
    c = pyrt.Context(pyrt.Scene("cubes", 16, 16))
    yield c
    c.close()


def _check(ctx, ph7, q, ks, tag):
    for k in ks:
        idx, dist, vis = ctx.knn_wide(q, k)
        ri, rd, rv = orc.knn(ph7, q, k)
        assert idx.shape == (len(q), k)
        bad_i = (idx != ri).any(1)
        bad_d = ((bits(dist) != bits(rd)) & ~(np.isnan(dist) & np.isnan(rd))).any(1)
        bad = bad_i | bad_d
        assert not bad.any(), (tag, k, int(bad_i.sum()), int(bad_d.sum()), q[bad][:4])
        assert (vis <= rv).all(), (tag, k, q[vis > rv][:4])


@pytest.mark.parametrize("n", [17, 100, 1000, 65534, 65535, 100003])
def test_knn_wide_equals_oracle(ctx, n):
    """Every k of KS up to n (and k = n on the small maps, where the initial heap is the whole map), on all
    four tie families; 65,534 photons walk with 16-bit stack entries and heap indices, 65,535 and up with
    32-bit ones."""
    rng = np.random.default_rng(300 + n)
    ks = [k for k in KS if k <= n] + ([n] if n <= 256 and n not in KS else [])
    for kind in range(4):
        pos = _family(rng, n, kind)
        ph7 = _upload(ctx, pos)
        _check(ctx, ph7, _queries(rng, pos, 96 if n > 1000 else 128), ks, (kind, n))


@pytest.mark.parametrize("e", [-40, -20, 0, 40, 62])
def test_knn_wide_equals_oracle_scaled(ctx, e):
    """The lattice and the repeated positions at 2^e: squared distances go subnormal, approach FLT_MAX or
    overflow to inf (everything ties)."""
    rng = np.random.default_rng(2000 + e)
    for kind in (0, 1):
        for n in (40, 1000):
            pos = _family(rng, n, kind)
            q = _queries(rng, pos, 24)
            ph7 = _upload(ctx, np.ldexp(pos, e).astype(np.float32))
            _check(ctx, ph7, np.ldexp(q, e).astype(np.float32), [k for k in (17, 64, 256) if k <= n], (e, kind, n))


def test_knn_wide_is_knn_up_to_16(ctx):
    """k <= 16 runs rt_knn's instance: the same indices, distances and visit counts."""
    rng = np.random.default_rng(11)
    pos = _family(rng, 5000, 2)
    _upload(ctx, pos)
    q = _queries(rng, pos, 200)
    for k in range(1, 17):
        a, b = ctx.knn(q, k), ctx.knn_wide(q, k)
        assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1])) and np.array_equal(a[2], b[2]), k


def test_knn_wide_errors_and_batches(ctx):
    rng = np.random.default_rng(12)
    pos = _family(rng, 1000, 0)
    ph7 = _upload(ctx, pos)
    for nq in (0, 1, 63, 65):  # partial workgroups
        _check(ctx, ph7, _queries(rng, pos, nq), (17, 64), nq)
    q = _queries(rng, pos, 4)
    for k in (0, 257):
        with pytest.raises(pyrt.RtError) as err:
            ctx.knn_wide(q, k)
        assert err.value.code == RT_ERR_UNSUPPORTED
        assert "256" in str(err.value) or k == 0
    # rt_knn keeps its 1..16 contract
    with pytest.raises(pyrt.RtError) as err:
        ctx.knn(q, 17)
    assert err.value.code == RT_ERR_UNSUPPORTED
    _upload(ctx, pos[:40])
    with pytest.raises(pyrt.RtError) as err:
        ctx.knn_wide(q, 41)
    assert err.value.code == RT_ERR_STATE
    ctx.set_photons(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32))
    with pytest.raises(pyrt.RtError) as err:
        ctx.knn_wide(q, 64)
    assert err.value.code == RT_ERR_STATE
