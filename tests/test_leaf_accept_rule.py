"""The precondition Trav::test_pair's acceptance rests on (rt_kernels.hip): for a candidate that passed the triangle test
with t > 0 and a `best` that is never negative and never NaN, RayTracer.h:40's rule — t < best, or t == best and the
lower triangle id — is one unsigned compare of the 64-bit keys `t bits << 32 | id`, the order the vertex pool's publish /
refresh_best keep.  Exhaustive over a cross product of the floats where bit order and float order could part; a candidate
that failed the test carries anything (NaN, -1, -0) and is never accepted.  numpy only."""
import itertools

import numpy as np

F = np.float32
ULP_DOWN, ULP_UP = F(-np.inf), F(np.inf)


def _with_neighbours(values):
    """The values and, for each, the floats one ulp below and above it that are still positive and no NaN."""
    out = set()
    for v in values:
        v = F(v)
        with np.errstate(over="ignore"):  # (the float above FLT_MAX is +inf)
            near = (v, np.nextafter(v, ULP_DOWN), np.nextafter(v, ULP_UP))
        for x in near:
            if x > 0 and not np.isnan(x):
                out.add(F(x).tobytes())
    return np.sort(np.array([np.frombuffer(b, F)[0] for b in out], F))


DENORM_MIN = np.frombuffer(np.uint32(1).tobytes(), F)[0]
DENORM_MAX = np.frombuffer(np.uint32(0x007FFFFF).tobytes(), F)[0]
FLT_MIN = np.finfo(F).tiny
FLT_MAX = np.finfo(F).max
# smallest and largest denormal, FLT_MIN, 1 - ulp, 1, 1 + ulp, FLT_MAX, +inf, and every pair one ulp apart around them
T = _with_neighbours([DENORM_MIN, DENORM_MAX, FLT_MIN, np.nextafter(F(1), ULP_DOWN), F(1), np.nextafter(F(1), ULP_UP), FLT_MAX, F(np.inf)])
BEST = np.concatenate([np.array([0.0], F), T])  # every best is >= 0 and no NaN (+0: nothing positive is below it)
IDS = np.array([0, 1, 2 ** 31, 2 ** 32 - 1], np.uint32)
REJECTED_T = np.concatenate([np.array([np.nan, -1.0, -0.0], F), T])  # what a lane that failed the test may hold


def key(t, i):
    return (np.ascontiguousarray(t, F).view(np.uint32).astype(np.uint64) << np.uint64(32)) | i.astype(np.uint64)


def float_rule(h, t, i, best, best_id):
    with np.errstate(invalid="ignore"):
        return h & ((t < best) | ((t == best) & (i < best_id)))


def key_rule(h, t, i, best, best_id):
    return h & (key(t, i) < key(best, best_id))


def grid(*axes):
    return [g.reshape(-1) for g in np.meshgrid(*axes, indexing="ij")]


def test_the_values_are_what_they_claim():
    assert DENORM_MIN > 0 and DENORM_MIN == np.nextafter(F(0), ULP_UP) and np.nextafter(DENORM_MAX, ULP_UP) == FLT_MIN
    assert (T > 0).all() and not np.isnan(T).any() and np.isinf(T[-1]) and T[0] == DENORM_MIN
    assert (BEST >= 0).all() and not np.signbit(BEST).any()
    one = int(np.nonzero(T == 1)[0][0])
    assert T[one - 1] < 1 < T[one + 1] and np.nextafter(T[one - 1], ULP_UP) == 1 and np.nextafter(F(1), ULP_UP) == T[one + 1]
    # positive floats order as their bits, equal floats have equal bits
    assert (np.diff(T.view(np.uint32).astype(np.int64)) > 0).all()


def test_one_accepted_candidate():
    t, i, best, best_id = grid(T, IDS, BEST, IDS)
    h = np.ones(len(t), bool)
    want = float_rule(h, t, i, best, best_id)
    assert np.array_equal(key_rule(h, t, i, best, best_id), want)
    assert want.any() and not want.all()
    ties = t == best
    assert ties.any() and np.array_equal(want[ties], (i < best_id)[ties])


def test_a_rejected_candidate_is_never_accepted():
    t, i, best, best_id = grid(REJECTED_T, IDS, BEST, IDS)
    h = np.zeros(len(t), bool)
    assert not key_rule(h, t, i, best, best_id).any() and not float_rule(h, t, i, best, best_id).any()
    # ... although its key alone would often win: the mask is what discards it
    assert (key(t, i) < key(best, best_id)).any()


def pair(rule_is_key, isany, ha, ta, ida, hb, tb, idb, best, best_id):
    """test_pair's A-then-B chain: (ba, bb, best bits, bestId) under either rule."""
    if rule_is_key:
        k0, ka, kb = key(best, best_id), key(ta, ida), key(tb, idb)
        ba = ~isany & ha & (ka < k0)
        k1 = np.where(ba, ka, k0)
        bb = ~isany & hb & (kb < k1)
        k2 = np.where(bb, kb, k1)
        return ba, bb, (k2 >> np.uint64(32)).astype(np.uint32), (k2 & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    ba = ~isany & float_rule(ha, ta, ida, best, best_id)
    b1, i1 = np.where(ba, ta, best), np.where(ba, ida, best_id)
    bb = ~isany & float_rule(hb, tb, idb, b1, i1)
    b2, i2 = np.where(bb, tb, b1), np.where(bb, idb, i1)
    return ba, bb, np.ascontiguousarray(b2, F).view(np.uint32), i2.astype(np.uint32)


def test_the_pair_chain():
    """A then B as test_pair applies them, every combination of passed / failed tests (a failed lane's t drawn from NaN, -1,
    -0 as well), closest and any-hit rays: the same acceptances and the same (best, bestId) bits."""
    small_t = np.concatenate([np.array([np.nan, -1.0, -0.0], F), T[[0, 1]], T[np.nonzero(T == 1)[0][0] - 1:][:3], T[-3:]])
    small_best = np.concatenate([np.array([0.0], F), T[[0]], T[np.nonzero(T == 1)[0][0] - 1:][:3], T[-3:]])
    ids2 = np.array([0, 2 ** 31, 2 ** 32 - 1], np.uint32)
    n = 0
    for isany, pa, pb in itertools.product((False, True), (False, True), (False, True)):
        ta, ida, tb, idb, best, best_id = grid(small_t, ids2, small_t, ids2, small_best, IDS)
        with np.errstate(invalid="ignore"):
            ha, hb = pa & (ta > 0), pb & (tb > 0)  # (an accepted t is positive; the other lanes keep whatever t they hold)
        any_ = np.full(len(ta), isany)
        got = pair(True, any_, ha, ta, ida, hb, tb, idb, best, best_id)
        want = pair(False, any_, ha, ta, ida, hb, tb, idb, best, best_id)
        for g, w, what in zip(got, want, ("ba", "bb", "best", "bestId")):
            assert np.array_equal(g, w), (what, isany, pa, pb)
        if isany or not (pa or pb):
            assert not got[0].any() and not got[1].any()
        n += len(ta)
    assert n == 8 * (len(small_t) * len(ids2)) ** 2 * len(small_best) * len(IDS)
