"""tests/pick_ref.py on the oracle alone (no GPU): the conditions under which a bit-exact comparison against it means
something.  Every light that can be picked is picked in every slot of every case; a kernel that picks other lights, or
forgets the 1 / m of the weight, does not pass; the picked frame estimates the frame of all lights; and the table's edge
cases."""
import numpy as np
import pytest

import lens_ref
import orc
import pick_ref

F32, F64 = np.float32, np.float64


@pytest.mark.parametrize("case", pick_ref.CASES, ids=pick_ref.case_id)
def test_every_light_that_can_be_picked_is_picked_in_every_slot(case):
    """A condition on the inputs: a case that fails it is changed, not this check."""
    t, k = pick_ref.case_table(case), pick_ref.case_picks(case)
    n, m = len(t["p"]), pick_ref.case_slots(case)
    assert k.shape[-1] == m and k.min() >= 0 and k.max() < n
    for j in range(m):
        count = np.bincount(k[..., j].ravel(), minlength=n)
        assert (count[t["p"] > 0] > 0).all(), (j, count)
        assert (count[t["p"] == 0] == 0).all(), (j, count)


def test_the_picks_are_the_samples_own_and_chain():
    """Sample i of a pixel has the same picks whatever range it is rendered in."""
    whole = next(c for c in pick_ref.CASES if c[3] is pick_ref.SPP7)
    t = pick_ref.case_table(whole)["thresholds"]
    k = pick_ref.case_picks(whole)
    tail = pick_ref.picks(pick_ref.case_params(whole, spp_begin=3, spp_count=4), t, pick_ref.case_slots(whole))
    assert (tail == k[:, :, 3:7]).all() and (k[:, :, 0] != k[:, :, 1]).any()


@pytest.mark.parametrize("case", pick_ref.CASES, ids=pick_ref.case_id)
def test_wrong_picks_and_wrong_weights_change_the_reference(case):
    ref, t, k = pick_ref.case_reference(case), pick_ref.case_table(case), pick_ref.case_picks(case)
    m, positive = pick_ref.case_slots(case), int((t["p"] > 0).sum())
    shifted = pick_ref.build(case, t["lights"], pick_ref.shifted(case, k))
    share = pick_ref.changed_rgb_words(ref["accum"], shifted["accum"])
    print("%s: shifted picks change %.3f of the rgb words" % (pick_ref.case_id(case), share))
    if positive > 1:
        assert share > pick_ref.MIN_CHANGED_SHIFT
    else:
        assert share == 0
    plain = pick_ref.build(case, pick_ref.case_table(case, drop_slots=True)["lights"], k, tag="no 1/m")
    share = pick_ref.changed_rgb_words(ref["accum"], plain["accum"])
    print("%s: weights without 1 / m change %.3f of the rgb words" % (pick_ref.case_id(case), share))
    if m > 1:
        assert share > pick_ref.MIN_CHANGED_NO_SLOTS
    else:
        assert share == 0
    # P3: the counts and the hits are the same whatever is picked
    for other in (shifted, plain):
        assert (other["closest"], other["shadow"]) == (ref["closest"], ref["shadow"])
        assert (other["accum"][..., 3] == ref["accum"][..., 3]).all()


def test_caller_importance_and_the_default_give_different_frames():
    a, b = [c for c in pick_ref.CASES if c[0] == ("lowres", False, 6)]
    assert (a[7] is None) != (b[7] is None)
    assert (pick_ref.case_picks(a) != pick_ref.case_picks(b)).any()
    assert pick_ref.changed_rgb_words(pick_ref.case_reference(a)["accum"], pick_ref.case_reference(b)["accum"]) > pick_ref.MIN_CHANGED_SHIFT


def test_the_estimator_estimates_the_frame():
    """Where the clamp never acts, the picked frame is the frame of all lights up to noise of the frame's own size — and
    the frame built without the 1 / m of the weight is not."""
    c = pick_ref.ESTIMATE_CASE
    p = pick_ref.case_params(c)
    k = pick_ref.case_picks(c)
    picked = pick_ref.case_reference(c)
    plain = pick_ref.build(c, pick_ref.case_table(c, drop_slots=True)["lights"], k, tag="no 1/m")
    full, other = pick_ref.full_frame(c), pick_ref.full_frame(c, seed=pick_ref.SEED + 1)
    peak_full = 0.0
    for i in range(p.spp):
        _, acc, _ = orc.render(pick_ref.case_scene(c), pick_ref._one_sample(p, i), math_mode=orc.MATH_DET, accel=orc.ACCEL_OBVH)
        peak_full = max(peak_full, float(acc[..., :3].max()))
    print("largest per-sample value: %.3f over the tuples' frames, %.3f over the full list's, %.3f without 1 / m" % (
        picked["peak"], peak_full, plain["peak"]))
    assert picked["peak"] < 1 and peak_full < 1 and plain["peak"] < 1, "the clamp acts"
    assert (picked["accum"][..., 3] == full["accum"][..., 3]).all()

    def distance(a, b):
        return float(np.abs(a["accum"][..., :3].astype(F64) - b["accum"][..., :3].astype(F64)).mean() / p.spp)

    yard, got, wrong = distance(full, other), distance(picked, full), distance(plain, full)
    print("picked against full %.5f, yardstick %.5f, without 1 / m %.5f" % (got, yard, wrong))
    assert yard > 0
    assert got <= pick_ref.ESTIMATE_MULTIPLE * yard
    assert wrong > pick_ref.ESTIMATE_MULTIPLE * yard


def _lights(n):
    return pick_ref.many_lights(pick_ref.scene_lights(pick_ref.scene(("cubes", False, 3), 8, 8)), n)


def test_a_tiny_probability_shares_its_predecessors_threshold_and_is_never_picked():
    q = np.array([1.0, 1e-12, 1.0], F32)
    t = pick_ref.table(_lights(3), 2, q)
    assert t["p"][1] > 0 and t["thresholds"][1] == t["thresholds"][0] and t["thresholds"][2] == 1
    u = np.array([0.0, np.nextafter(t["thresholds"][0], F32(0)), t["thresholds"][0], 0.99999994], F32)
    assert list(pick_ref.pick(t["thresholds"], u)) == [0, 0, 2, 2]
    assert np.isfinite(t["weights"]).all()  # (its weight is large and finite: it scales a light that no u reaches)


def test_a_zero_first_importance_and_zero_tails():
    q = np.array([0.0, 2.0, 0.0, 2.0, 0.0], F32)
    t = pick_ref.table(_lights(5), 1, q)
    assert list(t["thresholds"]) == [0.0, 0.5, 0.5, 1.0, 1.0]
    assert list(pick_ref.pick(t["thresholds"], np.array([0.0, 0.49999997, 0.5, 0.99999994], F32))) == [1, 1, 3, 3]
    assert list(t["weights"]) == [1.0, 2.0, 1.0, 2.0, 1.0]
    L = _lights(5)
    assert (t["lights"][[0, 2, 4]] == L[[0, 2, 4]]).all()
    assert (t["lights"][1, pick_ref.COLOR] == (F32(2) * L[1, pick_ref.COLOR]).astype(F32)).all()
    # the last light that can be picked takes every u up to 1, whatever the running sum rounds to
    q = np.full(10, 0.1, F32)
    assert pick_ref.table(_lights(10), 3, q)["thresholds"][-1] == 1


def test_all_black_lights_are_picked_uniformly():
    L = _lights(4)
    L[:, pick_ref.COLOR] = 0
    assert (pick_ref.default_importance(L) == 1).all()
    t = pick_ref.table(L, 2)
    assert list(t["thresholds"]) == [0.25, 0.5, 0.75, 1.0] and (t["weights"] == 2).all()
    # a light whose default importance is not finite or not positive counts as 0
    L = _lights(4)
    L[0, pick_ref.INTENSITY], L[1, pick_ref.SIDE], L[2, pick_ref.COLOR] = np.inf, 0.0, (-1.0, -1.0, 1.0)
    q = pick_ref.default_importance(L)
    assert list(q[:3]) == [0, 0, 0] and q[3] > 0
    assert list(pick_ref.table(L, 1)["thresholds"]) == [0, 0, 0, 1]


def test_the_table_keeps_every_other_word_of_a_light():
    L = _lights(6)
    t = pick_ref.table(L, 3)
    rest = np.ones(21, bool)
    rest[pick_ref.COLOR] = False
    assert (t["lights"][:, rest] == L[:, rest]).all()
    w = (1.0 / (3.0 * t["p"])).astype(F32)
    assert (t["weights"] == w).all() and (t["lights"][:, pick_ref.COLOR] == (w[:, None] * L[:, pick_ref.COLOR]).astype(F32)).all()
    assert abs(float((t["p"] * t["weights"].astype(F64) * 3).mean()) - 1) < 1e-6
    assert lens_ref.SPP7_34 is pick_ref.SPP7_34
