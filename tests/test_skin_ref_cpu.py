"""tests/skin_ref.py checked on its own, without a GPU: the restatement against transform_ref.apply where the two must
agree, its rules for zero weights, and — for every pose tests/test_gpu_skin.py compares on the device — the conditions that
keep a kernel that skips the blend, drops a slot or blends in another order from passing there."""
import numpy as np
import pytest

import pyrt
import skin_ref as sk
import transform_ref as xf


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def lowres():
    return pyrt.Scene("lowres", 24, 24).arrays()


def mesh_of_vertex(a):
    counts = np.diff(a["vtx_begin"].astype(np.int64))
    return np.repeat(np.arange(len(counts)), counts)


@pytest.mark.parametrize("slot", range(sk.SLOTS))
def test_single_unit_weight_is_the_rigid_transform(lowres, slot):
    """Every vertex on the bone of its mesh alone, weight 1 in one slot: transform_ref.apply with the bones as the meshes'
    matrices, bit for bit except where that gives -0 (the blend starts from +0, and +0 + -0 = +0)."""
    a = dict(lowres)
    a["pos"], a["nrm"] = a["pos"].copy(), a["nrm"].copy()
    n = len(a["vtx_begin"]) - 1
    t = sk.random_bones(n, 3)
    # mesh 1 under the identity with a translation of -0: rest coordinates of -0 stay -0 in the rigid transform
    t["m"][1], t["n"][1] = np.eye(3, 4, dtype=np.float32), np.eye(3, dtype=np.float32)
    t["m"][1, :, 3] = np.float32(-0.0)
    b = int(a["vtx_begin"][1])
    a["pos"][b], a["nrm"][b] = np.float32(-0.0), np.float32(-0.0)
    mesh = mesh_of_vertex(a)
    bone, weight = np.zeros((len(mesh), sk.SLOTS), np.uint16), np.zeros((len(mesh), sk.SLOTS), np.float32)
    bone[:, slot], weight[:, slot] = mesh, 1.0
    pos, nrm = sk.apply(a, bone, weight, t)
    rpos, rnrm = xf.apply(a, t)
    assert np.array_equal(pos, rpos) and np.array_equal(nrm, rnrm)  # in value (-0 == +0)
    for got, ref in ((pos, rpos), (nrm, rnrm)):
        keep = ~(np.signbit(ref) & (ref == 0))
        assert np.array_equal(bits(got)[keep], bits(ref)[keep])
        assert not np.signbit(got[~keep]).any()  # +0 + (1 * -0) = +0
    assert (np.signbit(rpos) & (rpos == 0)).any(), "no -0 among the rigid results: the case above is not exercised"


def test_all_zero_vertices_keep_their_bits(lowres):
    a = dict(lowres)
    a["pos"], a["nrm"] = a["pos"].copy(), a["nrm"].copy()
    a["pos"][::5, 1] = np.float32(-0.0)
    a["nrm"][1::5, 2] = np.float32(-0.0)
    bone, weight = sk.random_skin(len(a["pos"]), 9, 4)
    still = ~sk.skinned_rows(weight)
    assert still.sum() > 10 and (np.signbit(weight[still]).any()) and (~still).sum() > 10
    pos, nrm = sk.apply(a, bone, weight, sk.random_bones(9, 1))
    assert np.array_equal(bits(pos[still]), bits(a["pos"][still])) and np.array_equal(bits(nrm[still]), bits(a["nrm"][still]))
    assert (np.signbit(pos[still]) & (pos[still] == 0)).any()
    assert not np.array_equal(pos[~still], a["pos"][~still])


def test_zero_weight_slots_do_not_count(lowres):
    a = lowres
    bone, weight = sk.random_skin(len(a["pos"]), 9, 5)
    bones = sk.random_bones(9, 2)
    ref = sk.apply(a, bone, weight, bones)
    rng = np.random.default_rng(0)
    other = np.where(weight == 0, rng.integers(0, 9, bone.shape), bone).astype(np.uint16)
    assert (other != bone).any()
    got = sk.apply(a, other, weight, bones)
    assert np.array_equal(bits(got[0]), bits(ref[0])) and np.array_equal(bits(got[1]), bits(ref[1]))
    # ... nor does the sign of the zero
    flipped = np.where(weight == 0, -weight, weight)
    assert (np.signbit(flipped) != np.signbit(weight)).any()
    got = sk.apply(a, bone, flipped, bones)
    assert np.array_equal(bits(got[0]), bits(ref[0])) and np.array_equal(bits(got[1]), bits(ref[1]))


def test_the_random_rig_has_what_the_device_cases_need():
    bone, weight = sk.random_skin(513, 65536, 7)
    counts = (weight != 0).sum(axis=1)
    for wave in range(0, 513 - 63, 64):
        assert set(counts[wave:wave + 64]) == {0, 1, 2, 3, 4}, wave  # the lanes of every whole wave take 0 .. 4 slots
    gaps = (weight[:, 0] != 0) & (weight[:, 1] == 0) & (weight[:, 2] != 0)
    assert gaps.any() and np.signbit(weight[weight == 0]).any() and not np.signbit(weight[weight == 0]).all()
    assert (bone[weight != 0] == 65535).any() and (weight == 1).any()
    nz = weight[(weight != 0) & (weight != 1)]
    assert (nz > 0.1).all() and (nz < 0.9).all()


CASES = list(sk.all_cases())


@pytest.mark.parametrize("name,a,bone,weight,bones", CASES, ids=[c[0] for c in CASES])
def test_device_cases_tell_a_wrong_kernel(name, a, bone, weight, bones):
    pos, nrm = sk.apply(a, bone, weight, bones)
    assert np.isfinite(pos).all() and np.isfinite(nrm).all()
    skinned = sk.skinned_rows(weight)
    assert skinned.any()
    # a kernel that copies the rest pose
    moved = bits(pos[skinned]) != bits(a["pos"][skinned])
    assert moved.mean() > 0.5, moved.mean()
    # a kernel that takes one slot for the blend: every blended vertex against the pose of each of its bones alone
    blended = (weight != 0).sum(axis=1) >= 2
    if name.startswith("bend"):
        assert blended[skinned].all() and ((weight[skinned, :2] > 0.1) & (weight[skinned, :2] < 0.9)).all()
    assert blended.any()
    for k in range(sk.SLOTS):
        rows = blended & (weight[:, k] != 0)
        if not rows.any():
            continue
        one = np.zeros_like(weight)
        one[rows, k] = 1.0
        single, _ = sk.apply(a, bone, one, bones)
        differ = bits(pos[rows]) != bits(single[rows])
        assert differ.mean() > 0.5, (k, differ.mean())
    # a kernel that pairs weights and slots wrongly: the weights of slots 0 and 1 exchanged.  (Under a table of ONE bone no
    # pairing can show: every slot blends the same P, w0 P + w1 P is w1 P + w0 P bit for bit, and a weight that moves to an
    # empty slot meets the same bone there — so there the exchange must change nothing, and the pairing is the other
    # cases' to tell.)
    swapped = weight.copy()
    swapped[:, [0, 1]] = weight[:, [1, 0]]
    spos, _ = sk.apply(a, bone, swapped, bones)
    assert np.array_equal(bits(spos), bits(pos)) == (len(bones) == 1)
