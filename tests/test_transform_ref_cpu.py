"""tests/transform_ref.py against the other spellings of the same rotation, without a GPU."""
import numpy as np

import pyrt
import transform_ref
from test_gpu_update import turned


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def dot_loop(R, p):
    """The reference's `dot` (Vec3.h: (a.x b.x + a.y b.y) + a.z b.z) of each row of R with p, one float32 operation at a time."""
    f = np.float32
    return [f(f(f(f(R[i][0]) * f(p[0])) + f(f(R[i][1]) * f(p[1]))) + f(f(R[i][2]) * f(p[2]))) for i in range(3)]


def test_rotation_reproduces_turned_on_lowres():
    """apply with m = n = rotationY's rows on slot 3 of lowres equals, bit for bit, a scalar Python loop of the reference's
    dot over the same rest arrays (the zero translation changes no bit of a value that is not -0).
    test_gpu_update.turned spells the product as numpy's float32 matmul, which does NOT keep that association (its BLAS
    kernel fuses or reorders): measured on lowres, positions differ by up to 63 ulp at 5 degrees and 17 ulp at 20 degrees,
    normals by up to 52 and 119 ulp (cancelling sums), nothing at 90 degrees — in 241 to 336 of the 1,923 values.  So the
    bit match is asserted against the loop only; against turned the test prints the gap and holds it to the rounding bound
    of two such evaluations, at most three roundings of 2^-24 (|x| + |z|) each: |gap| <= 2^-21 (|x| + |z|)."""
    s = pyrt.Scene("lowres", 24, 24)
    a = s.arrays()
    b, e = int(a["vtx_begin"][3]), int(a["vtx_begin"][4])
    for deg in (5.0, 20.0, 90.0):
        R = transform_ref.rotation_y(deg)
        t = transform_ref.set_mesh(pyrt.make_transforms(len(a["vtx_begin"]) - 1), 3, R)
        pos, nrm = transform_ref.apply(a, t)
        tp, tn = turned(a, deg)
        gap = np.abs(bits(pos).astype(np.int64) - bits(tp).astype(np.int64)).max()
        print("deg %g: largest gap to numpy's matmul %d ulp" % (deg, gap))
        loop = np.array([dot_loop(R, p) for p in a["pos"][b:e]], np.float32) + np.float32(0)
        assert np.array_equal(bits(pos[b:e]), bits(loop))
        loopn = np.array([dot_loop(R, p) for p in a["nrm"][b:e]], np.float32)
        assert np.array_equal(bits(nrm[b:e]), bits(loopn))
        for got, ref, rest in ((pos, tp, a["pos"]), (nrm, tn, a["nrm"])):
            assert np.array_equal(bits(got[:b]), bits(ref[:b])) and np.array_equal(bits(got[e:]), bits(ref[e:]))
            bound = np.float32(2.0 ** -21) * (np.abs(rest[b:e, 0]) + np.abs(rest[b:e, 2]))
            assert (np.abs(got[b:e].astype(np.float64) - ref[b:e]) <= bound[:, None]).all()
        # n = identity: "normals are left as loaded" up to the sign of zero
        t = transform_ref.set_mesh(pyrt.make_transforms(len(a["vtx_begin"]) - 1), 3, R, normal=np.eye(3))
        pos2, nrm2 = transform_ref.apply(a, t)
        assert np.array_equal(bits(pos2), bits(pos)) and np.array_equal(nrm2, a["nrm"])
    s.close()


def test_negative_zero_under_identity_and_static():
    a = dict(pos=np.array([[-0.0, 1.0, -0.0], [2.0, -0.0, 3.0]], np.float32), nrm=np.array([[-0.0, -0.0, 1.0], [0.0, 1.0, -0.0]], np.float32),
             vtx_begin=np.array([0, 1, 2], np.uint32))
    t = pyrt.make_transforms(2)
    assert (t["flags"] == pyrt.XF_STATIC).all()
    pos, nrm = transform_ref.apply(a, t)
    assert np.array_equal(bits(pos), bits(a["pos"])) and np.array_equal(bits(nrm), bits(a["nrm"]))
    t["flags"][:] = 0  # identity matrices, not static
    pos, nrm = transform_ref.apply(a, t)
    assert np.array_equal(pos, a["pos"]) and np.array_equal(nrm, a["nrm"])
    assert not np.signbit(pos).any() and not np.signbit(nrm).any()
    assert np.signbit(a["pos"]).sum() == 3
    t["flags"][1] = pyrt.XF_STATIC
    pos, _ = transform_ref.apply(a, t)
    assert np.array_equal(bits(pos[1]), bits(a["pos"][1])) and not np.signbit(pos[0]).any()
