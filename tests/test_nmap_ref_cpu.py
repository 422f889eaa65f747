"""tests/nmap_ref.py against the oracle, mat_ref and a float64 evaluation alone (no GPU).  The reference walks its paths
itself, so before anything trusts it: with no normal maps it is mat_ref.frame on every case bit for bit — accumulator,
image and both ray counts, which validates the restated draw order and light sample against the oracle's own ray dump —
and, where T1 / M1 apply, orc.render of the plain scene; N1 holds on the reference itself (flat maps of every shape, filter
and wrap); every frame is finite; the perturbation alone, on random inputs, means what the header says (|N'| = 1, T
orthogonal to N, dot(N', N) = z / |(x, y, z)|) and keeps N under each of its five conditions; and the mixed cases differ
from the material frame in more than nmap_ref.MIN_CHANGED_N of their rgb words."""
import numpy as np
import pytest

import mat_ref
import nmap_ref
import tex_ref
from tex_ref import T_ALBEDO, T_FACES, T_MIXED, T_NONE

F32, F64 = np.float32, np.float64
MIXED = [c for c in nmap_ref.CASES if c[6] == T_MIXED]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(ref, exp, what):
    assert np.array_equal(bits(ref["accum"]), bits(exp["accum"])), "accum " + what
    assert np.array_equal(bits(ref["out"]), bits(exp["out"])), "out " + what
    assert (ref["closest"], ref["shadow"]) == (exp["closest"], exp["shadow"]), what


# ---- the walk --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("brute", [False, True], ids=["bvh", "loop"])
@pytest.mark.parametrize("case", nmap_ref.CASES, ids=nmap_ref.case_id)
def test_without_normal_maps_it_is_the_material_reference(case, brute):
    """mesh_normal None (even cases) or RT_TEX_NONE everywhere (odd cases): mat_ref.frame, whose rays are the oracle's."""
    s, p, bg = nmap_ref.case_scene(case), nmap_ref.case_params(case), nmap_ref.case_background(case)
    mset = dict(nmap_ref.case_maps(case))
    odd = nmap_ref.CASES.index(case) % 2 == 1
    mset["mesh_normal"] = np.full(len(mset["mesh_texture"]), nmap_ref.NONE, np.uint32) if odd else None
    got = nmap_ref.frame(s, p, mset, bg, brute)
    same(got, mat_ref.case_reference(case, brute), nmap_ref.case_id(case))
    assert got["bent"] == 0
    if case[6] in (T_NONE, T_ALBEDO):  # (with T1 and M1: the oracle's own frame)
        same(got, tex_ref.plain_frame(s, case, brute), "against the plain frame " + nmap_ref.case_id(case))


@pytest.mark.parametrize("case", nmap_ref.CASES[::2], ids=nmap_ref.case_id)
def test_n1_flat_maps_are_the_material_reference(case):
    s, p, bg = nmap_ref.case_scene(case), nmap_ref.case_params(case), nmap_ref.case_background(case)
    mset = nmap_ref.flat_set(mat_ref.case_maps(case), s, nmap_ref.CASES.index(case))
    assert (mset["mesh_normal"] != nmap_ref.NONE).all()
    got = nmap_ref.frame(s, p, mset, bg)
    same(got, mat_ref.case_reference(case), nmap_ref.case_id(case))
    assert got["bent"] == 0


@pytest.mark.parametrize("case", nmap_ref.CASES, ids=nmap_ref.case_id)
def test_every_reference_frame_is_finite(case):
    ref = nmap_ref.case_reference(case)
    assert np.isfinite(ref["accum"]).all() and np.isfinite(ref["out"]).all()


def test_the_sets_cover_what_they_claim():
    nx = len(tex_ref.MIXED_TEXTURES)
    used, degenerate, kept = set(), 0, 0
    events = dict.fromkeys(nmap_ref.EVENTS, 0)
    for case in nmap_ref.CASES:
        t, base = nmap_ref.case_maps(case), mat_ref.case_maps(case)
        n0 = len(base["textures"])
        assert len(t["textures"]) == n0 + nx + 1
        for k in range(nx):
            (w, h), ws, wt, f = tex_ref.MIXED_TEXTURES[k]
            x, xs, xt, xf = t["textures"][n0 + k]
            assert x.shape == (h, w, 3) and (xs, xt, xf) == (ws, wt, f)
            assert 0 <= x[..., :2].min() and x[..., :2].max() < 1 and 0.5 <= x[..., 2].min() and x[..., 2].max() < 1
        assert np.array_equal(t["textures"][n0 + nx][0], np.broadcast_to(np.array(nmap_ref.FLAT, F32), (2, 2, 3)))
        mn = t["mesh_normal"]
        assert len(mn) >= 4 and mn[2] == nmap_ref.NONE and mn[3] == n0 + nx and (mn != nmap_ref.NONE).sum() == len(mn) - 1
        used |= {int(x) - n0 for x in mn if x != nmap_ref.NONE}
        degenerate += nmap_ref.degenerate_triangles(nmap_ref.case_scene(case), t)
        if case[6] != T_FACES:
            kept += nmap_ref.case_reference(case)["kept_r0"]
            for name, n in nmap_ref.case_reference(case)["events"].items():
                events[name] += n
    assert used == set(range(nx + 1))  # every shape, both filters, both wraps, and the flat map
    assert degenerate > 0
    assert kept > 0, "no case beside the strips shades a vertex of a triangle with degenerate uvs"
    # ... and each keep condition on its own (nmap_ref.EVENTS).  These cases reach the degenerate uv triangle, the flat
    # texel and mirrored uvs; a vanishing Tp, an overflowing V, z < 0 and subnormal terms are tests/probe_card.py's
    print(events)
    assert events["kept_r0"] == kept and events["kept_flat"] > 0 and events["r_neg"] > 0


# ---- the perturbation alone ------------------------------------------------------------------------------------------------
def random_inputs(n, seed):
    g = np.random.default_rng(seed)
    N = g.normal(size=(n, 3))
    N = (N / np.linalg.norm(N, axis=1)[:, None]).astype(F32)
    N = nmap_ref.aov_ref._unit(N)
    e1, e2 = g.normal(size=(n, 3)).astype(F32), g.normal(size=(n, 3)).astype(F32)
    uv = g.uniform(-2, 3, (3, n, 2)).astype(F32)
    m = np.stack([g.uniform(0, 1, n), g.uniform(0, 1, n), g.uniform(0.5, 1, n)], axis=1).astype(F32)
    return N, e1, e2, uv, m


def test_the_perturbation_against_float64():
    """What the formula means, without stating it twice: N' is unit, T is orthogonal to N, and the cosine between N' and N
    is z / |(x, y, z)| — true of any orthonormal (T, B, N), whatever T's direction in the tangent plane."""
    N, e1, e2, uv, m = random_inputs(4000, 5)
    got, parts = nmap_ref.bend(N, e1, e2, uv[0], uv[1], uv[2], m, parts=True)
    # (triangles whose projected tangent nearly vanishes lose T's direction to cancellation: not the property under test)
    Tr = (uv[2][:, 1] - uv[0][:, 1])[:, None].astype(F64) * e1 - (uv[1][:, 1] - uv[0][:, 1])[:, None].astype(F64) * e2
    Tp = Tr - (N.astype(F64) * Tr).sum(axis=1)[:, None] * N
    ok = ~parts["kept"] & (np.linalg.norm(Tp, axis=1) > 1e-2 * np.linalg.norm(Tr, axis=1))
    assert ok.sum() > 3000
    g64, N64, T64 = got[ok].astype(F64), N[ok].astype(F64), parts["T"][ok].astype(F64)
    assert np.abs(np.linalg.norm(g64, axis=1) - 1).max() < 4 * np.finfo(F32).eps
    assert np.abs((T64 * N64).sum(axis=1)).max() < 1e-5
    xyz = 2.0 * m[ok].astype(F64) - 1.0
    assert np.abs((g64 * N64).sum(axis=1) - xyz[:, 2] / np.linalg.norm(xyz, axis=1)).max() < 1e-5
    # B completes a frame on the side of the uv bitangent
    B64 = parts["B"][ok].astype(F64)
    assert np.abs(np.linalg.norm(B64, axis=1) - 1).max() < 1e-5 and np.abs((B64 * T64).sum(axis=1)).max() < 1e-5


def test_the_perturbation_keeps_n_under_each_condition():
    N, e1, e2, uv, m = random_inputs(64, 6)
    base = nmap_ref.bend(N, e1, e2, uv[0], uv[1], uv[2], m)
    assert (bits(base) != bits(N)).any(axis=1).all()

    def kept(**kw):
        args = dict(N=N, e1=e1, e2=e2, uv0=uv[0], uv1=uv[1], uv2=uv[2], m=m)
        args.update(kw)
        return np.array_equal(bits(nmap_ref.bend(**args)), bits(N))

    assert kept(m=np.full_like(m, np.nan))  # RT_TEX_NONE
    flat = m.copy()
    flat[:, :2] = 0.5
    assert kept(m=flat)  # x == 0 && y == 0, any z
    assert kept(uv2=uv[1]) and kept(uv1=uv[0], uv2=uv[0])  # r == 0
    assert kept(uv1=np.full_like(uv[1], np.nan))  # r is NaN
    assert kept(e1=np.zeros_like(e1), e2=np.zeros_like(e2))  # Tp == 0
    axis = np.broadcast_to(np.array([0, 0, 1], F32), N.shape)  # (edges along an axis-aligned N project to exactly 0)
    assert np.array_equal(bits(nmap_ref.bend(axis, axis, (F32(2) * axis).astype(F32), uv[0], uv[1], uv[2], m)), bits(axis))
    # V not finite: edges whose raw tangent overflows (b1 is near 500) leave a T of NaN
    huge = np.full_like(e1, 3e38)
    assert kept(e1=huge, e2=-huge, uv1=(uv[1] + F32(500)).astype(F32))


# ---- the change floor ------------------------------------------------------------------------------------------------------
def test_the_mixed_maps_change_the_material_frame():
    shares = {}
    for case in MIXED:
        ref, base = nmap_ref.case_reference(case), nmap_ref.case_material_reference(case)
        same(base, mat_ref.case_reference(case), "the appended textures change nothing")
        shares[nmap_ref.case_id(case)] = nmap_ref.changed_rgb_words(ref["accum"], base["accum"])
        assert ref["bent"] > 0
        if case[4] == tex_ref.PATH and case[5] > 1:  # the bounce moved: other rays
            assert (ref["closest"], ref["shadow"]) != (base["closest"], base["shadow"]) or (bits(ref["accum"]) != bits(base["accum"])).any()
    for cid, share in shares.items():
        print("%-48s %.4f" % (cid, share))
    low = min(shares.values())
    print("smallest share: %.4f (floor %.4f)" % (low, nmap_ref.MIN_CHANGED_N))
    assert low > nmap_ref.MIN_CHANGED_N, shares
    assert nmap_ref.MIN_CHANGED_N >= 0.45 * low, "the floor is half the smallest share: %r" % shares
