"""tests/probe_card.py against the references alone (no GPU): the card reaches every limit its table names, counted by the
references' own parts (tex_ref.sample(parts=True), nmap_ref.frame's events, mat_ref.frame's nonfinite), so that
tests/test_gpu_surface_limits.py cannot pass by missing its target.  These are conditions on the card, not measurements
of the library: the card's geometry and uvs were adjusted until the references met them, and they stay fixed.  Then the
float32 sampler against a float64 evaluation of the header's formula on the card's own first hits."""
import numpy as np
import pytest

import aov_ref
import mat_ref
import nmap_ref
import probe_card as pc
import tex_ref

F32, F64 = np.float32, np.float64
EPS = float(np.finfo(F32).eps)
AT_LEAST = 8  # occurrences of an event
FRAMES = [(nl, spp) for nl in (3, 1) for spp in (1, 4)]
_frames = {}


def frame_id(f):
    return "%d-lights-spp%d" % f


def frames(nl, spp):
    """(textured, material, normal-mapped) reference frames of the card at path depth 3, computed once."""
    if (nl, spp) not in _frames:
        s, p, m = pc.scene(nl), pc.params(spp, 3), pc.map_set()
        _frames[nl, spp] = (tex_ref.frame(s, p, m, touched=False), mat_ref.frame(s, p, m), nmap_ref.frame(s, p, m))
    return _frames[nl, spp]


def test_the_card_is_what_its_table_says():
    s, m = pc.scene(3), pc.map_set()
    a = s.arrays()
    assert len(a["tri_begin"]) - 1 == pc.N_QUADS + 2 and len(a["pos"]) == 4 * (pc.N_QUADS + 2) and len(a["tri"]) == 2 * (pc.N_QUADS + 2)
    assert len(pc.scene(1).arrays()["lights"]) == 1 and len(a["lights"]) == 3
    assert np.abs(m["uv"]).max() == 1024 and np.isfinite(m["uv"]).all()  # the set's own bound, reached
    assert all(np.isfinite(t[0]).all() for t in m["textures"])
    shapes = {t[0].shape[:2] for t in m["textures"]}
    assert {(1, 16384), (16384, 1), (2, 16384), (16384, 2), (1, 1), (5, 1), (1, 5), (2, 3), (5, 7)} <= shapes
    for table in pc.TABLES:
        assert (m[table][pc.N_QUADS:] == pc.NONE).all()
    # every quad is seen: about 7 x 7 pixels, the two B1 quads (seen from the side) half of that
    per_mesh = np.bincount(pc.first_hits(s, pc.one_sample())["mesh"], minlength=pc.N_QUADS + 2)
    print(per_mesh)
    assert (per_mesh[:pc.N_QUADS] >= 24).all() and np.median(per_mesh[:pc.N_QUADS]) >= 49
    assert pc.first_hits(s, pc.one_sample())["hit"].all()  # (the wall closes the view)


@pytest.mark.parametrize("p", [pc.one_sample(), pc.params(4, 3)], ids=["spp1", "spp4"])
def test_sampler_events_at_the_first_hits(p):
    """Every event on s and on t, at AT_LEAST first hits.  The largest |s W| is 2^24 exactly: a set's uvs are bounded by
    1024 and its sides by 16384, and barycentrics keep a hit's coordinate between its vertices', so no resident set can
    go beyond (the 2^27 of include/rt_amd.h bounds the expression for u, v anywhere in [0, 1], which no hit has)."""
    counts, largest = pc.sampler_events(pc.map_set(), pc.first_hits(pc.scene(3), p))
    for ax in "st":
        print(ax, counts[ax], largest[ax])
        for name in pc.SAMPLER_EVENTS:
            assert counts[ax][name] >= AT_LEAST, (ax, name, counts[ax])
        assert largest[ax] == 2.0 ** 24, (ax, largest)


def test_the_event_counters_mean_what_they_say():
    """sampler_events on hand-made coordinates of a 4 x 1 texture, one event each."""
    tex = (np.arange(12, dtype=F32).reshape(1, 4, 3), tex_ref.REPEAT, tex_ref.CLAMP, tex_ref.BILINEAR)
    s = np.array([-0.125, 1.125, 0.0, 0.375, 0.25, 0.3], F32)  # x = -1, 4, -0.5, 1, 0.5, 0.7
    c, parts = tex_ref.sample(tex, s, np.full(6, 0.5, F32), parts=True)
    assert parts["xi"].tolist() == [-1, 4, -1, 1, 0, 0] and parts["i0"].tolist() == [3, 0, 3, 1, 0, 0] and parts["i1"].tolist() == [0, 1, 0, 2, 1, 1]
    assert parts["fx"].tolist() == [0, 0, 0.5, 0, 0.5, F32(F32(1.2) - F32(0.5))]
    assert parts["yj"].tolist() == [0] * 6 and (parts["j0"] == 0).all() and (parts["j1"] == 0).all() and (parts["fy"] == 0).all()
    assert np.array_equal(c[3], tex[0][0, 1]) and np.array_equal(c[2], ((tex[0][0, 3] + tex[0][0, 0]) / 2))
    near = (tex[0], tex_ref.CLAMP, tex_ref.REPEAT, tex_ref.NEAREST)
    c, parts = tex_ref.sample(near, np.array([-0.01, 0.5, 1.0], F32), np.array([-1.0, 0.0, 2.5], F32), parts=True)
    assert parts["xi"].tolist() == [-1, 2, 4] and parts["i0"].tolist() == [0, 2, 3] and parts["yj"].tolist() == [-1, 0, 2]
    assert not parts["bilinear"] and np.array_equal(c, tex[0][0, [0, 2, 3]])
    # without parts: the same sample, bit for bit
    assert np.array_equal(c, tex_ref.sample(near, np.array([-0.01, 0.5, 1.0], F32), np.array([-1.0, 0.0, 2.5], F32)))


def bend_at_first_hits(quad, p=None):
    """(N, N', parts) of nmap_ref.bend at the first hits of one quad."""
    s, m = pc.scene(3), pc.map_set()
    a, fh = s.arrays(), pc.first_hits(s, p or pc.one_sample())
    rows = np.nonzero(fh["mesh"] == quad)[0]
    tv, u, v = fh["tv"][rows], fh["u"][rows], fh["v"][rows]
    wgt = ((F32(1) - u) - v)[:, None]
    n0, n1, n2 = (a["nrm"][tv[:, k]] for k in range(3))
    p0, p1, p2 = (a["pos"][tv[:, k]] for k in range(3))
    N = aov_ref._unit((wgt * n0 + u[:, None] * n1) + v[:, None] * n2)
    mesh = np.full(len(rows), quad, np.int64)
    smp = mat_ref.vertex_sample(m, m["mesh_normal"], mesh, tv, u, v, np.full((len(rows), 3), np.nan, F32))
    uv = m["uv"]
    N2, parts = nmap_ref.bend(N, (p1 - p0).astype(F32), (p2 - p0).astype(F32), uv[tv[:, 0]], uv[tv[:, 1]], uv[tv[:, 2]], smp, parts=True)
    return N, N2, parts


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_b1_the_projected_tangent_is_exactly_zero():
    """On both B1 quads, at every first hit: Tr is along z, N is (0, 0, 1) bit for bit, Tp is exactly 0 and N stays."""
    for quad in pc.B1_QUADS:
        N, N2, parts = bend_at_first_hits(quad)
        assert len(N) >= 24
        assert np.array_equal(bits(N), bits(np.broadcast_to(np.array([0, 0, 1], F32), N.shape)))
        assert (parts["Tr"][:, :2] == 0).all() and (parts["Tr"][:, 2] != 0).all() and (parts["r"] != 0).all()
        assert (parts["Tp"] == 0).all() and parts["tp0"].all() and not parts["r0"].any()
        assert parts["flat"].all() == (pc.QUADS[quad][5] == "flat")
        assert np.array_equal(bits(N), bits(N2))


def test_the_normal_probes_do_what_the_table_says():
    """B2 to B7, each on its own quad's first hits."""
    quad = {name: [q for q, row in enumerate(pc.QUADS) if name in row[0].split()] for name in ("B2", "B3", "B4", "B5", "B6", "B7")}
    # B2: both texels occur; the 1e30 one overflows V's squared length, the other is the smallest x and moves N
    N, N2, parts = bend_at_first_hits(quad["B2"][0])
    huge = parts["xyz"][:, 0] > 1e29
    assert huge.sum() >= AT_LEAST and (~huge).sum() >= AT_LEAST
    assert np.isinf(parts["vv"][huge]).all() and parts["v0"][huge].all() and np.array_equal(bits(N2[huge]), bits(N[huge]))
    assert (parts["xyz"][~huge] == np.array([2.0 ** -23, 0, 0], F32)).all() and not parts["kept"][~huge].any()
    assert (bits(N2[~huge]) != bits(N[~huge])).any(axis=1).all()
    # B3: one triangle of each sign
    N, N2, parts = bend_at_first_hits(quad["B3"][0])
    assert (parts["r"] < 0).sum() >= AT_LEAST and (parts["r"] > 0).sum() >= AT_LEAST and not parts["kept"].any()
    # B4: below the horizon and far from N
    N, N2, parts = bend_at_first_hits(quad["B4"][0])
    below = (parts["xyz"][:, 2] < 0) & ~parts["kept"]
    assert below.sum() >= AT_LEAST and (np.abs(parts["xyz"][:, :2]).max(axis=1) > 3).sum() >= AT_LEAST
    assert ((N2[below] * N[below]).sum(axis=1) < 0).all()
    # B5: N is within 1e-3 of unit3(Tr), so Tp is a residue of the cancellation, and not zero
    N, N2, parts = bend_at_first_hits(quad["B5"][0])
    Tr, Tp = parts["Tr"].astype(F64), parts["Tp"].astype(F64)
    away = np.linalg.norm(N - Tr / np.linalg.norm(Tr, axis=1)[:, None], axis=1)
    assert away.max() < 1e-3 and (np.linalg.norm(Tp, axis=1) < 1e-3 * np.linalg.norm(Tr, axis=1)).all()
    assert not parts["kept"].any() and len(N) >= AT_LEAST
    # B6: r and |Tp|^2 are subnormal and not zero at every hit
    N, N2, parts = bend_at_first_hits(quad["B6"][0])
    tt = nmap_ref._dot(parts["Tp"], parts["Tp"])
    tiny = nmap_ref.TINY
    assert ((parts["r"] != 0) & (np.abs(parts["r"]) < tiny)).all() and ((tt > 0) & (tt < tiny)).all()
    assert not parts["kept"].any() and (bits(N2) != bits(N)).any(axis=1).all() and len(N) >= AT_LEAST
    # B7: two conditions at once, on both quads
    for q in quad["B7"]:
        N, N2, parts = bend_at_first_hits(q)
        two = sum(parts[k].astype(int) for k in ("flat", "r0", "tp0", "v0")) >= 2
        assert two.all() and len(N) >= AT_LEAST and np.array_equal(bits(N2), bits(N)), q
    N, N2, parts = bend_at_first_hits(5)
    assert parts["r0"].all() and parts["v0"].all() and np.isinf(parts["vv"]).all() and not parts["tp0"].any()


@pytest.mark.parametrize("f", FRAMES, ids=frame_id)
def test_normal_events_over_the_paths(f):
    """Every event at AT_LEAST shaded vertices of the normal-mapped frame, all depths together."""
    ev = frames(*f)[2]["events"]
    print(ev)
    assert set(ev) == set(nmap_ref.EVENTS)
    for name in nmap_ref.EVENTS:
        assert ev[name] >= AT_LEAST, (name, ev)
    assert ev["kept_r0"] == frames(*f)[2]["kept_r0"]


@pytest.mark.parametrize("f", FRAMES, ids=frame_id)
def test_frame_content(f):
    """The material frame reaches sums that are not finite (they clamp to 1: fmaxf(fminf(NaN, 1), 0) is 1), and none of the
    three frames is a wash: most words of the card's pixels are finite and neither 0 nor the sample count."""
    nl, spp = f
    tex, mat, nrm = frames(nl, spp)
    print("words not finite before the clamp: %d" % mat["nonfinite"])
    assert mat["nonfinite"] >= 16
    card = (pc.first_hit_mesh(pc.scene(nl), pc.params(spp, 3)) < pc.N_QUADS).any(axis=2)
    assert card.mean() > 0.7
    for name, ref in (("textured", tex), ("material", mat), ("normal-mapped", nrm)):
        rgb = ref["accum"][..., :3]
        assert np.isfinite(ref["accum"]).all()  # (the clamp leaves nothing else)
        live = (np.isfinite(rgb) & (rgb != 0) & (rgb != spp)).all(axis=2)
        print("%-14s %.4f of the card's pixels" % (name, live[card].mean()))
        assert live[card].mean() >= 0.25, name
    assert (bits(mat["accum"]) != bits(tex["accum"])).any() and (bits(nrm["accum"]) != bits(mat["accum"])).any()
    assert (nrm["closest"], nrm["shadow"]) != (mat["closest"], mat["shadow"])


def test_the_sampler_against_float64():
    """The float32 restatement against the header's formula in float64 on the same float32 coordinates, at every first
    hit of all four tables where both choose the same four texels.

    The bound, per hit, with M = max |texel| of the texture and eps = 2^-23: three lerps, each two roundings of operands
    bounded by 2 M, give 16 eps M for EQUAL weights.  The weights are not equal: fx = x - floorf(x) is exact, but
    x = fl(fl(s W) - 0.5) carries two roundings of up to eps / 2 (|s W| + 0.5) each, so |fx32 - fx64| <= eps (|s W| + 0.5),
    and a weight's error moves the sample by at most 2 M times itself (on x through a and b alike, on y through b - a).
    So |c32 - c64| <= M eps (16 + 2 (|s W| + |t H| + 1)).  On the 16384-wide maps at |s| >= 512 the second term says all
    there is to say: x has no fraction bits left, fx32 is 0 where fx64 is 0.5.  The measured maximum of error / bound is
    printed (0.283), with the largest error in units of eps M (7.6e6, on those maps) and the largest on the hits where
    |s W| + |t H| is below 16 (7.3)."""
    s, m = pc.scene(3), pc.map_set()
    worst, worst_small, worst_all, n_same, n_all = 0.0, 0.0, 0.0, 0, 0
    for p in (pc.one_sample(), pc.params(4, 3)):
        fh = pc.first_hits(s, p)
        for table in pc.TABLES:
            for k, (rows, cs, ct, c32, parts) in pc.table_samples(m, table, fh).items():
                tex = m["textures"][k]
                c64, i0, i1, j0, j1 = pc.sample64(tex, cs, ct)
                same = (i0 == parts["i0"]) & (i1 == parts["i1"]) & (j0 == parts["j0"]) & (j1 == parts["j1"])
                n_same, n_all = n_same + int(same.sum()), n_all + len(same)
                if not same.any():
                    continue
                M = float(np.abs(tex[0]).max())
                err = np.abs(c32.astype(F64) - c64).max(axis=1)[same]
                reach = (np.abs(parts["sw"]).astype(F64) + np.abs(parts["th"]).astype(F64))[same]
                bound = M * EPS * (16 + 2 * (reach + 1))
                if tex[3] == tex_ref.NEAREST:
                    assert (err == 0).all(), m["names"][k]
                worst = max(worst, float((err / bound).max()))
                worst_all = max(worst_all, float((err / (M * EPS)).max()))
                if (reach < 16).any():
                    worst_small = max(worst_small, float((err / (M * EPS))[reach < 16].max()))
                assert (err <= bound).all(), (m["names"][k], table, float((err / bound).max()))
    print("same texels at %d of %d samples; largest error / bound %.4f; largest error %.4g eps M, and %.3f eps M where "
          "|s W| + |t H| < 16" % (n_same, n_all, worst, worst_all, worst_small))
    assert n_same >= 0.8 * n_all
