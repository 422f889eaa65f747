"""The synthetic filter cases (tests/filter_cases.py) through the numpy restatements alone, no GPU: every case reaches the
edge its overlays and settings name, the case lists together take every branch and every comparison edge the restatements
count, and the float32 evaluation stays within the recorded T of the float64 one (the tolerance of
tests/test_gpu_filter_cases.py, which is never derived from the device)."""
import numpy as np
import pytest

import aov_ref
import filter_cases as fc
import svgf_ref as sv
import temporal_ref as tr

ids = lambda cases: [c["name"] for c in cases]


def failed(c, filt, info, finfo=None):
    n = c["size"][0] * c["size"][1]
    src = dict(t=info, a=info, f=finfo)
    return [(where, name, src[where][name]) for where, (name, test) in fc.expectations(c, filt) if not test(src[where][name], n)]


def test_the_case_lists_hold_what_they_promise():
    sizes = set(fc.S.values())
    for cases in (fc.SVGF_CASES, fc.TEMPORAL_CASES, fc.DENOISE_CASES):
        names = ids(cases)
        assert len(set(names)) == len(names)
        assert {c["size"] for c in cases} <= sizes
        assert all(w * h <= 130 * 21 or (w, h) == (513, 3) for w, h in (c["size"] for c in cases))
        assert sum(n.startswith("default_sigmas") for n in names) == 1
    assert {c["size"] for c in fc.SVGF_CASES} == sizes
    assert set(fc.T_SVGF) == set(ids(fc.SVGF_CASES)) and set(fc.T_DENOISE) == set(ids(fc.DENOISE_CASES))
    used = {o for cases in (fc.SVGF_CASES, fc.TEMPORAL_CASES, fc.DENOISE_CASES) for c in cases for o in c["overlays"]}
    assert used == set(fc.OVERLAYS) - {"FOLLOW"}
    kws = lambda k, cases: {c["kw"].get(k, 0) for c in cases}
    assert kws("max_history", fc.SVGF_CASES) >= {0, 1, 4, 1000} and kws("max_history", fc.TEMPORAL_CASES) >= {0, 1, 4, 1000}
    assert kws("alpha_min", fc.SVGF_CASES) >= {0, 0.4, 1.0} and kws("alpha_min", fc.TEMPORAL_CASES) >= {0, 0.4, 1.0}
    assert kws("alpha_min_moments", fc.SVGF_CASES) >= {0, 1.0}
    assert kws("iterations", fc.SVGF_CASES) >= {0, 1, 2, 8} and kws("denoise_iterations", fc.DENOISE_CASES) >= {1, 5, 8}
    for names, cases in ((fc.DEVICE_FORM_CASES, fc.SVGF_CASES), (fc.ONE_CONTEXT_ORDER, fc.SVGF_CASES),
                         (fc.DENOISE_DEVICE_FORM_CASES, fc.DENOISE_CASES), (fc.DENOISE_ONE_CONTEXT_ORDER, fc.DENOISE_CASES)):
        assert set(names) <= set(ids(cases))


def test_the_inputs_are_in_range_and_deterministic():
    for c in fc.SVGF_CASES:
        b, b2 = fc.build(c), fc.build(c)
        w, h = c["size"]
        assert b["rgb"].shape == (h, w, 3) and b["rgb"].min() >= 0 and b["rgb"].max() <= 1
        hits = b["sums"]["hits"]
        assert set(np.unique(hits)) <= {0, 1, 4, 7}
        mean = b["sums"]["albedo"][hits > 0] / hits[hits > 0, None]
        if c["low_albedo"]:
            assert (mean < 1e-3).any() and (sv.demodulate(b["rgb"], b["sums"])[0][hits > 0] == np.float32(1e-3)).any()
        else:
            assert mean.size == 0 or (mean.min() >= 0.2 - 1e-6 and mean.max() <= 1 + 1e-6)
        assert ("holes_all" in c["overlays"]) or 1 <= len(np.unique(b["cur"]["mesh"][b["cur"]["mesh"] != sv.MISS])) <= 4
        assert w < 64 or h < 2 or len(np.unique(b["svgf_hist"]["mesh"])) >= 2
        assert (b["cur"]["mesh"][hits == 0] == sv.MISS).all()  # (as the renderer's passes relate)
        for k in ("svgf_hist", "temporal_hist", "cur", "sums"):
            for ch, v in b[k].items():
                assert np.array_equal(v, b2[k][ch], equal_nan=v.dtype.kind == "f"), (c["name"], k, ch)
                if ch != "motion":
                    assert np.isfinite(v).all() if v.dtype.kind == "f" else True
        if b["scene"] is None:
            assert b["svgf_kw"]["sigma_position"] == fc.SIGMA_POSITION and b["svgf_kw"]["sigma_reproject"] == 0.5
    assert any((fc.build(c)["cur"]["mesh"] == 0xfffffffe).any() for c in fc.SVGF_CASES)


@pytest.mark.parametrize("c", fc.SVGF_CASES, ids=ids(fc.SVGF_CASES))
def test_svgf_case_reaches_its_edge_and_holds_its_T(c):
    b = fc.build(c)
    A, o64, o32 = fc.svgf_refs(b)
    assert failed(c, "svgf", A["info"], o64["filter_info"]) == []
    assert o64["filter_info"] == o32["filter_info"]
    T = tuple(float(np.abs(o32[k].astype(np.float64) - o64[k].astype(np.float64)).max()) for k in sv.FILTERED)
    print(c["name"], "T measured", T, "recorded", fc.T_SVGF[c["name"]])
    for k, t, rec in zip(sv.FILTERED, T, fc.T_SVGF[c["name"]]):
        assert t <= rec, (k, t, rec)
        assert np.isfinite(o64[k]).all() and np.isfinite(o32[k]).all()
    # what the GPU test asserts of pixels without a hit holds in the restatement
    inv = ~A["valid"]
    assert np.array_equal(o64["rgb"][inv], b["rgb"][inv]) and (o64["variance"][inv] == 0).all()
    assert np.array_equal(o64["color"][inv], A["accum"][inv])


@pytest.mark.parametrize("c", fc.TEMPORAL_CASES, ids=ids(fc.TEMPORAL_CASES))
def test_temporal_case_reaches_its_edge(c):
    b = fc.build(c)
    out, length, info = tr.accumulate_ref(b["rgb"], b["cur"], b["temporal_hist"], scene=b["scene"], **b["temporal_kw"])
    assert failed(c, "temporal", info) == []
    assert np.isfinite(out).all() and (length >= 1).all()


@pytest.mark.parametrize("c", fc.DENOISE_CASES, ids=ids(fc.DENOISE_CASES))
def test_denoise_case_holds_its_T_below_the_file_tolerance(c):
    b = fc.build(c)
    o64, T = fc.measure_denoise(b)
    rec = fc.T_DENOISE[c["name"]]
    print(c["name"], "T measured", T, "recorded", rec)
    assert T <= rec and sv.TOLERANCE_FACTOR * rec < 1e-4
    hits = b["sums"]["hits"]
    assert np.array_equal(o64[hits == 0], b["rgb"][hits == 0]) and np.isfinite(o64).all()
    if any(o.startswith("holes") for o in c["overlays"]):
        assert (hits == 0).any()
    if c["size"] == (513, 3):  # every one of the five step-128 taps of x = 256 lies in the image (the guides decide which weigh)
        assert b["denoise_kw"]["iterations"] == 8 and all(0 <= 256 + k * 128 < 513 for k in (-2, -1, 1, 2))


def test_the_lists_together_take_every_branch_and_every_edge():
    seen, fseen, far = {}, {}, {}
    for c in fc.SVGF_CASES:
        A, o64, _ = fc.svgf_refs(fc.build(c))
        for k, v in A["info"].items():
            seen[k] = seen.get(k, 0) + v
        for k in ("isolated_valid", "zero_variance_centre"):
            fseen[k] = fseen.get(k, 0) + o64["filter_info"][k]
        for s, v in o64["filter_info"]["far_tap_in_range"].items():
            far[s] = far.get(s, 0) + v
    for name in sv.BRANCHES + sv.EDGES:
        assert seen[name] > 0, name
    assert fseen["isolated_valid"] > 0 and fseen["zero_variance_centre"] > 0
    assert all(far.get(1 << i, 0) > 0 for i in range(8)), far
    tseen = {}
    for c in fc.TEMPORAL_CASES:
        b = fc.build(c)
        for k, v in tr.accumulate_ref(b["rgb"], b["cur"], b["temporal_hist"], scene=b["scene"], **b["temporal_kw"])[2].items():
            tseen[k] = tseen.get(k, 0) + v
    for name in tr.EDGES + ("miss", "nonfinite", "outside", "no_weight", "tap_mesh", "tap_position", "tap_nolength", "history",
                            "saturated", "alpha_bound"):
        assert tseen[name] > 0, name


def test_atrous_f32_is_the_float64_filter_to_rounding_and_one_iteration_of_svgf():
    """The float32 evaluation against things that do not share its code: the float64 atrous (three exponentials), and
    filter_stages(f32=True) with the luminance weight switched off."""
    b = fc.build(fc.by_name(fc.DENOISE_CASES, "33x16_5"))
    o32 = aov_ref.atrous(b["rgb"], b["sums"], 1, 1e15, 0.5, fc.SIGMA_POSITION, f32=True)
    o64 = aov_ref.atrous(b["rgb"], b["sums"], 1, 1e15, 0.5, fc.SIGMA_POSITION)
    assert o32.dtype == np.float32 and np.abs(o32.astype(np.float64) - o64).max() < 1e-6
    A = sv.stage_a(b["rgb"], b["sums"], b["cur"], sv.empty_history(33, 16), sigma_reproject=0.5)
    f = sv.filter_stages(A, b["sums"], iterations=1, sigma_luminance=1e30, sigma_position=fc.SIGMA_POSITION, f32=True)
    assert np.abs(f["rgb"].astype(np.float64) - o32).max() < 1e-6
