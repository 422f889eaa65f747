"""rt_temporal_accumulate, rt_svgf and rt_denoise on the synthetic cases of tests/filter_cases.py against their numpy
restatements, at every pixel of every case: stage A and the accumulation bit for bit, the filtered outputs within
svgf_ref.TOLERANCE_FACTOR (4) times the case's T — the largest |float32 - float64 evaluation| of the restatement, measured on
the CPU and recorded in filter_cases.T_SVGF / T_DENOISE; tests/test_filter_cases_cpu.py holds the restatement to it and
shows that every case reaches the edge it is named for.  Then the device forms and the in-place forms against the host
form, and one context across sizes (the scratch grows at 513x3 and is reused at 1x1 and 130x21)."""
import functools

import numpy as np
import pytest

import aov_ref
import filter_cases as fc
import pyrt
import svgf_ref as sv
import temporal_ref as tr

pytestmark = pytest.mark.gpu

TOL = 1e-4  # the file-level tolerance of tests/test_gpu_denoise.py: rt_denoise is held to min(TOL, 4 T)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def context():
    """(the explicit sigmas make the scene irrelevant; the default_sigmas cases take the box of this one)"""
    return pyrt.Context(pyrt.Scene("cubes", 130, 21))


@functools.lru_cache(maxsize=None)
def svgf_case(name):
    """(case, arrays, stage A, float64 outputs): computed once, shared by the tests, never written to."""
    c = fc.by_name(fc.SVGF_CASES, name)
    b = fc.build(c)
    A, o64, _ = fc.svgf_refs(b)
    return c, b, A, o64


@functools.lru_cache(maxsize=None)
def denoise_case(name):
    c = fc.by_name(fc.DENOISE_CASES, name)
    b = fc.build(c)
    return c, b, aov_ref.atrous(b["rgb"], b["sums"], scene=b["scene"], **b["denoise_kw"])


def run_svgf(ctx, b):
    return ctx.svgf(b["rgb"], b["sums"], b["cur"], b["svgf_hist"], **b["svgf_kw"])


def svgf_failures(name, out, worst=None):
    """Every way `out` misses the restatement of case `name` (empty: none); prints the case's figures."""
    c, b, A, ref = svgf_case(name)
    bad = []
    for ch in ("moments", "length", "accum"):
        ne = bits(out[ch]) != bits(A[ch])
        if ne.any():
            bad.append("%s: %s differs from stage_a at %d values, first at %s" % (name, ch, int(ne.sum()), np.argwhere(ne)[0]))
    T = dict(zip(sv.FILTERED, fc.T_SVGF[name]))
    for ch in sv.FILTERED:
        if not np.isfinite(out[ch]).all():
            bad.append("%s: %s is not finite" % (name, ch))
            continue
        diff = np.abs(out[ch].astype(np.float64) - ref[ch].astype(np.float64))
        d = float(diff.max())
        print("%s: max |%s - float64 restatement| = %.3e (T %.3e, allowed %.3e)" % (name, ch, d, T[ch], sv.TOLERANCE_FACTOR * T[ch]))
        if worst is not None:
            worst[ch] = max(worst[ch], (d / T[ch] if T[ch] else (0.0 if d == 0 else np.inf), d, T[ch], name))
        if d > sv.TOLERANCE_FACTOR * T[ch]:
            bad.append("%s: %s off by %.3e at %s, allowed %.3e" % (name, ch, d, np.unravel_index(diff.argmax(), diff.shape),
                                                                  sv.TOLERANCE_FACTOR * T[ch]))
    inv = b["sums"]["hits"] == 0
    if not np.array_equal(bits(out["rgb"][inv]), bits(b["rgb"][inv])):
        bad.append("%s: rgb of the pixels without a hit is not cur_rgb" % name)
    if not (out["variance"][inv] == 0).all():
        bad.append("%s: variance of the pixels without a hit is not 0" % name)
    if not np.array_equal(bits(out["color"][inv]), bits(out["accum"][inv])):
        bad.append("%s: color of the pixels without a hit is not accum" % name)
    return bad


def denoise_failures(name, out, rgb, worst=None):
    c, b, ref = denoise_case(name)
    T = fc.T_DENOISE[name]
    allowed = min(TOL, sv.TOLERANCE_FACTOR * T)
    bad = []
    if not np.isfinite(out).all():
        return ["%s: the output is not finite" % name]
    diff = np.abs(out.astype(np.float64) - ref.astype(np.float64))
    d = float(diff.max())
    print("%s: max |rt_denoise - float64 restatement| = %.3e (T %.3e, allowed %.3e)" % (name, d, T, allowed))
    if worst is not None:
        worst["out"] = max(worst["out"], (d / T if T else (0.0 if d == 0 else np.inf), d, T, name))
    if d > allowed:
        bad.append("%s: off by %.3e at %s, allowed %.3e" % (name, d, np.unravel_index(diff.argmax(), diff.shape), allowed))
    miss = b["sums"]["hits"] == 0
    if not np.array_equal(bits(out[miss]), bits(rgb[miss])):
        bad.append("%s: pixels without a hit changed" % name)
    return bad


def test_temporal_accumulate_equals_the_restatement_bit_for_bit():
    ctx = context()
    bad = []
    for c in fc.TEMPORAL_CASES:
        b = fc.build(c)
        out, length = ctx.temporal_accumulate(b["rgb"], b["cur"], b["temporal_hist"], **b["temporal_kw"])
        ref, rlen, _ = tr.accumulate_ref(b["rgb"], b["cur"], b["temporal_hist"], scene=b["scene"], **b["temporal_kw"])
        for ch, got, exp in (("out_rgb", out, ref), ("out_length", length, rlen)):
            ne = bits(got) != bits(exp)
            if ne.any():
                bad.append("%s: %s differs at %d values, first at %s" % (c["name"], ch, int(ne.sum()), np.argwhere(ne)[0]))
    ctx.close()
    assert not bad, "\n".join(bad)


def test_svgf_equals_the_restatement_within_the_recorded_T():
    """moments, length and accum bit for bit; color, rgb and variance within 4 T of the float64 evaluation at every pixel;
    pixels without a hit: rgb is cur_rgb, variance 0, color accum; everything finite."""
    ctx = context()
    bad, worst = [], dict.fromkeys(sv.FILTERED, (0.0, 0.0, 0.0, ""))
    for c in fc.SVGF_CASES:
        bad += svgf_failures(c["name"], run_svgf(ctx, svgf_case(c["name"])[1]), worst)
    ctx.close()
    for ch, (ratio, d, T, name) in worst.items():
        print("largest difference / T of %s on this device: %.2f (%.3e against T %.3e, case %s)" % (ch, ratio, d, T, name))
    assert not bad, "\n".join(bad)


def test_denoise_equals_the_restatement_within_the_recorded_T():
    ctx = context()
    bad, worst = [], dict(out=(0.0, 0.0, 0.0, ""))
    for c in fc.DENOISE_CASES:
        b = denoise_case(c["name"])[1]
        bad += denoise_failures(c["name"], ctx.denoise(b["rgb"], b["sums"], **b["denoise_kw"]), b["rgb"], worst)
    ctx.close()
    print("largest difference / T on this device: %.2f (%.3e against T %.3e, case %s)" % worst["out"])
    assert not bad, "\n".join(bad)


def test_device_forms_and_in_place_equal_the_host_form():
    import torch
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.int32 if x.dtype == np.uint32 else x.dtype).copy()).cuda()
    ptrs = lambda d: {k: v.data_ptr() for k, v in d.items()}
    ctx = context()
    stream = torch.cuda.current_stream()
    for name in fc.DEVICE_FORM_CASES:
        b = svgf_case(name)[1]
        w, h = svgf_case(name)[0]["size"]
        host = run_svgf(ctx, b)
        inplace = b["rgb"].copy()
        got = ctx.svgf(inplace, b["sums"], b["cur"], b["svgf_hist"], out_rgb=inplace, **b["svgf_kw"])
        assert got["rgb"] is inplace
        for ch in host:
            assert np.array_equal(bits(got[ch]), bits(host[ch])), (name, "host, in place", ch)
        d_rgb = dev(b["rgb"])
        d_aov = {k: dev(b["sums"][k]) for k in ("albedo", "normal", "position", "hits")}
        d_cur = {k: dev(b["cur"][k]) for k in ("motion", "prev_position", "mesh")}
        d_hist = {k: dev(v) for k, v in b["svgf_hist"].items()}
        d_out = {k: torch.full((h, w, n) if n > 1 else (h, w), -7.0, device="cuda") for k, n in pyrt.SVGF_OUT_CHANNELS}
        torch.cuda.synchronize()
        ctx.svgf_device(w, h, d_rgb.data_ptr(), ptrs(d_aov), ptrs(d_cur), ptrs(d_hist), ptrs(d_out), stream=stream.cuda_stream,
                        **b["svgf_kw"])
        stream.synchronize()
        for ch, _ in pyrt.SVGF_OUT_CHANNELS:
            assert np.array_equal(bits(d_out[ch].cpu().numpy()), bits(host[ch])), (name, "device", ch)
        o = ptrs(d_out)
        o["rgb"] = d_rgb.data_ptr()
        for v in d_out.values():
            v.fill_(-7.0)
        torch.cuda.synchronize()
        ctx.svgf_device(w, h, d_rgb.data_ptr(), ptrs(d_aov), ptrs(d_cur), ptrs(d_hist), o, stream=stream.cuda_stream, **b["svgf_kw"])
        stream.synchronize()
        assert np.array_equal(bits(d_rgb.cpu().numpy()), bits(host["rgb"])), (name, "device, in place")
        for ch, _ in pyrt.SVGF_OUT_CHANNELS[1:]:
            assert np.array_equal(bits(d_out[ch].cpu().numpy()), bits(host[ch])), (name, "device, in place", ch)
    for name in fc.DENOISE_DEVICE_FORM_CASES:
        c, b, _ = denoise_case(name)
        w, h = c["size"]
        host = ctx.denoise(b["rgb"], b["sums"], **b["denoise_kw"])
        buf = b["rgb"].copy()
        ctx.denoise(buf, b["sums"], out=buf, **b["denoise_kw"])
        assert np.array_equal(bits(buf), bits(host)), (name, "host, in place")
        d_aov = {k: dev(b["sums"][k]) for k in ("albedo", "normal", "position", "hits")}
        d_rgb = dev(b["rgb"])
        d_out = torch.full((h, w, 3), -7.0, device="cuda")
        torch.cuda.synchronize()
        ctx.denoise_device(w, h, d_rgb.data_ptr(), ptrs(d_aov), d_out.data_ptr(), stream.cuda_stream, **b["denoise_kw"])
        stream.synchronize()
        assert np.array_equal(bits(d_out.cpu().numpy()), bits(host)), (name, "device")
        ctx.denoise_device(w, h, d_rgb.data_ptr(), ptrs(d_aov), d_rgb.data_ptr(), stream.cuda_stream, **b["denoise_kw"])
        stream.synchronize()
        assert np.array_equal(bits(d_rgb.cpu().numpy()), bits(host)), (name, "device, in place")
    ctx.close()


def test_one_context_across_sizes():
    """513x3, then 1x1, then 130x21 on one context — the scratch both filters share grows, then serves smaller images — each
    held to its restatement; the 130x21 case run again last equals its first result bit for bit."""
    ctx = context()
    bad, results = [], {}
    for name, dname in zip(fc.ONE_CONTEXT_ORDER, fc.DENOISE_ONE_CONTEXT_ORDER):
        out = run_svgf(ctx, svgf_case(name)[1])
        bad += svgf_failures(name, out)
        b = denoise_case(dname)[1]
        dout = ctx.denoise(b["rgb"], b["sums"], **b["denoise_kw"])
        bad += denoise_failures(dname, dout, b["rgb"])
        for key, o in ((("svgf", name), out), (("denoise", dname), dict(out=dout))):
            first = results.setdefault(key, o)
            bad += ["%s: %s of the second run differs from the first" % (key[1], ch) for ch in o
                    if not np.array_equal(bits(o[ch]), bits(first[ch]))]
    ctx.close()
    assert fc.ONE_CONTEXT_ORDER[-1] == fc.ONE_CONTEXT_ORDER[-2] and fc.DENOISE_ONE_CONTEXT_ORDER[-1] == fc.DENOISE_ONE_CONTEXT_ORDER[-2]
    assert not bad, "\n".join(bad)
