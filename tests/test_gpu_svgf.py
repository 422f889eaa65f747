"""rt_svgf on the GPU against the CPU restatement (tests/svgf_ref.py): the seven-frame animated sequence at two sizes and
three settings, stage A bit for bit and the filtered outputs within the float32-against-float64 tolerance measured on the
CPU; the device forms, aliasing, rejected calls; and the quality of the 8-frame turntable."""
import numpy as np
import pytest

import aov_ref
import orc
import pyrt
import svgf_ref as sv
import temporal_ref as tr
from temporal_ref import scene_of, turned

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("w,h", sv.SEQ_SIZES, ids=["%dx%d" % s for s in sv.SEQ_SIZES])
def test_sequence_equals_the_restatement_and_takes_every_branch(w, h):
    """Seven frames through the GPU calls, the GPU's own outputs fed forward as the history; at every frame the
    restatement is given the same history: out.moments, out.length and out.accum equal bit for bit, out.color, out.rgb
    and out.variance at every pixel within TOLERANCE_FACTOR x T_CPU of the float64 evaluation.  T_CPU (svgf_ref.py): the
    largest |float32 - float64 evaluation| over these frames at this size with this setting, measured on the CPU — the
    largest of them: colour 1.55e-6, rgb 1.50e-6, variance 1.34e-5; the largest differences seen on the MI355X:
    1.67e-6, 1.55e-6, 1.34e-5 (at most 0.27 of what their size and setting allow)."""
    seq = sv.sequence_inputs(w, h)
    bg = pyrt.background(w, h)
    seen, worst = {}, dict.fromkeys(sv.FILTERED, 0.0)
    for si, kw in enumerate(sv.SEQ_SETTINGS):
        T = sv.tolerance((w, h), si)
        ctx = pyrt.Context(pyrt.Scene("lowres", w, h))
        hist = pyrt.empty_svgf_history(w, h)
        for k, q in enumerate(seq):
            f = q["frame"]
            ctx.update(pos=f["pos"], nrm=f["nrm"], camera=f["camera"])
            rgb, _, _ = ctx.render(q["params"], bg)
            assert np.array_equal(bits(rgb), bits(q["rgb"])), "frame %d differs from the oracle's" % k
            sums = ctx.render_aov(q["params"], raw=True)
            cur = ctx.render_motion(q["params"], prev_pos=q["prev"]["pos"], prev_camera=q["prev"]["camera"])
            for c in ("albedo", "normal", "position", "hits"):
                assert np.array_equal(bits(sums[c]), bits(q["sums"][c])), (k, c)
            for c in pyrt.MOTION_CHANNELS:
                assert np.array_equal(bits(cur[c]), bits(q["cur"][c])), (k, c)
            out = ctx.svgf(rgb, sums, cur, hist, **kw)
            ref = sv.svgf_ref(q["rgb"], q["sums"], q["cur"], hist, scene=q["scene"], **kw)
            for c in ("moments", "length", "accum"):
                ne = bits(out[c]) != bits(ref[c])
                assert not ne.any(), "frame %d %s: %s differs at %d values" % (k, kw, c, int(ne.sum()))
            for c in sv.FILTERED:
                assert np.isfinite(out[c]).all(), (k, kw, c)
                d = float(np.abs(out[c].astype(np.float64) - ref[c].astype(np.float64)).max())
                worst[c] = max(worst[c], d)
                print("frame %d %s: max |%s - restatement| = %.3e (allowed %.3e)" % (k, kw, c, d, sv.TOLERANCE_FACTOR * T[c]))
                assert d <= sv.TOLERANCE_FACTOR * T[c], (k, kw, c, d)
            hist = sv.next_history(out, cur)
            for name, v in ref["info"].items():
                seen[name] = seen.get(name, 0) + v
        ctx.close()
    print("largest differences on this device:", worst)
    for name in sv.BRANCHES:
        assert seen[name] > 0, "the sequence never takes the branch %r" % name


def test_device_forms_aliasing_rejected_calls_and_an_undisturbed_context():
    """The device form on torch tensors equals the host form bit for bit; out.rgb may be cur_rgb; the optional outputs
    may be left out; a rejected call writes nothing; afterwards rt_render still gives the oracle's frame."""
    import torch
    w, h = sv.SEQ_SIZES[0]
    a = pyrt.Scene("lowres", w, h).arrays()
    frames = tr.animated_sequence(a)[:2]
    P = lambda k: pyrt.make_params(w, h, 4, mode=pyrt.MODE_PATH, seed=frames[k]["seed"])
    bg = pyrt.background(w, h)
    ctx = pyrt.Context(pyrt.Scene("lowres", w, h))
    rgb0, _, _ = ctx.render(P(0), bg)
    cur0 = ctx.render_motion(P(0))
    out0 = ctx.svgf(rgb0, ctx.render_aov(P(0), raw=True), cur0, pyrt.empty_svgf_history(w, h))
    hist = sv.next_history(out0, cur0)
    f = frames[1]
    ctx.update(pos=f["pos"], nrm=f["nrm"], camera=f["camera"])
    rgb1, _, _ = ctx.render(P(1), bg)
    sums1 = ctx.render_aov(P(1), raw=True)
    cur1 = ctx.render_motion(P(1), prev_pos=a["pos"], prev_camera=a["camera"])
    out1 = ctx.svgf(rgb1, sums1, cur1, hist)
    assert (out1["length"] == 2).sum() > 1000
    # in place on the host, and without the optional outputs
    inplace = rgb1.copy()
    part = ctx.svgf(inplace, sums1, cur1, hist, want=(), out_rgb=inplace)
    assert sorted(part) == ["color", "length", "moments", "rgb"] and part["rgb"] is inplace
    for c in part:
        assert np.array_equal(bits(part[c]), bits(out1[c])), c

    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.int32 if x.dtype == np.uint32 else x.dtype)).cuda()
    stream = torch.cuda.current_stream()
    d_rgb = dev(rgb1)
    d_aov = {k: dev(sums1[k]) for k in ("albedo", "normal", "position", "hits")}
    d_cur = {k: dev(cur1[k]) for k in ("motion", "prev_position", "mesh")}
    d_hist = {k: dev(v) for k, v in hist.items()}
    d_out = {k: torch.full((h, w, n) if n > 1 else (h, w), -7.0, device="cuda") for k, n in pyrt.SVGF_OUT_CHANNELS}
    torch.cuda.synchronize()
    ptrs = lambda d: {k: v.data_ptr() for k, v in d.items()}
    ctx.svgf_device(w, h, d_rgb.data_ptr(), ptrs(d_aov), ptrs(d_cur), ptrs(d_hist), ptrs(d_out), stream=stream.cuda_stream)
    stream.synchronize()
    for c, _ in pyrt.SVGF_OUT_CHANNELS:
        assert np.array_equal(bits(d_out[c].cpu().numpy()), bits(out1[c])), c
    # in place on the device: out.rgb = cur_rgb
    o = ptrs(d_out)
    o["rgb"] = d_rgb.data_ptr()
    ctx.svgf_device(w, h, d_rgb.data_ptr(), ptrs(d_aov), ptrs(d_cur), ptrs(d_hist), o)
    torch.cuda.synchronize()
    assert np.array_equal(bits(d_rgb.cpu().numpy()), bits(out1["rgb"]))
    d_rgb.copy_(dev(rgb1))

    # rejected calls write nothing
    for v in d_out.values():
        v.fill_(5.0)
    torch.cuda.synchronize()
    o = ptrs(d_out)
    o["color"] = d_hist["color"].data_ptr()
    bad_calls = [dict(out=o), dict(kw=dict(alpha_min=2.0)), dict(kw=dict(iterations=9)), dict(kw=dict(sigma_luminance=-1.0))]
    o2 = ptrs(d_out)
    o2["variance"] = d_out["length"].data_ptr()
    bad_calls.append(dict(out=o2))
    for b in bad_calls:
        with pytest.raises(pyrt.RtError) as e:
            ctx.svgf_device(w, h, d_rgb.data_ptr(), ptrs(d_aov), ptrs(d_cur), ptrs(d_hist), b.get("out", ptrs(d_out)), **b.get("kw", {}))
        assert e.value.code == 1, b
    torch.cuda.synchronize()
    assert all(bool((v == 5).all()) for v in d_out.values())
    for k, v in hist.items():
        assert np.array_equal(bits(d_hist[k].cpu().numpy()), bits(v)), k
    # the context renders as before
    _, acc, _ = ctx.render(P(1))
    _, ref_acc, _ = orc.render(scene_of(a, pos=f["pos"], nrm=f["nrm"], camera=f["camera"]), P(1), math_mode=orc.MATH_DET)
    assert np.array_equal(bits(acc), bits(ref_acc))
    ctx.close()


# F measured on the CPU (tools/svgf_sweep.py: oracle frames through svgf_ref, the cubes turntable, the defaults): DESIGN.md
# "Variance-guided spatiotemporal filtering".  The test allows twice that: another seed moves it.
F_MEASURED = 0.0616


def test_turntable_quality():
    """cubes 128x128, 4 spp, path mode, the 8-frame turntable of the accumulation's quality test, defaults:
    F = MSE(frame 8, 1024-spp frame 8 of another seed) / MSE(raw frame 8, same reference); rt_svgf's is at most
    2 F_MEASURED and below that of rt_temporal_accumulate alone on the same frames."""
    n, spp = 128, 4
    a = pyrt.Scene("cubes", n, n).arrays()
    bg = pyrt.background(n, n)
    ctx = pyrt.Context(pyrt.Scene("cubes", n, n))
    hist, thist = pyrt.empty_svgf_history(n, n), pyrt.empty_history(n, n)
    prev = None
    for k in range(8):
        pos, nrm = turned(a, 5.0 * k) if k else (a["pos"], a["nrm"])
        if k:
            ctx.update(pos=pos, nrm=nrm)
        p = pyrt.make_params(n, n, spp, mode=pyrt.MODE_PATH, seed=1 + k)
        rgb, _, _ = ctx.render(p, bg)
        cur = ctx.render_motion(p, prev_pos=prev)
        out = ctx.svgf(rgb, ctx.render_aov(p, raw=True), cur, hist)
        tout, tlen = ctx.temporal_accumulate(rgb, cur, thist)
        hist, thist, prev = sv.next_history(out, cur), tr.next_history(tout, tlen, cur), pos
    ref, _, _ = ctx.render(pyrt.make_params(n, n, 1024, mode=pyrt.MODE_PATH, seed=1000), bg)
    raw = aov_ref.mse(rgb, ref)
    F, Ft = aov_ref.mse(out["rgb"], ref) / raw, aov_ref.mse(tout, ref) / raw
    print("turntable quality: F_svgf = %.4f (measured on the CPU: %.4f), temporal accumulation alone %.4f, mean history "
          "length %.2f" % (F, F_MEASURED, Ft, float(out["length"].mean())))
    assert F <= 2 * F_MEASURED and F < Ft
    ctx.close()
