"""rt_render_adaptive_shutter against its definition (include/rt_amd.h, guarantee A1): the passes of an adaptive frame are
rt_render_shutter frames.  The chain is K rt_render_shutter_device calls with seeds seed + k on a zero accumulator; the
retirement rule restated in numpy (tests/adaptive_ref.py run_rule, assemble) over it gives the accumulator, the spp map,
the image and the report, bit for bit.  One case takes its chain from the CPU oracle (tests/shutter_ref.py) instead of the
GPU.  Then: a shutter that changes nothing is rt_render_adaptive, the host form is the device form, and the rejections
write nothing."""
import ctypes as C

import numpy as np
import pytest
import torch

import adaptive_ref
import lens_ref
import pyrt
import shutter_ref
from adaptive_cases import bits, check_result

pytestmark = pytest.mark.gpu

P, PASSES, SEED = 2, 5, 17
INVALID, UNSUPPORTED = 1, 4
F32 = np.float32
# thresholds tried, coarse to fine: 2 down to 0.004 in steps of 10 %
LADDER = tuple(float(F32(2.0 * 0.9 ** i)) for i in range(60))
# (preset, open = without mesh 0, w, h, what the shutter does).  13x9: two by two granules, partial at both edges; 24x16:
# three by two whole ones.
CASES = [("cubes", False, 13, 9, "move_lens"), ("cubes", False, 24, 16, "turn"), ("lowres", True, 13, 9, "turn"),
         ("lowres", True, 24, 16, "move_lens")]


def case_id(c):
    return "%s%s-%dx%d-%s" % (c[0], "_open" if c[1] else "", c[2], c[3], c[4])


def case_scene(c):
    return lens_ref.scene(c[0], c[1], c[2], c[3])


def case_shutter_args(c):
    """(camera_close, open, close, aperture, focus_distance)"""
    A = shutter_ref.no_negative_zero(np.asarray(case_scene(c).arrays()["camera"], F32).reshape(4, 3))
    if c[4] == "move_lens":
        return shutter_ref.translated(A, shutter_ref.SMALL), 0.0, 1.0, lens_ref.APERTURES[0], lens_ref.FOCUS[1]
    return shutter_ref.turned(shutter_ref.translated(A, shutter_ref.SMALL), shutter_ref.TURN_DEGREES), 0.25, 0.5, 0.0, 0.0


def case_params(c, **kw):
    return pyrt.make_params(c[2], c[3], P, mode=pyrt.MODE_PATH, seed=SEED, **kw)


def with_seed(p, k):
    q = pyrt.Params.from_buffer_copy(p)
    q.seed = (p.seed + k) & 0xffffffff
    return q


def gpu_chain(ctx, p, sh, passes):
    """Accumulators after passes 0 .. passes - 1 of rt_render_shutter_device, seed + k, the whole range, into one
    accumulator that started at zero."""
    acc = torch.zeros((p.height, p.width, 4), dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream()
    out = []
    for k in range(passes):
        ctx.render_shutter_device(with_seed(p, k), sh, acc.data_ptr(), stream=stream.cuda_stream)
        stream.synchronize()
        out.append(acc.cpu().numpy().copy())
    return out


def oracle_chain(c, p, passes):
    """The same chain on the CPU: every sample of every pass is shutter_ref.expected over the one-sample range of that
    sample (a row per pixel), added to the accumulator in float32 in sample order, as the kernel adds it."""
    B, op, cl, ap, fo = case_shutter_args(c)
    acc = np.zeros((p.height, p.width, 4), F32)
    out = []
    for k in range(passes):
        for i in range(p.spp):
            q = with_seed(p, k)
            q.spp_begin, q.spp_count = i, 1
            acc = (acc + shutter_ref.expected(case_scene(c), B, q, op, cl, ap, fo)["accum"]).astype(F32)
        out.append(acc.copy())
    return out


def splitting_threshold(chain, bg):
    """A threshold of the ladder at which the reference rule retires some granules after min_passes and keeps others to
    the last pass; asserted on the reference itself."""
    for t in LADDER:
        K, active = adaptive_ref.run_rule(chain, bg, P, t, PASSES)
        if (K < PASSES).any() and (K == PASSES).any():
            assert K.min() >= min(adaptive_ref.DEFAULT_MIN_PASSES, PASSES) and active[-1] >= 1 and active[-1] < K.size
            return t, K, active
    raise AssertionError("no threshold of the ladder retires a part of the frame")


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_a1_passes_are_rt_render_shutter_frames(case):
    ctx = pyrt.Context(case_scene(case))
    try:
        bg = pyrt.background(case[2], case[3])
        sh = pyrt.make_shutter(*case_shutter_args(case))
        for kw in (dict(), dict(no_pool=True, lanes_per_pixel=1)):
            p = case_params(case, **kw)
            chain = gpu_chain(ctx, p, sh, PASSES)
            # threshold 0: nothing retires, the frame is the whole chain
            K, active = adaptive_ref.run_rule(chain, bg, P, 0.0, PASSES)
            assert (K == PASSES).all()
            check_result(p, bg, chain, K, active, ctx.render_adaptive_shutter(p, sh, bg, 0.0, PASSES))
            # a threshold that retires a part of the frame
            t, K, active = splitting_threshold(chain, bg)
            check_result(p, bg, chain, K, active, ctx.render_adaptive_shutter(p, sh, bg, t, PASSES))
        # the moving camera matters: the chain is not the still frame's
        still = pyrt.make_shutter(np.asarray(case_scene(case).arrays()["camera"], F32).reshape(4, 3), 0.0, 0.0)
        assert (bits(gpu_chain(ctx, p, still, 1)[0]) != bits(gpu_chain(ctx, p, sh, 1)[0])).mean() > 0.25
    finally:
        ctx.close()


def test_a1_against_the_cpu_oracle():
    case = CASES[0]
    ctx = pyrt.Context(case_scene(case))
    try:
        bg = pyrt.background(case[2], case[3])
        p = case_params(case)
        sh = pyrt.make_shutter(*case_shutter_args(case))
        chain = oracle_chain(case, p, PASSES)
        t, K, active = splitting_threshold(chain, bg)
        check_result(p, bg, chain, K, active, ctx.render_adaptive_shutter(p, sh, bg, t, PASSES))
        K0, active0 = adaptive_ref.run_rule(chain, bg, P, 0.0, PASSES)
        check_result(p, bg, chain, K0, active0, ctx.render_adaptive_shutter(p, sh, bg, 0.0, PASSES))
    finally:
        ctx.close()


@pytest.mark.parametrize("case", CASES[:2], ids=case_id)
def test_a_shutter_that_changes_nothing_is_rt_render_adaptive(case):
    ctx = pyrt.Context(case_scene(case))
    try:
        bg = pyrt.background(case[2], case[3])
        p = case_params(case)
        A = shutter_ref.no_negative_zero(np.asarray(case_scene(case).arrays()["camera"], F32).reshape(4, 3))
        chain = gpu_chain(ctx, p, pyrt.make_shutter(A, 0.0, 0.0), PASSES)
        t, _, _ = splitting_threshold(chain, bg)
        for thr in (0.0, t):
            eout, eacc, espp, erep, est = ctx.render_adaptive(p, bg, thr, PASSES)
            for sh in (pyrt.make_shutter(A, 0.0, 0.0), pyrt.make_shutter(A, 0.0, 1.0), pyrt.make_shutter(A, 0.25, 0.5, 0.0, 3.0)):
                out, acc, spp, rep, st = ctx.render_adaptive_shutter(p, sh, bg, thr, PASSES)
                assert np.array_equal(bits(acc), bits(eacc)) and np.array_equal(bits(out), bits(eout)) and np.array_equal(spp, espp)
                assert rep.passes == erep.passes and list(rep.active) == list(erep.active) and rep.pixel_samples == erep.pixel_samples
                assert (st.rays_closest, st.rays_shadow, st.samples) == (est.rays_closest, est.rays_shadow, est.samples)
    finally:
        ctx.close()


def test_device_form_equals_host_form():
    case = CASES[1]
    w, h = case[2], case[3]
    ctx = pyrt.Context(case_scene(case))
    try:
        bg = pyrt.background(w, h)
        p = case_params(case)
        sh = pyrt.make_shutter(*case_shutter_args(case))
        t, _, _ = splitting_threshold(gpu_chain(ctx, p, sh, PASSES), bg)
        out, acc, spp, rep, st = ctx.render_adaptive_shutter(p, sh, bg, t, PASSES)
        d_bg = torch.from_numpy(bg).cuda()
        d_acc = torch.full((h, w, 4), 7.0, dtype=torch.float32, device="cuda")  # overwritten
        d_out = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
        d_spp = torch.empty((h, w), dtype=torch.int32, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        rep2, st2 = ctx.render_adaptive_shutter_device(p, sh, d_bg.data_ptr(), d_acc.data_ptr(), d_out.data_ptr(), t, PASSES,
                                                       d_spp=d_spp.data_ptr(), stream=stream, stats=True)
        torch.cuda.synchronize()
        assert np.array_equal(bits(d_out.cpu().numpy()), bits(out)) and np.array_equal(bits(d_acc.cpu().numpy()), bits(acc))
        assert np.array_equal(d_spp.cpu().numpy().view(np.uint32), spp)
        assert rep2.passes == rep.passes and list(rep2.active) == list(rep.active)
        assert rep2.pixel_samples == rep.pixel_samples == st2.samples
        assert (st2.rays_closest, st2.rays_shadow) == (st.rays_closest, st.rays_shadow)
        # without report, stats or spp: the same image once the stream has run
        d_out2 = torch.empty_like(d_out)
        rep3, _ = ctx.render_adaptive_shutter_device(p, sh, d_bg.data_ptr(), d_acc.data_ptr(), d_out2.data_ptr(), t, PASSES, stream=stream)
        torch.cuda.synchronize()
        assert np.array_equal(bits(d_out2.cpu().numpy()), bits(out)) and rep3.passes == rep.passes
    finally:
        ctx.close()


def test_rejections_write_nothing_and_leave_the_context_working():
    case = CASES[0]
    w, h = case[2], case[3]
    L = pyrt.amd()
    ctx = pyrt.Context(case_scene(case))
    try:
        bg = pyrt.background(w, h)
        p = case_params(case)
        B, op, cl, ap, fo = case_shutter_args(case)
        good = pyrt.make_shutter(B, op, cl, ap, fo)
        before = ctx.render_adaptive_shutter(p, good, bg, 0.5, PASSES)
        out, acc, spp = np.full((h, w, 3), 3.0, F32), np.full((h, w, 4), 3.0, F32), np.full((h, w), 3, np.uint32)
        rep = pyrt.AdaptiveReport()
        rep.passes = 7
        a = pyrt.make_adaptive(0.5, PASSES)
        ptr = lambda x: x.ctypes.data_as(C.c_void_p)

        def call(q=p, sh=good):
            return L.rt_render_adaptive_shutter(ctx._h, C.byref(q), C.byref(a), None if sh is None else C.byref(sh), ptr(bg), ptr(out),
                                                ptr(acc), ptr(spp), C.byref(rep), None)

        assert call(sh=None) == INVALID and b"null" in L.rt_last_error()
        reserved = pyrt.make_shutter(B, op, cl, ap, fo)
        reserved.reserved[2] = 1
        A = np.asarray(case_scene(case).arrays()["camera"], F32).reshape(4, 3)
        for bad, word in ((reserved, b"reserved"), (pyrt.make_shutter(B, 0.6, 0.5), b"exposure"), (pyrt.make_shutter(B, 0.0, 1.0, 0.1, 0.0), b"focus_distance"),
                          (pyrt.make_shutter(B, 0.0, 1.0, 1e9, 1.0), b"origin bound"), (pyrt.make_shutter(shutter_ref.turned(A, 120.0)), b"90 degrees")):
            assert call(sh=bad) == INVALID and word in L.rt_last_error(), L.rt_last_error()
        assert call(q=case_params(case, use_photons=1, k=4, photons_requested=100)) == UNSUPPORTED
        assert call(q=case_params(case, wavefront=True)) == UNSUPPORTED
        assert call(q=case_params(case, world=2)) == UNSUPPORTED
        assert call(q=pyrt.make_params(w, h, 4, seed=SEED, spp_begin=1, spp_count=2)) == INVALID
        assert (out == 3).all() and (acc == 3).all() and (spp == 3).all() and rep.passes == 7
        after = ctx.render_adaptive_shutter(p, good, bg, 0.5, PASSES)
        assert np.array_equal(bits(after[1]), bits(before[1])) and np.array_equal(after[2], before[2])
    finally:
        ctx.close()
