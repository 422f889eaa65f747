"""rt_render_adaptive against its definition (include/rt_amd.h, DESIGN.md "Adaptive sampling"): a chain of
rt_render_passes calls with seeds seed + j, the retirement rule restated in numpy (tests/adaptive_ref.py) over it, and
then bit for bit: spp == K * P, the accumulator equal to the chain's after K passes, the image equal to the resolve with
N = K * P; the per-pass active counts, the device form, and the error codes."""
import ctypes as C

import numpy as np
import pytest

import adaptive_ref
import pyrt
from adaptive_cases import bits, chain_of, check_frame, pick_threshold

pytestmark = pytest.mark.gpu

P = 4
PASSES = 8
SEED = 17
INVALID, UNSUPPORTED, STATE = 1, 4, 5  # rt_amd.h RT_ERR_*


@pytest.mark.parametrize("kind,w,h", [("cubes", 64, 64), ("lowres", 96, 64), ("cubes", 70, 45)],
                         ids=["cubes64", "lowres96x64", "cubes70x45"])
def test_adaptive_matches_chain(kind, w, h):
    s = pyrt.Scene(kind, w, h)
    ctx = pyrt.Context(s)
    bg = pyrt.background(w, h)
    p = pyrt.make_params(w, h, P, mode=pyrt.MODE_PATH, seed=SEED)
    chain = chain_of(ctx, p, bg, PASSES)
    t, K = pick_threshold(chain, bg, PASSES, P)
    Kg, *_ = check_frame(ctx, p, bg, chain, t, PASSES)
    assert len(np.unique(Kg)) >= 3 and Kg.min() >= 4  # granules retired at several passes, none before min_passes
    # explicit min_passes and floor
    check_frame(ctx, p, bg, chain, t, PASSES, min_passes=2, floor=0.05)
    ctx.close()


def test_threshold_zero_and_huge():
    w, h = 72, 40
    s = pyrt.Scene("cubes", w, h)
    ctx = pyrt.Context(s)
    bg = pyrt.background(w, h)
    p = pyrt.make_params(w, h, P, mode=pyrt.MODE_PATH, seed=SEED)
    chain = chain_of(ctx, p, bg, 6)
    # threshold 0: every granule runs max_passes — the full chain and its plain resolve
    K, out, acc, spp, rep = check_frame(ctx, p, bg, chain, 0., 6)
    assert (K == 6).all() and np.array_equal(bits(acc), bits(chain[5]))
    assert np.array_equal(bits(out), bits(adaptive_ref.resolve(chain[5], bg, np.full((h, w), 6 * P))))
    assert rep.active[:6] == [K.size] * 6
    # a huge threshold: everything retires at min_passes (default 4, and an explicit 3)
    K, *_ = check_frame(ctx, p, bg, chain, 1e30, 6)
    assert (K == 4).all()
    K, *_ = check_frame(ctx, p, bg, chain, 1e30, 6, min_passes=3)
    assert (K == 3).all()
    # max_passes 1: one pass of seed
    K, out, acc, spp, rep = check_frame(ctx, p, bg, chain, 0.1, 1)
    assert (K == 1).all() and rep.passes == 1
    ctx.close()


def _photons(ctx, nph=3000):
    pos, dir_, wt = ctx.emit_photons(nph, seed=2)
    kp, kd_, _ = pyrt.kd_order(pos, dir_, wt)
    ctx.set_photons(kp, kd_)


@pytest.mark.parametrize("case", ["photon", "brute", "q8", "lanes2", "ray"])
def test_adaptive_variants(case):
    w, h = 64, 48
    kind = "lowres" if case == "q8" else "cubes"
    s = pyrt.Scene(kind, w, h)
    ctx = pyrt.Context(s, node_format=pyrt.NODES_Q8) if case == "q8" else pyrt.Context(s)
    if case == "q8":
        assert ctx.bvh_info().node_format == pyrt.NODES_Q8
    kw = {}
    if case == "photon":
        _photons(ctx)
        kw = dict(use_photons=1, k=10, photons_requested=3000, mode=pyrt.MODE_RAY)
    elif case == "brute":
        kw = dict(accel=pyrt.ACCEL_BRUTE)
    elif case == "lanes2":
        kw = dict(lanes_per_pixel=2)
    elif case == "ray":
        kw = dict(mode=pyrt.MODE_RAY)
    kw.setdefault("mode", pyrt.MODE_PATH)
    bg = pyrt.background(w, h)
    p = pyrt.make_params(w, h, P, seed=SEED, **kw)
    chain = chain_of(ctx, p, bg, 6)
    t, _ = pick_threshold(chain, bg, 6, P)
    check_frame(ctx, p, bg, chain, t, 6)
    ctx.close()


def test_device_form_equals_host_form():
    torch = pytest.importorskip("torch")
    w, h = 64, 40
    s = pyrt.Scene("cubes", w, h)
    ctx = pyrt.Context(s)
    bg = pyrt.background(w, h)
    p = pyrt.make_params(w, h, P, mode=pyrt.MODE_PATH, seed=SEED)
    chain = chain_of(ctx, p, bg, 6)
    t, _ = pick_threshold(chain, bg, 6, P)
    out, acc, spp, rep, _ = ctx.render_adaptive(p, bg, t, 6)
    dev = torch.device("cuda:0")
    d_bg = torch.from_numpy(bg).to(dev)
    d_acc = torch.full((h, w, 4), 7.0, dtype=torch.float32, device=dev)  # overwritten
    d_out = torch.empty((h, w, 3), dtype=torch.float32, device=dev)
    d_spp = torch.empty((h, w), dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    rep2, st2 = ctx.render_adaptive_device(p, d_bg.data_ptr(), d_acc.data_ptr(), d_out.data_ptr(), t, 6,
                                           d_spp=d_spp.data_ptr(), stream=stream, stats=True)
    torch.cuda.synchronize()
    assert np.array_equal(bits(d_out.cpu().numpy()), bits(out))
    assert np.array_equal(bits(d_acc.cpu().numpy()), bits(acc))
    assert np.array_equal(d_spp.cpu().numpy().view(np.uint32), spp)
    assert rep2.passes == rep.passes and list(rep2.active) == list(rep.active)
    assert rep2.pixel_samples == rep.pixel_samples == st2.samples
    # without report, stats or spp: the same image once the stream has run
    d_out2 = torch.empty_like(d_out)
    a = pyrt.make_adaptive(t, 6)
    rc = pyrt.amd().rt_render_adaptive_device(ctx._h, C.byref(p), C.byref(a), C.c_void_p(d_bg.data_ptr()),
                                              C.c_void_p(d_acc.data_ptr()), C.c_void_p(d_out2.data_ptr()), None,
                                              C.c_void_p(stream), None, None)
    assert rc == 0
    torch.cuda.synchronize()
    assert np.array_equal(bits(d_out2.cpu().numpy()), bits(out))
    ctx.close()


def test_rejections_leave_the_context_working():
    w, h = 40, 32
    s = pyrt.Scene("cubes", w, h)
    ctx = pyrt.Context(s)
    bg = pyrt.background(w, h)
    p = pyrt.make_params(w, h, P, mode=pyrt.MODE_PATH, seed=SEED)
    before, _, _ = ctx.render(p, bg)
    L = pyrt.amd()
    out = np.empty((h, w, 3), np.float32)

    def rc(a=None, bgp=bg, outp=out, **kw):
        q = pyrt.make_params(w, h, P, mode=pyrt.MODE_PATH, seed=SEED, **kw)
        a = a if a is not None else pyrt.make_adaptive(0.1, 4)
        return L.rt_render_adaptive(ctx._h, C.byref(q), C.byref(a), pyrt._ptr(bgp), pyrt._ptr(outp), None, None, None, None)

    assert rc() == 0
    assert L.rt_render_adaptive(ctx._h, None, C.byref(pyrt.make_adaptive(0.1, 4)), pyrt._ptr(bg), pyrt._ptr(out),
                                None, None, None, None) == INVALID
    assert L.rt_render_adaptive(ctx._h, C.byref(p), None, pyrt._ptr(bg), pyrt._ptr(out), None, None, None, None) == INVALID
    assert rc(bgp=None) == INVALID and rc(outp=None) == INVALID
    assert rc(spp_begin=1, spp_count=2) == INVALID
    assert rc(spp_count=4) == INVALID
    for a in (pyrt.make_adaptive(0.1, 0), pyrt.make_adaptive(0.1, 4, min_passes=1), pyrt.make_adaptive(0.1, 4, min_passes=5),
              pyrt.make_adaptive(-0.1, 4), pyrt.make_adaptive(float("nan"), 4), pyrt.make_adaptive(float("inf"), 4),
              pyrt.make_adaptive(0.1, 4, floor=-1.), pyrt.make_adaptive(0.1, 4, floor=float("inf")),
              pyrt.make_adaptive(0.1, 0x7fffffff)):
        assert rc(a) == INVALID, (a.max_passes, a.min_passes, a.threshold, a.floor)
    a = pyrt.make_adaptive(0.1, 4)
    a.reserved[3] = 1
    assert rc(a) == INVALID
    assert L.rt_render_adaptive(ctx._h, C.byref(pyrt.make_params(0, h, P)), C.byref(pyrt.make_adaptive(0.1, 4)),
                                pyrt._ptr(bg), pyrt._ptr(out), None, None, None, None) == INVALID
    assert rc(rank=0, world=2) == UNSUPPORTED
    assert rc(wavefront=True) == UNSUPPORTED
    assert rc(use_photons=1, k=5, photons_requested=100) == STATE  # no photon map
    after, _, _ = ctx.render(p, bg)
    assert np.array_equal(bits(before), bits(after))
    ctx.close()
