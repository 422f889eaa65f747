"""rt_render_motion and rt_temporal_accumulate on the GPU, bit for bit against the CPU restatements (tests/temporal_ref.py):
the motion pass over turned geometry, moved cameras, sizes, sample ranges, accelerators and tree builders; an animated
sequence carried through the accumulation on both sides with every branch of the rule exercised; the device forms, the
rejected calls, and the quality of an 8-frame turntable."""
import numpy as np
import pytest

import aov_ref
import orc
import pyrt
import temporal_ref as tr
from temporal_ref import moved_camera, scene_of, turned

pytestmark = pytest.mark.gpu

CHANNELS = pyrt.MOTION_CHANNELS
CAM_DELTA = (0.11, -0.07, 0.05)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_motion_equal(got, exp, what=""):
    for k in CHANNELS:
        assert got[k].shape == exp[k].shape, (what, k)
        ne = (bits(got[k]) != bits(exp[k])).reshape(got[k].shape[0], got[k].shape[1], -1).any(axis=2)
        assert not ne.any(), "%s: channel %s differs at %d pixels" % (what, k, int(ne.sum()))


def oracle_accel(kind):
    return orc.ACCEL_OBVH if kind == "hires" else orc.ACCEL_LOOP


def animated(kind, w, h, deg, delta):
    """(arrays of the preset, current scene): slot 3 turned by deg, the camera moved by delta."""
    a = pyrt.Scene(kind, w, h).arrays()
    pos, nrm = turned(a, deg) if deg else (a["pos"], a["nrm"])
    cam = moved_camera(a["camera"], delta) if delta is not None else a["camera"]
    return a, scene_of(a, pos=pos, nrm=nrm, camera=cam)


MOTION_CASES = [
    # id, kind, builder, expected builder, w, h, degrees, camera move, sample range, accelerator
    ("lowres_turn5", "lowres", pyrt.BVH_AUTO, pyrt.BVH_HOST, 24, 24, 5.0, None, dict(spp=4), pyrt.ACCEL_BVH),
    ("lowres_turn20_range", "lowres", pyrt.BVH_AUTO, pyrt.BVH_HOST, 40, 56, 20.0, None, dict(spp=7, spp_begin=3, spp_count=4), pyrt.ACCEL_BVH),
    ("lowres_camera_odd", "lowres", pyrt.BVH_AUTO, pyrt.BVH_HOST, 37, 23, 0.0, CAM_DELTA, dict(spp=4), pyrt.ACCEL_BVH),
    ("lowres_both_brute", "lowres", pyrt.BVH_AUTO, pyrt.BVH_HOST, 24, 24, 20.0, CAM_DELTA, dict(spp=4, spp_begin=1, spp_count=2), pyrt.ACCEL_BRUTE),
    ("hires_turn5_device", "hires", pyrt.BVH_AUTO, pyrt.BVH_DEVICE, 24, 24, 5.0, None, dict(spp=4), pyrt.ACCEL_BVH),
    ("hires_both_device_range", "hires", pyrt.BVH_AUTO, pyrt.BVH_DEVICE, 40, 56, 20.0, CAM_DELTA, dict(spp=7, spp_begin=3, spp_count=4), pyrt.ACCEL_BVH),
    ("hires_both_hybrid_odd", "hires", pyrt.BVH_HYBRID, pyrt.BVH_HYBRID, 37, 23, 20.0, CAM_DELTA, dict(spp=4), pyrt.ACCEL_BVH),
    ("hires_turn20_brute", "hires", pyrt.BVH_AUTO, pyrt.BVH_DEVICE, 24, 24, 20.0, None, dict(spp=4), pyrt.ACCEL_BRUTE),
]


@pytest.mark.parametrize("name,kind,builder,expect,w,h,deg,delta,rng,accel", MOTION_CASES, ids=[c[0] for c in MOTION_CASES])
def test_motion_bit_exact(name, kind, builder, expect, w, h, deg, delta, rng, accel):
    """A resident scene follows the animation by rt_update; the motion pass against last frame's positions and camera
    equals the restatement bit for bit, its mesh is rt_render_aov's and its position rt_render_aov's one-sample sum."""
    a, cur = animated(kind, w, h, deg, delta)
    ctx = pyrt.Context(pyrt.Scene(kind, w, h), bvh_builder=builder)
    assert ctx.bvh_info().builder == expect
    ca = cur.arrays()
    ctx.update(pos=ca["pos"], nrm=ca["nrm"], camera=ca["camera"])
    p = pyrt.make_params(w, h, seed=11, mode=pyrt.MODE_PATH, accel=accel, **rng)
    got = ctx.render_motion(p, prev_pos=a["pos"], prev_camera=a["camera"])
    exp = tr.motion_ref(cur, p, prev_pos=a["pos"], prev_camera=a["camera"], accel=oracle_accel(kind))
    assert_motion_equal(got, exp, name)
    hit = got["mesh"] != tr.MISS
    assert (got["motion"][hit] != 0).any(), "the case moves nothing"
    s0 = p.spp_begin if p.spp_count else 0
    one = pyrt.make_params(w, h, seed=11, mode=pyrt.MODE_PATH, accel=accel, spp=p.spp, spp_begin=s0, spp_count=1)
    aov = ctx.render_aov(one, raw=True, channels=("position", "mesh"))
    assert np.array_equal(aov["mesh"], got["mesh"])
    assert np.array_equal(ctx.render_aov(p, raw=True, channels=("mesh",))["mesh"], got["mesh"])
    assert np.array_equal(aov["position"], got["position"])  # (in value: the sum starts from +0)
    ctx.close()


def test_motion_q8_context():
    """An RT_NODES_Q8 context (no rt_update: created on the current frame's scene) walks its resident 32-byte records."""
    w, h = 40, 56
    a, cur = animated("hires", w, h, 20.0, CAM_DELTA)
    ctx = pyrt.Context(cur, bvh_builder=pyrt.BVH_HOST, node_format=pyrt.NODES_Q8)
    assert ctx.bvh_info().node_format == pyrt.NODES_Q8
    p = pyrt.make_params(w, h, 4, seed=6, mode=pyrt.MODE_PATH)
    got = ctx.render_motion(p, prev_pos=a["pos"], prev_camera=a["camera"])
    assert_motion_equal(got, tr.motion_ref(cur, p, prev_pos=a["pos"], prev_camera=a["camera"], accel=orc.ACCEL_OBVH), "q8")
    ctx.close()


def test_points_behind_the_previous_camera_have_infinite_motion():
    w, h = 40, 56
    s = pyrt.Scene("lowres", w, h)
    a = s.arrays()
    inside = moved_camera(a["camera"], (0.0, 0.0, -3.0))  # (in the room: the near part of the floor lies behind it)
    ctx = pyrt.Context(s)
    p = pyrt.make_params(w, h, 4, seed=24, mode=pyrt.MODE_PATH)
    got = ctx.render_motion(p, prev_camera=inside)
    exp = tr.motion_ref(s, p, prev_camera=inside)
    assert_motion_equal(got, exp, "behind the camera")
    inf = np.isposinf(got["motion"])
    assert inf[..., 0].sum() > 100 and np.array_equal(inf[..., 0], inf[..., 1]) and np.isfinite(got["motion"][~inf]).all()
    assert np.array_equal(bits(got["prev_position"]), bits(got["position"]))  # (the geometry did not move)
    ctx.close()


@pytest.mark.parametrize("kind,pan", [("lowres", 2.5), ("hires", 0.0)])
def test_null_prev_is_the_contexts_own(kind, pan):
    """NULL prev members = the context's own arrays and camera: motion exactly 0, prev_position bit-equal to position;
    with the camera panned past the room's wall, misses are all zero with mesh 0xffffffff."""
    w, h = 40, 56
    a = pyrt.Scene(kind, w, h).arrays()
    s = scene_of(a, camera=tr.panned_camera(a["camera"], pan))
    ctx = pyrt.Context(s)
    p = pyrt.make_params(w, h, 4, seed=2, mode=pyrt.MODE_PATH)
    none = ctx.render_motion(p)
    own = ctx.render_motion(p, prev_pos=a["pos"], prev_camera=s.arrays()["camera"])
    assert_motion_equal(none, own, "NULL prev")
    assert_motion_equal(none, tr.motion_ref(s, p, accel=oracle_accel(kind)), "NULL prev vs restatement")
    hit = none["mesh"] != tr.MISS
    assert not none["motion"].any() and np.array_equal(bits(none["prev_position"]), bits(none["position"]))
    assert not none["position"][~hit].any()
    assert (~hit).sum() > 100 if pan else hit.all()
    # only some channels
    part = ctx.render_motion(p, channels=("motion", "mesh"))
    assert sorted(part) == ["mesh", "motion"] and np.array_equal(part["mesh"], none["mesh"])
    ctx.close()


# ---- the accumulation --------------------------------------------------------------------------------------------------
SEQ_W, SEQ_H = 40, 56


def seq_params(frames):
    return lambda k: pyrt.make_params(SEQ_W, SEQ_H, 4, mode=pyrt.MODE_PATH, seed=frames[k]["seed"])


def test_sequence_equals_the_restatement_and_takes_every_branch():
    """Seven frames (turntable, camera moves, a pan past the wall, a jump into the room; seeds differing per frame; 4 spp,
    path mode) through accumulate_ref and through the GPU calls, the history fed forward on each side independently:
    out_rgb and out_length equal at every frame, once with the defaults and once with max_history 3 and alpha_min 0.4.
    The restatement's own bookkeeping shows that the two runs take every branch of the rule."""
    a = pyrt.Scene("lowres", SEQ_W, SEQ_H).arrays()
    frames = tr.animated_sequence(a)
    assert len(frames) >= 6
    P = seq_params(frames)
    bg = pyrt.background(SEQ_W, SEQ_H)
    scenes = [scene_of(a, pos=f["pos"], nrm=f["nrm"], camera=f["camera"]) for f in frames]
    ref_rgb = [orc.render(s, P(k), math_mode=orc.MATH_DET, bg=bg)[0] for k, s in enumerate(scenes)]
    seen = {}
    for kw in (dict(), dict(max_history=3, alpha_min=0.4)):
        ref = tr.run_sequence_ref(a, frames, ref_rgb, P, **kw)
        ctx = pyrt.Context(pyrt.Scene("lowres", SEQ_W, SEQ_H))
        hist = pyrt.empty_history(SEQ_W, SEQ_H)
        for k, f in enumerate(frames):
            ctx.update(pos=f["pos"], nrm=f["nrm"], camera=f["camera"])
            rgb, _, _ = ctx.render(P(k), bg)
            assert np.array_equal(bits(rgb), bits(ref_rgb[k])), "frame %d differs from the oracle's" % k
            prev = frames[k - 1] if k else f
            cur = ctx.render_motion(P(k), prev_pos=prev["pos"], prev_camera=prev["camera"])
            assert_motion_equal(cur, ref[k][0], "frame %d" % k)
            out, length = ctx.temporal_accumulate(rgb, cur, hist, **kw)
            print("frame %d %s: %s" % (k, kw, ref[k][3]))
            assert np.array_equal(bits(out), bits(ref[k][1])), "frame %d %s: out_rgb differs at %d pixels" % (
                k, kw, int((bits(out) != bits(ref[k][1])).any(axis=2).sum()))
            assert np.array_equal(bits(length), bits(ref[k][2])), "frame %d %s: out_length differs" % (k, kw)
            hist = tr.next_history(out, length, cur)
            for name, v in ref[k][3].items():
                seen[name] = seen.get(name, 0) + v
        ctx.close()
    for name in ("miss", "nonfinite", "outside", "no_weight", "tap_mesh", "tap_position", "history", "saturated", "alpha_bound"):
        assert seen[name] > 0, "the sequence never takes the branch %r" % name


def test_device_forms_rejected_calls_and_an_undisturbed_context():
    """The device forms on torch tensors equal the host forms; a rejected call leaves its outputs untouched; afterwards
    rt_render of the same params still gives the oracle's frame."""
    import torch
    w, h = SEQ_W, SEQ_H
    a = pyrt.Scene("lowres", w, h).arrays()
    frames = tr.animated_sequence(a)[:2]
    P = seq_params(frames)
    bg = pyrt.background(w, h)
    ctx = pyrt.Context(pyrt.Scene("lowres", w, h))
    rgb0, _, _ = ctx.render(P(0), bg)
    cur0 = ctx.render_motion(P(0))
    out0, len0 = ctx.temporal_accumulate(rgb0, cur0, pyrt.empty_history(w, h))
    hist = tr.next_history(out0, len0, cur0)
    f = frames[1]
    ctx.update(pos=f["pos"], nrm=f["nrm"], camera=f["camera"])
    rgb1, _, _ = ctx.render(P(1), bg)
    cur1 = ctx.render_motion(P(1), prev_pos=a["pos"], prev_camera=a["camera"])
    out1, len1 = ctx.temporal_accumulate(rgb1, cur1, hist)
    assert (len1 == 2).sum() > 1000

    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.int32 if x.dtype == np.uint32 else x.dtype)).cuda()
    stream = torch.cuda.current_stream()
    d_prev = dev(a["pos"])
    d_cur = {k: torch.full(cur1[k].shape, -7, dtype=torch.int32 if k == "mesh" else torch.float32, device="cuda") for k in CHANNELS}
    torch.cuda.synchronize()
    ctx.render_motion_device(P(1), {k: v.data_ptr() for k, v in d_cur.items()}, d_prev_pos=d_prev.data_ptr(),
                             prev_camera=a["camera"], stream=stream.cuda_stream)
    stream.synchronize()
    assert_motion_equal({k: v.cpu().numpy().view(cur1[k].dtype) for k, v in d_cur.items()}, cur1, "device form")
    d_hist = {k: dev(v) for k, v in hist.items()}
    d_rgb, d_out, d_len = dev(rgb1), torch.full((h, w, 3), -7.0, device="cuda"), torch.full((h, w), -7.0, device="cuda")
    torch.cuda.synchronize()
    cur_ptrs = {k: d_cur[k].data_ptr() for k in ("motion", "prev_position", "mesh")}
    hist_ptrs = {k: v.data_ptr() for k, v in d_hist.items()}
    ctx.temporal_accumulate_device(w, h, d_rgb.data_ptr(), cur_ptrs, hist_ptrs, d_out.data_ptr(), d_len.data_ptr(),
                                   stream=stream.cuda_stream)
    stream.synchronize()
    assert np.array_equal(bits(d_out.cpu().numpy()), bits(out1)) and np.array_equal(bits(d_len.cpu().numpy()), bits(len1))
    # in place: out_rgb may be cur_rgb
    ctx.temporal_accumulate_device(w, h, d_rgb.data_ptr(), cur_ptrs, hist_ptrs, d_rgb.data_ptr(), d_len.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(bits(d_rgb.cpu().numpy()), bits(out1))

    # rejected calls write nothing
    d_out.fill_(5.0), d_len.fill_(5.0)
    torch.cuda.synchronize()
    with pytest.raises(pyrt.RtError) as e:  # the outputs alias the history
        ctx.temporal_accumulate_device(w, h, d_rgb.data_ptr(), cur_ptrs, hist_ptrs, d_hist["rgb"].data_ptr(), d_len.data_ptr())
    assert e.value.code == 1
    with pytest.raises(pyrt.RtError) as e:
        ctx.temporal_accumulate_device(w, h, d_rgb.data_ptr(), cur_ptrs, hist_ptrs, d_out.data_ptr(), d_len.data_ptr(), alpha_min=2.0)
    assert e.value.code == 1
    for k, v in d_cur.items():
        v.fill_(5)
    torch.cuda.synchronize()
    for kw, code in ((dict(world=2), 4), (dict(world=2, rank=3), 1), (dict(width=0), 1), (dict(spp_begin=2, spp_count=3), 1), (dict(spp=0), 1)):
        q = P(1)
        for k, v in kw.items():
            setattr(q, k, v)
        with pytest.raises(pyrt.RtError) as e:
            ctx.render_motion_device(q, {k: v.data_ptr() for k, v in d_cur.items()}, d_prev_pos=d_prev.data_ptr())
        assert e.value.code == code, kw
    nonfinite = a["camera"].copy()
    nonfinite[0, 0] = np.inf
    with pytest.raises(pyrt.RtError) as e:
        ctx.render_motion_device(P(1), {k: v.data_ptr() for k, v in d_cur.items()}, prev_camera=nonfinite)
    assert e.value.code == 1
    torch.cuda.synchronize()
    assert bool((d_out == 5).all()) and bool((d_len == 5).all()) and all(bool((v == 5).all()) for v in d_cur.values())
    assert np.array_equal(bits(d_hist["rgb"].cpu().numpy()), bits(hist["rgb"]))
    # the fields that do not affect the pass
    q = P(1)
    q.use_photons, q.k, q.photons_requested, q.mode, q.max_depth = 1, 5, 100, 7, 9
    again = ctx.render_motion(q, prev_pos=a["pos"], prev_camera=a["camera"])
    assert_motion_equal(again, cur1, "mode, max_depth and the photon fields")
    # the context renders as before
    _, acc, _ = ctx.render(P(1))
    _, ref_acc, _ = orc.render(scene_of(a, pos=f["pos"], nrm=f["nrm"], camera=f["camera"]), P(1), math_mode=orc.MATH_DET)
    assert np.array_equal(bits(acc), bits(ref_acc))
    ctx.close()


# F measured on the CPU (tools/temporal_sweep.py: oracle frames through accumulate_ref, the cubes turntable): DESIGN.md
# "Motion vectors and temporal accumulation".  The test allows twice that: another seed moves it.
F_MEASURED = 0.2604


def test_turntable_quality():
    """cubes 128x128, 4 spp, path mode, an 8-frame turntable (slot 3 turned 5 degrees per frame), defaults:
    F = MSE(temporal frame 8, 1024-spp frame 8 of another seed) / MSE(raw frame 8, same reference) <= 2 F_MEASURED, and
    F < 1 in any case."""
    n, spp = 128, 4
    a = pyrt.Scene("cubes", n, n).arrays()
    bg = pyrt.background(n, n)
    ctx = pyrt.Context(pyrt.Scene("cubes", n, n))
    hist = pyrt.empty_history(n, n)
    prev = None
    for k in range(8):
        pos, nrm = turned(a, 5.0 * k) if k else (a["pos"], a["nrm"])
        if k:
            ctx.update(pos=pos, nrm=nrm)
        p = pyrt.make_params(n, n, spp, mode=pyrt.MODE_PATH, seed=1 + k)
        rgb, _, _ = ctx.render(p, bg)
        cur = ctx.render_motion(p, prev_pos=prev)
        out, length = ctx.temporal_accumulate(rgb, cur, hist)
        hist, prev = tr.next_history(out, length, cur), pos
    ref, _, _ = ctx.render(pyrt.make_params(n, n, 1024, mode=pyrt.MODE_PATH, seed=1000), bg)
    F = aov_ref.mse(out, ref) / aov_ref.mse(rgb, ref)
    print("turntable quality: F = %.4f (measured on the CPU: %.4f), mean history length %.2f" % (F, F_MEASURED, float(length.mean())))
    assert F < 1 and F <= 2 * F_MEASURED
    ctx.close()
