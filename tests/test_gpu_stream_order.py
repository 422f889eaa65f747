"""The `_device` forms on a busy non-blocking stream, back to back (DESIGN.md "Stream order").

Every call here is issued while its stream still runs a delay (tests/busystream.py): the device inputs hold poison — another
valid input of the same kind — until copies behind the delay give them their contents, the outputs hold a sentinel, and an
accumulator is zeroed behind the delay.  Whatever the library does outside the caller's stream (a blocking copy on the
null stream, scratch freed under a launch that still reads it, staging overwritten before its upload ran) then gives a
wrong frame.  Expected values: the host form of the same call on a second, fresh context, bit for bit; one case is also
tied to the CPU oracle directly.  `still busy` after the last call proves that the inputs were poison when the calls were
issued; the pairs that regrow scratch may block in hipFree and only print it."""
import functools
import os

import numpy as np
import pytest
import torch

import orc
import pyrt
import pyrt.dist as rdist
import temporal_ref as tr
import transform_ref as xf
from busystream import MISS, Busy
from raybatch import ray_batch
from test_gpu_aov_views import orbit, pad_rule

pytestmark = pytest.mark.gpu

Q8 = os.environ.get("RT_NODES") == "q8"
needs_refit = pytest.mark.skipif(Q8, reason="RT_NODES_Q8 contexts cannot be refit")

AOV, AOV4 = pyrt.AOV_CHANNELS, ("albedo", "normal", "position", "hits")
MOTION, MOTION3 = pyrt.MOTION_CHANNELS, ("motion", "prev_position", "mesh")
W, H = 37, 29  # more than one wave tile each way, no multiple of 8


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_bits(got, exp, what):
    assert sorted(got) == sorted(exp), what
    for k in exp:
        g = got[k].numpy() if hasattr(got[k], "numpy") else got[k]
        assert g.shape == exp[k].shape, (what, k, g.shape, exp[k].shape)
        ne = bits(g) != bits(exp[k])
        assert not ne.any(), "%s: %s differs in %d of %d words" % (what, k, int(ne.sum()), ne.size)


def differing(e1, e2):
    """Fraction of the output words in which two host-form results differ (over what they have in common)."""
    ne = n = 0
    for k in e1:
        x, y = bits(e1[k]).reshape(-1), bits(e2[k]).reshape(-1)
        m = min(len(x), len(y))
        ne, n = ne + int((x[:m] != y[:m]).sum()), n + m
    return ne / n


def assert_distinct(e1, e2, what):
    f = differing(e1, e2)
    assert f >= 0.1, "%s: the two host-form results differ in %.3f of their words only: a swap could pass" % (what, f)


def close_all(*ctxs):
    for c in ctxs:
        c.close()


def two(kind, w=W, h=H):
    s = pyrt.Scene(kind, w, h)
    return s, s.arrays(), pyrt.Context(s), pyrt.Context(s)


def tri_limit(a):
    return int(np.diff(a["tri_begin"]).max())


def channel_limit(a, k, spp):
    return {"mesh": len(a["tri_begin"]) - 1, "tri": tri_limit(a), "hits": spp + 1}.get(k)


def late(b, a, real, poison, k, spp=2):
    """Channel k of an AOV, motion or history set: index channels within the scene's ranges; maps that two frames may share
    need not differ."""
    return b.late(real[k], poison[k], limit=channel_limit(a, k, spp), distinct=k not in ("mesh", "hits", "length"))


def ptrs(d):
    return {k: v.ptr for k, v in d.items()}


def run(b, issues, expected, what, regrow=False, between=None):
    """Behind one delay: every issue() (it returns its output buffers), still_busy, the copies, one synchronisation."""
    b.start()
    outs = []
    for i, f in enumerate(issues):
        o = f()
        outs.append({k: b.fetch(v) for k, v in o.items()} if between and i in between else o)
    busy = b.issued()
    got = [{k: (v if between and i in between else b.fetch(v)) for k, v in o.items()} for i, o in enumerate(outs)]
    b.finish()
    print("%s: issued in %.3f ms, still busy: %s%s" % (what, b.issue_ms, busy, " (regrow: may block in hipFree)" if regrow else ""))
    for i, (g, e) in enumerate(zip(got, expected)):
        assert_bits(g, e, "%s, call %d" % (what, i))
    if not regrow:
        assert busy, "%s: the delay ended before the calls were issued (%.3f ms): the inputs may not have been poison" % (what, b.issue_ms)
    return busy


# ---- the calls: each maker registers buffers with b, computes the host form on `ref` and returns (issue, expected) ------
def mk_render(b, ctx, ref, p, acc=None):
    acc = acc or b.out((p.height, p.width, 4), zeroed=True)
    exp = ref.render(p)[1]
    return (lambda: (ctx.render_device(p, acc.ptr, stream=b.ptr), {"accum": acc})[1]), {"accum": exp}


def mk_views(b, ctx, ref, p, cams, seeds):
    acc = b.out((len(cams), p.height, p.width, 4), zeroed=True)
    exp = ref.render_views(p, cams, None, seeds=seeds)[1]
    return (lambda: (ctx.render_views_device(p, cams, acc.ptr, stream=b.ptr, seeds=seeds), {"accum": acc})[1]), {"accum": exp}


def aov_outs(b, shape, channels=AOV):
    return {k: b.out(shape + ((3,) if k in pyrt.AOV_FLOAT3 else ()), np.float32 if k in pyrt.AOV_FLOAT3 or k == "depth" else np.uint32)
            for k in channels}


def mk_aov(b, ctx, ref, p):
    out = aov_outs(b, (p.height, p.width))
    exp = ref.render_aov(p, raw=True)
    return (lambda: (ctx.render_aov_device(p, ptrs(out), stream=b.ptr), out)[1]), exp


def mk_aov_views(b, ctx, ref, p, cams, seeds):
    out = aov_outs(b, (len(cams), p.height, p.width))
    exp = ref.render_aov_views(p, cams, seeds=seeds)
    return (lambda: (ctx.render_aov_views_device(p, cams, ptrs(out), stream=b.ptr, seeds=seeds), out)[1]), exp


def mk_ao(b, ctx, ref, p, n_rays, **kw):
    h, w = p.height, p.width
    out = dict(unoccluded=b.out((h, w), np.uint32), hits=b.out((h, w), np.uint32), bent=b.out((h, w, 3)))
    exp = ref.render_ao(p, n_rays, **kw)
    return (lambda: (ctx.render_ao_device(p, n_rays, ptrs(out), stream=b.ptr, **kw), out)[1]), exp


def motion_outs(b, shape):
    return dict(motion=b.out(shape + (2,)), position=b.out(shape + (3,)), prev_position=b.out(shape + (3,)), mesh=b.out(shape, np.uint32))


def mk_motion(b, ctx, ref, p, prev_pos, poison_pos, prev_camera):
    out = motion_outs(b, (p.height, p.width))
    d_prev = b.late(prev_pos, poison_pos)
    exp = ref.render_motion(p, prev_pos=prev_pos, prev_camera=prev_camera)
    return (lambda: (ctx.render_motion_device(p, ptrs(out), d_prev_pos=d_prev.ptr, prev_camera=prev_camera, stream=b.ptr), out)[1]), exp


def mk_motion_views(b, ctx, ref, p, cams, seeds, prev_pos, poison_pos, prev_cams):
    out = motion_outs(b, (len(cams), p.height, p.width))
    d_prev = b.late(prev_pos, poison_pos)
    exp = ref.render_motion_views(p, cams, prev_pos=prev_pos, prev_cameras=prev_cams, seeds=seeds)
    return (lambda: (ctx.render_motion_views_device(p, cams, ptrs(out), d_prev_pos=d_prev.ptr, prev_cameras=prev_cams, stream=b.ptr,
                                                     seeds=seeds), out)[1]), exp


def mk_rays(b, ctx, ref, p, rays, poison_rays, index=None, poison_index=None):
    n = len(rays)
    acc = b.out((n, 4), zeroed=True)
    d_rays = b.late(rays, poison_rays)
    d_idx = None if index is None else b.late(index, poison_index, limit=n)
    exp = ref.render_rays(p, rays, stream_index=index)[1]
    return (lambda: (ctx.render_rays_device(p, d_rays.ptr, n, acc.ptr, d_stream_index=d_idx.ptr if d_idx else None, stream=b.ptr),
                     {"accum": acc})[1]), {"accum": exp}


def mk_denoise(b, ctx, ref, a, f, g, spp, **kw):
    """f: the frame's inputs (frame_inputs), g: another frame's of the same size, the poison."""
    h, w = f["rgb"].shape[:2]
    d_rgb = b.late(f["rgb"], g["rgb"])
    d_aov = {k: late(b, a, f["sums"], g["sums"], k, spp) for k in AOV4}
    out = b.out((h, w, 3))
    exp = ref.denoise(f["rgb"], f["sums"], **kw)
    return (lambda: (ctx.denoise_device(w, h, d_rgb.ptr, ptrs(d_aov), out.ptr, stream=b.ptr, **kw), {"out": out})[1]), {"out": exp}


def mk_denoise_batch(b, ctx, ref, a, fs, gs, spp):
    h, w = fs[0]["rgb"].shape[:2]
    stack = lambda xs, pick: np.stack([pick(x) for x in xs])
    rgb, prgb = stack(fs, lambda x: x["rgb"]), stack(gs, lambda x: x["rgb"])
    sums = {k: stack(fs, lambda x: x["sums"][k]) for k in AOV4}
    d_rgb = b.late(rgb, prgb)
    d_aov = {k: late(b, a, sums, {k: stack(gs, lambda x: x["sums"][k])}, k, spp) for k in AOV4}
    out = b.out(rgb.shape)
    exp = ref.denoise_batch(rgb, sums)
    return (lambda: (ctx.denoise_batch_device(w, h, len(fs), d_rgb.ptr, ptrs(d_aov), out.ptr, stream=b.ptr), {"out": out})[1]), {"out": exp}


def stream_queue(rays):
    """rt_trace_stream_device's queue of `rays`: three any-hit rays, then a closest-hit ray, like a path vertex."""
    n = len(rays)
    anyk = (np.arange(n) % 4) != 3
    O, D = np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32)
    O[:, 0:3], D[:, 0:3] = rays["origin"], rays["direction"]
    O[:, 3] = anyk.astype(np.uint32).view(np.float32)
    return O, D, anyk


def mk_trace_stream(b, ctx, ref, a, rays, poison_rays):
    """Expected from rt_trace on `ref` (the stream kernel has no host form of its own): t bits and the global triangle id
    of the closest hits, the flag of the any-hit rays (tests/test_gpu_parity_big.py)."""
    n = len(rays)
    O, D, anyk = stream_queue(rays)
    pO, pD, _ = stream_queue(poison_rays)
    dO, dD, res = b.late(O, pO), b.late(D, pD), b.out((n, 2), np.uint32)
    ha, hc = ref.trace(rays, pyrt.ACCEL_BVH, pyrt.TRACE_ANY), ref.trace(rays, pyrt.ACCEL_BVH)
    hit = hc["hit"] == 1
    exp = np.full((n, 2), MISS, np.uint32)
    exp[hit, 0], exp[hit, 1] = bits(hc["d"])[hit], (a["tri_begin"][np.where(hit, hc["mesh"], 0)] + hc["tri"])[hit]
    exp[anyk, 0], exp[anyk, 1] = ha["hit"][anyk].astype(np.uint32), 0
    return (lambda: (ctx.trace_stream_device(dO.ptr, dD.ptr, n, res.ptr, stream=b.ptr), {"res": res})[1]), {"res": exp}


# ---- shared inputs, computed once ------------------------------------------------------------------------------------
def finite_rays(scene, n, seed):
    """The parity tests' batch without its NaN ray (poison is never NaN)."""
    r = ray_batch(scene, n, seed)
    bad = ~np.isfinite(r["direction"]).all(axis=1)
    r["direction"][bad] = np.float32([0.0, 0.0, -1.0])
    return r


def near_views(a, degs, scales, pad):
    """Look-at cameras on orbits inside the context camera's distance: none asks for a wider box padding (no refit, so the
    views forms stay asynchronous, and RT_NODES_Q8 contexts take them)."""
    cams = orbit(a["camera"], degs, scales)
    assert all(pad_rule(dict(a, camera=c)) <= pad for c in cams), "a view needs a refit"
    return cams


@functools.lru_cache(maxsize=None)
def sequence(kind, w, h, spp=2):
    """Three animated frames through the host forms: slot 3 turned by 5 k degrees, a camera of its own per frame.  Per
    frame: p, pos, nrm, camera, rgb, sums (rt_render_aov), cur (rt_render_motion against the frame before)."""
    s = pyrt.Scene(kind, w, h)
    a = s.arrays()
    ctx = pyrt.Context(s)
    bg = pyrt.background(w, h)
    cams = [a["camera"], tr.moved_camera(a["camera"], (0.05, 0.0, 0.0)), tr.moved_camera(a["camera"], (0.04, 0.02, 0.0))]
    out, prev = [], None
    for k in range(3):
        pos, nrm = tr.turned(a, 5.0 * k) if k else (a["pos"], a["nrm"])
        p = pyrt.make_params(w, h, spp, seed=30 + k)
        if not Q8:
            ctx.update(pos=pos, nrm=nrm, camera=cams[k])
        else:  # (no refit: the frames differ by their seeds alone, the motion comes from the previous positions and camera)
            pos, nrm, cams[k] = a["pos"], a["nrm"], a["camera"]
        f = dict(p=p, pos=pos, nrm=nrm, camera=cams[k], rgb=ctx.render(p, bg)[0], sums=ctx.render_aov(p, raw=True),
                 cur=ctx.render_motion(p, prev_pos=prev["pos"] if prev else tr.turned(a, -5.0)[0],
                                       prev_camera=prev["camera"] if prev else tr.moved_camera(a["camera"], (-0.05, 0.0, 0.0))))
        assert np.isfinite(f["cur"]["motion"]).all()
        out.append(f)
        prev = dict(pos=tr.turned(a, 5.0 * k)[0], camera=tr.moved_camera(a["camera"], (0.05 * k, 0.0, 0.0))) if Q8 else f
    ctx.close()
    return out


@functools.lru_cache(maxsize=None)
def frame_inputs(kind, w, h, seed, spp=2):
    """rgb and AOV sums of one frame through the host forms."""
    ctx = pyrt.Context(pyrt.Scene(kind, w, h))
    p = pyrt.make_params(w, h, spp, seed=seed)
    f = dict(rgb=ctx.render(p, pyrt.background(w, h))[0], sums=ctx.render_aov(p, raw=True))
    ctx.close()
    return f


# ---- a. each asynchronous form alone behind the delay -----------------------------------------------------------------
@pytest.mark.parametrize("variant", ["pooled", "no_pool", "wavefront"])
@pytest.mark.parametrize("kind", ["cubes", "lowres"])
def test_render_device_alone(kind, variant):
    s, a, ctx, ref = two(kind)
    b = Busy()
    p = pyrt.make_params(W, H, 3, seed=5, no_pool=variant == "no_pool", wavefront=variant == "wavefront")
    issue, exp = mk_render(b, ctx, ref, p)
    if variant == "pooled":  # the anchor: the host form's accumulator is the CPU oracle's
        _, oacc, _ = orc.render(s, p, math_mode=orc.MATH_DET)
        assert np.array_equal(bits(exp["accum"]), bits(oacc))
    run(b, [issue], [exp], "render_device %s %s" % (variant, kind))
    close_all(ctx, ref)


def test_resolve_device_alone():
    s, a, ctx, ref = two("lowres")
    p, q = pyrt.make_params(W, H, 3, seed=5), pyrt.make_params(W, H, 3, seed=6)
    bg = pyrt.background(W, H)
    out_rgb, acc, _ = ref.render(p, bg)
    b = Busy()
    d_acc = b.late(acc, ref.render(q)[1])
    d_bg = b.late(bg, np.ascontiguousarray(bg[::-1, ::-1]))
    out = b.out((H, W, 3))
    run(b, [lambda: (ctx.resolve_device(W, H, 3, d_acc.ptr, d_bg.ptr, out.ptr, stream=b.ptr), {"out": out})[1]], [{"out": out_rgb}],
        "resolve_device")
    close_all(ctx, ref)


VIEW_DEGS, VIEW_SCALES, SEEDS = [15.0, -40.0, 90.0], [0.7, 0.9, 0.5], [11, 12, 40000]


@pytest.mark.parametrize("form", ["views", "aov_views", "motion_views"])
def test_views_forms_alone(form):
    s, a, ctx, ref = two("lowres")
    cams = near_views(a, VIEW_DEGS, VIEW_SCALES, ctx.bvh_info().pad)
    p = pyrt.make_params(W, H, 2, seed=8)
    b = Busy()
    if form == "views":
        issue, exp = mk_views(b, ctx, ref, p, cams, SEEDS)
    elif form == "aov_views":
        issue, exp = mk_aov_views(b, ctx, ref, p, cams, SEEDS)
    else:
        issue, exp = mk_motion_views(b, ctx, ref, p, cams, SEEDS, tr.turned(a, 10.0)[0], tr.turned(a, -25.0)[0], cams[::-1])
        assert exp["motion"].any()
    run(b, [issue], [exp], form)
    close_all(ctx, ref)


def test_aov_device_alone():
    s, a, ctx, ref = two("cubes")
    b = Busy()
    issue, exp = mk_aov(b, ctx, ref, pyrt.make_params(W, H, 3, seed=4))
    run(b, [issue], [exp], "render_aov_device")
    close_all(ctx, ref)


@pytest.mark.parametrize("bias", [0.0, 2e-3], ids=["default_bias", "bias"])
def test_ao_device_alone(bias):
    s, a, ctx, ref = two("lowres")
    b = Busy()
    issue, exp = mk_ao(b, ctx, ref, pyrt.make_params(W, H, 2, seed=4), 3, bias=bias, max_distance=0.8)
    run(b, [issue], [exp], "render_ao_device bias %g" % bias)
    close_all(ctx, ref)


@pytest.mark.parametrize("indexed", [False, True], ids=["own_index", "stream_index"])
def test_rays_device_alone(indexed):
    s, a, ctx, ref = two("cubes")
    n = W * H
    rays = pyrt.pixel_rays(a["camera"], W, H)
    poison = pyrt.pixel_rays(orbit(a["camera"], [30.0], [0.8])[0], W, H)
    rng = np.random.default_rng(3)
    idx, pidx = (rng.permutation(n).astype(np.uint32), rng.permutation(n).astype(np.uint32)) if indexed else (None, None)
    b = Busy()
    issue, exp = mk_rays(b, ctx, ref, pyrt.make_params(W, H, 3, seed=9), rays, poison, idx, pidx)
    run(b, [issue], [exp], "render_rays_device")
    close_all(ctx, ref)


def test_motion_device_alone():
    s, a, ctx, ref = two("lowres")
    b = Busy()
    issue, exp = mk_motion(b, ctx, ref, pyrt.make_params(W, H, 2, seed=7), tr.turned(a, 10.0)[0], tr.turned(a, -25.0)[0],
                           tr.moved_camera(a["camera"], (0.05, 0.0, 0.0)))
    assert exp["motion"].any()
    run(b, [issue], [exp], "render_motion_device")
    close_all(ctx, ref)


def late_frame(b, a, f, g, spp=2):
    """Frame f's device inputs (rgb, AOV sums, motion channels), poisoned with frame g's."""
    return dict(rgb=b.late(f["rgb"], g["rgb"]),
                aov={k: late(b, a, f["sums"], g["sums"], k, spp) for k in AOV4},
                cur={k: late(b, a, f["cur"], g["cur"], k, spp) for k in MOTION})


def poison_history(f):
    """A valid history that is not the empty one: frame f's own image and first hits, of length 1."""
    return dict(rgb=f["rgb"], position=f["cur"]["position"], mesh=f["cur"]["mesh"], length=np.ones(f["rgb"].shape[:2], np.float32))


def test_temporal_accumulate_device_alone():
    s, a, ctx, ref = two("lowres")
    seq = sequence("lowres", W, H)
    o0, l0 = ref.temporal_accumulate(seq[0]["rgb"], seq[0]["cur"], pyrt.empty_history(W, H))
    hist = tr.next_history(o0, l0, seq[0]["cur"])
    exp = dict(zip(("rgb", "length"), ref.temporal_accumulate(seq[1]["rgb"], seq[1]["cur"], hist)))
    assert (exp["length"] == 2).sum() > 100
    b = Busy()
    d = late_frame(b, a, seq[1], seq[2])
    empty = pyrt.empty_history(W, H)
    d_hist = {k: late(b, a, hist, empty, k) for k in pyrt.HISTORY_CHANNELS}
    out = dict(rgb=b.out((H, W, 3)), length=b.out((H, W)))
    cur = {k: d["cur"][k] for k in MOTION3}
    run(b, [lambda: (ctx.temporal_accumulate_device(W, H, d["rgb"].ptr, ptrs(cur), ptrs(d_hist), out["rgb"].ptr, out["length"].ptr,
                                                    stream=b.ptr), out)[1]], [exp], "temporal_accumulate_device")
    close_all(ctx, ref)


def svgf_outs(b, w, h):
    return {k: b.out((h, w, n) if n > 1 else (h, w)) for k, n in pyrt.SVGF_OUT_CHANNELS}


def svgf_next(out, cur):
    return dict(color=out["color"], moments=out["moments"], position=cur["position"], mesh=cur["mesh"], length=out["length"])


def test_svgf_device_alone():
    s, a, ctx, ref = two("lowres")
    seq = sequence("lowres", W, H)
    o0 = ref.svgf(seq[0]["rgb"], seq[0]["sums"], seq[0]["cur"], pyrt.empty_svgf_history(W, H))
    hist = svgf_next(o0, seq[0]["cur"])
    exp = ref.svgf(seq[1]["rgb"], seq[1]["sums"], seq[1]["cur"], hist)
    assert (exp["length"] == 2).sum() > 100
    b = Busy()
    d = late_frame(b, a, seq[1], seq[2])
    empty = pyrt.empty_svgf_history(W, H)
    d_hist = {k: late(b, a, hist, empty, k) for k in pyrt.SVGF_HISTORY_CHANNELS}
    out = svgf_outs(b, W, H)
    cur = {k: d["cur"][k] for k in MOTION3}
    run(b, [lambda: (ctx.svgf_device(W, H, d["rgb"].ptr, ptrs(d["aov"]), ptrs(cur), ptrs(d_hist), ptrs(out), stream=b.ptr), out)[1]],
        [exp], "svgf_device")
    close_all(ctx, ref)


def test_denoise_device_alone():
    s, a, ctx, ref = two("cubes")
    b = Busy()
    issue, exp = mk_denoise(b, ctx, ref, a, frame_inputs("cubes", W, H, 3), frame_inputs("cubes", W, H, 4), 2)
    run(b, [issue], [exp], "denoise_device")
    close_all(ctx, ref)


def test_denoise_batch_device_alone():
    s, a, ctx, ref = two("cubes")
    fs = [frame_inputs("cubes", W, H, sd) for sd in (3, 4, 5)]
    b = Busy()
    issue, exp = mk_denoise_batch(b, ctx, ref, a, fs, fs[1:] + fs[:1], 2)
    run(b, [issue], [exp], "denoise_batch_device")
    close_all(ctx, ref)


def pack_case(b, ctx, w, h, rank, world, tile, frame, poison):
    """rt_pack_owned_device of `frame`, then rt_unpack_owned_device into a caller-zeroed frame; expected from the numpy
    statement of the granule order (pyrt.dist.owned_granule_index: the calls have no host form)."""
    p = pyrt.make_params(w, h, 1, rank=rank, world=world, tile=tile)
    n = pyrt.owned_granules(p, rank)
    d_frame, packed, back = b.late(frame, poison), b.out((n * 64, 4)), b.out((h, w, 4), zeroed=True)
    ix = rdist.owned_granule_index(w, h, rank, world, tile).reshape(-1)
    want = np.zeros((n * 64, 4), np.float32)
    want[ix >= 0] = frame.reshape(-1, 4)[ix[ix >= 0]]
    own = np.zeros((h * w, 4), np.float32)
    own[ix[ix >= 0]] = frame.reshape(-1, 4)[ix[ix >= 0]]

    def issue():
        ctx.pack_owned(p, d_frame.ptr, packed.ptr, stream=b.ptr)
        ctx.unpack_owned(p, rank, packed.ptr, back.ptr, stream=b.ptr)
        return dict(packed=packed, frame=back)
    return issue, dict(packed=want, frame=own.reshape(h, w, 4))


def test_pack_unpack_owned_device_alone():
    w, h = 45, 37
    s, a, ctx, ref = two("cubes", w, h)
    frame = (np.arange(w * h * 4, dtype=np.float32) + 1).reshape(h, w, 4)
    b = Busy()
    issue, exp = pack_case(b, ctx, w, h, 1, 3, 16, frame, -frame)
    run(b, [issue], [exp], "pack / unpack")
    close_all(ctx, ref)


def test_trace_stream_device_alone():
    s, a, ctx, ref = two("lowres")
    b = Busy()
    issue, exp = mk_trace_stream(b, ctx, ref, a, finite_rays(s, 3001, 17), finite_rays(s, 3001, 18))
    run(b, [issue], [exp], "trace_stream_device")
    close_all(ctx, ref)


# ---- b. pairs: two calls of one form back to back behind one delay -----------------------------------------------------
def run_pair(b, cases, what, regrow=False, distinct=((0, 1),)):
    for i, j in distinct:
        assert_distinct(cases[i][1], cases[j][1], what)
    return run(b, [c[0] for c in cases], [c[1] for c in cases], what, regrow=regrow)


def test_render_pair_frame_sizes():
    """40x24 then 24x40: the tile list is rebuilt (freed and uploaded again) under the first launch."""
    s, a, ctx, ref = two("cubes", 40, 24)
    b = Busy()
    cases = [mk_render(b, ctx, ref, pyrt.make_params(40, 24, 3, seed=5)), mk_render(b, ctx, ref, pyrt.make_params(24, 40, 3, seed=6))]
    run_pair(b, cases, "render_device 40x24 then 24x40", regrow=True)
    close_all(ctx, ref)


@pytest.mark.parametrize("no_pool", [False, True], ids=["pooled", "no_pool"])
def test_render_pair_ranks(no_pool):
    """Rank 0 then rank 1 of world 2, tile 16: each into its own accumulator (another tile list per rank)."""
    w, h = 45, 37
    s, a, ctx, ref = two("lowres", w, h)
    b = Busy()
    cases = [mk_render(b, ctx, ref, pyrt.make_params(w, h, 2, seed=5, rank=r, world=2, tile=16, no_pool=no_pool)) for r in (0, 1)]
    run_pair(b, cases, "render_device rank 0 then rank 1", regrow=True)
    close_all(ctx, ref)


@pytest.mark.parametrize("no_pool", [False, True], ids=["pooled", "no_pool"])
def test_render_pair_sample_ranges_and_resolve(no_pool):
    """[0, 2) then [2, 4) into ONE accumulator, resolved after each: rt_render_passes' accumulators and images."""
    s, a, ctx, ref = two("cubes")
    bg = pyrt.background(W, H)
    ps = [pyrt.make_params(W, H, 4, seed=5, spp_begin=b0, spp_count=2, no_pool=no_pool) for b0 in (0, 2)]
    acc_io = np.zeros((H, W, 4), np.float32)
    exp = []
    for p in ps:
        out, _ = ref.render_passes(p, bg, acc_io)
        exp.append(dict(accum=acc_io.copy(), out=out))
    b = Busy()
    acc, d_bg = b.out((H, W, 4), zeroed=True), b.late(bg, np.ascontiguousarray(bg[::-1, ::-1]))
    outs = [b.out((H, W, 3)), b.out((H, W, 3))]

    def issue(i):
        ctx.render_device(ps[i], acc.ptr, stream=b.ptr)
        ctx.resolve_device(W, H, 2 * (i + 1), acc.ptr, d_bg.ptr, outs[i].ptr, stream=b.ptr)
        return dict(accum=acc, out=outs[i])
    assert_distinct(exp[0], exp[1], "sample ranges")
    run(b, [lambda: issue(0), lambda: issue(1)], exp, "render_device [0,2) then [2,4) + resolve", between={0})
    close_all(ctx, ref)


def test_render_pair_wavefront_regrow():
    """The wavefront integrator on a small frame, then on one large enough to regrow its state block."""
    s, a, ctx, ref = two("lowres", 45, 37)
    b = Busy()
    cases = [mk_render(b, ctx, ref, pyrt.make_params(16, 9, 2, seed=5, wavefront=True)),
             mk_render(b, ctx, ref, pyrt.make_params(45, 37, 4, seed=6, wavefront=True))]
    run_pair(b, cases, "render_device wavefront small then large", regrow=True)
    close_all(ctx, ref)


def views_pair(form, b, ctx, ref, a, p, specs):
    """specs: (cameras, seeds, previous cameras) per call."""
    cases = []
    for k, (cams, seeds, prev) in enumerate(specs):
        if form == "views":
            cases.append(mk_views(b, ctx, ref, p, cams, seeds))
        elif form == "aov_views":
            cases.append(mk_aov_views(b, ctx, ref, p, cams, seeds))
        else:
            cases.append(mk_motion_views(b, ctx, ref, p, cams, seeds, tr.turned(a, 10.0 + 20.0 * k)[0], tr.turned(a, -25.0)[0], prev))
    return cases


@pytest.mark.parametrize("form", ["views", "aov_views", "motion_views"])
def test_views_pair_same_n(form):
    """The same n with other cameras and seeds (and other previous cameras): the second call stages its view records while
    the first call's upload has not run."""
    s, a, ctx, ref = two("lowres")
    pad = ctx.bvh_info().pad
    c1, c2 = near_views(a, VIEW_DEGS, VIEW_SCALES, pad), near_views(a, [-70.0, 120.0, 33.0], [0.6, 0.8, 0.95], pad)
    b = Busy()
    cases = views_pair(form, b, ctx, ref, a, pyrt.make_params(W, H, 2, seed=8), [(c1, SEEDS, c1[::-1]), (c2, [7, 8, 9], c1)])
    run_pair(b, cases, "%s, same n" % form)
    close_all(ctx, ref)


@pytest.mark.parametrize("form", ["views", "aov_views", "motion_views"])
def test_views_pair_capacity_regrow(form):
    """n = 2 then n = 3: the view tables (and rt_render_views' tile list) grow under the first launch."""
    s, a, ctx, ref = two("cubes")
    pad = ctx.bvh_info().pad
    c1, c2 = near_views(a, VIEW_DEGS[:2], VIEW_SCALES[:2], pad), near_views(a, [-70.0, 120.0, 33.0], [0.6, 0.8, 0.95], pad)
    b = Busy()
    cases = views_pair(form, b, ctx, ref, a, pyrt.make_params(W, H, 2, seed=8), [(c1, SEEDS[:2], c1[::-1]), (c2, [7, 8, 9], c2[::-1])])
    run_pair(b, cases, "%s, n = 2 then 3" % form, regrow=True)
    close_all(ctx, ref)


def test_views_calls_beyond_the_staging_ring():
    """Six calls behind one delay, more than the pinned staging copies the context keeps: a call that finds its copy still
    unread waits for that upload (the host may block: printed), and every frame is its own."""
    s, a, ctx, ref = two("lowres", 24, 19)
    pad = ctx.bvh_info().pad
    p = pyrt.make_params(24, 19, 1, seed=8)
    b = Busy()
    cases = [mk_aov_views(b, ctx, ref, p, near_views(a, [20.0 * k - 50.0, 10.0 * k], [0.6 + 0.05 * k, 0.9], pad), [k, 100 + k]) for k in range(6)]
    run_pair(b, cases, "aov_views x 6", regrow=True, distinct=((0, 1), (1, 2), (4, 5)))
    close_all(ctx, ref)


def test_ao_pair_default_bias():
    """Bias 0 twice: both calls reduce the scene's extent into the one block the context owns."""
    s, a, ctx, ref = two("lowres")
    b = Busy()
    cases = [mk_ao(b, ctx, ref, pyrt.make_params(W, H, 2, seed=4), 3, bias=0.0, max_distance=0.5),
             mk_ao(b, ctx, ref, pyrt.make_params(W, H, 2, seed=5), 3, bias=0.0, max_distance=1.5)]
    run_pair(b, cases, "render_ao_device, bias 0 twice")
    close_all(ctx, ref)


def test_motion_pair():
    s, a, ctx, ref = two("lowres")
    b = Busy()
    cases = [mk_motion(b, ctx, ref, pyrt.make_params(W, H, 2, seed=7), tr.turned(a, 10.0)[0], tr.turned(a, -25.0)[0],
                       tr.moved_camera(a["camera"], (0.05, 0.0, 0.0))),
             mk_motion(b, ctx, ref, pyrt.make_params(W, H, 2, seed=8), tr.turned(a, 30.0)[0], tr.turned(a, -25.0)[0],
                       tr.moved_camera(a["camera"], (0.0, 0.08, 0.0)))]
    run_pair(b, cases, "render_motion_device twice")
    close_all(ctx, ref)


def test_denoise_small_large_small():
    """17x15, then 45x37 (the filter scratch regrows), then the first frame again into a third buffer."""
    s, a, ctx, ref = two("cubes")
    small, large = [frame_inputs("cubes", 17, 15, sd) for sd in (3, 4)], [frame_inputs("cubes", 45, 37, sd) for sd in (3, 4)]
    b = Busy()
    cases = [mk_denoise(b, ctx, ref, a, small[0], small[1], 2), mk_denoise(b, ctx, ref, a, large[0], large[1], 2, iterations=3),
             mk_denoise(b, ctx, ref, a, small[0], small[1], 2)]
    run_pair(b, cases, "denoise_device small, large, small", regrow=True)
    close_all(ctx, ref)


def test_denoise_batch_pair_regrow():
    s, a, ctx, ref = two("cubes")
    fs = [frame_inputs("cubes", W, H, sd) for sd in (3, 4, 5, 6)]
    b = Busy()
    cases = [mk_denoise_batch(b, ctx, ref, a, fs[:2], fs[2:], 2), mk_denoise_batch(b, ctx, ref, a, fs[1:], fs[:3], 2)]
    run_pair(b, cases, "denoise_batch_device n = 2 then 3", regrow=True)
    close_all(ctx, ref)


def test_temporal_three_chained_frames():
    """Three frames, the history ping-ponged on the stream: frame k's outputs are frame k + 1's history, frame 2 writes
    over frame 0's."""
    s, a, ctx, ref = two("lowres")
    seq = sequence("lowres", W, H)
    hist, exp = pyrt.empty_history(W, H), []
    for f in seq:
        o, l = ref.temporal_accumulate(f["rgb"], f["cur"], hist)
        exp.append(dict(rgb=o, length=l))
        hist = tr.next_history(o, l, f["cur"])
    assert exp[2]["length"].max() == 3
    b = Busy()
    d = [late_frame(b, a, seq[k], seq[(k + 1) % 3]) for k in range(3)]
    empty, poison = pyrt.empty_history(W, H), poison_history(seq[1])
    h0 = {k: late(b, a, empty, poison, k) for k in pyrt.HISTORY_CHANNELS}
    sets = [dict(rgb=b.out((H, W, 3)), length=b.out((H, W))) for _ in range(2)]

    def issue(k):
        prev = h0 if k == 0 else dict(rgb=sets[(k - 1) % 2]["rgb"], position=d[k - 1]["cur"]["position"], mesh=d[k - 1]["cur"]["mesh"],
                                      length=sets[(k - 1) % 2]["length"])
        out = sets[k % 2]
        ctx.temporal_accumulate_device(W, H, d[k]["rgb"].ptr, ptrs({c: d[k]["cur"][c] for c in MOTION3}), ptrs(prev), out["rgb"].ptr,
                                       out["length"].ptr, stream=b.ptr)
        return out
    assert_distinct(exp[0], exp[1], "temporal"), assert_distinct(exp[1], exp[2], "temporal")
    run(b, [functools.partial(issue, k) for k in range(3)], exp, "temporal_accumulate_device x 3", between={0, 1})
    close_all(ctx, ref)


def test_svgf_three_chained_frames():
    s, a, ctx, ref = two("lowres")
    seq = sequence("lowres", W, H)
    hist, exp = pyrt.empty_svgf_history(W, H), []
    for f in seq:
        exp.append(ref.svgf(f["rgb"], f["sums"], f["cur"], hist))
        hist = svgf_next(exp[-1], f["cur"])
    b = Busy()
    d = [late_frame(b, a, seq[k], seq[(k + 1) % 3]) for k in range(3)]
    empty = pyrt.empty_svgf_history(W, H)
    poison = dict(color=seq[1]["rgb"], moments=np.ones((H, W, 2), np.float32), position=seq[1]["cur"]["position"], mesh=seq[1]["cur"]["mesh"],
                  length=np.ones((H, W), np.float32))
    h0 = {k: late(b, a, empty, poison, k) for k in pyrt.SVGF_HISTORY_CHANNELS}
    sets = [svgf_outs(b, W, H) for _ in range(2)]

    def issue(k):
        prev = h0 if k == 0 else svgf_next(sets[(k - 1) % 2], d[k - 1]["cur"])
        out = sets[k % 2]
        ctx.svgf_device(W, H, d[k]["rgb"].ptr, ptrs(d[k]["aov"]), ptrs({c: d[k]["cur"][c] for c in MOTION3}), ptrs(prev), ptrs(out),
                        stream=b.ptr)
        return out
    assert_distinct(exp[0], exp[1], "svgf"), assert_distinct(exp[1], exp[2], "svgf")
    run(b, [functools.partial(issue, k) for k in range(3)], exp, "svgf_device x 3", between={0, 1})
    close_all(ctx, ref)


def test_rays_pair_small_then_large():
    s, a, ctx, ref = two("cubes")
    p = pyrt.make_params(1, 1, 3, seed=9)
    other = orbit(a["camera"], [30.0], [0.8])[0]
    rng = np.random.default_rng(5)
    b = Busy()
    cases = [mk_rays(b, ctx, ref, p, pyrt.pixel_rays(a["camera"], 10, 10), pyrt.pixel_rays(other, 10, 10)),
             mk_rays(b, ctx, ref, pyrt.make_params(1, 1, 2, seed=10), pyrt.pixel_rays(other, 100, 50), pyrt.pixel_rays(a["camera"], 100, 50),
                     rng.permutation(5000).astype(np.uint32), rng.permutation(5000).astype(np.uint32))]
    run_pair(b, cases, "render_rays_device n = 100 then 5000")
    close_all(ctx, ref)


def test_pack_pair_ranks():
    w, h = 45, 37
    s, a, ctx, ref = two("cubes", w, h)
    frame = (np.arange(w * h * 4, dtype=np.float32) + 1).reshape(h, w, 4)
    b = Busy()
    cases = [pack_case(b, ctx, w, h, r, 2, 16, frame * (r + 1), -frame) for r in (0, 1)]
    run_pair(b, cases, "pack / unpack rank 0 then rank 1")
    close_all(ctx, ref)


def test_trace_stream_pair():
    s, a, ctx, ref = two("lowres")
    b = Busy()
    cases = [mk_trace_stream(b, ctx, ref, a, finite_rays(s, 3001, 17), finite_rays(s, 3001, 18)),
             mk_trace_stream(b, ctx, ref, a, finite_rays(s, 4999, 19), finite_rays(s, 4999, 20))]
    run_pair(b, cases, "trace_stream_device twice")
    close_all(ctx, ref)


def test_mixed_chain_on_one_context():
    """render, AOVs, ambient occlusion, views and render again on one context: the last frame is the first."""
    s, a, ctx, ref = two("lowres")
    p = pyrt.make_params(W, H, 3, seed=5)
    cams = near_views(a, VIEW_DEGS, VIEW_SCALES, ctx.bvh_info().pad)
    b = Busy()
    first = mk_render(b, ctx, ref, p)
    cases = [first, mk_aov(b, ctx, ref, pyrt.make_params(W, H, 2, seed=6)), mk_ao(b, ctx, ref, pyrt.make_params(W, H, 2, seed=7), 3),
             mk_views(b, ctx, ref, pyrt.make_params(W, H, 2, seed=8), cams, SEEDS), mk_render(b, ctx, ref, p)]
    cases[4] = (cases[4][0], first[1])
    run(b, [c[0] for c in cases], [c[1] for c in cases], "mixed chain")
    close_all(ctx, ref)


# ---- c. a frame loop ---------------------------------------------------------------------------------------------------
def loop_transforms(a, k):
    t = pyrt.make_transforms(len(a["vtx_begin"]) - 1)
    xf.set_mesh(t, 3, xf.rotation_y(5.0 * (k + 1)))
    return xf.set_mesh(t, 4, translate=(-0.03 * (k + 1), 0.02 * (k + 1), 0.03 * (k + 1)))


@needs_refit
def test_frame_loop_on_a_side_stream():
    """Three animated frames — rt_update_transforms, then render, AOVs, motion, resolve and rt_svgf on the device buffers —
    on one side stream without a synchronisation of the test's own, against the same loop through the host forms on a
    second context.  rt_update_transforms synchronises its stream by design, so the delay stands behind it."""
    s, a, ctx, ref = two("lowres")
    bg = pyrt.background(W, H)
    ps = [pyrt.make_params(W, H, 2, seed=40 + k) for k in range(3)]
    # the host loop
    exp, hist, prev_pos = [], pyrt.empty_svgf_history(W, H), a["pos"]
    for k in range(3):
        pos, nrm = xf.apply(a, loop_transforms(a, k))
        ref.update(pos=pos, nrm=nrm)
        rgb, acc, _ = ref.render(ps[k], bg)
        sums = ref.render_aov(ps[k], raw=True)
        cur = ref.render_motion(ps[k], prev_pos=prev_pos)
        out = ref.svgf(rgb, sums, cur, hist)
        exp.append(dict(accum=acc, resolved=rgb, **{"aov_" + c: sums[c] for c in AOV}, **{"cur_" + c: cur[c] for c in MOTION},
                        **{"svgf_" + c: out[c] for c in out}))
        hist, prev_pos = svgf_next(out, cur), pos
    assert exp[2]["svgf_length"].max() >= 2 and exp[1]["cur_motion"].any()
    # the device loop
    b = Busy()
    empty = pyrt.empty_svgf_history(W, H)
    poison = dict(color=exp[0]["resolved"], moments=np.ones((H, W, 2), np.float32), position=exp[0]["cur_position"], mesh=exp[0]["cur_mesh"],
                  length=np.ones((H, W), np.float32))
    h0 = {c: late(b, a, empty, poison, c) for c in pyrt.SVGF_HISTORY_CHANNELS}
    d_bg = b.late(bg, np.ascontiguousarray(bg[::-1, ::-1]))
    d_prev = b.out((len(a["pos"]), 3))
    fr = [dict(acc=b.out((H, W, 4)), rgb=b.out((H, W, 3)), aov=aov_outs(b, (H, W)), cur=motion_outs(b, (H, W)), svgf=svgf_outs(b, W, H))
          for _ in range(2)]
    got, busy = [], []
    for k in range(3):
        f, last = fr[k % 2], fr[(k - 1) % 2]
        ctx.update_transforms(loop_transforms(a, k), d_prev_pos=d_prev.ptr, stream=b.ptr)  # (synchronises the stream)
        b.start()
        with torch.cuda.stream(b.stream):
            f["acc"].t.zero_()
        ctx.render_device(ps[k], f["acc"].ptr, stream=b.ptr)
        ctx.render_aov_device(ps[k], ptrs(f["aov"]), stream=b.ptr)
        ctx.render_motion_device(ps[k], ptrs(f["cur"]), d_prev_pos=d_prev.ptr, stream=b.ptr)
        ctx.resolve_device(W, H, 2, f["acc"].ptr, d_bg.ptr, f["rgb"].ptr, stream=b.ptr)
        prev = h0 if k == 0 else svgf_next(last["svgf"], last["cur"])
        ctx.svgf_device(W, H, f["rgb"].ptr, ptrs({c: f["aov"][c] for c in AOV4}), ptrs({c: f["cur"][c] for c in MOTION3}), ptrs(prev),
                        ptrs(f["svgf"]), stream=b.ptr)
        busy.append(b.issued())
        got.append(dict(accum=b.fetch(f["acc"]), resolved=b.fetch(f["rgb"]), **{"aov_" + c: b.fetch(f["aov"][c]) for c in AOV},
                        **{"cur_" + c: b.fetch(f["cur"][c]) for c in MOTION}, **{"svgf_" + c: b.fetch(v) for c, v in f["svgf"].items()}))
        print("frame %d: issued in %.3f ms, still busy: %s" % (k, b.issue_ms, busy[-1]))
    b.finish()
    for k in range(3):
        assert_bits(got[k], exp[k], "frame %d" % k)
    assert all(busy), busy
    close_all(ctx, ref)


# ---- d. forms that read results back: they synchronise the caller's stream --------------------------------------------
COUNTERS = ("samples", "rays_closest", "rays_shadow", "nodes_visited", "tris_tested")


def stats_of(st):
    return {k: getattr(st, k) for k in COUNTERS}


def test_render_device_with_stats():
    s, a, ctx, ref = two("cubes")
    p = pyrt.make_params(W, H, 3, seed=5, collect_stats=1)
    _, exp, est = ref.render(p)
    b = Busy()
    acc = b.out((H, W, 4), zeroed=True)
    b.start()
    st = ctx.render_device(p, acc.ptr, stream=b.ptr, stats=True)
    assert b.issued() is False, "the call returned before its stream had finished"
    got = b.fetch(acc)
    b.finish()
    assert stats_of(st) == stats_of(est) and est.rays_closest > 0
    assert_bits({"accum": got}, {"accum": exp}, "render_device with stats")
    close_all(ctx, ref)


def test_render_views_device_with_stats():
    s, a, ctx, ref = two("lowres")
    cams = near_views(a, VIEW_DEGS, VIEW_SCALES, ctx.bvh_info().pad)
    p = pyrt.make_params(W, H, 2, seed=8, collect_stats=1)
    _, exp, est = ref.render_views(p, cams, None, seeds=SEEDS)
    b = Busy()
    acc = b.out((3, H, W, 4), zeroed=True)
    b.start()
    st = ctx.render_views_device(p, cams, acc.ptr, stream=b.ptr, seeds=SEEDS, stats=True)
    assert b.issued() is False
    got = b.fetch(acc)
    b.finish()
    assert stats_of(st) == stats_of(est) and est.rays_closest > 0
    assert_bits({"accum": got}, {"accum": exp}, "render_views_device with stats")
    close_all(ctx, ref)


def test_render_adaptive_device():
    s, a, ctx, ref = two("cubes")
    bg = pyrt.background(W, H)
    p = pyrt.make_params(W, H, 2, seed=5)
    kw = dict(threshold=0.01, max_passes=4, min_passes=2)
    eout, eacc, espp, erep, est = ref.render_adaptive(p, bg, **kw)
    b = Busy()
    d_bg = b.late(bg, np.ascontiguousarray(bg[::-1, ::-1]))
    acc, out, spp = b.out((H, W, 4)), b.out((H, W, 3)), b.out((H, W), np.uint32)
    b.start()
    rep, st = ctx.render_adaptive_device(p, d_bg.ptr, acc.ptr, out.ptr, d_spp=spp.ptr, stream=b.ptr, stats=True, **kw)
    assert b.issued() is False
    got = dict(out=b.fetch(out), accum=b.fetch(acc), spp=b.fetch(spp))
    b.finish()
    strip = lambda r: {k: v for k, v in r.as_dict().items() if not k.endswith("_ms")}
    assert strip(rep) == strip(erep) and 1 < erep.passes and stats_of(st) == stats_of(est)
    assert_bits(got, dict(out=eout, accum=eacc, spp=espp), "render_adaptive_device")
    close_all(ctx, ref)


@needs_refit
def test_update_vertices_device():
    """Late-filled positions and normals: the report, the tree and the next frame are rt_update's."""
    s, a, ctx, ref = two("lowres")
    pos, nrm = tr.turned(a, 20.0)
    ppos, pnrm = tr.turned(a, -35.0)
    erep = ref.update(pos=pos, nrm=nrm)
    p = pyrt.make_params(W, H, 2, seed=5)
    exp = ref.render(p)[1]
    b = Busy()
    d_pos, d_nrm = b.late(pos, ppos), b.late(nrm, pnrm)
    acc = b.out((H, W, 4), zeroed=True)
    b.start()
    rep = ctx.update_vertices_device(d_pos.ptr, d_nrm.ptr, stream=b.ptr)
    assert b.issued() is False
    ctx.render_device(p, acc.ptr, stream=b.ptr)
    got = b.fetch(acc)
    b.finish()
    assert (rep["refitted"], rep["photons_dropped"]) == (erep["refitted"], erep["photons_dropped"]) == (1, 0)
    for g, e in zip(ctx.bvh_export(), ref.bvh_export()):
        assert np.array_equal(g, e)
    assert_bits({"accum": got}, {"accum": exp}, "the frame after update_vertices_device")
    close_all(ctx, ref)
