"""The CPU restatements of rt_render_motion and rt_temporal_accumulate (tests/temporal_ref.py) against things that do not
share their formulas: a static frame, the forward camera ray through the reprojected position, and a running mean."""
import ctypes as C

import numpy as np
import pytest

import orc
import pyrt
import temporal_ref as tr
from temporal_ref import moved_camera, panned_camera, scene_of, turned


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("kind,w,h,pan,rng", [("lowres", 24, 24, 1.5, dict(spp=4)),
                                              ("cubes", 40, 56, 3.0, dict(spp=7, spp_begin=3, spp_count=4))])
def test_static_scene_has_zero_motion(kind, w, h, pan, rng):
    """(a) Same positions, same camera: motion exactly 0 at every hit, prev_position bit-equal to position; a miss is all
    zero with mesh 0xffffffff."""
    a = pyrt.Scene(kind, w, h).arrays()
    s = scene_of(a, camera=panned_camera(a["camera"], pan))  # (past the room's wall: some rays miss)
    a = s.arrays()
    p = pyrt.make_params(w, h, seed=11, **rng)
    for kw in (dict(), dict(prev_pos=a["pos"], prev_camera=a["camera"])):
        m = tr.motion_ref(s, p, **kw)
        hit = m["mesh"] != tr.MISS
        assert 0 < hit.sum() < w * h
        assert not m["motion"].any()
        assert np.array_equal(bits(m["prev_position"]), bits(m["position"]))
        assert not m["position"][~hit].any() and not m["prev_position"][~hit].any()


CASES = [("turn5", 5.0, None), ("turn20", 20.0, None), ("camera", 0.0, (0.11, -0.07, 0.05)), ("both", 20.0, (0.11, -0.07, 0.05))]


@pytest.mark.parametrize("name,deg,delta", CASES, ids=[c[0] for c in CASES])
def test_reprojected_position_lies_on_the_previous_cameras_ray(name, deg, delta):
    """(b) The restated motion m, added to the hit point's current screen position, names a screen position (s', t') of
    the PREVIOUS camera; the forward camera ray through it (Camera.h:27-30: lower_left + s' horizontal + t' vertical -
    position, not the inverse the restatement solves) must pass the previous-frame surface point X'.

    The bound, per pixel, from the frame's own numbers.  m is the float32 rounding of a float64 difference, so each
    component is off by at most half an ulp of itself, in pixels.  One pixel of the previous camera is, at X', a step of
    lambda |horizontal| / width (lambda |vertical| / height) in world units, lambda = qn / den being the multiple of the
    unnormalised ray direction that reaches X'.  So the ray misses X' by at most
        ulp(mx) / 2 * lambda |H| / width + ulp(my) / 2 * lambda |V| / height,
    and the test allows 4 times that (the margin for the float32 direction normalisation of a renderer's ray), plus the evaluation error of the float64 apparatus itself,
    32 * 2^-53 |X' - position| (a few dozen roundings at the scale of that distance; it only matters where m == 0).
    That bound is checked on the ray evaluated in float64.

    The oracle's own rayAt (orc_ray_at) takes s', t' as float32 and returns a float32 unit direction, which cannot resolve
    half an ulp of m: s' and t' are rounded (half an ulp of each, times lambda |H| resp. lambda |V|), each component of
    the unnormalised direction takes 4 roundings at the scale M = |lower_left| + |H| + |V| + |position| and the
    normalisation 3 more, an angle of at most sqrt(3) (4 M / |direction| + 3) 2^-24 seen from |X' - position| away.
    Its ray is held to the first bound plus exactly those terms."""
    w = h = 24
    s0 = pyrt.Scene("lowres", w, h)
    a = s0.arrays()
    pos, nrm = turned(a, deg) if deg else (a["pos"], a["nrm"])
    cam = moved_camera(a["camera"], delta) if delta else a["camera"]
    cur = scene_of(a, pos=pos, nrm=nrm, camera=cam)
    p = pyrt.make_params(w, h, 4, seed=3)
    m = tr.motion_ref(cur, p, prev_pos=a["pos"], prev_camera=a["camera"])
    ok = m["hit"] & np.isfinite(m["motion"]).all(axis=-1)
    assert ok.sum() > 50
    moving = ok & (m["motion"] != 0).any(axis=-1)
    assert moving.sum() > 20, "the case moves nothing"
    pc = a["camera"].astype(np.float64)
    av, H, V = pc[1] - pc[0], pc[2], pc[3]
    nH, nV = np.linalg.norm(H), np.linalg.norm(V)
    M = np.linalg.norm(pc[1]) + nH + nV + np.linalg.norm(pc[0])
    worst = worst32 = 0.0
    for y, x in zip(*np.nonzero(ok)):
        mx, my = m["motion"][y, x]
        sp, tp = (m["sx"][y, x] + float(mx)) / w, 1.0 - (m["sy"][y, x] + float(my)) / h
        q = m["prev_position"][y, x].astype(np.float64) - pc[0]
        lam = m["lam_prev"][y, x]
        assert lam > 0
        bound = 4 * (np.spacing(np.abs(mx)) / 2 * lam * nH / w + np.spacing(np.abs(my)) / 2 * lam * nV / h)
        bound += 32 * 2.0 ** -53 * np.linalg.norm(q)
        d = av + sp * H + tp * V
        dist = np.linalg.norm(np.cross(q, d)) / np.linalg.norm(d)
        worst = max(worst, dist / bound)
        assert dist <= bound, (x, y, dist, bound)
        # the oracle's rayAt, float32
        o3, d3 = np.zeros(3, np.float32), np.zeros(3, np.float32)
        pcam = pyrt.Camera.from_buffer_copy(np.ascontiguousarray(a["camera"], np.float32).tobytes())
        orc.lib().orc_ray_at(C.byref(pcam), float(np.float32(sp)), float(np.float32(tp)), orc._p(o3), orc._p(d3))
        assert np.array_equal(o3, a["camera"][0])
        d32 = d3.astype(np.float64)
        dist32 = np.linalg.norm(np.cross(q, d32)) / np.linalg.norm(d32)
        bound32 = bound + (np.spacing(np.float32(abs(sp))) / 2 * lam * nH + np.spacing(np.float32(abs(tp))) / 2 * lam * nV
                           + np.sqrt(3) * (4 * M / np.linalg.norm(d) + 3) * 2.0 ** -24 * np.linalg.norm(q))
        worst32 = max(worst32, dist32 / bound32)
        assert dist32 <= bound32, (x, y, dist32, bound32)
    print("%s: %d pixels (%d moving), worst distance / bound: float64 ray %.3f, orc_ray_at %.3f"
          % (name, ok.sum(), moving.sum(), worst, worst32))


def test_static_sequence_is_the_running_mean():
    """(c) n frames of a static scene (the colour's seed changes, the motion pass's does not), alpha_min 0, max_history
    >= n: every hit pixel's output is the float64 running mean m_k = m_(k-1) + (c_k - m_(k-1)) / k, rounded to float32 after
    every frame as the rule rounds it, and its length is k; a miss shows the current frame with length 1."""
    w = h = 24
    n = 6
    a = pyrt.Scene("lowres", w, h).arrays()
    s = scene_of(a, camera=panned_camera(a["camera"], 1.5))
    bg = pyrt.background(w, h)
    cur = tr.motion_ref(s, pyrt.make_params(w, h, 4, seed=1))
    hit = cur["mesh"] != tr.MISS
    assert 0 < hit.sum() < w * h
    hist = pyrt.empty_history(w, h)
    mean = None
    for k in range(1, n + 1):
        c, _, _ = orc.render(s, pyrt.make_params(w, h, 4, seed=100 + k), math_mode=orc.MATH_DET, bg=bg)
        out, length, info = tr.accumulate_ref(c, cur, hist, max_history=n, scene=s)
        c64 = c.astype(np.float64)
        mean = c if k == 1 else (mean.astype(np.float64) + (1.0 / k) * (c64 - mean.astype(np.float64))).astype(np.float32)
        assert np.array_equal(bits(out[hit]), bits(mean[hit])), k
        assert (length[hit] == k).all() and (length[~hit] == 1).all()
        assert np.array_equal(bits(out[~hit]), bits(c[~hit]))
        assert info["miss"] == int((~hit).sum()) and info["history"] == (int(hit.sum()) if k > 1 else 0)
        hist = tr.next_history(out, length, cur)
    # ... and it is a mean: close to the plain float64 average of the n frames
    frames = [orc.render(s, pyrt.make_params(w, h, 4, seed=100 + k), math_mode=orc.MATH_DET, bg=bg)[0] for k in range(1, n + 1)]
    assert np.allclose(out[hit], np.mean(np.asarray(frames, np.float64), axis=0)[hit], rtol=1e-5, atol=1e-6)
