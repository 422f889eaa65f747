#!/usr/bin/env python3
"""The defaults of rt_svgf_params and the quality figures of DESIGN.md "Variance-guided spatiotemporal filtering", on the
CPU: oracle frames (the GPU's frames bit for bit) through the numpy restatement tests/svgf_ref.py (float64 stages).

The two 8-frame turntables of tools/temporal_sweep.py (128x128, 4 spp, path mode, slot 3 turned 5 degrees per frame;
`cubes` with a fixed camera, `lowres` with the camera drifting as well; seeds differing per frame).  Score of a setting:
F = MSE(rt_svgf's frame 8, reference) / MSE(raw frame 8, reference), the reference being frame 8 at --ref-spp samples of
another seed.  Sweeps sigma_luminance x max_history (the sequences have 8 frames: a max_history of 8 or more never saturates, so 8 and 16
stand for every longer memory), then sigma_normal and sigma_position around the best pair; then, for
the defaults, F of rt_svgf, of the a-trous filter alone, of temporal accumulation alone and followed by the a-trous
filter, and the flicker of each: the mean squared difference between consecutive output frames of a STATIC scene (frame
0's) rendered with per-frame seeds.  One JSON line per row.  Needs no GPU.

  usage: tools/svgf_sweep.py [--ref-spp 1024] [--size 128] [--no-sweep] [--cache frames.pkl] > profiles/svgf/svgf_sweep.jsonl"""
import argparse
import json
import os
import pickle
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "ray-tracing-engine_amd"), ROOT]
import aov_ref  # noqa: E402
import orc  # noqa: E402
import pyrt  # noqa: E402
import svgf_ref as sv  # noqa: E402
import temporal_ref as tr  # noqa: E402

FRAMES, SPP, STEP_DEG = 8, 4, 5.0
KEEP = ("motion", "position", "prev_position", "mesh")


def turntable(a, drift, static=False):
    out = []
    for k in range(FRAMES):
        pos, nrm = tr.turned(a, STEP_DEG * k) if k and not static else (a["pos"], a["nrm"])
        cam = tr.moved_camera(a["camera"], (0.02 * k, 0.01 * k, 0.0)) if drift and not static else a["camera"]
        out.append(dict(pos=pos, nrm=nrm, camera=cam, seed=1 + k))
    return out


def sequence(kind, drift, n, ref_spp, static=False):
    """Per frame: the oracle's image, rt_render_aov's sums and rt_render_motion's channels; the reference of the last."""
    bg = pyrt.background(n, n)
    a = pyrt.Scene(kind, n, n).arrays()
    frames = turntable(a, drift, static)
    q = dict(kind=kind, static=static, rgbs=[], sums=[], curs=[], sigma=[])
    for k, f in enumerate(frames):
        s = tr.scene_of(a, pos=f["pos"], nrm=f["nrm"], camera=f["camera"])
        p = pyrt.make_params(n, n, SPP, mode=pyrt.MODE_PATH, seed=f["seed"])
        q["rgbs"].append(orc.render(s, p, math_mode=orc.MATH_DET, bg=bg, accel=orc.ACCEL_OBVH)[0])
        q["sums"].append(aov_ref.aov_sums(s, p, accel=orc.ACCEL_OBVH))
        prev = frames[k - 1] if k else f
        cur = tr.motion_ref(s, p, prev_pos=prev["pos"], prev_camera=prev["camera"], accel=orc.ACCEL_OBVH)
        q["curs"].append({c: cur[c] for c in KEEP})
        q["sigma"].append(float(tr.default_sigma_position(s)))
    if not static:
        q["ref"] = orc.render(s, pyrt.make_params(n, n, ref_spp, mode=pyrt.MODE_PATH, seed=1000), math_mode=orc.MATH_DET, bg=bg,
                              accel=orc.ACCEL_OBVH)[0]
        q["raw"] = aov_ref.mse(q["rgbs"][-1], q["ref"])
    return q


def run_svgf(q, max_history=0, sigma_position_pct=0., **kw):
    """rt_svgf's output frames over the sequence (the sigmas given explicitly: the default is 2 % of the diagonal)."""
    n = q["rgbs"][0].shape[0]
    hist, outs = sv.empty_history(n, n), []
    for k in range(FRAMES):
        sx = (sigma_position_pct or 2.0) / 2.0 * q["sigma"][k]
        o = sv.svgf_ref(q["rgbs"][k], q["sums"][k], q["curs"][k], hist, max_history=max_history, sigma_position=sx,
                        sigma_reproject=q["sigma"][k], **kw)
        outs.append(o["rgb"])
        hist = sv.next_history(o, q["curs"][k])
    return outs


def run_others(q):
    """The frames of the a-trous filter alone, of temporal accumulation alone and of the pair (defaults)."""
    n = q["rgbs"][0].shape[0]
    hist, den, tmp, pair = pyrt.empty_history(n, n), [], [], []
    for k in range(FRAMES):
        sig = q["sigma"][k]
        den.append(aov_ref.atrous(q["rgbs"][k], q["sums"][k], sigma_position=sig))
        o, l, _ = tr.accumulate_ref(q["rgbs"][k], q["curs"][k], hist, sigma_position=sig)
        tmp.append(o)
        pair.append(aov_ref.atrous(o, q["sums"][k], sigma_position=sig))
        hist = tr.next_history(o, l, q["curs"][k])
    return den, tmp, pair


def flicker(frames):
    return float(np.mean([aov_ref.mse(frames[k], frames[k - 1]) for k in range(1, len(frames))]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref-spp", type=int, default=1024)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--no-sweep", action="store_true", help="only the defaults' figures")
    ap.add_argument("--cache", help="keep the oracle's frames in this file between runs (a pickle: only load one you wrote)")
    args = ap.parse_args()
    n = args.size
    if args.cache and os.path.exists(args.cache):
        with open(args.cache, "rb") as f:
            seqs = pickle.load(f)
    else:
        seqs = [sequence("cubes", False, n, args.ref_spp), sequence("lowres", True, n, args.ref_spp),
                sequence("cubes", False, n, args.ref_spp, static=True)]
        if args.cache:
            with open(args.cache, "wb") as f:
                pickle.dump(seqs, f)
    moving, still = seqs[:2], seqs[2]

    def row(**kw):
        f = [aov_ref.mse(run_svgf(q, **kw)[-1], q["ref"]) / q["raw"] for q in moving]
        d = dict(kw)
        d.update(F={q["kind"]: round(x, 4) for q, x in zip(moving, f)}, mean=round(float(np.mean(f)), 4))
        print(json.dumps(d), flush=True)
        return float(np.mean(f))
    if not args.no_sweep:
        best = (np.inf, None)
        for sl in (1.0, 2.0, 4.0, 8.0):
            for mh in (2, 3, 4, 6, 8, 16):
                best = min(best, (row(sigma_luminance=sl, max_history=mh), (sl, mh)))
        sl, mh = best[1]
        for snv in (0.25, 0.5, 1.0):
            row(sigma_luminance=sl, max_history=mh, sigma_normal=snv)
        for pct in (1.0, 2.0, 5.0):
            row(sigma_luminance=sl, max_history=mh, sigma_position_pct=pct)
    for q in moving:
        den, tmp, pair = run_others(q)
        F = lambda x: round(aov_ref.mse(x[-1], q["ref"]) / q["raw"], 4)
        print(json.dumps(dict(sequence=q["kind"], defaults=True, raw_mse=q["raw"], F_svgf=F(run_svgf(q)), F_denoise_alone=F(den),
                              F_temporal=F(tmp), F_temporal_then_denoise=F(pair))), flush=True)
    den, tmp, pair = run_others(still)
    print(json.dumps(dict(sequence="cubes, static, per-frame seeds", flicker=dict(
        raw=flicker(still["rgbs"]), svgf=flicker(run_svgf(still)), denoise_alone=flicker(den), temporal=flicker(tmp),
        temporal_then_denoise=flicker(pair)))), flush=True)


if __name__ == "__main__":
    main()
