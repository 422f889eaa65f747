#!/usr/bin/env python3
"""The defaults of rt_temporal_params and the quality figure of DESIGN.md "Motion vectors and temporal accumulation", on
the CPU: oracle frames (the GPU's frames bit for bit) through the numpy restatement tests/temporal_ref.py.

Two 8-frame turntable sequences at 128x128, 4 spp, path mode (slot 3 turned 5 degrees per frame; `cubes` with a fixed
camera, `lowres` with the camera drifting as well), seeds differing per frame.  Score of a setting:
F = MSE(temporal frame 8, reference) / MSE(raw frame 8, reference), the reference being frame 8 at --ref-spp samples of
another seed.  Prints one JSON line per setting, then the figure for the defaults and for temporal followed by the
a-trous filter.  Needs no GPU.    usage: tools/temporal_sweep.py [--ref-spp 1024] [--size 128] > sweep.jsonl"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "ray-tracing-engine_amd"), ROOT]
import aov_ref  # noqa: E402
import orc  # noqa: E402
import pyrt  # noqa: E402
import temporal_ref as tr  # noqa: E402

FRAMES, SPP, STEP_DEG = 8, 4, 5.0


def turntable(a, drift):
    out = []
    for k in range(FRAMES):
        pos, nrm = tr.turned(a, STEP_DEG * k) if k else (a["pos"], a["nrm"])
        cam = tr.moved_camera(a["camera"], (0.02 * k, 0.01 * k, 0.0)) if drift else a["camera"]
        out.append(dict(pos=pos, nrm=nrm, camera=cam, seed=1 + k))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref-spp", type=int, default=1024)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--no-sweep", action="store_true", help="only the defaults' figures")
    args = ap.parse_args()
    n = args.size
    bg = pyrt.background(n, n)
    seqs = []
    for kind, drift in (("cubes", False), ("lowres", True)):
        a = pyrt.Scene(kind, n, n).arrays()
        frames = turntable(a, drift)
        scenes = [tr.scene_of(a, pos=f["pos"], nrm=f["nrm"], camera=f["camera"]) for f in frames]
        params = lambda k, frames=frames: pyrt.make_params(n, n, SPP, mode=pyrt.MODE_PATH, seed=frames[k]["seed"])
        rgbs = [orc.render(s, params(k), math_mode=orc.MATH_DET, bg=bg, accel=orc.ACCEL_OBVH)[0] for k, s in enumerate(scenes)]
        ref = orc.render(scenes[-1], pyrt.make_params(n, n, args.ref_spp, mode=pyrt.MODE_PATH, seed=1000), math_mode=orc.MATH_DET,
                         bg=bg, accel=orc.ACCEL_OBVH)[0]
        seqs.append(dict(kind=kind, a=a, frames=frames, scenes=scenes, params=params, rgbs=rgbs, ref=ref,
                         raw=aov_ref.mse(rgbs[-1], ref), diag=float(tr.default_sigma_position(scenes[-1])) / tr.SIGMA_POSITION_SCALE))

    def score(q, **kw):
        out = tr.run_sequence_ref(q["a"], q["frames"], q["rgbs"], q["params"], **kw)
        return aov_ref.mse(out[-1][1], q["ref"]) / q["raw"], out
    if not args.no_sweep:
        for mh in (4, 8, 16, 32, 64):
            for pct in (0.5, 1.0, 2.0, 5.0):
                f = [score(q, max_history=mh, sigma_position=pct / 100 * q["diag"])[0] for q in seqs]
                print(json.dumps(dict(max_history=mh, sigma_position_pct=pct, F={q["kind"]: round(x, 4) for q, x in zip(seqs, f)},
                                      mean=round(float(np.mean(f)), 4))), flush=True)
    for q in seqs:
        f, out = score(q)
        sums = aov_ref.aov_sums(q["scenes"][-1], q["params"](FRAMES - 1), accel=orc.ACCEL_OBVH)
        fd = aov_ref.mse(aov_ref.atrous(out[-1][1], sums, scene=q["scenes"][-1]), q["ref"]) / q["raw"]
        fs = aov_ref.mse(aov_ref.atrous(q["rgbs"][-1], sums, scene=q["scenes"][-1]), q["ref"]) / q["raw"]
        print(json.dumps(dict(sequence=q["kind"], defaults=True, raw_mse=q["raw"], F_temporal=round(f, 4),
                              F_temporal_then_denoise=round(fd, 4), F_denoise_alone=round(fs, 4),
                              mean_length=round(float(out[-1][2].mean()), 2))), flush=True)


if __name__ == "__main__":
    main()
