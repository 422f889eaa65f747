"""What adaptive sampling (rt_render_adaptive) saves on the preset scenes, and what it costs.  Per workload: a reference
frame of --ref-spp samples with another seed; then per threshold one adaptive frame (passes of --pass samples, at most
--max-passes of them) and a uniform frame (rt_render) with the SAME total pixel-samples, both scored by their MSE
against the reference.  One JSON row per (workload, threshold):
  spp_mean                pixel_samples / pixels of the adaptive frame (the uniform frame's spp, rounded)
  mse_adaptive / _uniform MSE of the resolved image against the reference (float64 over all channels)
  relmse_adaptive / _uniform  the same relative to the reference: mean of (a - r)^2 / (r^2 + 0.01) — closer to what
                          the retirement rule targets (a relative standard error)
  active                  fraction of the granules each pass rendered
  render_ms / adapt_ms    device time of the render passes / of the statistics and compaction kernels
  total_ms                wall time of the call; uniform_ms: kernel time of the uniform frame
  ms_per_gsample          render_ms per 1e9 pixel-samples, adaptive and uniform (the tail: late passes with few
                          granules leave most CUs idle)
The threshold-0 row runs every pass over the whole frame: the cost of the pass structure itself.

  python tools/adaptive_bench.py [--workloads C2 C4] [--thresholds 0 0.2 0.1 0.05] [--out file.jsonl]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ray-tracing-engine_amd"))
import pyrt  # noqa: E402

# name: (scene, width, height) — bench.py WORKLOADS
WORKLOADS = {"C2": ("lowres", 1024, 1024), "C4": ("hires", 2048, 2048)}


def mse(a, b):
    return float(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))


def relmse(a, b):
    b = b.astype(np.float64)
    return float(np.mean((a.astype(np.float64) - b) ** 2 / (b * b + 0.01)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", nargs="+", default=["C2", "C4"], choices=sorted(WORKLOADS))
    ap.add_argument("--thresholds", nargs="+", type=float, default=[0.0, 0.2, 0.1, 0.05])
    ap.add_argument("--pass", dest="pass_spp", type=int, default=16)
    ap.add_argument("--max-passes", type=int, default=64)
    ap.add_argument("--min-passes", type=int, default=0)
    ap.add_argument("--floor", type=float, default=0.)
    ap.add_argument("--ref-spp", type=int, default=1024)
    ap.add_argument("--out", default=None, help="also write the rows to this file (JSON lines)")
    args = ap.parse_args()
    with open(args.out, "w") if args.out else open(os.devnull, "w") as f:
        for wl in args.workloads:
            kind, w, h = WORKLOADS[wl]
            t0 = time.time()
            s = pyrt.Scene(kind, w, h)
            ctx = pyrt.Context(s)
            bg = pyrt.background(w, h)
            ref, _, rst = ctx.render(pyrt.make_params(w, h, args.ref_spp, mode=pyrt.MODE_PATH, seed=9001), bg, want_accum=False)
            print("%s: reference %d spp in %.1f ms (set-up %.1f s)" % (wl, args.ref_spp, rst.kernel_ms, time.time() - t0), flush=True)
            p = pyrt.make_params(w, h, args.pass_spp, mode=pyrt.MODE_PATH, seed=1)
            ctx.render_adaptive(p, bg, 0.1, 2)  # (warm-up: scratch, kernels)
            for t in args.thresholds:
                out, _, spp, rep, _ = ctx.render_adaptive(p, bg, t, args.max_passes, args.min_passes, args.floor)
                n = rep.pixel_samples / float(w * h)
                nu = max(1, int(round(n)))
                ctx.render(pyrt.make_params(w, h, nu, mode=pyrt.MODE_PATH, seed=1), bg, want_accum=False)  # (warm-up)
                uni, _, ust = ctx.render(pyrt.make_params(w, h, nu, mode=pyrt.MODE_PATH, seed=1), bg, want_accum=False)
                act = [round(a / rep.granules, 4) for a in list(rep.active)[:min(rep.passes, 64)]]
                row = dict(workload=wl, threshold=t, pass_spp=args.pass_spp, max_passes=args.max_passes,
                           min_passes=args.min_passes or min(4, args.max_passes), floor=args.floor or 0.01,
                           passes=rep.passes, spp_mean=round(n, 2), spp_max=int(spp.max()), spp_min=int(spp.min()),
                           uniform_spp=nu, mse_adaptive=mse(out, ref), mse_uniform=mse(uni, ref),
                           relmse_adaptive=relmse(out, ref), relmse_uniform=relmse(uni, ref),
                           render_ms=round(rep.render_ms, 3), adapt_ms=round(rep.adapt_ms, 3), total_ms=round(rep.total_ms, 3),
                           uniform_ms=round(ust.kernel_ms, 3),
                           ms_per_gsample=round(rep.render_ms / (rep.pixel_samples / 1e9), 2),
                           ms_per_gsample_uniform=round(ust.kernel_ms / (w * h * nu / 1e9), 2), active=act)
                print(json.dumps(row), flush=True)
                f.write(json.dumps(row) + "\n")
            ctx.close()
            s.close()


if __name__ == "__main__":
    main()
