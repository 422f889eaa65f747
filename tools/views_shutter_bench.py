"""What one multi-view shutter launch (rt_render_views_shutter_device) gains over the loop a caller writes without it: per
view, a camera-only rt_update followed by rt_render_shutter_device, on one stream.  Both sides render the same views
(look-at cameras on an orbit about the point the scene's camera looks at), the same seeds, shutter records and pixels:
every view moves by SMALL over the whole exposure and every second view carries a lens.  After the warm-up and before any
timed run the two accumulators are checked bit for bit (the tool fails otherwise).  Both sides run the one-wave kernel
family, so the gain is the loop's launch tails and host synchronisations.  One JSON row per workload:
  batch_dev_ms / loop_dev_ms    device time from events around the whole batch / loop (median of --repeats)
  batch_wall_ms / loop_wall_ms  host wall time of the same, ending in a device synchronise (median)
  *_min / *_max                 the spread of the repeats
  speedup_dev / speedup_wall    loop over batch
  ns_per_sample_*               device ns per pixel-sample
Each side is warmed up --warmup times before its --repeats timed runs, the two sides alternating.  --adaptive adds one
example row of an adaptive shutter frame (rt_render_adaptive_shutter_device) beside the fixed-count frame of its budget.

  python tools/views_shutter_bench.py [--workloads c1x16 ...] [--warmup 3] [--repeats 10] [--adaptive]
                                      [--out profiles/views_shutter/views_shutter_bench.jsonl]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ray-tracing-engine_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pyrt  # noqa: E402
from views_bench import orbit, timed  # noqa: E402

# name: (scene, width, height, spp, views) — views_bench's small-frame and large-frame workloads
WORKLOADS = {
    "c1x16": ("cubes", 256, 256, 8, 16),
    "c1x64": ("cubes", 256, 256, 8, 64),
    "lowres128x64": ("lowres", 128, 128, 16, 64),
    "lowres1024x4": ("lowres", 1024, 1024, 16, 4),
}
SMALL = (0.2, 0.1, 0.0)
APERTURE, FOCUS = 0.02, 2.5  # (tools/shutter_bench.py's lens)


def moved(cam, move):
    """The camera translated by `move`: position and lower_left shifted in float32."""
    B = np.asarray(cam, np.float32).reshape(4, 3).copy()
    m = np.asarray(move, np.float32)
    B[0], B[1] = B[0] + m, B[1] + m
    return B


def shutters_of(cams):
    """Every view moves by SMALL with the shutter open throughout; the odd views carry the lens."""
    return [pyrt.make_shutter(moved(c, SMALL), 0.0, 1.0, APERTURE if j % 2 else 0.0, FOCUS) for j, c in enumerate(cams)]


def adaptive_row(warmup, repeats):
    """One example: cubes 256x256, passes of 4 samples, at most 8 passes, under a moving camera with a lens — the adaptive
    frame's wall time beside the fixed-count frame of the same budget (32 spp)."""
    import time
    w, h, P, passes, thr = 256, 256, 4, 8, 0.05
    s = pyrt.Scene("cubes", w, h)
    ctx = pyrt.Context(s)
    sh = pyrt.make_shutter(moved(s.arrays()["camera"], SMALL), 0.0, 1.0, APERTURE, FOCUS)
    bg = torch.from_numpy(pyrt.background(w, h)).cuda()
    acc = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    out = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    p, full = pyrt.make_params(w, h, P, mode=pyrt.MODE_PATH), pyrt.make_params(w, h, P * passes, mode=pyrt.MODE_PATH)
    ad, fx, rep = [], [], None
    for r in range(warmup + repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rep, _ = ctx.render_adaptive_shutter_device(p, sh, bg.data_ptr(), acc.data_ptr(), out.data_ptr(), thr, passes, stream=stream)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        acc.zero_()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        ctx.render_shutter_device(full, sh, acc.data_ptr(), stream=stream)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        if r >= warmup:
            ad.append((t1 - t0) * 1e3), fx.append((t3 - t2) * 1e3)
    ctx.close()
    return dict(workload="adaptive_c1", scene="cubes", width=w, height=h, spp_per_pass=P, max_passes=passes, threshold=thr,
                passes=rep.passes, pixel_samples=rep.pixel_samples, full_samples=w * h * P * passes,
                adaptive_wall_ms=float(np.median(ad)), adaptive_wall_ms_min=float(np.min(ad)), adaptive_wall_ms_max=float(np.max(ad)),
                fixed_wall_ms=float(np.median(fx)), fixed_wall_ms_min=float(np.min(fx)), fixed_wall_ms_max=float(np.max(fx)),
                warmup=warmup, repeats=repeats)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", nargs="+", default=list(WORKLOADS), choices=list(WORKLOADS))
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--adaptive", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "views_shutter", "views_shutter_bench.jsonl"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for wl in args.workloads:
            kind, w, h, spp, n = WORKLOADS[wl]
            s = pyrt.Scene(kind, w, h)
            cams = orbit(s.arrays()["camera"], n)
            shutters = shutters_of(cams)
            seeds = np.arange(n, dtype=np.uint32) + 1
            batch_ctx, loop_ctx = pyrt.Context(s), pyrt.Context(s)
            p = pyrt.make_params(w, h, spp, mode=pyrt.MODE_PATH)
            per_view = [pyrt.Params.from_buffer_copy(p) for _ in range(n)]
            for j in range(n):
                per_view[j].seed = int(seeds[j])
            acc_b = torch.zeros((n, h, w, 4), dtype=torch.float32, device="cuda")
            acc_l = torch.zeros_like(acc_b)
            stream = torch.cuda.current_stream().cuda_stream

            def batch():
                batch_ctx.render_views_shutter_device(p, cams, shutters, acc_b.data_ptr(), stream=stream, seeds=seeds)

            def loop():
                for j in range(n):
                    loop_ctx.update(camera=cams[j])
                    loop_ctx.render_shutter_device(per_view[j], shutters[j], acc_l[j].data_ptr(), stream=stream)

            sides = (("batch", batch, acc_b), ("loop", loop, acc_l))
            res = {"batch": ([], []), "loop": ([], [])}
            for name, fn, acc in sides:
                timed(fn, args.warmup, 0, acc)
            # the two sides bit for bit, before any timed run
            same = bool(torch.equal(acc_b.view(torch.int32), acc_l.view(torch.int32))) and bool(acc_b.any())
            if not same:
                sys.exit("%s: the batch's accumulators differ from the loop's" % wl)
            for _ in range(args.repeats):
                for name, fn, acc in sides:
                    d, wl_ = timed(fn, 0, 1, acc)
                    res[name][0].extend(d), res[name][1].extend(wl_)
            samples = n * w * h * spp
            row = dict(workload=wl, scene=kind, width=w, height=h, spp=spp, views=n, lens_views=n // 2, identical=same,
                       warmup=args.warmup, repeats=args.repeats)
            for name in ("batch", "loop"):
                d, wa = res[name]
                row.update({"%s_dev_ms" % name: float(np.median(d)), "%s_dev_ms_min" % name: float(np.min(d)),
                            "%s_dev_ms_max" % name: float(np.max(d)), "%s_wall_ms" % name: float(np.median(wa)),
                            "%s_wall_ms_min" % name: float(np.min(wa)), "%s_wall_ms_max" % name: float(np.max(wa)),
                            "ns_per_sample_%s" % name: float(np.median(d)) * 1e6 / samples})
            row["speedup_dev"] = row["loop_dev_ms"] / row["batch_dev_ms"]
            row["speedup_wall"] = row["loop_wall_ms"] / row["batch_wall_ms"]
            print(json.dumps(row), flush=True)
            f.write(json.dumps(row) + "\n")
            f.flush()
            batch_ctx.close(), loop_ctx.close()
            del acc_b, acc_l
            torch.cuda.empty_cache()
        if args.adaptive:
            row = adaptive_row(args.warmup, args.repeats)
            print(json.dumps(row), flush=True)
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
