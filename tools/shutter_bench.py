"""Device time of rt_render_shutter_device beside rt_render_device and rt_render_lens_device on the C2
frame: `lowres`, 1024 x 1024, 128 spp, path mode, depth 3.

  render_no_persist    rt_render_device with RT_NO_PERSIST=1: k_render, the one-wave-per-workgroup family the shutter
                       instances belong to — the like-for-like baseline
  lens_a0              rt_render_lens_device at aperture 0: the same frame through the lens instances
  shutter_still        rt_render_shutter_device with camera_close == the context's camera: the same frame again, now with
                       the time drawn, the camera interpolated and the dividing unit3 (the cost of the generator alone)
  shutter_small        the camera translated by (0.2, 0.1, 0) over the exposure
  shutter_large        ... by (0.6, 0.3, 0.1): primary rays that no longer leave one point
  shutter_large_lens   the large move with a lens of radius 0.02 focused at 2.5 on the moving camera

RT_NO_PERSIST is read once per process, so the sweep runs in one child process that has it set.  There every shape is
warmed, then the shapes take turns launch by launch for --repeats rounds.  Every figure is the library's own event pair
round the kernel (rt_stats.kernel_ms); a row carries the median and the spread (min, max) of its identical launches and
the ratio of its median to render_no_persist's.

  python tools/shutter_bench.py [--repeats 5] [--warmup 2] [--out profiles/shutter/shutter_bench.jsonl]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENE, SIZE, SPP = "lowres", 1024, 128
FOCUS, APERTURE = 2.5, 0.02
SMALL, LARGE = (0.2, 0.1, 0.0), (0.6, 0.3, 0.1)


def child(args):
    sys.path.insert(0, os.path.join(ROOT, "ray-tracing-engine_amd"))
    import numpy as np
    import torch
    import pyrt
    stream = torch.cuda.current_stream()
    scene = pyrt.Scene(SCENE, SIZE, SIZE)
    ctx = pyrt.Context(scene)
    p = pyrt.make_params(SIZE, SIZE, SPP, mode=pyrt.MODE_PATH, max_depth=3, seed=1)
    acc = torch.zeros((SIZE, SIZE, 4), dtype=torch.float32, device="cuda")
    A = np.asarray(scene.arrays()["camera"], np.float32).reshape(4, 3)

    def moved(m):
        B = A.copy()
        B[0], B[1] = B[0] + np.asarray(m, np.float32), B[1] + np.asarray(m, np.float32)
        return B

    def frame():
        return ctx.render_device(p, acc.data_ptr(), stream=stream.cuda_stream, stats=True)

    def lens():
        return ctx.render_lens_device(p, pyrt.make_lens(0.0, FOCUS), acc.data_ptr(), stream=stream.cuda_stream, stats=True)

    def shutter(m, aperture=0.0):
        sh = pyrt.make_shutter(moved(m), 0.0, 1.0, aperture, FOCUS)
        return lambda: ctx.render_shutter_device(p, sh, acc.data_ptr(), stream=stream.cuda_stream, stats=True)

    moves = {"shutter_still": (0.0, 0.0, 0.0), "shutter_small": SMALL, "shutter_large": LARGE, "shutter_large_lens": LARGE}
    shapes = {"render_no_persist": frame, "lens_a0": lens, "shutter_still": shutter(moves["shutter_still"]),
              "shutter_small": shutter(SMALL), "shutter_large": shutter(LARGE), "shutter_large_lens": shutter(LARGE, APERTURE)}
    ms, last = {k: [] for k in shapes}, {}
    for it in range(args.warmup + args.repeats):
        for k, fn in shapes.items():
            st = fn()
            last[k] = st
            if it >= args.warmup:
                ms[k].append(st.kernel_ms)
    ctx.close()
    for k, v in ms.items():
        v.sort()
        med, st = v[len(v) // 2], last[k]
        rays = st.rays_closest + st.rays_shadow
        print(json.dumps(dict(shape=k, rt_no_persist=True, scene=SCENE, width=SIZE, height=SIZE, spp=SPP, repeats=len(v),
                              kernel_ms=round(med, 3), ms_min=round(v[0], 3), ms_max=round(v[-1], 3),
                              spread_pct=round(100 * (v[-1] - v[0]) / med, 2), rays=rays, grays_s=round(rays / med / 1e6, 3),
                              move=moves.get(k), aperture=APERTURE if k == "shutter_large_lens" else 0.0 if k != "render_no_persist" else None)),
              flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shutter", "shutter_bench.jsonl"))
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    env = dict(os.environ)
    env["RT_NO_PERSIST"] = "1"
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--repeats", str(args.repeats), "--warmup", str(args.warmup)],
                       env=env, stdout=subprocess.PIPE, text=True, check=True)
    rows = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    base = next(r for r in rows if r["shape"] == "render_no_persist")["kernel_ms"]
    for r in rows:
        r["ratio_to_no_persist"] = round(r["kernel_ms"] / base, 4)
        print(json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        for r in rows:
            fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
