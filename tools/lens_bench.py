"""Device time of rt_render_lens_device beside rt_render_device on the C2 frame: `lowres`, 1024 x 1024,
128 spp, path mode, depth 3.

  render_no_persist   rt_render_device with RT_NO_PERSIST=1: k_render, the one-wave-per-workgroup family the lens
                      instances belong to — the like-for-like baseline
  render_default      rt_render_device as shipped: the persistent LDS-tree kernel
  lens_a0             rt_render_lens_device at aperture 0: the same frame through the lens instances (the cost of the
                      record, the wave-uniform branch and the dividing unit3)
  lens_small / _large aperture 0.02 and 0.3, focused at 2.5: the generator, and primary rays that no longer leave one point

The environment variable is read once per process, so the sweep runs in two child processes, one after the other: one
with RT_NO_PERSIST=1 (render_no_persist and, beside it, the three lens rows again: they do not depend on the variable,
which the repetition shows) and one without.  Inside a process every shape is warmed, then the shapes take turns launch by
launch for --repeats rounds.  Every figure is the library's own event pair round the kernel (rt_stats.kernel_ms); a row
carries the median and the spread (min, max) of its identical launches.

  python tools/lens_bench.py [--repeats 5] [--warmup 2] [--out profiles/lens/lens_bench.jsonl]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENE, SIZE, SPP = "lowres", 1024, 128
FOCUS, SMALL, LARGE = 2.5, 0.02, 0.3


def child(args):
    sys.path.insert(0, os.path.join(ROOT, "ray-tracing-engine_amd"))
    import torch
    import pyrt
    no_persist = os.environ.get("RT_NO_PERSIST") is not None
    stream = torch.cuda.current_stream()
    ctx = pyrt.Context(pyrt.Scene(SCENE, SIZE, SIZE))
    p = pyrt.make_params(SIZE, SIZE, SPP, mode=pyrt.MODE_PATH, max_depth=3, seed=1)
    acc = torch.zeros((SIZE, SIZE, 4), dtype=torch.float32, device="cuda")

    def frame():
        return ctx.render_device(p, acc.data_ptr(), stream=stream.cuda_stream, stats=True)

    def lens(a):
        return lambda: ctx.render_lens_device(p, pyrt.make_lens(a, FOCUS), acc.data_ptr(), stream=stream.cuda_stream, stats=True)

    shapes = {"render_no_persist" if no_persist else "render_default": frame, "lens_a0": lens(0.0), "lens_small": lens(SMALL),
              "lens_large": lens(LARGE)}
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
        print(json.dumps(dict(shape=k, rt_no_persist=no_persist, scene=SCENE, width=SIZE, height=SIZE, spp=SPP, repeats=len(v),
                              kernel_ms=round(med, 3), ms_min=round(v[0], 3), ms_max=round(v[-1], 3),
                              spread_pct=round(100 * (v[-1] - v[0]) / med, 2), rays=rays, grays_s=round(rays / med / 1e6, 3),
                              aperture={"lens_a0": 0.0, "lens_small": SMALL, "lens_large": LARGE}.get(k),
                              focus_distance=FOCUS if k.startswith("lens") else None)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lens", "lens_bench.jsonl"))
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    rows = []
    for no_persist in (True, False):
        env = dict(os.environ)
        env.pop("RT_NO_PERSIST", None)
        if no_persist:
            env["RT_NO_PERSIST"] = "1"
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--repeats", str(args.repeats), "--warmup", str(args.warmup)],
                           env=env, stdout=subprocess.PIPE, text=True, check=True)
        rows += [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
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
