"""What the batched passes (rt_render_aov_views_device + rt_render_motion_views_device + rt_denoise_batch_device, three
calls) gain over the loop a caller writes without them: per view a camera-only rt_update, rt_render_aov_device,
rt_render_motion_device and rt_denoise_device, on one stream.  Both sides work on the same views (look-at cameras on an
orbit, last frame's cameras one step back on it), seeds, pixels and noisy frames (rt_render_views, untimed).

The loop can be timed on another build of the library (--loop-lib: the parent commit's, where those calls exist), so each
side runs in a process of its own: the driver starts them alternately, --rounds times each, and compares a digest of
every output buffer between the sides (the tool fails when they differ).  One JSON row per workload:
  batch_dev_ms / loop_dev_ms    device time from events around the three calls / the loop (median over all runs)
  batch_wall_ms / loop_wall_ms  host wall time of the same, ending in a device synchronise (median)
  *_min / *_max                 the spread of the runs
  speedup_dev / speedup_wall    loop over batch

  python tools/aov_views_bench.py [--workloads c1x16 ...] [--rounds 3] [--warmup 2] [--repeats 5] [--loop-lib path/librt_amd.so]
                                  [--out profiles/aov_views/aov_views_bench.jsonl]
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ray-tracing-engine_amd"))

# name: (scene, width, height, spp, views)   (DESIGN.md "Multi-view frames": the small frames of its table)
WORKLOADS = {
    "c1x16": ("cubes", 256, 256, 8, 16),
    "c1x64": ("cubes", 256, 256, 8, 64),
    "lowres128x64": ("lowres", 128, 128, 16, 64),
}
AOV = ("albedo", "normal", "position", "depth", "hits", "mesh", "tri")
MOTION = ("motion", "position", "prev_position", "mesh")


def side(args):
    """One side of one workload in this process: prints a JSON line of its timings and the digest of its outputs."""
    import torch
    import pyrt
    from views_bench import orbit
    kind, w, h, spp, n = WORKLOADS[args.workload]
    s = pyrt.Scene(kind, w, h)
    cams = orbit(s.arrays()["camera"], n)
    prev_cams = np.roll(cams, 1, axis=0)
    seeds = np.arange(n, dtype=np.uint32) + 1
    ctx = pyrt.Context(s)
    p = pyrt.make_params(w, h, spp, mode=pyrt.MODE_PATH)
    per_view = [pyrt.Params.from_buffer_copy(p) for _ in range(n)]
    for j in range(n):
        per_view[j].seed = int(seeds[j])
    stream = torch.cuda.current_stream().cuda_stream
    # the noisy frames, by calls both builds have
    acc = torch.zeros((n, h, w, 4), dtype=torch.float32, device="cuda")
    ctx.render_views_device(p, cams, acc.data_ptr(), stream=stream, seeds=seeds)
    bg = torch.from_numpy(pyrt.background(w, h)).cuda()
    rgb = torch.empty((n, h, w, 3), dtype=torch.float32, device="cuda")
    for j in range(n):
        ctx.resolve_device(w, h, spp, acc[j].data_ptr(), bg.data_ptr(), rgb[j].data_ptr(), stream=stream)
    f32 = lambda *shape: torch.zeros((n, h, w) + shape, dtype=torch.float32, device="cuda")
    u32 = lambda: torch.zeros((n, h, w), dtype=torch.int32, device="cuda")
    aov = dict(albedo=f32(3), normal=f32(3), position=f32(3), depth=f32(), hits=u32(), mesh=u32(), tri=u32())
    mot = dict(motion=f32(2), position=f32(3), prev_position=f32(3), mesh=u32())
    out = f32(3)
    guides = ("albedo", "normal", "position", "hits")

    def batch():
        ctx.render_aov_views_device(p, cams, {k: v.data_ptr() for k, v in aov.items()}, stream=stream, seeds=seeds)
        ctx.render_motion_views_device(p, cams, {k: v.data_ptr() for k, v in mot.items()}, prev_cameras=prev_cams, stream=stream,
                                       seeds=seeds)
        ctx.denoise_batch_device(w, h, n, rgb.data_ptr(), {k: aov[k].data_ptr() for k in guides}, out.data_ptr(), stream=stream)

    def loop():
        for j in range(n):
            ctx.update(camera=cams[j])
            ctx.render_aov_device(per_view[j], {k: v[j].data_ptr() for k, v in aov.items()}, stream=stream)
            ctx.render_motion_device(per_view[j], {k: v[j].data_ptr() for k, v in mot.items()}, prev_camera=prev_cams[j], stream=stream)
            ctx.denoise_device(w, h, rgb[j].data_ptr(), {k: aov[k][j].data_ptr() for k in guides}, out[j].data_ptr(), stream=stream)

    fn = batch if args.side == "batch" else loop
    dev, wall = [], []
    for r in range(args.warmup + args.repeats):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if r >= args.warmup:
            dev.append(e0.elapsed_time(e1)), wall.append((t1 - t0) * 1e3)
    digest = hashlib.sha256()
    for d, names in ((aov, AOV), (mot, MOTION)):
        for k in names:
            digest.update(d[k].cpu().numpy().tobytes())
    digest.update(out.cpu().numpy().tobytes())
    ctx.close()
    print(json.dumps(dict(side=args.side, dev=dev, wall=wall, digest=digest.hexdigest())), flush=True)


def drive(args):
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    failed = False
    with open(args.out, "w") as f:
        for wl in args.workloads:
            kind, w, h, spp, n = WORKLOADS[wl]
            res = {"batch": dict(dev=[], wall=[], digest=set()), "loop": dict(dev=[], wall=[], digest=set())}
            for _ in range(args.rounds):
                for name in ("batch", "loop"):
                    env = dict(os.environ)
                    if name == "loop" and args.loop_lib:
                        env["RT_AMD_LIB"] = os.path.abspath(args.loop_lib)
                    cmd = [sys.executable, os.path.abspath(__file__), "--side", name, "--workload", wl, "--warmup", str(args.warmup),
                           "--repeats", str(args.repeats)]
                    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=args.child_timeout)
                    if r.returncode != 0:
                        sys.stderr.write(r.stdout + r.stderr)
                        sys.exit("%s: the %s side ended with status %d" % (wl, name, r.returncode))
                    row = json.loads(r.stdout.strip().splitlines()[-1])
                    res[name]["dev"] += row["dev"]
                    res[name]["wall"] += row["wall"]
                    res[name]["digest"].add(row["digest"])
            same = len(res["batch"]["digest"] | res["loop"]["digest"]) == 1
            row = dict(workload=wl, scene=kind, width=w, height=h, spp=spp, views=n, identical=same, rounds=args.rounds,
                       warmup=args.warmup, repeats=args.repeats, loop_lib="parent" if args.loop_lib else "this")
            for name in ("batch", "loop"):
                d, wa = res[name]["dev"], res[name]["wall"]
                row.update({"%s_dev_ms" % name: float(np.median(d)), "%s_dev_ms_min" % name: float(np.min(d)),
                            "%s_dev_ms_max" % name: float(np.max(d)), "%s_wall_ms" % name: float(np.median(wa)),
                            "%s_wall_ms_min" % name: float(np.min(wa)), "%s_wall_ms_max" % name: float(np.max(wa))})
            row["speedup_dev"] = row["loop_dev_ms"] / row["batch_dev_ms"]
            row["speedup_wall"] = row["loop_wall_ms"] / row["batch_wall_ms"]
            print(json.dumps(row), flush=True)
            f.write(json.dumps(row) + "\n")
            f.flush()
            failed |= not same
    if failed:
        sys.exit("the batched outputs differ from the loop's")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", nargs="+", default=list(WORKLOADS), choices=list(WORKLOADS))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--loop-lib", default=None, help="librt_amd.so of the build the loop is timed on (default: this one)")
    ap.add_argument("--child-timeout", type=float, default=180)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aov_views", "aov_views_bench.jsonl"))
    ap.add_argument("--side", choices=("batch", "loop"), help=argparse.SUPPRESS)
    ap.add_argument("--workload", choices=list(WORKLOADS), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.side:
        sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
        side(args)
    else:
        drive(args)


if __name__ == "__main__":
    main()
