"""Device time of rt_render_colors_device on one MI355X.

Workload C2: `lowres`, 1024 x 1024, 128 spp, path mode, depth 3, its own three lights (the pooled body).
  lens_a0         rt_render_lens_device at aperture 0: the same kernel family, instance set and rays without colours
                  (those instances are the parent commit's, digest for digest: profiles/vcol/digest_compare.txt)
  colors_c1       rt_render_colors_device with every vertex carrying its mesh's albedo (C1): lens_a0's frame bit for bit,
                  which the run checks; the difference is the price of three gathers, the interpolation and three
                  divisions per vertex, and of the three parked rows of LDS
  colors_smooth   the same with a colour that varies inside every triangle (other frames, the same rays)
  render          rt_render_device: the persistent kernel, recorded beside them
The shapes take turns launch by launch for --repeats rounds after --warmup rounds; every figure is the library's own event
pair round the kernel (rt_stats.kernel_ms).  `no_pool` repeats lens_a0 and colors_c1 on the sequential body.

  python tools/vcol_bench.py [--repeats 3] [--warmup 1] [--out profiles/vcol/vcol_bench.jsonl]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C2 = ("lowres", 1024, 128)


def summary(v):
    v = sorted(v)
    med = v[len(v) // 2]
    return dict(median=round(med, 3), min=round(v[0], 3), max=round(v[-1], 3), spread_pct=round(100 * (v[-1] - v[0]) / med, 2))


def setup():
    sys.path.insert(0, os.path.join(ROOT, "ray-tracing-engine_amd"))
    import numpy as np
    import torch
    import pyrt
    return np, torch, pyrt


def take_turns(shapes, args):
    ms, last = {k: [] for k in shapes}, {}
    for it in range(args.warmup + args.repeats):
        for k, fn in shapes.items():
            last[k] = fn()
            if it >= args.warmup:
                ms[k].append(last[k].kernel_ms)
    return ms, last


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vcol", "vcol_bench.jsonl"))
    args = ap.parse_args()
    np, torch, pyrt = setup()
    stream = torch.cuda.current_stream()
    rows = []

    def emit(**row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    name, size, spp = C2
    scene = pyrt.Scene(name, size, size)
    a = scene.arrays()
    mesh_of_vertex = np.repeat(np.arange(len(a["vtx_begin"]) - 1), np.diff(a["vtx_begin"].astype(np.int64)))
    c1 = np.ascontiguousarray(a["materials"][mesh_of_vertex, 2:5], np.float32)
    ext = a["pos"].max(axis=0) - a["pos"].min(axis=0)
    smooth = np.ascontiguousarray(0.1 + 0.8 * (a["pos"] - a["pos"].min(axis=0)) / ext, np.float32)
    lens = pyrt.make_lens(0.0, 1.0)
    plain, colored = pyrt.Context(scene), pyrt.Context(scene)
    colored.set_vertex_colors(c1)
    smoothed = pyrt.Context(scene)
    smoothed.set_vertex_colors(smooth)
    for part, kw in (("pooled", dict()), ("no_pool", dict(no_pool=True))):
        p = pyrt.make_params(size, size, spp, mode=pyrt.MODE_PATH, max_depth=3, seed=1, **kw)
        accs = {k: torch.zeros((size, size, 4), dtype=torch.float32, device="cuda") for k in ("lens_a0", "colors_c1", "colors_smooth", "render")}

        def zeroed(k, fn):
            def run():
                accs[k].zero_()
                return fn(accs[k].data_ptr())
            return run

        shapes = {"lens_a0": zeroed("lens_a0", lambda d: plain.render_lens_device(p, lens, d, stream=stream.cuda_stream, stats=True)),
                  "colors_c1": zeroed("colors_c1", lambda d: colored.render_colors_device(p, d, stream=stream.cuda_stream, stats=True))}
        if part == "pooled":
            shapes["colors_smooth"] = zeroed("colors_smooth", lambda d: smoothed.render_colors_device(p, d, stream=stream.cuda_stream, stats=True))
            shapes["render"] = zeroed("render", lambda d: plain.render_device(p, d, stream=stream.cuda_stream, stats=True))
        ms, last = take_turns(shapes, args)
        torch.cuda.synchronize()
        same = bool(torch.equal(accs["lens_a0"].view(torch.int32), accs["colors_c1"].view(torch.int32)))
        if not same:  # (the rows below would compare the times of two different frames)
            sys.exit("%s: the C1 frame is not rt_render_lens' frame at aperture 0 bit for bit" % part)
        base = summary(ms["lens_a0"])
        for k, v in ms.items():
            s, st = summary(v), last[k]
            rays = st.rays_closest + st.rays_shadow
            emit(part=part, shape=k, scene=name, width=size, height=size, spp=spp, repeats=len(v), kernel_ms=s["median"], ms_min=s["min"],
                 ms_max=s["max"], spread_pct=s["spread_pct"], rays=rays, grays_s=round(rays / s["median"] / 1e6, 3),
                 ratio_to_lens_a0=round(s["median"] / base["median"], 4), c1_frame_is_lens_a0_frame=same)
    for c in (plain, colored, smoothed):
        c.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        for r in rows:
            fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
