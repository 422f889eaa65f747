"""Device time of rt_render_textured_device on one MI355X.

Workload C2: `lowres`, 1024 x 1024, 128 spp, path mode, depth 3, its own three lights (the pooled body).
  colors_c1       rt_render_colors_device with every vertex carrying its mesh's albedo: the baseline — the same rays, the
                  same parked rows of LDS, and the parent commit's instances digest for digest
                  (profiles/tex/digest_compare.txt)
  tex_t1          rt_render_textured_device with a 4 x 4 texture of its albedo on every mesh, bilinear (T1): colors_c1's
                  frame bit for bit, which the run checks; the difference is the price of the descriptor and the texel
                  loads behind the uv gathers, and of the sampler's arithmetic
  tex_bilinear    the same with one 1024 x 1024 texture of random texels on every mesh, bilinear and repeating: texel
                  loads that miss more often (other frames, the same rays)
  tex_nearest     that texture under the nearest filter: one texel load per vertex instead of four
The forms take turns launch by launch for --repeats rounds after --warmup rounds; every figure is the library's own event
pair round the kernel (rt_stats.kernel_ms).  `no_pool` repeats colors_c1 and tex_t1 on the sequential body.

  python tools/tex_bench.py [--repeats 3] [--warmup 1] [--out profiles/tex/tex_bench.jsonl]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C2 = ("lowres", 1024, 128)
BIG = 1024


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tex", "tex_bench.jsonl"))
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
    nm = len(a["vtx_begin"]) - 1
    mesh_of_vertex = np.repeat(np.arange(nm), np.diff(a["vtx_begin"].astype(np.int64)))
    c1 = np.ascontiguousarray(a["materials"][mesh_of_vertex, 2:5], np.float32)
    ext = a["pos"].max(axis=0) - a["pos"].min(axis=0)
    q = (a["pos"] - a["pos"].min(axis=0)) / ext
    uv = np.ascontiguousarray(np.stack([q[:, 0] + 0.5 * q[:, 2], q[:, 1] + 0.5 * q[:, 2]], axis=1) * 2.0 - 0.5, np.float32)
    albedo = [np.broadcast_to(a["materials"][m, 2:5].astype(np.float32), (4, 4, 3)).copy() for m in range(nm)]
    big = np.random.default_rng(1).uniform(0.05, 1.0, (BIG, BIG, 3)).astype(np.float32)
    colored, t1, bil, near = (pyrt.Context(scene) for _ in range(4))
    colored.set_vertex_colors(c1)
    t1.set_textures(albedo, np.arange(nm, dtype=np.uint32), uv)
    bil.set_textures([(big, pyrt.TEX_REPEAT, pyrt.TEX_REPEAT, pyrt.TEX_BILINEAR)], np.zeros(nm, np.uint32), uv)
    near.set_textures([(big, pyrt.TEX_REPEAT, pyrt.TEX_REPEAT, pyrt.TEX_NEAREST)], np.zeros(nm, np.uint32), uv)
    for part, kw in (("pooled", dict()), ("no_pool", dict(no_pool=True))):
        p = pyrt.make_params(size, size, spp, mode=pyrt.MODE_PATH, max_depth=3, seed=1, **kw)
        accs = {k: torch.zeros((size, size, 4), dtype=torch.float32, device="cuda") for k in ("colors_c1", "tex_t1", "tex_bilinear", "tex_nearest")}

        def zeroed(k, fn):
            def run():
                accs[k].zero_()
                return fn(accs[k].data_ptr())
            return run

        shapes = {"colors_c1": zeroed("colors_c1", lambda d: colored.render_colors_device(p, d, stream=stream.cuda_stream, stats=True)),
                  "tex_t1": zeroed("tex_t1", lambda d: t1.render_textured_device(p, d, stream=stream.cuda_stream, stats=True))}
        if part == "pooled":
            shapes["tex_bilinear"] = zeroed("tex_bilinear", lambda d: bil.render_textured_device(p, d, stream=stream.cuda_stream, stats=True))
            shapes["tex_nearest"] = zeroed("tex_nearest", lambda d: near.render_textured_device(p, d, stream=stream.cuda_stream, stats=True))
        ms, last = take_turns(shapes, args)
        torch.cuda.synchronize()
        same = bool(torch.equal(accs["colors_c1"].view(torch.int32), accs["tex_t1"].view(torch.int32)))
        if not same:  # (the rows below would compare the times of two different frames)
            sys.exit("%s: the T1 frame is not rt_render_colors' C1 frame bit for bit" % part)
        base = summary(ms["colors_c1"])
        for k, v in ms.items():
            s, st = summary(v), last[k]
            rays = st.rays_closest + st.rays_shadow
            emit(part=part, shape=k, scene=name, width=size, height=size, spp=spp, repeats=len(v), kernel_ms=s["median"], ms_min=s["min"],
                 ms_max=s["max"], spread_pct=s["spread_pct"], rays=rays, grays_s=round(rays / s["median"] / 1e6, 3),
                 ratio_to_colors_c1=round(s["median"] / base["median"], 4),
                 interval_overlaps_colors_c1=bool(s["min"] <= base["max"] and base["min"] <= s["max"]), t1_frame_is_c1_frame=same)
    for c in (colored, t1, bil, near):
        c.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        for r in rows:
            fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
