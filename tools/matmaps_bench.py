"""Device time of rt_render_material_device on one MI355X.

Workload C2: `lowres`, 1024 x 1024, 128 spp, path mode, depth 3, its own three lights (the pooled body).
  tex_t1          rt_render_textured_device with §6u's T1 set, a 4 x 4 texture of its albedo on every mesh, bilinear: the
                  baseline — the same rays, and the parent commit's instances digest for digest
                  (profiles/matmaps/digest_compare.txt)
  mat_m1          rt_render_material_device with that set and, per mesh, a 4 x 4 texture of its own f0 and one of its
                  own (kd, alpha, 9) (M1): tex_t1's frame bit for bit, which the run checks; the difference is the price
                  of two more samples, of bsdf_base on an rt_material instead of the hoisted record, and of eight parked
                  rows of LDS instead of three
  mat_big         rt_render_material_device with one 1024 x 1024 texture of random texels, bilinear and repeating, in
                  all three roles on every mesh: texel loads that miss more often (other frames, the same rays)
The forms take turns launch by launch for --repeats rounds after --warmup rounds; every figure is the library's own event
pair round the kernel (rt_stats.kernel_ms).  `no_pool` repeats tex_t1 and mat_m1 on the sequential body.

  python tools/matmaps_bench.py [--repeats 3] [--warmup 1] [--out profiles/matmaps/matmaps_bench.jsonl]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "matmaps", "matmaps_bench.jsonl"))
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
    ext = a["pos"].max(axis=0) - a["pos"].min(axis=0)
    q = (a["pos"] - a["pos"].min(axis=0)) / ext
    uv = np.ascontiguousarray(np.stack([q[:, 0] + 0.5 * q[:, 2], q[:, 1] + 0.5 * q[:, 2]], axis=1) * 2.0 - 0.5, np.float32)
    mats = a["materials"].astype(np.float32)
    flat = lambda rgb: np.broadcast_to(np.asarray(rgb, np.float32), (4, 4, 3)).copy()
    albedo = [flat(mats[m, 2:5]) for m in range(nm)]
    own_f0 = [flat(mats[m, 5:8]) for m in range(nm)]
    own_kda = [flat([mats[m, 0], mats[m, 1], 9.0]) for m in range(nm)]
    g = np.random.default_rng(1)
    # every channel is a plausible value in each of its roles: albedo and f0 in [0.05, 1), kd (r) and alpha (g) likewise
    big = g.uniform(0.05, 1.0, (BIG, BIG, 3)).astype(np.float32)
    ids = np.arange(nm, dtype=np.uint32)
    t1, m1, mbig = (pyrt.Context(scene) for _ in range(3))
    t1.set_textures(albedo, ids, uv)
    m1.set_textures(albedo + own_f0 + own_kda, ids, uv)
    m1.set_material_maps(nm + ids, 2 * nm + ids)
    mbig.set_textures([(big, pyrt.TEX_REPEAT, pyrt.TEX_REPEAT, pyrt.TEX_BILINEAR)], np.zeros(nm, np.uint32), uv)
    mbig.set_material_maps(np.zeros(nm, np.uint32), np.zeros(nm, np.uint32))
    for part, kw in (("pooled", dict()), ("no_pool", dict(no_pool=True))):
        p = pyrt.make_params(size, size, spp, mode=pyrt.MODE_PATH, max_depth=3, seed=1, **kw)
        accs = {k: torch.zeros((size, size, 4), dtype=torch.float32, device="cuda") for k in ("tex_t1", "mat_m1", "mat_big")}

        def zeroed(k, fn):
            def run():
                accs[k].zero_()
                return fn(accs[k].data_ptr())
            return run

        shapes = {"tex_t1": zeroed("tex_t1", lambda d: t1.render_textured_device(p, d, stream=stream.cuda_stream, stats=True)),
                  "mat_m1": zeroed("mat_m1", lambda d: m1.render_material_device(p, d, stream=stream.cuda_stream, stats=True))}
        if part == "pooled":
            shapes["mat_big"] = zeroed("mat_big", lambda d: mbig.render_material_device(p, d, stream=stream.cuda_stream, stats=True))
        ms, last = take_turns(shapes, args)
        torch.cuda.synchronize()
        same = bool(torch.equal(accs["tex_t1"].view(torch.int32), accs["mat_m1"].view(torch.int32)))
        if not same:  # (the rows below would compare the times of two different frames)
            sys.exit("%s: the M1 frame is not rt_render_textured's T1 frame bit for bit" % part)
        base = summary(ms["tex_t1"])
        for k, v in ms.items():
            s, st = summary(v), last[k]
            rays = st.rays_closest + st.rays_shadow
            emit(part=part, shape=k, scene=name, width=size, height=size, spp=spp, repeats=len(v), kernel_ms=s["median"], ms_min=s["min"],
                 ms_max=s["max"], spread_pct=s["spread_pct"], rays=rays, grays_s=round(rays / s["median"] / 1e6, 3),
                 ratio_to_tex_t1=round(s["median"] / base["median"], 4),
                 interval_overlaps_tex_t1=bool(s["min"] <= base["max"] and base["min"] <= s["max"]), m1_frame_is_t1_frame=same)
    for c in (t1, m1, mbig):
        c.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        for r in rows:
            fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
