"""Device time of rt_render_normal_mapped_device on one MI355X.

Workload C2: `lowres`, 1024 x 1024, 128 spp, path mode, depth 3, its own three lights (the pooled body).
  mat_m1          rt_render_material_device with §6w's M1 set — per mesh a 4 x 4 texture of its albedo, one of its own f0
                  and one of its own (kd, alpha, 9), bilinear: the baseline — the same rays, and the parent commit's
                  instances digest for digest (profiles/normalmaps/digest_compare.txt)
  nmap_n1         rt_render_normal_mapped_device with that set, those maps and, on every mesh, a 4 x 4 normal map whose
                  texels are (0.5, 0.5, 1) (N1): mat_m1's frame bit for bit, which the run checks; the difference is the
                  OVERHEAD of the feature — the tangent frame of every vertex, one more sample, the larger set-up
  nmap_big        rt_render_normal_mapped_device with the M1 material maps and one 1024 x 1024 normal map of random
                  texels (r, g in [0, 1), b in [0.5, 1)), bilinear and repeating, on every mesh.  This one CHANGES THE
                  RAYS — every bounce leaves along another direction — so its row is the cost of the feature in use on
                  other paths, not an overhead figure: compare its rays per second, not its milliseconds
The forms take turns launch by launch for --repeats rounds after --warmup rounds; every figure is the library's own event
pair round the kernel (rt_stats.kernel_ms).  `no_pool` repeats mat_m1 and nmap_n1 on the sequential body.

  python tools/nmap_bench.py [--repeats 3] [--warmup 1] [--out profiles/normalmaps/nmap_bench.jsonl]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "normalmaps", "nmap_bench.jsonl"))
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
    big = np.stack([g.uniform(0.0, 1.0, (BIG, BIG)), g.uniform(0.0, 1.0, (BIG, BIG)), g.uniform(0.5, 1.0, (BIG, BIG))], axis=-1).astype(np.float32)
    ids = np.arange(nm, dtype=np.uint32)
    m1, n1, nbig = (pyrt.Context(scene) for _ in range(3))
    m1.set_textures(albedo + own_f0 + own_kda, ids, uv)
    m1.set_material_maps(nm + ids, 2 * nm + ids)
    n1.set_textures(albedo + own_f0 + own_kda + [flat([0.5, 0.5, 1.0])], ids, uv)
    n1.set_material_maps(nm + ids, 2 * nm + ids)
    n1.set_normal_maps(np.full(nm, 3 * nm, np.uint32))
    nbig.set_textures(albedo + own_f0 + own_kda + [(big, pyrt.TEX_REPEAT, pyrt.TEX_REPEAT, pyrt.TEX_BILINEAR)], ids, uv)
    nbig.set_material_maps(nm + ids, 2 * nm + ids)
    nbig.set_normal_maps(np.full(nm, 3 * nm, np.uint32))
    for part, kw in (("pooled", dict()), ("no_pool", dict(no_pool=True))):
        p = pyrt.make_params(size, size, spp, mode=pyrt.MODE_PATH, max_depth=3, seed=1, **kw)
        accs = {k: torch.zeros((size, size, 4), dtype=torch.float32, device="cuda") for k in ("mat_m1", "nmap_n1", "nmap_big")}

        def zeroed(k, fn):
            def run():
                accs[k].zero_()
                return fn(accs[k].data_ptr())
            return run

        shapes = {"mat_m1": zeroed("mat_m1", lambda d: m1.render_material_device(p, d, stream=stream.cuda_stream, stats=True)),
                  "nmap_n1": zeroed("nmap_n1", lambda d: n1.render_normal_mapped_device(p, d, stream=stream.cuda_stream, stats=True))}
        if part == "pooled":
            shapes["nmap_big"] = zeroed("nmap_big", lambda d: nbig.render_normal_mapped_device(p, d, stream=stream.cuda_stream, stats=True))
        ms, last = take_turns(shapes, args)
        torch.cuda.synchronize()
        same = bool(torch.equal(accs["mat_m1"].view(torch.int32), accs["nmap_n1"].view(torch.int32)))
        if not same:  # (the rows below would compare the times of two different frames)
            sys.exit("%s: the N1 frame is not rt_render_material's M1 frame bit for bit" % part)
        base = summary(ms["mat_m1"])
        for k, v in ms.items():
            s, st = summary(v), last[k]
            rays = st.rays_closest + st.rays_shadow
            emit(part=part, shape=k, scene=name, width=size, height=size, spp=spp, repeats=len(v), kernel_ms=s["median"], ms_min=s["min"],
                 ms_max=s["max"], spread_pct=s["spread_pct"], rays=rays, grays_s=round(rays / s["median"] / 1e6, 3),
                 ratio_to_mat_m1=round(s["median"] / base["median"], 4),
                 interval_overlaps_mat_m1=bool(s["min"] <= base["max"] and base["min"] <= s["max"]), n1_frame_is_m1_frame=same,
                 same_rays_as_mat_m1=k != "nmap_big")
    for c in (m1, n1, nbig):
        c.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        for r in rows:
            fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
