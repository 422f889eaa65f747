"""Device time of rt_render_views_shutter_albedo_device on one MI355X.

Workload C2: `lowres`, 1024 x 1024, 128 spp, path mode, depth 3, its own three lights (the pooled body).
  textured_t1        rt_render_textured_device with a 4 x 4 texture of its albedo on every mesh, bilinear (§6u's T1)
  albedo_still_t1    the new form with one still pinhole view at the context's camera and the same set: textured_t1's
                     frame bit for bit (X2), which the run checks; the difference is the price of the view and shutter
                     tables under the shutter generator
  views_shutter      rt_render_views_shutter_device with that view: the same rays without the surface (X3's other
                     side); the difference to albedo_still_t1 is the price of the surface under the shutter generator
  move_plain         one view with a lens and a moving camera, untextured
  move_bilinear      the same view with one 1024 x 1024 texture of random texels on every mesh, bilinear and repeating
  four_views         four views of 512 x 512 (a still one, a lens, two moving cameras with a lens) in one launch, with the
                     1024 x 1024 texture
  four_launches      the same four views as four single-view launches (the sum of their kernel times); the slices are
                     four_views' bit for bit (X1), which the run checks
The forms take turns launch by launch for --repeats rounds after --warmup rounds; every figure is the library's own event
pair round the kernel (rt_stats.kernel_ms).

  python tools/albedo_views_bench.py [--repeats 3] [--warmup 1] [--out profiles/albedo_views/albedo_views_bench.jsonl]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C2 = ("lowres", 1024, 128)
BIG = 1024
APERTURE, FOCUS, MOVE = 0.3, 1.5, (0.2, 0.1, 0.0)


def summary(v):
    v = sorted(v)
    med = v[len(v) // 2]
    return dict(median=round(med, 3), min=round(v[0], 3), max=round(v[-1], 3), spread_pct=round(100 * (v[-1] - v[0]) / med, 2))


class Sum:
    """The stats of several launches as one: kernel times and ray counts added."""

    def __init__(self, stats):
        self.kernel_ms = sum(s.kernel_ms for s in stats)
        self.rays_closest = sum(s.rays_closest for s in stats)
        self.rays_shadow = sum(s.rays_shadow for s in stats)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "albedo_views", "albedo_views_bench.jsonl"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "ray-tracing-engine_amd"))
    import numpy as np
    import torch
    import pyrt
    stream = torch.cuda.current_stream().cuda_stream
    rows = []

    def emit(**row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    def translated(cam, move):
        b = np.asarray(cam, np.float32).reshape(4, 3).copy()
        b[0], b[1] = b[0] + np.asarray(move, np.float32), b[1] + np.asarray(move, np.float32)
        return b

    def texture_sets(scene):
        a = scene.arrays()
        nm = len(a["vtx_begin"]) - 1
        ext = a["pos"].max(axis=0) - a["pos"].min(axis=0)
        q = (a["pos"] - a["pos"].min(axis=0)) / ext
        uv = np.ascontiguousarray(np.stack([q[:, 0] + 0.5 * q[:, 2], q[:, 1] + 0.5 * q[:, 2]], axis=1) * 2.0 - 0.5, np.float32)
        albedo = [np.broadcast_to(a["materials"][m, 2:5].astype(np.float32), (4, 4, 3)).copy() for m in range(nm)]
        big = np.random.default_rng(1).uniform(0.05, 1.0, (BIG, BIG, 3)).astype(np.float32)
        return (albedo, np.arange(nm, dtype=np.uint32), uv), ([(big, pyrt.TEX_REPEAT, pyrt.TEX_REPEAT, pyrt.TEX_BILINEAR)], np.zeros(nm, np.uint32), uv)

    def take_turns(shapes):
        ms, last = {k: [] for k in shapes}, {}
        for it in range(args.warmup + args.repeats):
            for k, fn in shapes.items():
                last[k] = fn()
                if it >= args.warmup:
                    ms[k].append(last[k].kernel_ms)
        torch.cuda.synchronize()
        return ms, last

    def report(part, ms, last, base, size, n, **extra):
        b = summary(ms[base])
        for k, v in ms.items():
            s, st = summary(v), last[k]
            rays = st.rays_closest + st.rays_shadow
            emit(part=part, shape=k, scene=C2[0], width=size, height=size, views=n, spp=C2[2], repeats=len(v), kernel_ms=s["median"],
                 ms_min=s["min"], ms_max=s["max"], spread_pct=s["spread_pct"], rays=rays, grays_s=round(rays / s["median"] / 1e6, 3),
                 baseline=base, ratio_to_baseline=round(s["median"] / b["median"], 4),
                 interval_overlaps_baseline=bool(s["min"] <= b["max"] and b["min"] <= s["max"]), **extra)

    name, size, spp = C2
    # ---- one view of 1024 x 1024 ------------------------------------------------------------------------------------------
    scene = pyrt.Scene(name, size, size)
    cam = np.asarray(scene.arrays()["camera"], np.float32).reshape(4, 3) + np.float32(0.0)
    t1_set, big_set = texture_sets(scene)
    t1, bil = pyrt.Context(scene), pyrt.Context(scene)
    t1.set_textures(*t1_set)
    bil.set_textures(*big_set)
    p = pyrt.make_params(size, size, spp, mode=pyrt.MODE_PATH, max_depth=3, seed=1)
    still = [pyrt.make_shutter(cam, 0.0, 0.0)]
    move = [pyrt.make_shutter(translated(cam, MOVE), 0.0, 1.0, APERTURE, FOCUS)]
    accs = {k: torch.zeros((1, size, size, 4), dtype=torch.float32, device="cuda")
            for k in ("textured_t1", "albedo_still_t1", "views_shutter", "move_plain", "move_bilinear")}

    def zeroed(k, fn):
        def run():
            accs[k].zero_()
            return fn(accs[k].data_ptr())
        return run

    shapes = {
        "textured_t1": zeroed("textured_t1", lambda d: t1.render_textured_device(p, d, stream=stream, stats=True)),
        "albedo_still_t1": zeroed("albedo_still_t1", lambda d: t1.render_views_shutter_albedo_device(
            p, cam[None], still, d, albedo=pyrt.ALBEDO_TEXTURES, stream=stream, stats=True)),
        "views_shutter": zeroed("views_shutter", lambda d: t1.render_views_shutter_device(p, cam[None], still, d, stream=stream, stats=True)),
        "move_plain": zeroed("move_plain", lambda d: bil.render_views_shutter_device(p, cam[None], move, d, stream=stream, stats=True)),
        "move_bilinear": zeroed("move_bilinear", lambda d: bil.render_views_shutter_albedo_device(
            p, cam[None], move, d, albedo=pyrt.ALBEDO_TEXTURES, stream=stream, stats=True)),
    }
    ms, last = take_turns(shapes)
    bits = lambda k: accs[k].view(torch.int32)
    same = bool(torch.equal(bits("textured_t1"), bits("albedo_still_t1"))) and bool(torch.equal(bits("views_shutter"), bits("albedo_still_t1")))
    if not same:  # (the rows below would compare the times of different frames)
        sys.exit("the still T1 frame of the new form is not rt_render_textured's and rt_render_views_shutter's bit for bit")
    report("one_view", ms, last, "textured_t1", size, 1, still_frames_identical=same)
    t1.close()
    bil.close()
    # ---- four views of 512 x 512 ------------------------------------------------------------------------------------------
    half = size // 2
    scene = pyrt.Scene(name, half, half)
    cam = np.asarray(scene.arrays()["camera"], np.float32).reshape(4, 3) + np.float32(0.0)
    cams = np.stack([translated(cam, (0.1 * j, 0.0, 0.0)) for j in range(4)])
    recs = [pyrt.make_shutter(cams[0], 0.0, 0.0), pyrt.make_shutter(cams[1], 0.0, 0.0, APERTURE, FOCUS),
            pyrt.make_shutter(translated(cams[2], MOVE), 0.0, 1.0, APERTURE, FOCUS),
            pyrt.make_shutter(translated(cams[3], MOVE), 0.25, 0.5, APERTURE, FOCUS)]
    seeds = [1, 2, 3, 4]
    ctx = pyrt.Context(scene)
    ctx.set_textures(*texture_sets(scene)[1])
    p = pyrt.make_params(half, half, spp, mode=pyrt.MODE_PATH, max_depth=3, seed=1)
    accs = {k: torch.zeros((4, half, half, 4), dtype=torch.float32, device="cuda") for k in ("four_views", "four_launches")}
    slice_bytes = half * half * 16

    def four_launches(d):
        return Sum([ctx.render_views_shutter_albedo_device(p, cams[j:j + 1], recs[j:j + 1], d + j * slice_bytes, albedo=pyrt.ALBEDO_TEXTURES,
                                                           stream=stream, seeds=seeds[j:j + 1], stats=True) for j in range(4)])

    shapes = {"four_launches": zeroed("four_launches", four_launches),
              "four_views": zeroed("four_views", lambda d: ctx.render_views_shutter_albedo_device(
                  p, cams, recs, d, albedo=pyrt.ALBEDO_TEXTURES, stream=stream, seeds=seeds, stats=True))}
    ms, last = take_turns(shapes)
    same = bool(torch.equal(bits("four_views"), bits("four_launches")))
    if not same:
        sys.exit("the slices of the four-view launch are not the four single-view launches' bit for bit")
    report("four_views", ms, last, "four_launches", half, 4, slices_identical=same)
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        for r in rows:
            fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
