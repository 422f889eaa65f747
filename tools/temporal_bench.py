"""Device time of the motion pass (rt_render_motion_device) next to the one-sample AOV pass (rt_render_aov_device) at
1024x1024 on `lowres` and on the 1 M-triangle stress scene, and of the temporal accumulation
(rt_temporal_accumulate_device) at 1024x1024 and 2048x2048.  Each figure: events around --batch back-to-back calls on one
stream, divided by the batch (so the launch gap is amortised); median, min and max over --repeats batches after --warmup
untimed ones.  For per-kernel times run the tool under `rocprofv3 --kernel-trace --stats -- python tools/temporal_bench.py`
(a run of its own).  One JSON row per measurement.

  python tools/temporal_bench.py [--warmup 3] [--repeats 10] [--batch 20] [--out profiles/temporal/temporal_bench.jsonl]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ray-tracing-engine_amd"))
import pyrt  # noqa: E402


def timed(fn, warmup, repeats, batch):
    """ms per call of fn: `repeats` batches of `batch` calls between two events, after `warmup` untimed batches."""
    out = []
    for r in range(warmup + repeats):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(batch):
            fn()
        e1.record()
        torch.cuda.synchronize()
        if r >= warmup:
            out.append(e0.elapsed_time(e1) / batch)
    return out


def row(name, ms, **kw):
    d = dict(measurement=name, us_median=float(np.median(ms)) * 1e3, us_min=float(np.min(ms)) * 1e3, us_max=float(np.max(ms)) * 1e3)
    d.update(kw)
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal", "temporal_bench.jsonl"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    stream = torch.cuda.current_stream().cuda_stream
    rows = []
    f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device="cuda")
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device="cuda")
    n = 1024
    for kind in ("lowres", "stress"):
        s = pyrt.Scene(kind, n, n)
        ctx = pyrt.Context(s)
        p = pyrt.make_params(n, n, 1, mode=pyrt.MODE_PATH, seed=1)
        ch = dict(motion=f32(n, n, 2), position=f32(n, n, 3), prev_position=f32(n, n, 3), mesh=i32(n, n))
        prev = torch.from_numpy(s.arrays()["pos"]).cuda()
        mptr = {k: v.data_ptr() for k, v in ch.items()}
        aov = dict(albedo=f32(n, n, 3), normal=f32(n, n, 3), position=f32(n, n, 3), depth=f32(n, n), hits=i32(n, n), mesh=i32(n, n),
                   tri=i32(n, n))
        aptr = {k: v.data_ptr() for k, v in aov.items()}
        motion = lambda: ctx.render_motion_device(p, mptr, d_prev_pos=prev.data_ptr(), stream=stream)
        one_aov = lambda: ctx.render_aov_device(p, aptr, stream)
        # alternate the two passes: warm both, then the timed batches in rounds
        timed(motion, args.warmup, 0, args.batch), timed(one_aov, args.warmup, 0, args.batch)
        tm, ta = [], []
        for _ in range(args.repeats):
            tm += timed(motion, 0, 1, args.batch)
            ta += timed(one_aov, 0, 1, args.batch)
        rows.append(row("motion", tm, scene=kind, width=n, height=n, triangles=int(s.desc.n_triangles)))
        rows.append(row("aov_one_sample", ta, scene=kind, width=n, height=n, triangles=int(s.desc.n_triangles)))
        if kind == "lowres":
            for m in (1024, 2048):
                if m != n:
                    # (the accumulation does not cast rays: any buffers of the size do; a constant motion of (0.4, 0.3)
                    # pixels makes every pixel take four taps)
                    ch = dict(motion=f32(m, m, 2), position=f32(m, m, 3), prev_position=f32(m, m, 3), mesh=i32(m, m))
                    ch["motion"][..., 0], ch["motion"][..., 1] = 0.4, 0.3
                else:
                    motion()
                    torch.cuda.synchronize()
                    ch["motion"][..., 0] += 0.4
                    ch["motion"][..., 1] += 0.3
                hist = dict(rgb=f32(m, m, 3), position=ch["prev_position"].clone(), mesh=ch["mesh"].clone(), length=f32(m, m) + 4)
                rgb, out, length = f32(m, m, 3) + 0.5, f32(m, m, 3), f32(m, m)
                cur = {k: ch[k].data_ptr() for k in ("motion", "prev_position", "mesh")}
                hp = {k: v.data_ptr() for k, v in hist.items()}
                for sigma, label in ((0.1, "accumulate"), (0.0, "accumulate_default_sigma")):
                    acc = lambda: ctx.temporal_accumulate_device(m, m, rgb.data_ptr(), cur, hp, out.data_ptr(), length.data_ptr(),
                                                                 stream=stream, sigma_position=sigma)
                    t = timed(acc, args.warmup, args.repeats, args.batch)
                    torch.cuda.synchronize()
                    rows.append(row(label, t, width=m, height=m, bytes_per_pixel_min=4 * (3 + 2 + 3 + 1 + 3 + 1),
                                    mean_length_out=float(length.mean())))
        ctx.close()
        torch.cuda.empty_cache()
    with open(args.out, "w") as f:
        for r in rows:
            r.update(warmup=args.warmup, repeats=args.repeats, batch=args.batch)
            print(json.dumps(r), flush=True)
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
