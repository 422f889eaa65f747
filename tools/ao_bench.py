"""Device time of rt_render_ao_device on the frames its schedule was chosen on: `lowres` as it is (a
closed room: every wave tile full) and `lowres` without its room (mesh 0: most tiles empty or partly filled), 1024 x 1024,
1 spp x 16 rays and 4 spp x 4 rays, unbounded and limited to 10 % of the scene's diagonal.  Every launch is timed by an
event pair on the stream; the launches of a workload repeat --repeats times after --warmup, and the spread of those
identical launches is reported beside the median.  One JSON row per workload:
  ms / ms_min / ms_max   device time of one launch (median and spread over the repeats)
  rays                   primary rays + occlusion rays cast (from the counts the pass returns)
  mrays_s                rays / ms / 1e3

--trace-db FILE reduces instead of measuring: FILE is the database a `rocprofv3 --kernel-trace --stats` run of this tool
left (its `kernels` view), read without a GPU.  The k_ao dispatches are taken in start order and dealt to the workloads
in the order the loop below launches them, --warmup + --repeats launches each (the same values as the traced run's), and
one row per workload gives kernel_ms / kernel_ms_min / kernel_ms_max over the repeats.  --alternated K: the traced build
launched K kernels in turn for every repeat; one row per workload and kernel, named by the kernel's template arguments.

profiles/ao/schedule_events.jsonl and schedule_kernel_trace.jsonl, the comparison the schedule was chosen by, came from
this loop and this reduction (--alternated 2 --warmup 1 --repeats 3) on a build that held both candidate kernels and
launched them in turn; the library as it stands holds the winner only, so those two files cannot be made again from it.

  python tools/ao_bench.py [--size 1024] [--repeats 7] [--warmup 2] [--out profiles/ao/ao_bench.jsonl]
  rocprofv3 --kernel-trace --stats -d DIR -o ao -- python tools/ao_bench.py --repeats 3 --warmup 1
  python tools/ao_bench.py --trace-db DIR/ao_results.db --repeats 3 --warmup 1 [--out profiles/ao/ao_kernel_trace.jsonl]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ray-tracing-engine_amd"))


def without_mesh0(pyrt, scene):
    a = scene.arrays()
    nv, nt = int(a["vtx_begin"][1]), int(a["tri_begin"][1])
    return pyrt.ArrayScene(a["pos"][nv:], a["nrm"][nv:], a["tri"][nt:] - np.uint32(nv), a["tri_begin"][1:] - np.uint32(nt),
                           a["vtx_begin"][1:] - np.uint32(nv), a["materials"][1:], a["lights"], a["camera"])


def diagonal(scene):
    a = scene.arrays()
    p = a["pos"][a["tri"].reshape(-1)]
    return float(np.linalg.norm(p.max(axis=0) - p.min(axis=0)))


WORKLOADS = [(name, spp, n_rays, share) for name in ("lowres", "lowres_open") for spp, n_rays in ((1, 16), (4, 4)) for share in (0.0, 0.1)]


def write_rows(rows, out):
    for r in rows:
        print(json.dumps(r), flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as fh:
            for r in rows:
                fh.write(json.dumps(r) + "\n")


def reduce_trace(db, warmup, repeats, alternated, out):
    """Rows of kernel time per workload (and kernel, when several alternated) from a rocprofv3 kernel-trace database."""
    import sqlite3
    con = sqlite3.connect(db)
    disp = list(con.execute("select name, start, end from kernels where name like '%k_ao<%' order by start"))
    per = (warmup + repeats) * alternated
    if len(disp) != per * len(WORKLOADS):
        raise SystemExit("%d k_ao dispatches in %s, expected %d workloads x (%d + %d) launches x %d kernels"
                         % (len(disp), db, len(WORKLOADS), warmup, repeats, alternated))
    rows = []
    for w, (name, spp, n_rays, share) in enumerate(WORKLOADS):
        chunk = disp[w * per:(w + 1) * per]
        for k in range(alternated):
            mine = chunk[k::alternated]
            if len({m[0] for m in mine}) != 1:
                raise SystemExit("workload %d: slot %d of the alternation holds several kernels" % (w, k))
            t = sorted((e - s) / 1e6 for _, s, e in mine[warmup:])
            row = dict(scene=name, spp=spp, n_rays=n_rays, max_distance_share=share, kernel_ms=round(t[len(t) // 2], 4),
                       kernel_ms_min=round(t[0], 4), kernel_ms_max=round(t[-1], 4))
            if alternated > 1:
                row["kernel"] = mine[0][0][mine[0][0].index("k_ao<"):].split("(")[0]
            rows.append(row)
    write_rows(rows, out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    ap.add_argument("--trace-db", default="")
    ap.add_argument("--alternated", type=int, default=1)
    args = ap.parse_args()
    if args.trace_db:
        return reduce_trace(args.trace_db, args.warmup, args.repeats, args.alternated, args.out)
    import torch
    import pyrt
    n = args.size
    closed = pyrt.Scene("lowres", n, n)
    scenes = (("lowres", closed), ("lowres_open", without_mesh0(pyrt, closed)))
    stream = torch.cuda.current_stream()
    un = torch.zeros((n, n), dtype=torch.int32, device="cuda")
    hits = torch.zeros((n, n), dtype=torch.int32, device="cuda")
    bent = torch.zeros((n, n, 3), dtype=torch.float32, device="cuda")
    ptrs = dict(unoccluded=un.data_ptr(), hits=hits.data_ptr(), bent=bent.data_ptr())
    rows = []
    for name, scene in scenes:
        ctx = pyrt.Context(scene)
        for spp, n_rays, share in [w[1:] for w in WORKLOADS if w[0] == name]:
            p = pyrt.make_params(n, n, spp, seed=1)
            dist = share * diagonal(scene)
            t = []
            for it in range(args.warmup + args.repeats):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                ctx.render_ao_device(p, n_rays, ptrs, max_distance=dist, stream=stream.cuda_stream)
                e1.record(stream)
                e1.synchronize()
                if it >= args.warmup:
                    t.append(e0.elapsed_time(e1))
            h = int(hits.sum().item())
            rays = n * n * spp + h * n_rays
            t.sort()
            ms = t[len(t) // 2]
            row = dict(scene=name, size=n, spp=spp, n_rays=n_rays, max_distance_share=share, ms=round(ms, 4), ms_min=round(t[0], 4),
                       ms_max=round(t[-1], 4), rays=rays, mrays_s=round(rays / ms / 1e3, 1), unoccluded=int(un.sum().item()),
                       hit_samples=h)
            rows.append(row)
        ctx.close()
    write_rows(rows, args.out)


if __name__ == "__main__":
    main()
