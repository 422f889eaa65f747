"""Per-kernel times of tools/svgf_bench.py from the csv of a run under `rocprofv3 --kernel-trace` (a run of its own):

  rocprofv3 --kernel-trace --output-format csv -d DIR -o svgf -- python tools/svgf_bench.py --out DIR/bench.jsonl
  python tools/svgf_trace_stats.py DIR [--warmup 3] [--repeats 10] [--batch 20] > profiles/svgf/kernel_trace_stats.jsonl

Dispatches are split by image size (the grid) and, for the rt_svgf kernels, by the bench's measurement: the tool issues
its calls in a fixed order (one host call, the warm-up batches of each state, then the states alternating), so the index of
a dispatch gives the state it belongs to; the global a-trous dispatches also by step.  The options must be those the bench
ran with; a kernel whose dispatch count does not fit the schedule is reported as one group.  One JSON row per group:
median, min and max in microseconds."""
import argparse
import csv
import glob
import json
import os
import re

import numpy as np

STATES = ["first_frame", "steady_defaults", "steady_max_history_8"]


def schedule(warmup, repeats, batch):
    s = ["host_first_frame"]
    for st in STATES:
        s += [st] * (warmup * batch)
    for _ in range(repeats):
        for st in STATES:
            s += [st] * batch
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dir")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 2048])
    args = ap.parse_args()
    rows = []
    for f in glob.glob(os.path.join(args.dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(f) as fh:
            rows += list(csv.DictReader(fh))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    by = {}
    for r in rows:
        n = re.sub(r"^void ", "", r["Kernel_Name"]).replace("(anonymous namespace)::", "").split("(")[0]
        n = re.sub(r"^(\w+::)+", "", n)
        if not re.match(r"k_(svgf|dn|tp)_", n):
            continue
        g = int(r["Grid_Size_X"]) * int(r["Grid_Size_Y"]) * int(r["Grid_Size_Z"])
        by.setdefault(n, []).append((g, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
    sched = schedule(args.warmup, args.repeats, args.batch)
    for n in sorted(by):
        grids = sorted({g for g, _ in by[n]})  # (the sigma kernels have one grid whatever the image)
        for gi, g in enumerate(grids):
            t = [us for gg, us in by[n] if gg == g]
            size = sorted(args.sizes)[gi] if len(grids) == len(args.sizes) else None
            groups = {"all": t}
            per = 4 if n == "k_svgf_atrous<false>" else 1  # steps 2, 4, 8, 16 of the default five iterations
            if n.startswith("k_svgf_") and size is not None and len(t) == per * len(sched):
                groups = {}
                for i, us in enumerate(t):
                    key = sched[i // per] + (" step %d" % (2 << (i % per)) if per > 1 else "")
                    groups.setdefault(key, []).append(us)
            for key, v in groups.items():
                print(json.dumps(dict(kernel=n, size=size, measurement=key, dispatches=len(v), us_median=round(float(np.median(v)), 1),
                                      us_min=round(float(np.min(v)), 1), us_max=round(float(np.max(v)), 1))))


if __name__ == "__main__":
    main()
