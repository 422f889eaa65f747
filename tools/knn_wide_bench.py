#!/usr/bin/env python3
"""Photon-map frames at large k: config-3-shaped frames (cubes, 1024^2, 16 spp, ray mode, 50,000 photons
requested, map built on the device) at k in {10, 16, 17, 32, 64, 128, 256}, for each wide k-heap layout
(RT_KNN_WIDE_LAYOUT: 16 the split planes, 8 the interleaved entries, auto the launcher's rule).

Per (layout, k) it prints one JSON line: ms per frame (device events around rt_render_device, median of
--steps after --warmup), k-NN queries per second, kd nodes visited per query (a separate collect_stats frame),
the instance that ran and its waves per CU (the runtime's occupancy for its LDS, RT_KNN_VERBOSE); then the
CPU oracle's k-NN queries per second on the same map and a smaller frame (--oracle-size, --oracle-threads).
k <= 16 runs k_render, whatever the layout.  Each layout runs in a child process: the library reads
RT_KNN_WIDE_LAYOUT once.
usage: python tools/knn_wide_bench.py [--layouts 16,8,auto] [--ks 10,16,...] [--steps 5] [--warmup 2]
                                      [--oracle-size 128] [--oracle-threads 16] [--out file.jsonl]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = H = 1024
SPP, NPH = 16, 50000


def child(args):
    sys.path.insert(0, os.path.join(ROOT, "ray-tracing-engine_amd"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch
    import pyrt

    dev = torch.device("cuda:0")
    scene = pyrt.Scene("cubes", W, H)
    ctx = pyrt.Context(scene, device=0)
    nstored, _ = ctx.build_photon_map(NPH, seed=1)
    accum = torch.zeros((H, W, 4), dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    for k in args.ks:
        p = pyrt.make_params(W, H, SPP, mode=pyrt.MODE_RAY, seed=1, use_photons=1, k=k, photons_requested=NPH)
        p.collect_stats = 1
        accum.zero_()
        st = ctx.render_device(p, accum.data_ptr(), stream, stats=True)
        torch.cuda.synchronize()
        p.collect_stats = 0
        times = []
        for i in range(args.warmup + args.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            accum.zero_()
            e0.record()
            ctx.render_device(p, accum.data_ptr(), stream)
            e1.record()
            torch.cuda.synchronize()
            if i >= args.warmup:
                times.append(e0.elapsed_time(e1))
        ms = float(np.median(times))
        print(json.dumps({"layout": args.layout, "k": k, "photons": nstored, "ms_per_frame": round(ms, 3),
                          "ms_min": round(min(times), 3), "ms_max": round(max(times), 3),
                          "knn_queries": st.knn_queries, "queries_per_s": st.knn_queries / ms * 1e3,
                          "kd_visited_per_query": st.kd_visited / max(st.knn_queries, 1)}), flush=True)
    ctx.close()


def oracle(args):
    """The CPU oracle on the device-built map: k-NN queries per second of a smaller frame."""
    sys.path.insert(0, os.path.join(ROOT, "ray-tracing-engine_amd"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import orc
    import pyrt

    ctx = pyrt.Context(pyrt.Scene("cubes", 16, 16), device=0)
    n, _ = ctx.build_photon_map(NPH, seed=1)
    pos, dir_, w = ctx.get_photons(n)
    ctx.close()
    ph7 = np.concatenate([pos, dir_, w[:, None]], 1)
    s = args.oracle_size
    scene = pyrt.Scene("cubes", s, s)
    for k in args.ks:
        p = pyrt.make_params(s, s, SPP, mode=pyrt.MODE_RAY, seed=1, use_photons=1, k=k, photons_requested=NPH)
        t0 = time.perf_counter()
        _, _, st = orc.render(scene, p, math_mode=orc.MATH_DET, threads=args.oracle_threads, ext_photons=ph7,
                              accel=orc.ACCEL_OBVH)
        sec = time.perf_counter() - t0
        print(json.dumps({"oracle": True, "k": k, "size": "%dx%dx%d" % (s, s, SPP), "threads": args.oracle_threads,
                          "seconds": round(sec, 3), "knn_queries": st.knn_queries,
                          "queries_per_s": st.knn_queries / sec}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layouts", default="16,8,auto")
    ap.add_argument("--ks", default="10,16,17,32,64,128,256")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--oracle-size", type=int, default=128)
    ap.add_argument("--oracle-threads", type=int, default=16)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--oracle-only", action="store_true")
    ap.add_argument("--layout", default="auto")
    args = ap.parse_args()
    args.ks = [int(x) for x in args.ks.split(",")]
    if args.child:
        return child(args)
    if args.oracle_only:
        return oracle(args)
    lines = []
    for layout in args.layouts.split(","):
        env = dict(os.environ, RT_KNN_VERBOSE="1", RT_KNN_WIDE_LAYOUT=layout)
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--layout", layout, "--ks",
               ",".join(map(str, args.ks)), "--steps", str(args.steps), "--warmup", str(args.warmup)]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            sys.exit("layout %s: the child exited with %d" % (layout, r.returncode))
        inst = {}  # k -> (kernel, waves per CU) of the timed instance (the last report line of that k)
        for l in r.stderr.splitlines():
            if l.startswith("{\"knn_kernel\""):
                d = json.loads(l)
                inst[d["k"]] = (d["knn_kernel"], d["layout"], d["lds_bytes"], d["waves_per_cu"])
        for l in r.stdout.splitlines():
            d = json.loads(l)
            kern = inst.get(d["k"])
            if kern:
                d.update(kernel=kern[0], heap_layout=kern[1], lds_bytes=kern[2], waves_per_cu=kern[3])
            lines.append(d)
            print(json.dumps(d), flush=True)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--oracle-only", "--ks", ",".join(map(str, args.ks)),
                        "--oracle-size", str(args.oracle_size), "--oracle-threads", str(args.oracle_threads)],
                       capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        sys.exit("oracle: exited with %d" % r.returncode)
    for l in r.stdout.splitlines():
        lines.append(json.loads(l))
        print(l, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
