"""What a refit (rt_update) costs and what it costs the frames: slot 3 of a preset scene turned about the y axis (the
reference's rotationY, Main.cpp:88-99) by 5, 20 and 90 degrees from its pose at rt_create.  Per workload and angle, one
JSON row:
  refit_ms / update_ms   device time of the refit kernels / wall time of rt_update (upload + magnitude pass + refit)
  build_ms               rt_bvh_info.build_ms of a fresh rt_create of the turned scene (what a rebuild costs instead)
  frame_ms_refit / _new  kernel ms of one frame on the refit tree / on the fresh tree
  nodes_refit / _new     node records visited per ray in that frame (collect_stats) — the tree quality lost
The frames are the workload's image size at --spp samples (not bench.py's full frame: the ratio is the point).

  python tools/refit_bench.py [--workloads C4 C5 C5x8] [--spp 16] [--out file.jsonl]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ray-tracing-engine_amd"))
import pyrt  # noqa: E402

# name: (scene, width, height) — bench.py WORKLOADS
WORKLOADS = {"C4": ("hires", 2048, 2048), "C5": ("stress", 1024, 1024), "C5x8": ("stress8", 1024, 1024)}


def turned(a, deg, slot=3):
    phi = np.float32(np.deg2rad(deg))
    c, s = np.cos(phi, dtype=np.float32), np.sin(phi, dtype=np.float32)
    R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], np.float32)
    b, e = a["vtx_begin"][slot], a["vtx_begin"][slot + 1]
    pos, nrm = a["pos"].copy(), a["nrm"].copy()
    pos[b:e] = (pos[b:e] @ R.T).astype(np.float32)
    nrm[b:e] = (nrm[b:e] @ R.T).astype(np.float32)
    return pos, nrm


def frame(ctx, w, h, spp):
    """(kernel ms of a frame, node records visited per ray of the same frame)"""
    p = pyrt.make_params(w, h, spp, mode=pyrt.MODE_PATH, seed=1)
    ctx.render(p, want_accum=False)  # (warm-up)
    _, _, st = ctx.render(p, want_accum=False)
    _, _, sc = ctx.render(pyrt.make_params(w, h, spp, mode=pyrt.MODE_PATH, seed=1, collect_stats=1), want_accum=False)
    return st.kernel_ms, sc.nodes_visited / max(1, sc.rays_closest + sc.rays_shadow)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", nargs="+", default=["C4", "C5", "C5x8"], choices=sorted(WORKLOADS))
    ap.add_argument("--angles", nargs="+", type=float, default=[5.0, 20.0, 90.0])
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--out", default=None, help="also write the rows to this file (JSON lines)")
    args = ap.parse_args()
    with open(args.out, "w") if args.out else open(os.devnull, "w") as f:
        for wl in args.workloads:
            kind, w, h = WORKLOADS[wl]
            t0 = time.time()
            s = pyrt.Scene(kind, w, h)
            a = s.arrays()
            ctx = pyrt.Context(s)
            bi = ctx.bvh_info()
            base_ms, base_nodes = frame(ctx, w, h, args.spp)
            print("%s: %d triangles, %d nodes, build %.1f ms, frame %.2f ms at %d spp, %.2f nodes/ray (scene set-up %.1f s)"
                  % (wl, bi.n_tri_records, bi.n_nodes, bi.build_ms, base_ms, args.spp, base_nodes, time.time() - t0), flush=True)
            for deg in args.angles:
                pos, nrm = turned(a, deg)
                rep = ctx.update(pos=pos, nrm=nrm)
                ms_r, nodes_r = frame(ctx, w, h, args.spp)
                fresh = pyrt.Context(pyrt.ArrayScene(pos, nrm, a["tri"], a["tri_begin"], a["vtx_begin"], a["materials"],
                                                     a["lights"], a["camera"]))
                ms_n, nodes_n = frame(fresh, w, h, args.spp)
                row = dict(workload=wl, deg=deg, spp=args.spp, triangles=bi.n_tri_records, refit_ms=round(rep["refit_ms"], 3),
                           update_ms=round(rep["total_ms"], 3), build_ms=round(fresh.bvh_info().build_ms, 3),
                           frame_ms_refit=round(ms_r, 3), frame_ms_new=round(ms_n, 3), nodes_refit=round(nodes_r, 3),
                           nodes_new=round(nodes_n, 3), frame_ms_untouched=round(base_ms, 3), nodes_untouched=round(base_nodes, 3))
                fresh.close()
                print(json.dumps(row), flush=True)
                f.write(json.dumps(row) + "\n")
            ctx.close()
            s.close()


if __name__ == "__main__":
    main()
