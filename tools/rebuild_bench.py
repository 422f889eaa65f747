"""Does rt_bvh_quality's ratio track what a refit costs the frames, and what does rt_rebuild cost beside rt_create?  The
workloads and angles of tools/refit_bench.py: slot 3 of a preset scene turned about the y axis by 5, 20 and 90 degrees
from its pose at rt_create.  Per workload and angle, one JSON row:
  ratio                  rt_bvh_quality.ratio of the refit tree (cost / cost_built; cost and cost_built beside it)
  nodes_ratio            node records visited per ray on the refit tree / on a fresh tree of the same pose (collect_stats)
  frame_ratio            kernel ms of one frame on the refit tree / on the fresh tree
  quality_ms / refit_ms  device ms of one rt_bvh_quality_get / of the rt_update refit of the same context
  rebuild_*              rt_rebuild's report on the refit context: total, build, read-back and host-plan ms
                         (device build + renumbering = build - plan)
  create_ms / create_build_ms   wall ms of a fresh rt_create of the same arrays in the same process / its rt_bvh_info.build_ms
  nodes_rebuilt_ratio    nodes per ray on the rebuilt tree / on the fresh tree (1.0: the same tree)
The frames are the workload's image size at --spp samples (the ratios are the point).

  python tools/rebuild_bench.py [--workloads C4 C5 C5x8] [--spp 16] [--out profiles/rebuild/rebuild_bench.jsonl]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ray-tracing-engine_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pyrt  # noqa: E402
from refit_bench import WORKLOADS, frame, turned  # noqa: E402


def quality_ms(ctx):
    """(device ms of one rt_bvh_quality_get — the second of two calls —, its result)"""
    ctx.bvh_quality()
    ctx.profile_reset()
    q = ctx.bvh_quality()
    ms, n = ctx.profile_collect()
    assert n == 1
    return ms, q


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", nargs="+", default=["C4", "C5", "C5x8"], choices=sorted(WORKLOADS))
    ap.add_argument("--angles", nargs="+", type=float, default=[5.0, 20.0, 90.0])
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rebuild", "rebuild_bench.jsonl"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for wl in args.workloads:
            kind, w, h = WORKLOADS[wl]
            s = pyrt.Scene(kind, w, h)
            a = s.arrays()
            for deg in args.angles:
                # a context per angle: every row is ONE refit away from the build, as in refit_bench's table
                ctx = pyrt.Context(s)
                pos, nrm = turned(a, deg)
                rep = ctx.update(pos=pos, nrm=nrm)
                q_ms, q = quality_ms(ctx)
                ms_r, nodes_r = frame(ctx, w, h, args.spp)
                t0 = time.perf_counter()
                fresh = pyrt.Context(pyrt.ArrayScene(pos, nrm, a["tri"], a["tri_begin"], a["vtx_begin"], a["materials"],
                                                     a["lights"], a["camera"]))
                create_ms = (time.perf_counter() - t0) * 1e3
                ms_n, nodes_n = frame(fresh, w, h, args.spp)
                rb = ctx.rebuild()
                ms_b, nodes_b = frame(ctx, w, h, args.spp)
                row = dict(workload=wl, deg=deg, spp=args.spp, triangles=ctx.bvh_info().n_tri_records, nodes=q["n_nodes"],
                           ratio=round(q["ratio"], 6), cost=round(q["cost"], 4), cost_built=round(q["cost_built"], 4),
                           nodes_ratio=round(nodes_r / nodes_n, 4), frame_ratio=round(ms_r / ms_n, 4),
                           nodes_refit=round(nodes_r, 3), nodes_new=round(nodes_n, 3), frame_ms_refit=round(ms_r, 3),
                           frame_ms_new=round(ms_n, 3), quality_ms=round(q_ms, 4), refit_ms=round(rep["refit_ms"], 3),
                           rebuild_total_ms=round(rb["total_ms"], 3), rebuild_build_ms=round(rb["build_ms"], 3),
                           rebuild_readback_ms=round(rb["readback_ms"], 3), rebuild_plan_ms=round(rb["plan_ms"], 3),
                           rebuild_builder=rb["builder"], cost_after=round(rb["cost_after"], 4), create_ms=round(create_ms, 3),
                           create_build_ms=round(fresh.bvh_info().build_ms, 3), nodes_rebuilt_ratio=round(nodes_b / nodes_n, 4),
                           frame_ms_rebuilt=round(ms_b, 3))
                fresh.close()
                ctx.close()
                print(json.dumps(row), flush=True)
                f.write(json.dumps(row) + "\n")
                f.flush()
            s.close()


if __name__ == "__main__":
    main()
