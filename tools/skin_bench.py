"""What posing a skinned scene costs by each of the four update calls.  Every vertex of a preset scene hangs on a "bend" of
64 bones stacked along y (bone j turned about y by (j + 1) x 0.5 degrees and moved a little), by one, two or four
influences.  Per workload and rig one JSON row; in one process, after --warmup rounds, --rounds rounds of the four calls one
after the other, the wall time of each call (the report's total_ms) as [min, median, max]:
  skin_ms          rt_update_skin: 88 bytes per bone cross the bus, the device blends
  host_ms          rt_update with the posed arrays in host memory (24 bytes per vertex cross the bus)
  host_prepare_ms  numpy's own time to blend those arrays on the host — beside host_ms, not inside it
  device_ms        rt_update_vertices_device with arrays already in device memory
  transforms_ms    rt_update_transforms with one record per mesh (mesh 3 turned)
  *_refit_ms       the median device time of the call's refit kernels
  skin_below_host  skin_ms's max < host_ms's min: the two intervals do not overlap
  same_tree        rt_update_skin and rt_update with numpy's arrays leave the same export (checked once per row)
The rest pose is shared by rt_update_transforms and rt_update_skin and taken anew after a call that gives arrays: a round
gives the rest arrays back (the device form) and takes the snapshot in an untimed call, so that neither timed call pays it.

  python tools/skin_bench.py [--workloads C4 C5 C5x8] [--rounds 5] [--out file.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ray-tracing-engine_amd"))
import pyrt  # noqa: E402

# name: (scene, width, height) — bench.py WORKLOADS
WORKLOADS = {"C4": ("hires", 2048, 2048), "C5": ("stress", 1024, 1024), "C5x8": ("stress8", 1024, 1024)}
N_BONES = 64
SLOT = 3


def bend_bones(step_deg=0.5):
    j = np.arange(1, N_BONES + 1)
    phi = np.deg2rad(j * step_deg).astype(np.float32)
    c, s = np.cos(phi, dtype=np.float32), np.sin(phi, dtype=np.float32)
    t = pyrt.make_transforms(N_BONES)
    t["flags"] = 0
    for f in ("m", "n"):
        t[f][:, 0, 0], t[f][:, 0, 2], t[f][:, 2, 0], t[f][:, 2, 2] = c, s, -s, c
    t["m"][:, :, 3] = (j[:, None] * np.array([1e-4, 2e-4, -1e-4])).astype(np.float32)
    return t


def bend_skin(pos, influences):
    """Every vertex on the `influences` bones nearest to its height."""
    y = pos[:, 1].astype(np.float64)
    t = (y - y.min()) / max(y.max() - y.min(), 1e-30) * (N_BONES - 1)
    j0 = np.minimum(np.floor(t), N_BONES - 2).astype(np.int64)
    f = (t - j0).astype(np.float32)
    bone, weight = np.zeros((len(pos), 4), np.uint16), np.zeros((len(pos), 4), np.float32)
    if influences == 1:
        bone[:, 0], weight[:, 0] = np.rint(t), 1.0
    elif influences == 2:
        bone[:, 0], bone[:, 1] = j0, j0 + 1
        weight[:, 0], weight[:, 1] = np.float32(1) - f, f
        weight[:, :2][weight[:, :2] == 0] = np.float32(1e-3)  # (both slots in use everywhere)
    else:
        for k, share in enumerate((0.1, 0.4, 0.3, 0.2)):
            bone[:, k], weight[:, k] = np.clip(j0 - 1 + k, 0, N_BONES - 1), share
    assert ((weight != 0).sum(axis=1) == influences).all()
    return bone, weight


def blend(pos, nrm, bone, weight, bones):
    """The header's blend in numpy, float32, column by column."""
    X, Y = np.zeros_like(pos), np.zeros_like(nrm)
    for k in range(4):
        on = weight[:, k] != 0
        if not on.any():
            continue
        w, m, n = weight[on, k], bones["m"][bone[on, k]], bones["n"][bone[on, k]]
        x, y, z = pos[on, 0], pos[on, 1], pos[on, 2]
        a, b, c = nrm[on, 0], nrm[on, 1], nrm[on, 2]
        for i in range(3):
            X[on, i] = X[on, i] + w * (((m[:, i, 0] * x + m[:, i, 1] * y) + m[:, i, 2] * z) + m[:, i, 3])
            Y[on, i] = Y[on, i] + w * ((n[:, i, 0] * a + n[:, i, 1] * b) + n[:, i, 2] * c)
    return X, Y


def spread(reps, key):
    v = sorted(r[key] for r in reps)
    return [round(v[0], 4), round(statistics.median(v), 4), round(v[-1], 4)]


def same(e1, e2):
    return bool(np.array_equal(e1[0], e2[0]) and np.array_equal(e1[1], e2[1]))


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", nargs="+", default=["C4", "C5", "C5x8"], choices=sorted(WORKLOADS))
    ap.add_argument("--influences", nargs="+", type=int, default=[2, 1, 4], choices=[1, 2, 4])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the rows to this file (JSON lines)")
    args = ap.parse_args()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") if args.out else open(os.devnull, "w") as f:
        for wl in args.workloads:
            kind, w, h = WORKLOADS[wl]
            s = pyrt.Scene(kind, w, h)
            a = s.arrays()
            n_meshes = len(a["vtx_begin"]) - 1
            ctx = pyrt.Context(s)
            bi = ctx.bvh_info()
            stream = torch.cuda.current_stream().cuda_stream
            print("%s: %d triangles, %d vertices, %d meshes" % (wl, bi.n_tri_records, len(a["pos"]), n_meshes), flush=True)
            d_rest_p, d_rest_n = torch.from_numpy(a["pos"]).cuda(), torch.from_numpy(a["nrm"]).cuda()
            static = pyrt.make_transforms(n_meshes)
            turn = pyrt.make_transforms(n_meshes)
            R = bend_bones(20.0)[0]
            turn["m"][SLOT], turn["n"][SLOT], turn["flags"][SLOT] = R["m"], R["n"], 0
            bones = bend_bones()
            for infl in args.influences:
                bone, weight = bend_skin(a["pos"], infl)
                t0 = time.perf_counter()
                pos, nrm = blend(a["pos"], a["nrm"], bone, weight, bones)
                prepare_ms = (time.perf_counter() - t0) * 1e3
                ctx.set_skin(bone, weight, N_BONES)
                torch.cuda.synchronize()
                reps = dict(host=[], device=[], transforms=[], skin=[])
                ok = None
                for rnd in range(args.warmup + args.rounds):
                    got = dict(host=ctx.update(pos=pos, nrm=nrm))
                    ref = ctx.bvh_export() if ok is None else None
                    got["device"] = ctx.update_vertices_device(d_rest_p.data_ptr(), d_rest_n.data_ptr(), stream)
                    ctx.update_transforms(static, stream=stream)  # (untimed: takes the rest pose)
                    got["transforms"] = ctx.update_transforms(turn, stream=stream)
                    got["skin"] = ctx.update_skin(bones, stream=stream)
                    if ok is None:
                        ok = same(ref, ctx.bvh_export())
                    if rnd >= args.warmup:
                        for k, v in got.items():
                            reps[k].append(v)
                row = dict(workload=wl, influences=infl, bones=N_BONES, triangles=bi.n_tri_records, vertices=len(a["pos"]),
                           meshes=n_meshes, rounds=args.rounds, host_prepare_ms=round(prepare_ms, 3), same_tree=ok)
                for k, v in reps.items():
                    row[k + "_ms"], row[k + "_refit_ms"] = spread(v, "total_ms"), spread(v, "refit_ms")[1]
                row["skin_below_host"] = row["skin_ms"][2] < row["host_ms"][0]
                print(json.dumps(row), flush=True)
                f.write(json.dumps(row) + "\n")
                ctx.update(pos=a["pos"], nrm=a["nrm"])
            ctx.close()
            s.close()


if __name__ == "__main__":
    main()
