"""Device time of rt_render_lights_device on one MI355X, in two parts.

like (C2: `lowres`, 1024 x 1024, 128 spp, path mode, depth 3; RT_NO_PERSIST=1, one process):
  render_no_persist    rt_render_device: k_render, the one-wave-per-workgroup family the light-group instances belong to —
                       the like-for-like baseline
  lights_all_g1        rt_render_lights_device, one group of all lights: the same frame, what the group bookkeeping costs
                       when it changes nothing
  lights_singletons_g3 one group per light: three frames from the rays of one
  The shapes take turns launch by launch for --repeats rounds after --warmup rounds; every figure is the library's own
  event pair round the kernel (rt_stats.kernel_ms).

claim (C2 and `cubes`, 256 x 256, 8 spp; the default environment, so rt_render_device runs its persistent kernel):
  call                 ONE rt_render_lights_device call with one group per light
  loop_with_update     what a user writes today: per light, rt_update(lights with the others' colours zeroed) and
                       rt_render_device on one context
  loop_no_update       the same three frames on three contexts whose lights were zeroed beforehand: the loop without its
                       rt_update calls
  Before any timed run the accumulators of the call and of the loop are compared bit for bit (bits_equal,
  pixels_differing_per_slice); a differing pixel is taken apart by one-sample ranges into `difference` rows: the header's
  L1 holds where no unoccluded term of a zeroed light is non-finite.  kernel_ms is the sum of the
  event pairs of a side's launches; wall_ms is the host's clock from the first call to the end of a stream
  synchronisation, rt_update included.  The sides take turns for --repeats rounds after --warmup rounds; `disjoint` says
  whether the call's min..max lies wholly below the loop's.

  python tools/lights_bench.py [--repeats 5] [--warmup 2] [--out profiles/lights/lights_bench.jsonl]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C2 = ("lowres", 1024, 128)
SMALL = ("cubes", 256, 8)


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


def like(args):
    np, torch, pyrt = setup()
    name, size, spp = C2
    stream = torch.cuda.current_stream()
    scene = pyrt.Scene(name, size, size)
    nl = len(scene.arrays()["lights"])
    ctx = pyrt.Context(scene)
    p = pyrt.make_params(size, size, spp, mode=pyrt.MODE_PATH, max_depth=3, seed=1)
    acc = torch.zeros((nl, size, size, 4), dtype=torch.float32, device="cuda")
    shapes = {"render_no_persist": lambda: ctx.render_device(p, acc.data_ptr(), stream=stream.cuda_stream, stats=True),
              "lights_all_g1": lambda: ctx.render_lights_device(p, [(1 << nl) - 1], acc.data_ptr(), stream=stream.cuda_stream, stats=True),
              "lights_singletons_g%d" % nl: lambda: ctx.render_lights_device(p, [1 << l for l in range(nl)], acc.data_ptr(),
                                                                             stream=stream.cuda_stream, stats=True)}
    ms, last = {k: [] for k in shapes}, {}
    for it in range(args.warmup + args.repeats):
        for k, fn in shapes.items():
            last[k] = fn()
            if it >= args.warmup:
                ms[k].append(last[k].kernel_ms)
    ctx.close()
    base = summary(ms["render_no_persist"])["median"]
    for k, v in ms.items():
        s, st = summary(v), last[k]
        rays = st.rays_closest + st.rays_shadow
        print(json.dumps(dict(part="like", shape=k, rt_no_persist=True, scene=name, width=size, height=size, spp=spp, repeats=len(v),
                              kernel_ms=s["median"], ms_min=s["min"], ms_max=s["max"], spread_pct=s["spread_pct"], rays=rays,
                              grays_s=round(rays / s["median"] / 1e6, 3), ratio_to_no_persist=round(s["median"] / base, 4))), flush=True)


def claim(args):
    np, torch, pyrt = setup()
    stream = torch.cuda.current_stream()
    for name, size, spp in (C2, SMALL):
        scene = pyrt.Scene(name, size, size)
        lights = np.array(scene.arrays()["lights"], np.float32).reshape(-1, 21)
        nl = len(lights)
        masks = [1 << l for l in range(nl)]

        def only(l):
            z = lights.copy()
            for j in range(nl):
                if j != l:
                    z[j, 3:6] = 0.0
            return z

        p = pyrt.make_params(size, size, spp, mode=pyrt.MODE_PATH, max_depth=3, seed=1)
        one, loop = pyrt.Context(scene), pyrt.Context(scene)
        fixed = [pyrt.Context(scene) for _ in range(nl)]
        for l, c in enumerate(fixed):
            c.update(lights=only(l))
        a_call = torch.zeros((nl, size, size, 4), dtype=torch.float32, device="cuda")
        a_loop = torch.zeros_like(a_call)

        def call():
            a_call.zero_()
            stream.synchronize()
            t0 = time.perf_counter()
            st = one.render_lights_device(p, masks, a_call.data_ptr(), stream=stream.cuda_stream, stats=True)
            stream.synchronize()
            return (time.perf_counter() - t0) * 1e3, st.kernel_ms, st.rays_closest + st.rays_shadow

        def loop_with_update():
            a_loop.zero_()
            stream.synchronize()
            t0, k, rays = time.perf_counter(), 0.0, 0
            for l in range(nl):
                loop.update(lights=only(l))
                st = loop.render_device(p, a_loop[l].data_ptr(), stream=stream.cuda_stream, stats=True)
                k, rays = k + st.kernel_ms, rays + st.rays_closest + st.rays_shadow
            stream.synchronize()
            return (time.perf_counter() - t0) * 1e3, k, rays

        def loop_no_update():
            a_loop.zero_()
            stream.synchronize()
            t0, k, rays = time.perf_counter(), 0.0, 0
            for l in range(nl):
                st = fixed[l].render_device(p, a_loop[l].data_ptr(), stream=stream.cuda_stream, stats=True)
                k, rays = k + st.kernel_ms, rays + st.rays_closest + st.rays_shadow
            stream.synchronize()
            return (time.perf_counter() - t0) * 1e3, k, rays

        # the two sides' accumulators, bit for bit, before any timed run.  Where they differ, every differing pixel is taken
        # apart sample by sample (one-sample ranges on both sides) and reported in a row of its own: the header's L1 holds
        # on the condition that no unoccluded term of a zeroed light is non-finite, and a frame of 134 M samples may hold one.
        call()
        got = a_call.cpu().numpy().copy()
        differing = None
        for side in (loop_with_update, loop_no_update):
            side()
            d = (a_loop.cpu().numpy().view(np.uint32) != got.view(np.uint32)).any(-1)
            assert differing is None or (d == differing).all(), "%s: the loop's two forms differ from each other" % name
            differing = d
        bits_equal = not differing.any()
        for g, y, x in np.argwhere(differing)[:8]:
            for i in range(spp):
                q = pyrt.make_params(size, size, spp, mode=pyrt.MODE_PATH, max_depth=3, seed=1, spp_begin=i, spp_count=1)
                a_call.zero_(), a_loop.zero_()
                one.render_lights_device(q, masks, a_call.data_ptr(), stream=stream.cuda_stream)
                for l in range(nl):
                    fixed[l].render_device(q, a_loop[l].data_ptr(), stream=stream.cuda_stream)
                stream.synchronize()
                ca, lo = a_call[:, y, x].cpu().numpy(), a_loop[:, y, x].cpu().numpy()
                if (ca[g].view(np.uint32) != lo[g].view(np.uint32)).any():
                    print(json.dumps(dict(part="claim", shape="difference", scene=name, width=size, height=size, spp=spp, slice=int(g),
                                          y=int(y), x=int(x), sample=i, call_per_slice=ca.tolist(), loop_per_frame=lo.tolist())), flush=True)
        sides = {"call": call, "loop_with_update": loop_with_update, "loop_no_update": loop_no_update}
        wall, kern, rays = {k: [] for k in sides}, {k: [] for k in sides}, {}
        for it in range(args.warmup + args.repeats):
            for k, fn in sides.items():
                w, km, rays[k] = fn()
                if it >= args.warmup:
                    wall[k].append(w), kern[k].append(km)
        for c in [one, loop] + fixed:
            c.close()
        cw, ck = summary(wall["call"]), summary(kern["call"])
        for k in sides:
            w, km = summary(wall[k]), summary(kern[k])
            row = dict(part="claim", shape=k, scene=name, width=size, height=size, spp=spp, groups=nl, repeats=len(wall[k]), bits_equal=bool(bits_equal),
                       pixels_differing_per_slice=differing.reshape(nl, -1).sum(1).tolist(),
                       rays=rays[k], kernel_ms=km["median"], kernel_ms_min=km["min"], kernel_ms_max=km["max"],
                       wall_ms=w["median"], wall_ms_min=w["min"], wall_ms_max=w["max"])
            if k != "call":
                row.update(kernel_ratio_to_call=round(km["median"] / ck["median"], 3), wall_ratio_to_call=round(w["median"] / cw["median"], 3),
                           kernel_disjoint=ck["max"] < km["min"], wall_disjoint=cw["max"] < w["min"])
            print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lights", "lights_bench.jsonl"))
    ap.add_argument("--child", choices=("like", "claim"))
    args = ap.parse_args()
    if args.child:
        return like(args) if args.child == "like" else claim(args)
    rows = []
    for part in ("like", "claim"):
        env = dict(os.environ)
        env.pop("RT_NO_PERSIST", None)
        if part == "like":
            env["RT_NO_PERSIST"] = "1"  # (read once per process)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", part, "--repeats", str(args.repeats), "--warmup", str(args.warmup)],
                           env=env, stdout=subprocess.PIPE, text=True, check=True)
        for l in r.stdout.splitlines():
            if l.startswith("{"):
                rows.append(json.loads(l))
                print(l, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        for r in rows:
            fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
