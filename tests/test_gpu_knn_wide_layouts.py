"""Every wide k-NN instance on both heap layouts, against the oracle bit for bit.

k_render_wide (BRUTE x STATS x layout) and k_knn_wide ((S16, SPLIT16), (S16, WIDE8), (32-bit, WIDE8)) run in three
child processes: the launcher's own choice and the two layouts forced by RT_KNN_WIDE_LAYOUT (the library reads it, and
RT_KNN_VERBOSE, once per process).  Each child runs the same jobs and writes their outputs; its stderr carries the
verbose line of every wide launch.  The parent computes each oracle result once and holds every child's output to it:
rt_knn_wide query by query on the tie families across the 16-bit / 32-bit boundary, photon frames on cubes (every
instance), on tied results, with k = n on tiny maps, and on the deep BVHs of hires and stress, where the stack rows come
from the BVH and not the kd tree.  The verbose lines pin the launch plan: the layout the rule of DESIGN.md section 4.8
gives (restated below), the LDS it asks for, and that all eleven instances ran."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import orc
import pyrt
from test_gpu_knn import _family, _queries, _upload
from test_gpu_photon_wide import _map

pytestmark = pytest.mark.gpu

HEAP_WIDE8, HEAP_SPLIT16 = 0, 1
ROWS_PER_CU = 640  # LDS rows (64 words) of a CU: 160 KiB
STACK = 32  # rtbvh::kMaxDepth
KNN_KS = (17, 18, 31, 33, 63, 64, 100, 127, 128, 129, 200, 255, 256)
FRAME_KS = (17, 64, 128, 200, 256)
CHILDREN = (("auto", None), ("wide8", "8"), ("split16", "16"))
CHILD_TIMEOUT = 300  # seconds per child (each runs in well under a minute)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---------------------------------------------------------------- the launcher's rule, restated
def kd_rows(n):
    """rt_api.cpp kd_stack: stack rows of the k-NN walk over n photons (16-bit entries, two per row, below 65,535)."""
    kd = 1
    while (1 << kd) <= n:
        kd += 1
    return (kd + 3) // 2 if n < 65535 else kd + 1


def stack_levels(depth, n):
    """A frame's stack rows (depth: bvh_info().max_depth); rt_knn_wide's with depth 0."""
    return min(max(depth, 1, kd_rows(n)), STACK) + 1


def heap_rows(hl, k):
    return k + (k + 1) // 2 if hl == HEAP_SPLIT16 else 2 * k


def auto_layout(n, s, k):
    """wide_layout: the split planes where the indices fit 16 bits and they give the CU more waves."""
    split = ROWS_PER_CU // (s + heap_rows(HEAP_SPLIT16, k)) > ROWS_PER_CU // (s + heap_rows(HEAP_WIDE8, k))
    return HEAP_SPLIT16 if n < 65535 and split else HEAP_WIDE8


def expected_layout(force, n, s, k):
    if n >= 65535 or force == "8":
        return HEAP_WIDE8
    if force == "16":
        return HEAP_SPLIT16
    return auto_layout(n, s, k)


# ---------------------------------------------------------------- the jobs every child runs
class _Keep:
    """Stands in for a Context in test_gpu_knn._upload: the parent only needs the map in kdtree order (the children
    install it)."""

    def set_photons(self, pos, dir_):
        pass


def _jobs():
    """(jobs, arrays): rt_knn_wide calls and photon frames, in an order that changes scene and map rarely."""
    arrays, jobs = {}, []
    # 1. rt_knn_wide: the four tie families at 300 / 5,000 / 65,534 photons (16-bit), then 65,535 and 100,003 (32-bit)
    for n in (300, 5000, 65534, 65535, 100003):
        rng = np.random.default_rng(7100 + n)
        for kind in range(4):
            pos = _family(rng, n, kind)
            name = "knn_%d_%d" % (kind, n)
            arrays[name] = _upload(_Keep(), pos)
            arrays[name + "_q"] = _queries(rng, pos, 96 if n > 1000 else 128)
            jobs += [dict(op="knn", map=name, n=n, k=k) for k in KNN_KS if k <= n]

    def frames(group, scene, w, h, spp, mode, ks, mapname, nreq, accels, stats=(0, 1)):
        for k in ks:
            for accel in accels:
                for st in stats:
                    jobs.append(dict(op="frame", group=group, scene=scene, w=w, h=h, spp=spp, mode=mode, k=k,
                                     map=mapname, n=len(arrays[mapname]), nreq=nreq, stats=st, accel=accel))

    both = (pyrt.ACCEL_BVH, pyrt.ACCEL_BRUTE)
    # 2. every k_render_wide instance on cubes, ray and path mode; the doubled map's exactly tied results
    arrays["cubes"] = _map("cubes", 3000, seed=2)
    arrays["cubes_tied"] = _map("cubes", 4000, seed=3, doubled=True)
    for mode in (pyrt.MODE_RAY, pyrt.MODE_PATH):
        frames("instances", "cubes", 32, 24, 2, mode, FRAME_KS, "cubes", 3000, both)
        frames("tied", "cubes", 32, 24, 2, mode, (64, 256), "cubes_tied", 4000, (pyrt.ACCEL_BVH,))
    # 4. k = n: the seeded heap is the whole map
    for n in (17, 18, 33, 129, 256):
        arrays["cubes_%d" % n] = _map("cubes", 3000, seed=4, n=n)
        frames("k_is_n", "cubes", 32, 24, 2, pyrt.MODE_PATH if n % 2 else pyrt.MODE_RAY, (n,), "cubes_%d" % n, n, both)
    # 3. deep BVHs: hires (depth 16) and stress (depth 24); 16-bit maps of a few thousand photons and 32-bit ones
    for scene, w, seed, n32 in (("hires", 32, 8, 65535), ("stress", 20, 10, None)):
        arrays[scene + "_16"] = _map(scene, 5000, seed=seed)
        arrays[scene + "_32"] = _map(scene, 100000, seed=seed + 1, n=n32)
        frames("deep", scene, w, w, 2, pyrt.MODE_RAY, FRAME_KS, scene + "_16", 5000, (pyrt.ACCEL_BVH,))
        frames("deep", scene, w, w, 1, pyrt.MODE_PATH, (128 if scene == "hires" else 200,), scene + "_16", 5000,
               (pyrt.ACCEL_BVH,))
        frames("deep", scene, w, w, 2, pyrt.MODE_RAY, (64, 256), scene + "_32", n32 or 100000, (pyrt.ACCEL_BVH,))
    assert 3000 < len(arrays["stress_16"]) < 65535 and len(arrays["stress_32"]) >= 65535
    assert 3000 < len(arrays["hires_16"]) < 65535
    return jobs, arrays


CHILD = r'''
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import pyrt
jobs = json.load(open(sys.argv[2]))
arrays = np.load(sys.argv[3])
out, cur, scene, ctx, installed = {}, None, None, None, None
for i, j in enumerate(jobs):
    sys.stderr.write(json.dumps({"job": i}) + "\n")
    sys.stderr.flush()
    where = ("cubes", 16, 16) if j["op"] == "knn" else (j["scene"], j["w"], j["h"])
    if where != cur:
        if ctx is not None:
            ctx.close()
        scene = pyrt.Scene(*where)
        ctx, cur, installed = pyrt.Context(scene), where, None
    if j["map"] != installed:
        ph7 = arrays[j["map"]]
        ctx.set_photons(ph7[:, 0:3], ph7[:, 3:6])
        installed = j["map"]
    if j["op"] == "knn":
        out["%d_idx" % i], out["%d_dist" % i], out["%d_vis" % i] = ctx.knn_wide(arrays[j["map"] + "_q"], j["k"])
    else:
        w, h = j["w"], j["h"]
        p = pyrt.make_params(w, h, j["spp"], mode=j["mode"], seed=5, use_photons=1, k=j["k"], photons_requested=j["nreq"],
                             collect_stats=j["stats"], accel=j["accel"])
        img, acc, st = ctx.render(p, pyrt.background(w, h))
        out["%d_img" % i], out["%d_acc" % i] = img, acc
        out["%d_st" % i] = np.array([st.knn_queries, st.kd_visited], np.uint64)
        out["%d_depth" % i] = np.array(ctx.bvh_info().max_depth)
ctx.close()
np.savez(sys.argv[4], **out)
'''


def _wide_lines(stderr, njobs):
    """The verbose lines of each job's wide launches (the child marks where a job starts)."""
    by_job, cur = [[] for _ in range(njobs)], None
    for line in stderr.splitlines():
        try:
            rec = json.loads(line)
        except ValueError:
            continue
        if not isinstance(rec, dict):
            continue
        if "job" in rec:
            cur = rec["job"]
        elif "knn_kernel" in rec:
            assert cur is not None, line
            by_job[cur].append(rec)
    return by_job


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """(jobs, arrays, {child: (forced layout, outputs, verbose lines per job)}).  One child at a time, each under its own
    timeout; the first that fails ends the fixture, and no further child starts."""
    tmp = tmp_path_factory.mktemp("knn_wide_layouts")
    jobs, arrays = _jobs()
    (tmp / "jobs.json").write_text(json.dumps(jobs))
    np.savez(tmp / "arrays.npz", **arrays)
    (tmp / "child.py").write_text(CHILD)
    res = {}
    for name, force in CHILDREN:
        env = dict(os.environ, RT_KNN_VERBOSE="1")
        env.pop("RT_KNN_WIDE_LAYOUT", None)
        if force:
            env["RT_KNN_WIDE_LAYOUT"] = force
        dst = tmp / (name + ".npz")
        cmd = [sys.executable, str(tmp / "child.py"), os.path.join(pyrt.ROOT, "ray-tracing-engine_amd"), str(tmp / "jobs.json"),
               str(tmp / "arrays.npz"), str(dst)]
        try:
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
        except subprocess.TimeoutExpired:
            pytest.fail("child %s ran out of its %d s" % (name, CHILD_TIMEOUT))
        if r.returncode != 0:
            pytest.fail("child %s exited with %d:\n%s" % (name, r.returncode, r.stderr[-3000:]))
        res[name] = (force, dict(np.load(dst)), _wide_lines(r.stderr, len(jobs)))
    return jobs, arrays, res


_oracle_frames = {}


def _oracle_frame(j, arrays):
    """The oracle's frame for a frame job (any accel, either stats setting: the oracle counts always), once."""
    key = tuple(j[f] for f in ("scene", "w", "h", "spp", "mode", "k", "map", "nreq"))
    if key not in _oracle_frames:
        w, h = j["w"], j["h"]
        p = pyrt.make_params(w, h, j["spp"], mode=j["mode"], seed=5, use_photons=1, k=j["k"], photons_requested=j["nreq"],
                             collect_stats=1)
        accel = orc.ACCEL_LOOP if j["scene"] == "cubes" else orc.ACCEL_OBVH
        out, acc, st = orc.render(pyrt.Scene(j["scene"], w, h), p, math_mode=orc.MATH_DET, bg=pyrt.background(w, h),
                                  ext_photons=arrays[j["map"]], accel=accel)
        _oracle_frames[key] = (out, acc, int(st.knn_queries), int(st.kd_visited))
    return _oracle_frames[key]


def _check_frames(runs, group):
    jobs, arrays, res = runs
    checked = 0
    for i, j in enumerate(jobs):
        if j["op"] != "frame" or j["group"] != group:
            continue
        ref_out, ref_acc, ref_q, ref_v = _oracle_frame(j, arrays)
        for name, (_, out, lines) in res.items():
            tag = (name, j["scene"], j["w"], j["h"], j["spp"], j["mode"], j["k"], j["map"], j["n"], j["stats"], j["accel"],
                   [l["layout"] for l in lines[i]])
            assert np.array_equal(bits(out["%d_acc" % i]), bits(ref_acc)), tag
            assert np.array_equal(bits(out["%d_img" % i]), bits(ref_out)), tag
            q, v = (int(x) for x in out["%d_st" % i])
            assert q == ref_q, (tag, q, ref_q)
            if j["stats"]:
                assert 0 < v <= ref_v, (tag, v, ref_v)
            checked += 1
    return checked


def test_knn_wide_on_both_layouts_equals_oracle(runs):
    """rt_knn_wide under the launcher's choice and both forced layouts: indices and distance bits (NaN as NaN) of every
    query, visits never more than the oracle's; from 65,535 photons even RT_KNN_WIDE_LAYOUT=16 takes WIDE8."""
    jobs, arrays, res = runs
    for i, j in enumerate(jobs):
        if j["op"] != "knn":
            continue
        ri, rd, rv = orc.knn(arrays[j["map"]], arrays[j["map"] + "_q"], j["k"])
        for name, (force, out, lines) in res.items():
            idx, dist, vis = out["%d_idx" % i], out["%d_dist" % i], out["%d_vis" % i]
            tag = (name, j["map"], j["k"], [l["layout"] for l in lines[i]])
            assert idx.shape == ri.shape, tag
            bad_i = (idx != ri).any(1)
            bad_d = ((bits(dist) != bits(rd)) & ~(np.isnan(dist) & np.isnan(rd))).any(1)
            assert not (bad_i | bad_d).any(), (tag, int(bad_i.sum()), int(bad_d.sum()))
            assert (vis <= rv).all(), tag
            if force == "16" and j["n"] >= 65535:
                assert [l["layout"] for l in lines[i]] == [HEAP_WIDE8], tag


def test_every_render_wide_instance_equals_oracle(runs):
    """cubes, ray and path mode, k = 17 .. 256: BVH and brute force, timed and counting, on both layouts."""
    assert _check_frames(runs, "instances") == 3 * 2 * len(FRAME_KS) * 4


def test_tied_results_on_both_layouts(runs):
    """Every position twice (the copy with another photon's direction): k results that tie exactly."""
    assert _check_frames(runs, "tied") == 3 * 2 * 2 * 2


def test_k_equal_to_map_size(runs):
    """Maps of 17, 18, 33, 129 and 256 photons at k = n: nothing can be pruned."""
    assert _check_frames(runs, "k_is_n") == 3 * 5 * 4


def test_deep_bvhs_equal_oracle(runs):
    """hires and stress: the BVH, not the kd tree, sets the 16-bit maps' stack rows; the 1 M-triangle scene's launcher
    puts k = 128 and 200 over a 16-bit map on WIDE8 (the production path), and k = 256 over a 32-bit map asks for the
    largest LDS of any wide launch."""
    jobs, _, res = runs
    assert _check_frames(runs, "deep") == 3 * 2 * 2 * (len(FRAME_KS) + 1 + 2)
    _, auto, lines = res["auto"]
    stress_wide8 = set()
    for i, j in enumerate(jobs):
        if j["op"] == "frame" and j["group"] == "deep" and j["n"] < 65535:
            assert int(auto["%d_depth" % i]) > kd_rows(j["n"]), j  # the stack rows come from the BVH
            if j["scene"] == "stress" and lines[i][0]["layout"] == HEAP_WIDE8:
                stress_wide8.add(j["k"])
    assert {128, 200} <= stress_wide8, stress_wide8


def test_launch_plan_matches_the_rule(runs):
    """Every wide launch reports the layout the rule gives (or the forced one), LDS = 4 x (stack rows + heap rows) x 64,
    and together the children ran all eight k_render_wide and all three k_knn_wide instances."""
    jobs, _, res = runs
    render, knn, report = set(), set(), {}
    for name, (force, out, lines) in res.items():
        for i, j in enumerate(jobs):
            assert len(lines[i]) == 1, (name, i, j, lines[i])
            rec = lines[i][0]
            depth = int(out["%d_depth" % i]) if j["op"] == "frame" else 0
            s = stack_levels(depth, j["n"])
            hl = expected_layout(force, j["n"], s, j["k"])
            tag = (name, j, s, rec)
            assert rec["knn_kernel"] == ("k_knn_wide" if j["op"] == "knn" else "k_render_wide"), tag
            assert (rec["k"], rec["layout"]) == (j["k"], hl), tag
            assert rec["lds_bytes"] == 4 * (s + heap_rows(hl, j["k"])) * 64, tag
            if j["op"] == "knn":
                knn.add((j["n"] < 65535, hl))
            else:
                render.add((j["accel"], j["stats"], hl))
                if force and j["accel"] == pyrt.ACCEL_BVH and not j["stats"]:
                    report.setdefault((j["scene"], j["n"] < 65535, j["k"]), {})[hl] = (rec["lds_bytes"], rec["waves_per_cu"])
    assert render == {(a, st, hl) for a in (pyrt.ACCEL_BVH, pyrt.ACCEL_BRUTE) for st in (0, 1)
                      for hl in (HEAP_WIDE8, HEAP_SPLIT16)}, render
    assert knn == {(True, HEAP_SPLIT16), (True, HEAP_WIDE8), (False, HEAP_WIDE8)}, knn
    # occupancy is the runtime's and a performance matter: reported, not asserted
    for (scene, kd16, k), by in sorted(report.items()):
        print("k_render_wide %-6s %s-bit map k=%3d: " % (scene, "16" if kd16 else "32", k)
              + ", ".join("%s %d B %d waves/CU" % (("WIDE8", "SPLIT16")[hl], *by[hl]) for hl in sorted(by)))
