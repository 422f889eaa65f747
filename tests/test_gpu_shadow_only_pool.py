"""The vertex pool's shadow-only body (vertex_pool<..., BOUNCE = false>: the pool of a path's deepest vertex and the only
pool of a ray-mode frame, walked by the any-hit traversal; the instances with the whole tree in LDS have it, which is what
these small scenes run by default) against the sequential shading, the oracle, the schedule of the general body it
replaced there, and the instances that keep the general body (other pool layouts, tree placements, kernel families)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import orc
import pyrt

pytestmark = pytest.mark.gpu

W, H = 20, 12  # (the wave tiles overhang the image on two sides)
SEED = 13
# (mode, max_depth): ray mode's only pool is shadow-only, a path's last pool is
MODES = ((pyrt.MODE_RAY, 3), (pyrt.MODE_PATH, 1), (pyrt.MODE_PATH, 2), (pyrt.MODE_PATH, 3))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def scenes():
    out = {}
    for kind in ("cubes", "lowres"):
        s = pyrt.Scene(kind, W, H)
        out[kind] = dict(scene=s, ctx=pyrt.Context(s), ref={})
    yield out
    for f in out.values():
        f["ctx"].close()


def oracle(f, mode, depth, spp):
    key = (mode, depth, spp)
    if key not in f["ref"]:
        _, acc, st = orc.render(f["scene"], pyrt.make_params(W, H, spp, mode=mode, max_depth=depth, seed=SEED), math_mode=orc.MATH_DET)
        acc.setflags(write=False)
        f["ref"][key] = (acc, st.rays_closest, st.rays_shadow)
    return f["ref"][key]


@pytest.mark.parametrize("lpp", (1, 4, 16, 64))
@pytest.mark.parametrize("spp", (16, 19))  # (19: a short last group)
@pytest.mark.parametrize("mode,depth", MODES, ids=("ray", "path1", "path2", "path3"))
@pytest.mark.parametrize("kind", ("cubes", "lowres"))
def test_pooled_frame_equals_sequential_and_oracle(scenes, kind, mode, depth, spp, lpp):
    f = scenes[kind]
    kw = dict(mode=mode, max_depth=depth, seed=SEED, lanes_per_pixel=lpp)
    _, acc, st = f["ctx"].render(pyrt.make_params(W, H, spp, **kw))
    _, seq, sq = f["ctx"].render(pyrt.make_params(W, H, spp, no_pool=True, **kw))
    ref, closest, shadow = oracle(f, mode, depth, spp)
    assert np.array_equal(bits(acc), bits(seq))
    assert np.array_equal(bits(acc), bits(ref))
    assert (st.rays_closest, st.rays_shadow) == (closest, shadow) == (sq.rays_closest, sq.rays_shadow)
    assert st.rays_shadow > 0


# The counted pass of one 32 x 32 x 16 frame of the 1,222-triangle scene at max_depth 3 (seed 13, the default samples per
# wave), where four rounds in ten are tail rounds: node visits and triangle tests depend on which lanes steal which
# subtrees and when, so equal totals show that the any-hit body hands out and steals exactly as the mixed one did.
# Recorded from the kernel of commit 73f83ef (the parent of the shadow-only body), on MI355X.
PARENT_COMMIT = "73f83ef"
PARENT_NODES_VISITED = 1362354
PARENT_TRIS_TESTED = 525814
PARENT_RAYS = (46589, 127476)  # (closest, shadow)


def test_stealing_schedule_is_the_mixed_body_s():
    s = pyrt.Scene("lowres", 32, 32)
    ctx = pyrt.Context(s)
    _, _, st = ctx.render(pyrt.make_params(32, 32, 16, mode=pyrt.MODE_PATH, max_depth=3, seed=SEED, collect_stats=1))
    ctx.close()
    print("nodes_visited %d tris_tested %d rays %d %d" % (st.nodes_visited, st.tris_tested, st.rays_closest, st.rays_shadow))
    assert (st.rays_closest, st.rays_shadow) == PARENT_RAYS
    assert st.nodes_visited == PARENT_NODES_VISITED, PARENT_COMMIT
    assert st.tris_tested == PARENT_TRIS_TESTED, PARENT_COMMIT


def test_shadow_only_frame_is_the_same_under_every_layout(tmp_path):
    """One frame whose pools are all shadow-only (path mode, max_depth 1) with the pool layout, the tree placement, the
    wave count and the kernel family forced the other way (the knobs are read once per process: child processes)."""
    script = tmp_path / "frame.py"
    script.write_text('''
import sys, numpy as np
sys.path.insert(0, sys.argv[1] + "/ray-tracing-engine_amd")
import pyrt
s = pyrt.Scene("lowres", 44, 28); ctx = pyrt.Context(s)
_, acc, st = ctx.render(pyrt.make_params(44, 28, 7, mode=pyrt.MODE_PATH, max_depth=1, seed=13))
np.savez(sys.argv[2], acc=acc, rays=np.array([st.rays_closest, st.rays_shadow]))
ctx.close()
''')
    variants = (("default", {}), ("compact", {"RT_COMPACT": "1"}), ("compact2", {"RT_COMPACT": "2"}), ("no_lds_tree", {"RT_TOPK": "0"}),
                ("eight_waves", {"RT_PERSIST_WAVES": "8"}), ("one_wave_per_group", {"RT_NO_PERSIST": "1"}))
    runs = {}
    for name, env in variants:
        out = tmp_path / (name + ".npz")
        r = subprocess.run([sys.executable, str(script), pyrt.ROOT, str(out)], env=dict(os.environ, **env), capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 0, (name, r.stderr[-2000:])
        runs[name] = np.load(out)
    assert runs["default"]["rays"][1] > 0
    for name, _ in variants[1:]:
        assert np.array_equal(bits(runs["default"]["acc"]), bits(runs[name]["acc"])), name
        assert np.array_equal(runs["default"]["rays"], runs[name]["rays"]), name
