"""ao_ref (the CPU restatement of rt_render_ao) against the oracle, without a GPU: its numpy sampler reproduces the
oracle's own bounce rays bit for bit, its hits are aov_ref's, and the references the GPU tests compare against are
worth comparing against — neither all occluded nor all free, and the open scenes' frames hold empty, sparse and full
wave tiles."""
import ctypes as C

import numpy as np
import pytest

import ao_ref
import aov_ref
import orc
import pyrt

PRESETS = ("cubes", "lowres", "hires")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_sampler_equals_the_oracles_depth_1_bounce_rays():
    """A zero-light copy of cubes, 37x23, 1 spp, path mode, max_depth 2: no light is sampled, so the bounce direction of
    every primary hit is the hemisphere sample drawn right after the jitter's four engine calls, and the oracle's ray dump
    holds it as the depth-1 closest ray.  Every hit pixel: direction and origin bit for bit."""
    w, h = 37, 23
    a = pyrt.Scene("cubes", w, h).arrays()
    dark = pyrt.ArrayScene(a["pos"], a["nrm"], a["tri"], a["tri_begin"], a["vtx_begin"], a["materials"], a["lights"][:0], a["camera"])
    p = pyrt.make_params(w, h, 1, mode=pyrt.MODE_PATH, seed=11, max_depth=2)
    dump = orc.dump_rays(dark, p)
    tag = np.ascontiguousarray(dump[:, 3]).view(np.uint32)
    bounce = dump[tag == (1 << 8)]
    hit, nrm, pt = ao_ref.vertices(dark, p)
    hit, nrm, pt = hit[:, :, 0], nrm[:, :, 0], pt[:, :, 0]
    assert hit.all() and len(bounce) == w * h  # (a closed room)
    state = ao_ref.stream_seed(p.seed, ao_ref.STREAM_PIXEL, np.arange(w * h).reshape(h, w), np.zeros((h, w), np.uint32))
    for _ in range(4):
        state = ao_ref.engine_next(state)
    d, _ = ao_ref.hemisphere_sample(state, nrm)
    assert np.array_equal(bits(d).reshape(-1, 3), bits(bounce[:, 4:7]))
    assert np.array_equal(bits(pt).reshape(-1, 3), bits(bounce[:, 0:3]))


def test_sampler_pieces_equal_the_oracles():
    """The seed, the engine and the whole sampler against the oracle's unit entry points, on normals that take every
    branch of two_orthogonals."""
    L = orc.lib()
    rng = np.random.default_rng(5)
    idx, sub = rng.integers(0, 2 ** 32, 64, dtype=np.uint64), rng.integers(0, 2 ** 32, 64, dtype=np.uint64)
    got = ao_ref.stream_seed(77, ao_ref.STREAM_AO, idx, sub)
    assert [int(x) for x in got] == [L.orc_stream_seed(77, ao_ref.STREAM_AO, int(i), int(s)) for i, s in zip(idx, sub)]
    normals = np.concatenate([np.eye(3), -np.eye(3), [[1, 1, 1], [1, -1, 0], [0, 2, 2], [-0.0, 1, -0.0], [3, 0, 3]],
                              rng.normal(size=(240, 3))]).astype(np.float32)
    states = ao_ref.stream_seed(3, ao_ref.STREAM_AO, np.arange(len(normals)), np.zeros(len(normals)))
    d, end = ao_ref.hemisphere_sample(states, normals)
    for k in range(len(normals)):
        st, out = C.c_uint32(int(states[k])), np.zeros(3, np.float32)
        nk = np.ascontiguousarray(normals[k])
        L.orc_hsphere(C.byref(st), orc.MATH_DET, nk.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
        assert np.array_equal(bits(out), bits(d[k])) and st.value == int(end[k]), k


@pytest.mark.parametrize("case", ao_ref.CASES, ids=ao_ref.case_id)
def test_references_are_neither_all_occluded_nor_all_free(case):
    """Every reference test_gpu_ao.py compares against, the one-pixel frames included: between 2 % and 98 % of its
    occlusion rays are occluded, its hits are aov_ref's, and no pixel has more escaped rays than rays."""
    name, opened, w, h, rng, n_rays, brute, bias, dist = case
    ref = ao_ref.case_reference(case)
    print(ao_ref.case_id(case), "occluded share %.4f" % ref["occluded_share"])
    assert 0.02 <= ref["occluded_share"] <= 0.98
    sums = aov_ref.aov_sums(ao_ref.case_scene(name, opened, w, h), ao_ref.case_params(case), accel=orc.ACCEL_OBVH)
    assert np.array_equal(ref["hits"], sums["hits"])
    assert (ref["unoccluded"] <= ref["hits"] * n_rays).all()


def scene_of(name, opened, w, h):
    return ao_ref.case_scene(name, opened, w, h)


@pytest.mark.parametrize("name", ("cubes", "lowres"))
def test_open_scenes_hold_empty_sparse_and_full_tiles(name):
    w, h = 64, 48
    s = scene_of(name, True, w, h)
    hit, _, _ = ao_ref.vertices(s, pyrt.make_params(w, h, 1, seed=9), accel=orc.ACCEL_OBVH)
    per_tile = hit[:, :, 0].reshape(h // 8, 8, w // 8, 8).sum(axis=(1, 3)).reshape(-1)
    print(name, sorted(per_tile))
    assert (per_tile == 0).any() and ((per_tile >= 1) & (per_tile <= 8)).any() and (per_tile == 64).any()
