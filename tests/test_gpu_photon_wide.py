"""Photon-map frames with 17 <= k <= 256 (k_render_wide: the wide k-heap) against the oracle's frames,
accumulator and image bit for bit: ray and path mode on two scenes, maps whose k results tie exactly,
the 16-bit / 32-bit boundary, brute force, both the timed and the counting instance; then the same frame
split over ranks, over a group and over sample ranges, and the applications' -k above 16."""
import os
import subprocess

import numpy as np
import pytest

import orc
import pyrt
from pyrt import dist as rdist
from test_gpu_app import APP, DROPIN, _expected

pytestmark = pytest.mark.gpu

KS = (17, 32, 64, 128, 256)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _map(kind, nreq, seed, n=None, doubled=False):
    """An emitted photon map in kdtree order as [n][7] (first n photons; doubled: every position twice, the
    copy carrying another photon's direction, so a query's k results tie exactly)."""
    c = pyrt.Context(pyrt.Scene(kind, 16, 16))
    pos, dir_, w = c.emit_photons(nreq, seed=seed)
    c.close()
    if n is not None:
        assert len(pos) >= n
        pos, dir_, w = pos[:n], dir_[:n], w[:n]
    if doubled:
        other = np.roll(np.arange(len(pos)), 7)
        pos, dir_, w = np.concatenate([pos, pos]), np.concatenate([dir_, dir_[other]]), np.concatenate([w, w])
    kp, kd_, kw = pyrt.kd_order(pos, dir_, w)
    return np.concatenate([kp, kd_, kw[:, None]], 1)


def _frame(kind, mode, k, ph7, nreq, w=32, h=24, spp=2, stats=1, accel=pyrt.ACCEL_BVH):
    s = pyrt.Scene(kind, w, h)
    c = pyrt.Context(s)
    c.set_photons(ph7[:, 0:3], ph7[:, 3:6])
    bg = pyrt.background(w, h)
    p = pyrt.make_params(w, h, spp, mode=mode, seed=5, use_photons=1, k=k, photons_requested=nreq, collect_stats=stats,
                         accel=accel)
    out, acc, st = c.render(p, bg)
    c.close()
    ref_out, ref_acc, ref_st = orc.render(s, p, math_mode=orc.MATH_DET, bg=bg, ext_photons=ph7)
    tag = (kind, mode, k, len(ph7), stats, accel)
    assert np.array_equal(bits(acc), bits(ref_acc)), tag
    assert np.array_equal(bits(out), bits(ref_out)), tag
    assert st.knn_queries == ref_st.knn_queries, tag
    if stats:
        assert 0 < st.kd_visited <= ref_st.kd_visited, tag
    return acc


@pytest.mark.parametrize("kind,nreq", [("cubes", 3000), ("lowres", 2000)])
@pytest.mark.parametrize("mode", [pyrt.MODE_RAY, pyrt.MODE_PATH])
def test_wide_k_frames_equal_oracle(kind, nreq, mode):
    ph7 = _map(kind, nreq, seed=2)
    for k in KS:
        _frame(kind, mode, k, ph7, nreq, stats=1)
        _frame(kind, mode, k, ph7, nreq, stats=0)


@pytest.mark.parametrize("mode", [pyrt.MODE_RAY, pyrt.MODE_PATH])
def test_wide_k_frames_with_tied_results(mode):
    ph7 = _map("cubes", 4000, seed=3, doubled=True)
    for k in (17, 64, 256):
        _frame("cubes", mode, k, ph7, 4000)


@pytest.mark.parametrize("n", [65534, 65535])
def test_wide_k_frames_across_the_16_bit_boundary(n):
    """65,534 photons: 16-bit stack entries and heap indices; 65,535: 32-bit."""
    ph7 = _map("cubes", 140000, seed=4, n=n)
    for stats in (0, 1):
        _frame("cubes", pyrt.MODE_RAY, 64, ph7, n, stats=stats)


def test_wide_k_brute_force():
    ph7 = _map("cubes", 3000, seed=6)
    for stats in (0, 1):
        _frame("cubes", pyrt.MODE_PATH, 32, ph7, 3000, stats=stats, accel=pyrt.ACCEL_BRUTE)


@pytest.fixture(scope="module")
def big():
    """256 x 256 x 4, 50,000 photons requested, k = 64: the frame, its map and the one-rank accumulator."""
    w = h = 256
    ph7 = _map("cubes", 50000, seed=1)
    acc = _frame("cubes", pyrt.MODE_PATH, 64, ph7, 50000, w=w, h=h, spp=4, stats=0)
    return ph7, acc


def _params(w, h, **kw):
    return pyrt.make_params(w, h, 4, mode=pyrt.MODE_PATH, seed=5, use_photons=1, k=64, photons_requested=50000, **kw)


def test_wide_k_big_frame_over_ranks_group_and_passes(big):
    ph7, full = big
    w = h = 256
    s = pyrt.Scene("cubes", w, h)
    c = pyrt.Context(s)
    c.set_photons(ph7[:, 0:3], ph7[:, 3:6])
    for world in (2, 3):
        total = np.zeros((h, w, 4), np.float32)
        for r in range(world):
            _, part, st = c.render(_params(w, h, rank=r, world=world))
            owned = rdist.owned_granule_index(w, h, r, world, 8).reshape(-1) >= 0
            assert st.samples == owned.sum() * 4
            total += part  # adding zeros is exact
        assert np.array_equal(bits(total), bits(full)), world
    # two sample ranges on top of each other = one call
    bg = pyrt.background(w, h)
    acc = np.zeros((h, w, 4), np.float32)
    c.render_passes(_params(w, h, spp_begin=0, spp_count=1), bg, acc)
    out, _ = c.render_passes(_params(w, h, spp_begin=1, spp_count=3), bg, acc)
    assert np.array_equal(bits(acc), bits(full))
    ref_out, _, _ = c.render(_params(w, h), bg, want_accum=False)
    assert np.array_equal(bits(out), bits(ref_out))
    c.close()
    g = pyrt.Group(s, [0, 0])
    g.set_photons(ph7[:, 0:3], ph7[:, 3:6])
    _, gacc, _ = g.render(_params(w, h), bg)
    g.close()
    assert np.array_equal(bits(gacc), bits(full))


def test_application_k_40(tmp_path):
    out = tmp_path / "o.ppm"
    args = ["-width", "48", "-height", "40", "-m", "0", "-N", "2", "-p", "3000", "-k", "40"]
    r = subprocess.run([APP] + args + ["-meshdir", pyrt.MESH_DIR, "-o", str(out)], cwd=tmp_path, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert out.read_bytes() == _expected("cubes", 48, 40, 2, 0, 3000, 40)
    # above the cap the library's message names it
    r = subprocess.run([APP] + args[:-1] + ["257", "-meshdir", pyrt.MESH_DIR, "-o", str(out)], cwd=tmp_path,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "1..256" in r.stdout + r.stderr


@pytest.mark.skipif(not os.path.exists(DROPIN), reason="oracle/_ref/RayTracer_dropin is built only where /root/reference exists")
def test_reference_main_unchanged_k_40(tmp_path):
    (tmp_path / "build").mkdir()
    os.symlink(pyrt.MESH_DIR, tmp_path / "meshes")
    r = subprocess.run([DROPIN, "-width", "48", "-height", "40", "-m", "0", "-N", "2", "-p", "5000", "-k", "40"],
                       cwd=tmp_path / "build", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert (tmp_path / "build" / "output.ppm").read_bytes() == _expected("cubes", 48, 40, 2, 0, 5000, 40)
