"""The RayTracer application's -lights flag: the per-group files <output stem>_g<k>.ppm are, byte for byte, the PPMs of
the frames the Python API's render_lights returns for the same scene, size, samples and seed; the frame itself stays
the frame; and the flag is refused where the call is (-p, -gpus > 1, -adaptive, -shutter, -aperture, more than four
groups, a mask that is no number)."""
import os
import subprocess

import pytest

import orc
import pyrt

pytestmark = pytest.mark.gpu

APP = os.path.join(pyrt.ROOT, "ray-tracing-engine_amd", "bin", "RayTracer")


def run(tmp_path, args):
    return subprocess.run([APP] + args + ["-meshdir", pyrt.MESH_DIR], cwd=tmp_path, capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("kind,w,h,spp,mode,flag,masks", [
    ("cubes", 40, 32, 4, 1, "each", (1, 2, 4)),
    ("lowres", 33, 24, 3, 0, "3,0x6,0,7", (3, 6, 0, 7)),
])
def test_group_files_match_the_python_api(tmp_path, kind, w, h, spp, mode, flag, masks):
    out = tmp_path / "o.ppm"
    r = run(tmp_path, ["-width", str(w), "-height", str(h), "-m", str(mode), "-N", str(spp), "-scene", kind, "-lights", flag, "-o", str(out)])
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Light groups: %d frames from one launch" % len(masks) in r.stdout
    ctx = pyrt.Context(pyrt.Scene(kind, w, h))
    try:
        bg = pyrt.background(w, h)
        p = pyrt.make_params(w, h, spp, mode=mode, seed=1)
        frames, _, _ = ctx.render_lights(p, masks, bg=bg)
        whole, _, _ = ctx.render(p, bg)
    finally:
        ctx.close()
    for k in range(len(masks)):
        assert (tmp_path / ("o_g%d.ppm" % k)).read_bytes() == orc.ppm_bytes(frames[k]), k
    assert not (tmp_path / ("o_g%d.ppm" % len(masks))).exists()
    assert out.read_bytes() == orc.ppm_bytes(whole)
    files = {k: (tmp_path / ("o_g%d.ppm" % k)).read_bytes() for k in range(len(masks))}
    assert len({files[k] for k in range(len(masks))}) == len(set(masks))  # (different masks, different pictures)


def test_the_flag_is_refused_where_the_call_is(tmp_path):
    base = ["-width", "16", "-height", "16", "-N", "1"]
    for extra, word in ((["-lights", "each", "-p", "100"], "-lights runs on one GPU"), (["-lights", "1,2", "-gpus", "2"], "-lights runs on one GPU"),
                        (["-lights", "each", "-adaptive", "0.1", "-pass", "1"], "-lights runs on one GPU"),
                        (["-lights", "each", "-shutter", "0.1,0,0"], "-lights runs on one GPU"),
                        (["-lights", "1", "-aperture", "0.1", "-focus", "2"], "-lights runs on one GPU"),
                        (["-lights", "1,2,4,3,5"], "at most 4 groups"), (["-lights", "1,x"], "-lights must be"), (["-lights", "1,,2"], "-lights must be"),
                        (["-lights", "-1"], "-lights must be"), (["-lights", "4294967296"], "-lights must be"), (["-lights", "all"], "-lights must be")):
        r = run(tmp_path, base + extra)
        assert r.returncode == 1 and word in r.stderr, (extra, r.stderr)
        assert not (tmp_path / "output_g0.ppm").exists(), extra
    # a mask beyond the scene's three lights: the library's own rejection, after the frame
    r = run(tmp_path, base + ["-lights", "8"])
    assert r.returncode == 1 and "n_lights 3" in r.stderr, r.stderr
