"""RayTracer -ao N [-aodist D]: <stem>_ao.ppm is the Python API's ao mean of the same frame (rt_render_ao with the
default bias) after the PPM writer's truncation, the -o image stays the frame byte for byte, and -gpus > 1 refuses the
flag."""
import os
import subprocess

import numpy as np
import pytest

import orc
import pyrt

pytestmark = pytest.mark.gpu

APP = os.path.join(pyrt.ROOT, "ray-tracing-engine_amd", "bin", "RayTracer")
W, H = 48, 32
BASE = ["-scene", "cubes", "-width", str(W), "-height", str(H), "-m", "1", "-N", "4"]


def _run(cwd, extra):
    os.makedirs(cwd, exist_ok=True)
    r = subprocess.run([APP] + BASE + ["-meshdir", pyrt.MESH_DIR, "-o", "frame.ppm"] + extra, cwd=cwd, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return r


def grey(ao):
    return np.repeat(ao[..., None], 3, axis=2).astype(np.float32)


def test_ao_output(tmp_path):
    plain, flag, near = tmp_path / "plain", tmp_path / "flag", tmp_path / "near"
    _run(plain, [])
    _run(flag, ["-ao", "4"])
    _run(near, ["-ao", "4", "-aodist", "0.5"])
    assert (flag / "frame.ppm").read_bytes() == (plain / "frame.ppm").read_bytes()
    assert (near / "frame.ppm").read_bytes() == (plain / "frame.ppm").read_bytes()
    assert not (plain / "frame_ao.ppm").exists()
    ctx = pyrt.Context(pyrt.Scene("cubes", W, H))
    p = pyrt.make_params(W, H, 4, mode=pyrt.MODE_PATH, seed=1)
    far = pyrt.ao_means(ctx.render_ao(p, 4), 4)["ao"]
    assert (flag / "frame_ao.ppm").read_bytes() == orc.ppm_bytes(grey(far))
    lim = pyrt.ao_means(ctx.render_ao(p, 4, max_distance=0.5), 4)["ao"]
    assert (near / "frame_ao.ppm").read_bytes() == orc.ppm_bytes(grey(lim))
    assert (lim >= far).all() and (lim > far).any()  # (a limit only frees rays)
    ctx.close()


def test_flag_refused_with_several_gpus(tmp_path):
    r = subprocess.run([APP] + BASE + ["-meshdir", pyrt.MESH_DIR, "-o", "f.ppm", "-gpus", "2", "-ao", "4"], cwd=tmp_path,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "one GPU" in r.stderr
    assert not (tmp_path / "f.ppm").exists()
