"""RayTracer -textures 1 -matmaps 1 on the committed STOFF cube (tests/golden/meshes/cube_st.off with cube_st.ppm,
cube_st_f0.ppm and cube_st_kda.ppm beside it): the -o image is the Python API's rt_render_material frame of the same scene
— the three images bilinear and repeating on the cube, RT_TEX_NONE in all three tables on every other mesh — after the
PPM writer's truncation; it is neither the textured nor the plain frame; without the flag nothing changes; and the flag
is refused, by its own check, without -textures 1 and with the flags -textures does not compose with."""
import os

import numpy as np
import pytest

import orc
import pyrt
from test_gpu_app_tex import CUBE, H, W, _run, p3_texels, stoff_uvs

pytestmark = pytest.mark.gpu


def material_context():
    """A context of the cube's scene with the set and the maps -textures 1 -matmaps 1 give it, and the frame's parameters."""
    scene = pyrt.Scene("file:" + CUBE, W, H)
    a = scene.arrays()
    nm = len(a["tri_begin"]) - 1
    uv = np.zeros((len(a["pos"]), 2), np.float32)
    cube = stoff_uvs(os.path.join(pyrt.MESH_DIR, CUBE))
    v0 = int(a["vtx_begin"][3])  # (the preset's fourth mesh is the file's)
    assert int(a["vtx_begin"][4]) - v0 == len(cube) == 8
    uv[v0:v0 + 8] = cube
    tables = [np.full(nm, pyrt.TEX_NONE, np.uint32) for _ in range(3)]
    textures = []
    for k, (name, shape) in enumerate((("cube_st.ppm", (3, 4, 3)), ("cube_st_f0.ppm", (2, 2, 3)), ("cube_st_kda.ppm", (2, 3, 3)))):
        texels = p3_texels(os.path.join(pyrt.MESH_DIR, name))
        assert texels.shape == shape
        textures.append((texels, pyrt.TEX_REPEAT, pyrt.TEX_REPEAT, pyrt.TEX_BILINEAR))
        tables[k][3] = k
    assert textures[2][0][..., 1].min() > 0  # (no alpha of 0 in the fixture)
    ctx = pyrt.Context(scene)
    ctx.set_textures(textures, tables[0], uv)
    ctx.set_material_maps(tables[1], tables[2])
    return ctx, pyrt.make_params(W, H, 4, mode=pyrt.MODE_PATH, seed=1)


def test_material_frame(tmp_path):
    plain, tex, mat = tmp_path / "plain", tmp_path / "tex", tmp_path / "mat"
    for cwd, extra in ((plain, []), (tex, ["-textures", "1"]), (mat, ["-textures", "1", "-matmaps", "1"])):
        r = _run(cwd, extra)
        assert r.returncode == 0, r.stdout + r.stderr
    assert "textures of 1 of" in r.stdout and "Material maps: 2 images" in r.stdout
    ctx, p = material_context()
    out, _, _ = ctx.render_material(p, bg=pyrt.background(W, H))
    tout, _, _ = ctx.render_textured(p, bg=pyrt.background(W, H))
    ctx.close()
    assert (mat / "frame.ppm").read_bytes() == orc.ppm_bytes(out)
    assert (tex / "frame.ppm").read_bytes() == orc.ppm_bytes(tout)  # (the maps' textures in the set change nothing there)
    assert (mat / "frame.ppm").read_bytes() != (tex / "frame.ppm").read_bytes() != (plain / "frame.ppm").read_bytes()
    assert (mat / "frame.ppm").read_bytes() != (plain / "frame.ppm").read_bytes()
    assert (mat / "update.ppm").read_bytes() == (mat / "frame.ppm").read_bytes()


def test_a_scene_without_textured_meshes_renders_as_it_did(tmp_path):
    plain, mat = tmp_path / "plain", tmp_path / "mat"
    for cwd, extra in ((plain, []), (mat, ["-textures", "1", "-matmaps", "1"])):
        r = _run(cwd, extra, scene="cubes")
        assert r.returncode == 0, r.stdout + r.stderr
    assert "Material maps" not in r.stdout
    assert (mat / "frame.ppm").read_bytes() == (plain / "frame.ppm").read_bytes()


def test_matmaps_needs_textures(tmp_path):
    r = _run(tmp_path, ["-matmaps", "1"])
    assert r.returncode != 0 and "error: -matmaps needs -textures 1" in r.stderr, r.stdout + r.stderr
    assert "USAGE" not in r.stderr and not (tmp_path / "frame.ppm").exists()


@pytest.mark.parametrize("extra,word", [(["-p", "1000"], "without -p"), (["-lights", "each"], "-lights"), (["-lightpick", "2"], "-lightpick"),
                                        (["-aperture", "0.3", "-focus", "2"], "-aperture"), (["-shutter", "0.1,0,0"], "-shutter"),
                                        (["-adaptive", "0.01"], "-adaptive"), (["-vcolors", "1"], "-vcolors"), (["-gpus", "2"], "one GPU")])
def test_flag_refused(tmp_path, extra, word):
    r = _run(tmp_path, ["-textures", "1", "-matmaps", "1"] + extra)
    # (the check's own message: an unknown flag would exit non-zero too, with a usage text that names every flag)
    assert r.returncode != 0 and "error: -matmaps runs on one GPU, without" in r.stderr and word in r.stderr, r.stdout + r.stderr
    assert "USAGE" not in r.stderr
    assert not (tmp_path / "frame.ppm").exists()
