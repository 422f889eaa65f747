"""RayTracer -textures 1 -normalmaps 1 on the committed STOFF cube (tests/golden/meshes/cube_st.off with cube_st.ppm and
cube_st_n.ppm beside it): the -o image is the Python API's rt_render_normal_mapped frame of the same scene — the images
bilinear and repeating on the cube, RT_TEX_NONE in every table on every other mesh — after the PPM writer's truncation,
without -matmaps 1 (no material maps resident) and with it; it is neither the textured nor the material frame; without
the flag nothing changes; and the flag is refused, by its own check, without -textures 1 and with the flags -textures does
not compose with."""
import os

import numpy as np
import pytest

import orc
import pyrt
from test_gpu_app_tex import CUBE, H, W, _run, p3_texels, stoff_uvs

pytestmark = pytest.mark.gpu


def normal_mapped_context(matmaps):
    """A context of the cube's scene with the set and the maps -textures 1 -normalmaps 1 (and -matmaps 1) give it, in the
    order the application loads the images, and the frame's parameters."""
    scene = pyrt.Scene("file:" + CUBE, W, H)
    a = scene.arrays()
    nm = len(a["tri_begin"]) - 1
    uv = np.zeros((len(a["pos"]), 2), np.float32)
    cube = stoff_uvs(os.path.join(pyrt.MESH_DIR, CUBE))
    v0 = int(a["vtx_begin"][3])  # (the preset's fourth mesh is the file's)
    assert int(a["vtx_begin"][4]) - v0 == len(cube) == 8
    uv[v0:v0 + 8] = cube
    names = ["cube_st.ppm"] + (["cube_st_f0.ppm", "cube_st_kda.ppm"] if matmaps else []) + ["cube_st_n.ppm"]
    tables = {n: np.full(nm, pyrt.TEX_NONE, np.uint32) for n in ("cube_st.ppm", "cube_st_f0.ppm", "cube_st_kda.ppm", "cube_st_n.ppm")}
    textures = []
    for k, name in enumerate(names):
        textures.append((p3_texels(os.path.join(pyrt.MESH_DIR, name)), pyrt.TEX_REPEAT, pyrt.TEX_REPEAT, pyrt.TEX_BILINEAR))
        tables[name][3] = k
    assert textures[-1][0].shape == (3, 3, 3) and textures[-1][0][..., 2].min() > 0.5
    ctx = pyrt.Context(scene)
    ctx.set_textures(textures, tables["cube_st.ppm"], uv)
    if matmaps:
        ctx.set_material_maps(tables["cube_st_f0.ppm"], tables["cube_st_kda.ppm"])
    ctx.set_normal_maps(tables["cube_st_n.ppm"])
    return ctx, pyrt.make_params(W, H, 4, mode=pyrt.MODE_PATH, seed=1)


def test_normal_mapped_frame(tmp_path):
    tex, mat, nrm, both = (tmp_path / n for n in ("tex", "mat", "nrm", "both"))
    for cwd, extra in ((tex, ["-textures", "1"]), (mat, ["-textures", "1", "-matmaps", "1"]), (nrm, ["-textures", "1", "-normalmaps", "1"]),
                       (both, ["-textures", "1", "-matmaps", "1", "-normalmaps", "1"])):
        r = _run(cwd, extra)
        assert r.returncode == 0, r.stdout + r.stderr
        assert ("Normal maps: 1 images" in r.stdout) == ("-normalmaps" in extra) and "textures of 1 of" in r.stdout
    assert "Material maps: 2 images" in r.stdout
    frames = {}
    for name, matmaps in (("nrm", False), ("both", True)):
        ctx, p = normal_mapped_context(matmaps)
        frames[name], _, _ = ctx.render_normal_mapped(p, bg=pyrt.background(W, H))
        ctx.close()
    assert (nrm / "frame.ppm").read_bytes() == orc.ppm_bytes(frames["nrm"])
    assert (both / "frame.ppm").read_bytes() == orc.ppm_bytes(frames["both"])
    images = [(d / "frame.ppm").read_bytes() for d in (tex, mat, nrm, both)]
    assert len(set(images)) == 4
    assert (nrm / "update.ppm").read_bytes() == (nrm / "frame.ppm").read_bytes()


def test_a_scene_without_textured_meshes_renders_as_it_did(tmp_path):
    plain, nrm = tmp_path / "plain", tmp_path / "nrm"
    for cwd, extra in ((plain, []), (nrm, ["-textures", "1", "-normalmaps", "1"])):
        r = _run(cwd, extra, scene="cubes")
        assert r.returncode == 0, r.stdout + r.stderr
    assert "Normal maps" not in r.stdout
    assert (nrm / "frame.ppm").read_bytes() == (plain / "frame.ppm").read_bytes()


def test_normalmaps_needs_textures(tmp_path):
    r = _run(tmp_path, ["-normalmaps", "1"])
    assert r.returncode != 0 and "error: -normalmaps needs -textures 1" in r.stderr, r.stdout + r.stderr
    assert "USAGE" not in r.stderr and not (tmp_path / "frame.ppm").exists()


@pytest.mark.parametrize("extra,word", [(["-p", "1000"], "without -p"), (["-lights", "each"], "-lights"), (["-lightpick", "2"], "-lightpick"),
                                        (["-aperture", "0.3", "-focus", "2"], "-aperture"), (["-shutter", "0.1,0,0"], "-shutter"),
                                        (["-adaptive", "0.01"], "-adaptive"), (["-vcolors", "1"], "-vcolors"), (["-gpus", "2"], "one GPU")])
def test_flag_refused(tmp_path, extra, word):
    r = _run(tmp_path, ["-textures", "1", "-normalmaps", "1"] + extra)
    # (the check's own message: an unknown flag would exit non-zero too, with a usage text that names every flag)
    assert r.returncode != 0 and "error: -normalmaps runs on one GPU, without" in r.stderr and word in r.stderr, r.stdout + r.stderr
    assert "USAGE" not in r.stderr
    assert not (tmp_path / "frame.ppm").exists()
