#!/usr/bin/env python3
"""Regenerate the shading-sweep fixtures from the REAL reference (build container only).

Writes the inputs tests/shading_sweep.py draws to a scratch file, runs oracle/_ref/ref_harness `shading` on it (our
driver over the reference's own Material, LightSource and Renderer, see oracle/ref_harness.cpp) and stores what it
answered, as data:

  tests/golden/ref_shading.npz      inputs and outputs (bit patterns) of Material::evaluateColorResponse,
                                    LightSource::evaluateLight and the LightSource constructor's basis
  tests/golden/manifest.json        "shading_*" entries: md5, size, mode, N and the swept materials and lights
                                    (bit patterns) of each small frame
  tests/golden/ppm/shading_*.ppm    those frames (legacy serial RNG, seed 1)

tests/test_oracle_shading.py pins the oracle and the host's LightSource to them, tests/test_gpu_shading.py the device.
Usage:  python tests/golden/make_shading_golden.py
"""
import hashlib
import json
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
HARNESS = os.path.join(ROOT, "oracle", "_ref", "ref_harness")
MESHES = os.path.join(HERE, "meshes")
sys.path.insert(0, os.path.join(ROOT, "tests"))

import shading_sweep as sw  # noqa: E402

# what the fixture holds (tests/test_oracle_shading.py redraws the same and compares)
BSDF_SEED, BSDF_INTERIOR, BSDF_PER_CLASS = 11, 30, 8
LIGHT_SEED, N_LIGHTS, POINTS_PER_LIGHT = 13, 48, 6
# (swept scene, w, h, mode, N)
FRAMES = [(0, 32, 32, 1, 2), (2, 32, 32, 0, 4), (3, 24, 32, 1, 1), (4, 32, 24, 0, 2), (5, 28, 28, 1, 3), (6, 32, 32, 0, 1)]


def frame_name(idx, w, h, mode, n):
    return "shading_s%d_%dx%d_m%d_N%d" % (idx, w, h, mode, n)


def inputs():
    mats, mcls = sw.materials(BSDF_SEED, BSDF_INTERIOR)
    tri, dcls = sw.directions(BSDF_SEED + 1, BSDF_PER_CLASS)
    rows, rm, rd = sw.bsdf_rows(mats, mcls, tri, dcls)
    specs, att, ori = sw.light_specs(LIGHT_SEED, N_LIGHTS)
    li, pts = sw.eval_points(LIGHT_SEED + 1, specs, POINTS_PER_LIGHT)
    scene_lights = np.concatenate([sw.scene_spec(i)[1] for i in range(sw.N_SCENES)])
    basis_in = np.concatenate([specs[:, [0, 1, 2, 6, 7, 8]], scene_lights[:, [0, 1, 2, 6, 7, 8]]])
    return dict(bsdf_rows=rows, bsdf_mat_cls=rm, bsdf_dir_cls=rd, light_specs=specs, light_att_cls=att, light_ori_cls=ori,
                eval_light=li, eval_points=pts, basis_in=np.ascontiguousarray(basis_in, np.float32))


def save_npz(path, arrays):
    """np.savez_compressed with fixed member dates, so that a regenerated fixture is the same file byte for byte."""
    import io
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(zi, buf.getvalue())


def main():
    if not os.path.exists(HARNESS):
        sys.exit("oracle/_ref/ref_harness is missing: it is built only where the reference sources exist")
    d = inputs()
    ev = np.concatenate([d["light_specs"][d["eval_light"]], d["eval_points"]], 1).astype(np.float32)
    man_path = os.path.join(HERE, "manifest.json")
    manifest = json.load(open(man_path))
    os.makedirs(os.path.join(HERE, "ppm"), exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        src, out = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.json")
        with open(src, "wb") as f:
            f.write(struct.pack("<8I", 0x44414853, len(d["bsdf_rows"]), len(ev), len(d["basis_in"]), len(FRAMES), 0, 0, 0))
            f.write(d["bsdf_rows"].astype("<f4").tobytes())
            f.write(ev.astype("<f4").tobytes())
            f.write(d["basis_in"].astype("<f4").tobytes())
            for idx, w, h, mode, n in FRAMES:
                mats, specs = sw.scene_spec(idx)
                f.write(struct.pack("<6I", w, h, mode, n, len(specs), 0))
                f.write(mats.astype("<f4").tobytes())
                f.write(specs.astype("<f4").tobytes())
        # (the reference's Renderer writes update.ppm into its working directory every pass)
        subprocess.run([HARNESS, "shading", MESHES, src, out, os.path.join(tmp, "frame")], cwd=tmp, check=True,
                       capture_output=True, timeout=1800)
        res = json.load(open(out))
        d["bsdf_out"] = np.array(res["bsdf"], np.uint32).reshape(-1, 3)
        d["eval_out"] = np.array(res["evaluateLight"], np.uint32).reshape(-1, 3)
        d["basis_out"] = np.array(res["basis"], np.uint32).reshape(-1, 9)
        assert len(d["bsdf_out"]) == len(d["bsdf_rows"]) and len(d["eval_out"]) == len(ev) and len(d["basis_out"]) == len(d["basis_in"])
        for i, (idx, w, h, mode, n) in enumerate(FRAMES):
            name = frame_name(idx, w, h, mode, n)
            data = open(os.path.join(tmp, "frame%d.ppm" % i), "rb").read()
            mats, specs = sw.scene_spec(idx)
            manifest[name] = dict(scene="cubes", sweep=idx, w=w, h=h, mode=mode, N=n, p=0, k=0,
                                  md5=hashlib.md5(data).hexdigest(), ppm="ppm/%s.ppm" % name,
                                  materials=mats.view(np.uint32).ravel().tolist(), lights=specs.view(np.uint32).ravel().tolist())
            with open(os.path.join(HERE, manifest[name]["ppm"]), "wb") as f:
                f.write(data)
            print(name, manifest[name]["md5"], flush=True)
    # inputs as bit patterns too: the fixture stands on its own
    for k in ("bsdf_rows", "light_specs", "eval_points", "basis_in"):
        d[k] = np.ascontiguousarray(d[k], np.float32).view(np.uint32)
    npz = os.path.join(HERE, "ref_shading.npz")
    save_npz(npz, d)
    print("ref_shading.npz", os.path.getsize(npz), "bytes;", len(d["bsdf_rows"]), "bsdf rows,", len(ev), "light rows,",
          len(d["basis_in"]), "bases")
    json.dump(manifest, open(man_path, "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
