"""Reference -> oracle over the swept shading space (tests/shading_sweep.py): tests/golden/ref_shading.npz and the
"shading_*" entries of tests/golden/manifest.json hold what the reference's own Material::evaluateColorResponse,
LightSource::evaluateLight, LightSource constructor and Renderer answered (tests/golden/make_shading_golden.py).
The oracle's restatement in libm mode, and the product's host LightSource, must reproduce them.

Comparison rule (shading_sweep.assert_same_bits): 32-bit patterns, no row left out; an expected NaN must be met by a
NaN, everything else — +-0 and +-inf included — bit for bit."""
import hashlib
import os
import sys

import numpy as np
import pytest

import orc
import pyrt
import shading_sweep as sw

sys.path.insert(0, os.path.join(pyrt.ROOT, "tests", "golden"))
import make_shading_golden as gold  # noqa: E402  (the draw parameters of the fixture)


@pytest.fixture(scope="module")
def ref():
    d = dict(np.load(os.path.join(pyrt.ROOT, "tests", "golden", "ref_shading.npz")))
    for k in ("bsdf_rows", "light_specs", "eval_points", "basis_in", "bsdf_out", "eval_out", "basis_out"):
        d[k] = d[k].view(np.float32)
    return d


def test_generator_is_deterministic_and_is_what_the_fixture_holds(ref):
    """The sweep redrawn today gives the rows the reference was asked about, bit for bit, and every class is there."""
    d = gold.inputs()
    for k in ("bsdf_rows", "light_specs", "eval_points", "basis_in"):
        assert np.array_equal(d[k].view(np.uint32), ref[k].view(np.uint32)), k
    for k in ("bsdf_mat_cls", "bsdf_dir_cls", "light_att_cls", "light_ori_cls", "eval_light"):
        assert np.array_equal(d[k], ref[k]), k
    assert set(ref["bsdf_mat_cls"]) == set(range(len(sw.MATERIAL_CLASSES)))
    assert set(ref["bsdf_dir_cls"]) == set(range(len(sw.DIRECTION_CLASSES)))
    assert set(ref["light_att_cls"]) == set(range(len(sw.ATTENUATION_CLASSES)))
    assert set(ref["light_ori_cls"]) == set(range(len(sw.ORIENTATION_CLASSES)))
    assert len(ref["bsdf_rows"]) >= 3000
    kd = ref["bsdf_rows"][:, 0]
    assert (kd == np.float32(np.pi)).any() and (ref["bsdf_rows"][:, 1] == 0).any() and (ref["bsdf_rows"][:, 1] > 1).any()


def test_regular_rows_are_finite_in_the_reference(ref):
    """Every regular direction class with every material of alpha >= 1e-4 is finite in the reference's own output
    (there the comparison rule is plain bit equality); the degenerate classes do produce NaNs and infinities."""
    must = sw.must_be_finite(ref["bsdf_rows"], ref["bsdf_dir_cls"])
    assert must.sum() >= 700
    assert np.isfinite(ref["bsdf_out"][must]).all()
    assert np.isnan(ref["bsdf_out"]).any(1).sum() > 100  # (the NaN rule is exercised)


def test_oracle_bsdf_reproduces_the_reference(ref):
    got = orc.bsdf_rows(ref["bsdf_rows"], orc.MATH_LIBM)
    sw.assert_same_bits(got, ref["bsdf_out"], "orc_bsdf (libm)")
    must = sw.must_be_finite(ref["bsdf_rows"], ref["bsdf_dir_cls"])
    assert np.array_equal(got[must].view(np.uint32), ref["bsdf_out"][must].view(np.uint32))


def test_oracle_bsdf_det_mode_on_the_reference_rows(ref):
    """The deterministic math mode (x * x and (x * x) * (x * x) * x for pow: what the device evaluates) gives the
    reference's bits on the same rows: both pows are within an ulp of libm's in double, which the narrowing to float
    hides but for one case in ~1e8 (tests/test_gpu_parity.py test_bsdf_golden)."""
    sw.assert_same_bits(orc.bsdf_rows(ref["bsdf_rows"], orc.MATH_DET), ref["bsdf_out"], "orc_bsdf (det)")


def _eval_rows(ref, basis):
    lights = sw.light_rows(ref["light_specs"], basis)
    return np.concatenate([lights[ref["eval_light"]], ref["eval_points"]], 1)


def test_oracle_eval_light_reproduces_the_reference(ref):
    n = len(ref["light_specs"])
    rows = _eval_rows(ref, ref["basis_out"][:n])
    sw.assert_same_bits(orc.eval_light_rows(rows), ref["eval_out"], "orc_eval_light")
    # the sweep reaches d = 0 and vanishing attenuation: infinities and NaNs are in the reference's answers
    assert np.isinf(ref["eval_out"]).any() and np.isnan(ref["eval_out"]).any()
    fin = np.isfinite(ref["eval_out"]).all(1)
    assert fin.mean() > 0.8


def test_host_light_constructor_reproduces_the_reference_basis(ref):
    """The product's host/LightSource.h derives the square's basis itself (rt_light's is "computed by the host"):
    the swept orientations — axis-aligned ones, whose basis collapses along x, and direction == position included."""
    got = pyrt.light_basis(ref["basis_in"][:, 0:3], ref["basis_in"][:, 3:6])
    sw.assert_same_bits(got, ref["basis_out"], "LightSource basis")
    null = (ref["basis_out"][:, 0:6] == 0).all(1)
    assert null.any() and not null.all()


SHADING_FRAMES = [gold.frame_name(*f) for f in gold.FRAMES]


def _golden_scene(e):
    """The scene of a "shading_*" manifest entry from the bit patterns it records (not from the generator)."""
    mats = np.array(e["materials"], np.uint32).view(np.float32).reshape(5, 8)
    specs = np.array(e["lights"], np.uint32).view(np.float32).reshape(-1, 16)
    a = pyrt.Scene(e["scene"], e["w"], e["h"]).arrays()
    lights = sw.light_rows(specs, pyrt.light_basis(specs[:, 0:3], specs[:, 6:9]))
    return pyrt.ArrayScene(a["pos"], a["nrm"], a["tri"], a["tri_begin"], a["vtx_begin"], mats, lights, a["camera"]), mats, specs


@pytest.mark.parametrize("name", SHADING_FRAMES)
def test_legacy_mode_reproduces_reference_frames_of_swept_scenes(golden, name):
    e = golden["manifest"][name]
    scene, mats, specs = _golden_scene(e)
    gm, gs = sw.scene_spec(e["sweep"])
    assert np.array_equal(gm.view(np.uint32), mats.view(np.uint32)) and np.array_equal(gs.view(np.uint32), specs.view(np.uint32))
    p = pyrt.make_params(e["w"], e["h"], e["N"], mode=e["mode"], rng_mode=pyrt.RNG_LEGACY)
    out, _, _ = orc.render(scene, p, math_mode=orc.MATH_LIBM, bg=pyrt.background(e["w"], e["h"]))
    data = orc.ppm_bytes(out)
    assert data == open(os.path.join(golden["dir"], e["ppm"]), "rb").read()
    assert hashlib.md5(data).hexdigest() == e["md5"]


def test_frames_cover_both_modes_and_sizes():
    assert len(gold.FRAMES) >= 6 and {f[3] for f in gold.FRAMES} == {0, 1}
    assert all(w <= 32 and h <= 32 and n <= 4 for _, w, h, _, n in gold.FRAMES)
