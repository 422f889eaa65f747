"""rt_set_skin / rt_update_skin's C ABI without a GPU: the entry points exist, the ctypes views have the header's layout,
and every check that reads only the arguments answers RT_ERR_INVALID before anything asks for a context or a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pyrt

ROOT = pyrt.ROOT


def test_entry_points_exist():
    for name in ("rt_set_skin", "rt_update_skin"):
        assert hasattr(pyrt.amd(), name) and name in pyrt.AMD_SYMBOLS
    assert pyrt.amd().rt_abi_version() == 2


def test_structs_match_header(tmp_path):
    """sizeof and field offsets of rt_skin / rt_skin_update as the C compiler lays them out."""
    classes = {"rt_skin": pyrt.Skin, "rt_skin_update": pyrt.SkinUpdate}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rt_amd.h"', "int main(void) {",
             '  printf("RT_SKIN_INFLUENCES %d\\n", (int)RT_SKIN_INFLUENCES);']
    for st, cls in classes.items():
        lines.append('  printf("%%s %%zu\\n", "%s", sizeof(%s));' % (st, st))
        for n, _ in cls._fields_:
            lines.append('  printf("%%s.%%s %%zu\\n", "%s", "%s", offsetof(%s, %s));' % (st, n, st, n))
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["RT_SKIN_INFLUENCES"]) == pyrt.SKIN_INFLUENCES == 4
    for st, cls in classes.items():
        assert int(got[st]) == C.sizeof(cls)
        for n, _ in cls._fields_:
            assert int(got["%s.%s" % (st, n)]) == getattr(cls, n).offset, (st, n)
    # the skin update is the transform update with bones for meshes
    assert C.sizeof(pyrt.SkinUpdate) == C.sizeof(pyrt.TransformUpdate)
    for (n, _), (m, _) in zip(pyrt.SkinUpdate._fields_[2:], pyrt.TransformUpdate._fields_[2:]):
        assert n == m and getattr(pyrt.SkinUpdate, n).offset == getattr(pyrt.TransformUpdate, m).offset


# ---- rt_set_skin ----------------------------------------------------------------------------------------------------------
NV = 40


def skin_of(bone, weight, n_bones, n_vertices=None):
    s = pyrt.Skin()
    s.n_vertices, s.n_bones = len(bone) if n_vertices is None else n_vertices, n_bones
    s.bone, s.weight = C.cast(bone.ctypes.data, C.POINTER(C.c_uint16)), C.cast(weight.ctypes.data, C.POINTER(C.c_float))
    return s


def clean_skin(n_bones=7):
    rng = np.random.default_rng(1)
    return rng.integers(0, n_bones, (NV, 4)).astype(np.uint16), rng.uniform(0.1, 0.9, (NV, 4)).astype(np.float32)


def set_skin(s):
    L = pyrt.amd()
    rc = L.rt_set_skin(None, C.byref(s) if s is not None else None)
    return rc, L.rt_last_error().decode()


def test_set_skin_null_arguments():
    bone, weight = clean_skin()
    rc, msg = set_skin(None)
    assert rc == 1 and "null" in msg
    s = skin_of(bone, weight, 7)
    s.bone = None
    rc, msg = set_skin(s)
    assert rc == 1 and "bone/weight is null" in msg
    s = skin_of(bone, weight, 7)
    s.weight = None
    rc, msg = set_skin(s)
    assert rc == 1 and "bone/weight is null" in msg
    # a clean skin gets as far as the null context
    rc, msg = set_skin(skin_of(bone, weight, 7))
    assert rc == 1 and "ctx" in msg and "vertex" not in msg


def test_set_skin_reserved_words_and_bone_count():
    bone, weight = clean_skin()
    for k in range(6):
        s = skin_of(bone, weight, 7)
        s.reserved[k] = 1
        rc, msg = set_skin(s)
        assert rc == 1 and "reserved" in msg
    for n in (0, 65537, 0xffffffff):
        rc, msg = set_skin(skin_of(bone, weight, n))
        assert rc == 1 and "n_bones" in msg and "65536" in msg
    # 65,536 bones are admitted: every uint16 is an index
    bone[5, 2] = 65535
    rc, msg = set_skin(skin_of(bone, weight, 65536))
    assert rc == 1 and "ctx" in msg


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("vertex,slot", [(0, 0), (17, 3), (NV - 1, 1)])
def test_set_skin_non_finite_weight_names_the_vertex(bad, vertex, slot):
    bone, weight = clean_skin()
    weight[vertex, slot] = bad
    rc, msg = set_skin(skin_of(bone, weight, 7))
    assert rc == 1 and "vertex %d:" % vertex in msg and "non-finite" in msg
    # beyond n_vertices it is not read
    rc, msg = set_skin(skin_of(bone, weight, 7, n_vertices=vertex))
    assert rc == 1 and "ctx" in msg


@pytest.mark.parametrize("w", [0.0, -0.0, 0.5])
@pytest.mark.parametrize("vertex,slot", [(0, 0), (17, 3), (NV - 1, 1)])
def test_set_skin_index_names_the_vertex_and_slot(w, vertex, slot):
    """... under a zero weight of either sign too: a skipped slot's index is still validated."""
    bone, weight = clean_skin()
    bone[vertex, slot], weight[vertex, slot] = 7, w
    rc, msg = set_skin(skin_of(bone, weight, 7))
    assert rc == 1 and "vertex %d slot %d" % (vertex, slot) in msg and "index 7" in msg
    rc, msg = set_skin(skin_of(bone, weight, 8))
    assert rc == 1 and "ctx" in msg
    # the first offending vertex is the one named, and within it the weight comes first
    bone[vertex, slot], bone[3, 1], bone[2, 3] = 6, 9, 8
    weight[3, 2] = weight[30, 0] = np.nan
    rc, msg = set_skin(skin_of(bone, weight, 7))
    assert rc == 1 and "vertex 2 slot 3" in msg
    bone[2, 3] = 0
    rc, msg = set_skin(skin_of(bone, weight, 7))
    assert rc == 1 and "vertex 3:" in msg and "non-finite" in msg


# ---- rt_update_skin -------------------------------------------------------------------------------------------------------
def bones_of(n):
    t = pyrt.make_transforms(n)
    t["flags"] = 0
    return t


def update_of(t):
    u = pyrt.SkinUpdate()
    u.bones = C.cast(t.ctypes.data, C.POINTER(pyrt.MeshTransform))
    u.n_bones = len(t)
    return u


def call(u):
    L = pyrt.amd()
    rep = pyrt.UpdateReport()
    rep.refitted = 7
    rc = L.rt_update_skin(None, C.byref(u) if u is not None else None, None, C.byref(rep))
    assert rep.refitted == 0 and rep.photons_dropped == 0 and rep.refit_ms == 0 and rep.total_ms == 0
    return rc, L.rt_last_error().decode()


def test_update_skin_null_arguments():
    assert call(None)[0] == 1 and "null" in call(None)[1]
    rc, msg = call(update_of(bones_of(2)))
    assert rc == 1 and "ctx" in msg and "bone" not in msg
    u = update_of(bones_of(2))
    u.bones = None
    rc, msg = call(u)
    assert rc == 1 and "bones is null" in msg
    assert pyrt.amd().rt_update_skin(None, C.byref(update_of(bones_of(2))), None, None) == 1  # (no report is fine)


@pytest.mark.parametrize("field,where", [("m", (1, 2, 3)), ("m", (1, 0, 0)), ("n", (1, 1, 2))])
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_update_skin_non_finite_entry_names_the_bone(field, where, bad):
    t = bones_of(3)
    t[field][where] = bad
    rc, msg = call(update_of(t))
    assert rc == 1 and "bone 1" in msg and "non-finite" in msg
    u = update_of(t)
    u.n_bones = 1  # (beyond n_bones it is not read)
    rc, msg = call(u)
    assert rc == 1 and "ctx" in msg


def test_update_skin_flags_reserved_words_and_lights():
    for flags in (pyrt.XF_STATIC, 2, 0x80000000):
        t = bones_of(3)
        t["flags"][2] = flags
        rc, msg = call(update_of(t))
        assert rc == 1 and "bone 2" in msg and "flags" in msg
    # flags before the entries of the same bone, bones in order
    t = bones_of(3)
    t["flags"][1], t["m"][1, 0, 0], t["n"][0, 0, 0] = 1, np.nan, np.nan
    rc, msg = call(update_of(t))
    assert rc == 1 and "bone 0" in msg and "non-finite" in msg
    t["n"][0, 0, 0] = 1
    rc, msg = call(update_of(t))
    assert rc == 1 and "bone 1" in msg and "flags" in msg
    t = bones_of(3)
    for k in range(6):
        u = update_of(t)
        u.reserved[k] = 1
        rc, msg = call(u)
        assert rc == 1 and "reserved" in msg
    u = update_of(t)
    u.n_lights = 2
    rc, msg = call(u)
    assert rc == 1 and "lights is null" in msg
