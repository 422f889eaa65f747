"""rt_update_transforms' C ABI without a GPU: the entry point exists, the ctypes and numpy views have the header's
layout, and every check that reads only the update answers RT_ERR_INVALID before anything asks for a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pyrt

ROOT = pyrt.ROOT


def test_entry_point_exists():
    assert hasattr(pyrt.amd(), "rt_update_transforms") and "rt_update_transforms" in pyrt.AMD_SYMBOLS
    assert pyrt.amd().rt_abi_version() == 2


def test_structs_match_header(tmp_path):
    """sizeof and field offsets of rt_mesh_transform / rt_transform_update as the C compiler lays them out; the numpy
    record of make_transforms is the same 88 bytes."""
    classes = {"rt_mesh_transform": pyrt.MeshTransform, "rt_transform_update": pyrt.TransformUpdate}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rt_amd.h"', "int main(void) {",
             '  printf("RT_XF_STATIC %d\\n", (int)RT_XF_STATIC);']
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
    assert int(got["RT_XF_STATIC"]) == pyrt.XF_STATIC == 1
    for st, cls in classes.items():
        assert int(got[st]) == C.sizeof(cls)
        for n, _ in cls._fields_:
            assert int(got["%s.%s" % (st, n)]) == getattr(cls, n).offset, (st, n)
    assert C.sizeof(pyrt.MeshTransform) == pyrt.TRANSFORM_DTYPE.itemsize == 88
    for n in ("m", "n", "flags"):
        assert pyrt.TRANSFORM_DTYPE.fields[n][1] == getattr(pyrt.MeshTransform, n).offset


def test_make_transforms_is_all_static_identity():
    t = pyrt.make_transforms(3)
    assert t.shape == (3,) and (t["flags"] == pyrt.XF_STATIC).all()
    assert np.array_equal(t["m"][1], np.eye(3, 4, dtype=np.float32)) and np.array_equal(t["n"][2], np.eye(3, dtype=np.float32))


def update_of(t):
    u = pyrt.TransformUpdate()
    u.transforms = C.cast(t.ctypes.data, C.POINTER(pyrt.MeshTransform))
    u.n_meshes = len(t)
    return u


def call(ctx, u):
    L = pyrt.amd()
    rep = pyrt.UpdateReport()
    rep.refitted = 7
    rc = L.rt_update_transforms(ctx, C.byref(u) if u is not None else None, None, C.byref(rep))
    assert rep.refitted == 0
    return rc, L.rt_last_error().decode()


def test_null_arguments():
    t = pyrt.make_transforms(2)
    assert call(None, None)[0] == 1
    rc, msg = call(None, update_of(t))
    assert rc == 1 and "null" in msg
    u = update_of(t)
    u.transforms = None
    rc, msg = call(None, u)
    assert rc == 1 and "transforms is null" in msg


@pytest.mark.parametrize("field,where", [("m", (1, 2, 3)), ("m", (1, 0, 0)), ("n", (1, 1, 2))])
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_entry_names_the_mesh(field, where, bad):
    t = pyrt.make_transforms(3)
    t["flags"][1] = 0
    t[field][where] = bad
    rc, msg = call(None, update_of(t))
    assert rc == 1 and "mesh 1" in msg and "non-finite" in msg
    # the same entry in a static mesh is not read: the call gets as far as the null context
    t["flags"][1] = pyrt.XF_STATIC
    rc, msg = call(None, update_of(t))
    assert rc == 1 and "mesh" not in msg and "null" in msg


def test_unknown_flags_reserved_words_and_lights():
    t = pyrt.make_transforms(3)
    t["flags"][2] = 2
    rc, msg = call(None, update_of(t))
    assert rc == 1 and "mesh 2" in msg and "flags" in msg
    t["flags"][2] = 3
    assert call(None, update_of(t))[0] == 1 and "flags" in call(None, update_of(t))[1]
    t = pyrt.make_transforms(3)
    for k in range(6):
        u = update_of(t)
        u.reserved[k] = 1
        rc, msg = call(None, u)
        assert rc == 1 and "reserved" in msg
    u = update_of(t)
    u.n_lights = 2
    rc, msg = call(None, u)
    assert rc == 1 and "lights is null" in msg
