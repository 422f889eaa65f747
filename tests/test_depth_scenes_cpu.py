"""The conditions tests/test_gpu_depth_forms.py rests on, shown without a GPU: the depths of depth_scenes' trees (if a
builder change moves one, this says so instead of the GPU tests quietly losing a row count), the liveness of every shallow
scene — shadow rays occluded and not, bounce rays that hit, vertices at path depths 1 and 2 — and the sensitivity of the
frames to the geometry: a kernel that lost a part of a scene would not pass a bit-for-bit comparison."""
import numpy as np
import pytest

import depth_scenes as ds
import lights_ref
import orc
import pyrt


def ident(name):
    return "%s-depth%d" % (name, ds.max_depth(ds.PREFIX + name))


@pytest.mark.parametrize("name", ds.NAMES + ds.FOUR_LIGHTS, ids=ident)
def test_the_host_builder_gives_the_tables_tree(name):
    meshes, leaf, n_tris, n_nodes, depth = ds.SHALLOW[ds.base(name)]
    s = ds.scene(name, ds.W, ds.H)
    info, _, _ = pyrt.bvh_build_host(s, leaf)
    print("%s: %d triangles, leaf_max %d, %d nodes, max_depth %d, %d stack rows, %d lights" % (
        name, len(s.arrays()["tri"]), info.leaf_max, info.n_nodes, info.max_depth, info.max_depth + 1, len(s.arrays()["lights"])))
    assert (len(s.arrays()["tri"]), info.leaf_max, info.n_nodes, info.max_depth) == (n_tris, leaf, n_nodes, depth)
    assert len(s.arrays()["lights"]) == (4 if name in ds.FOUR_LIGHTS else 3)
    assert ds.leaf_max(ds.PREFIX + name) == leaf and ds.max_depth(ds.PREFIX + name) == depth


def test_every_row_count_from_2_to_5_on_both_sides_of_the_two_record_leaf():
    rows = {}
    for name in ds.NAMES:
        _, leaf, _, _, depth = ds.SHALLOW[name]
        rows.setdefault(depth + 1, set()).add(leaf <= 2)
    assert rows == {2: {True, False}, 3: {True, False}, 4: {True, False}, 5: {False}}


@pytest.mark.parametrize("name", ds.Q8_NAMES, ids=ident)
def test_the_q8_trees_have_the_same_depth(name):
    """RT_NODES_Q8 records hold leaves of at most two triangles: the scenes of leaf_max 2 pack, C and G do not."""
    got = pyrt.bvh_check_host(ds.scene(name, ds.W, ds.H), ds.SHALLOW[name][1], pyrt.NODES_Q8)
    print("%s as RT_NODES_Q8: %s" % (name, got))
    assert got["depth"] == ds.SHALLOW[name][4]
    for other in ("C", "G"):
        with pytest.raises(pyrt.RtError, match="at most 2 triangles"):
            pyrt.bvh_check_host(ds.scene(other, ds.W, ds.H), ds.SHALLOW[other][1], pyrt.NODES_Q8)


@pytest.mark.parametrize("preset,w,h", [("hires", 13, 9), ("stress", 8, 6)])
def test_the_deep_presets(preset, w, h):
    info, _, _ = pyrt.bvh_build_host(pyrt.Scene(preset, w, h))
    print("%s: %d nodes, max_depth %d, %d stack rows" % (preset, info.n_nodes, info.max_depth, info.max_depth + 1))
    assert info.max_depth == ds.DEEP[preset] == ds.max_depth(preset)


def test_a_sub_scene_of_every_mesh_is_the_preset_and_without_mesh_0_is_ao_refs():
    import ao_ref
    s = pyrt.Scene("cubes", ds.W, ds.H)
    for got, want in ((ds.sub_scene(s, (0, 1, 2, 3, 4)), s), (ds.sub_scene(s, (1, 2, 3, 4)), ao_ref.without_mesh0(s))):
        a, b = got.arrays(), want.arrays()
        assert sorted(a) == sorted(b)
        for k in a:
            assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("name", ds.NAMES + ds.FOUR_LIGHTS, ids=ident)
def test_liveness(name):
    """Under the parameters the GPU frames run with: shadow rays occluded and not, bounce rays that hit, vertices at path
    depths 1 and 2; A, C and G closed, the others with misses."""
    lv = ds.liveness(ds.scene(name, ds.W, ds.H), ds.params())
    print("%s: primary hit %.3f, %d shadow rays %.3f occluded, %d bounce rays %.3f hit, vertices at depths %s" % (
        name, lv["primary_hit"], lv["shadow"], lv["occluded"], lv["bounce"], lv["bounce_hit"], lv["depths"]))
    assert lv["occluded"] > ds.MIN_OCCLUDED and 1 - lv["occluded"] > ds.MIN_UNOCCLUDED
    assert lv["bounce_hit"] > ds.MIN_BOUNCE_HIT
    assert 1 in lv["depths"] and 2 in lv["depths"]
    assert (lv["primary_hit"] == 1.0) == (ds.base(name) in ds.CLOSED)


@pytest.mark.parametrize("name", ds.SENSITIVE)
def test_a_dropped_mesh_shows_in_the_frame(name):
    s, p = ds.scene(name, ds.W, ds.H), ds.params()
    _, full, _ = orc.render(s, p, math_mode=orc.MATH_DET, accel=orc.ACCEL_OBVH)
    for mesh in range(len(s.arrays()["tri_begin"]) - 1):
        _, less, _ = orc.render(ds.without_mesh(name, ds.W, ds.H, mesh), p, math_mode=orc.MATH_DET, accel=orc.ACCEL_OBVH)
        share = lights_ref.changed_rgb_words(full, less)
        print("%s without its mesh %d: %.3f of the rgb words change" % (name, mesh, share))
        assert share > ds.MIN_CHANGED, (name, mesh, share)
