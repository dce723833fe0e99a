"""The uploaded BVH, read back (mcpt_debug_bvh_read) and compared with tests/bvh_ref.py.

Device-built trees (csrc/bvh_build.hip, "ploc" and "lbvh") must equal the reference builders' node
arrays bit for bit -- boxes, refs and numbering -- with the permuted triangle records, root ref, depth,
pair count and PLOC round count; every tree, device- or host-built, must pass bvh_ref.check_tree: each
ref reached once, each triangle in one leaf, boxes that contain their subtrees and nest, a reported
depth equal to the true height, and margin words equal to their subtree maxima of the oracle's W'_T
(this is what the upload's cull_ok / nest_ok and its pair_depth + 2 margin passes take on trust for a
device-built tree).  No rays are traced here; hit parity is tests/test_gpu.py's.

The host Scene accepts the `huge` input (triangles spanning +-3e38 on x, flat in z), so the NaN-area
branch of k_ploc_nn is part of the cases."""
import os

import numpy as np
import pytest

import bvh_ref as R
from test_pair_tree_host import host_tree, pair_tree_exe  # noqa: F401 (the fixture)

pytestmark = pytest.mark.gpu
F = np.float32


def u32(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


@pytest.fixture(scope="module")
def pt(mcpt_mod):
    p = mcpt_mod.PathTracer(0)
    yield p
    p.close()


_INPUTS = {}


def family(mcpt_mod, oracle, name):
    """(scene, arrays, oracle margins) of an input family, built once per session."""
    if name not in _INPUTS:
        s = R.scene_of(mcpt_mod, {**R.SMALL_FAMILIES, **R.LARGE_PLOC}[name]())
        a = s.arrays()
        _INPUTS[name] = (s, a, oracle.model_margins(a))
    return _INPUTS[name]


def check_device_tree(pt, s, a, margins, builder):
    pt.upload_scene(s, gpu_bvh=builder)
    nodes, tris, info = pt.bvh_read()
    ref = R.BUILDERS[builder](a["v0"], a["v1"], a["v2"])
    n = len(a["v0"])
    # (c) root ref, depth, pair count, rounds, root box
    assert info["gpu_built"] == 1 and info["ntri"] == n
    assert (info["root_ref"], info["depth"], info["npairs"]) == (ref["root_ref"], ref["depth"], ref["npairs"])
    if builder == "ploc":
        assert info["rounds"] == ref["rounds"]
    assert np.array_equal(u32(info["root_mn"]), u32(ref["root_mn"])) and np.array_equal(u32(info["root_mx"]), u32(ref["root_mx"]))
    # (a) the whole node array: boxes, refs, numbering (the margin words are check_tree's)
    got = nodes.copy()
    got[:, 3, 2:] = 0
    assert got.shape == ref["nodes"].shape
    diff = (u32(got) != u32(ref["nodes"])).reshape(len(got), 16).any(axis=1)
    assert not diff.any(), f"{int(diff.sum())} of {len(got)} nodes differ from the reference, first {int(np.argmax(diff))}"
    # (b) the permuted triangle records
    assert np.array_equal(u32(tris), u32(R.tri_records(a, info["tri_f4"])[ref["order"]]))
    # (d) the invariants, margins included
    R.check_tree(nodes, tris, info, a, margins)
    return nodes, tris, info, ref


@pytest.mark.parametrize("builder", ["ploc", "lbvh"])
@pytest.mark.parametrize("name", list(R.SMALL_FAMILIES))
def test_device_tree_equals_reference(mcpt_mod, oracle, pt, name, builder):
    s, a, m = family(mcpt_mod, oracle, name)
    _, _, info, ref = check_device_tree(pt, s, a, m, builder)
    if name == "chain" and builder == "lbvh":
        # ten levels peel the x cells 1023 .. 1 off, then 70 equal codes split on position bits:
        # more levels than the first batch of 16 bottom-up passes
        assert info["depth"] == ref["depth"] and info["depth"] >= 17
    if name == "random1":
        assert info["npairs"] == 0 and info["root_ref"] < 0 and info["depth"] == 0


@pytest.mark.parametrize("n", [32769, 32770])
def test_ploc_at_the_layout_switch(mcpt_mod, oracle, pt, n):
    """32768 nodes are exactly 2 MiB: sibling-pair numbering; one node more: depth-first."""
    s, a, m = family(mcpt_mod, oracle, f"random{n}")
    *_, ref = check_device_tree(pt, s, a, m, "ploc")
    assert ref["layout"] == (1 if n == 32769 else 0)


@pytest.mark.parametrize("builder", ["ploc", "lbvh"])
@pytest.mark.parametrize("which", ["scene_c2", "scene_cube"])
def test_device_tree_of_real_meshes(request, oracle, pt, which, builder):
    s, a = request.getfixturevalue(which)
    check_device_tree(pt, s, a, oracle.model_margins(a), builder)


def with_env(pt, s, env, **kw):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        pt.upload_scene(s, **kw)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return pt.bvh_read()


def test_device_pairs_unchanged_by_the_4_wide_collapse(mcpt_mod, oracle, pt):
    s, a, m = family(mcpt_mod, oracle, "random513")
    pt.upload_scene(s, gpu_bvh="ploc")
    nodes2, tris2, info2 = pt.bvh_read()
    nodes4, tris4, info4 = with_env(pt, s, {"MCPT_BVH_WIDTH": "4"}, gpu_bvh="ploc")
    assert (info2["width"], info4["width"]) == (2, 4)
    assert np.array_equal(u32(nodes2), u32(nodes4)) and np.array_equal(u32(tris2), u32(tris4))
    assert {k: v for k, v in info2.items() if k not in ("width", "root_mn", "root_mx")} == \
           {k: v for k, v in info4.items() if k not in ("width", "root_mn", "root_mx")}
    R.check_tree(nodes4, tris4, info4, a, m)


@pytest.mark.parametrize("which", ["scene_c2", "scene_cube"])
def test_host_trees_in_every_numbering(request, oracle, pt, pair_tree_exe, tmp_path, which):
    """The host path's pair conversion (csrc/host/pair_tree.cpp): four numberings, pad nodes in layout 3,
    leaves expanded to one triangle each -- every one a valid tree, and all the same tree: equal (box,
    margin) per leaf range, equal interior (box, margin) multisets, equal depth.  What is on the device is
    what the stand-alone host program (tests/test_pair_tree_host.py) computes, margins apart."""
    s, a = request.getfixturevalue(which)
    m = oracle.model_margins(a)
    assert m["contained"]
    tables, depths = [], []
    cases = [({"MCPT_SIBLING_LAYOUT": str(l)}, l, 2) for l in range(4)] + [({"MCPT_SIBLING_LAYOUT": "3", "MCPT_BVH_WIDTH": "4"}, 3, 4)]
    for env, layout, width in cases:
        nodes, tris, info = with_env(pt, s, env)
        assert (info["layout"], info["width"], info["gpu_built"], info["rounds"]) == (layout, width, 0, 0)
        assert np.array_equal(u32(tris), u32(R.tri_records(a, info["tri_f4"])))
        assert np.array_equal(u32(info["root_mn"]), u32(a["bmin"][0])) and np.array_equal(u32(info["root_mx"]), u32(a["bmax"][0]))
        R.check_tree(nodes, tris, info, a, m)
        host_nodes, host_tris, *_ = host_tree(pair_tree_exe, str(tmp_path), a, layout)
        no_margins = nodes.copy()
        no_margins[:, 3, 2:] = 0
        assert np.array_equal(u32(no_margins), u32(host_nodes)) and np.array_equal(u32(tris), u32(host_tris))
        tables.append(R.leaf_table(nodes, info))
        depths.append(info["depth"])
    assert len(set(depths)) == 1
    for leaves, inner in tables[1:]:
        assert np.array_equal(leaves, tables[0][0]) and np.array_equal(inner, tables[0][1])
    # one triangle per leaf after the expansion, every record in one
    assert np.array_equal(tables[0][0][:, 0], np.arange(len(a["v0"]))) and (tables[0][0][:, 1] == 1).all()


def test_host_depth_counts_each_leafs_own_expansion(oracle, pt, scene_c2):
    """Config 2's deepest desc leaf holds fewer triangles than its largest leaf: the upload once added
    the deepest expansion anywhere to the deepest leaf and reported 18 for a tree 17 high."""
    s, a = scene_c2
    _, _, info = with_env(pt, s, {})
    depth_of = np.zeros(len(a["nprims"]), np.int64)
    for i in range(len(a["nprims"])):  # children follow their parent
        if a["nprims"][i] == 0:
            depth_of[i + 1] = depth_of[a["offset"][i]] = depth_of[i] + 1
    leaf = a["nprims"] > 0
    own = depth_of[leaf] + np.ceil(np.log2(a["nprims"][leaf])).astype(np.int64)
    assert info["depth"] == own.max()
    assert depth_of[leaf].max() + int(np.ceil(np.log2(a["nprims"].max()))) > own.max()  # the old sum over-reports here


def test_empty_and_single_leaf_trees_read_back(mcpt_mod, oracle, pt):
    s, a, m = family(mcpt_mod, oracle, "random1")
    for kw in ({}, {"gpu_bvh": "ploc"}, {"gpu_bvh": "lbvh"}):
        pt.upload_scene(s, **kw)
        nodes, tris, info = pt.bvh_read()
        assert nodes.shape == (0, 4, 4) and info["npairs"] == 0 and info["root_ref"] < 0 and info["ntri"] == 1
        assert np.array_equal(u32(tris), u32(R.tri_records(a, info["tri_f4"])))
        R.check_tree(nodes, tris, info, a, m)
    e = mcpt_mod.Scene()
    e.set_env_color((1, 1, 1), 1.0)
    e.build(8)
    for kw in ({}, {"gpu_bvh": "ploc"}):
        pt.upload_scene(e, **kw)
        nodes, tris, info = pt.bvh_read()
        assert nodes.size == 0 and tris.size == 0
        assert (info["npairs"], info["root_ref"], info["ntri"], info["depth"]) == (0, 0, 0, 0)
        R.check_tree(nodes, tris, info, e.arrays(), None)
