"""tests/refit_ref.py on its own (no GPU): the numpy refits of a desc tree and of a child-pair node array,
on moved inputs, against brute-force per-subtree vertex unions and bvh_ref.check_tree -- so a pass of
tests/test_geometry_update_gpu.py means something."""
import numpy as np
import pytest

import bvh_ref as R
import refit_ref as RF

F = np.float32
FAMILIES = ["random1", "random2", "random37", "random513", "lattice600", "coincident300", "chain"]


def u32(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def arrays_of(v):
    v = np.ascontiguousarray(v, F)
    return {"v0": v[:, 0].copy(), "v1": v[:, 1].copy(), "v2": v[:, 2].copy(), "tri_id": np.arange(len(v), dtype=np.int32)}


def test_warp_moves_every_vertex_off_the_coordinate_planes_and_keeps_shared_vertices():
    v = R.SMALL_FAMILIES["random513"]()
    w = RF.warp(v)
    assert w.dtype == F and w.shape == v.shape and (w != v).all() and (w != 0).all()
    assert np.array_equal(RF.warp(v[:7]), w[:7])  # a function of the position alone
    c = RF.warp(R.coincident_tris(5))
    assert (c == c[0]).all()


def median_split_desc(v, leaf=3):
    """A desc tree (depth-first, first child at i + 1) over the triangles in their order: halve the range
    until it holds at most `leaf` triangles.  Boxes are left zero: refit_desc fills them."""
    offset, nprims, ranges = [], [], []

    def rec(lo, hi):
        i = len(offset)
        offset.append(0), nprims.append(0), ranges.append((lo, hi))
        if hi - lo <= leaf:
            offset[i], nprims[i] = lo, hi - lo
            return
        mid = (lo + hi) // 2
        rec(lo, mid)
        offset[i] = len(offset)
        rec(mid, hi)

    rec(0, len(v))
    a = arrays_of(v)
    a["offset"], a["nprims"] = np.array(offset, np.int32), np.array(nprims, np.int32)
    return a, ranges


@pytest.mark.parametrize("n", [1, 2, 37, 272])
def test_refit_desc_equals_brute_force_subtree_unions(n):
    a, ranges = median_split_desc(R.random_tris(n))
    m = RF.moved_arrays(a)
    bmin, bmax = RF.refit_desc(m)
    allv = np.stack([m["v0"], m["v1"], m["v2"]], axis=1)
    for i, (lo, hi) in enumerate(ranges):
        t = allv[lo:hi].reshape(-1, 3)
        assert np.array_equal(u32(bmin[i]), u32(t.min(axis=0))) and np.array_equal(u32(bmax[i]), u32(t.max(axis=0)))
    # the unmoved boxes are not the moved ones: the refit did something
    b0, _ = RF.refit_desc(a)
    assert not np.array_equal(b0, bmin)


@pytest.mark.parametrize("builder", ["lbvh", "ploc"])
@pytest.mark.parametrize("family", FAMILIES)
def test_refit_nodes_pass_the_checker_on_the_moved_mesh(builder, family):
    a = arrays_of(R.SMALL_FAMILIES[family]())
    ref = R.BUILDERS[builder](a["v0"], a["v1"], a["v2"])
    m = RF.moved_arrays(a)
    nodes, rmn, rmx = RF.refit_nodes(ref["nodes"], ref["root_ref"], ref["order"], m["v0"], m["v1"], m["v2"])
    # topology and numbering stay
    assert np.array_equal(R.node_views(nodes)[2], R.node_views(ref["nodes"])[2])
    info = R.ref_info(ref, len(a["v0"]))
    info["root_mn"], info["root_mx"] = rmn, rmx
    tris = R.tri_records(m)[ref["order"]]
    R.check_tree(nodes, tris, info, m)
    # every leaf box is the exact vertex min / max, the root box the union of everything
    pmn, pmx, _ = R.prim_boxes(m["v0"], m["v1"], m["v2"])
    cmn, cmx, refs, _ = R.node_views(nodes)
    leaf = refs < 0
    off, cnt = R.leaf_range(refs[leaf])
    assert (cnt == 1).all()
    assert np.array_equal(u32(cmn[leaf]), u32(pmn[ref["order"]][off])) and np.array_equal(u32(cmx[leaf]), u32(pmx[ref["order"]][off]))
    assert np.array_equal(u32(rmn), u32(pmn.min(axis=0))) and np.array_equal(u32(rmx), u32(pmx.max(axis=0)))
    # refitting with the unmoved vertices gives the builder's own boxes back
    back, bmn, bmx = RF.refit_nodes(nodes, ref["root_ref"], ref["order"], a["v0"], a["v1"], a["v2"])
    assert np.array_equal(u32(back), u32(ref["nodes"]))
    assert np.array_equal(u32(bmn), u32(ref["root_mn"])) and np.array_equal(u32(bmx), u32(ref["root_mx"]))


def test_check_tree_rejects_an_unrefitted_tree():
    """The builder's boxes around the moved mesh: a leaf box misses its vertices."""
    a = arrays_of(R.random_tris(37))
    ref = R.ploc(a["v0"], a["v1"], a["v2"])
    m = RF.moved_arrays(a)
    with pytest.raises(AssertionError):
        R.check_tree(ref["nodes"], R.tri_records(m)[ref["order"]], R.ref_info(ref, 37), m)
