"""tests/bvh_ref.py on its own (no GPU): the reference builders satisfy the tree invariants on every input
family of tests/test_bvh_build_gpu.py, the two LBVH formulations agree, and check_tree rejects
deliberately broken trees -- so a pass of the GPU tests means something."""
import numpy as np
import pytest

import bvh_ref as R

F = np.float32


def arrays_of(v):
    v = np.ascontiguousarray(v, F)
    return {"v0": v[:, 0].copy(), "v1": v[:, 1].copy(), "v2": v[:, 2].copy(), "tri_id": np.arange(len(v), dtype=np.int32)}


def build(name, v):
    a = arrays_of(v)
    ref = R.BUILDERS[name](a["v0"], a["v1"], a["v2"])
    tris = R.tri_records(a)[ref["order"]]
    return ref, tris, R.ref_info(ref, len(v)), a


@pytest.mark.parametrize("builder", ["lbvh", "ploc"])
@pytest.mark.parametrize("family", sorted(R.SMALL_FAMILIES))
def test_reference_trees_pass_the_checker(builder, family):
    ref, tris, info, a = build(builder, R.SMALL_FAMILIES[family]())
    R.check_tree(ref["nodes"], tris, info, a)
    # the front end sorts by code, stably
    _, _, code, order = R.sorted_prims(a["v0"], a["v1"], a["v2"])
    assert (np.diff(code.astype(np.int64)) >= 0).all()
    assert (np.diff(order)[np.diff(code.astype(np.int64)) == 0] > 0).all()


@pytest.mark.parametrize("n", [32769, 32770])
def test_reference_ploc_at_the_layout_switch(n):
    """n - 1 = 32768 nodes are exactly 2 MiB (sibling pairs, layout 1); one more is depth-first (0)."""
    ref, tris, info, a = build("ploc", R.LARGE_PLOC[f"random{n}"]())
    assert ref["layout"] == (1 if n == 32769 else 0)
    R.check_tree(ref["nodes"], tris, info, a)
    refs = R.node_views(ref["nodes"])[2]
    inner = refs >= 0
    if ref["layout"] == 0:  # a first interior child follows its parent
        first = np.where(inner[:, 0], refs[:, 0], np.where(inner[:, 1], refs[:, 1], -1))
        has = first >= 0
        assert np.array_equal(first[has], np.flatnonzero(has) + 1)
    else:  # two interior children sit side by side
        both = inner.all(axis=1)
        assert both.any() and np.array_equal(refs[both, 1], refs[both, 0] + 1)


@pytest.mark.parametrize("layout", [0, 1])
def test_reference_ploc_numberings_describe_one_tree(layout):
    a = arrays_of(R.random_tris(513))
    one = R.ploc(a["v0"], a["v1"], a["v2"], layout=layout)
    other = R.ploc(a["v0"], a["v1"], a["v2"], layout=1 - layout)
    info = R.ref_info(one, 513)
    for x, y in zip(R.leaf_table(one["nodes"], info), R.leaf_table(other["nodes"], info)):
        assert np.array_equal(x, y)
    assert one["depth"] == other["depth"] and one["rounds"] == other["rounds"]


@pytest.mark.parametrize("family", sorted(R.SMALL_FAMILIES))
def test_lbvh_formulations_agree(family):
    """Top-down radix-tree splits == Karras' per-node construction, child for child."""
    a = arrays_of(R.SMALL_FAMILIES[family]())
    if len(a["v0"]) < 2:
        return
    code = R.sorted_prims(a["v0"], a["v1"], a["v2"])[2]
    assert np.array_equal(R.radix_children(code)[0], R.karras_children(code))


def test_chain_input_is_deep():
    """x cells 1023, 511, ..., 1 peel off one per level (ten levels); the 70 triangles of cell 0 have
    equal codes and split on position bits, at least ceil(log2(70)) = 7 more levels: more than the 16
    bottom-up passes build_lbvh launches before it first looks for the root."""
    v = R.chain_tris()
    code = R.sorted_prims(v[:, 0], v[:, 1], v[:, 2])[2]
    cells = sorted(set(int(c) for c in code))
    assert len(cells) == 11 and (code == 0).sum() == 70
    ref, *_ = build("lbvh", v)
    assert ref["depth"] >= 17


def test_huge_input_takes_the_nan_branch():
    v = R.huge_tris()
    mn, mx, _ = R.prim_boxes(v[:, 0], v[:, 1], v[:, 2])
    with np.errstate(over="ignore", invalid="ignore"):
        area = R._half_area(mn[0], mx[0], mn[1], mx[1])
    assert np.isnan(area)


# ---- the margins' two host statements agree ---------------------------------------------------
@pytest.fixture(scope="module")
def cull_margin_host(tmp_path_factory):
    import os
    import subprocess

    from conftest import REPO

    d = tmp_path_factory.mktemp("cull_margin")
    exe = str(d / "cull_margin_host")
    subprocess.run(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
                    "-I", os.path.join(REPO, "mc-path-tracer_amd", "csrc"), "-I", os.path.join(REPO, "include"),
                    os.path.join(REPO, "tests", "native", "cull_margin_host.cpp"), "-o", exe], check=True)

    def run(a):
        np.concatenate([a["v0"], a["v1"], a["v2"]], axis=1).astype(F).tofile(str(d / "in.bin"))
        subprocess.run([exe, str(d / "in.bin"), str(d / "out.bin")], check=True, timeout=60)
        out = np.fromfile(str(d / "out.bin"), F)
        return out[:-1], out[-1]

    return run


@pytest.mark.parametrize("name", ["c2", "cube", "random513", "planar200", "coincident300", "huge", "random32769"])
def test_oracle_margins_round_as_the_product_core(name, request, mcpt_mod, oracle, cull_margin_host):
    """oracle.model_margins (trav_model.c, C) and cull_tri_margin / cull_to_float_up (mcpt_core.hpp, the
    code k_cull_tri runs, built for the host) give the same W'_T and P bit for bit: the arbiter for
    check_tree's margin comparison.  (They once differed: the restatement took the third edge as
    v2 - v1 where the product has only e2 - e1 of its record, and rounded P to nearest, not up.)"""
    if name in ("c2", "cube"):
        a = request.getfixturevalue("scene_" + name)[1]
    else:
        a = R.scene_of(mcpt_mod, {**R.SMALL_FAMILIES, **R.LARGE_PLOC}[name]()).arrays()
    m = oracle.model_margins(a)
    w, p = cull_margin_host(a)
    assert len(w) == len(a["v0"])
    assert np.array_equal(m["tri_w"][:len(w)].view(np.uint32), w.view(np.uint32))
    assert F(m["p"]).view(np.uint32) == p.view(np.uint32)
    if name == "huge":
        assert np.isinf(w).all()


# ---- the checker can fail -------------------------------------------------------------------
def margins_for(a, seed=3):
    """Synthetic per-triangle margins (the checker only needs some W'_T per triangle)."""
    rng = np.random.default_rng(seed)
    return {"tri_w": rng.uniform(1e-6, 1e-3, len(a["v0"])).astype(F), "p": F(1.5e-6)}


@pytest.fixture(scope="module", params=["lbvh", "ploc"])
def good(request):
    ref, tris, info, a = build(request.param, R.random_tris(37))
    m = margins_for(a)
    nodes = ref["nodes"].copy()
    refs = R.node_views(nodes)[2]
    nodes[:, 3, 2:] = R.expected_margins(refs, ref["root_ref"], m["tri_w"][ref["order"]])
    info = dict(info, cull_p=m["p"])
    R.check_tree(nodes, tris, info, a, m)
    return nodes, tris, info, a, m


def ulp_down(x):
    return np.nextafter(F(x), F(-np.inf))


def test_checker_rejects_swapped_child(good):
    nodes, tris, info, a, m = good
    bad = nodes.copy()
    refs = R.node_views(bad)[2]
    k = int(np.flatnonzero((refs >= 0).any(axis=1))[0])
    bad.view(np.int32)[k, 3, :2] = refs[k, ::-1]  # the refs swap, the boxes stay
    with pytest.raises(AssertionError):
        R.check_tree(bad, tris, info, a, m)


def test_checker_rejects_box_shrunk_by_one_ulp(good):
    nodes, tris, info, a, m = good
    for k, slot in ((0, 2), (len(nodes) - 1, 3)):  # a max of child 0 of the root, of child 1 of the last node
        bad = nodes.copy()
        bad[k, 1, slot] = ulp_down(bad[k, 1, slot])
        with pytest.raises(AssertionError):
            R.check_tree(bad, tris, info, a, m)


def test_checker_rejects_duplicated_leaf(good):
    nodes, tris, info, a, m = good
    refs = R.node_views(nodes)[2]
    both = np.flatnonzero((refs < 0).all(axis=1))
    k = int(both[0])
    bad = nodes.copy()
    bad[k, :3, 1], bad[k, :3, 3] = bad[k, :3, 0], bad[k, :3, 2]
    bad.view(np.int32)[k, 3, 1] = refs[k, 0]
    bad[k, 3, 3] = bad[k, 3, 2]
    with pytest.raises(AssertionError, match="no leaf or in two"):
        R.check_tree(bad, tris, info, a, m)
    # ... and a triangle id that sits in two records
    t2 = tris.copy()
    t2[1] = t2[0]
    with pytest.raises(AssertionError):
        R.check_tree(nodes, t2, info, a, m)


@pytest.mark.parametrize("off", [-1, 1])
def test_checker_rejects_depth_off_by_one(good, off):
    nodes, tris, info, a, m = good
    with pytest.raises(AssertionError, match="true height"):
        R.check_tree(nodes, tris, dict(info, depth=info["depth"] + off), a, m)


def test_checker_rejects_margin_lowered_by_one_ulp(good):
    nodes, tris, info, a, m = good
    for k in (0, len(nodes) // 2):
        bad = nodes.copy()
        bad[k, 3, 2] = ulp_down(bad[k, 3, 2])
        with pytest.raises(AssertionError, match="margin"):
            R.check_tree(bad, tris, info, a, m)
    with pytest.raises(AssertionError):
        R.check_tree(nodes, tris, dict(info, cull_p=ulp_down(info["cull_p"])), a, m)
    R.check_tree(nodes, tris, info, a, None)  # margins skipped: still a valid tree


def test_checker_rejects_pads_outside_layout_3(good):
    nodes, tris, info, a, m = good
    pad = np.zeros((1, 4, 4), F)
    pad.view(np.int32)[0, 3, :2] = R.K_END
    bad = np.concatenate([nodes, pad])
    with pytest.raises(AssertionError):
        R.check_tree(bad, tris, dict(info, npairs=len(bad), gpu_built=0), a, m)
    R.check_tree(bad, tris, dict(info, npairs=len(bad), gpu_built=0, layout=3), a, m)


def test_single_leaf_and_empty_trees():
    ref, tris, info, a = build("ploc", R.random_tris(1))
    assert ref["npairs"] == 0 and ref["root_ref"] < 0 and ref["depth"] == 0
    R.check_tree(ref["nodes"], tris, info, a)
    empty = {"v0": np.zeros((0, 3), F), "v1": np.zeros((0, 3), F), "v2": np.zeros((0, 3), F)}
    R.check_tree(np.zeros((0, 4, 4), F), np.zeros((0, 3, 4), F),
                 dict(info, ntri=0, root_ref=0, root_mn=F([1, 1, 1]), root_mx=F([-1, -1, -1])), empty)
