"""The host half of a scene upload (csrc/host/pair_tree.cpp), built as a stand-alone program
(tests/native/pair_tree_host.cpp) and run without a device: the pair tree of real scenes in every
numbering against tests/bvh_ref.py's checker, hand-written descs for the expansion, the fall-back to
layout 0, the containment flags and the error strings, the 4-wide collapse, and one run under the
address and undefined-behaviour sanitizers.  No GPU.  tests/test_bvh_build_gpu.py ties the program's
output to what an upload puts on the device."""
import os
import subprocess

import numpy as np
import pytest

import bvh_ref as R
from conftest import REPO

F = np.float32
CSRC = os.path.join(REPO, "mc-path-tracer_amd", "csrc")
SRCS = [os.path.join(REPO, "tests", "native", "pair_tree_host.cpp"), os.path.join(CSRC, "host", "pair_tree.cpp")]
FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-I", CSRC, "-I", os.path.join(REPO, "include")]
QUAD_NO_SRC = 0xFFFFFFFF


def u32(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def build_exe(path, extra=()):
    subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, *extra, *SRCS, "-o", path], check=True)
    return path


@pytest.fixture(scope="session")
def pair_tree_exe(tmp_path_factory):
    return build_exe(str(tmp_path_factory.mktemp("pair_tree_host") / "pair_tree_host"))


def host_tree(exe, tmp, a, request=-1):
    """The program's output for Scene.arrays()-style arrays: (nodes (m, 4, 4), tris, info, extra), or the
    error string of a rejected desc.  info is what PathTracer.bvh_read() would report for a 2-wide upload."""
    T, N = len(a["mat"]), len(a["nprims"])
    tid = a.get("tri_id")
    fin, pre = os.path.join(tmp, "desc.bin"), os.path.join(tmp, "out")
    with open(fin, "wb") as f:
        f.write(np.array([T, N, len(a["mat_params"]) if "mat_params" in a else 1, tid is not None], np.int32).tobytes())
        for k in ("v0", "v1", "v2", "n0", "n1", "n2"):
            f.write(np.ascontiguousarray(a[k], F).tobytes())
        f.write(np.ascontiguousarray(a["mat"], np.int32).tobytes())
        if tid is not None:
            f.write(np.ascontiguousarray(tid, np.int32).tobytes())
        for k, dt in (("bmin", F), ("bmax", F), ("offset", np.int32), ("nprims", np.int32)):
            f.write(np.ascontiguousarray(a[k], dt).tobytes())
    line = subprocess.run([exe, str(request), fin, pre], check=True, timeout=120, capture_output=True, text=True).stdout.strip()
    if line.startswith("error: "):
        return line[len("error: "):]
    word = dict(w.split("=") for w in line.split()[1:])
    assert line.startswith("ok ") and len(word) == 10
    v = {k: int(x) for k, x in word.items()}
    nodes = np.fromfile(pre + ".pairs", F).reshape(-1, 4, 4)
    tris = np.fromfile(pre + ".tri", F).reshape(T, v["tri_f4"], 4)
    assert len(nodes) == v["npairs"]
    root = (a["bmin"][0], a["bmax"][0]) if T else (F([1, 1, 1]), F([-1, -1, -1]))
    info = {"npairs": v["npairs"], "root_ref": v["root_ref"], "depth": v["depth"], "width": 2, "layout": v["layout"], "ntri": T,
            "tri_f4": v["tri_f4"], "gpu_built": 0, "rounds": 0, "root_mn": F(root[0]), "root_mx": F(root[1]), "cull_p": F(0)}
    extra = {"contained": bool(v["contained"]), "nested": bool(v["nested"]), "quad_root": v["quad_root"], "max_push": v["max_push"],
             "quads": np.fromfile(pre + ".quads", F).reshape(-1, 8, 4), "src": np.fromfile(pre + ".src", np.uint32).reshape(-1, 4),
             "sh": np.fromfile(pre + ".sh", F).reshape(T, 3, 4)}
    assert len(extra["quads"]) == len(extra["src"]) == v["nquads"]
    return nodes, tris, info, extra


def sh_records(a):
    n = np.concatenate([np.asarray(a[k], F).reshape(-1, 3) for k in ("n0", "n1", "n2")], axis=1)
    out = np.zeros((len(n), 12), F)
    out[:, :9] = n
    out.view(np.int32)[:, 9] = a["mat"]
    return out.reshape(-1, 3, 4)


def check_scene(exe, tmp, a, pads):
    """Every layout request of a real scene; returns the layout-0 result.  pads: layout 3 must have some (a node
    without an interior child leaves one, unless it is the last)."""
    tables, depths, first = [], [], None
    for layout in range(4):
        nodes, tris, info, x = host_tree(exe, tmp, a, layout)
        assert info["layout"] == layout and x["contained"] and x["nested"]
        assert np.array_equal(u32(tris), u32(R.tri_records(a, info["tri_f4"]))) and np.array_equal(u32(x["sh"]), u32(sh_records(a)))
        R.check_tree(nodes, tris, info, a)
        pad = (R.node_views(nodes)[2] == R.K_END).all(axis=1)
        if layout == 3:
            assert (pad.any() or not pads) and not (nodes[pad][:, :3] != 0).any()  # (check_tree: nothing references a pad)
        else:
            assert not pad.any()
        tables.append(R.leaf_table(nodes, info))
        depths.append(info["depth"])
        first = first or (nodes, tris, info, x)
    assert len(set(depths)) == 1
    for leaves, inner in tables[1:]:
        assert np.array_equal(leaves, tables[0][0]) and np.array_equal(inner, tables[0][1])
    # one triangle per leaf after the expansion, every record in one
    assert np.array_equal(tables[0][0][:, 0], np.arange(len(a["v0"]))) and (tables[0][0][:, 1] == 1).all()
    return first


@pytest.mark.parametrize("which", ["scene_c1", "scene_c2", "scene_cube"])
def test_scene_trees_in_every_numbering(request, pair_tree_exe, tmp_path, which):
    """tests/test_bvh_build_gpu.py::test_host_trees_in_every_numbering without a device (so without margins)."""
    _, a = request.getfixturevalue(which)
    if which != "scene_cube":
        assert (a["nprims"] > 1).sum() == {"scene_c1": 392, "scene_c2": 1884}[which] and a["nprims"].max() <= 3
    first = check_scene(pair_tree_exe, str(tmp_path), a, pads=which != "scene_cube")  # (the cube's tree is a chain)
    if which == "scene_c2":
        check_quads(*first)


# ---------------------------------------------------------------------------------------------
# hand-written descs
def desc(nodes, ntri, seed=0):
    """nodes: depth-first rows (bmin, bmax, offset, nprims); random triangles inside the unit cube."""
    rng = np.random.default_rng(seed)
    a = {k: rng.uniform(0, 1, (ntri, 3)).astype(F) for k in ("v0", "v1", "v2")}
    a.update({k: rng.uniform(-1, 1, (ntri, 3)).astype(F) for k in ("n0", "n1", "n2")})
    a["mat"] = np.zeros(ntri, np.int32)
    a["bmin"] = np.array([n[0] for n in nodes], F).reshape(-1, 3)
    a["bmax"] = np.array([n[1] for n in nodes], F).reshape(-1, 3)
    a["offset"] = np.array([n[2] for n in nodes], np.int32)
    a["nprims"] = np.array([n[3] for n in nodes], np.int32)
    return a


def fit_boxes(a):
    """Every node's box = the exact union of its subtree's vertices (children follow their parent)."""
    verts = np.stack([a["v0"], a["v1"], a["v2"]], axis=1)
    for i in range(len(a["nprims"]) - 1, -1, -1):
        if a["nprims"][i] > 0:
            v = verts[a["offset"][i]:a["offset"][i] + a["nprims"][i]].reshape(-1, 3)
            a["bmin"][i], a["bmax"][i] = v.min(axis=0), v.max(axis=0)
        else:
            ch = [i + 1, a["offset"][i]]
            a["bmin"][i], a["bmax"][i] = a["bmin"][ch].min(axis=0), a["bmax"][ch].max(axis=0)
    return a


Z, O = (0, 0, 0), (1, 1, 1)


def two_leaves():
    """A root over a leaf of 8 triangles and a leaf of 5."""
    return fit_boxes(desc([(Z, O, 2, 0), (Z, O, 0, 8), (Z, O, 8, 5)], 13))


def seven_nodes():
    """A full tree of four one-triangle leaves: nodes 0 (1 (2 3)) (4 (5 6))."""
    return fit_boxes(desc([(Z, O, 4, 0), (Z, O, 3, 0), (Z, O, 0, 1), (Z, O, 1, 1), (Z, O, 6, 0), (Z, O, 2, 1), (Z, O, 3, 1)], 4))


def test_expansion_depth_and_boxes(pair_tree_exe, tmp_path):
    a = two_leaves()
    verts = np.stack([a["v0"], a["v1"], a["v2"]], axis=1)
    for layout in (-1, 0, 3):
        nodes, tris, info, x = host_tree(pair_tree_exe, str(tmp_path), a, layout)
        R.check_tree(nodes, tris, info, a)
        # a leaf's own depth (1: the root pair) plus ceil(log2 n): 1 + 3 for the leaf of 8 and for the leaf of 5
        assert info["depth"] == 1 + 3 and info["npairs"] == 1 + 7 + 4 and x["contained"] and x["nested"]
        # every expansion box (all but the root pair's) is the union of its triangles' vertices, bit for bit
        cmn, cmx, refs, _ = R.node_views(nodes)

        def tris_under(ref):
            if ref < 0:
                o, c = R.leaf_range(np.int32(ref))
                return list(range(int(o), int(o) + int(c)))
            return tris_under(refs[ref, 0]) + tris_under(refs[ref, 1])

        for p in range(1, len(refs)):
            for k in range(2):
                v = verts[tris_under(refs[p, k])].reshape(-1, 3)
                assert np.array_equal(u32(cmn[p, k]), u32(v.min(axis=0))) and np.array_equal(u32(cmx[p, k]), u32(v.max(axis=0)))
        check_quads(nodes, tris, info, x)
    # each leaf counts its own expansion: a deeper leaf of 2 beside the leaf of 8 gives max(1 + 3, 2 + 1), not 2 + 3
    b = fit_boxes(desc([(Z, O, 2, 0), (Z, O, 0, 8), (Z, O, 4, 0), (Z, O, 8, 2), (Z, O, 10, 1)], 11))
    assert host_tree(pair_tree_exe, str(tmp_path), b)[2]["depth"] == 4


def test_inputs_that_are_no_tree_keep_layout_0(pair_tree_exe, tmp_path):
    dag = fit_boxes(desc([(Z, O, 2, 0), (Z, O, 3, 0), (Z, O, 3, 0), (Z, O, 0, 1), (Z, O, 1, 1)], 2))  # 0 -> (1, 2), 1 -> (2, 3), 2 -> (3, 4)
    unreachable = fit_boxes(desc([(Z, O, 5, 0), (Z, O, 0, 1), (Z, O, 4, 0), (Z, O, 1, 1), (Z, O, 2, 1), (Z, O, 3, 1)], 4))  # 2 -> (3, 4) has no parent
    for a, npairs in ((dag, 3), (unreachable, 2)):
        for layout in (-1, 0, 1, 2, 3):
            nodes, _, info, _ = host_tree(pair_tree_exe, str(tmp_path), a, layout)
            assert info["layout"] == 0 and info["npairs"] == npairs
            assert not (R.node_views(nodes)[2] == R.K_END).any()
    nodes, tris, info, _ = host_tree(pair_tree_exe, str(tmp_path), seven_nodes(), 3)  # the same shapes as a tree: renumbered
    assert info["layout"] == 3
    R.check_tree(nodes, tris, info, seven_nodes())


def test_containment_and_nesting_flags(pair_tree_exe, tmp_path):
    good = seven_nodes()
    assert host_tree(pair_tree_exe, str(tmp_path), good)[3]["contained"]
    miss = seven_nodes()
    miss["bmax"][5] = miss["bmax"][5] - F(1e-3)  # a leaf box that misses a vertex of its triangle
    x = host_tree(pair_tree_exe, str(tmp_path), miss)[3]
    assert (x["contained"], x["nested"]) == (False, False)
    poke = seven_nodes()
    poke["bmax"][5] = poke["bmax"][4] + F(1e-3)  # a child box larger than its parent's: still contains its triangle
    x = host_tree(pair_tree_exe, str(tmp_path), poke)[3]
    assert (x["contained"], x["nested"]) == (True, False)


def test_rejected_descs_give_the_upload_error_strings(pair_tree_exe, tmp_path):
    t = str(tmp_path)
    for off in (0, -1, 7):  # not after the node itself, or outside the array
        a = seven_nodes()
        a["offset"][0] = off
        assert host_tree(pair_tree_exe, t, a) == "bad BVH child offset"
    a = seven_nodes()
    a["nprims"][6], a["offset"][6] = 0, 7  # an interior node last
    assert host_tree(pair_tree_exe, t, a) == "bad BVH child offset"
    assert host_tree(pair_tree_exe, t, fit_boxes(desc([(Z, O, 0, 9)], 9))) == "leaf with more than 8 primitives"
    a = two_leaves()
    a["offset"][2] = 9  # 9 + 5 > 13
    assert host_tree(pair_tree_exe, t, a) == "bad leaf range"
    a = two_leaves()
    a["nprims"][1], a["offset"][1] = 9, 20  # the first failing check decides
    assert host_tree(pair_tree_exe, t, a) == "leaf with more than 8 primitives"
    a = two_leaves()
    a["mat"][3] = 1
    assert host_tree(pair_tree_exe, t, a) == "material id out of range"
    assert host_tree(pair_tree_exe, t, desc([], 2)) == "triangles without BVH"


def test_empty_and_single_leaf_descs(pair_tree_exe, tmp_path):
    for layout in (-1, 3):
        nodes, tris, info, x = host_tree(pair_tree_exe, str(tmp_path), desc([], 0), layout)
        assert nodes.size == 0 and tris.size == 0 and x["quads"].size == 0
        assert (info["npairs"], info["root_ref"], info["depth"], info["layout"], x["quad_root"], x["max_push"]) == (0, 0, 0, 0, 0, 0)
        R.check_tree(nodes, tris, info, desc([], 0))
        one = fit_boxes(desc([(Z, O, 0, 1)], 1))
        nodes, tris, info, x = host_tree(pair_tree_exe, str(tmp_path), one, layout)
        assert nodes.size == 0 and info["root_ref"] == np.int32(-2 ** 31) and info["depth"] == 0 and info["layout"] == 0
        assert x["quads"].size == 0 and x["quad_root"] == info["root_ref"] and x["max_push"] == 0
        R.check_tree(nodes, tris, info, one)
        three = fit_boxes(desc([(Z, O, 0, 3)], 3))  # one leaf of three: its expansion is the whole tree
        nodes, tris, info, x = host_tree(pair_tree_exe, str(tmp_path), three, layout)
        assert (info["npairs"], info["root_ref"], info["depth"]) == (2, 0, 2)
        R.check_tree(nodes, tris, info, three)
        check_quads(nodes, tris, info, x)


# ---------------------------------------------------------------------------------------------
# the 4-wide collapse
def check_quads(nodes, tris, info, x):
    """pairs_to_quads' output against the pair array it was made from.  A quad row is 8 float4, component
    = slot: mn.x mx.x mn.y mx.y mn.z mx.z, refs, margins."""
    quads, src, m = x["quads"], x["src"], len(nodes)
    refs = R.node_views(nodes)[2]
    root = info["root_ref"]
    if root < 0 or m == 0:  # no interior node: nothing to collapse, the root ref stays
        assert quads.size == 0 and x["quad_root"] == root and x["max_push"] == 0
        return
    assert x["quad_root"] == 0
    used = src != QUAD_NO_SRC
    by_slot = np.moveaxis(quads, 2, 1)  # (quad, slot, row)
    # a used slot's box, margin and ref are those of pair child (src >> 1, src & 1)
    p, k = (src[used] >> 1).astype(np.int64), (src[used] & 1).astype(np.int64)
    assert (p < m).all()
    slot = by_slot[used]
    for ax in range(3):
        assert np.array_equal(u32(slot[:, 2 * ax]), u32(nodes[p, ax, k]))
        assert np.array_equal(u32(slot[:, 2 * ax + 1]), u32(nodes[p, ax, 2 + k]))
    assert np.array_equal(u32(slot[:, 7]), u32(nodes[p, 3, 2 + k]))
    pair_ref, qref = refs[p, k], np.ascontiguousarray(slot).view(np.int32)[:, 6]
    leaf = pair_ref < 0
    assert np.array_equal(qref[leaf], pair_ref[leaf])  # a leaf ref as it is
    # ... an interior ref g as the 4-wide node made of g: its first slot copies g's first child, or that child's
    assert ((qref[~leaf] >= 0) & (qref[~leaf] < len(quads))).all()
    g = pair_ref[~leaf]
    first = np.where(refs[g, 0] < 0, 2 * g, 2 * refs[g, 0].clip(0))
    assert np.array_equal(src[qref[~leaf], 0], first) and src[0, 0] == (2 * root if refs[root, 0] < 0 else 2 * refs[root, 0])
    # empty slots: the no-source mark, the end ref and zeros, after the used ones; a node has two to four children
    empty = np.ascontiguousarray(by_slot[~used])
    assert (empty.view(np.int32)[:, 6] == R.K_END).all() and not (empty[:, :6] != 0).any() and not (empty[:, 7] != 0).any()
    assert (used[:, :-1] >= used[:, 1:]).all() and (used.sum(axis=1) >= 2).all()
    # no pair child in two slots; every leaf child of the tree in one (the quads hold every triangle); an interior
    # child is in one unless a 4-wide node took its two children in its place
    in_slot = np.zeros((m, 2), np.int64)
    np.add.at(in_slot, (p, k), 1)
    assert in_slot.max() == 1
    reach = np.concatenate(R.tree_levels(refs, root)[0])
    r = refs[reach]
    assert (in_slot[reach][r < 0] == 1).all()
    assert ((in_slot[reach] == 1) | (r < 0) | (in_slot[r.clip(0)] == 1).all(axis=2)).all()
    assert in_slot.sum() == in_slot[reach].sum()  # nothing else (no pad, no unreachable node)
    # max_push: the most pushes (children - 1 per node) along a root-to-leaf path, from the quad array
    qrefs = quads.view(np.int32)[:, 6, :]
    push, stack = 0, [(0, 0)]
    while stack:
        q, acc = stack.pop()
        acc += int(used[q].sum()) - 1
        push = max(push, acc)
        stack += [(int(c), acc) for c, u in zip(qrefs[q], used[q]) if u and c >= 0]
    assert x["max_push"] == push


def test_quads_of_the_hand_written_trees(pair_tree_exe, tmp_path):
    for a in (seven_nodes(), two_leaves()):
        for layout in (0, 2, 3):
            check_quads(*host_tree(pair_tree_exe, str(tmp_path), a, layout))


def test_sanitized_build_runs_clean(scene_c2, pair_tree_exe, tmp_path):
    """The stand-alone program once more with the address and undefined-behaviour sanitizers on its host
    code (it has no device code), on config 2 in layout 3: same bytes, no report."""
    san = "-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all".split()
    exe = build_exe(str(tmp_path / "pair_tree_host_san"), ["-g", *san])
    _, a = scene_c2
    (tmp_path / "a").mkdir(), (tmp_path / "b").mkdir()
    got = host_tree(exe, str(tmp_path / "a"), a, 3)
    ref = host_tree(pair_tree_exe, str(tmp_path / "b"), a, 3)
    assert got[2]["layout"] == 3 and np.array_equal(u32(got[0]), u32(ref[0])) and np.array_equal(u32(got[1]), u32(ref[1]))
    assert np.array_equal(u32(got[3]["quads"]), u32(ref[3]["quads"])) and np.array_equal(got[3]["src"], ref[3]["src"])
