"""mcpt_scene_update_geometry: new vertex positions for the uploaded scene, the tree refitted on the device
(csrc/refit.hip) or rebuilt, and exactly the geometry-dependent state derived again.

Results do not depend on the tree, so everything is checked to the bit: the
read-back tree (mcpt_debug_bvh_read) against tests/refit_ref.py, tests/bvh_ref.py and fresh uploads of
the moved mesh, hits against fresh contexts holding the moved mesh in another tree, films and their
counters against fresh uploads.  Moved inputs are the original vertices through refit_ref.warp (a
smooth warp plus a fixed offset, so that no box face lands on +-0)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch  # noqa: F401 -- before libmcpt.so is loaded, as in a run of the whole suite: one HIP runtime for both

import bvh_ref as R
import refit_ref as RF

pytestmark = pytest.mark.gpu
F = np.float32
ASSETS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "assets")
HDR = os.path.join(ASSETS, "HDR_029_Sky_Cloudy_Env.hdr")


def u32(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def same_tree(x, y, margins=True):
    """Two bvh_read() results, word for word: nodes, records, every info field."""
    (n0, t0, i0), (n1, t1, i1) = x, y
    if not margins:
        n0, n1 = n0.copy(), n1.copy()
        n0[:, 3, 2:] = 0
        n1[:, 3, 2:] = 0
    assert n0.shape == n1.shape and t0.shape == t1.shape
    diff = (u32(n0) != u32(n1)).reshape(len(n0), 16).any(axis=1)
    assert not diff.any(), f"{int(diff.sum())} of {len(n0)} nodes differ, first {int(np.argmax(diff))}"
    assert np.array_equal(u32(t0), u32(t1)), "triangle records differ"
    assert set(i0) == set(i1)
    for k in i0:
        if k in ("root_mn", "root_mx", "cull_p"):
            assert np.array_equal(u32(i0[k]), u32(i1[k])), k
        else:
            assert i0[k] == i1[k], k


@pytest.fixture(scope="module")
def pt(mcpt_mod):
    p = mcpt_mod.PathTracer(0)
    yield p
    p.close()


@pytest.fixture(scope="module")
def pt2(mcpt_mod):
    p = mcpt_mod.PathTracer(0)
    yield p
    p.close()


_INPUTS = {}


def family(mcpt_mod, name):
    """(scene, arrays) of a bvh_ref input family, built once per session."""
    if name not in _INPUTS:
        s = R.scene_of(mcpt_mod, R.SMALL_FAMILIES[name]())
        _INPUTS[name] = (s, s.arrays())
    return _INPUTS[name]


def with_env(env, fn):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def update(pt, m, **kw):
    pt.update_geometry(m["v0"], m["v1"], m["v2"], **kw)


# ---------------------------------------------------------------------------------------------
# 1. device-built trees, refit
DEVICE_CASES = [(n, b) for b in ("ploc", "lbvh")
                for n in ("random1", "random2", "random37", "random513", "lattice600", "coincident300")] + [("chain", "lbvh")]


@pytest.mark.parametrize("name,builder", DEVICE_CASES)
def test_device_tree_refit(mcpt_mod, oracle, pt, name, builder):
    s, a = family(mcpt_mod, name)
    pt.upload_scene(s, gpu_bvh=builder)
    nodes0, tris0, info0 = pt.bvh_read()
    m = RF.moved_arrays(a)
    update(pt, m)
    nodes, tris, info = pt.bvh_read()
    # refs, numbering, npairs, depth and rounds are the upload's
    assert np.array_equal(R.node_views(nodes)[2], R.node_views(nodes0)[2])
    for k in ("npairs", "root_ref", "depth", "rounds", "width", "layout", "ntri", "tri_f4", "gpu_built"):
        assert info[k] == info0[k], k
    if name == "chain":
        assert info["depth"] >= 17  # more levels than one batch of 16 passes
    # the records of the moved mesh in the upload's order, bit for bit (ids untouched)
    ref = R.BUILDERS[builder](a["v0"], a["v1"], a["v2"])
    assert np.array_equal(u32(tris), u32(R.tri_records(m, info["tri_f4"])[ref["order"]]))
    # the whole node array equals the numpy refit of the reference builder's tree
    exp, rmn, rmx = RF.refit_nodes(ref["nodes"], ref["root_ref"], ref["order"], m["v0"], m["v1"], m["v2"])
    got = nodes.copy()
    got[:, 3, 2:] = 0
    assert np.array_equal(u32(got), u32(exp))
    assert np.array_equal(u32(info["root_mn"]), u32(rmn)) and np.array_equal(u32(info["root_mx"]), u32(rmx))
    # the invariants, margins and P included, against the oracle's margins of the moved mesh
    R.check_tree(nodes, tris, info, m, oracle.model_margins(m))
    # every leaf box is the exact vertex min / max
    pmn, pmx, _ = R.prim_boxes(m["v0"], m["v1"], m["v2"])
    cmn, cmx, refs, _ = R.node_views(nodes)
    leaf = refs < 0
    off, _ = R.leaf_range(refs[leaf])
    assert np.array_equal(u32(cmn[leaf]), u32(pmn[ref["order"]][off])) and np.array_equal(u32(cmx[leaf]), u32(pmx[ref["order"]][off]))


# ---------------------------------------------------------------------------------------------
# 2. host trees, refit
HOST_ENVS = [{"MCPT_SIBLING_LAYOUT": str(l)} for l in range(4)] + [{"MCPT_SIBLING_LAYOUT": "3", "MCPT_BVH_WIDTH": "4"}]


def halved_tree(a, leaf=8):
    """The arrays `a` under a desc tree that halves the triangle range until at most `leaf` triangles
    are left (depth-first, first child at i + 1): leaves of several triangles, which the upload expands."""
    offset, nprims = [], []

    def rec(lo, hi):
        i = len(offset)
        offset.append(0), nprims.append(0)
        if hi - lo <= leaf:
            offset[i], nprims[i] = lo, hi - lo
            return
        mid = (lo + hi) // 2
        rec(lo, mid)
        offset[i] = len(offset)
        rec(mid, hi)

    rec(0, len(a["v0"]))
    b = dict(a)
    b["offset"], b["nprims"] = np.array(offset, np.int32), np.array(nprims, np.int32)
    b["axis"] = np.zeros(len(offset), np.int32)
    b["bmin"], b["bmax"] = RF.refit_desc(b)
    return b


def host_arrays(request, mcpt_mod, which):
    if which == "random272":  # 8 prims per leaf (the SAH builder splits random triangles down to one)
        return halved_tree(family(mcpt_mod, "random272")[1], 8)
    return request.getfixturevalue(which)[1]


def doubled(a):
    """Every vertex times two (exact): every box extent doubles and every box area quadruples exactly, so
    no comparison of two areas changes."""
    m = dict(a)
    for k in ("v0", "v1", "v2"):
        m[k] = (np.ascontiguousarray(a[k], F) * F(2.0)).astype(F)
    m["bmin"], m["bmax"] = RF.refit_desc(m)
    return m


@pytest.mark.parametrize("which", ["scene_cube", "scene_c2", "random272"])
def test_host_tree_refit_equals_a_fresh_upload(request, mcpt_mod, oracle, pt, pt2, which):
    """Numberings 0-2 follow from the topology alone, so after a refit the tree equals a fresh upload of
    the warped mesh word for word.  Numbering 3 (line pairs) puts a node's larger-AREA interior child
    beside it: it is a function of the boxes, a refit keeps the upload's numbering (and its pad nodes),
    and a fresh upload of a warped mesh may number differently.  There the word-for-word comparison
    takes a move that keeps every area comparison (every vertex doubled, exact), and the warped mesh is
    checked for what a renumbering cannot change: the same (box, margin) per leaf range, the same
    interior (box, margin) multiset, a valid tree."""
    a = host_arrays(request, mcpt_mod, which)
    assert (a["nprims"] > 1).any()  # leaves the upload expands
    d0 = mcpt_mod.desc_from_arrays(a)
    warped, twice = RF.refitted_desc_arrays(a), doubled(a)
    for env in HOST_ENVS:
        layout, width = int(env["MCPT_SIBLING_LAYOUT"]), 4 if "MCPT_BVH_WIDTH" in env else 2
        for m in ([warped] if layout < 3 else [twice, warped]):
            with_env(env, lambda: pt.upload_scene(d0))
            before = pt.bvh_read()
            update(pt, m)
            after = pt.bvh_read()
            with_env(env, lambda: pt2.upload_scene(mcpt_mod.desc_from_arrays(m)))
            fresh = pt2.bvh_read()
            assert (after[2]["width"], after[2]["layout"]) == (width, layout)
            assert not np.array_equal(u32(before[0]), u32(after[0]))
            assert np.array_equal(R.node_views(before[0])[2], R.node_views(after[0])[2])  # refs, numbering, pads
            if m is warped and layout == 3:
                R.check_tree(*after, m, oracle.model_margins(m))
                for x, y in zip(R.leaf_table(after[0], after[2]), R.leaf_table(fresh[0], fresh[2])):
                    assert np.array_equal(x, y)
                assert np.array_equal(u32(after[1]), u32(fresh[1]))
                assert {k: v for k, v in after[2].items() if k not in ("npairs", "root_mn", "root_mx", "cull_p")} == \
                       {k: v for k, v in fresh[2].items() if k not in ("npairs", "root_mn", "root_mx", "cull_p")}
                for k in ("root_mn", "root_mx", "cull_p"):
                    assert np.array_equal(u32(after[2][k]), u32(fresh[2][k])), k
            else:
                same_tree(after, fresh)


# ---------------------------------------------------------------------------------------------
# 3. history-free
def test_updates_are_history_free(mcpt_mod, pt, pt2):
    s, a = family(mcpt_mod, "random513")
    pt.upload_scene(s, gpu_bvh="ploc")
    A = pt.bvh_read()
    B, Cc = RF.moved_arrays(a, phase=0.5), RF.moved_arrays(a, amp=0.2, phase=2.0, offset=(-0.4, 0.3, 0.9))
    for m in (B, Cc, a):
        update(pt, m)
    same_tree(pt.bvh_read(), A)
    # ten successive updates equal one direct update
    steps = [RF.moved_arrays(a, phase=0.3 * k, amp=0.02 * (k + 1)) for k in range(10)]
    for m in steps:
        update(pt, m)
    pt2.upload_scene(s, gpu_bvh="ploc")
    update(pt2, steps[-1])
    same_tree(pt.bvh_read(), pt2.bvh_read())


# ---------------------------------------------------------------------------------------------
# 4. rebuild
@pytest.mark.parametrize("builder,then", [("ploc", "ploc"), ("lbvh", "lbvh"), ("ploc", "lbvh"), ("lbvh", "ploc")])
def test_rebuild_equals_a_fresh_device_upload(mcpt_mod, oracle, pt, pt2, builder, then):
    s, a = family(mcpt_mod, "random513")
    m = RF.moved_arrays(a, amp=0.3)
    pt.upload_scene(s, gpu_bvh=builder)
    if then != builder:  # the builder switched between upload and update
        pt._ck(mcpt_mod.lib().mcpt_set_gpu_bvh_builder(pt.h, 0 if then == "lbvh" else 1))
    update(pt, m, mode="rebuild")
    got = pt.bvh_read()
    pt2.upload_scene(mcpt_mod.desc_from_arrays(m), gpu_bvh=then)
    same_tree(got, pt2.bvh_read())
    R.check_tree(*got, m, oracle.model_margins(m))
    # a refit after the rebuild writes through the new order
    update(pt, a)
    pt2.upload_scene(mcpt_mod.desc_from_arrays(m), gpu_bvh=then)
    update(pt2, a)
    same_tree(pt.bvh_read(), pt2.bvh_read())


def test_rebuild_of_single_leaf_and_width4(mcpt_mod, pt, pt2):
    s, a = family(mcpt_mod, "random1")
    m = RF.moved_arrays(a)
    pt.upload_scene(s, gpu_bvh="ploc")
    update(pt, m, mode="rebuild")
    pt2.upload_scene(mcpt_mod.desc_from_arrays(m), gpu_bvh="ploc")
    same_tree(pt.bvh_read(), pt2.bvh_read())
    s, a = family(mcpt_mod, "random513")
    m = RF.moved_arrays(a, amp=0.3)
    with_env({"MCPT_BVH_WIDTH": "4"}, lambda: pt.upload_scene(s, gpu_bvh="ploc"))
    update(pt, m, mode="rebuild")  # the width is the upload's, with the variable gone
    with_env({"MCPT_BVH_WIDTH": "4"}, lambda: pt2.upload_scene(mcpt_mod.desc_from_arrays(m), gpu_bvh="ploc"))
    same_tree(pt.bvh_read(), pt2.bvh_read())
    assert pt.bvh_read()[2]["width"] == 4
    ro, rd = rays(m)
    for x, y in zip(pt.trace_closest(ro, rd), pt2.trace_closest(ro, rd)):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))


# ---------------------------------------------------------------------------------------------
# 5. hits
def rays(m, n=4096, seed=77):
    """Fixed-seed rays from outside the mesh's box (aimed into it) and from inside (any direction)."""
    g = np.random.default_rng(seed)
    v = np.concatenate([m["v0"], m["v1"], m["v2"]])
    lo, hi = v.min(axis=0), v.max(axis=0)
    c, r = 0.5 * (lo + hi), 0.5 * np.linalg.norm(hi - lo)
    h = n // 2
    d = g.normal(size=(h, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o_out = c + 2.5 * r * d
    t_out = g.uniform(lo, hi, (h, 3)) - o_out
    o_in = g.uniform(lo, hi, (n - h, 3))
    t_in = g.normal(size=(n - h, 3))
    ro = np.concatenate([o_out, o_in]).astype(F)
    rd = np.concatenate([t_out, t_in])
    rd = (rd / np.linalg.norm(rd, axis=1, keepdims=True)).astype(F)
    return ro, rd


def same_hits(p, q, m):
    ro, rd = rays(m)
    a, b = p.trace_closest(ro, rd), q.trace_closest(ro, rd)
    assert (a[2] >= 0).sum() > 100 and (a[2] < 0).sum() > 100  # hits and misses both
    for x, y, what in zip(a, b, ("position, t", "normal, material", "triangle")):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), what
    assert np.array_equal(p.trace_any(ro, rd), q.trace_any(ro, rd))


@pytest.mark.parametrize("width", [2, 4])
def test_hits_equal_a_fresh_context_with_another_tree(mcpt_mod, pt, pt2, width):
    v = R.random_tris(513, size=0.25)
    s = R.scene_of(mcpt_mod, v)            # host SAH tree over the original mesh
    a = s.arrays()
    s_moved = R.scene_of(mcpt_mod, RF.warp(v, amp=0.2))  # host SAH tree over the moved mesh (another topology)
    m = RF.moved_arrays(a, amp=0.2)        # the same positions in the uploaded desc's order (warp is per position)
    env = {"MCPT_BVH_WIDTH": str(width)}
    # updated host tree against a fresh PLOC tree
    with_env(env, lambda: pt.upload_scene(s))
    update(pt, m)
    assert pt.bvh_read()[2]["width"] == width
    pt2.upload_scene(s_moved, gpu_bvh="ploc")
    same_hits(pt, pt2, m)
    # updated PLOC tree against a fresh host SAH tree
    with_env(env, lambda: pt.upload_scene(s, gpu_bvh="ploc"))
    before = pt.trace_closest(*rays(m))[2].copy()
    update(pt, m)
    pt2.upload_scene(s_moved)
    same_hits(pt, pt2, m)
    assert not np.array_equal(before, pt.trace_closest(*rays(m))[2])  # the mesh did move


# ---------------------------------------------------------------------------------------------
# 6. films
W, H, SPP = 48, 32, 8


def quad(y, half, cx=0.0, cz=0.0):
    p = F([[cx - half, y, cz - half], [cx + half, y, cz - half], [cx + half, y, cz + half], [cx - half, y, cz + half]])
    return np.stack([p[[0, 2, 1]], p[[0, 3, 2]]])  # two triangles, (2, 3, 3)


def film_scene(mcpt_mod, device_tables=False):
    """A floor, a blocker above it in the directional light's path, a few small triangles, an HDR
    environment."""
    clutter = R.random_tris(37, size=0.1) * F(0.5) + F([0.0, 0.6, 0.0])
    v = np.concatenate([quad(0.0, 2.0), quad(1.0, 0.5), clutter]).astype(F)
    s = mcpt_mod.Scene()
    nrm = np.tile(F([0, 1, 0]), (len(v), 1))
    s.add_mesh(v[:, 0], v[:, 1], v[:, 2], nrm, nrm, nrm, (0.7, 0.6, 0.5))
    s.add_dir_light((0.0, -1.0, 0.0), (1.0, 1.0, 1.0), 3.0)
    s.set_env_hdr(HDR, 1, device_tables=device_tables)
    s.build(8)
    return s


def film_moved(a):
    """Everything through a small warp; the blocker (the triangles at y == 1) also 4 units along x, out
    of the light's path over the floor."""
    m = RF.moved_arrays(a, amp=0.02)
    blocker = (a["v0"][:, 1] == 1) & (a["v1"][:, 1] == 1) & (a["v2"][:, 1] == 1)
    assert blocker.sum() == 2
    for k in ("v0", "v1", "v2"):
        m[k] = m[k].copy()
        m[k][blocker] += F([4.0, 0.0, 0.0])
    m["bmin"], m["bmax"] = RF.refit_desc(m)
    return m


def film_ctx(mcpt_mod, scene, **kw):
    p = mcpt_mod.PathTracer(0, mcpt_mod.default_config(spp=SPP, max_depth=4, tile=64))
    p.upload_scene(scene, **kw)
    p.set_camera(mcpt_mod.make_camera((0.4, 1.6, 5.0), -90.0, -14.0, aspect=F(W) / F(H)))
    p.resize(W, H, 64, 64)
    return p


def frame(p):
    p.render()
    Ld, smp = p.film()
    return dict(Ld=Ld.copy(), samples=smp.copy(), rays=p.ray_counts(), occ=p.occ_stats(), keys=p.occ_complete_stats()["keys"])


def test_film_after_an_update_equals_fresh_uploads(mcpt_mod):
    s = film_scene(mcpt_mod)
    a = s.arrays()
    m = film_moved(a)
    p = film_ctx(mcpt_mod, s)
    before = frame(p)
    update(p, m)
    got = frame(p)
    assert (got["samples"][: H - 1, : W - 1] == SPP).all() and got["samples"].max() == SPP
    assert not np.array_equal(before["Ld"], got["Ld"])
    # the same topology, uploaded fresh: the film and every counter
    q = film_ctx(mcpt_mod, mcpt_mod.desc_from_arrays(m))
    ref = frame(q)
    assert np.array_equal(u32(got["Ld"]), u32(ref["Ld"])) and np.array_equal(got["samples"], ref["samples"])
    assert got["rays"] == ref["rays"] and got["occ"] == ref["occ"] and got["keys"] == ref["keys"]
    assert ref["occ"][1] and ref["rays"]["any_hit"] > 0
    same_tree(p.bvh_read(), q.bvh_read())
    q.close()
    # another tree: the film and the total ray counts
    q = film_ctx(mcpt_mod, mcpt_mod.desc_from_arrays(m), gpu_bvh="ploc")
    other = frame(q)
    assert np.array_equal(u32(got["Ld"]), u32(other["Ld"])) and np.array_equal(got["samples"], other["samples"])
    assert (got["rays"]["extension"], got["rays"]["any_hit"]) == (other["rays"]["extension"], other["rays"]["any_hit"])
    # ... and that tree updated back to the original mesh gives the original film
    update(q, a)
    back = frame(q)
    assert np.array_equal(u32(back["Ld"]), u32(before["Ld"]))
    q.close()
    p.close()
    # without the occluder cache: the same film
    p = with_env({"MCPT_OCC_G": "0"}, lambda: film_ctx(mcpt_mod, s))
    update(p, m)
    off = frame(p)
    assert not off["occ"][1]
    assert np.array_equal(u32(off["Ld"]), u32(got["Ld"])) and np.array_equal(off["samples"], got["samples"])
    p.close()


# ---------------------------------------------------------------------------------------------
# 7. dependents
def test_dependents_see_an_update_as_a_re_upload(mcpt_mod):
    s = film_scene(mcpt_mod, device_tables=True)
    a = s.arrays()
    m = film_moved(a)
    p = film_ctx(mcpt_mod, s)
    eh, ew = a["env_tex"].shape[:2]
    env0, env_ms = p.env_tables(ew, eh), p.last_env_build_ms
    assert env0["device_built"] and env_ms > 0
    p.render()
    p.render_guides(1)
    p.denoise()
    p.temporal_accumulate()
    builds = p.primary_stats()["builds"]
    assert builds >= 1
    update(p, m)
    with pytest.raises(mcpt_mod.McptError):  # the guides are stale
        p.denoise()
    with pytest.raises(mcpt_mod.McptError):  # the temporal history is gone
        p.temporal()
    p.render()                               # auto-clear: a whole new frame, not SPP more samples
    Ld, smp = p.film()
    assert (smp[: H - 1, : W - 1] == SPP).all() and smp.max() == SPP
    assert p.primary_stats()["builds"] == builds + 1
    p.render_guides(1)
    p.denoise()
    p.temporal_accumulate()
    assert np.array_equal(p.temporal()["nsamples"], smp.astype(F))  # nothing accumulated: N' == s
    env1 = p.env_tables(ew, eh)
    for k in ("marginal_y", "conds_y", "pdf"):
        assert np.array_equal(u32(env0[k]), u32(env1[k])), k
    assert (env1["device_built"], env1["guides"]) == (env0["device_built"], env0["guides"])
    assert p.last_env_build_ms == env_ms
    ms = p.geometry_update_ms()
    assert ms["total"] > 0 and ms["records"] > 0 and ms["tree"] > 0
    p.close()


# ---------------------------------------------------------------------------------------------
# 8. device-pointer entry
def test_device_pointer_entry_equals_the_host_entry(mcpt_mod):
    s = film_scene(mcpt_mod)
    a = s.arrays()
    m = film_moved(a)
    nn = {k: (a[k] * F(-1.0)).astype(F) for k in ("n0", "n1", "n2")}  # normals through both entries too
    p, q = film_ctx(mcpt_mod, s, gpu_bvh="ploc"), film_ctx(mcpt_mod, s, gpu_bvh="ploc")
    p.update_geometry(m["v0"], m["v1"], m["v2"], nn["n0"], nn["n1"], nn["n2"])
    dev = [torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0") for x in (m["v0"], m["v1"], m["v2"], nn["n0"], nn["n1"], nn["n2"])]
    q.update_geometry(*dev)
    q.device = 1  # tensors of another GPU than the context's are refused before the call
    with pytest.raises(ValueError, match="context's GPU"):
        q.update_geometry(*dev[:3])
    q.device = 0
    same_tree(p.bvh_read(), q.bvh_read())
    fp, fq = frame(p), frame(q)
    assert np.array_equal(u32(fp["Ld"]), u32(fq["Ld"])) and np.array_equal(fp["samples"], fq["samples"]) and fp["rays"] == fq["rays"]
    ro, rd = rays(m)
    assert np.array_equal(u32(p.trace_closest(ro, rd)[1]), u32(q.trace_closest(ro, rd)[1]))  # the new normals
    q.update_geometry(*dev[:3], mode="rebuild")
    p.update_geometry(m["v0"], m["v1"], m["v2"], mode="rebuild")
    same_tree(p.bvh_read(), q.bvh_read())
    p.close()
    q.close()


@pytest.mark.parametrize("builder", [False, "ploc", "lbvh"])
def test_new_normals_equal_a_fresh_upload_and_survive_a_rebuild(mcpt_mod, builder):
    """Normals given to an update against a fresh context that was uploaded with them; on a device-built
    scene a later rebuild WITHOUT normals keeps them (NULL = keep), not the upload's."""
    s = film_scene(mcpt_mod)
    a = s.arrays()
    m = film_moved(a)
    g = np.random.default_rng(3)
    for k in ("n0", "n1", "n2"):  # per-vertex normals unlike the upload's, unit length
        v = g.normal(size=a[k].shape)
        m[k] = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F)
    p = film_ctx(mcpt_mod, s, gpu_bvh=builder)
    q = film_ctx(mcpt_mod, mcpt_mod.desc_from_arrays(m), gpu_bvh=builder)  # the reference: uploaded with the new normals
    ro, rd = rays(m)
    old = p.trace_closest(ro, rd)[1].copy()

    def same_as_fresh():
        got, ref = p.trace_closest(ro, rd), q.trace_closest(ro, rd)
        assert (ref[2] >= 0).sum() > 100
        for x, y, what in zip(got, ref, ("position, t", "normal, material", "triangle")):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), what
        fp, fq = frame(p), frame(q)
        assert np.array_equal(u32(fp["Ld"]), u32(fq["Ld"])) and np.array_equal(fp["samples"], fq["samples"]) and fp["rays"] == fq["rays"]

    p.update_geometry(m["v0"], m["v1"], m["v2"], m["n0"], m["n1"], m["n2"])
    same_as_fresh()
    assert not np.array_equal(u32(old), u32(p.trace_closest(ro, rd)[1]))
    update(p, m)  # positions alone: the normals stay
    same_as_fresh()
    if builder:
        update(p, m, mode="rebuild")  # no normals given: the refit's, not the upload's
        same_as_fresh()
        same_tree(p.bvh_read(), q.bvh_read())
        p.update_geometry(a["v0"], a["v1"], a["v2"], a["n0"], a["n1"], a["n2"], mode="rebuild")  # normals through a rebuild
        update(p, m)
        p.update_geometry(m["v0"], m["v1"], m["v2"], mode="rebuild")
        got, ref = p.trace_closest(ro, rd), film_ctx(mcpt_mod, mcpt_mod.desc_from_arrays({**m, **{k: a[k] for k in ("n0", "n1", "n2")}}), gpu_bvh=builder)
        for x, y in zip(got, ref.trace_closest(ro, rd)):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
        ref.close()
    p.close()
    q.close()


# ---------------------------------------------------------------------------------------------
# 9. errors
def test_rejected_updates_leave_the_scene_as_it_was(mcpt_mod):
    lib = mcpt_mod.lib()
    s, a = family(mcpt_mod, "random37")
    m = RF.moved_arrays(a)
    n = len(a["v0"])
    f = [mcpt_mod.fptr(np.ascontiguousarray(m[k], F)) for k in ("v0", "v1", "v2")]
    nf = [mcpt_mod.fptr(np.ascontiguousarray(a[k], F)) for k in ("n0", "n1", "n2")]
    p = mcpt_mod.PathTracer(0)
    assert lib.mcpt_scene_update_geometry(p.h, n, *f, None, None, None, 0) == -1 and b"no scene" in lib.mcpt_last_error(p.h)
    assert lib.mcpt_scene_update_geometry(None, n, *f, None, None, None, 0) == -1
    out = (C.c_float * 8)()
    assert lib.mcpt_debug_geometry_update_ms(None, out) == -1 and lib.mcpt_debug_geometry_update_ms(p.h, None) == -1
    ro, rd = rays(a, 512)
    for kw, host_tree in (({}, True), ({"gpu_bvh": "ploc"}, False)):
        p.upload_scene(s, **kw)
        tree, hits = p.bvh_read(), p.trace_closest(ro, rd)
        bad = [(n - 1, f, [None] * 3, 0, b"ntri"), (n + 1, f, [None] * 3, 0, b"ntri"), (0, f, [None] * 3, 0, b"ntri"),
               (n, f, [nf[0], None, None], 0, b"normals"), (n, f, [nf[0], nf[1], None], 0, b"normals"),
               (n, f, [None, None, nf[2]], 0, b"normals"), (n, f, [None] * 3, 2, b"mode"), (n, f, [None] * 3, -1, b"mode"),
               (n, [f[0], None, f[2]], [None] * 3, 0, b"null")]
        if host_tree:
            bad.append((n, f, [None] * 3, 1, b"REBUILD"))
        for nt, vv, nrm, mode, word in bad:
            for entry in (lib.mcpt_scene_update_geometry, lib.mcpt_scene_update_geometry_device):
                vals = [C.cast(x, C.c_void_p) if x is not None else None for x in vv + nrm] if entry is lib.mcpt_scene_update_geometry_device else vv + nrm
                assert entry(p.h, nt, *vals, mode) == -1, (nt, mode, word)
                assert word in lib.mcpt_last_error(p.h), (word, lib.mcpt_last_error(p.h))
        with pytest.raises(ValueError):
            p.update_geometry(m["v0"], m["v1"], m["v2"], mode="squash")
        same_tree(p.bvh_read(), tree)
        for x, y in zip(p.trace_closest(ro, rd), hits):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
        update(p, m)  # ... and the scene is still usable
        assert not np.array_equal(u32(p.bvh_read()[1]), u32(tree[1]))
    # a scene without triangles accepts ntri == 0 and does nothing
    e = mcpt_mod.Scene()
    e.set_env_color((1, 1, 1), 1.0)
    e.build(8)
    for kw in ({}, {"gpu_bvh": "ploc"}):
        p.upload_scene(e, **kw)
        assert lib.mcpt_scene_update_geometry(p.h, 0, None, None, None, None, None, None, 0) == 0
        assert lib.mcpt_scene_update_geometry(p.h, 1, *f, None, None, None, 0) == -1
        assert p.bvh_read()[2]["ntri"] == 0
    p.close()
