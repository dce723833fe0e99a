"""Reference BVH builders and a tree checker for the device builders (csrc/bvh_build.hip) -- numpy only.

Both device builders are deterministic (Morton codes from correctly rounded float32 arithmetic, a stable
sort, code ties broken by position, PLOC node indices from prefix sums), so a restatement of the rules
reproduces the uploaded child-pair node array bit for bit.  This file states the rules from their
definitions (bvh_build.hip's header and comments):

* front end: triangle boxes, centroids, centroid bounds, 30-bit Morton codes, stable sort;
* lbvh():  the binary radix tree over the distinct keys (code << 32) | position, built top-down by
           splitting each range where the highest differing key bit changes (karras_children() is the
           second formulation, Karras 2012 Fig. 4 node by node, for small inputs);
* ploc():  parallel locally-ordered clustering with search radius 16, then the locality numbering;
* check_tree(): the invariants every uploaded pair tree must satisfy, built on the device or the host.

Float arrays are float32 throughout; comparisons with read-back trees go through .view(np.uint32).
"""
import numpy as np

F = np.float32
LEAF_BIT = 0x80000000
K_END = -1          # "no child": pad nodes of layout 3 only
K_MAX_STACK = 64    # kernels.hpp kMaxStack
PLOC_RADIUS = 16    # bvh_build.hip kPlocR


# ---------------------------------------------------------------------------------------------
# shared front end
def prim_boxes(v0, v1, v2):
    """Per-triangle box (min / max of the three vertices) and centroid 0.5f * (mn + mx)."""
    v0, v1, v2 = (np.ascontiguousarray(v, F).reshape(-1, 3) for v in (v0, v1, v2))
    mn = np.fmin(np.fmin(v0, v1), v2)
    mx = np.fmax(np.fmax(v0, v1), v2)
    with np.errstate(over="ignore", invalid="ignore"):
        cen = F(0.5) * (mn + mx)
    return mn, mx, cen


def _expand_bits(v):
    """10 bits -> every third bit."""
    v = v.astype(np.uint64)
    out = np.zeros_like(v)
    for b in range(10):
        out |= ((v >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b)
    return out.astype(np.uint32)


def morton_codes(cen):
    """k_morton: per axis ext > 0 ? (c - mn) / ext : 0, times 1024, clamped to [0, 1023], truncated;
    interleaved with x highest."""
    cmn, cmx = np.fmin.reduce(cen, axis=0), np.fmax.reduce(cen, axis=0)
    q = []
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for k in range(3):
            ext = F(cmx[k] - cmn[k])
            f = (cen[:, k] - cmn[k]) / ext if ext > 0 else np.zeros(len(cen), F)
            f = np.fmin(np.fmax(f.astype(F) * F(1024.0), F(0.0)), F(1023.0))
            q.append(f.astype(np.uint32))
    return (_expand_bits(q[0]) << np.uint32(2)) | (_expand_bits(q[1]) << np.uint32(1)) | _expand_bits(q[2])


def sorted_prims(v0, v1, v2):
    """(box min, box max, sorted codes, order): order[p] = the input triangle at sorted position p."""
    mn, mx, cen = prim_boxes(v0, v1, v2)
    code = morton_codes(cen)
    order = np.argsort(code, kind="stable")
    return mn, mx, code[order], order


def tri_records(arrays, tri_f4=3):
    """The intersection records of a scene in storage (scene) order: (v0.xyz, e1.x) (e1.yz, e2.xy)
    (e2.z, id, 0, 0) [pad], edges as float32 differences."""
    p0, p1, p2 = (np.ascontiguousarray(arrays[k], F).reshape(-1, 3) for k in ("v0", "v1", "v2"))
    with np.errstate(over="ignore", invalid="ignore"):
        e1, e2 = p1 - p0, p2 - p0
    n = len(p0)
    ids = np.asarray(arrays["tri_id"], np.int32) if len(arrays.get("tri_id", ())) else np.arange(n, dtype=np.int32)
    rec = np.zeros((n, tri_f4, 4), F)
    rec[:, 0, :3] = p0
    rec[:, 0, 3] = e1[:, 0]
    rec[:, 1, 0], rec[:, 1, 1], rec[:, 1, 2], rec[:, 1, 3] = e1[:, 1], e1[:, 2], e2[:, 0], e2[:, 1]
    rec[:, 2, 0] = e2[:, 2]
    rec.view(np.int32)[:, 2, 1] = ids
    return rec


def _emit(cmn, cmx, refs):
    """Child-pair nodes from per-node child boxes (m, 2, 3) and refs (m, 2): 4 x float4 per node, per
    axis (mn0, mn1, mx0, mx1), then (ref0, ref1, margin0 = 0, margin1 = 0)."""
    m = len(refs)
    nodes = np.zeros((m, 4, 4), F)
    for a in range(3):
        nodes[:, a, 0], nodes[:, a, 1] = cmn[:, 0, a], cmn[:, 1, a]
        nodes[:, a, 2], nodes[:, a, 3] = cmx[:, 0, a], cmx[:, 1, a]
    nodes.view(np.int32)[:, 3, :2] = refs
    return nodes


def _leaf_ref(pos):
    return (np.asarray(pos, np.int64) | LEAF_BIT).astype(np.uint32).view(np.int32)


def _single_leaf(mn, mx, order):
    return {"nodes": np.zeros((0, 4, 4), F), "root_ref": int(np.int32(-(1 << 31))), "depth": 0, "npairs": 0, "rounds": 0,
            "root_mn": mn[order[0]].copy(), "root_mx": mx[order[0]].copy(), "order": order}


# ---------------------------------------------------------------------------------------------
# LBVH
def _msb(x):
    """Index of the highest set bit of every (non-zero) uint64."""
    x = x.copy()
    r = np.zeros(x.shape, np.int64)
    for s in (32, 16, 8, 4, 2, 1):
        hi = x >> np.uint64(s)
        m = hi != 0
        r[m] += s
        x = np.where(m, hi, x)
    return r


def radix_children(code_sorted):
    """The binary radix tree over the keys (code << 32) | position, top-down.  A node covers a range
    [lo, hi] of sorted positions; it splits after the last key whose bit at the range's highest differing
    position is 0.  Numbering as Karras' construction implies: the root is 0 and, for a split at g, an
    interior left child is node g and an interior right child node g + 1.  Children are encoded as in
    k_karras: interior k -> k, leaf k -> (n - 1) + k.  Returns (child (n - 1, 2), levels: the node indices
    of every tree level, root first)."""
    n = len(code_sorted)
    keys = (code_sorted.astype(np.uint64) << np.uint64(32)) | np.arange(n, dtype=np.uint64)
    child = np.full((n - 1, 2), -1, np.int64)
    node, lo, hi = np.zeros(1, np.int64), np.zeros(1, np.int64), np.full(1, n - 1, np.int64)
    levels = []
    while len(node):
        levels.append(node)
        b = _msb(keys[lo] ^ keys[hi]).astype(np.uint64)
        target = ((keys[lo] >> b) | np.uint64(1)) << b  # the range's common prefix, then a 1, then zeros
        g = np.searchsorted(keys, target, side="left").astype(np.int64) - 1  # last key below it
        assert ((g >= lo) & (g < hi)).all()
        lleaf, rleaf = g == lo, g + 1 == hi
        child[node, 0] = np.where(lleaf, (n - 1) + g, g)
        child[node, 1] = np.where(rleaf, (n - 1) + g + 1, g + 1)
        node = np.concatenate([g[~lleaf], g[~rleaf] + 1])
        lo, hi = np.concatenate([lo[~lleaf], g[~rleaf] + 1]), np.concatenate([g[~lleaf], hi[~rleaf]])
    return child, levels


def karras_children(code_sorted):
    """Karras 2012, Fig. 4, one interior node at a time (the second formulation; small inputs)."""
    n = len(code_sorted)
    keys = [(int(c) << 32) | p for p, c in enumerate(code_sorted)]

    def delta(i, j):
        return -1 if j < 0 or j >= n else 64 - (keys[i] ^ keys[j]).bit_length()

    child = np.zeros((n - 1, 2), np.int64)
    for i in range(n - 1):
        d = 1 if delta(i, i + 1) - delta(i, i - 1) >= 0 else -1
        dmin = delta(i, i - d)
        lmax = 2
        while delta(i, i + lmax * d) > dmin:
            lmax *= 2
        l, t = 0, lmax // 2
        while t >= 1:
            if delta(i, i + (l + t) * d) > dmin:
                l += t
            t //= 2
        j = i + l * d
        dnode = delta(i, j)
        s, t = 0, l
        while True:
            t = (t + 1) // 2
            if delta(i, i + (s + t) * d) > dnode:
                s += t
            if t <= 1:
                break
        g = i + s * d + min(d, 0)
        child[i, 0] = (n - 1) + g if min(i, j) == g else g
        child[i, 1] = (n - 1) + g + 1 if max(i, j) == g + 1 else g + 1
    return child


def lbvh(v0, v1, v2):
    """The LBVH upload's pair tree: nodes in k_emit's layout (leaf refs 0x80000000 | sorted position),
    exact min / max union boxes, depth = the root's height (interior nodes on the longest path)."""
    mn, mx, code, order = sorted_prims(v0, v1, v2)
    n = len(order)
    if n == 1:
        return _single_leaf(mn, mx, order)
    child, levels = radix_children(code)
    leaf = child >= n - 1
    bmn, bmx = np.zeros((n - 1, 3), F), np.zeros((n - 1, 3), F)
    height = np.zeros(n - 1, np.int64)
    cmn, cmx = np.zeros((n - 1, 2, 3), F), np.zeros((n - 1, 2, 3), F)
    for lv in reversed(levels):  # children before parents
        for k in range(2):
            c, lf = child[lv, k], leaf[lv, k]
            prim = order[np.where(lf, c - (n - 1), 0)]
            ci = np.where(lf, 0, c)
            cmn[lv, k] = np.where(lf[:, None], mn[prim], bmn[ci])
            cmx[lv, k] = np.where(lf[:, None], mx[prim], bmx[ci])
        bmn[lv], bmx[lv] = np.fmin(cmn[lv, 0], cmn[lv, 1]), np.fmax(cmx[lv, 0], cmx[lv, 1])
        hc = np.where(leaf[lv], 0, height[np.where(leaf[lv], 0, child[lv])])
        height[lv] = 1 + hc.max(axis=1)
    refs = np.where(leaf, _leaf_ref(np.where(leaf, child - (n - 1), 0)), child.astype(np.int32))
    return {"nodes": _emit(cmn, cmx, refs), "root_ref": 0, "depth": int(height[0]), "npairs": n - 1, "rounds": 0,
            "root_mn": bmn[0].copy(), "root_mx": bmx[0].copy(), "order": order, "child": child}


# ---------------------------------------------------------------------------------------------
# PLOC
def _half_area(amn, amx, bmn, bmx):
    with np.errstate(over="ignore", invalid="ignore"):
        d = np.fmax(amx, bmx) - np.fmin(amn, bmn)
        dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
        return (dx * dy + dy * dz) + dz * dx


def ploc_layout(n):
    """Locality numbering bvh_build.hip picks: sibling pairs (1) for trees of at most 2 MiB of 64-byte
    nodes, plain depth-first (0) beyond."""
    return 1 if (n - 1) * 64 <= (2 << 20) else 0


def relabel(raw_refs, count, layout):
    """New index of every raw node (root = raw node 0 -> 0), from the definitions:
    layout 0, depth-first: a node's interior children at p + 1 and p + 1 + count(first child);
    layout 1, depth-first by sibling pairs: a node's interior children side by side at the start of its
    descendants' range, then the first child's descendants, then the second's.
    count[k] = interior nodes in raw node k's subtree (itself included)."""
    m = len(raw_refs)
    new = np.full(m, -1, np.int64)
    new[0] = 0
    stack = [(0, 1)]  # (raw node, start of its descendants' range)
    while stack:
        k, ds = stack.pop()
        kids = [int(c) for c in raw_refs[k] if c >= 0]
        if layout == 0:
            nxt = new[k] + 1
            for c in kids:
                new[c] = nxt
                stack.append((c, nxt + 1))
                nxt += count[c]
        else:
            sub = ds + len(kids)
            for t, c in enumerate(kids):
                new[c] = ds + t
                stack.append((c, sub))
                sub += count[c] - 1
    return new


def ploc(v0, v1, v2, layout=None):
    """The PLOC upload's pair tree.  Clusters start as one leaf per triangle in Morton order.  Each round
    every cluster picks, among the clusters within 16 positions, the one minimising (half-area of the
    union box dx*dy + dy*dz + dz*dx in float32 with NaN counted as +inf, index distance, parity of the
    lower index, lower index); mutual pairs merge into raw node top - rank (rank in position order, top
    counting down from n - 2, so the last merge is raw node 0) with the lower position as first child;
    the survivors are compacted in order.  Then the raw nodes get the locality numbering."""
    mn, mx, _, order = sorted_prims(v0, v1, v2)
    n = len(order)
    if n == 1:
        return _single_leaf(mn, mx, order)
    cref = _leaf_ref(np.arange(n))
    cmn, cmx = mn[order].copy(), mx[order].copy()
    hgt, cnt = np.zeros(n, np.int64), np.zeros(n, np.int64)
    raw_mn, raw_mx = np.zeros((n - 1, 2, 3), F), np.zeros((n - 1, 2, 3), F)
    raw_refs, count = np.zeros((n - 1, 2), np.int32), np.zeros(n - 1, np.int64)
    top, rounds = n - 2, 0
    offs = np.array([d for d in range(-PLOC_RADIUS, PLOC_RADIUS + 1) if d != 0], np.int64)
    while len(cref) > 1:
        nc = len(cref)
        i = np.arange(nc, dtype=np.int64)[:, None]
        j = i + offs[None, :]
        valid = (j >= 0) & (j < nc)
        jc = np.clip(j, 0, nc - 1)
        area = _half_area(cmn[:, None, :], cmx[:, None, :], cmn[jc], cmx[jc])
        area = np.where(np.isnan(area), F(np.inf), area)
        lower = np.minimum(i, jc).astype(np.uint64)
        key = (np.abs(offs)[None, :].astype(np.uint64) << np.uint64(32)) | ((lower & np.uint64(1)) << np.uint64(31)) | (lower >> np.uint64(1))
        key = np.where(valid, key, np.uint64(1) << np.uint64(63))
        best = np.where(valid, area, F(np.inf)).min(axis=1)
        cand = valid & (area == best[:, None])
        pick = np.where(cand, key, np.uint64(0xFFFFFFFFFFFFFFFF)).argmin(axis=1)
        nn = jc[np.arange(nc), pick]
        assert valid[np.arange(nc), pick].all()
        idx = np.arange(nc)
        mutual = nn[nn] == idx
        merge, absorbed = mutual & (idx < nn), mutual & (idx > nn)
        nm = int(merge.sum())
        assert nm > 0, "no mutual pair: the pair order is not strict"
        a = idx[merge]
        b = nn[a]
        k = top - np.arange(nm)  # rank = position order of the lower cluster
        raw_mn[k, 0], raw_mn[k, 1], raw_mx[k, 0], raw_mx[k, 1] = cmn[a], cmn[b], cmx[a], cmx[b]
        raw_refs[k, 0], raw_refs[k, 1] = cref[a], cref[b]
        h = np.minimum(np.maximum(hgt[a], hgt[b]) + 1, 255)
        c = cnt[a] + cnt[b] + 1
        count[k] = c
        cref, hgt, cnt = cref.copy(), hgt.copy(), cnt.copy()
        cmn, cmx = cmn.copy(), cmx.copy()
        cmn[a], cmx[a] = np.fmin(raw_mn[k, 0], raw_mn[k, 1]), np.fmax(raw_mx[k, 0], raw_mx[k, 1])
        cref[a], hgt[a], cnt[a] = k.astype(np.int32), h, c
        keep = ~absorbed
        cref, hgt, cnt, cmn, cmx = cref[keep], hgt[keep], cnt[keep], cmn[keep], cmx[keep]
        top -= nm
        rounds += 1
    assert top == -1 and cref[0] == 0
    layout = ploc_layout(n) if layout is None else layout
    new = relabel(raw_refs, count, layout)
    assert sorted(new) == list(range(n - 1))
    refs = np.where(raw_refs >= 0, new[np.where(raw_refs >= 0, raw_refs, 0)].astype(np.int32), raw_refs)
    nodes = np.zeros((n - 1, 4, 4), F)
    nodes[new] = _emit(raw_mn, raw_mx, refs)
    return {"nodes": nodes, "root_ref": 0, "depth": int(hgt[0]), "npairs": n - 1, "rounds": rounds, "layout": layout,
            "root_mn": cmn[0].copy(), "root_mx": cmx[0].copy(), "order": order}


BUILDERS = {"lbvh": lbvh, "ploc": ploc}


def ref_info(ref, ntri, layout=0, width=2, gpu_built=1, cull_p=0.0):
    """An info dict for check_tree from a reference build (the fields mcpt_debug_bvh_read reports)."""
    return {"npairs": ref["npairs"], "root_ref": ref["root_ref"], "depth": ref["depth"], "width": width, "layout": layout,
            "ntri": ntri, "tri_f4": 3, "gpu_built": gpu_built, "rounds": ref["rounds"], "root_mn": ref["root_mn"],
            "root_mx": ref["root_mx"], "cull_p": F(cull_p)}


# ---------------------------------------------------------------------------------------------
# the checker
def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def node_views(nodes):
    """(child box min (m, 2, 3), child box max (m, 2, 3), refs (m, 2) int32, margins (m, 2)) of a node array."""
    nodes = np.ascontiguousarray(nodes, F).reshape(-1, 4, 4)
    cmn = np.stack([nodes[:, :3, 0], nodes[:, :3, 1]], axis=1)
    cmx = np.stack([nodes[:, :3, 2], nodes[:, :3, 3]], axis=1)
    refs = nodes.view(np.int32)[:, 3, :2].copy()
    return cmn, cmx, refs, nodes[:, 3, 2:].copy()


def leaf_range(ref):
    u = np.asarray(ref, np.int32).view(np.uint32).astype(np.int64)
    return u & 0xFFFFFF, ((u >> 24) & 7) + 1


def tree_levels(refs, root_ref):
    """Node indices by level from the root (breadth-first); asserts that no node is reached twice."""
    m = len(refs)
    seen = np.zeros(m, np.int64)
    levels = []
    front = np.array([root_ref], np.int64) if root_ref >= 0 else np.zeros(0, np.int64)
    while len(front):
        assert ((front >= 0) & (front < m)).all(), "interior ref out of range"
        np.add.at(seen, front, 1)
        assert (seen[front] == 1).all(), "a node is reached more than once"
        levels.append(front)
        kids = refs[front].reshape(-1)
        front = kids[kids >= 0].astype(np.int64)
    return levels, seen


def tri_position_of_id(arrays, ids):
    """Scene-array position of every triangle id (tri_id is a permutation of the positions)."""
    n = len(arrays["v0"])
    tid = np.asarray(arrays["tri_id"], np.int64) if len(arrays.get("tri_id", ())) else np.arange(n)
    inv = np.full(int(tid.max()) + 1 if n else 0, -1, np.int64)
    inv[tid] = np.arange(n)
    ids = np.asarray(ids, np.int64)
    assert ((ids >= 0) & (ids < len(inv))).all() and (inv[ids] >= 0).all(), "unknown triangle id in a record"
    return inv[ids]


def expected_margins(refs, root_ref, rec_w):
    """Per child the largest W'_T over the triangle records beneath it (rec_w: per record)."""
    levels, _ = tree_levels(refs, root_ref)
    exp = np.zeros(refs.shape, F)
    for lv in reversed(levels):
        r = refs[lv]
        inner = r >= 0
        w = np.where(inner, exp[np.where(inner, r, 0)].max(axis=2), F(0.0)).astype(F)
        off, cnt = leaf_range(r)
        for t in range(8):
            use = (~inner) & (r != K_END) & (t < cnt) & (off + t < len(rec_w))
            w = np.where(use, np.fmax(w, rec_w[np.where(use, off + t, 0)]), w)
        exp[lv] = w
    return exp


def check_tree(nodes, tris, info, arrays, margins=None):
    """Assert the invariants of an uploaded pair tree (device- or host-built).  nodes / tris / info as
    PathTracer.bvh_read() returns them, arrays as Scene.arrays().  margins: oracle.model_margins(arrays)
    (its "tri_w" in scene-array order and "p"); None skips the margin part."""
    cmn, cmx, refs, marg = node_views(nodes)
    m, ntri = len(refs), int(info["ntri"])
    tris = np.ascontiguousarray(tris, F).reshape(ntri, int(info["tri_f4"]), 4)
    root = int(info["root_ref"])
    assert m == int(info["npairs"]) and ntri == len(arrays["v0"])
    root_mn, root_mx = np.asarray(info["root_mn"], F), np.asarray(info["root_mx"], F)
    assert int(info["depth"]) <= K_MAX_STACK
    if ntri == 0:
        assert m == 0 and root == 0 and int(info["depth"]) == 0
        return
    ids = tris.view(np.int32)[:, 2, 1]
    pos = tri_position_of_id(arrays, ids)
    assert len(np.unique(ids)) == ntri, "a triangle id appears in two records"
    verts = np.stack([np.asarray(arrays[k], F).reshape(-1, 3)[pos] for k in ("v0", "v1", "v2")], axis=1)  # per record

    # reachability: every node exactly once, pads (layout 3 only) never
    levels, seen = tree_levels(refs, root)
    pad = (refs == K_END).all(axis=1)
    assert np.array_equal(seen, (~pad).astype(np.int64)), "a node is unreachable, or a pad node is referenced"
    assert not (refs[~pad] == K_END).any(), "a reachable node has an empty child"
    assert int(info["layout"]) == 3 or not pad.any(), "pad nodes outside layout 3"

    # leaves: ranges inside the triangle array, disjoint, covering every record once
    live = refs[~pad]
    leaf_refs = np.concatenate([live[live < 0], np.array([root], np.int32)[:1 if root < 0 else 0]])
    off, cnt = leaf_range(leaf_refs)
    assert (off + cnt <= ntri).all(), "leaf range outside the triangle array"
    cover = np.zeros(ntri + 8, np.int64)
    for t in range(8):
        np.add.at(cover, off[cnt > t] + t, 1)
    assert (cover[:ntri] == 1).all(), "a triangle record is in no leaf or in two"
    if int(info["gpu_built"]):
        assert m == ntri - 1 and (cnt == 1).all(), "device trees have ntri - 1 nodes and one triangle per leaf"

    # the reported depth is the true height: interior nodes on the longest root-to-leaf path
    assert int(info["depth"]) == len(levels), f"reported depth {info['depth']}, true height {len(levels)}"

    if root < 0:  # the whole tree is one leaf: the root box is its box
        o, c = leaf_range(np.int32(root))
        v = verts[int(o):int(o) + int(c)].reshape(-1, 3)
        assert (v >= root_mn).all() and (v <= root_mx).all(), "root leaf box misses a vertex"
    else:
        live_idx = np.flatnonzero(~pad)
        for k in range(2):
            r = refs[live_idx, k]
            inner = r >= 0
            # a leaf's box contains its triangles' vertices
            lo, lc = leaf_range(r[~inner])
            bmn, bmx = cmn[live_idx[~inner], k], cmx[live_idx[~inner], k]
            for t in range(8):
                use = lc > t
                v = verts[lo[use] + t]
                assert (v >= bmn[use][:, None, :]).all() and (v <= bmx[use][:, None, :]).all(), "leaf box misses a vertex"
            # an interior child's box is the union of that node's two child boxes, bit for bit
            ci = r[inner]
            umn, umx = np.fmin(cmn[ci, 0], cmn[ci, 1]), np.fmax(cmx[ci, 0], cmx[ci, 1])
            assert np.array_equal(_bits(cmn[live_idx[inner], k]), _bits(umn)), "interior box min is not its children's union"
            assert np.array_equal(_bits(cmx[live_idx[inner], k]), _bits(umx)), "interior box max is not its children's union"
            # ... and lies inside the root box
            assert (cmn[live_idx[inner], k] >= root_mn).all() and (cmx[live_idx[inner], k] <= root_mx).all(), "box outside the root box"
        assert np.array_equal(_bits(root_mn), _bits(np.fmin(cmn[root, 0], cmn[root, 1]))), "root box min"
        assert np.array_equal(_bits(root_mx), _bits(np.fmax(cmx[root, 0], cmx[root, 1]))), "root box max"

    if margins is not None:
        rec_w = np.asarray(margins["tri_w"], F)[pos]
        exp = expected_margins(refs, root, rec_w)
        bad = _bits(marg) != _bits(exp)
        bad[pad] = False
        assert not bad.any(), (f"{int(bad.sum())} margin words differ from their subtree maxima, first at node "
                               f"{int(np.argwhere(bad)[0][0])}: {marg[bad][0]!r} != {exp[bad][0]!r}")
        assert _bits(info["cull_p"]) == _bits(F(margins["p"])), f"P {info['cull_p']!r} != {F(margins['p'])!r}"


def leaf_table(nodes, info):
    """Rows (offset, count, box min bits, box max bits, margin bits) of every leaf, sorted by offset, and
    the sorted rows (box bits, margin bits) of every interior child: what a renumbering must not change."""
    cmn, cmx, refs, marg = node_views(nodes)
    pad = (refs == K_END).all(axis=1)
    rows = np.concatenate([refs.view(np.uint32)[..., None].astype(np.int64), _bits(cmn).astype(np.int64),
                           _bits(cmx).astype(np.int64), _bits(marg)[..., None].astype(np.int64)], axis=2)[~pad].reshape(-1, 8)
    leaf = rows[:, 0] >= LEAF_BIT
    lr = rows[leaf]
    off, cnt = lr[:, 0] & 0xFFFFFF, ((lr[:, 0] >> 24) & 7) + 1
    leaves = np.concatenate([off[:, None], cnt[:, None], lr[:, 1:]], axis=1)
    leaves = leaves[np.argsort(leaves[:, 0], kind="stable")]
    inner = rows[~leaf][:, 1:]
    inner = inner[np.lexsort(inner.T[::-1])]
    return leaves, inner


# ---------------------------------------------------------------------------------------------
# input families (vertices (n, 3, 3) float32), the smallest that reach each edge of the builders
def random_tris(n, seed=0, size=0.1):
    rng = np.random.default_rng(1000 + seed + n)
    c = rng.uniform(-1, 1, (n, 1, 3))
    return np.clip(c + rng.uniform(-size, size, (n, 3, 3)), -1, 1).astype(F)


def coincident_tris(n=300):
    return np.repeat(random_tris(1, seed=7, size=0.5), n, axis=0)


def lattice_tris(n=600):
    """Small triangles whose centroids sit exactly on a 4 x 4 x 4 lattice: many equal Morton codes."""
    rng = np.random.default_rng(11)
    cell = rng.integers(0, 4, (n, 3))
    c = (cell.astype(F) * F(0.5) - F(0.75))[:, None, :]   # exact in float32
    d = (rng.integers(1, 8, (n, 1, 3)).astype(F) * F(2.0 ** -7))
    # vertices c - d, c + d, and a third inside their box: box centre = c exactly
    third = c + d * rng.choice(np.float32([-0.5, 0.0, 0.5]), (n, 1, 3))
    return np.concatenate([c - d, c + d, third], axis=1).astype(F)


def planar_tris(n=200):
    """Every centroid in the plane z = 0.25 (zero centroid extent on one axis)."""
    v = random_tris(n, seed=3)
    h = (np.random.default_rng(5).integers(1, 9, n).astype(F) * F(2.0 ** -6))[:, None]
    v[:, :, 2] = F(0.25) + h * np.float32([-1.0, 1.0, 0.0])[None, :]
    return v


def chain_tris(per=5):
    """Centroids at (2^-k, 0, 0), k = 0..23, `per` triangles each (all values exact in float32).  The
    y and z extents are 0, so the codes come from x alone: cells 1023, 511, 255, ..., 1 for k = 0..9
    ((2^-k - m) / (1 - m) * 1024 with m = 2^-23 lies just below 2^(10-k)) and 0 for k >= 10.  The radix
    tree peels one cell off per level for ten levels, then orders the 14 * per = 70 equal codes by position
    (seven more levels): 17 in all, one more than build_lbvh's first batch of 16 bottom-up passes."""
    rng = np.random.default_rng(13)
    out = []
    for k in range(24):
        x = F(2.0 ** -k)
        for _ in range(per):
            d = x * F(2.0 ** -4) * F(rng.integers(1, 4))
            w = F(2.0 ** -6) * F(rng.integers(1, 9))
            out.append([[x - d, -w, w], [x + d, w, -w], [x, 0, 0]])
    return np.array(out, F)


def huge_tris():
    """Triangles spanning about +-3e38 on x and flat in z: the union extent overflows to +inf on x and
    is 0 on z, so the half-area inf * 0 is NaN (k_ploc_nn's NaN branch)."""
    b = F(3.0e38)
    v = [[[-b, 0, 0], [b, 1, 0], [0, 2, 0]],
         [[-b, 1, 0], [b, 2, 0], [0, 3, 0]],
         [[-b, -1, 0], [b, -3, 0], [0, 0, 0]],
         [[-b, 4, 0], [b, 5, 0], [0, 4.5, 0]],
         [[-b, 2, 0], [b, 2.5, 0], [0, 2.25, 0]]]
    return np.array(v, F)


def scene_of(mcpt_mod, v):
    """A built host scene of the triangles v (n, 3, 3): what the GPU tests upload."""
    s = mcpt_mod.Scene()
    nrm = np.tile(F([0, 0, 1]), (len(v), 1))
    s.add_mesh(v[:, 0], v[:, 1], v[:, 2], nrm, nrm, nrm, (0.5, 0.5, 0.5))
    s.set_env_color((1, 1, 1), 1.0)
    s.build(8)
    return s


SMALL_FAMILIES = {
    **{f"random{n}": (lambda n=n: random_tris(n)) for n in (1, 2, 3, 4, 5, 37, 255, 256, 257, 272, 273, 513)},
    "coincident300": coincident_tris,
    "lattice600": lattice_tris,
    "planar200": planar_tris,
    "chain": chain_tris,
    "huge": huge_tris,
}
LARGE_PLOC = {f"random{n}": (lambda n=n: random_tris(n, size=0.02)) for n in (32769, 32770)}
