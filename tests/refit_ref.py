"""numpy references for the device BVH refit (csrc/refit.hip, mcpt_scene_update_geometry).

A refit keeps a tree's topology and recomputes its boxes from moved vertices:
* a leaf's box is the exact float32 min / max of its triangles' nine vertex components per axis;
* an interior node's box is the union of its two children's boxes.
min and max are exact, so no evaluation order changes a bit (signed zeros on box faces are not part
of the contract: the tests move every vertex off the coordinate planes).

refit_desc():  the bmin / bmax of a scene desc (flattened depth-first tree: a node's first child is
               i + 1, its second offset[i]; a leaf holds triangles offset[i] .. + nprims[i] - 1).
refit_nodes(): a bvh_ref child-pair node array under its storage order (record p holds scene
               triangle order[p]).
warp():        the smooth per-vertex warp plus a fixed offset the tests move meshes with.
"""
import numpy as np

import bvh_ref as R

F = np.float32
OFFSET = F([0.37, -0.21, 0.11])


def warp(v, amp=0.05, phase=0.0, offset=OFFSET):
    """v (..., 3) float32 -> v + amp * q(v; phase) + offset with a quadratic q per axis, in float32.  A
    function of the position alone, made of float32 multiplications and additions only (each
    correctly rounded wherever and however numpy evaluates it): a vertex shared by several triangles
    stays shared, and the same position moves to the same bits in whichever array it stands."""
    v = np.ascontiguousarray(v, F)
    x, y, z = v[..., 0], v[..., 1], v[..., 2]
    a, ph = F(amp), F(phase)
    with np.errstate(over="ignore", invalid="ignore"):
        d = np.stack([F(0.8) * y * y - F(0.6) * z + ph * F(0.3) * y,
                      F(0.7) * z * x + F(0.5) * x - ph * F(0.2) * z,
                      F(0.9) * x * x - F(0.4) * y * x + ph * F(0.1) * x], axis=-1).astype(F)
        return (v + a * d + np.asarray(offset, F)).astype(F)


def moved_arrays(a, **kw):
    """Scene arrays with every vertex through warp(); everything else (tree included) as it was."""
    m = dict(a)
    for k in ("v0", "v1", "v2"):
        m[k] = warp(a[k], **kw)
    return m


def refit_desc(a):
    """(bmin, bmax) of the desc tree of `a` refitted to a's vertices: nodes N-1 .. 0 (children follow
    their parent), a leaf's box the vertex union of its range, an interior node's its children's union."""
    N = len(a["nprims"])
    v = np.stack([np.ascontiguousarray(a[k], F).reshape(-1, 3) for k in ("v0", "v1", "v2")], axis=1)  # (T, 3, 3)
    bmin, bmax = np.zeros((N, 3), F), np.zeros((N, 3), F)
    for i in range(N - 1, -1, -1):
        n = int(a["nprims"][i])
        if n > 0:
            t = v[int(a["offset"][i]):int(a["offset"][i]) + n].reshape(-1, 3)
            bmin[i], bmax[i] = np.fmin.reduce(t, axis=0), np.fmax.reduce(t, axis=0)
        else:
            c0, c1 = i + 1, int(a["offset"][i])
            bmin[i], bmax[i] = np.fmin(bmin[c0], bmin[c1]), np.fmax(bmax[c0], bmax[c1])
    return bmin, bmax


def refitted_desc_arrays(a, **kw):
    """moved_arrays(a) with the desc tree's boxes refitted: what a fresh upload of the moved mesh in
    the same topology takes."""
    m = moved_arrays(a, **kw)
    m["bmin"], m["bmax"] = refit_desc(m)
    return m


def refit_nodes(nodes, root_ref, order, v0, v1, v2):
    """A child-pair node array (m, 4, 4) with the same refs and numbering and the boxes of the moved
    vertices (scene order; record p = triangle order[p]); margin words zero, pad nodes unchanged.
    Returns (nodes, root_mn, root_mx)."""
    nodes = np.ascontiguousarray(nodes, F).reshape(-1, 4, 4).copy()
    mn, mx, _ = R.prim_boxes(v0, v1, v2)
    rmn, rmx = mn[order], mx[order]  # per record
    _, _, refs, _ = R.node_views(nodes)

    def leaf_box(ref):
        off, cnt = R.leaf_range(np.int32(ref))
        return np.fmin.reduce(rmn[int(off):int(off) + int(cnt)], axis=0), np.fmax.reduce(rmx[int(off):int(off) + int(cnt)], axis=0)

    if root_ref < 0:
        return (nodes,) + leaf_box(root_ref)
    levels, _ = R.tree_levels(refs, root_ref)
    box = {}
    for lv in reversed(levels):
        for i in lv:
            cb = []
            for k in range(2):
                r = int(refs[i, k])
                cb.append(leaf_box(r) if r < 0 else box[r])
                for ax in range(3):
                    nodes[i, ax, k], nodes[i, ax, 2 + k] = cb[k][0][ax], cb[k][1][ax]
            nodes[i, 3, 2:] = 0
            box[int(i)] = (np.fmin(cb[0][0], cb[1][0]), np.fmax(cb[0][1], cb[1][1]))
    return (nodes,) + box[int(root_ref)]
