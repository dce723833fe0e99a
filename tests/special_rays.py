"""Axis-aligned, nearly axis-aligned and non-finite rays for the traversal's second box test.

k_trace tests boxes with packed arithmetic when the ray's inverse direction is finite in all three
components, and with slab() (csrc/kernels.hip, the reference's sign-selected test, Bounds3f.h:121-153)
when it is not.  In slab() a NaN product (0 * inf: an origin exactly on a box plane of an axis the ray
does not move along) compares false and passes.  Around that path stand cull_iota (-inf for such rays,
-FLT_MAX for |d|^2 > kCullNormMax, an overflow to +inf for a finite inverse next to FLT_MAX), keep_box
(a NaN margin), the 4-wide sort's NaN keys, the occluder cache's `fin` test and k_shade's
ray_misses_scene.  tests/adversarial.py and random_rays never produce a zero direction component;
special_rays() produces little else.

special_rays(a, m, seed, planes=None) -> (ro, rd, cls): float32 (m, 3), float32 (m, 3), int (m).

Most rays (85 %) are aimed: a point q inside a random triangle, a direction of the ray's class made
front-facing for that triangle (d . (e1 x e2) < 0), the origin t * |d| behind q, t in [0.005, 0.3] of
the root box's largest extent (0.05 .. 3 units on the 10 x 10 floor scene).  The others start anywhere
in 1.5 x the root box.  The zeroed axes are chosen at random, with a preference (0.7) for the ones that
leave the direction a component along the triangle's normal.

Classes (cls), in equal parts (the last one small):

  0 ZERO1      one direction component exactly zero, the other two renormalised.  The zero's sign is
               random: +0.0 (inverse +inf) or -0.0 (inverse -inf, the reference's dirIsNeg true).
  1 ZERO2      two components exactly zero, signs random, the third +-1.
  2 ON_PLANE   ZERO1 / ZERO2 (half each) with the origin coordinate of every zero axis set exactly to
               a coordinate of `planes` ((k, 3) points; by default the scene's vertices, whose
               coordinates are the leaf-box planes of every builder's tree and, through the unions,
               planes of their ancestors; for a read-back tree pass tree_planes(pt.bvh_read()[0])):
               the slab product of that plane is 0 * inf = NaN.  The coordinate is the one next to
               q's in sorted order, or up to two further, so the ray still passes by q.
  3 SUBNORMAL  the zeros replaced by signed subnormals, |d_a| in [1e-45, 2.5e-39]: not zero, but
               1 / d_a overflows to +-inf.
  4 TINY       the zeros replaced by signed |d_a| in [2^-128 (1 + 2^-21), 1e-30]: 1 / d_a is finite.
               A quarter take |d_a| = (2^21 + k) 2^-149, k = 1..8: max |1/d| (1 + 2^-18), cull_iota's
               product, overflows although the inverse is finite.  A third have on-plane origins
               (0 * finite = +-0).
  5 SCALED     any of classes 0..4 with the direction multiplied by a length: log-uniform in
               [1e-3, 1e3], or (a third) one of 1 - 2^-9, 1 + 2^-11, 1 + 2^-10, 1 + 2^-9 around
               kCullNormMax (|d|^2 <= 1 + 2^-9), whose far side takes cull_iota's -FLT_MAX branch.
  6 NONFINITE  any of classes 0..4 with one origin component NaN, +inf, -inf, +1e30 or -1e30, or one
               direction component NaN, +inf or -inf, or the direction all zeros with mixed signs.
               A NaN origin passes every box and visits the whole tree, so this class has at most
               NONFINITE_MAX rays and is left out for scenes of more than NONFINITE_TRIS triangles.

Measured shares (200,000 rays, seed 1).  Per class 0..6 the share the oracle's closest trace hits; the
share its any-hit trace finds occluded is the same to two digits (both traces run to infinity).  NaN:
the share of ON_PLANE rays with a NaN slab product against at least one box of the scene's desc tree.
8,215 TINY rays of each batch have a scale that overflows (iota_overflows).

                    zero1 zero2 on_plane subnormal tiny scaled nonfinite   NaN
  floor scene        0.87  0.87   0.83     0.87    0.85  0.85    0.04     1.000
  config 2 x1        0.91  0.90   0.91     0.90    0.90  0.90    0.16     0.990
  config 2 x1e3      0.91  0.90   0.91     0.90    0.90  0.90    0.16     0.987
  config 2 x1e-3     0.75  0.78   0.77     0.76    0.76  0.57    0.16     0.987

(At x1e-3 Moller-Trumbore's det threshold 1e-6 rejects the grazing and the short-direction rays.)
On an MI355X every one of these rays, under every tree and kernel variant of
tests/test_special_rays.py, gets the oracle's answer on the tree the device holds, bit for bit; one
ray in 120,000 of the floor scene's batch has an answer that belongs to the tree (tree_arrays()).
"""
from __future__ import annotations

import numpy as np

F = np.float32
ZERO1, ZERO2, ON_PLANE, SUBNORMAL, TINY, SCALED, NONFINITE = range(7)
CLASS_NAMES = ("zero1", "zero2", "on_plane", "subnormal", "tiny", "scaled", "nonfinite")
NONFINITE_MAX = 3000    # rays of class 6 per call, at most
NONFINITE_TRIS = 5000   # ... and none for scenes with more triangles
AIMED = 0.85
SLACK = F(1.0) + F(2.0 ** -18)  # kCullSlackF: cull_iota's factor
NORM_LENGTHS = (1.0 - 2.0 ** -9, 1.0 + 2.0 ** -11, 1.0 + 2.0 ** -10, 1.0 + 2.0 ** -9)


def inverse(rd):
    """1 / d per component in float32, as the kernels and the reference form it."""
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        return (F(1.0) / np.ascontiguousarray(rd, F)).astype(F)


def nonfinite_inverse(rd):
    """Per ray: some inverse direction component is +-inf or NaN (the ray takes slab())."""
    return ~np.isfinite(inverse(rd)).all(axis=1)


def iota_overflows(rd):
    """Per ray: the inverse is finite and max_a |1 / d_a| (1 + 2^-18) overflows in float32."""
    inv = inverse(rd)
    with np.errstate(over="ignore", invalid="ignore"):
        io = (np.abs(inv).max(axis=1) * SLACK).astype(F)
    return np.isfinite(inv).all(axis=1) & np.isinf(io)


def nan_product(ro, rd, bmin, bmax):
    """Per ray: some box (bmin, bmax (N, 3)) has a NaN slab product, (plane - o_a) * (1 / d_a) with an
    infinite inverse and the origin exactly on the plane (0 * inf)."""
    ro = np.ascontiguousarray(ro, F)
    inv = inverse(rd)
    out = np.zeros(len(ro), bool)
    for ax in range(3):
        pl = np.unique(np.concatenate([np.asarray(bmin, F).reshape(-1, 3)[:, ax], np.asarray(bmax, F).reshape(-1, 3)[:, ax]]))
        out |= np.isinf(inv[:, ax]) & np.isin(ro[:, ax], pl)
    return out


def tree_planes(nodes):
    """The box planes of a read-back tree (PathTracer.bvh_read()'s nodes (npairs, 4, 4): per axis
    (mn0, mn1, mx0, mx1)) as (k, 3) points for special_rays(planes=...); pad nodes' non-finite planes
    are dropped."""
    nodes = np.ascontiguousarray(nodes, F).reshape(-1, 4, 4)
    p = nodes[:, :3, :].transpose(0, 2, 1).reshape(-1, 3)
    return p[np.isfinite(p).all(axis=1)]


def tree_arrays(a, nodes, tris, info):
    """The scene arrays `a` under the tree the device holds (PathTracer.bvh_read()), as a desc tree the
    oracle traverses: triangles in storage order, one desc node per child box, first child at i + 1.

    The reference's box test lets a NaN product pass, so a box can pass for a ray that misses its
    ancestors, and which triangles such a ray reaches depends on the boxes above them: on these rays
    the reference's answer belongs to a tree, and the product's is checked against the oracle on the
    product's own tree.  4-wide nodes (info["width"] == 4, csrc/host/pair_tree.cpp pairs_to_quads: a
    4-wide node is a pair node at even depth, its slots the children of its two children) never test
    the box of an interior child of such a pair node; that box becomes (-inf, +inf), which passes
    for every ray."""
    import bvh_ref as R

    nodes = np.ascontiguousarray(nodes, F).reshape(-1, 4, 4)
    tris = np.ascontiguousarray(tris, F).reshape(int(info["ntri"]), int(info["tri_f4"]), 4)
    order = R.tri_position_of_id(a, tris[:, 2, 1].copy().view(np.int32))
    cmn, cmx, refs, _ = R.node_views(nodes)
    quad = int(info["width"]) == 4
    inf3 = np.full(3, np.inf, F)
    bmin, bmax, offset, nprims = [], [], [], []

    def rec(ref, mn, mx, quad_root):
        i = len(offset)
        bmin.append(mn), bmax.append(mx), offset.append(0), nprims.append(0)
        if ref < 0:
            off, cnt = R.leaf_range(np.int32(ref))
            offset[i], nprims[i] = int(off), int(cnt)
            return
        for k in range(2):
            c = int(refs[ref, k])
            if k == 1:
                offset[i] = len(offset)
            if quad and quad_root and c >= 0:
                rec(c, -inf3, inf3, False)
            else:
                rec(c, cmn[ref, k], cmx[ref, k], True)

    rec(int(info["root_ref"]), np.asarray(info["root_mn"], F), np.asarray(info["root_mx"], F), True)  # (depth <= 64)
    b = dict(a)
    for k in ("v0", "v1", "v2", "n0", "n1", "n2", "mat", "tri_id"):
        b[k] = np.ascontiguousarray(np.asarray(a[k])[order])
    b["bmin"], b["bmax"] = np.array(bmin, F).reshape(-1, 3), np.array(bmax, F).reshape(-1, 3)
    b["offset"], b["nprims"] = np.array(offset, np.int32), np.array(nprims, np.int32)
    b["axis"] = np.zeros(len(offset), np.int32)
    return b


def class_shares(cls, tri, vis):
    """Per class present: (name, rays, share hit by the closest trace, share occluded by the any-hit trace)."""
    out = []
    for c in np.unique(cls):
        k = cls == c
        out.append((CLASS_NAMES[c], int(k.sum()), float((tri[k] >= 0).mean()), float((vis[k] == 0).mean())))
    return out


def format_shares(cls, tri, vis):
    return " ".join(f"{n}:{h:.2f}/{o:.2f}" for n, _, h, o in class_shares(cls, tri, vis))


def _signed_zero(rng, n):
    return np.where(rng.random(n) < 0.5, -0.0, 0.0)


def _log_uniform(rng, lo, hi, n):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), n))


def _base(a, n, rng, kind):
    """n rays with zeroed direction components: kind 1 / 2 = that many zeros per ray (an array).
    Returns ro (float64), rd (float64, unit, exact signed zeros), zero mask (n, 3), q (the aim points)."""
    v0, v1, v2 = (np.asarray(a[k], np.float64).reshape(-1, 3) for k in ("v0", "v1", "v2"))
    mn, mx = np.asarray(a["bmin"], np.float64).reshape(-1, 3)[0], np.asarray(a["bmax"], np.float64).reshape(-1, 3)[0]
    ext = float(np.max(mx - mn))
    T = rng.integers(0, len(v0), n)
    e1, e2 = v1[T] - v0[T], v2[T] - v0[T]
    nrm = np.cross(e1, e2)
    ln = np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm = np.where(ln > 0, nrm / np.where(ln > 0, ln, 1.0), np.array([0.0, 1.0, 0.0]))
    u, v = rng.random(n), rng.random(n)
    flip = u + v > 1
    u[flip], v[flip] = 1 - u[flip], 1 - v[flip]
    q = v0[T] + u[:, None] * e1 + v[:, None] * e2
    aimed = rng.random(n) < AIMED
    # the axes to zero: a random order of the three, or (0.7) the normal's smallest components first
    order = np.argsort(rng.random((n, 3)), axis=1)
    by_n = np.argsort(np.abs(nrm) + 1e-9 * rng.random((n, 3)), axis=1)
    order = np.where((rng.random(n) < 0.7)[:, None], by_n, order)
    zero = np.zeros((n, 3), bool)
    r = np.arange(n)
    zero[r, order[:, 0]] = True
    two = kind == 2
    zero[r[two], order[two, 1]] = True
    d = rng.normal(size=(n, 3))
    d[np.abs(d) < 1e-3] = 1e-3  # the kept components are not tiny by accident
    d[zero] = 0.0
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    back = np.sum(d * nrm, axis=1) > 0
    d[back] = -d[back]
    d = np.where(zero, _signed_zero(rng, (n, 3)), d)
    t = ext * rng.uniform(0.005, 0.3, n)
    o = q - t[:, None] * np.where(zero, 0.0, d)
    c, h = 0.5 * (mn + mx), 0.75 * (mx - mn)
    free = ~aimed
    o[free] = c + h * rng.uniform(-1.0, 1.0, (int(free.sum()), 3))
    q = np.where(aimed[:, None], q, o)
    return o, d, zero, q


def _snap(o, q, zero, planes, rng, sel):
    """Origins of the rays `sel` put exactly on a plane coordinate on each of their zero axes: the
    coordinate of `planes` next to q's in sorted order, or up to two places further."""
    o = o.copy()
    for ax in range(3):
        pl = np.unique(np.asarray(planes, F).reshape(-1, 3)[:, ax])
        pl = pl[np.isfinite(pl)]
        k = np.nonzero(sel & zero[:, ax])[0]
        if not len(pl) or not len(k):
            continue
        i = np.searchsorted(pl, q[k, ax].astype(F)) + rng.integers(-2, 3, len(k))
        o[k, ax] = pl[np.clip(i, 0, len(pl) - 1)]
    return o


def _rays_of(a, n, rng, cls, planes):
    """float32 (ro, rd) of n rays of one class 0..4."""
    kind = {ZERO1: np.ones(n, int), ZERO2: np.full(n, 2)}.get(cls)
    if kind is None:
        kind = rng.integers(1, 3, n)
    o, d, zero, q = _base(a, n, rng, kind)
    if cls == ON_PLANE:
        o = _snap(o, q, zero, planes, rng, np.ones(n, bool))
    ro, rd = o.astype(F), d.astype(F)  # (a float32 plane coordinate survives the cast exactly)
    if cls == SUBNORMAL:
        mag = np.maximum(_log_uniform(rng, 1e-45, 2.5e-39, (n, 3)).astype(F), F(1.4e-45))
        sub = (mag * np.where(rng.random((n, 3)) < 0.5, F(-1.0), F(1.0))).astype(F)
        rd = np.where(zero, sub, rd)
    if cls == TINY:
        lo = 2.0 ** -128 * (1.0 + 2.0 ** -21)
        mag = _log_uniform(rng, lo, 1e-30, (n, 3)).astype(F)
        mag = np.maximum(mag, F(lo))
        edge = rng.random(n) < 0.25
        near = ((2 ** 21 + rng.integers(1, 9, (n, 3))).astype(np.float64) * 2.0 ** -149).astype(F)
        mag = np.where(edge[:, None], near, mag)
        tiny = (mag * np.where(rng.random((n, 3)) < 0.5, F(-1.0), F(1.0))).astype(F)
        rd = np.where(zero, tiny, rd)
        on = rng.random(n) < 1.0 / 3.0
        ro = np.where(zero & on[:, None], _snap(o, q, zero, planes, rng, on).astype(F), ro)
    return ro, rd


def _mixed(a, n, rng, planes):
    """n rays drawn from classes 0..4 in equal parts (the material of SCALED and NONFINITE)."""
    parts = [_rays_of(a, len(idx), rng, c, planes) for c, idx in enumerate(np.array_split(np.arange(n), 5))]
    ro, rd = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    perm = rng.permutation(n)
    return ro[perm], rd[perm]


def special_rays(a, m, seed, planes=None):
    """m rays (ro, rd, cls) of the classes above on the scene arrays `a` (mcpt.Scene.arrays(): the
    triangles and the root box bmin[0] / bmax[0]); planes: (k, 3) points whose coordinates the
    on-plane origins take (default: a's vertices)."""
    rng = np.random.default_rng(seed)
    if planes is None:
        planes = np.concatenate([np.asarray(a[k], F).reshape(-1, 3) for k in ("v0", "v1", "v2")])
    n_nf = min(NONFINITE_MAX, m // 7) if len(a["v0"]) <= NONFINITE_TRIS else 0
    split = np.array_split(np.arange(m - n_nf), 6)
    ros, rds, cls = [], [], []
    for c in range(5):
        ro, rd = _rays_of(a, len(split[c]), rng, c, planes)
        ros.append(ro), rds.append(rd), cls.append(np.full(len(ro), c))
    # SCALED
    n = len(split[5])
    ro, rd = _mixed(a, n, rng, planes)
    length = _log_uniform(rng, 1e-3, 1e3, n)
    near1 = rng.random(n) < 1.0 / 3.0
    length[near1] = np.asarray(NORM_LENGTHS)[rng.integers(0, len(NORM_LENGTHS), int(near1.sum()))]
    with np.errstate(over="ignore", under="ignore"):
        rd = (rd * length.astype(F)[:, None]).astype(F)
    ros.append(ro), rds.append(rd), cls.append(np.full(n, SCALED))
    # NONFINITE
    if n_nf:
        ro, rd = _mixed(a, n_nf, rng, planes)
        what = rng.integers(0, 9, n_nf)
        ax = rng.integers(0, 3, n_nf)
        r = np.arange(n_nf)
        ovals = F([np.nan, np.inf, -np.inf, 1e30, -1e30])
        dvals = F([np.nan, np.inf, -np.inf])
        k = what < 5
        ro[r[k], ax[k]] = ovals[what[k]]
        k = (what >= 5) & (what < 8)
        rd[r[k], ax[k]] = dvals[what[k] - 5]
        k = what == 8
        rd[k] = _signed_zero(rng, (int(k.sum()), 3)).astype(F)
        ros.append(ro), rds.append(rd), cls.append(np.full(n_nf, NONFINITE))
    ro, rd, cls = np.concatenate(ros), np.concatenate(rds), np.concatenate(cls)
    perm = rng.permutation(len(ro))  # classes interleaved: a wave holds rays of both box tests
    return np.ascontiguousarray(ro[perm], F), np.ascontiguousarray(rd[perm], F), cls[perm].astype(np.int64)
