"""Reference for base-colour textures.

or_stage_material reads its triangle only through make_isect (vertices, normals, mat[id]) and never
touches the BVH, so a textured material stage is the oracle's own stage over an *exploded scene*: one
triangle and one material per path, the path's hit triangle with its material's parameters, whose base
colour is multiplied by the numpy texture lookup at the path's texture coordinate,

    tc   = (u * uv1 + v * uv2) + w * uv0         float32, per component, this order
    T    = lookup(texture of the material, tc)   device/texture.hpp restated below
    base = base_factor * T

with u, v the Moller-Trumbore coordinates of the stored ray on the hit triangle (uv_of: float32 products
in the oracle's order, the three quotients in double; it reproduces or_trace_closest's t and normal bit
for bit, tests/test_texture_host.py).  The rest of the loop is tests/emission_ref.py's.  With tex=None
the loop is oracle.render, bit for bit.

A texture set here is a dict {"uv0", "uv1", "uv2": (ntri, 2) float32 in the arrays' triangle order,
"textures": [(h, w, 3 or 4) uint8], "mat_tex": per material a texture index or -1}: the arguments of
PathTracer.set_textures."""
import numpy as np

from emission_ref import HASVIS

F = np.float32


def dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1).astype(F)


def normalize(x):
    l = np.sqrt(dot(x, x)).astype(F)
    with np.errstate(all="ignore"):
        return np.where(l[:, None] == 0, x, x / l[:, None]).astype(F)


def _v(a, k):
    return np.asarray(a[k], F).reshape(-1, 3)


def uv_of(a, tri, o, d):
    """Moller-Trumbore (u, v, t) of rays (o, d) on triangles tri (indices into the arrays of a), as
    tri_intersect forms them: float32 products, the three quotients of one determinant in double."""
    o, d = np.asarray(o, F).reshape(-1, 3), np.asarray(d, F).reshape(-1, 3)
    p0, p1, p2 = _v(a, "v0")[tri], _v(a, "v1")[tri], _v(a, "v2")[tri]
    e1, e2 = p1 - p0, p2 - p0
    with np.errstate(all="ignore"):
        pv = cross(d, e2)
        det = dot(e1, pv).astype(np.float64)
        tv = o - p0
        u = dot(tv, pv)
        qv = cross(tv, e1)
        v = dot(d, qv)
        t = dot(e2, qv)
        inv = 1.0 / det
        return ((u.astype(np.float64) * inv).astype(F), (v.astype(np.float64) * inv).astype(F),
                (t.astype(np.float64) * inv).astype(F))


def hit_normal(a, tri, u, v):
    """The hit record's normal: the interpolated vertex normal, normalised twice (Triangle.cu:76, 82)."""
    w = (F(1) - u) - v
    n = (_v(a, "n1")[tri] * u[:, None] + _v(a, "n2")[tri] * v[:, None]) + _v(a, "n0")[tri] * w[:, None]
    return normalize(normalize(n.astype(F)))


def tex_coord(tex, tri, u, v):
    """tc (n, 2) = (u * uv1 + v * uv2) + w * uv0, float32."""
    uv0, uv1, uv2 = (np.asarray(tex[k], F).reshape(-1, 2)[tri] for k in ("uv0", "uv1", "uv2"))
    w = (F(1) - u) - v
    with np.errstate(all="ignore"):
        return ((u[:, None] * uv1 + v[:, None] * uv2) + w[:, None] * uv0).astype(F)


def texels(img):
    """(h, w, 3) float32: byte / 255, correctly rounded (numpy's float32 division)."""
    return (np.asarray(img)[..., :3].astype(F) / F(255)).astype(F)


def q8(x):
    return (np.floor(x * F(256) + F(0.5)) * F(1 / 256)).astype(F)


def lookup(img, uv):
    """tex_bilinear_rgba8 (device/texture.hpp) in numpy float32: (n, 3) for uv (n, 2).  Wrap addressing,
    8-bit fractional weights, the sum ((w00 t00 + w10 t10) + w01 t01) + w11 t11; a coordinate that is NaN
    or at least 65536 in magnitude counts as 0."""
    T = texels(img)
    H, W = T.shape[:2]
    uv = np.asarray(uv, F).reshape(-1, 2)
    with np.errstate(all="ignore"):
        u = np.where(np.abs(uv[:, 0]) < F(65536), uv[:, 0], F(0)).astype(F)
        v = np.where(np.abs(uv[:, 1]) < F(65536), uv[:, 1], F(0)).astype(F)
    x = (u * F(W) - F(0.5)).astype(F)
    y = (v * F(H) - F(0.5)).astype(F)
    fx, fy = np.floor(x), np.floor(y)
    ax, ay = q8(x - fx), q8(y - fy)
    ix, iy = fx.astype(np.int64), fy.astype(np.int64)
    i0, i1, j0, j1 = ix % W, (ix + 1) % W, iy % H, (iy + 1) % H
    bx, by = F(1) - ax, F(1) - ay
    w00, w10, w01, w11 = bx * by, ax * by, bx * ay, ax * ay
    return (((w00[:, None] * T[j0, i0] + w10[:, None] * T[j0, i1]) + w01[:, None] * T[j1, i0]) +
            w11[:, None] * T[j1, i1]).astype(F)


def base_colour(a, tex, tri, o, d):
    """(n, 3) float32: the shaded base colour of rays (o, d) at their hits on triangles tri."""
    mat = np.asarray(a["mat"], np.int32)[tri]
    base = np.asarray(a["mat_params"], F).reshape(-1, 8)[mat, :3].copy()
    u, v, _ = uv_of(a, tri, o, d)
    tc = tex_coord(tex, tri, u, v)
    mt = np.asarray(tex["mat_tex"], np.int32)[mat]
    for k, img in enumerate(tex["textures"]):
        sel = mt == k
        if sel.any():
            base[sel] = base[sel] * lookup(img, tc[sel])
    return base


def exploded(a, tex, tri, o, d):
    """The scene in which path i hits triangle i of material i: a's triangle tri[i] with its material's
    parameters, the base colour textured (tex=None: as it is).  The tree arrays stay (never read)."""
    n = len(tri)
    b = dict(a)
    for k in ("v0", "v1", "v2", "n0", "n1", "n2"):
        b[k] = _v(a, k)[tri]
    b["mat"] = np.arange(n, dtype=np.int32)
    b["tri_id"] = np.arange(n, dtype=np.int32)
    mp = np.asarray(a["mat_params"], F).reshape(-1, 8)[np.asarray(a["mat"], np.int32)[tri]].copy()
    if tex is not None:
        mp[:, :3] = base_colour(a, tex, tri, o, d)
    b["mat_params"] = mp
    return b


def stage_material(oracle, a, tex, state, **kw):
    """or_stage_material under the texture set: the oracle's stage over the exploded scene."""
    tri = np.asarray(state["hit_tri"], np.int32)
    ms = dict(state)
    ms["hit_tri"] = np.arange(len(tri), dtype=np.int32)
    return oracle.stage_material(exploded(a, tex, tri, state["ray_o"], state["ray_d"]), ms, **kw)


def render(oracle, arrays, cam, W, H, spp, max_depth=5, rr_depth=3, seed=0x5EED2026, fixed=False, tex=None, explode=None):
    """Returns (Ld[H, W, 3], samples[H, W], counters) like oracle.render, under the texture set tex.
    explode (default: tex is not None) runs the material stage over the exploded scene."""
    n = W * H
    explode = (tex is not None) if explode is None else explode
    kw = dict(max_depth=max_depth, rr_depth=rr_depth, seed=seed, fixed=fixed)
    inv = np.argsort(arrays["tri_id"])  # scene triangle id -> position in the scene's triangle arrays
    st = {"flags": np.ones(n, np.uint32), "samples": np.zeros(n, np.uint32), "hit_tri": np.full(n, -1, np.int32),
          "ray_o": np.zeros((n, 3), F), "ray_d": np.zeros((n, 3), F), "beta": np.zeros((n, 4), F),
          "nee0": np.zeros((n, 4), F), "nee1": np.zeros((n, 4), F), "vis": np.zeros((n, 2), np.uint8),
          "Ld": np.zeros((n, 3), F)}
    cnt = {"extend_rays": 0, "shadow_rays": 0, "vis_rays": 0, "iterations": 0}
    while True:
        out = oracle.stage_logic(arrays, cam, W, H, st, spp, **kw)
        cont, gen = (out["queued"] & 2) != 0, (out["queued"] & 1) != 0
        for k in ("flags", "samples", "ray_o", "ray_d", "beta", "Ld"):
            st[k] = out[k]
        if not cont.any() and not gen.any():
            break
        cnt["iterations"] += 1
        if cont.any():
            # the whole film goes in (or_stage_material keys its draws by the array index as the pixel);
            # non-continuing paths take a dummy triangle, whose rows (NaN uvs included) never come back
            ms = dict(st)
            ms["hit_tri"] = np.where(cont, st["hit_tri"], 0).astype(np.int32)
            m = stage_material(oracle, arrays, tex, ms, **kw) if explode else oracle.stage_material(arrays, ms, **kw)
            for k in ("flags", "ray_o", "ray_d", "beta", "nee0", "nee1"):
                st[k][cont] = m[k][cont]
            st["vis"][cont, 0] = oracle.trace_any(arrays, m["light_o"][cont], m["light_d"][cont])
            has = cont & ((m["flags"] & HASVIS) != 0)
            st["vis"][cont, 1] = 0
            st["vis"][has, 1] = oracle.trace_any(arrays, m["bvis_o"][has], m["bvis_d"][has])
            cnt["shadow_rays"] += int(cont.sum())
            cnt["vis_rays"] += int(has.sum())
        ext = cont | gen
        _, _, tri = oracle.trace_closest(arrays, st["ray_o"][ext], st["ray_d"][ext])
        st["hit_tri"][ext] = np.where(tri >= 0, inv[np.maximum(tri, 0)], -1).astype(np.int32)
        cnt["extend_rays"] += int(ext.sum())
    return st["Ld"].reshape(H, W, 3), st["samples"].reshape(H, W), cnt


def random_set(a, sizes=((8, 8), (5, 3)), untextured=(), seed=1, lo=-1.0, hi=2.0):
    """A deterministic texture set for the arrays a: uvs uniform in [lo, hi), one random RGBA8 texture per
    (h, w) of sizes, dealt to the materials in turn; the materials in `untextured` get none."""
    rng = np.random.default_rng(seed)
    ntri, nmat = len(a["mat"]), len(np.asarray(a["mat_params"]).reshape(-1, 8))
    t = {k: (rng.random((ntri, 2)) * (hi - lo) + lo).astype(F) for k in ("uv0", "uv1", "uv2")}
    t["textures"] = [rng.integers(0, 256, (h, w, 4)).astype(np.uint8) for h, w in sizes]
    t["mat_tex"] = np.array([-1 if m in untextured else m % len(sizes) for m in range(nmat)], np.int32)
    return t
