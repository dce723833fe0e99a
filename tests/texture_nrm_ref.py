"""Reference for normal-map textures: texture_mr_ref's exploded scene with the three
vertex normals of path i's triangle replaced by the tangent-space perturbation of each,

    t   = lookup(normal texture of the material, tc)          texture_ref.lookup at texture_ref's tc, unchanged
    c.x = (2 * t.x - 1) * scale    c.y = (2 * t.y - 1) * scale    c.z = 2 * t.z - 1
    B_i = cross(N_i, T_i) * s_i
    m_i = (T_i * c.x + B_i * c.y) + N_i * c.z                  float32, this order

for a material whose mat_nrm index is not -1 (selection, not arithmetic, for the others).  The oracle's
make_isect then interpolates and normalises m_i as it does N_i: interpolation is linear, so this is the
usual perturbation of the interpolated frame, and everything the material stage reads of the normal follows.

A texture set is texture_mr_ref's dict with up to five more keys: "tan0", "tan1", "tan2" (ntri, 4) float32
{T.xyz, s} per corner in the arrays' triangle order, "mat_nrm" per material an index into the same texture
list or -1, "nrm_scale" one float32 per material.  Without them the loop is texture_mr_ref.render, bit for
bit (tests/test_texture_nrm_host.py).

tangents_from_uv restates host/tangents.cpp in numpy float64, in its order.

fixture() is the set the tests share: texture_mr_ref.fixture's glossy config-2 proxy and its `both` set, one
more random 6 x 7 image whose B channel lies in 128..255 (the perturbed normal keeps to the side of the vertex
normal) on every material but 1 and 4, scales 0.5 + 0.25 (m mod 4), tangents from the restatement."""
import numpy as np

import texture_mr_ref as MR
import texture_ref as TR

F = np.float32
D = np.float64
NO_NRM = (1, 4)


# ---------------------------------------------------------------------------------------------
# tangents (host/tangents.cpp restated)
def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)


def _fallback(N):
    """normalize(cross(N, axis of N's smallest component in magnitude, the first on a tie)); (1, 0, 0) where
    that cross has no finite non-zero length."""
    with np.errstate(all="ignore"):
        A = np.abs(N)
        k = np.where(A[:, 1] < A[:, 0], 1, 0)  # the two comparisons of the C code, in its order
        k = np.where(A[:, 2] < A[np.arange(len(N)), k], 2, k)
        ax = np.zeros_like(N)
        ax[np.arange(len(N)), k] = 1.0
        q = _cross(N, ax)
        l = np.sqrt(_dot(q, q))
        ok = np.isfinite(l) & (l > 0)
        T = np.where(ok[:, None], q / np.where(ok, l, 1.0)[:, None], np.array([1.0, 0.0, 0.0]))
    return T


def tangents_from_uv(v0, v1, v2, n0, n1, n2, uv0, uv1, uv2):
    """(tan0, tan1, tan2), (ntri, 4) float32 each: {T.xyz, s} per corner.  All float64 on the float32 inputs:
        e1 = p1 - p0, e2 = p2 - p0; du1, dv1 = uv1 - uv0; du2, dv2 = uv2 - uv0
        det = du1 * dv2 - du2 * dv1;  r = 1 / det
        Tt = (e1 * dv2 - e2 * dv1) * r;  Bt = (e2 * du1 - e1 * du2) * r
        q = Tt - N * dot(N, Tt);  l = sqrt(dot(q, q));  T = q / l;  s = -1 if dot(cross(N, T), Bt) < 0 else +1
    and the fallback (s = +1) where det is 0 or not finite or l is 0 or not finite."""
    p = [np.asarray(x, F).reshape(-1, 3).astype(D) for x in (v0, v1, v2)]
    N = [np.asarray(x, F).reshape(-1, 3).astype(D) for x in (n0, n1, n2)]
    c = [np.asarray(x, F).reshape(-1, 2).astype(D) for x in (uv0, uv1, uv2)]
    out = []
    with np.errstate(all="ignore"):
        e1, e2 = p[1] - p[0], p[2] - p[0]
        du1, dv1 = c[1][:, 0] - c[0][:, 0], c[1][:, 1] - c[0][:, 1]
        du2, dv2 = c[2][:, 0] - c[0][:, 0], c[2][:, 1] - c[0][:, 1]
        det = du1 * dv2 - du2 * dv1
        r = 1.0 / det
        Tt = (e1 * dv2[:, None] - e2 * dv1[:, None]) * r[:, None]
        Bt = (e2 * du1[:, None] - e1 * du2[:, None]) * r[:, None]
        det_ok = np.isfinite(det) & (det != 0)
        for Ni in N:
            q = Tt - Ni * _dot(Ni, Tt)[:, None]
            l = np.sqrt(_dot(q, q))
            ok = det_ok & np.isfinite(l) & (l > 0)
            T = q / np.where(ok, l, 1.0)[:, None]
            s = np.where(_dot(_cross(Ni, T), Bt) < 0, -1.0, 1.0)
            T = np.where(ok[:, None], T, _fallback(Ni))
            s = np.where(ok, s, 1.0)
            out.append(np.concatenate([T, s[:, None]], 1).astype(F))
    return tuple(out)


# ---------------------------------------------------------------------------------------------
# the exploded scene
def mat_nrm_of(tex, nmat):
    k = None if tex is None else tex.get("mat_nrm")
    return np.full(nmat, -1, np.int32) if k is None else np.asarray(k, np.int32)


def has_normals(tex):
    return tex is not None and (mat_nrm_of(tex, 0) >= 0).any()


def mapped_normals(a, tex, tri, o, d):
    """(m0, m1, m2), (n, 3) float32 each: the perturbed vertex normals of rays (o, d) on triangles tri."""
    tri = np.asarray(tri, np.int32)
    mat = np.asarray(a["mat"], np.int32)[tri]
    nmat = len(np.asarray(a["mat_params"]).reshape(-1, 8))
    N = [TR._v(a, k)[tri].copy() for k in ("n0", "n1", "n2")]
    if not has_normals(tex):
        return tuple(N)
    tan = [np.asarray(tex[k], F).reshape(-1, 4)[tri] for k in ("tan0", "tan1", "tan2")]
    u, v, _ = TR.uv_of(a, tri, o, d)
    tc = TR.tex_coord(tex, tri, u, v)
    nm = mat_nrm_of(tex, nmat)[mat]
    scale = np.asarray(tex["nrm_scale"], F).reshape(-1)[mat]
    with np.errstate(all="ignore"):
        for k, img in enumerate(tex["textures"]):
            sel = nm == k
            if not sel.any():
                continue
            t = TR.lookup(img, tc[sel])
            cx = ((F(2) * t[:, 0] - F(1)) * scale[sel]).astype(F)[:, None]
            cy = ((F(2) * t[:, 1] - F(1)) * scale[sel]).astype(F)[:, None]
            cz = (F(2) * t[:, 2] - F(1)).astype(F)[:, None]
            for i in range(3):
                Ni, Ti, si = N[i][sel], tan[i][sel, :3], tan[i][sel, 3:4]
                B = (TR.cross(Ni, Ti) * si).astype(F)
                N[i][sel] = ((Ti * cx + B * cy) + Ni * cz).astype(F)
    return tuple(N)


def exploded(a, tex, tri, o, d):
    """texture_mr_ref.exploded with n0, n1, n2 of path i's triangle replaced by m_i."""
    b = MR.exploded(a, tex, tri, o, d)
    if has_normals(tex):
        b["n0"], b["n1"], b["n2"] = mapped_normals(a, tex, tri, o, d)
    return b


def stage_material(oracle, a, tex, state, **kw):
    """or_stage_material under the set: the oracle's stage over the exploded scene."""
    tri = np.asarray(state["hit_tri"], np.int32)
    ms = dict(state)
    ms["hit_tri"] = np.arange(len(tri), dtype=np.int32)
    return oracle.stage_material(exploded(a, tex, tri, state["ray_o"], state["ray_d"]), ms, **kw)


def hit_normal(a, tex, tri, o, d):
    """The hit record's normal under the set: texture_ref.hit_normal over m_i."""
    tri = np.asarray(tri, np.int32)
    m0, m1, m2 = mapped_normals(a, tex, tri, o, d)
    u, v, _ = TR.uv_of(a, tri, o, d)
    k = np.arange(len(tri))
    return TR.hit_normal({"n0": m0, "n1": m1, "n2": m2}, k, u, v)


class _Textured:
    """The oracle with its material stage run over the exploded scene of a set (texture_mr_ref._Textured)."""

    def __init__(self, oracle, tex):
        self._oracle, self._tex = oracle, tex

    def __getattr__(self, k):
        return getattr(self._oracle, k)

    def stage_material(self, arrays, state, **kw):
        return stage_material(self._oracle, arrays, self._tex, state, **kw)


def render(oracle, arrays, cam, W, H, spp, max_depth=5, rr_depth=3, seed=0x5EED2026, fixed=False, tex=None):
    """(Ld[H, W, 3], samples[H, W], counters) like texture_mr_ref.render, under a set that may carry normals."""
    o = oracle if tex is None else _Textured(oracle, tex)
    return TR.render(o, arrays, cam, W, H, spp, max_depth=max_depth, rr_depth=rr_depth, seed=seed, fixed=fixed, tex=None,
                     explode=False)


# ---------------------------------------------------------------------------------------------
def nrm_fields(g, uvs, nmat, index, seed):
    """The normal fields of the fixture over the arrays g and a set's uvs: tangents from the restatement,
    every material but NO_NRM on texture `index`, scales 0.5 + 0.25 (m mod 4)."""
    t0, t1, t2 = tangents_from_uv(g["v0"], g["v1"], g["v2"], g["n0"], g["n1"], g["n2"], uvs["uv0"], uvs["uv1"], uvs["uv2"])
    assert all(np.isfinite(t).all() for t in (t0, t1, t2))
    return dict(tan0=t0, tan1=t1, tan2=t2,
                mat_nrm=np.array([-1 if m in NO_NRM else index for m in range(nmat)], np.int32),
                nrm_scale=np.array([0.5 + 0.25 * (m % 4) for m in range(nmat)], F))


def normal_image(seed=1, hw=(6, 7), b_lo=128):
    rng = np.random.default_rng(seed + 6)
    img = rng.integers(0, 256, hw + (4,)).astype(np.uint8)
    img[..., 2] = rng.integers(b_lo, 256, hw).astype(np.uint8)
    return img


def fixture(a, seed=1):
    """(glossy arrays, {"all": base + MR + normal, "both": base + MR, "base", "nrm": normal only})."""
    g, both, base, _ = MR.fixture(a, seed=seed)
    nmat = len(np.asarray(g["mat_params"]).reshape(-1, 8))
    # the fixture's random uvs give a non-zero uv determinant on every triangle: no fallback tangent
    c = [np.asarray(both[k], D) for k in ("uv0", "uv1", "uv2")]
    det = (c[1][:, 0] - c[0][:, 0]) * (c[2][:, 1] - c[0][:, 1]) - (c[2][:, 0] - c[0][:, 0]) * (c[1][:, 1] - c[0][:, 1])
    assert (det != 0).all() and np.isfinite(det).all()
    imgs = list(both["textures"]) + [normal_image(seed)]
    nf = nrm_fields(g, both, nmat, len(imgs) - 1, seed)
    full = dict(both, textures=imgs, **nf)
    only = dict(full, mat_tex=np.full(nmat, -1, np.int32), mat_mr=np.full(nmat, -1, np.int32))
    return g, {"all": full, "both": both, "base": base, "nrm": only}
