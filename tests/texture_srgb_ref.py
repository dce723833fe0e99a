"""Reference for sRGB base colour: texture_nrm_ref's exploded scene with the base-colour
columns of paths on flagged materials recomputed through the sRGB table,

    L[c]  = x / 12.92 for x <= 0.04045, else ((x + 0.055) / 1.055) ** 2.4,  x = c / 255 in float64, rounded to float32
    texel = L[c] in place of c / 255             per channel, before the filter
    T     = texture_ref.lookup's arithmetic over those texels, unchanged
    base  = base_factor * T

for a material whose base-colour texture carries MCPT_TEX_SRGB (bit 0 of its word in "tex_flags").  The
metallic-roughness and normal lookups never decode, whatever the flag of the texture they read.

A texture set is texture_nrm_ref's dict with one more key, "tex_flags": one uint32 per texture of the list, or
absent (all 0).  Without a flag on a texture that a base-colour slot uses the loop is texture_nrm_ref.render,
bit for bit (tests/test_texture_srgb_host.py).

fixture() is the set the tests share: texture_nrm_ref.fixture's sets with the two images that serve as base
colours (and, on other materials, as metallic-roughness textures) flagged."""
import numpy as np

import texture_nrm_ref as NR
import texture_ref as TR

F = np.float32
SRGB = 1  # MCPT_TEX_SRGB


def table():
    """The 256 floats of device/srgb_table.hpp in numpy: float64 arithmetic, rounded to float32."""
    x = np.arange(256, dtype=np.float64) / 255.0
    return np.where(x <= 0.04045, x / 12.92, ((x + 0.055) / 1.055) ** 2.4).astype(F)


def unorm_table():
    """byte / 255, correctly rounded: texture_ref.texels as a table."""
    return (np.arange(256).astype(F) / F(255)).astype(F)


def lookup(img, uv, tab):
    """texture_ref.lookup with texel = tab[byte]: (n, 3) float32 for uv (n, 2)."""
    T = np.asarray(tab, F)[np.asarray(img)[..., :3]]
    H, W = T.shape[:2]
    uv = np.asarray(uv, F).reshape(-1, 2)
    with np.errstate(all="ignore"):
        u = np.where(np.abs(uv[:, 0]) < F(65536), uv[:, 0], F(0)).astype(F)
        v = np.where(np.abs(uv[:, 1]) < F(65536), uv[:, 1], F(0)).astype(F)
    x = (u * F(W) - F(0.5)).astype(F)
    y = (v * F(H) - F(0.5)).astype(F)
    fx, fy = np.floor(x), np.floor(y)
    ax, ay = TR.q8(x - fx), TR.q8(y - fy)
    ix, iy = fx.astype(np.int64), fy.astype(np.int64)
    i0, i1, j0, j1 = ix % W, (ix + 1) % W, iy % H, (iy + 1) % H
    bx, by = F(1) - ax, F(1) - ay
    w00, w10, w01, w11 = bx * by, ax * by, bx * ay, ax * ay
    return (((w00[:, None] * T[j0, i0] + w10[:, None] * T[j0, i1]) + w01[:, None] * T[j1, i0]) +
            w11[:, None] * T[j1, i1]).astype(F)


def flags_of(tex):
    n = len(tex["textures"])
    f = tex.get("tex_flags")
    return np.zeros(n, np.uint32) if f is None else np.asarray(f, np.uint32)


def flagged_materials(tex, nmat):
    """bool (nmat,): the material's base-colour texture is flagged sRGB."""
    mt = np.asarray(tex["mat_tex"], np.int32)
    fl = flags_of(tex)
    return (mt >= 0) & ((fl[np.maximum(mt, 0)] & SRGB) != 0)


def base_colour(a, tex, tri, o, d):
    """(n, 3) float32: texture_ref.base_colour with the texels of flagged textures decoded through the table."""
    mat = np.asarray(a["mat"], np.int32)[tri]
    base = np.asarray(a["mat_params"], F).reshape(-1, 8)[mat, :3].copy()
    u, v, _ = TR.uv_of(a, tri, o, d)
    tc = TR.tex_coord(tex, tri, u, v)
    mt = np.asarray(tex["mat_tex"], np.int32)[mat]
    fl = flags_of(tex)
    for k, img in enumerate(tex["textures"]):
        sel = mt == k
        if sel.any():
            base[sel] = base[sel] * lookup(img, tc[sel], table() if fl[k] & SRGB else unorm_table())
    return base


def exploded(a, tex, tri, o, d):
    """texture_nrm_ref.exploded with the base-colour columns of paths on flagged materials recomputed."""
    b = NR.exploded(a, tex, tri, o, d)
    if tex is None:
        return b
    tri = np.asarray(tri, np.int32)
    nmat = len(np.asarray(a["mat_params"]).reshape(-1, 8))
    sel = flagged_materials(tex, nmat)[np.asarray(a["mat"], np.int32)[tri]]
    if sel.any():
        o, d = np.asarray(o, F).reshape(-1, 3), np.asarray(d, F).reshape(-1, 3)
        b["mat_params"][sel, :3] = base_colour(a, tex, tri[sel], o[sel], d[sel])
    return b


def stage_material(oracle, a, tex, state, **kw):
    """or_stage_material under the set: the oracle's stage over the exploded scene."""
    tri = np.asarray(state["hit_tri"], np.int32)
    ms = dict(state)
    ms["hit_tri"] = np.arange(len(tri), dtype=np.int32)
    return oracle.stage_material(exploded(a, tex, tri, state["ray_o"], state["ray_d"]), ms, **kw)


class _Textured:
    """The oracle with its material stage run over the exploded scene of a set (texture_nrm_ref._Textured)."""

    def __init__(self, oracle, tex):
        self._oracle, self._tex = oracle, tex

    def __getattr__(self, k):
        return getattr(self._oracle, k)

    def stage_material(self, arrays, state, **kw):
        return stage_material(self._oracle, arrays, self._tex, state, **kw)


def render(oracle, arrays, cam, W, H, spp, max_depth=5, rr_depth=3, seed=0x5EED2026, fixed=False, tex=None):
    """(Ld[H, W, 3], samples[H, W], counters) like texture_nrm_ref.render, under a set that may carry tex_flags."""
    o = oracle if tex is None else _Textured(oracle, tex)
    return TR.render(o, arrays, cam, W, H, spp, max_depth=max_depth, rr_depth=rr_depth, seed=seed, fixed=fixed, tex=None,
                     explode=False)


def fixture(a, seed=1):
    """(glossy arrays, sets): texture_nrm_ref.fixture's sets, and
    "srgb": `all` with images 0 and 1 (the base-colour images, which other materials use as MR textures) flagged,
    "srgb_base": `base` (no MR, no normal maps) with the same two flagged,
    "srgb_unused": `all` with only the normal image flagged: no base-colour slot uses it,
    "srgb_both": `both` (base + MR, no normal maps) with images 0 and 1 flagged: render_emitters' set."""
    g, sets = NR.fixture(a, seed=seed)
    full = sets["all"]
    assert set(np.asarray(full["mat_tex"])[np.asarray(full["mat_tex"]) >= 0]) == {0, 1} and len(full["textures"]) == 3
    sets = dict(sets)
    sets["srgb"] = dict(full, tex_flags=np.array([SRGB, SRGB, 0], np.uint32))
    sets["srgb_base"] = dict(sets["base"], tex_flags=np.array([SRGB, SRGB], np.uint32))
    sets["srgb_unused"] = dict(full, tex_flags=np.array([0, 0, SRGB], np.uint32))
    sets["srgb_both"] = dict(sets["both"], tex_flags=np.array([SRGB, SRGB], np.uint32))
    return g, sets


def render_emitters(oracle, arrays, cam, W, H, spp, tex, emission, max_depth=5, rr_depth=3, seed=0x5EED2026, fixed=False, mis=False):
    """emitter_mis_ref.render (emitter sampling on, with or without MIS) under a set without normal maps: the
    material stage runs over the exploded scene, and the emitter sample's f, its MIS weight's BRDF pdf and pdf_s
    read the hit's own material row of that scene (the textured base colour, roughness and metallic) in place of
    the material's.  The hit's normal is the traced one: a set with normal maps is refused.  With tex=None the
    loop is emitter_mis_ref.render(sample=True), bit for bit (tests/test_texture_srgb_host.py)."""
    import emitter_mis_ref as XR
    from emitter_ref import F_DEAD, HASVIS, film_line, scene_table

    assert not NR.has_normals(tex)
    n = W * H
    kw = dict(max_depth=max_depth, rr_depth=rr_depth, seed=seed, fixed=fixed)
    mat = np.asarray(arrays["mat"], np.int32)
    inv = np.argsort(arrays["tri_id"])
    tab = scene_table(arrays, emission)
    assert len(tab["cdf"]) > 0  # sampling is active
    pick_rec = XR.pick_by_record(tab, len(mat)) if mis else None
    yy, xx = np.divmod(np.arange(n), W)
    rendered = (xx < W - 1) & (yy < H - 1)
    st = {"flags": np.ones(n, np.uint32), "samples": np.zeros(n, np.uint32), "hit_tri": np.full(n, -1, np.int32),
          "ray_o": np.zeros((n, 3), F), "ray_d": np.zeros((n, 3), F), "beta": np.zeros((n, 4), F), "nee0": np.zeros((n, 4), F),
          "nee1": np.zeros((n, 4), F), "vis": np.zeros((n, 2), np.uint8), "Ld": np.zeros((n, 3), F)}
    nee2, ve, nrm = np.zeros((n, 4), F), np.zeros(n, np.uint8), np.zeros((n, 3), F)
    cnt = {"extend_rays": 0, "shadow_rays": 0, "vis_rays": 0, "iterations": 0, "emitter_rays": 0}
    while True:
        fl_in = st["flags"].copy()
        len_in = (fl_in >> np.uint32(1)) & np.uint32(0xFF)
        alive = rendered & ((fl_in & F_DEAD) == 0) & ((fl_in >> np.uint32(13)) < np.uint32(spp))
        take = alive & (len_in > 1) & (len_in <= max_depth)
        Ld_own = film_line(st["Ld"], take, st["beta"][:, :3], fl_in, st["nee0"], st["nee1"], st["vis"], nee2, ve)
        out = oracle.stage_logic(arrays, cam, W, H, st, spp, **kw)
        cont, gen = (out["queued"] & 2) != 0, (out["queued"] & 1) != 0
        for k in ("flags", "samples", "ray_o", "ray_d", "beta", "Ld"):
            st[k] = out[k]
        st["Ld"] = np.where(take[:, None], Ld_own, st["Ld"])
        if mis:
            XR.collect(st["Ld"], cont, len_in, st["hit_tri"], st["beta"], mat, emission, pick_rec, nee2[:, 3], arrays,
                       st["ray_o"], st["ray_d"])
        else:
            XR.MR.emission_line(st["Ld"], cont & (len_in == 1), st["hit_tri"], st["beta"], mat, emission)
        if not cont.any() and not gen.any():
            break
        cnt["iterations"] += 1
        if cont.any():
            ms = dict(st)
            ms["hit_tri"] = np.where(cont, st["hit_tri"], 0).astype(np.int32)
            wo = -st["ray_d"]
            ci = np.flatnonzero(cont)
            if tex is None:
                m = oracle.stage_material(arrays, ms, **kw)
                rows = np.asarray(arrays["mat_params"], F).reshape(-1, 8)[mat[st["hit_tri"][ci]]]
            else:
                m = stage_material(oracle, arrays, tex, ms, **kw)
                rows = exploded(arrays, tex, st["hit_tri"][ci], st["ray_o"][ci], st["ray_d"][ci])["mat_params"]
            for k in ("flags", "ray_o", "ray_d", "beta", "nee0", "nee1"):
                st[k][cont] = m[k][cont]
            st["vis"][cont, 0] = oracle.trace_any(arrays, m["light_o"][cont], m["light_d"][cont])
            has = cont & ((m["flags"] & HASVIS) != 0)
            st["vis"][cont, 1] = 0
            st["vis"][has, 1] = oracle.trace_any(arrays, m["bvis_o"][has], m["bvis_d"][has])
            cnt["shadow_rays"] += int(cont.sum())
            cnt["vis_rays"] += int(has.sum())
            # (emitter_sample reads arrays["mat_params"][hit_mat]: row j of `rows` is path ci[j]'s)
            per_hit = dict(arrays, mat_params=np.ascontiguousarray(rows, F))
            cE, valid, ldir, tmax = XR.emitter_sample(oracle, per_hit, tab, emission, ci, fl_in[ci] >> np.uint32(13), len_in[ci],
                                                      m["light_o"][ci], nrm[ci], wo[ci], np.arange(len(ci)), seed, mis)
            nee2[ci, :3] = cE
            if mis:
                nee2[ci, 3] = XR.brdf_pdf(oracle, rows, nrm[ci], m["ray_d"][ci], wo[ci])[1]
            ve[ci] = 0
            vi = ci[valid]
            if len(vi):
                pos_t, _, tri = oracle.trace_closest(arrays, m["light_o"][vi], ldir[valid])
                ve[vi] = ~((tri >= 0) & (pos_t[:, 3] < tmax[valid]))
            cnt["emitter_rays"] += int(valid.sum())
        ext = cont | gen
        _, nm, tri = oracle.trace_closest(arrays, st["ray_o"][ext], st["ray_d"][ext])
        st["hit_tri"][ext] = np.where(tri >= 0, inv[np.maximum(tri, 0)], -1).astype(np.int32)
        nrm[ext] = nm[:, :3]
        cnt["extend_rays"] += int(ext.sum())
    return st["Ld"].reshape(H, W, 3), st["samples"].reshape(H, W), cnt
