"""Reference for metallic-roughness textures: texture_ref's exploded scene with two
more columns.  Path i's material row gets, beside the textured base colour of section 19,

    T     = lookup(MR texture of the material, tc)      texture_ref.lookup at texture_ref's tc, unchanged
    rough = mat_params[6] * T.g                          float32; the oracle's fmax(roughness, eps) clamps it
    metal = mat_params[7] * T.b                          float32

for a material whose mat_mr index is not -1.  A texture set is texture_ref's dict with one more key,
"mat_mr": per material the index of its metallic-roughness texture in the same list, or -1 (absent: all
-1).  Without an MR index the loop is texture_ref.render, bit for bit (tests/test_texture_mr_host.py).

fixture() is the set the tests share: config 2's proxy wearing ten glossy, partly metallic rows of
material_fixtures.PALETTE, texture_ref.random_set's uvs, images and base-colour indices, and MR indices
that leave materials with both textures, with either alone and (material 6) with none."""
import numpy as np

import material_fixtures as mf
import texture_ref as TR

F = np.float32
PALETTE_ROWS = (1, 2, 4, 5, 7, 8, 10, 11, 16, 18)  # every row: metallic > 0, a non-dyadic roughness
NO_MR = (2, 6)  # material 2 keeps its base-colour texture alone; 6 has neither (random_set's untextured=(1, 6))


def glossy(a):
    """The arrays with PALETTE_ROWS as the ten materials' rows, their own base colours kept."""
    b = dict(a)
    mp = mf.PALETTE[list(PALETTE_ROWS)].copy()
    old = np.asarray(a["mat_params"], F).reshape(-1, 8)
    assert len(old) == len(mp)
    mp[:, :3] = old[:, :3]
    b["mat_params"] = mp
    return b


def mr_indices(nmat):
    return np.array([-1 if m in NO_MR else (m + 1) % 2 for m in range(nmat)], np.int32)


def fixture(a, seed=1):
    """(glossy arrays, base + MR set, the same set without MR indices, the MR-only set)."""
    g = glossy(a)
    base = TR.random_set(g, sizes=((8, 8), (3, 5)), untextured=(1, 6), seed=seed)
    both = dict(base, mat_mr=mr_indices(len(g["mat_params"])))
    only = dict(both, mat_tex=np.full_like(base["mat_tex"], -1))
    return g, both, base, only


def mat_mr_of(tex, nmat):
    mr = tex.get("mat_mr")
    return np.full(nmat, -1, np.int32) if mr is None else np.asarray(mr, np.int32)


def rough_metal(a, tex, tri, o, d):
    """(n, 2) float32: the roughness (before the clamp) and metallic of rays (o, d) at their hits on tri."""
    mat = np.asarray(a["mat"], np.int32)[tri]
    mp = np.asarray(a["mat_params"], F).reshape(-1, 8)
    rm = mp[mat, 6:8].copy()
    u, v, _ = TR.uv_of(a, tri, o, d)
    tc = TR.tex_coord(tex, tri, u, v)
    mr = mat_mr_of(tex, len(mp))[mat]
    for k, img in enumerate(tex["textures"]):
        sel = mr == k
        if sel.any():
            T = TR.lookup(img, tc[sel])
            rm[sel] = (rm[sel] * T[:, 1:3]).astype(F)
    return rm


def exploded(a, tex, tri, o, d):
    """texture_ref.exploded with the roughness and metallic columns textured as well."""
    b = TR.exploded(a, tex, tri, o, d)
    if tex is not None and (mat_mr_of(tex, 0) >= 0).any():
        b["mat_params"][:, 6:8] = rough_metal(a, tex, tri, o, d)
    return b


def stage_material(oracle, a, tex, state, **kw):
    """or_stage_material under the set: the oracle's stage over the exploded scene."""
    tri = np.asarray(state["hit_tri"], np.int32)
    ms = dict(state)
    ms["hit_tri"] = np.arange(len(tri), dtype=np.int32)
    return oracle.stage_material(exploded(a, tex, tri, state["ray_o"], state["ray_d"]), ms, **kw)


class _Textured:
    """The oracle with its material stage run over the exploded scene of a set: texture_ref.render's loop
    then is the textured loop (that module's own explosion knows the base colour only)."""

    def __init__(self, oracle, tex):
        self._oracle, self._tex = oracle, tex

    def __getattr__(self, k):
        return getattr(self._oracle, k)

    def stage_material(self, arrays, state, **kw):
        return stage_material(self._oracle, arrays, self._tex, state, **kw)


def render(oracle, arrays, cam, W, H, spp, max_depth=5, rr_depth=3, seed=0x5EED2026, fixed=False, tex=None):
    """(Ld[H, W, 3], samples[H, W], counters) like texture_ref.render, under a set that may carry mat_mr."""
    o = oracle if tex is None else _Textured(oracle, tex)
    return TR.render(o, arrays, cam, W, H, spp, max_depth=max_depth, rr_depth=rr_depth, seed=seed, fixed=fixed, tex=None,
                     explode=False)
