"""Metallic-roughness textures on the device: k_material<TexMr, ...> against
tests/texture_mr_ref.py (the oracle's material stage over an exploded scene whose roughness and metallic
columns are textured too), bit for bit, and the set's life cycle on a live context.

24 x 16 film, 4 spp, config 2's proxy (10 materials) wearing glossy, partly metallic palette rows, unless
stated.  texture_mr_ref.fixture: materials with both textures, with either alone, and one with neither."""
import ctypes as C

import numpy as np
import pytest

import emission_ref as ER
import material_fixtures as mf
import refit_ref as RF
import texture_mr_ref as MR
from stage_checks import _check_stage
from test_gpu import film_close

pytestmark = pytest.mark.gpu
W, H, SPP = 24, 16, 4
F = np.float32
RAYS = ("extend_rays", "shadow_rays", "vis_rays")


def u32(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def same_film(f, g):
    return np.array_equal(u32(f[0]), u32(g[0])) and np.array_equal(f[1], g[1])


def rays(st):
    return tuple(int(getattr(st, k)) for k in RAYS)


def install(p, tex):
    p.set_textures(tex["uv0"], tex["uv1"], tex["uv2"], tex["textures"], tex["mat_tex"], mat_mr=tex.get("mat_mr"))


def ctx(mcpt, scene, cam, tex=None, fixed=False, depth=5, gpu_bvh=False, slots=1, E=None, samp=False, mis=False):
    p = mcpt.PathTracer(0, mcpt.default_config(spp=SPP, max_depth=depth, fixed=fixed))
    p.upload_scene(scene, gpu_bvh=gpu_bvh)
    if tex is not None:
        install(p, tex)
    if E is not None:
        p.set_emission(E)
    if samp:
        p.set_emitter_sampling(True)
    if mis:
        p.set_emitter_mis(True)
    p.set_camera(cam)
    p.resize(W, H)
    if slots != 1:
        p.set_path_slots(slots)
    return p


def frame(p):
    st = p.render()
    Ld, sm = p.film()
    return Ld.copy(), sm.copy(), rays(st)


def one(mcpt, *args, **kw):
    p = ctx(mcpt, *args, **kw)
    f = frame(p)
    p.close()
    return f


@pytest.fixture(scope="module")
def c2(mcpt_mod, scene_c2):
    _, a = scene_c2
    g, both, base, only = MR.fixture(a)
    return dict(a=g, scene=mcpt_mod.desc_from_arrays(g), both=both, base=base, only=only,
                cam=mcpt_mod.config_camera(mcpt_mod.CONFIGS[2], W, H))


_REF = {}


def ref_film(oracle, sc, which, fixed=False, depth=5):
    """texture_mr_ref.render of the fixture under set `which` (None: no set), computed once."""
    key = (which, fixed, depth)
    if key not in _REF:
        _REF[key] = MR.render(oracle, sc["a"], sc["cam"], W, H, SPP, max_depth=depth, fixed=fixed, tex=sc[which] if which else None)
    return _REF[key]


def guard(oracle, sc, which, against, fixed=False, depth=5):
    """More than 100 of the 384 pixels of the reference film change with the MR indices: no comparison
    below can pass because the MR lookups do nothing."""
    n = int((ref_film(oracle, sc, which, fixed, depth)[0] != ref_film(oracle, sc, against, fixed, depth)[0]).any(axis=2).sum())
    print(f"pixels changed by the MR set ({which} against {against}, fixed={fixed}, depth={depth}): {n} of {W * H}")
    assert n > 100


# ---------------------------------------------------------------------------------------------
# 1. the material stage
@pytest.mark.parametrize("kind", ["generic", "grazing"])
@pytest.mark.parametrize("fixed", [False, True])
def test_material_stage_equals_the_oracle_on_the_exploded_scene(mcpt_mod, oracle, fixed, kind):
    """Every output of mcpt_stage_run(MATERIAL), on 1024 generic paths and on up to 1024 grazing ones (near
    n.wo = 0 a per-hit roughness is most likely to expose an expression-order slip)."""
    import stage_fixtures as sf

    s = sf.stage_scene(mcpt_mod, 2)
    a, tex, _, _ = MR.fixture(s.arrays(), seed=4)
    kw = dict(max_depth=sf.DEPTH, rr_depth=sf.RR, fixed=fixed)
    if kind == "generic":
        inp = sf.material_state(a, oracle.trace_closest, 2, 1024)
    else:
        inp = mf.grazing_state(a, oracle.trace_closest, 1024, 11, 2)
        ndw = mf.n_dot_wo(a, oracle.trace_closest, inp)
        assert (ndw < 0.02).sum() >= 250 and (ndw < 0).sum() >= 100, ((ndw < 0.02).sum(), (ndw < 0).sum())
    mats = np.asarray(a["mat"])[inp["hit_tri"]]
    mt, mr = np.asarray(tex["mat_tex"])[mats], np.asarray(tex["mat_mr"])[mats]
    # both MR textures, a material with a base-colour texture alone, and one with neither are hit
    assert set(mr) == {-1, 0, 1} and ((mt >= 0) & (mr < 0)).any() and ((mt < 0) & (mr < 0)).any() and ((mt < 0) & (mr >= 0)).any()
    ref = MR.stage_material(oracle, a, tex, inp, **kw)
    base_only = MR.stage_material(oracle, a, dict(tex, mat_mr=None), inp, **kw)
    plain = oracle.stage_material(a, inp, **kw)
    assert (u32(ref["nee0"]) != u32(base_only["nee0"])).any(axis=1).sum() > 100
    assert np.array_equal(u32(ref["nee0"][mr < 0]), u32(base_only["nee0"][mr < 0]))
    pt = mcpt_mod.PathTracer(0, mcpt_mod.default_config(spp=sf.SPP, max_depth=sf.DEPTH, rr_depth=sf.RR, fixed=fixed))
    pt.upload_scene(mcpt_mod.desc_from_arrays(a))
    pt.set_camera(sf.stage_camera(mcpt_mod, 2))
    install(pt, tex)
    st = pt.texture_stats()
    assert st["in_effect"] and st["mr_in_effect"] and st["mr_materials"] == int((tex["mat_mr"] >= 0).sum())
    _check_stage("material", pt.stage("material", inp), ref, a, oracle)
    pt.set_textures()  # removed: the stage of a context without textures
    _check_stage("material", pt.stage("material", inp), plain, a, oracle)
    pt.close()


# ---------------------------------------------------------------------------------------------
# 2. the film
@pytest.mark.parametrize("gpu_bvh", [False, True])
@pytest.mark.parametrize("fixed", [False, True])
def test_film_equals_the_reference_loop(mcpt_mod, oracle, c2, fixed, gpu_bvh):
    """Base + MR set: bitwise in Ld and samples at one path slot, with the reference loop's ray counts, on
    the host tree and on the device-built one (whose records, and so the uv stream, are in Morton order)."""
    guard(oracle, c2, "both", "base", fixed)
    rLd, rsm, rc = ref_film(oracle, c2, "both", fixed)
    got = one(mcpt_mod, c2["scene"], c2["cam"], c2["both"], fixed=fixed, gpu_bvh=gpu_bvh)
    assert np.array_equal(got[1], rsm) and np.array_equal(u32(got[0]), u32(rLd))
    assert got[2] == tuple(rc[k] for k in RAYS)


@pytest.mark.parametrize("fixed", [False, True])
def test_an_mr_only_set_is_in_effect(mcpt_mod, oracle, c2, fixed):
    """Every mat_tex index -1: the set still shades, through k_material<TexMr, ...>."""
    guard(oracle, c2, "only", None, fixed)
    rLd, rsm, rc = ref_film(oracle, c2, "only", fixed)
    p = ctx(mcpt_mod, c2["scene"], c2["cam"], c2["only"], fixed=fixed)
    st = p.texture_stats()
    assert st["in_effect"] and st["mr_in_effect"] and st["textured_materials"] == 0 and st["mr_materials"] == 8
    got = frame(p)
    p.close()
    assert np.array_equal(got[1], rsm) and np.array_equal(u32(got[0]), u32(rLd)) and got[2] == tuple(rc[k] for k in RAYS)


def test_ray_counts_follow_the_set_below_the_roulette(mcpt_mod, oracle, c2):
    """max_depth 2 (rr_depth 3): no roulette, but a lower roughness and a higher metallic end more
    continuation samples with f == 0 or pdf == 0 (F_FZERO), so the extension-ray count is the reference
    loop's and not the untextured context's."""
    guard(oracle, c2, "both", "base", depth=2)
    rLd, rsm, rc = ref_film(oracle, c2, "both", depth=2)
    got = one(mcpt_mod, c2["scene"], c2["cam"], c2["both"], depth=2)
    plain = one(mcpt_mod, c2["scene"], c2["cam"], None, depth=2)
    assert np.array_equal(got[1], rsm) and np.array_equal(u32(got[0]), u32(rLd))
    assert got[2] == tuple(rc[k] for k in RAYS)
    assert plain[2] == tuple(ref_film(oracle, c2, None, depth=2)[2][k] for k in RAYS) and got[2][0] != plain[2][0]


@pytest.mark.parametrize("gpu_bvh", [False, True])
def test_three_path_slots(mcpt_mod, oracle, c2, gpu_bvh):
    """Slot k runs samples k, k + 3, ...: only the film's summation order differs (the project's tolerance
    for that), counts and samples exact."""
    guard(oracle, c2, "both", "base")
    rLd, rsm, rc = ref_film(oracle, c2, "both")
    got = one(mcpt_mod, c2["scene"], c2["cam"], c2["both"], slots=3, gpu_bvh=gpu_bvh)
    ok, bad = film_close(got[0], rLd)
    assert ok, bad
    assert np.array_equal(got[1], rsm) and got[2] == tuple(rc[k] for k in RAYS)


# ---------------------------------------------------------------------------------------------
# 3. identity across every instantiation
MODES = {"plain": {}, "fixed": dict(fixed=True), "samp": dict(samp=True), "samp_fixed": dict(samp=True, fixed=True),
         "mis": dict(samp=True, mis=True), "mis_fixed": dict(samp=True, mis=True, fixed=True)}


@pytest.mark.parametrize("mode", list(MODES))
def test_constant_mr_textures_are_channel_masks(mcpt_mod, c2, mode):
    """Every material wears a constant MR texture whose G and B are 0 or 255: the film is, bit for bit and
    with the same ray counts, that of the same scene with those columns of mat_params zeroed, and an all-255
    set reproduces the context without a set.  Exact: the weights are multiples of 2^-16 that sum to 1 and
    multiply 0 or 1, and a zeroed roughness meets the same clamp.  One wall and one sphere emit under a black
    environment, so the emitter sample's f and the MIS weight's BRDF pdf matter."""
    a = ER.black(c2["a"])
    nmat = len(a["mat_params"])
    E = ER.table(nmat, {ER.MATS_LIT[0]: (3.0, 2.0, 1.0), ER.MATS_LIT[1]: (0.5, 2.0, 8.0)})
    kw = dict(E=E, **MODES[mode])
    masks = np.array([[(1 + m % 3) & 1, (1 + m % 3) >> 1 & 1] for m in range(nmat)], np.uint8)  # G, B: 10, 01, 11 in turn
    sizes = [(1, 1), (3, 5), (8, 8)]
    texs = [np.broadcast_to(np.array([91, 255 * masks[m][0], 255 * masks[m][1], 77], np.uint8), sizes[m % 3] + (4,)).copy()
            for m in range(nmat)]
    tex = dict(c2["both"], textures=texs, mat_tex=np.full(nmat, -1, np.int32), mat_mr=np.arange(nmat, dtype=np.int32))
    zeroed = dict(a, mat_params=np.asarray(a["mat_params"], F).copy())
    zeroed["mat_params"][:, 6:8] *= masks
    d = mcpt_mod.desc_from_arrays(a)
    want = one(mcpt_mod, mcpt_mod.desc_from_arrays(zeroed), c2["cam"], None, **kw)
    plain = one(mcpt_mod, d, c2["cam"], None, **kw)
    p = ctx(mcpt_mod, d, c2["cam"], tex, **kw)
    assert p.texture_stats()["mr_in_effect"] and p.emitter_stats()["active"] == bool(kw.get("samp")) and p.emitter_stats()["mis"] == bool(kw.get("mis"))
    got = frame(p)
    white = dict(tex, textures=[np.full((2, 3, 4), 255, np.uint8)], mat_mr=np.zeros(nmat, np.int32))
    install(p, white)
    assert p.texture_stats()["mr_in_effect"]
    ones = frame(p)
    p.close()
    assert (plain[0] != 0).any(axis=2).sum() > 100
    assert ((want[0] != plain[0]).any(axis=2)).sum() > 100  # the masks matter: no vacuous identity
    assert same_film(got, want) and got[2] == want[2]
    assert same_film(ones, plain) and ones[2] == plain[2]


# ---------------------------------------------------------------------------------------------
# 4. the older call
def test_a_base_only_set_is_the_older_call(mcpt_mod, oracle, c2):
    """mcpt_set_material_textures is mcpt_set_material_texture_maps with NULL: the same film from either
    (mat_mr all -1 through the new call), the base-colour kernels and not the MR ones in effect."""
    base = c2["base"]
    old = one(mcpt_mod, c2["scene"], c2["cam"], base)
    p = ctx(mcpt_mod, c2["scene"], c2["cam"], dict(base, mat_mr=np.full_like(base["mat_tex"], -1)))
    st = p.texture_stats()
    assert st["in_effect"] and not st["mr_in_effect"] and st["mr_materials"] == 0
    new = frame(p)
    install(p, base)  # the older call with the same arrays: an identical set, nothing happens
    assert rays(p.iterate(1)) == (0, 0, 0)
    p.close()
    rLd, rsm, rc = ref_film(oracle, c2, "base")
    assert same_film(new, old) and new[2] == old[2]
    assert np.array_equal(u32(new[0]), u32(rLd)) and new[2] == tuple(rc[k] for k in RAYS)


# ---------------------------------------------------------------------------------------------
# 5. geometry updates
@pytest.mark.parametrize("mode", ["refit", "rebuild"])
def test_geometry_updates_keep_the_set(mcpt_mod, c2, mode):
    """After an update the film equals a fresh upload of the moved mesh with the set installed again."""
    gpu = mode == "rebuild"
    tex = c2["both"]
    m = RF.refitted_desc_arrays(c2["a"], amp=0.02)
    p = ctx(mcpt_mod, c2["scene"], c2["cam"], tex, gpu_bvh=gpu)
    before = frame(p)
    p.update_geometry(m["v0"], m["v1"], m["v2"], mode=mode)
    t = p.textures()
    assert all(np.array_equal(t[k], tex[k]) for k in ("uv0", "uv1", "uv2", "mat_tex", "mat_mr")) and p.texture_stats()["mr_in_effect"]
    moved = frame(p)
    p.close()
    fresh = one(mcpt_mod, mcpt_mod.desc_from_arrays(m), c2["cam"], tex, gpu_bvh=gpu)
    assert same_film(moved, fresh) and moved[2] == fresh[2] and not same_film(moved, before)


# ---------------------------------------------------------------------------------------------
# 6. state
def test_identical_changed_and_dropped_sets(mcpt_mod, c2):
    both, base = c2["both"], c2["base"]
    never = one(mcpt_mod, c2["scene"], c2["cam"], None)
    p = ctx(mcpt_mod, c2["scene"], c2["cam"], both)
    first = frame(p)
    t = p.textures()
    assert all(np.array_equal(t[k], both[k]) for k in ("uv0", "uv1", "uv2", "mat_tex", "mat_mr"))
    assert len(t["textures"]) == 2 and all(np.array_equal(x, y) for x, y in zip(t["textures"], both["textures"]))
    install(p, {k: (v.copy() if isinstance(v, np.ndarray) else [x.copy() for x in v]) for k, v in both.items()})
    assert rays(p.iterate(1)) == (0, 0, 0) and same_film((*p.film(),), first)  # an identical set: nothing happens
    p.render_guides(1)
    p.guides()
    other = both["mat_mr"].copy()
    other[0] = 1 - other[0]
    install(p, dict(both, mat_mr=other))  # mat_mr alone changed: the film stale, the guides stale
    with pytest.raises(mcpt_mod.McptError):
        p.guides()
    st = p.iterate(1)
    assert st.extend_rays > 0 and p.film()[1].max() < SPP
    assert not same_film(frame(p), first)
    install(p, base)  # the MR indices gone: section 19's kernels, and its film
    s = p.texture_stats()
    assert s["in_effect"] and not s["mr_in_effect"] and np.array_equal(p.textures()["mat_mr"], np.full(len(other), -1))
    assert same_film(frame(p), one(mcpt_mod, c2["scene"], c2["cam"], base))
    install(p, both)
    assert same_film(frame(p), first)
    p.upload_scene(c2["scene"])  # an upload drops the set
    assert p.textures() is None and p.texture_stats() == {"bytes": 0, "textured_materials": 0, "in_effect": False}
    assert same_film(frame(p), never)
    p.close()


def test_rejected_sets_leave_the_installed_one(mcpt_mod, c2):
    lib, tex, a = mcpt_mod.lib(), c2["both"], c2["a"]
    ntri, nmat = len(a["mat"]), len(a["mat_params"])
    f = lambda x: np.ascontiguousarray(x, F).ctypes.data_as(C.POINTER(C.c_float))
    u = [np.ascontiguousarray(tex[k], F) for k in ("uv0", "uv1", "uv2")]
    imgs = [np.ascontiguousarray(t) for t in tex["textures"]]

    def call(p, ntri_=ntri, nmat_=nmat, mt=tex["mat_tex"], mr=tex["mat_mr"], sizes=None, null_px=False, uvs=None):
        arr = (mcpt_mod.Texture * len(imgs))()
        for k, im in enumerate(imgs):
            arr[k].w, arr[k].h = sizes[k] if sizes else (im.shape[1], im.shape[0])
            arr[k].rgba8 = None if null_px and k == 1 else im.ctypes.data_as(C.POINTER(C.c_uint8))
        m, r = np.ascontiguousarray(mt, np.int32), np.ascontiguousarray(mr, np.int32)
        uu = uvs if uvs is not None else [f(x) for x in u]
        return lib.mcpt_set_material_texture_maps(p.h, ntri_, uu[0], uu[1], uu[2], len(imgs), arr, nmat_,
                                                  m.ctypes.data_as(C.POINTER(C.c_int32)), r.ctypes.data_as(C.POINTER(C.c_int32)))

    p = mcpt_mod.PathTracer(0, mcpt_mod.default_config(spp=SPP))
    assert call(p) == -1 and b"no scene" in lib.mcpt_last_error(p.h)
    p.close()
    p = ctx(mcpt_mod, c2["scene"], c2["cam"], tex)
    first = frame(p)
    hi, lo, thi = tex["mat_mr"].copy(), tex["mat_mr"].copy(), tex["mat_tex"].copy()
    hi[3], lo[0], thi[3] = 2, -2, 2
    cases = [dict(mr=hi), dict(mr=lo), dict(mt=thi), dict(ntri_=ntri - 1), dict(ntri_=ntri + 1), dict(nmat_=nmat - 1),
             dict(nmat_=nmat + 1), dict(sizes=[(0, 8), (5, 3)]), dict(sizes=[(8, 8), (5, 0)]), dict(sizes=[(16385, 1), (5, 3)]),
             dict(sizes=[(8, 8), (1, 16385)]), dict(null_px=True), dict(uvs=[f(u[0]), None, f(u[2])])]
    for kw in cases:
        assert call(p, **kw) == -1, kw
        t = p.textures()
        assert all(np.array_equal(t[k], tex[k]) for k in ("uv0", "uv1", "uv2", "mat_tex", "mat_mr")), kw
        assert all(np.array_equal(x, y) for x, y in zip(t["textures"], imgs)), kw
    assert b"metallic-roughness" in (call(p, mr=hi), lib.mcpt_last_error(p.h))[1]
    assert p.texture_stats()["mr_in_effect"]
    assert call(p) == 0 and rays(p.iterate(1)) == (0, 0, 0) and same_film((*p.film(),), first)  # and the film is not stale
    n = C.c_int32(0)
    mr = np.zeros(nmat, np.int32)
    assert lib.mcpt_material_mr_read(p.h, C.byref(n), mr.ctypes.data_as(C.POINTER(C.c_int32))) == 0
    assert n.value == nmat and np.array_equal(mr, tex["mat_mr"])
    p.close()
