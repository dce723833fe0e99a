"""sRGB base colour on the device: the sRGB sampler, k_material<TexSrgb, ...> and the
albedo guide against tests/texture_srgb_ref.py (the oracle's material stage over an exploded scene whose base
colours went through the decode table), bit for bit, and the flag's life cycle on a live context.

24 x 16 film, 4 spp, texture_srgb_ref.fixture: texture_nrm_ref's base + MR + normal set with the two images that
serve as base colours (and as other materials' MR textures) flagged.  Every film comparison first asserts that
the flag changes more than 100 of the reference film's 384 pixels."""
import ctypes as C

import numpy as np
import pytest

import emission_ref as ER
import refit_ref as RF
import texture_nrm_ref as NR
import texture_ref as TR
import texture_srgb_ref as SR
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
    tans = (tex["tan0"], tex["tan1"], tex["tan2"]) if "tan0" in tex else None
    p.set_textures(tex["uv0"], tex["uv1"], tex["uv2"], tex["textures"], tex["mat_tex"], mat_mr=tex.get("mat_mr"), tangents=tans,
                   mat_nrm=tex.get("mat_nrm"), nrm_scale=tex.get("nrm_scale"), tex_flags=tex.get("tex_flags"))


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
    g, sets = SR.fixture(a)
    return dict(a=g, scene=mcpt_mod.desc_from_arrays(g), cam=mcpt_mod.config_camera(mcpt_mod.CONFIGS[2], W, H), **sets)


_REF = {}


def ref_film(oracle, sc, which, fixed=False, depth=5):
    """texture_srgb_ref.render of the fixture under set `which`, computed once."""
    key = (which, fixed, depth)
    if key not in _REF:
        _REF[key] = SR.render(oracle, sc["a"], sc["cam"], W, H, SPP, max_depth=depth, fixed=fixed, tex=sc[which] if which else None)
    return _REF[key]


def guard(oracle, sc, which, against, fixed=False, depth=5):
    """More than 100 of the 384 pixels of the reference film change with the flag: no comparison below can pass
    because the decode does nothing."""
    n = int((ref_film(oracle, sc, which, fixed, depth)[0] != ref_film(oracle, sc, against, fixed, depth)[0]).any(axis=2).sum())
    print(f"pixels changed by the sRGB flag ({which} against {against}, fixed={fixed}, depth={depth}): {n} of {W * H}")
    assert n > 100


def installed_equals(p, tex):
    t = p.textures()
    ok = all(np.array_equal(t[k], tex[k]) for k in ("uv0", "uv1", "uv2", "mat_tex", "mat_mr", "mat_nrm"))
    ok = ok and all(np.array_equal(x, y) for x, y in zip(t["textures"], tex["textures"])) and len(t["textures"]) == len(tex["textures"])
    if tex.get("tex_flags") is None:
        return ok and "tex_flags" not in t
    return ok and t["tex_flags"].dtype == np.uint32 and np.array_equal(t["tex_flags"], tex["tex_flags"])


# ---------------------------------------------------------------------------------------------
# 1. the lookup alone
def special_uvs(rng, n):
    uv = (rng.random((n, 2)) * 6 - 3).astype(F)
    uv[:8] = [[np.nan, 0.3], [0.3, np.nan], [65536.0, 0.2], [0.2, -65536.0], [np.inf, -np.inf], [65535.996, -65535.996], [0.0, 1.0], [-0.0, 0.5]]
    return uv


def test_sampler_returns_the_table_at_texel_centres(mcpt_mod):
    """A 16 x 16 image holding every byte (R ascending, G descending), sampled at the exact texel centres: L[c]."""
    img = np.arange(256, dtype=np.uint8).reshape(16, 16, 1).repeat(4, axis=2)
    img[..., 1] = img[..., 0][::-1, ::-1]
    jj, ii = np.meshgrid(np.arange(16), np.arange(16), indexing="ij")
    uv = np.stack([(ii + 0.5) / 16, (jj + 0.5) / 16], -1).reshape(-1, 2).astype(F)
    p = mcpt_mod.PathTracer(0, mcpt_mod.default_config(spp=1))
    got = p.texture_sample(img, uv, srgb=True)
    plain = p.texture_sample(img, uv)
    p.close()
    L = SR.table()
    assert np.array_equal(u32(got[:, 0]), u32(L)) and np.array_equal(u32(got[:, 1]), u32(L[::-1])) and np.array_equal(u32(got[:, 2]), u32(L))
    assert np.array_equal(u32(plain), u32(TR.lookup(img, uv)))  # the unflagged sampler is what it was


def test_sampler_equals_the_reference_lookup(mcpt_mod):
    """Random and special uvs (NaN, >= 65536 in magnitude, wrap on both sides) over 1 x 1, 5 x 3 and 8 x 8 images
    that hold bytes 0, 10, 11 and 255 (both ends of both branches): bit for bit; an unknown flag is refused."""
    rng = np.random.default_rng(2)
    p = mcpt_mod.PathTracer(0, mcpt_mod.default_config(spp=1))
    for h, w in ((1, 1), (3, 5), (8, 8)):
        img = rng.integers(0, 256, (h, w, 4)).astype(np.uint8)
        img.reshape(-1)[:4] = [0, 10, 11, 255]
        uv = special_uvs(rng, 700)  # three blocks of 256 threads, the last partly filled
        assert np.array_equal(u32(p.texture_sample(img, uv, srgb=True)), u32(SR.lookup(img, uv, SR.table()))), (h, w)
        assert np.array_equal(u32(p.texture_sample(img, uv)), u32(TR.lookup(img, uv))), (h, w)
    im, uv, out = np.zeros((1, 1, 4), np.uint8), np.zeros((1, 2), F), np.zeros((1, 3), F)
    rc = mcpt_mod.lib().mcpt_texture_sample_run_ex(p.h, 1, 1, im.ctypes.data_as(C.POINTER(C.c_uint8)), 2, 1, mcpt_mod.fptr(uv), mcpt_mod.fptr(out))
    assert rc == -1 and b"unknown texture flag" in mcpt_mod.lib().mcpt_last_error(p.h)
    p.close()


# ---------------------------------------------------------------------------------------------
# 2. the material stage
@pytest.mark.parametrize("fixed", [False, True])
def test_material_stage_equals_the_oracle_on_the_exploded_scene(mcpt_mod, oracle, fixed):
    """Every output of mcpt_stage_run(MATERIAL) on 1024 paths under the flagged base + MR + normal set."""
    import stage_fixtures as sf

    s = sf.stage_scene(mcpt_mod, 2)
    a, sets = SR.fixture(s.arrays(), seed=4)
    tex = sets["srgb"]
    kw = dict(max_depth=sf.DEPTH, rr_depth=sf.RR, fixed=fixed)
    inp = sf.material_state(a, oracle.trace_closest, 2, 1024)
    on = SR.flagged_materials(tex, len(a["mat_params"]))[np.asarray(a["mat"])[inp["hit_tri"]]]
    assert on.any() and (~on).any()  # flagged and unflagged materials are hit
    ref = SR.stage_material(oracle, a, tex, inp, **kw)
    unflagged = NR.stage_material(oracle, a, sets["all"], inp, **kw)
    assert (u32(ref["nee0"]) != u32(unflagged["nee0"])).any(axis=1).sum() > 100
    for k in ("nee0", "ray_o", "ray_d", "beta"):  # selection: an unflagged material's paths are untouched
        assert np.array_equal(u32(ref[k][~on]), u32(unflagged[k][~on]))
    pt = mcpt_mod.PathTracer(0, mcpt_mod.default_config(spp=sf.SPP, max_depth=sf.DEPTH, rr_depth=sf.RR, fixed=fixed))
    pt.upload_scene(mcpt_mod.desc_from_arrays(a))
    pt.set_camera(sf.stage_camera(mcpt_mod, 2))
    install(pt, tex)
    st = pt.texture_stats()
    assert st["in_effect"] and st["srgb_in_effect"] and st["srgb_materials"] == int(SR.flagged_materials(tex, len(a["mat_params"])).sum())
    _check_stage("material", pt.stage("material", inp), ref, a, oracle)
    install(pt, sets["all"])  # without the flags: section 21's stage, and its keys
    assert "srgb_in_effect" not in pt.texture_stats()
    _check_stage("material", pt.stage("material", inp), unflagged, a, oracle)
    pt.close()


# ---------------------------------------------------------------------------------------------
# 3. the film
@pytest.mark.parametrize("gpu_bvh", [False, True])
@pytest.mark.parametrize("fixed", [False, True])
def test_film_equals_the_reference_loop(mcpt_mod, oracle, c2, fixed, gpu_bvh):
    """Flagged base + MR + normal set: bitwise in Ld and samples at one path slot, with the reference loop's ray
    counts, on the host tree and on the device-built one."""
    guard(oracle, c2, "srgb", "all", fixed)
    rLd, rsm, rc = ref_film(oracle, c2, "srgb", fixed)
    got = one(mcpt_mod, c2["scene"], c2["cam"], c2["srgb"], fixed=fixed, gpu_bvh=gpu_bvh)
    assert np.array_equal(got[1], rsm) and np.array_equal(u32(got[0]), u32(rLd))
    assert got[2] == tuple(rc[k] for k in RAYS)


@pytest.mark.parametrize("fixed", [False, True])
def test_an_srgb_base_only_set_runs_level_4(mcpt_mod, oracle, c2, fixed):
    """No MR texture, no normal map, no tangents: the flagged base colour alone still launches the sRGB kernels
    (whose MR and normal lookups find no texture)."""
    guard(oracle, c2, "srgb_base", "base", fixed)
    rLd, rsm, rc = ref_film(oracle, c2, "srgb_base", fixed)
    p = ctx(mcpt_mod, c2["scene"], c2["cam"], c2["srgb_base"], fixed=fixed)
    st = p.texture_stats()
    assert st["in_effect"] and st["srgb_in_effect"] and st["srgb_materials"] == 8 and st["mr_materials"] == 0 and "nrm_in_effect" not in st
    got = frame(p)
    p.close()
    assert np.array_equal(got[1], rsm) and np.array_equal(u32(got[0]), u32(rLd)) and got[2] == tuple(rc[k] for k in RAYS)


def test_depth_2(mcpt_mod, oracle, c2):
    guard(oracle, c2, "srgb", "all", depth=2)
    rLd, rsm, rc = ref_film(oracle, c2, "srgb", depth=2)
    got = one(mcpt_mod, c2["scene"], c2["cam"], c2["srgb"], depth=2)
    assert np.array_equal(got[1], rsm) and np.array_equal(u32(got[0]), u32(rLd)) and got[2] == tuple(rc[k] for k in RAYS)


def test_three_path_slots(mcpt_mod, oracle, c2):
    """Slot k runs samples k, k + 3, ...: only the film's summation order differs (the project's 1e-4 tolerance
    for that), counts and samples exact."""
    guard(oracle, c2, "srgb", "all")
    rLd, rsm, rc = ref_film(oracle, c2, "srgb")
    got = one(mcpt_mod, c2["scene"], c2["cam"], c2["srgb"], slots=3)
    ok, bad = film_close(got[0], rLd)
    assert ok, bad
    assert np.array_equal(got[1], rsm) and got[2] == tuple(rc[k] for k in RAYS)


# ---------------------------------------------------------------------------------------------
# 4. identity across every instantiation
MODES = {"plain": {}, "fixed": dict(fixed=True), "samp": dict(samp=True), "samp_fixed": dict(samp=True, fixed=True),
         "mis": dict(samp=True, mis=True), "mis_fixed": dict(samp=True, mis=True, fixed=True)}


@pytest.mark.parametrize("mode", list(MODES))
def test_bytes_0_and_255_decode_to_themselves(mcpt_mod, c2, mode):
    """L[0] = 0 = 0 / 255 and L[255] = 1 = 255 / 255: base-colour images of those two bytes alone give, flagged,
    the film and the ray counts of the same set unflagged, bit for bit, through k_material<TexSrgb, ...> against
    k_material<TexNrm, ...>.  One wall and one sphere emit under a black environment, so the emitter sample, its f
    and the MIS weight's BRDF pdf read the base colour too.  The same images with 0 replaced by 128 change the
    film when flagged: the identity is not vacuous."""
    a = ER.black(c2["a"])
    nmat = len(a["mat_params"])
    E = ER.table(nmat, {ER.MATS_LIT[0]: (3.0, 2.0, 1.0), ER.MATS_LIT[1]: (0.5, 2.0, 8.0)})
    kw = dict(E=E, **MODES[mode])
    full = c2["all"]
    rng = np.random.default_rng(5)
    ends = [(rng.integers(0, 2, t.shape) * 255).astype(np.uint8) for t in full["textures"][:2]]
    for t in ends:
        t[..., 3] = 77
    mids = [np.where(t == 0, 128, t).astype(np.uint8) for t in ends]
    flags = np.array([1, 1, 0], np.uint32)
    d = mcpt_mod.desc_from_arrays(a)
    want = one(mcpt_mod, d, c2["cam"], dict(full, textures=ends + full["textures"][2:]), **kw)
    p = ctx(mcpt_mod, d, c2["cam"], dict(full, textures=ends + full["textures"][2:], tex_flags=flags), **kw)
    st = p.texture_stats()
    assert st["srgb_in_effect"] and st["srgb_materials"] == 8 and st["nrm_in_effect"]
    assert p.emitter_stats()["active"] == bool(kw.get("samp")) and p.emitter_stats()["mis"] == bool(kw.get("mis"))
    got = frame(p)
    install(p, dict(full, textures=mids + full["textures"][2:], tex_flags=flags))
    decoded = frame(p)
    install(p, dict(full, textures=mids + full["textures"][2:]))
    stored = frame(p)
    p.close()
    assert (want[0] != 0).any(axis=2).sum() > 100
    assert (decoded[0] != stored[0]).any(axis=2).sum() > 100
    assert same_film(got, want) and got[2] == want[2]


@pytest.mark.parametrize("mode", ["samp", "samp_fixed", "mis", "mis_fixed"])
def test_sampling_instantiations_equal_the_emitter_reference(mcpt_mod, oracle, c2, mode):
    """The four emitter-sampling instantiations of k_material<TexSrgb, ...> against
    texture_srgb_ref.render_emitters, bit for bit with exact ray and emitter-ray counts: a black environment, one
    wall and one sphere emitting, the flagged base + MR set (no normal maps: that loop's normal is the traced one).
    The emitter sample's f, its MIS weight and pdf_s read the decoded colour of every byte the images hold."""
    a = ER.black(c2["a"])
    E = ER.table(len(a["mat_params"]), {ER.MATS_LIT[0]: (3.0, 2.0, 1.0), ER.MATS_LIT[1]: (0.5, 2.0, 8.0)})
    kw = MODES[mode]
    fixed, mis = bool(kw.get("fixed")), bool(kw.get("mis"))
    rLd, rsm, rc = SR.render_emitters(oracle, a, c2["cam"], W, H, SPP, c2["srgb_both"], E, fixed=fixed, mis=mis)
    stored = SR.render_emitters(oracle, a, c2["cam"], W, H, SPP, c2["both"], E, fixed=fixed, mis=mis)
    assert (rLd != stored[0]).any(axis=2).sum() > 100  # the flag changes this reference film
    p = ctx(mcpt_mod, mcpt_mod.desc_from_arrays(a), c2["cam"], c2["srgb_both"], E=E, **kw)
    p.set_skip_discarded(False)  # every stage as the reference runs it: with the switch on fewer emitter rays are made
    st, es = p.texture_stats(), p.emitter_stats()
    assert st["srgb_in_effect"] and st["mr_in_effect"] and es["active"] and es["mis"] == mis
    got = frame(p)
    emitter_rays = p.emitter_stats()["emitter_rays"]
    p.close()
    assert np.array_equal(got[1], rsm) and np.array_equal(u32(got[0]), u32(rLd))
    assert got[2] == tuple(rc[k] for k in RAYS) and emitter_rays == rc["emitter_rays"] > 0


# ---------------------------------------------------------------------------------------------
# 5. a flag no base-colour slot reads
def test_a_flag_on_a_texture_no_base_slot_uses_changes_nothing(mcpt_mod, oracle, c2):
    """Only the normal image flagged: the set launches what the unflagged set launches (the normal-map kernels, not
    the sRGB ones) and gives its film; installed over the unflagged set it is read back, and the film and the
    guides stay; a flag on a base-colour image then makes them stale."""
    unused, full = c2["srgb_unused"], c2["all"]
    rLd, rsm, rc = ref_film(oracle, c2, "all")
    p = ctx(mcpt_mod, c2["scene"], c2["cam"], full)
    first = frame(p)
    assert np.array_equal(u32(first[0]), u32(rLd)) and first[2] == tuple(rc[k] for k in RAYS)
    assert "srgb_in_effect" not in p.texture_stats() and "tex_flags" not in p.textures()
    p.render_guides(1)
    install(p, unused)
    st = p.texture_stats()
    assert st["srgb_materials"] == 0 and not st["srgb_in_effect"] and st["nrm_in_effect"] and installed_equals(p, unused)
    assert rays(p.iterate(1)) == (0, 0, 0) and same_film((*p.film(),), first)
    p.guides()
    install(p, dict(full, tex_flags=np.zeros(3, np.uint32)))  # the field present, every word 0: likewise
    assert rays(p.iterate(1)) == (0, 0, 0) and same_film((*p.film(),), first) and not p.texture_stats()["srgb_in_effect"]
    p.guides()
    p.clear()
    again = frame(p)
    install(p, c2["srgb"])
    with pytest.raises(mcpt_mod.McptError):
        p.guides()
    assert p.texture_stats()["srgb_in_effect"] and p.iterate(1).extend_rays > 0
    p.close()
    assert same_film(again, first) and again[2] == first[2]
    fresh = one(mcpt_mod, c2["scene"], c2["cam"], unused)
    assert same_film(fresh, first) and fresh[2] == first[2]


# ---------------------------------------------------------------------------------------------
# 6. the guides
@pytest.mark.parametrize("gpu_bvh", [False, True])
def test_albedo_guide_is_the_decoded_base_colour(mcpt_mod, oracle, c2, gpu_bvh):
    """lens_radius = 0: every guide sample's ray is the pixel's pinhole ray, so the albedo guide is
    texture_srgb_ref.base_colour at the oracle's first hit of that ray (1 at a miss), bit for bit; normal, depth
    and count are those of the unflagged set (the mapped normal of section 21)."""
    a, tex = c2["a"], c2["srgb"]
    cam = mcpt_mod.make_camera((0.0, 0.0, 3.5), aspect=F(W) / F(H), lens_radius=0.0)
    P = W * H
    dead = {"flags": np.ones(P, np.uint32), "hit_tri": np.full(P, -1, np.int32), "ray_d": np.zeros((P, 3), F),
            "beta": np.zeros((P, 4), F), "nee0": np.zeros((P, 4), F), "nee1": np.zeros((P, 4), F),
            "vis": np.zeros((P, 2), np.uint8), "Ld": np.zeros((P, 3), F), "samples": np.zeros(P, np.uint32)}
    out = oracle.stage_logic(a, cam, W, H, dead, spp=1)
    q = (out["queued"] & 1) != 0
    _, _, tri = oracle.trace_closest(a, out["ray_o"][q], out["ray_d"][q])
    hit = tri >= 0
    ix = np.argsort(a["tri_id"])[tri[hit]]
    want = np.zeros((P, 3), F)
    wq = np.ones((int(q.sum()), 3), F)
    wq[hit] = SR.base_colour(a, tex, ix, out["ray_o"][q][hit], out["ray_d"][q][hit])
    want[q] = wq
    p = ctx(mcpt_mod, c2["scene"], cam, c2["all"], gpu_bvh=gpu_bvh)
    p.render_guides(3)  # a pinhole's samples share one ray: one guide sample is accumulated
    g0 = p.guides()
    install(p, tex)
    with pytest.raises(mcpt_mod.McptError):  # the installed set made the guides stale
        p.guides()
    p.render_guides(3)
    g1 = p.guides()
    p.close()
    assert hit.sum() > P // 2 and g1["count"].max() == 1
    assert np.array_equal(u32(g1["albedo"].reshape(-1, 3)), u32(want))
    assert (u32(g1["albedo"]) != u32(g0["albedo"])).any(axis=2).sum() > 100
    for k in ("normal", "depth", "count"):
        assert np.array_equal(g1[k].view(np.uint32), g0[k].view(np.uint32)), k


# ---------------------------------------------------------------------------------------------
# 7. geometry updates
@pytest.mark.parametrize("mode", ["refit", "rebuild"])
def test_geometry_updates_keep_the_set(mcpt_mod, c2, mode):
    gpu = mode == "rebuild"
    tex = c2["srgb"]
    m = RF.refitted_desc_arrays(c2["a"], amp=0.02)
    p = ctx(mcpt_mod, c2["scene"], c2["cam"], tex, gpu_bvh=gpu)
    before = frame(p)
    p.update_geometry(m["v0"], m["v1"], m["v2"], mode=mode)
    assert installed_equals(p, tex) and p.texture_stats()["srgb_in_effect"]
    moved = frame(p)
    p.close()
    fresh = one(mcpt_mod, mcpt_mod.desc_from_arrays(m), c2["cam"], tex, gpu_bvh=gpu)
    assert same_film(moved, fresh) and moved[2] == fresh[2] and not same_film(moved, before)


# ---------------------------------------------------------------------------------------------
# 8. state
def test_identical_changed_and_dropped_flags(mcpt_mod, c2):
    flagged, full = c2["srgb"], c2["all"]
    unflagged_film = one(mcpt_mod, c2["scene"], c2["cam"], full)
    p = ctx(mcpt_mod, c2["scene"], c2["cam"], flagged)
    p.set_variance_fill()
    first = frame(p)
    assert installed_equals(p, flagged) and not same_film(first, unflagged_film)
    install(p, {k: (v.copy() if isinstance(v, np.ndarray) else [x.copy() for x in v]) for k, v in flagged.items()})
    assert rays(p.iterate(1)) == (0, 0, 0) and same_film((*p.film(),), first)  # an identical set: nothing happens
    # one flag of a base-colour image cleared: the film stale, the guides stale, the temporal history dropped
    p.render_guides(1)
    p.guides()
    p.temporal_accumulate()
    p.temporal()
    install(p, dict(flagged, tex_flags=np.array([1, 0, 0], np.uint32)))
    with pytest.raises(mcpt_mod.McptError):
        p.temporal()
    with pytest.raises(mcpt_mod.McptError):
        p.guides()
    st = p.iterate(1)
    assert st.extend_rays > 0 and p.film()[1].max() < SPP and p.texture_stats()["srgb_in_effect"]
    half = frame(p)
    assert not same_film(half, first) and not same_film(half, unflagged_film)
    install(p, full)  # the flags gone: section 21's kernels, film and keys
    s = p.texture_stats()
    assert s["nrm_in_effect"] and "srgb_in_effect" not in s and "tex_flags" not in p.textures()
    assert same_film(frame(p), unflagged_film)
    install(p, flagged)
    assert same_film(frame(p), first)
    p.upload_scene(c2["scene"])  # an upload drops the set
    assert p.textures() is None and p.texture_stats() == {"bytes": 0, "textured_materials": 0, "in_effect": False}
    p.close()


def test_an_unknown_flag_bit_leaves_the_installed_set(mcpt_mod, c2):
    tex = c2["srgb"]
    p = ctx(mcpt_mod, c2["scene"], c2["cam"], tex)
    first = frame(p)
    for bad in ([1, 2, 0], [0, 0, 0x80000000], [3, 1, 0]):
        with pytest.raises(mcpt_mod.McptError, match="unknown texture flag"):
            install(p, dict(tex, tex_flags=np.array(bad, np.uint32)))
        assert installed_equals(p, tex)
    with pytest.raises(ValueError):
        install(p, dict(tex, tex_flags=np.array([1, 1], np.uint32)))
    assert p.texture_stats()["srgb_in_effect"] and rays(p.iterate(1)) == (0, 0, 0) and same_film((*p.film(),), first)
    n = C.c_int32(-1)
    fl = np.zeros(3, np.uint32)
    L = mcpt_mod.lib().mcpt_material_texture_flags_read
    assert L(p.h, C.byref(n), fl.ctypes.data_as(C.POINTER(C.c_uint32))) == 0 and n.value == 3 and np.array_equal(fl, tex["tex_flags"])
    p.close()


def test_upload_scene_carries_a_scenes_flags(mcpt_mod, c2):
    """A Scene whose base-colour texture was attached with srgb=True installs flagged through upload_scene."""
    s = mcpt_mod.build_config_scene(2)
    t = s.textures()
    assert t is None
    img = np.random.default_rng(8).integers(0, 256, (4, 4, 4)).astype(np.uint8)
    s.set_texture(0, img, srgb=True)
    p = mcpt_mod.PathTracer(0, mcpt_mod.default_config(spp=SPP))
    p.upload_scene(s)
    st, got = p.texture_stats(), p.textures()
    p.close()
    assert st["srgb_in_effect"] and st["srgb_materials"] == 1 and np.array_equal(got["tex_flags"], [1])
