"""Normal-map textures on the device: k_material<TexNrm, ...> and the normal guide
against tests/texture_nrm_ref.py (the oracle's material stage over an exploded scene whose vertex normals
are the perturbed ones), bit for bit, and the set's life cycle on a live context.

24 x 16 film, 4 spp, texture_nrm_ref.fixture: texture_mr_ref's glossy config-2 proxy with its base + MR set
and a 6 x 7 normal map on every material but 1 and 4.  Every film comparison first asserts that the normal
maps change more than 100 of the reference film's 384 pixels."""
import ctypes as C

import numpy as np
import pytest

import emission_ref as ER
import material_fixtures as mf
import refit_ref as RF
import texture_nrm_ref as NR
import texture_ref as TR
from stage_checks import _check_stage
from test_gpu import film_close

pytestmark = pytest.mark.gpu
W, H, SPP = 24, 16, 4
F = np.float32
RAYS = ("extend_rays", "shadow_rays", "vis_rays")
NRM_KEYS = ("mat_nrm", "nrm_scale")


def u32(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def same_film(f, g):
    return np.array_equal(u32(f[0]), u32(g[0])) and np.array_equal(f[1], g[1])


def rays(st):
    return tuple(int(getattr(st, k)) for k in RAYS)


def install(p, tex):
    tans = (tex["tan0"], tex["tan1"], tex["tan2"]) if "tan0" in tex else None
    p.set_textures(tex["uv0"], tex["uv1"], tex["uv2"], tex["textures"], tex["mat_tex"], mat_mr=tex.get("mat_mr"), tangents=tans,
                   mat_nrm=tex.get("mat_nrm"), nrm_scale=tex.get("nrm_scale"))


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
    g, sets = NR.fixture(a)
    return dict(a=g, scene=mcpt_mod.desc_from_arrays(g), cam=mcpt_mod.config_camera(mcpt_mod.CONFIGS[2], W, H), **sets)


_REF = {}


def ref_film(oracle, sc, which, fixed=False, depth=5):
    """texture_nrm_ref.render of the fixture under set `which` (None: no set), computed once."""
    key = (which, fixed, depth)
    if key not in _REF:
        _REF[key] = NR.render(oracle, sc["a"], sc["cam"], W, H, SPP, max_depth=depth, fixed=fixed, tex=sc[which] if which else None)
    return _REF[key]


def guard(oracle, sc, which, against, fixed=False, depth=5):
    """More than 100 of the 384 pixels of the reference film change with the normal maps: no comparison below
    can pass because the normal lookups do nothing."""
    n = int((ref_film(oracle, sc, which, fixed, depth)[0] != ref_film(oracle, sc, against, fixed, depth)[0]).any(axis=2).sum())
    print(f"pixels changed by the normal maps ({which} against {against}, fixed={fixed}, depth={depth}): {n} of {W * H}")
    assert n > 100


def installed_equals(p, tex):
    t = p.textures()
    ok = all(np.array_equal(t[k], tex[k]) for k in ("uv0", "uv1", "uv2", "mat_tex", "mat_mr"))
    ok = ok and all(np.array_equal(u32(t[k]), u32(tex[k])) if k == "nrm_scale" else np.array_equal(t[k], tex[k]) for k in NRM_KEYS)
    return ok and all(np.array_equal(u32(x), u32(tex[k])) for x, k in zip(t["tangents"], ("tan0", "tan1", "tan2")))


# ---------------------------------------------------------------------------------------------
# 1. the material stage
@pytest.mark.parametrize("kind", ["generic", "grazing"])
@pytest.mark.parametrize("fixed", [False, True])
def test_material_stage_equals_the_oracle_on_the_exploded_scene(mcpt_mod, oracle, fixed, kind):
    """Every output of mcpt_stage_run(MATERIAL), on 1024 generic paths and on up to 1024 grazing ones (near
    n.wo = 0 the perturbed normal decides the side of the surface)."""
    import stage_fixtures as sf

    s = sf.stage_scene(mcpt_mod, 2)
    a, sets = NR.fixture(s.arrays(), seed=4)
    tex = sets["all"]
    kw = dict(max_depth=sf.DEPTH, rr_depth=sf.RR, fixed=fixed)
    if kind == "generic":
        inp = sf.material_state(a, oracle.trace_closest, 2, 1024)
    else:
        inp = mf.grazing_state(a, oracle.trace_closest, 1024, 11, 2)
    mats = np.asarray(a["mat"])[inp["hit_tri"]]
    mn = np.asarray(tex["mat_nrm"])[mats]
    assert (mn >= 0).any() and (mn < 0).any()  # mapped and unmapped materials are hit
    ref = NR.stage_material(oracle, a, tex, inp, **kw)
    no_nrm = NR.stage_material(oracle, a, sets["both"], inp, **kw)
    plain = oracle.stage_material(a, inp, **kw)
    assert (u32(ref["nee0"]) != u32(no_nrm["nee0"])).any(axis=1).sum() > 100
    for k in ("nee0", "ray_o", "ray_d", "beta"):  # selection: an unmapped material's paths are untouched
        assert np.array_equal(u32(ref[k][mn < 0]), u32(no_nrm[k][mn < 0]))
    pt = mcpt_mod.PathTracer(0, mcpt_mod.default_config(spp=sf.SPP, max_depth=sf.DEPTH, rr_depth=sf.RR, fixed=fixed))
    pt.upload_scene(mcpt_mod.desc_from_arrays(a))
    pt.set_camera(sf.stage_camera(mcpt_mod, 2))
    install(pt, tex)
    st = pt.texture_stats()
    assert st["in_effect"] and st["nrm_in_effect"] and st["nrm_materials"] == int((tex["mat_nrm"] >= 0).sum())
    _check_stage("material", pt.stage("material", inp), ref, a, oracle)
    install(pt, sets["both"])  # without the normal fields: section 20's stage
    assert "nrm_in_effect" not in pt.texture_stats()
    _check_stage("material", pt.stage("material", inp), no_nrm, a, oracle)
    pt.set_textures()  # removed: the stage of a context without textures
    _check_stage("material", pt.stage("material", inp), plain, a, oracle)
    pt.close()


# ---------------------------------------------------------------------------------------------
# 2. the film
@pytest.mark.parametrize("gpu_bvh", [False, True])
@pytest.mark.parametrize("fixed", [False, True])
def test_film_equals_the_reference_loop(mcpt_mod, oracle, c2, fixed, gpu_bvh):
    """Base + MR + normal set: bitwise in Ld and samples at one path slot, with the reference loop's ray
    counts, on the host tree and on the device-built one (whose records, and so the uv and tangent streams,
    are in Morton order)."""
    guard(oracle, c2, "all", "both", fixed)
    rLd, rsm, rc = ref_film(oracle, c2, "all", fixed)
    got = one(mcpt_mod, c2["scene"], c2["cam"], c2["all"], fixed=fixed, gpu_bvh=gpu_bvh)
    assert np.array_equal(got[1], rsm) and np.array_equal(u32(got[0]), u32(rLd))
    assert got[2] == tuple(rc[k] for k in RAYS)


@pytest.mark.parametrize("fixed", [False, True])
def test_a_normal_only_set_is_in_effect(mcpt_mod, oracle, c2, fixed):
    """Every mat_tex and mat_mr index -1: the set still shades, through k_material<TexNrm, ...>."""
    guard(oracle, c2, "nrm", None, fixed)
    rLd, rsm, rc = ref_film(oracle, c2, "nrm", fixed)
    p = ctx(mcpt_mod, c2["scene"], c2["cam"], c2["nrm"], fixed=fixed)
    st = p.texture_stats()
    assert st["in_effect"] and st["nrm_in_effect"] and st["textured_materials"] == 0 and st["mr_materials"] == 0 and st["nrm_materials"] == 8
    got = frame(p)
    p.close()
    assert np.array_equal(got[1], rsm) and np.array_equal(u32(got[0]), u32(rLd)) and got[2] == tuple(rc[k] for k in RAYS)


def test_ray_counts_follow_the_set_below_the_roulette(mcpt_mod, oracle, c2):
    """max_depth 2 (rr_depth 3): no roulette, but another normal ends other continuation samples, so the
    extension-ray count is the reference loop's and not that of the set without normal maps."""
    guard(oracle, c2, "all", "both", depth=2)
    rLd, rsm, rc = ref_film(oracle, c2, "all", depth=2)
    got = one(mcpt_mod, c2["scene"], c2["cam"], c2["all"], depth=2)
    without = one(mcpt_mod, c2["scene"], c2["cam"], c2["both"], depth=2)
    assert np.array_equal(got[1], rsm) and np.array_equal(u32(got[0]), u32(rLd))
    assert got[2] == tuple(rc[k] for k in RAYS)
    assert without[2] == tuple(ref_film(oracle, c2, "both", depth=2)[2][k] for k in RAYS) and got[2][0] != without[2][0]


@pytest.mark.parametrize("gpu_bvh", [False, True])
def test_three_path_slots(mcpt_mod, oracle, c2, gpu_bvh):
    """Slot k runs samples k, k + 3, ...: only the film's summation order differs (the project's tolerance
    for that), counts and samples exact."""
    guard(oracle, c2, "all", "both")
    rLd, rsm, rc = ref_film(oracle, c2, "all")
    got = one(mcpt_mod, c2["scene"], c2["cam"], c2["all"], slots=3, gpu_bvh=gpu_bvh)
    ok, bad = film_close(got[0], rLd)
    assert ok, bad
    assert np.array_equal(got[1], rsm) and got[2] == tuple(rc[k] for k in RAYS)


# ---------------------------------------------------------------------------------------------
# 3. identity across every instantiation
MODES = {"plain": {}, "fixed": dict(fixed=True), "samp": dict(samp=True), "samp_fixed": dict(samp=True, fixed=True),
         "mis": dict(samp=True, mis=True), "mis_fixed": dict(samp=True, mis=True, fixed=True)}


@pytest.mark.parametrize("mode", list(MODES))
def test_scale_0_and_blue_255_is_the_identity(mcpt_mod, c2, mode):
    """A normal image whose B is 255 everywhere (R, G, A arbitrary) at scale 0 gives c = (+-0, +-0, 1) and so
    m_i = N_i: the film and the ray counts of the same set without normal maps, bit for bit, through
    k_material<TexNrm, ...> against k_material<TexMr, ...>.  One wall and one sphere emit under a black
    environment, so the emitter sample, its f and the MIS weight's BRDF pdf read the normal too.  The fixture's
    own image and scales change the film: the identity is not vacuous."""
    a = ER.black(c2["a"])
    nmat = len(a["mat_params"])
    E = ER.table(nmat, {ER.MATS_LIT[0]: (3.0, 2.0, 1.0), ER.MATS_LIT[1]: (0.5, 2.0, 8.0)})
    kw = dict(E=E, **MODES[mode])
    full = c2["all"]
    flat = full["textures"][-1].copy()
    flat[..., 2] = 255
    ident = dict(full, textures=full["textures"][:-1] + [flat], nrm_scale=np.zeros(nmat, F))
    d = mcpt_mod.desc_from_arrays(a)
    want = one(mcpt_mod, d, c2["cam"], c2["both"], **kw)
    p = ctx(mcpt_mod, d, c2["cam"], ident, **kw)
    st = p.texture_stats()
    assert st["nrm_in_effect"] and st["nrm_materials"] == 8
    assert p.emitter_stats()["active"] == bool(kw.get("samp")) and p.emitter_stats()["mis"] == bool(kw.get("mis"))
    got = frame(p)
    install(p, full)
    bumped = frame(p)
    p.close()
    assert (want[0] != 0).any(axis=2).sum() > 100
    assert (bumped[0] != want[0]).any(axis=2).sum() > 100
    assert same_film(got, want) and got[2] == want[2]


# ---------------------------------------------------------------------------------------------
# 4. the older calls
def test_a_set_without_normal_fields_is_the_older_call(mcpt_mod, oracle, c2):
    """mcpt_set_material_texture_set with the new fields NULL is mcpt_set_material_texture_maps: the same film,
    the MR kernels and not the normal ones in effect, and the two calls install identical sets.  mat_nrm all
    -1 with tangents launches the MR kernels too, and reports its fields."""
    lib, both = mcpt_mod.lib(), c2["both"]
    old = one(mcpt_mod, c2["scene"], c2["cam"], both)
    p = ctx(mcpt_mod, c2["scene"], c2["cam"], None)
    u = [np.ascontiguousarray(both[k], F) for k in ("uv0", "uv1", "uv2")]
    imgs = [np.ascontiguousarray(t) for t in both["textures"]]
    arr = (mcpt_mod.Texture * len(imgs))()
    for k, im in enumerate(imgs):
        arr[k].w, arr[k].h, arr[k].rgba8 = im.shape[1], im.shape[0], im.ctypes.data_as(C.POINTER(C.c_uint8))
    mt, mr = np.ascontiguousarray(both["mat_tex"], np.int32), np.ascontiguousarray(both["mat_mr"], np.int32)
    ts = mcpt_mod.TextureSet()
    ts.ntri, ts.uv0, ts.uv1, ts.uv2 = len(u[0]), *(mcpt_mod.fptr(x) for x in u)
    ts.ntex, ts.textures, ts.nmat = len(imgs), arr, len(mt)
    ts.mat_tex, ts.mat_mr = mt.ctypes.data_as(C.POINTER(C.c_int32)), mr.ctypes.data_as(C.POINTER(C.c_int32))
    assert lib.mcpt_set_material_texture_set(p.h, C.byref(ts)) == 0
    st = p.texture_stats()
    assert st == {"bytes": st["bytes"], "textured_materials": int((mt >= 0).sum()), "in_effect": True,
                  "mr_materials": int((mr >= 0).sum()), "mr_in_effect": True}
    assert set(p.textures()) == {"uv0", "uv1", "uv2", "textures", "mat_tex", "mat_mr"}
    new = frame(p)
    install(p, both)  # the older call with the same arrays: an identical set, nothing happens
    assert rays(p.iterate(1)) == (0, 0, 0)
    none = dict(c2["all"], textures=both["textures"], mat_nrm=np.full_like(c2["all"]["mat_nrm"], -1))  # (the same two images)
    p.render_guides(1)
    install(p, none)  # the fields present, no material mapped: section 20's kernels, and no lookup changed, so
    st = p.texture_stats()  # the set is installed and the film and the guides stay
    assert st["mr_in_effect"] and st["nrm_materials"] == 0 and not st["nrm_in_effect"] and installed_equals(p, none)
    assert rays(p.iterate(1)) == (0, 0, 0) and same_film((*p.film(),), new)
    p.guides()
    scaled = dict(none, nrm_scale=(none["nrm_scale"] * F(3)))  # nor does the scale of a material without a normal map
    install(p, scaled)
    assert installed_equals(p, scaled) and rays(p.iterate(1)) == (0, 0, 0) and same_film((*p.film(),), new)
    p.clear()
    unmapped = frame(p)
    p.close()
    rLd, rsm, rc = ref_film(oracle, c2, "both")
    assert same_film(new, old) and new[2] == old[2] and same_film(unmapped, old) and unmapped[2] == old[2]
    assert np.array_equal(u32(new[0]), u32(rLd)) and new[2] == tuple(rc[k] for k in RAYS)


# ---------------------------------------------------------------------------------------------
# 5. the guides
@pytest.mark.parametrize("gpu_bvh", [False, True])
def test_normal_guide_is_the_mapped_normal(mcpt_mod, oracle, c2, gpu_bvh):
    """lens_radius = 0: every guide sample's ray is the pixel's pinhole ray, so the normal guide is
    texture_ref.hit_normal over m_i at the oracle's first hit of that ray (0 at a miss), summed in sample
    order (one sample: itself), bit for bit; albedo, depth and count are those of the same set without
    normal maps."""
    a, tex = c2["a"], c2["all"]
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
    wq = np.zeros((int(q.sum()), 3), F)
    wq[hit] = NR.hit_normal(a, tex, ix, out["ray_o"][q][hit], out["ray_d"][q][hit])
    want[q] = wq
    want = (np.zeros_like(want) + want).astype(F)  # the accumulation 0 + n (a -0 component becomes +0)
    plain_n = np.zeros((int(q.sum()), 3), F)
    u, v, _ = TR.uv_of(a, ix, out["ray_o"][q][hit], out["ray_d"][q][hit])
    plain_n[hit] = TR.hit_normal(a, ix, u, v)
    plain_n = (np.zeros_like(plain_n) + plain_n).astype(F)
    p = ctx(mcpt_mod, c2["scene"], cam, c2["both"], gpu_bvh=gpu_bvh)
    p.render_guides(3)  # a pinhole's samples share one ray: one guide sample is accumulated
    g0 = p.guides()
    install(p, tex)
    with pytest.raises(mcpt_mod.McptError):  # the installed set made the guides stale
        p.guides()
    p.render_guides(3)
    g1 = p.guides()
    p.close()
    assert hit.sum() > P // 2 and g1["count"].max() == 1
    assert np.array_equal(u32(g1["normal"].reshape(-1, 3)), u32(want))
    assert np.array_equal(u32(g0["normal"].reshape(-1, 3)[q]), u32(plain_n))
    assert (u32(g1["normal"]) != u32(g0["normal"])).any(axis=2).sum() > 100
    for k in ("albedo", "depth", "count"):
        assert np.array_equal(g1[k], g0[k]), k


# ---------------------------------------------------------------------------------------------
# 6. geometry updates
@pytest.mark.parametrize("mode", ["refit", "rebuild"])
def test_geometry_updates_keep_the_set(mcpt_mod, c2, mode):
    """After an update the film equals a fresh upload of the moved mesh with the set installed again (the
    tangents are the installed ones: the set is the caller's)."""
    gpu = mode == "rebuild"
    tex = c2["all"]
    m = RF.refitted_desc_arrays(c2["a"], amp=0.02)
    p = ctx(mcpt_mod, c2["scene"], c2["cam"], tex, gpu_bvh=gpu)
    before = frame(p)
    p.update_geometry(m["v0"], m["v1"], m["v2"], mode=mode)
    assert installed_equals(p, tex) and p.texture_stats()["nrm_in_effect"]
    moved = frame(p)
    p.close()
    fresh = one(mcpt_mod, mcpt_mod.desc_from_arrays(m), c2["cam"], tex, gpu_bvh=gpu)
    assert same_film(moved, fresh) and moved[2] == fresh[2] and not same_film(moved, before)


# ---------------------------------------------------------------------------------------------
# 7. state
def test_identical_changed_and_dropped_sets(mcpt_mod, c2):
    full, both = c2["all"], c2["both"]
    never = one(mcpt_mod, c2["scene"], c2["cam"], None)
    p = ctx(mcpt_mod, c2["scene"], c2["cam"], full)
    p.set_variance_fill()
    first = frame(p)
    assert installed_equals(p, full) and len(p.textures()["textures"]) == 3
    install(p, {k: (v.copy() if isinstance(v, np.ndarray) else [x.copy() for x in v]) for k, v in full.items()})
    assert rays(p.iterate(1)) == (0, 0, 0) and same_film((*p.film(),), first)  # an identical set: nothing happens
    # each new array alone: the film stale, the guides stale, the temporal history dropped
    for change in ("nrm_scale", "mat_nrm", "tan1"):
        p.render_guides(1)
        p.guides()
        p.temporal_accumulate()
        p.temporal()
        other = full[change].copy()
        if change == "nrm_scale":
            other[0] = 0.25
        elif change == "mat_nrm":
            other[0] = -1
        else:
            other[:, 3] = -other[:, 3]
        install(p, dict(full, **{change: other}))
        with pytest.raises(mcpt_mod.McptError):
            p.temporal()
        with pytest.raises(mcpt_mod.McptError):
            p.guides()
        st = p.iterate(1)
        assert st.extend_rays > 0 and p.film()[1].max() < SPP, change
        assert not same_film(frame(p), first), change
        install(p, full)
        assert same_film(frame(p), first), change
    install(p, both)  # the normal fields gone: section 20's kernels, its film, and its keys
    s = p.texture_stats()
    assert s["in_effect"] and s["mr_in_effect"] and "nrm_in_effect" not in s and "mat_nrm" not in p.textures()
    assert same_film(frame(p), one(mcpt_mod, c2["scene"], c2["cam"], both))
    install(p, full)
    assert same_film(frame(p), first)
    p.upload_scene(c2["scene"])  # an upload drops the set
    assert p.textures() is None and p.texture_stats() == {"bytes": 0, "textured_materials": 0, "in_effect": False}
    assert same_film(frame(p), never)
    p.close()


def test_rejected_sets_leave_the_installed_one(mcpt_mod, c2):
    lib, tex, a = mcpt_mod.lib(), c2["all"], c2["a"]
    ntri, nmat = len(a["mat"]), len(a["mat_params"])
    fp = lambda x: None if x is None else np.ascontiguousarray(x, F).ctypes.data_as(C.POINTER(C.c_float))
    ip = lambda x: None if x is None else np.ascontiguousarray(x, np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    imgs = [np.ascontiguousarray(t) for t in tex["textures"]]

    def call(p, **over):
        v = dict(tex, **over)
        arr = (mcpt_mod.Texture * len(imgs))()
        for k, im in enumerate(imgs):
            arr[k].w, arr[k].h, arr[k].rgba8 = im.shape[1], im.shape[0], im.ctypes.data_as(C.POINTER(C.c_uint8))
        keep = [np.ascontiguousarray(v[k], F) if v[k] is not None else None for k in ("uv0", "uv1", "uv2", "tan0", "tan1", "tan2", "nrm_scale")]
        keep += [np.ascontiguousarray(v[k], np.int32) if v[k] is not None else None for k in ("mat_tex", "mat_mr", "mat_nrm")]
        ts = mcpt_mod.TextureSet()
        ts.ntri, ts.ntex, ts.textures, ts.nmat = v.get("ntri_", ntri), len(imgs), arr, v.get("nmat_", nmat)
        ts.uv0, ts.uv1, ts.uv2, ts.tan0, ts.tan1, ts.tan2, ts.nrm_scale = (fp(x) for x in keep[:7])
        ts.mat_tex, ts.mat_mr, ts.mat_nrm = (ip(x) for x in keep[7:])
        return lib.mcpt_set_material_texture_set(p.h, C.byref(ts))

    p = mcpt_mod.PathTracer(0, mcpt_mod.default_config(spp=SPP))
    assert call(p) == -1 and b"no scene" in lib.mcpt_last_error(p.h)
    assert lib.mcpt_set_material_texture_set(p.h, None) == -1
    p.close()
    p = ctx(mcpt_mod, c2["scene"], c2["cam"], tex)
    first = frame(p)
    hi, lo = tex["mat_nrm"].copy(), tex["mat_nrm"].copy()
    hi[3], lo[0] = 3, -2
    bad_scale = [tex["nrm_scale"].copy() for _ in range(3)]
    bad_scale[0][2], bad_scale[1][9], bad_scale[2][0] = np.inf, np.nan, -np.inf
    bad_tan = [tex[k].copy() for k in ("tan0", "tan1", "tan2")]
    bad_tan[0][5, 0], bad_tan[1][0, 3], bad_tan[2][-1, 2] = np.nan, np.inf, -np.inf
    cases = [(dict(mat_nrm=hi), b"normal texture index"), (dict(mat_nrm=lo), b"normal texture index"),
             (dict(tan0=None, tan1=None, tan2=None), b"needs tangents"), (dict(tan1=None), b"tangent arrays"),
             (dict(tan0=None, tan2=None), b"tangent arrays"), (dict(nrm_scale=bad_scale[0]), b"normal scale"),
             (dict(nrm_scale=bad_scale[1]), b"normal scale"), (dict(nrm_scale=bad_scale[2]), b"normal scale"),
             (dict(tan0=bad_tan[0]), b"tangent component"), (dict(tan1=bad_tan[1]), b"tangent component"),
             (dict(tan2=bad_tan[2]), b"tangent component"), (dict(ntri_=ntri - 1), b"ntri"), (dict(nmat_=nmat + 1), b"nmat"),
             (dict(uv1=None), b"null"), (dict(mat_tex=None), b"null")]
    for over, msg in cases:
        assert call(p, **over) == -1 and msg in lib.mcpt_last_error(p.h), (over.keys(), lib.mcpt_last_error(p.h))
        assert installed_equals(p, tex), over.keys()
    assert p.texture_stats()["nrm_in_effect"]
    assert call(p) == 0 and rays(p.iterate(1)) == (0, 0, 0) and same_film((*p.film(),), first)  # and the film is not stale
    assert call(p, nrm_scale=None, mat_nrm=np.full(nmat, -1, np.int32), tan0=None, tan1=None, tan2=None) == 0  # no tangents needed
    t = p.textures()
    assert t["tangents"] is None and np.array_equal(t["nrm_scale"], np.ones(nmat, F)) and not p.texture_stats()["nrm_in_effect"]
    n, nt = C.c_int32(0), C.c_int32(-1)
    assert lib.mcpt_material_normal_read(p.h, C.byref(n), C.byref(nt), None, None, None, None, None) == 0 and (n.value, nt.value) == (nmat, 0)
    p.close()
