"""Base-colour textures on the device: the lookup kernel, k_material's textured
instantiations and the textured guide pass against tests/texture_ref.py (numpy restatements and the
oracle's material stage over an exploded scene), bit for bit, and the set's life cycle on a live context.

24 x 16 film, 4 spp, config 2's proxy (4810 triangles, 10 materials) unless stated."""
import ctypes as C

import numpy as np
import pytest

import emission_ref as ER
import refit_ref as RF
import texture_ref as TR
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
    p.set_textures(tex["uv0"], tex["uv1"], tex["uv2"], tex["textures"], tex["mat_tex"])


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
    s, a = scene_c2
    # two textures of different sizes dealt over the materials, two materials without, uvs beyond [0, 1]
    tex = TR.random_set(a, sizes=((8, 8), (3, 5)), untextured=(1, 6))
    return dict(scene=s, a=a, cam=mcpt_mod.config_camera(mcpt_mod.CONFIGS[2], W, H), tex=tex)


@pytest.fixture(scope="module")
def cube(mcpt_mod, scene_cube):
    """Cube.glb with its own TEXCOORD_0 and one 5 x 3 texture."""
    s, a = scene_cube
    rng = np.random.default_rng(11)
    tex = {"uv0": a["uv0"], "uv1": a["uv1"], "uv2": a["uv2"], "textures": [rng.integers(0, 256, (3, 5, 4)).astype(np.uint8)],
           "mat_tex": np.zeros(1, np.int32)}
    return dict(scene=s, a=a, cam=mcpt_mod.make_camera((0.3, 0.1, 3.0), aspect=F(W) / F(H)), tex=tex)


_REF = {}


def ref_film(oracle, sc, name, fixed=False, depth=5, tex=True):
    """texture_ref.render of a fixture, computed once per (scene, mode, depth, textured)."""
    key = (name, fixed, depth, tex)
    if key not in _REF:
        _REF[key] = TR.render(oracle, sc["a"], sc["cam"], W, H, SPP, max_depth=depth, fixed=fixed, tex=sc["tex"] if tex else None)
    return _REF[key]


# ---------------------------------------------------------------------------------------------
# 1. the lookup
def lookup_uvs(w, h):
    rng = np.random.default_rng(w * 131 + h)
    ii, jj = np.meshgrid(np.arange(-w, 2 * w + 1), np.arange(-h, 2 * h + 1))
    edges = np.stack([ii / w, jj / h], -1).reshape(-1, 2)  # texel edges, beyond [0, 1] on both sides
    centres = np.stack([(ii + 0.5) / w, (jj + 0.5) / h], -1).reshape(-1, 2)
    k = np.arange(-512, 1025)
    frac = np.stack([k / (512.0 * w), (k[::-1] + 0.5) / (512.0 * h)], -1)  # texel fractions of k / 512: where q8 rounds
    wide = rng.random((2048, 2)) * 9 - 4
    far = rng.random((256, 2)) * 131000 - 65500  # |uv| up to just below 65536
    bad = np.array([[np.nan, 0.3], [0.3, np.nan], [np.nan, np.nan], [65536.0, 0.3], [0.3, -65536.0], [np.inf, 0.3],
                    [0.3, -np.inf], [1e30, -1e30], [65535.996, 0.3], [-65535.996, 0.3], [0.0, 0.0], [-0.0, 1.0]])
    return np.concatenate([edges, centres, frac, wide, far, bad]).astype(F)


@pytest.mark.parametrize("w,h", [(1, 1), (5, 3), (8, 8)])
def test_lookup_equals_the_numpy_lookup(mcpt_mod, w, h):
    rng = np.random.default_rng(100 * w + h)
    img = rng.integers(0, 256, (h, w, 4)).astype(np.uint8)
    uv = lookup_uvs(w, h)
    p = mcpt_mod.PathTracer(0, mcpt_mod.default_config(spp=1))  # neither a scene nor a film
    got = p.texture_sample(img, uv)
    p.close()
    want = TR.lookup(img, uv)
    bad = (u32(got) != u32(want)).any(axis=1)
    assert not bad.any(), (int(bad.sum()), uv[bad][:4], got[bad][:4], want[bad][:4])
    assert len(np.unique(u32(want), axis=0)) > (1 if w * h == 1 else 100)


# ---------------------------------------------------------------------------------------------
# 2. the material stage
@pytest.mark.parametrize("fixed", [False, True])
def test_material_stage_equals_the_oracle_on_the_exploded_scene(mcpt_mod, oracle, fixed):
    import stage_fixtures as sf

    s = sf.stage_scene(mcpt_mod, 2)
    a = s.arrays()
    tex = TR.random_set(a, sizes=((8, 8), (3, 5)), untextured=(1, 6), seed=4)
    kw = dict(max_depth=sf.DEPTH, rr_depth=sf.RR, fixed=fixed)
    inp = sf.material_state(a, oracle.trace_closest, 2)
    mats = np.asarray(a["mat"])[inp["hit_tri"]]
    assert set(np.asarray(tex["mat_tex"])[mats]) == {-1, 0, 1}  # both textures and an untextured material are hit
    ref = TR.stage_material(oracle, a, tex, inp, **kw)
    plain = oracle.stage_material(a, inp, **kw)
    assert (u32(ref["nee0"]) != u32(plain["nee0"])).any(axis=1).sum() > 100
    untouched = np.asarray(tex["mat_tex"])[mats] < 0
    assert np.array_equal(u32(ref["nee0"][untouched]), u32(plain["nee0"][untouched]))
    pt = mcpt_mod.PathTracer(0, mcpt_mod.default_config(spp=sf.SPP, max_depth=sf.DEPTH, rr_depth=sf.RR, fixed=fixed))
    pt.upload_scene(s)
    pt.set_camera(sf.stage_camera(mcpt_mod, 2))
    install(pt, tex)
    assert pt.texture_stats()["in_effect"]
    got = pt.stage("material", inp)
    _check_stage("material", got, ref, a, oracle)
    pt.set_textures()  # removed: the stage of a context without textures
    _check_stage("material", pt.stage("material", inp), plain, a, oracle)
    pt.close()


# ---------------------------------------------------------------------------------------------
# 3. the film
@pytest.mark.parametrize("gpu_bvh", [False, True])
@pytest.mark.parametrize("fixed", [False, True])
@pytest.mark.parametrize("which", ["c2", "cube"])
def test_film_equals_the_reference_loop(request, mcpt_mod, oracle, which, fixed, gpu_bvh):
    """Bitwise in Ld and samples at one path slot, with the reference loop's ray counts.  A device-built
    tree stores its records in Morton order: the uv stream has to follow the upload's order array."""
    sc = request.getfixturevalue(which)
    rLd, rsm, rc = ref_film(oracle, sc, which, fixed)
    pLd, _, _ = ref_film(oracle, sc, which, fixed, tex=False)
    got = one(mcpt_mod, sc["scene"], sc["cam"], sc["tex"], fixed=fixed, gpu_bvh=gpu_bvh)
    changed = (rLd != pLd).any(axis=2)
    print("pixels changed by the textures:", int(changed.sum()), "of", (W - 1) * (H - 1))
    assert changed.sum() > 100
    assert np.array_equal(got[1], rsm) and np.array_equal(u32(got[0]), u32(rLd))
    assert got[2] == tuple(rc[k] for k in RAYS)


@pytest.mark.parametrize("which", ["c2", "cube"])
def test_ray_counts_are_the_untextured_ones_below_the_roulette(request, mcpt_mod, oracle, which):
    """The draws do not depend on the textures, and neither does any path until the roulette tests a
    throughput the base colour has scaled: at max_depth 2 (rr_depth 3) the ray counts are those of the
    untextured render, and the film is still the reference loop's."""
    sc = request.getfixturevalue(which)
    rLd, rsm, rc = ref_film(oracle, sc, which, depth=2)
    got = one(mcpt_mod, sc["scene"], sc["cam"], sc["tex"], depth=2)
    plain = one(mcpt_mod, sc["scene"], sc["cam"], None, depth=2)
    assert np.array_equal(got[1], rsm) and np.array_equal(u32(got[0]), u32(rLd))
    assert got[2] == plain[2] == tuple(rc[k] for k in RAYS) and not same_film(got, plain)


@pytest.mark.parametrize("gpu_bvh", [False, True])
def test_three_path_slots(mcpt_mod, oracle, c2, gpu_bvh):
    """Slot k runs samples k, k + 3, ...: every sample contributes what it does at one slot, only the
    film's summation order differs (the project's tolerance for that), counts exact."""
    rLd, rsm, rc = ref_film(oracle, c2, "c2")
    got = one(mcpt_mod, c2["scene"], c2["cam"], c2["tex"], slots=3, gpu_bvh=gpu_bvh)
    ok, bad = film_close(got[0], rLd)
    assert ok, bad
    assert np.array_equal(got[1], rsm) and got[2] == tuple(rc[k] for k in RAYS)


@pytest.mark.parametrize("mode", ["refit", "rebuild"])
def test_geometry_updates_keep_the_set(mcpt_mod, c2, mode):
    """After an update the film equals a fresh upload of the moved mesh with the textures installed again:
    a rebuild re-sorts the records, so the uv stream is permuted again; a refit keeps the order."""
    gpu = mode == "rebuild"
    m = RF.refitted_desc_arrays(c2["a"], amp=0.02)
    p = ctx(mcpt_mod, c2["scene"], c2["cam"], c2["tex"], gpu_bvh=gpu)
    before = frame(p)
    p.update_geometry(m["v0"], m["v1"], m["v2"], mode=mode)
    t = p.textures()
    assert all(np.array_equal(t[k], c2["tex"][k]) for k in ("uv0", "uv1", "uv2", "mat_tex")) and p.texture_stats()["in_effect"]
    moved = frame(p)
    p.close()
    fresh = one(mcpt_mod, mcpt_mod.desc_from_arrays(m), c2["cam"], c2["tex"], gpu_bvh=gpu)
    assert same_film(moved, fresh) and moved[2] == fresh[2] and not same_film(moved, before)


# ---------------------------------------------------------------------------------------------
# 4. identity across every instantiation
MODES = {"plain": {}, "fixed": dict(fixed=True), "samp": dict(samp=True), "samp_fixed": dict(samp=True, fixed=True),
         "mis": dict(samp=True, mis=True), "mis_fixed": dict(samp=True, mis=True, fixed=True)}


@pytest.mark.parametrize("mode", list(MODES))
def test_constant_textures_are_channel_masks(mcpt_mod, c2, mode):
    """Every material wears a constant texture whose channels are 0 or 255: the film is, bit for bit, that
    of the same scene with those channels of mat_params zeroed, and an all-255 set reproduces the untextured
    context.  Exact: the weights are multiples of 2^-16 that sum to 1 and multiply 0 or 1.  One wall and one
    sphere emit under a black environment, so the emitter sample's and the MIS weight's BRDF terms matter."""
    a = ER.black(c2["a"])
    nmat = len(a["mat_params"])
    E = ER.table(nmat, {ER.MATS_LIT[0]: (3.0, 2.0, 1.0), ER.MATS_LIT[1]: (0.5, 2.0, 8.0)})
    kw = dict(E=E, **MODES[mode])
    masks = np.array([[(1 + m % 7) >> c & 1 for c in range(3)] for m in range(nmat)], np.uint8)  # 1..7, 7 = all on
    sizes = [(1, 1), (3, 5), (8, 8)]
    texs = [np.broadcast_to(np.append(masks[m] * 255, 77).astype(np.uint8), sizes[m % 3] + (4,)).copy() for m in range(nmat)]
    tex = dict(c2["tex"], textures=texs, mat_tex=np.arange(nmat, dtype=np.int32))
    zeroed = dict(a, mat_params=np.asarray(a["mat_params"], F).copy())
    zeroed["mat_params"][:, :3] *= masks
    d = mcpt_mod.desc_from_arrays(a)
    want = one(mcpt_mod, mcpt_mod.desc_from_arrays(zeroed), c2["cam"], None, **kw)
    plain = one(mcpt_mod, d, c2["cam"], None, **kw)
    p = ctx(mcpt_mod, d, c2["cam"], tex, **kw)
    assert p.texture_stats()["in_effect"] and p.emitter_stats()["active"] == bool(kw.get("samp")) and p.emitter_stats()["mis"] == bool(kw.get("mis"))
    got = frame(p)
    white = dict(tex, textures=[np.full((2, 3, 4), 255, np.uint8)], mat_tex=np.zeros(nmat, np.int32))
    install(p, white)
    ones = frame(p)
    p.close()
    assert (plain[0] != 0).any(axis=2).sum() > 100 and not same_film(want, plain)
    assert same_film(got, want) and got[2] == want[2]
    assert same_film(ones, plain) and ones[2] == plain[2]


# ---------------------------------------------------------------------------------------------
# 5. the guides
@pytest.mark.parametrize("gpu_bvh", [False, True])
def test_albedo_guide_is_the_shaded_base_colour(mcpt_mod, oracle, c2, gpu_bvh):
    """lens_radius = 0: every guide sample's ray is the pixel's pinhole ray, so the albedo guide is
    base_factor * lookup at the oracle's first hit of that ray (1 at a miss), bit for bit; normal, depth
    and count are those of the untextured guide pass."""
    a, tex = c2["a"], c2["tex"]
    cam = mcpt_mod.make_camera((0.0, 0.0, 3.5), aspect=F(W) / F(H), lens_radius=0.0)
    P = W * H
    dead = {"flags": np.ones(P, np.uint32), "hit_tri": np.full(P, -1, np.int32), "ray_d": np.zeros((P, 3), F),
            "beta": np.zeros((P, 4), F), "nee0": np.zeros((P, 4), F), "nee1": np.zeros((P, 4), F),
            "vis": np.zeros((P, 2), np.uint8), "Ld": np.zeros((P, 3), F), "samples": np.zeros(P, np.uint32)}
    out = oracle.stage_logic(a, cam, W, H, dead, spp=1)
    q = (out["queued"] & 1) != 0
    assert q.sum() == (W - 1) * (H - 1)
    _, _, tri = oracle.trace_closest(a, out["ray_o"][q], out["ray_d"][q])
    hit = tri >= 0
    want = np.zeros((P, 3), F)
    wq = np.ones((int(q.sum()), 3), F)
    ix = np.argsort(a["tri_id"])[tri[hit]]
    wq[hit] = TR.base_colour(a, tex, ix, out["ray_o"][q][hit], out["ray_d"][q][hit])
    want[q] = wq
    p = ctx(mcpt_mod, c2["scene"], cam, None, gpu_bvh=gpu_bvh)
    p.render_guides(3)  # a pinhole's samples share one ray: one guide sample is accumulated
    g0 = p.guides()
    install(p, tex)
    with pytest.raises(mcpt_mod.McptError):  # the installed set made the guides stale
        p.guides()
    p.render_guides(3)
    g1 = p.guides()
    p.set_textures()
    with pytest.raises(mcpt_mod.McptError):
        p.guides()
    p.render_guides(3)
    g2 = p.guides()
    p.close()
    assert hit.sum() > P // 2 and g1["count"].max() == 1
    assert np.array_equal(u32(g1["albedo"].reshape(-1, 3)), u32(want))
    assert (u32(g1["albedo"]) != u32(g0["albedo"])).any(axis=2).sum() > 100
    for k in ("normal", "depth", "count"):
        assert np.array_equal(g1[k].view(np.uint32), g0[k].view(np.uint32)), k
    for k in g0:
        assert np.array_equal(g2[k].view(np.uint32), g0[k].view(np.uint32)), k


# ---------------------------------------------------------------------------------------------
# 6. state
def test_install_identical_removal_and_upload(mcpt_mod, c2):
    tex = c2["tex"]
    never = one(mcpt_mod, c2["scene"], c2["cam"], None)
    p = ctx(mcpt_mod, c2["scene"], c2["cam"], None)
    p.set_variance_fill()
    assert p.textures() is None and p.texture_stats() == {"bytes": 0, "textured_materials": 0, "in_effect": False}
    first = frame(p)
    assert same_film(first, never) and first[1].max() == SPP
    p.render_guides(1)
    p.temporal_accumulate()
    p.temporal()
    install(p, tex)  # an install: the film stale, the guides stale, the history dropped
    with pytest.raises(mcpt_mod.McptError):
        p.temporal()
    with pytest.raises(mcpt_mod.McptError):
        p.guides()
    st = p.iterate(1)
    assert st.extend_rays > 0 and p.film()[1].max() < SPP
    textured = frame(p)
    assert not same_film(textured, never)
    s = p.texture_stats()
    ntri, ntex_px = len(c2["a"]["mat"]), sum(t.shape[0] * t.shape[1] for t in tex["textures"])
    assert s["in_effect"] and s["textured_materials"] == int((tex["mat_tex"] >= 0).sum())
    assert s["bytes"] >= 24 * ntri + 4 * ntex_px + 16 * len(tex["mat_tex"])
    t = p.textures()
    assert all(np.array_equal(t[k], tex[k]) for k in ("uv0", "uv1", "uv2", "mat_tex"))
    assert len(t["textures"]) == 2 and all(np.array_equal(x, y) for x, y in zip(t["textures"], tex["textures"]))
    p.render_guides(1)
    p.temporal_accumulate()
    install(p, {k: (v.copy() if isinstance(v, np.ndarray) else [x.copy() for x in v]) for k, v in tex.items()})
    st = p.iterate(1)  # an identical set: nothing happens
    assert rays(st) == (0, 0, 0) and same_film((*p.film(),), textured)
    p.guides(), p.temporal()
    none = dict(tex, mat_tex=np.full_like(tex["mat_tex"], -1))  # every index -1: installed, not in effect
    install(p, none)
    assert p.textures() is not None and not p.texture_stats()["in_effect"]
    assert same_film(frame(p), never)
    install(p, tex)
    assert same_film(frame(p), textured)
    p.set_textures()  # a removal: back to the old kernels
    assert p.textures() is None and p.texture_stats() == {"bytes": 0, "textured_materials": 0, "in_effect": False}
    removed = frame(p)
    assert same_film(removed, never) and removed[2] == never[2]
    install(p, tex)
    p.upload_scene(c2["scene"])  # an upload drops the set
    assert p.textures() is None and not p.texture_stats()["in_effect"]
    assert same_film(frame(p), never)
    p.close()


def test_scene_textures_are_installed_by_the_upload(mcpt_mod, oracle, cube):
    """Scene.set_texture + upload_scene: the glb's own uvs and the attached image reach the context."""
    import os

    from conftest import ASSETS

    s = mcpt_mod.Scene()
    s.load_glb(os.path.join(ASSETS, "Cube.glb"))
    s.set_env_hdr(os.path.join(ASSETS, "HDR_029_Sky_Cloudy_Env.hdr"), 1)
    s.set_texture(0, cube["tex"]["textures"][0])
    s.build(8)
    p = ctx(mcpt_mod, s, cube["cam"], None)
    t = p.textures()
    assert t is not None and np.array_equal(t["uv1"], cube["a"]["uv1"]) and np.array_equal(t["textures"][0], cube["tex"]["textures"][0])
    got = frame(p)
    p.close()
    rLd, rsm, _ = ref_film(oracle, cube, "cube")
    assert np.array_equal(u32(got[0]), u32(rLd)) and np.array_equal(got[1], rsm)


def test_rejected_sets_leave_the_installed_one(mcpt_mod, c2):
    lib, tex, a = mcpt_mod.lib(), c2["tex"], c2["a"]
    ntri, nmat = len(a["mat"]), len(a["mat_params"])
    f = lambda x: np.ascontiguousarray(x, F).ctypes.data_as(C.POINTER(C.c_float))
    u = [np.ascontiguousarray(tex[k], F) for k in ("uv0", "uv1", "uv2")]
    imgs = [np.ascontiguousarray(t) for t in tex["textures"]]

    def call(p, ntri_=ntri, nmat_=nmat, mt=tex["mat_tex"], sizes=None, null_px=False, uvs=None, ntex=None):
        arr = (mcpt_mod.Texture * len(imgs))()
        for k, im in enumerate(imgs):
            arr[k].w, arr[k].h = sizes[k] if sizes else (im.shape[1], im.shape[0])
            arr[k].rgba8 = None if null_px and k == 1 else im.ctypes.data_as(C.POINTER(C.c_uint8))
        m = np.ascontiguousarray(mt, np.int32)
        uu = uvs if uvs is not None else [f(x) for x in u]
        return lib.mcpt_set_material_textures(p.h, ntri_, uu[0], uu[1], uu[2], len(imgs) if ntex is None else ntex, arr, nmat_,
                                              m.ctypes.data_as(C.POINTER(C.c_int32)))

    p = mcpt_mod.PathTracer(0, mcpt_mod.default_config(spp=SPP))
    assert call(p) == -1 and b"no scene" in lib.mcpt_last_error(p.h)
    p.close()
    p = ctx(mcpt_mod, c2["scene"], c2["cam"], tex)
    first = frame(p)
    hi, lo = tex["mat_tex"].copy(), tex["mat_tex"].copy()
    hi[3], lo[0] = 2, -2
    cases = [dict(ntri_=ntri - 1), dict(ntri_=ntri + 1), dict(nmat_=nmat - 1), dict(nmat_=nmat + 1), dict(mt=hi), dict(mt=lo),
             dict(sizes=[(0, 8), (5, 3)]), dict(sizes=[(8, 8), (5, 0)]), dict(sizes=[(16385, 1), (5, 3)]),
             dict(sizes=[(8, 8), (1, 16385)]), dict(sizes=[(-8, 8), (5, 3)]), dict(null_px=True),
             dict(uvs=[f(u[0]), None, f(u[2])])]
    for kw in cases:
        assert call(p, **kw) == -1, kw
        t = p.textures()
        assert all(np.array_equal(t[k], tex[k]) for k in ("uv0", "uv1", "uv2", "mat_tex")), kw
        assert all(np.array_equal(x, y) for x, y in zip(t["textures"], imgs)), kw
    # 2^31 texels or more in total: eight 16384 x 16384 textures (the sizes are checked before a texel is read)
    arr = (mcpt_mod.Texture * 8)()
    for k in range(8):
        arr[k].w = arr[k].h = 16384
        arr[k].rgba8 = imgs[0].ctypes.data_as(C.POINTER(C.c_uint8))
    m = np.zeros(nmat, np.int32)
    assert lib.mcpt_set_material_textures(p.h, ntri, f(u[0]), f(u[1]), f(u[2]), 8, arr, nmat, m.ctypes.data_as(C.POINTER(C.c_int32))) == -1
    assert b"2^31" in lib.mcpt_last_error(p.h)
    assert p.texture_stats()["in_effect"]
    assert rays(p.iterate(1)) == (0, 0, 0) and same_film((*p.film(),), first)  # and the film is not stale
    n = C.c_int32(0)
    assert lib.mcpt_material_textures_read(p.h, None, C.byref(n), None, None, 2, None, None, None, None, None, None) == -1
    p.close()
