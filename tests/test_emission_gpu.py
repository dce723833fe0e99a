"""Emissive materials on the device: k_shade's emission instantiations against
the reference loop of tests/emission_ref.py (the oracle's stages plus one numpy line), bit for bit, and
the properties the term has to keep: paths and ray counts untouched, the skip switch, the primary-hit
table, the compact layout, linearity, the table's life cycle on a live context.

24 x 16 film, 4 spp, config 2's proxy (4810 triangles, 10 materials) unless stated."""
import ctypes as C

import numpy as np
import pytest

import emission_ref as ER
import refit_ref as RF
from stage_checks import _check_stage
from test_gpu import film_close

pytestmark = pytest.mark.gpu
W, H, SPP = 24, 16, 4
RAYS = ("extend_rays", "shadow_rays", "vis_rays")


def u32(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def same_film(f, g):
    return np.array_equal(u32(f[0]), u32(g[0])) and np.array_equal(f[1], g[1])


def rays(st):
    return tuple(int(getattr(st, k)) for k in RAYS)


@pytest.fixture(scope="module")
def c2(mcpt_mod, scene_c2):
    s, a = scene_c2
    E = ER.table(len(a["mat_params"]), {ER.MATS_LIT[0]: (3.0, 2.0, 1.0), ER.MATS_LIT[1]: (0.5, 2.0, 8.0)})
    return dict(scene=s, a=a, cam=mcpt_mod.config_camera(mcpt_mod.CONFIGS[2], W, H), E=E)


def ctx(mcpt, scene, cam, E=None, fixed=False, depth=5, tile=256, gpu_bvh=False, compact=False, slots=1, tiles=None):
    p = mcpt.PathTracer(0, mcpt.default_config(spp=SPP, max_depth=depth, tile=tile, fixed=fixed))
    p.upload_scene(scene, gpu_bvh=gpu_bvh)
    if E is not None:
        p.set_emission(E)
    p.set_camera(cam)
    p.resize(W, H, tile, tile)
    if compact:
        p.set_compact_paths(True)
    if slots != 1:
        p.set_path_slots(slots)
    if tiles is not None:
        p.set_tiles(tiles)
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


# ---------------------------------------------------------------------------------------------
# 1. the film against the reference loop
@pytest.mark.parametrize("gpu_bvh", [False, True])
@pytest.mark.parametrize("depth", [5, 2])
@pytest.mark.parametrize("fixed", [False, True])
def test_film_equals_the_reference_loop(mcpt_mod, oracle, c2, fixed, depth, gpu_bvh):
    """One wall and one sphere emissive under the config's own environment, so emission adds to films
    that hold MIS terms too.  Bitwise in Ld and samples at one path slot; the ray counts are those of
    a render without emission (and the reference loop's).  With a device-built tree the records lie
    in Morton order: the material id has to come from the hit's record."""
    rLd, rsm, rc = ER.render(oracle, c2["a"], c2["cam"], W, H, SPP, max_depth=depth, fixed=fixed, emission=c2["E"])
    pLd, _, _ = ER.render(oracle, c2["a"], c2["cam"], W, H, SPP, max_depth=depth, fixed=fixed)
    got = one(mcpt_mod, c2["scene"], c2["cam"], c2["E"], fixed=fixed, depth=depth, gpu_bvh=gpu_bvh)
    plain = one(mcpt_mod, c2["scene"], c2["cam"], None, fixed=fixed, depth=depth, gpu_bvh=gpu_bvh)
    changed = (rLd != pLd).any(axis=2)
    print("pixels changed by emission:", int(changed.sum()), "of", (W - 1) * (H - 1))
    assert changed.sum() > 100
    assert np.array_equal(got[1], rsm) and np.array_equal(u32(got[0]), u32(rLd))
    assert np.array_equal(u32(plain[0]), u32(pLd))
    assert got[2] == plain[2] == tuple(rc[k] for k in RAYS)


# ---------------------------------------------------------------------------------------------
# 2. stage parity
@pytest.mark.parametrize("fixed", [False, True])
@pytest.mark.parametrize("cid", [1, 2])
def test_logic_stage_applies_the_table(mcpt_mod, oracle, cid, fixed):
    """mcpt_stage_run(LOGIC) over stage_fixtures' states (every logic case: dead paths, primary hits and
    misses, MIS terms, zero samples, roulette depths, the depth cap) equals or_stage_logic plus the numpy
    line in every output field; GENERATE and MATERIAL do not look at the table."""
    import stage_fixtures as sf

    s = sf.stage_scene(mcpt_mod, cid)
    a = s.arrays()
    cam = sf.stage_camera(mcpt_mod, cid)
    nmat = len(a["mat_params"])
    E = ER.table(nmat, {m: (0.5 + m, 2.0, 8.0 / (1 + m)) for m in range(0, nmat, 2)})
    kw = dict(max_depth=sf.DEPTH, rr_depth=sf.RR, fixed=fixed)
    inp = sf.logic_state(len(a["mat"]))
    ref = oracle.stage_logic(a, cam, sf.FILM[0], sf.FILM[1], inp, sf.SPP, **kw)
    plain_Ld = ref["Ld"].copy()
    cont = (ref["queued"] & 2) != 0
    ER.emission_line(ref["Ld"], cont, inp["hit_tri"], ref["beta"], a["mat"], E)
    lit = (ref["Ld"] != plain_Ld).any(axis=1)
    assert lit.sum() > 20 and not lit[~cont].any()
    pt = mcpt_mod.PathTracer(0, mcpt_mod.default_config(spp=sf.SPP, max_depth=sf.DEPTH, rr_depth=sf.RR, fixed=fixed))
    pt.upload_scene(s)
    pt.set_camera(cam)
    pt.set_emission(E)
    got = pt.stage("logic", inp, film=sf.FILM)
    _check_stage("logic", got, ref, a, oracle)
    # the other two stages: the outputs of a context without a table
    dead = sf.logic_state(len(a["mat"]), True)
    mat_in = sf.material_state(a, oracle.trace_closest, cid)
    with_gen, with_mat = pt.stage("generate", dead, film=sf.FILM), pt.stage("material", mat_in)
    pt.set_emission(None)
    for got_s, ref_s in ((with_gen, pt.stage("generate", dead, film=sf.FILM)), (with_mat, pt.stage("material", mat_in))):
        for k in ref_s:
            assert np.array_equal(got_s[k].view(np.uint8), ref_s[k].view(np.uint8)), k
    # an out-of-range triangle is an error, not a read past the records
    bad = dict(inp)
    bad["hit_tri"] = inp["hit_tri"].copy()
    bad["hit_tri"][np.flatnonzero(cont)[0]] = len(a["mat"])
    pt.set_emission(E)
    with pytest.raises(mcpt_mod.McptError):
        pt.stage("logic", bad, film=sf.FILM)
    pt.close()


# ---------------------------------------------------------------------------------------------
# 3. closed form
@pytest.mark.parametrize("fixed,depth", [(False, 5), (False, 1), (True, 1)])
def test_emissive_quad_closed_form(mcpt_mod, oracle, fixed, depth):
    """One emissive quad larger than the view under a black environment: every sample's primary hit
    collects Le with beta = (1, 1, 1), so a rendered pixel is exactly spp * Le (powers of two: the sum
    is exact).  At max_depth 1 nothing else can reach the film in either mode.  At depth 5 that holds in
    reference mode, where the reference's NaN frame at the quad's axis-aligned normal ends every path at
    its second vertex; fixed mode's orthonormal frame lets a few continuation rays graze the quad again
    (the reference loop shows the same), so it is pinned at depth 1 only."""
    F = np.float32
    q = np.array([[-10, -10, 0], [10, -10, 0], [10, 10, 0], [-10, 10, 0]], F)
    n = np.tile(F([0, 0, 1]), (2, 1))
    s = mcpt_mod.Scene()
    s.add_mesh(q[[0, 0]], q[[1, 2]], q[[2, 3]], n, n, n, (0.8, 0.8, 0.8))
    s.set_env_color((0.0, 0.0, 0.0))
    Le = F([0.5, 2.0, 8.0])
    s.set_emission(0, Le)
    s.build(8)
    cam = mcpt_mod.make_camera((0.0, 0.0, 4.0), aspect=F(W) / F(H))
    p = ctx(mcpt_mod, s, cam, None, fixed=fixed, depth=depth)  # upload_scene installs the scene's table
    assert np.array_equal(p.emission(), Le.reshape(1, 3))
    Ld, sm, _ = frame(p)
    p.close()
    assert (sm[:-1, :-1] == SPP).all() and not sm[-1].any() and not sm[:, -1].any()
    assert np.array_equal(Ld[:-1, :-1], np.broadcast_to(F(SPP) * Le, (H - 1, W - 1, 3)))
    assert not Ld[-1].any() and not Ld[:, -1].any()  # the never-rendered last row and column
    rLd, rsm, _ = ER.render(oracle, s.arrays(), cam, W, H, SPP, max_depth=depth, fixed=fixed, emission=Le.reshape(1, 3))
    assert np.array_equal(u32(Ld), u32(rLd)) and np.array_equal(sm, rsm)


# ---------------------------------------------------------------------------------------------
# 4. invariances
@pytest.mark.parametrize("fixed", [False, True])
def test_invariances(mcpt_mod, c2, fixed, monkeypatch):
    """The film with emission does not depend on how the iteration is run: the skip switch (a path ended
    at len == max_depth still collects there; one the roulette ends collects nothing), the primary-hit
    table, the compact layout over a tile subset, a uniform sample budget map (the map instantiation of
    k_shade) -- bitwise, with the ray counts -- and three path slots
    within the project's tolerance for a changed summation order."""
    T = 8  # 3 x 2 tiles, so a tile subset exists
    args = (c2["scene"], c2["cam"], c2["E"])
    base = one(mcpt_mod, *args, fixed=fixed, tile=T)
    assert same_film(base, one(mcpt_mod, *args, fixed=fixed))  # (and not on the tile size)
    p = ctx(mcpt_mod, *args, fixed=fixed, tile=T)
    p.set_skip_discarded(False)
    noskip = frame(p)
    assert p.discard_stats()["extension_untraced"] == 0
    p.set_skip_discarded(True)
    p.clear()
    skip = frame(p)
    assert p.discard_stats()["extension_untraced"] > 0
    p.close()
    assert same_film(noskip, base) and same_film(skip, base) and noskip[2] == skip[2] == base[2]
    monkeypatch.setenv("MCPT_PRIMARY_HITS", "0")
    p = ctx(mcpt_mod, *args, fixed=fixed, tile=T)
    notab = frame(p)
    assert p.primary_stats()["resolved"] == 0
    p.close()
    monkeypatch.delenv("MCPT_PRIMARY_HITS")
    assert same_film(notab, base) and notab[2] == base[2]
    mine = [(2, 1), (0, 0), (1, 1)]
    own = np.zeros((H, W), bool)
    for tx, ty in mine:
        own[ty * T:(ty + 1) * T, tx * T:(tx + 1) * T] = True
    part = one(mcpt_mod, *args, fixed=fixed, tile=T, compact=True, tiles=mine)
    assert np.array_equal(u32(part[0][own]), u32(base[0][own])) and np.array_equal(part[1][own], base[1][own])
    assert not part[0][~own].any() and not part[1][~own].any()
    # a uniform sample budget map: k_shade's map instantiation with emission
    p = ctx(mcpt_mod, *args, fixed=fixed, tile=T)
    p.set_sample_budget(np.full((H, W), SPP, np.uint32))
    mapped = frame(p)
    p.close()
    assert same_film(mapped, base) and mapped[2] == base[2]
    s3 = one(mcpt_mod, *args, fixed=fixed, tile=T, slots=3)
    ok, bad = film_close(s3[0], base[0])
    assert ok, bad
    assert np.array_equal(s3[1], base[1]) and s3[2] == base[2]


@pytest.mark.parametrize("fixed", [False, True])
def test_film_is_linear_in_the_table_on_the_device(mcpt_mod, oracle, c2, fixed):
    d = mcpt_mod.desc_from_arrays(ER.black(c2["a"]))
    f1 = one(mcpt_mod, d, c2["cam"], c2["E"], fixed=fixed)
    f4 = one(mcpt_mod, d, c2["cam"], np.float32(4.0) * c2["E"], fixed=fixed)
    assert (f1[0] != 0).any(axis=2).sum() > 100
    assert np.array_equal(u32(np.float32(4.0) * f1[0]), u32(f4[0])) and np.array_equal(f1[1], f4[1]) and f1[2] == f4[2]
    rLd, _, _ = ER.render(oracle, ER.black(c2["a"]), c2["cam"], W, H, SPP, fixed=fixed, emission=c2["E"])
    assert np.array_equal(u32(f1[0]), u32(rLd))


# ---------------------------------------------------------------------------------------------
# 5. none and zero
def test_zero_and_removed_tables_render_as_no_table(mcpt_mod, c2):
    never = one(mcpt_mod, c2["scene"], c2["cam"], None)
    p = ctx(mcpt_mod, c2["scene"], c2["cam"], np.zeros_like(c2["E"]))
    e = p.emission()
    assert e is not None and e.shape == c2["E"].shape and not e.any()  # stored ...
    n = C.c_int32(-1)
    assert mcpt_mod.lib().mcpt_material_emission_read(p.h, None, C.byref(n)) == 0 and n.value == len(e)  # ... none lit
    zero = frame(p)
    p.set_emission(c2["E"])
    assert mcpt_mod.lib().mcpt_material_emission_read(p.h, None, C.byref(n)) == 2
    lit = frame(p)
    p.set_emission(None)
    assert p.emission() is None
    assert mcpt_mod.lib().mcpt_material_emission_read(p.h, None, C.byref(n)) == 0 and n.value == 0
    removed = frame(p)
    p.close()
    assert same_film(zero, never) and same_film(removed, never) and zero[2] == removed[2] == never[2] == lit[2]
    assert not same_film(lit, never)


# ---------------------------------------------------------------------------------------------
# 6. life cycle
def test_a_set_marks_the_film_stale(mcpt_mod, c2):
    E = c2["E"]
    p = ctx(mcpt_mod, c2["scene"], c2["cam"], E)
    first = frame(p)
    assert first[1].max() == SPP
    p.set_emission(E.copy())  # identical values: nothing happens, the finished film stays
    st = p.iterate(1)
    assert rays(st) == (0, 0, 0) and same_film((*p.film(),), first)
    p.set_emission(np.float32(2.0) * E)  # other values: the next iteration starts from a cleared film
    st = p.iterate(1)
    assert st.extend_rays > 0 and p.film()[1].max() < SPP
    doubled = frame(p)
    assert doubled[1].max() == SPP and same_film(doubled, one(mcpt_mod, c2["scene"], c2["cam"], np.float32(2.0) * E))
    p.close()
    # MCPT_FLAG_NO_AUTO_CLEAR: the caller clears
    q = mcpt_mod.PathTracer(0, mcpt_mod.default_config(spp=SPP, auto_clear=False))
    q.upload_scene(c2["scene"])
    q.set_camera(c2["cam"])
    q.resize(W, H)
    q.set_emission(E)
    assert same_film(frame(q), first)
    q.set_emission(np.float32(2.0) * E)
    assert rays(q.iterate(1)) == (0, 0, 0) and same_film((*q.film(),), first)
    q.clear()
    assert same_film(frame(q), doubled)
    q.close()


@pytest.mark.parametrize("mode", ["refit", "rebuild"])
def test_geometry_updates_keep_the_table_and_uploads_drop_it(mcpt_mod, c2, mode):
    gpu = mode == "rebuild"
    m = RF.refitted_desc_arrays(c2["a"], amp=0.02)
    p = ctx(mcpt_mod, c2["scene"], c2["cam"], c2["E"], gpu_bvh=gpu)
    before = frame(p)
    p.update_geometry(m["v0"], m["v1"], m["v2"], mode=mode)
    assert np.array_equal(p.emission(), c2["E"])
    moved = frame(p)
    fresh = one(mcpt_mod, mcpt_mod.desc_from_arrays(m), c2["cam"], c2["E"], gpu_bvh=gpu)
    assert same_film(moved, fresh) and moved[2] == fresh[2] and not same_film(moved, before)
    p.upload_scene(c2["scene"], gpu_bvh=gpu)  # an upload drops the table
    assert p.emission() is None
    assert same_film(frame(p), one(mcpt_mod, c2["scene"], c2["cam"], None, gpu_bvh=gpu))
    p.close()


def test_rejected_tables_leave_the_installed_one(mcpt_mod, c2):
    lib, E = mcpt_mod.lib(), c2["E"]
    f = lambda a: np.ascontiguousarray(a, np.float32).ctypes.data_as(C.POINTER(C.c_float))
    p = mcpt_mod.PathTracer(0, mcpt_mod.default_config(spp=SPP))
    assert lib.mcpt_set_material_emission(p.h, len(E), f(E)) == -1 and b"no scene" in lib.mcpt_last_error(p.h)
    p.close()
    p = ctx(mcpt_mod, c2["scene"], c2["cam"], E)
    first = frame(p)
    neg, nan, inf = E.copy(), E.copy(), E.copy()
    neg[4, 1], nan[0, 0], inf[9, 2] = -1.0, np.nan, np.inf
    for nmat, tab in ((len(E) - 1, E[:-1]), (len(E) + 1, np.vstack([E, E[:1]])), (len(E), neg), (len(E), nan), (len(E), inf)):
        keep = np.ascontiguousarray(tab, np.float32)
        assert lib.mcpt_set_material_emission(p.h, nmat, f(keep)) == -1
        assert np.array_equal(p.emission(), E)
    assert rays(p.iterate(1)) == (0, 0, 0) and same_film((*p.film(),), first)  # and the film is not stale
    p.close()


def test_post_processing_runs_on_an_emissive_frame(mcpt_mod, c2):
    """A guided denoise and a temporal accumulate over a frame lit by emission; a changed table keeps
    the guides (albedo, normal and depth do not depend on emission) and drops the temporal history."""
    p = ctx(mcpt_mod, mcpt_mod.desc_from_arrays(ER.black(c2["a"])), c2["cam"], c2["E"])
    p.set_variance_fill()
    Ld, sm, _ = frame(p)
    p.render_guides(2)
    g0 = p.guides()
    p.denoise_guided()
    dn = p.denoised()
    assert np.isfinite(dn).all() and (dn[:-1, :-1] > 0).any()
    p.temporal_accumulate()
    t = p.temporal()
    assert np.isfinite(t["rgb"]).all() and np.array_equal(t["nsamples"], sm.astype(np.float32))
    p.set_emission(np.float32(4.0) * c2["E"])
    with pytest.raises(mcpt_mod.McptError):  # the history's colours belong to the old lighting
        p.temporal()
    g1 = p.guides()
    for k in g0:
        assert np.array_equal(g0[k].view(np.uint32), g1[k].view(np.uint32)), k
    Ld4, _, _ = frame(p)
    assert np.array_equal(u32(Ld4), u32(np.float32(4.0) * Ld))
    p.denoise_guided()  # with the guides rendered before the change
    p.temporal_accumulate()
    assert np.array_equal(p.temporal()["nsamples"], sm.astype(np.float32))  # nothing accumulated onto
    p.close()
