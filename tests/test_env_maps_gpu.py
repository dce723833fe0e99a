"""HRDI environment lights beyond the two 512x256 asset maps, on the device against the oracle (DESIGN.md
section 5): the map family of tests/env_maps.py through the table build, the guide flags, the material stage
(guided and plain CDF search, the light-sample tables with column -1, the pdf in the texture's alpha), the
logic stage at crafted escaping directions (the bilinear fetch's wrap in both axes and its non-finite rule)
and small films, in reference and fixed mode, with the tables built on the device and given.  The oracle
restates the light with plain upper_bound, a spherical direction per sample and env_L / env_pdf per
direction: no guides, no tabulated cells, no packed pdf.  Comparisons are bit for bit (NaNs as
stage_checks._same compares them) unless a test says otherwise.  What each map reaches is asserted from the
oracle's tables in tests/test_env_maps_host.py."""
import numpy as np
import pytest

import emission_ref as ER
import emitter_ref as MR
import env_maps as EM
import stage_fixtures as sf
from stage_checks import _check_stage, _same

pytestmark = pytest.mark.gpu
MODES = pytest.mark.parametrize("fixed", [False, True], ids=["reference", "fixed"])
TABLE_KEYS = ("marginal_y", "conds_y", "pdf")
STAGE_OUT = ("flags", "ray_o", "ray_d", "beta", "nee0", "nee1", "queued", "hit_tri", "vis", "light_o", "light_d",
             "bvis_o", "bvis_d")
FW, FH, FSPP, FDEPTH = 48, 32, 4, 3
FILM_MAPS = ("odd", "bands", "sun_last", "negative", "tiny_3x3")
LOGIC_MAPS = ("odd", "tiny_4x2", "tiny_3x3", "tiny_2x2", "sun_first", "sun_last", "bands")


@pytest.fixture(scope="module")
def stage(mcpt_mod, oracle):
    """Config 1's stage scene (its directional light stays: half the light choices are the env light) and the
    1024 material-stage paths every map is run on."""
    a = sf.stage_scene(mcpt_mod, 1).arrays()
    return {"a": a, "mat": sf.material_state(a, oracle.trace_closest, n=1024), "cam": sf.stage_camera(mcpt_mod, 1)}


def stage_ctx(mcpt, arrays, fixed):
    pt = mcpt.PathTracer(0, mcpt.default_config(spp=sf.SPP, max_depth=sf.DEPTH, rr_depth=sf.RR, fixed=fixed))
    pt.upload_scene(mcpt.desc_from_arrays(arrays))
    return pt


def same_tables(got, ref):
    return all(_same(got[k], ref[k]) for k in TABLE_KEYS)


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("given", [False, True], ids=["device_tables", "given_tables"])
@pytest.mark.parametrize("name", EM.REJECTED)
def test_upload_rejects_maps_one_texel_wide_or_high(mcpt_mod, stage, name, given):
    """A map with W < 2 or H < 2 ((W - 1) == 0 in env_pdf's cell; sin(pi v) == 0 in every term of a one-row
    table) is refused by validate_desc with MCPT_E_INVALID, whichever way its tables would come."""
    pt = mcpt_mod.PathTracer(0)
    with pytest.raises(mcpt_mod.McptError, match=EM.REJECT_MATCH):
        pt.upload_scene(mcpt_mod.desc_from_arrays(EM.scene_arrays(stage["a"], name, given)))
    pt.close()


@pytest.mark.parametrize("name", EM.ACCEPTED)
def test_tables_and_guide_flags(mcpt_mod, oracle, stage, name):
    """PathTracer.env_tables after a device build equals oracle.env_build, tables uploaded as given read back
    unchanged, and the search guides are on exactly where env_maps.guides_expected says."""
    W, H = EM.SIZES[name]
    ref = EM.tables(name)
    for given in (False, True):
        pt = mcpt_mod.PathTracer(0)
        pt.upload_scene(mcpt_mod.desc_from_arrays(EM.scene_arrays(stage["a"], name, given)))
        got = pt.env_tables(W, H)
        pt.close()
        assert got["device_built"] == (not given)
        assert same_tables(got, ref), f"given={given}"
        assert got["guides"] == (name not in EM.GUIDES_OFF) == EM.guides_expected(name), f"given={given}"


@MODES
@pytest.mark.parametrize("name", EM.ACCEPTED)
def test_material_stage(mcpt_mod, oracle, stage, name, fixed):
    """mcpt_stage_run(MATERIAL) over 1024 paths under each map: env_cell's guided or plain search, the
    light-sample tables (column -1 and fixed mode's clamps included), the BRDF sample's env_L_pdf with the
    pdf read from the texture's alpha, and the in-place resolution of light rays, against
    oracle.stage_material."""
    ao = EM.scene_arrays(stage["a"], name, True)
    ref = oracle.stage_material(ao, stage["mat"], max_depth=sf.DEPTH, rr_depth=sf.RR, fixed=fixed)
    ids = EM.material_env_draws(oracle, stage["mat"]["flags"])[2]
    assert len(ids) > 400
    for given in (False, True):
        pt = stage_ctx(mcpt_mod, EM.scene_arrays(stage["a"], name, given), fixed)
        got = pt.stage("material", stage["mat"])
        pt.close()
        _check_stage("material", got, ref, ao, oracle)


@MODES
@pytest.mark.parametrize("name", ["odd", "bands", "wide", "tall"])
def test_forced_plain_bisection(mcpt_mod, oracle, stage, monkeypatch, name, fixed):
    """MCPT_ENV_GUIDES=0 at upload: guides off on maps that would have them, and env_cell's plain-bisection
    branch gives the guided run's material-stage outputs and the oracle's."""
    ao = EM.scene_arrays(stage["a"], name, True)
    ref = oracle.stage_material(ao, stage["mat"], max_depth=sf.DEPTH, rr_depth=sf.RR, fixed=fixed)
    W, H = EM.SIZES[name]
    runs = []
    for knob in ("0", None):
        if knob is None:
            monkeypatch.delenv("MCPT_ENV_GUIDES", raising=False)
        else:
            monkeypatch.setenv("MCPT_ENV_GUIDES", knob)
        pt = stage_ctx(mcpt_mod, EM.scene_arrays(stage["a"], name, False), fixed)
        assert pt.env_tables(W, H)["guides"] == (knob is None)
        runs.append(pt.stage("material", stage["mat"]))
        pt.close()
    _check_stage("material", runs[0], ref, ao, oracle)
    for k in STAGE_OUT:
        assert _same(runs[0][k], runs[1][k]), k


def test_forced_plain_bisection_same_film(mcpt_mod, scene_c2, monkeypatch):
    """Config 2's film (160x90, 4 spp) with MCPT_ENV_GUIDES=0 equals the default film bit for bit."""
    from test_gpu import make_pt

    s, a = scene_c2
    rc = mcpt_mod.CONFIGS[2]
    W, H = 160, 90
    cam = mcpt_mod.config_camera(rc, W, H)
    films = []
    for knob in (None, "0"):
        if knob is not None:
            monkeypatch.setenv("MCPT_ENV_GUIDES", knob)
        pt = make_pt(mcpt_mod, s, cam, W, H, 4, rc.max_depth)
        assert pt.env_tables(a["env_tex"].shape[1], a["env_tex"].shape[0])["guides"] == (knob is None)
        pt.render()
        films.append(pt.film())
        pt.close()
    (L0, s0), (L1, s1) = films
    assert np.array_equal(s0, s1) and np.array_equal(L0.view(np.uint32), L1.view(np.uint32))


# ---------------------------------------------------------------------------------------------
def crafted_directions():
    """Escaping directions at the edges of spherical_map and tex_bilinear."""
    f = np.float32
    den, tiny = np.nextafter(f(0), f(1)), np.finfo(np.float32).tiny
    up = np.nextafter(f(1), f(2))
    nan, inf = f(np.nan), f(np.inf)
    d = [(-1, 0, 0.0), (-1, 0, -0.0),                       # the seam: u = 1 and u = 0
         (-1, 0, den), (-1, 0, -den), (-1, 0, tiny), (-1, 0, -tiny),  # its neighbours one ulp (and one normal) in z
         (0, 1, 0), (0, -1, 0),                             # the poles: v = 0 and v = 1
         (1, 0, 0), (0, 0, 1), (0, 0, -1),                  # the other axes
         (0, up, 0), (0, -up, 0),                           # asin beyond its domain
         (nan, 0.6, 0.8), (0.6, nan, 0.8), (0.6, 0.8, nan),
         (inf, 0, 0), (0, -inf, 0), (0, 0, inf),
         (0, 0, 0)]
    return np.array(d, np.float32)


@MODES
@pytest.mark.parametrize("name", LOGIC_MAPS)
def test_logic_stage_crafted_escaping_directions(mcpt_mod, oracle, stage, name, fixed):
    """mcpt_stage_run(LOGIC): the live paths that missed the scene get their direction from
    crafted_directions(), cycled over them; only those at length 1 collect the background, so the list is
    rotated over as many runs as it takes for every direction to reach one.  env_L through tex_bilinear's
    wrap in both axes (wrapi's i % n fallback on the maps 2-4 texels wide) and its non-finite rule, against
    oracle.stage_logic."""
    a = stage["a"]
    ao = EM.scene_arrays(a, name, True)
    W, H = sf.FILM
    base = sf.logic_state(len(a["mat"]))
    dirs = crafted_directions()
    i = np.arange(W * H)
    live = ((base["flags"] & 1) == 0) & (base["hit_tri"] == -1) & (i % W < W - 1) & (i // W < H - 1)
    first = live & (((base["flags"] >> 1) & 0xFF) == 1)
    i1, i2 = np.flatnonzero(first), np.flatnonzero(live & ~first)
    assert len(i1) >= 4 and len(i2) >= 4
    rounds = -(-len(dirs) // len(i1))
    pt = stage_ctx(mcpt_mod, EM.scene_arrays(a, name, False), fixed)
    pt.set_camera(stage["cam"])
    seen = set()
    for r in range(rounds):
        inp = dict(base)
        inp["ray_d"] = base["ray_d"].copy()
        k1 = (np.arange(len(i1)) + r * len(i1)) % len(dirs)
        inp["ray_d"][i1] = dirs[k1]
        inp["ray_d"][i2] = dirs[(np.arange(len(i2)) + r) % len(dirs)]
        seen.update(k1.tolist())
        ref = oracle.stage_logic(ao, stage["cam"], W, H, inp, sf.SPP, max_depth=sf.DEPTH, rr_depth=sf.RR, fixed=fixed)
        got = pt.stage("logic", inp, film=sf.FILM)
        _check_stage("logic", got, ref, ao, oracle)
    pt.close()
    assert seen == set(range(len(dirs)))


# ---------------------------------------------------------------------------------------------
def film_ctx(mcpt, arrays, cam, fixed=False, slots=1):
    pt = mcpt.PathTracer(0, mcpt.default_config(spp=FSPP, max_depth=FDEPTH, fixed=fixed))
    pt.upload_scene(mcpt.desc_from_arrays(arrays))
    pt.set_camera(cam)
    pt.resize(FW, FH)
    if slots != 1:
        pt.set_path_slots(slots)
    return pt


def check_counts(st, rays, cnt):
    """The frame's extension, shadow and BRDF-visibility ray counts and mcpt_debug_ray_counts' totals against the
    oracle's counters (the oracle does not split rays into traversed and resolved in place)."""
    assert (st.extend_rays, st.shadow_rays, st.vis_rays) == (cnt["extend_rays"], cnt["shadow_rays"], cnt["vis_rays"])
    assert rays["extension"] == cnt["extend_rays"] and rays["any_hit"] == cnt["shadow_rays"] + cnt["vis_rays"]
    assert rays["extension_traversed"] <= rays["extension"]
    assert rays["any_hit_traversed"] + rays["any_hit_occluder_cache"] <= rays["any_hit"]


@MODES
@pytest.mark.parametrize("name", FILM_MAPS)
def test_films(mcpt_mod, oracle, scene_c1, name, fixed):
    """Config 1's sphere under each map, 48x32, 4 spp, depth 3, one path slot: film, sample counts and ray
    counts equal oracle.render."""
    a = scene_c1[1]
    cam = mcpt_mod.config_camera(mcpt_mod.CONFIGS[1], FW, FH)
    rL, rs, cnt = oracle.render(EM.scene_arrays(a, name, True), cam, FW, FH, FSPP, FDEPTH, fixed=fixed)
    pt = film_ctx(mcpt_mod, EM.scene_arrays(a, name, False), cam, fixed)
    st = pt.render()
    Ld, smp = pt.film()
    rays = pt.ray_counts()
    pt.close()
    assert np.array_equal(smp, rs)
    assert _same(Ld, rL)
    check_counts(st, rays, cnt)
    if name != "sun_last":
        assert np.count_nonzero(rL) > rL.size // 2  # the light reaches the film


def test_film_two_path_slots(mcpt_mod, oracle, scene_c1):
    """`bands` with two path slots: sample counts equal, radiance within the project's 1e-4 summation-order
    bound."""
    from test_gpu import film_close

    a = scene_c1[1]
    cam = mcpt_mod.config_camera(mcpt_mod.CONFIGS[1], FW, FH)
    rL, rs, cnt = oracle.render(EM.scene_arrays(a, "bands", True), cam, FW, FH, FSPP, FDEPTH)
    pt = film_ctx(mcpt_mod, EM.scene_arrays(a, "bands", False), cam, slots=2)
    st = pt.render()
    Ld, smp = pt.film()
    rays = pt.ray_counts()
    pt.close()
    assert np.array_equal(smp, rs)
    ok, bad = film_close(Ld, rL)
    assert ok, f"{bad} values differ"
    check_counts(st, rays, cnt)


def lamp_scene(mcpt):
    """Config 1's sphere with an emissive quad above it (a material of its own), facing down."""
    s = mcpt.Scene()
    s.make_proxy(1)
    c, ux, uz = (np.array(v, np.float32) for v in ((0, 1.6, 0), (0.8, 0, 0), (0, 0, 0.8)))
    p = [c - ux - uz, c + ux - uz, c + ux + uz, c - ux + uz]
    n = np.tile(np.array((0, -1, 0), np.float32), (2, 1))
    s.add_mesh(np.array([p[0], p[0]]), np.array([p[1], p[2]]), np.array([p[2], p[3]]), n, n, n, (0.8, 0.8, 0.8))
    s.build(**mcpt.DEFAULT_BVH)
    a = s.arrays()
    lamp = np.flatnonzero(np.asarray(a["v0"])[:, 1] > 1.5)
    assert len(lamp) == 2
    mat = int(a["mat"][lamp[0]])
    assert (a["mat"] == mat).sum() == 2
    return a, ER.table(len(a["mat_params"]), {mat: (6.0, 5.0, 4.0)})


def test_film_with_emitter_sampling(mcpt_mod, oracle):
    """`bands` beside an emissive quad with emitter sampling on: the env light's term and the emitter's are
    added side by side; the film equals the loop of tests/emitter_ref.py."""
    a0, E = lamp_scene(mcpt_mod)
    cam = mcpt_mod.config_camera(mcpt_mod.CONFIGS[1], FW, FH)
    rL, rs, cnt = MR.render(oracle, EM.scene_arrays(a0, "bands", True), cam, FW, FH, FSPP, max_depth=FDEPTH,
                            emission=E, sample=True)
    pL = MR.render(oracle, EM.scene_arrays(a0, "bands", True), cam, FW, FH, FSPP, max_depth=FDEPTH, emission=E)[0]
    assert cnt["emitter_rays"] > 1000 and ((rL != pL).any(axis=2)).sum() > 100  # the emitter term is in the film
    pt = film_ctx(mcpt_mod, EM.scene_arrays(a0, "bands", False), cam)
    pt.set_emission(E)
    pt.set_emitter_sampling(True)
    pt.set_skip_discarded(False)  # every stage as the reference runs it
    st = pt.render()
    Ld, smp = pt.film()
    stats = pt.emitter_stats()
    pt.close()
    assert stats["active"] and stats["entries"] == 2
    assert np.array_equal(smp, rs) and _same(Ld, rL)
    assert (st.extend_rays, st.shadow_rays, st.vis_rays) == (cnt["extend_rays"], cnt["shadow_rays"], cnt["vis_rays"])
    assert stats["emitter_rays"] == cnt["emitter_rays"]
