"""Emitter sampling on the device: the sampling instantiations of k_shade and
k_material and k_trace's finite any-hit rays against the reference loop of tests/emitter_ref.py, bit
for bit, and the table's life on a live context.

32 x 32 film, 4 spp, depth 5, config 2's proxy (4810 triangles, 10 materials) under a black environment
with MATS_LIT emissive, unless stated.  Reference films are computed once per module."""
import os

import numpy as np
import pytest

import emission_ref as ER
import emitter_ref as MR
import refit_ref as RF
from conftest import ASSETS

pytestmark = pytest.mark.gpu
W = H = 32
SPP, DEPTH = 4, 5
RAYS = ("extend_rays", "shadow_rays", "vis_rays")


def u32(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def same_film(f, g):
    """Bitwise in Ld (a NaN in both counts as equal: its payload is not the reference's to fix) and samples."""
    a, b = np.asarray(f[0], np.float32), np.asarray(g[0], np.float32)
    both_nan = np.isnan(a) & np.isnan(b)
    return bool(((u32(a) == u32(b)) | both_nan).all()) and np.array_equal(f[1], g[1])


def rays(st):
    return tuple(int(getattr(st, k)) for k in RAYS)


@pytest.fixture(scope="module")
def c2(mcpt_mod, scene_c2):
    s, a0 = scene_c2
    a = ER.black(a0)
    E = ER.table(len(a["mat_params"]), {ER.MATS_LIT[0]: (3.0, 2.0, 1.0), ER.MATS_LIT[1]: (0.5, 2.0, 8.0)})
    return dict(desc=mcpt_mod.desc_from_arrays(a), a=a, cam=mcpt_mod.config_camera(mcpt_mod.CONFIGS[2], W, H), E=E)


@pytest.fixture(scope="module")
def refs(oracle, c2):
    """Reference films per (fixed, sampled), computed once."""
    cache = {}

    def get(fixed, sample=True):
        if (fixed, sample) not in cache:
            cache[(fixed, sample)] = MR.render(oracle, c2["a"], c2["cam"], W, H, SPP, max_depth=DEPTH, fixed=fixed,
                                               emission=c2["E"], sample=sample)
        return cache[(fixed, sample)]

    return get


def ctx(mcpt, scene, cam, E=None, sample=False, fixed=False, gpu_bvh=False, slots=1, skip=True, tiny=False):
    p = mcpt.PathTracer(0, mcpt.default_config(spp=SPP, max_depth=DEPTH, fixed=fixed))
    p.upload_scene(scene, gpu_bvh=gpu_bvh)
    if E is not None:
        p.set_emission(E)
    if sample:
        p.set_emitter_sampling(True)
    p.set_camera(cam)
    p.resize(W, H)
    if slots != 1:
        p.set_path_slots(slots)
    p.set_skip_discarded(skip)
    if tiny:
        p.set_tiny_lds_stack(True)
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
@pytest.mark.parametrize("fixed", [False, True])
def test_film_equals_the_reference_loop(mcpt_mod, c2, refs, fixed):
    rLd, rsm, rc = refs(fixed)
    cLd = refs(fixed, False)[0]
    assert ((rLd != cLd).any(axis=2)).sum() > 300  # sampling changes most of the film
    # skip switch off: every stage as the reference runs it
    p = ctx(mcpt_mod, c2["desc"], c2["cam"], c2["E"], sample=True, fixed=fixed, skip=False)
    got = frame(p)
    counts, stats = p.ray_counts(), p.emitter_stats()
    p.close()
    assert stats["active"] and stats["entries"] == len(MR.scene_table(c2["a"], c2["E"])["cdf"])
    assert same_film(got, (rLd, rsm))
    assert got[2] == tuple(rc[k] for k in RAYS)
    assert stats["emitter_rays"] == rc["emitter_rays"] > 0
    # mcpt_debug_ray_counts: those of the same scene without sampling
    q = ctx(mcpt_mod, c2["desc"], c2["cam"], c2["E"], sample=False, fixed=fixed, skip=False)
    plain = frame(q)
    pc = q.ray_counts()
    assert q.emitter_stats()["emitter_rays"] == 0 and not q.emitter_stats()["active"]
    q.close()
    assert same_film(plain, refs(fixed, False)[:2])
    assert plain[2] == got[2]
    assert counts == pc  # all five: emitter rays are no rays "as the reference traces them"
    # skip switch on (the default): the same film, no more emitter rays
    r = ctx(mcpt_mod, c2["desc"], c2["cam"], c2["E"], sample=True, fixed=fixed, skip=True)
    skipped = frame(r)
    n_skip = r.emitter_stats()["emitter_rays"]
    assert r.ray_counts()["extension"] == counts["extension"] and r.ray_counts()["any_hit"] == counts["any_hit"]
    r.close()
    assert same_film(skipped, got) and skipped[2] == got[2]
    assert 0 < n_skip <= stats["emitter_rays"]
    print("emitter rays", stats["emitter_rays"], "with the skip switch", n_skip)


def test_path_slots(mcpt_mod, c2, refs):
    from test_gpu import film_close

    rLd, rsm, _ = refs(False)
    got = one(mcpt_mod, c2["desc"], c2["cam"], c2["E"], sample=True, slots=3)
    assert np.array_equal(got[1], rsm)
    ok, bad = film_close(got[0], rLd)  # the project's 1e-4 summation-order tolerance
    assert ok, f"{bad} values differ"


def test_table_for_both_uploads(mcpt_mod, c2):
    t = MR.scene_table(c2["a"], c2["E"])
    films = []
    for gpu in (False, True):
        p = ctx(mcpt_mod, c2["desc"], c2["cam"], c2["E"], sample=True, gpu_bvh=gpu)
        cdf, pick, tid = p.emitter_table()
        assert np.array_equal(u32(cdf), u32(t["cdf"])) and np.array_equal(u32(pick), u32(t["pick"]))
        assert np.array_equal(tid, t["id"])
        assert p.emitter_stats()["total_weight"] == t["total"]
        films.append(frame(p))
        p.close()
    assert same_film(films[0], films[1]) and films[0][2] == films[1][2]


@pytest.mark.parametrize("fixed", [False, True])
def test_other_lights(mcpt_mod, oracle, fixed):
    """The config's HRDI environment and a directional light beside the emitters: a vertex that draws the
    delta light makes no BRDF visibility ray, and still an emitter ray."""
    s = mcpt_mod.Scene()
    s.make_proxy(2, mcpt_mod.ASSET_DIR)
    s.add_dir_light((-0.3, -1.0, -0.2), (1.0, 0.9, 0.8), 2.0)
    s.build(8)
    a = s.arrays()
    cam = mcpt_mod.config_camera(mcpt_mod.CONFIGS[2], W, H)
    E = ER.table(len(a["mat_params"]), {ER.MATS_LIT[0]: (3.0, 2.0, 1.0), ER.MATS_LIT[1]: (0.5, 2.0, 8.0)})
    rLd, rsm, rc = MR.render(oracle, a, cam, W, H, SPP, max_depth=DEPTH, fixed=fixed, emission=E, sample=True)
    assert 0 < rc["vis_rays"] < rc["shadow_rays"]  # some vertices drew the delta light
    p = ctx(mcpt_mod, s, cam, E, sample=True, fixed=fixed, skip=False)
    got = frame(p)
    n = p.emitter_stats()["emitter_rays"]
    p.close()
    assert same_film(got, (rLd, rsm)) and got[2] == tuple(rc[k] for k in RAYS) and n == rc["emitter_rays"]


@pytest.mark.parametrize("mode", ["refit", "rebuild"])
def test_geometry_update(mcpt_mod, c2, mode):
    gpu = mode == "rebuild"
    m = ER.black(RF.refitted_desc_arrays(c2["a"], amp=0.02))
    p = ctx(mcpt_mod, c2["desc"], c2["cam"], c2["E"], sample=True, gpu_bvh=gpu)
    before, tab0 = frame(p), p.emitter_table()
    p.update_geometry(m["v0"], m["v1"], m["v2"], mode=mode)
    tab1 = p.emitter_table()
    moved = frame(p)
    q = ctx(mcpt_mod, mcpt_mod.desc_from_arrays(m), c2["cam"], c2["E"], sample=True, gpu_bvh=gpu)
    tab2, fresh = q.emitter_table(), frame(q)
    q.close()
    t = MR.scene_table(m, c2["E"])
    for x, y in zip(tab1, tab2):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    assert np.array_equal(u32(tab1[0]), u32(t["cdf"])) and np.array_equal(u32(tab1[1]), u32(t["pick"]))
    assert not np.array_equal(u32(tab0[0]), u32(tab1[0]))  # the areas moved
    assert same_film(moved, fresh) and moved[2] == fresh[2] and not same_film(moved, before)
    p.upload_scene(c2["desc"], gpu_bvh=gpu)  # an upload drops the table; the switch stays
    assert len(p.emitter_table()[0]) == 0 and not p.emitter_stats()["active"]
    p.set_emission(c2["E"])
    assert np.array_equal(u32(p.emitter_table()[0]), u32(tab0[0])) and p.emitter_stats()["active"]
    assert same_film(frame(p), before)
    p.close()


def test_inactive_and_toggling(mcpt_mod, c2, refs):
    nmat = len(c2["a"]["mat_params"])
    off = one(mcpt_mod, c2["desc"], c2["cam"], None)
    # on with no table, and with an all-zero one: the films of a context that never heard of sampling
    for E in (None, np.zeros((nmat, 3), np.float32)):
        p = ctx(mcpt_mod, c2["desc"], c2["cam"], E, sample=True)
        assert same_film(frame(p), off)
        s = p.emitter_stats()
        assert not s["active"] and s["entries"] == 0 and s["emitter_rays"] == 0 and len(p.emitter_table()[0]) == 0
        p.close()
    # toggling marks the film stale: the next render starts over; the same value again does nothing
    p = ctx(mcpt_mod, c2["desc"], c2["cam"], c2["E"], sample=False)
    collected = frame(p)
    assert same_film(collected, refs(False, False)[:2])
    assert rays(p.render()) == (0, 0, 0)  # the film is complete
    p.set_emitter_sampling(False)
    assert rays(p.render()) == (0, 0, 0)
    p.set_emitter_sampling(True)
    sampled = frame(p)
    assert sampled[2] == collected[2] and same_film(sampled, refs(False)[:2])
    p.set_emitter_sampling(True)
    assert rays(p.render()) == (0, 0, 0)
    p.set_emitter_sampling(False)
    assert same_film(frame(p), collected)
    # the emission changes while sampling is on: the table follows
    p.set_emitter_sampling(True)
    p.set_emission(np.float32(2.0) * c2["E"])
    t = MR.scene_table(c2["a"], np.float32(2.0) * c2["E"])
    assert np.array_equal(u32(p.emitter_table()[0]), u32(t["cdf"])) and p.emitter_stats()["total_weight"] == t["total"]
    p.set_emission(None)
    assert not p.emitter_stats()["active"] and same_film(frame(p), off)
    p.close()


# ---------------------------------------------------------------------------------------------
def quad(c, ux, uz, nrm):
    """Two triangles of the quad c +- ux +- uz with the face normal nrm: (v0, v1, v2, n0, n1, n2)."""
    c, ux, uz = (np.asarray(v, np.float32) for v in (c, ux, uz))
    p = [c - ux - uz, c + ux - uz, c + ux + uz, c - ux + uz]
    v0, v1, v2 = np.array([p[0], p[0]]), np.array([p[1], p[2]]), np.array([p[2], p[3]])
    n = np.tile(np.asarray(nrm, np.float32), (2, 1))
    return v0, v1, v2, n, n, n


@pytest.fixture(scope="module")
def lamp_cube(mcpt_mod, scene_cube):
    """Cube.glb seen from inside: its top face is the lamp (material 0), the other faces material 1, a
    small quad hangs between the camera and the lamp (2), and a large quad lies above the cube (3):
    beyond the lamp, where only a ray that ignores its end can reach it."""
    a = scene_cube[1]
    tri = {k: np.asarray(a[k], np.float32).reshape(-1, 3) for k in ("v0", "v1", "v2", "n0", "n1", "n2")}
    allv = np.concatenate([tri["v0"], tri["v1"], tri["v2"]])
    lo, hi = allv.min(0), allv.max(0)
    cen, half = (lo + hi) / 2, (hi - lo) / 2
    top = (tri["v0"][:, 1] == hi[1]) & (tri["v1"][:, 1] == hi[1]) & (tri["v2"][:, 1] == hi[1])
    assert top.sum() == 2
    s = mcpt_mod.Scene()
    s.add_mesh(*[tri[k][top] for k in ("v0", "v1", "v2", "n0", "n1", "n2")], (0.8, 0.8, 0.8))
    s.add_mesh(*[tri[k][~top] for k in ("v0", "v1", "v2", "n0", "n1", "n2")], (0.7, 0.5, 0.3))
    ex, ez = np.array([half[0], 0, 0], np.float32), np.array([0, 0, half[2]], np.float32)
    s.add_mesh(*quad(cen + np.array([0, 0.5 * half[1], 0], np.float32), 0.3 * ex, 0.3 * ez, (0, -1, 0)), (0.2, 0.4, 0.8))
    s.add_mesh(*quad(cen + np.array([0, 1.5 * half[1], 0], np.float32), 2 * ex, 2 * ez, (0, -1, 0)), (0.9, 0.9, 0.9))
    s.set_env_color((0.0, 0.0, 0.0))
    s.set_emission(0, (6.0, 5.0, 4.0))
    s.build(8)
    cam = mcpt_mod.make_camera(tuple(float(x) for x in cen - np.array([0, 0.5 * half[1], 0])), yaw_deg=-90.0, pitch_deg=35.0,
                               fovy_deg=70.0, aspect=1.0)
    return s, s.arrays(), cam


@pytest.mark.parametrize("tiny", [False, True])
@pytest.mark.parametrize("fixed", [False, True])
def test_finite_rays_on_the_lamp_cube(mcpt_mod, oracle, lamp_cube, fixed, tiny):
    """Every emitter ray here ends on a face of a closed cube with a quad beyond it: a tmax that is
    ignored, or applied at one acceptance site only, has the lamp itself (or the quad above it) occlude
    the sample, and the film differs from the reference.  Some samples lie behind the hanging quad."""
    s, a, cam = lamp_cube
    E = s.emission()
    kw = dict(max_depth=DEPTH, fixed=fixed, emission=E)
    rLd, rsm, rc = MR.render(oracle, a, cam, W, H, SPP, sample=True, **kw)
    cLd = MR.render(oracle, a, cam, W, H, SPP, **kw)[0]
    lit = (rLd != cLd).any(axis=2)
    print("pixels the emitter samples change:", int(lit.sum()), "emitter rays", rc["emitter_rays"])
    assert lit.sum() > 300 and rc["emitter_rays"] > 1000
    p = ctx(mcpt_mod, s, cam, None, sample=True, fixed=fixed, skip=False, tiny=tiny)
    assert p.emitter_stats()["entries"] == 2
    got = frame(p)
    n = p.emitter_stats()["emitter_rays"]
    p.close()
    assert same_film(got, (rLd, rsm)) and got[2] == tuple(rc[k] for k in RAYS) and n == rc["emitter_rays"]
