"""MIS between emitter samples and collected emission on the device: the MIS
instantiations of k_shade and k_material and the pick-by-record table against the reference loop of
tests/emitter_mis_ref.py, bit for bit, and the switch's life on a live context.

32 x 32 film, 4 spp, depth 5, config 2's proxy under a black environment with MATS_LIT emissive, unless
stated, as in tests/test_emitter_gpu.py, whose helpers and lamp-cube scene are used.  Reference films are
computed once per module."""
import numpy as np
import pytest

import emission_ref as ER
import emitter_mis_ref as XR
import refit_ref as RF
from test_emitter_gpu import DEPTH, RAYS, SPP, H, W, ctx, frame, lamp_cube, rays, same_film  # noqa: F401  (lamp_cube: fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def c2(mcpt_mod, scene_c2):
    a = ER.black(scene_c2[1])
    E = ER.table(len(a["mat_params"]), {ER.MATS_LIT[0]: (3.0, 2.0, 1.0), ER.MATS_LIT[1]: (0.5, 2.0, 8.0)})
    return dict(desc=mcpt_mod.desc_from_arrays(a), a=a, cam=mcpt_mod.config_camera(mcpt_mod.CONFIGS[2], W, H), E=E)


@pytest.fixture(scope="module")
def refs(oracle, c2):
    """Reference MIS films per mode, computed once."""
    cache = {}

    def get(fixed):
        if fixed not in cache:
            cache[fixed] = XR.render(oracle, c2["a"], c2["cam"], W, H, SPP, max_depth=DEPTH, fixed=fixed, emission=c2["E"],
                                     sample=True, mis=True)
        return cache[fixed]

    return get


def mis_ctx(mcpt, *args, mis=True, **kw):
    p = ctx(mcpt, *args, **kw)
    p.set_emitter_mis(mis)
    return p


def one(mcpt, *args, **kw):
    p = mis_ctx(mcpt, *args, **kw)
    f = frame(p)
    p.close()
    return f


@pytest.mark.parametrize("fixed", [False, True])
def test_film_equals_the_reference_loop(mcpt_mod, c2, refs, fixed):
    rLd, rsm, rc = refs(fixed)
    # skip switch off: every stage as the reference runs it
    p = mis_ctx(mcpt_mod, c2["desc"], c2["cam"], c2["E"], sample=True, fixed=fixed, skip=False)
    got = frame(p)
    counts, stats = p.ray_counts(), p.emitter_stats()
    p.close()
    assert stats["active"] and stats["mis"]
    assert same_film(got, (rLd, rsm))
    assert got[2] == tuple(rc[k] for k in RAYS)
    assert stats["emitter_rays"] == rc["emitter_rays"] > 0
    # the run without MIS: the same rays, all five counts and the emitter rays; another film
    q = ctx(mcpt_mod, c2["desc"], c2["cam"], c2["E"], sample=True, fixed=fixed, skip=False)
    clean = frame(q)
    qc, qs = q.ray_counts(), q.emitter_stats()
    q.close()
    assert not qs["mis"] and clean[2] == got[2] and qc == counts and qs["emitter_rays"] == stats["emitter_rays"]
    differ = int((clean[0] != got[0]).any(axis=2).sum())
    print("pixels MIS changes:", differ)
    assert differ > 300
    # skip switch on (the default): the same film, from the ray kept in nee0 / nee1 for the paths it ends
    r = mis_ctx(mcpt_mod, c2["desc"], c2["cam"], c2["E"], sample=True, fixed=fixed, skip=True)
    skipped = frame(r)
    assert r.ray_counts()["extension"] == counts["extension"] and r.ray_counts()["any_hit"] == counts["any_hit"]
    r.close()
    assert same_film(skipped, got) and skipped[2] == got[2]


@pytest.mark.parametrize("fixed", [False, True])
def test_lamp_cube(mcpt_mod, oracle, lamp_cube, fixed):
    """Inside the closed cube most paths hit the lamp at len >= 2, so every branch of the collection weight
    runs; with the skip switch off and on."""
    s, a, cam = lamp_cube
    rLd, rsm, rc = XR.render(oracle, a, cam, W, H, SPP, max_depth=DEPTH, fixed=fixed, emission=s.emission(), sample=True,
                             mis=True)
    for skip in (False, True):
        p = mis_ctx(mcpt_mod, s, cam, None, sample=True, fixed=fixed, skip=skip)
        assert p.emitter_stats()["entries"] == 2 and p.emitter_stats()["mis"]
        got = frame(p)
        n = p.emitter_stats()["emitter_rays"]
        p.close()
        assert same_film(got, (rLd, rsm)) and got[2] == tuple(rc[k] for k in RAYS)
        assert n == rc["emitter_rays"] if not skip else 0 < n <= rc["emitter_rays"]


def test_path_slots(mcpt_mod, c2, refs):
    from test_gpu import film_close

    rLd, rsm, _ = refs(False)
    got = one(mcpt_mod, c2["desc"], c2["cam"], c2["E"], sample=True, slots=3)
    assert np.array_equal(got[1], rsm)
    ok, bad = film_close(got[0], rLd)  # the project's 1e-4 summation-order tolerance
    assert ok, f"{bad} values differ"


def test_budget_map(mcpt_mod, c2, refs):
    """k_shade's map instantiation with MIS: pixel p under a budget map is pixel p of the uniform render
    at its budget, bit for bit (the composition property of tests/test_sample_budget_gpu.py)."""
    p = mis_ctx(mcpt_mod, c2["desc"], c2["cam"], c2["E"], sample=True)
    full = frame(p)
    assert same_film(full, refs(False)[:2])
    p.set_spp(2)
    p.clear()
    half = frame(p)
    p.set_spp(SPP)
    yy, xx = np.mgrid[0:H, 0:W]
    m = np.where((xx + yy) % 2 == 0, 2, SPP).astype(np.uint32)
    p.set_sample_budget(m)
    p.clear()
    got = frame(p)
    assert p.emitter_stats()["mis"]
    p.close()
    want = (np.where((m == 2)[..., None], half[0], full[0]), np.where(m == 2, half[1], full[1]))
    assert same_film(got, want) and not same_film(got, full)


def test_both_uploads(mcpt_mod, c2, refs):
    """A device-built tree orders the records differently: pick_rec is keyed by record all the same."""
    host = one(mcpt_mod, c2["desc"], c2["cam"], c2["E"], sample=True, gpu_bvh=False)
    dev = one(mcpt_mod, c2["desc"], c2["cam"], c2["E"], sample=True, gpu_bvh=True)
    assert same_film(host, dev) and host[2] == dev[2] and same_film(host, refs(False)[:2])


def test_geometry_update_by_refit(mcpt_mod, c2):
    m = ER.black(RF.refitted_desc_arrays(c2["a"], amp=0.02))
    p = mis_ctx(mcpt_mod, c2["desc"], c2["cam"], c2["E"], sample=True)
    before = frame(p)
    p.update_geometry(m["v0"], m["v1"], m["v2"], mode="refit")
    assert p.emitter_stats()["mis"]
    moved = frame(p)
    p.close()
    fresh = one(mcpt_mod, mcpt_mod.desc_from_arrays(m), c2["cam"], c2["E"], sample=True)
    assert same_film(moved, fresh) and moved[2] == fresh[2] and not same_film(moved, before)


def test_toggling(mcpt_mod, c2, refs):
    # MIS on with sampling off, or with nothing that emits: the films of a context that never heard of it
    for E, sample in ((c2["E"], False), (None, True)):
        plain = ctx(mcpt_mod, c2["desc"], c2["cam"], E, sample=sample)
        want = frame(plain)
        plain.close()
        p = mis_ctx(mcpt_mod, c2["desc"], c2["cam"], E, sample=sample)
        assert same_film(frame(p), want) and not p.emitter_stats()["mis"]
        # ... and a change of the switch while sampling is not active restarts nothing
        p.set_emitter_mis(False)
        assert rays(p.render()) == (0, 0, 0) and not p.emitter_stats()["mis"]
        p.set_emitter_mis(True)
        assert rays(p.render()) == (0, 0, 0) and not p.emitter_stats()["mis"]
        p.close()
    p = ctx(mcpt_mod, c2["desc"], c2["cam"], c2["E"], sample=True)
    clean = frame(p)
    assert not p.emitter_stats()["mis"]
    p.set_emitter_mis(False)  # the same value: nothing
    assert rays(p.render()) == (0, 0, 0)
    p.set_emitter_mis(True)  # the film restarts
    assert p.emitter_stats()["mis"]
    on = frame(p)
    assert on[2] == clean[2] and same_film(on, refs(False)[:2]) and not same_film(on, clean)
    p.set_emitter_mis(True)
    assert rays(p.render()) == (0, 0, 0)
    p.set_emitter_mis(False)  # on -> off: the clean split again, bit for bit
    assert not p.emitter_stats()["mis"] and same_film(frame(p), clean)
    # sampling off and on under the switch: MIS follows it
    p.set_emitter_mis(True)
    p.set_emitter_sampling(False)
    assert not p.emitter_stats()["mis"]
    p.set_emitter_sampling(True)
    assert p.emitter_stats()["mis"] and same_film(frame(p), on)
    # the switch survives a scene upload
    p.upload_scene(c2["desc"])
    assert not p.emitter_stats()["mis"]
    p.set_emission(c2["E"])
    assert p.emitter_stats()["mis"] and same_film(frame(p), on)
    p.close()
