"""Glossy and metallic materials on the device against the CPU oracle (DESIGN.md "Parity tests").

Every loader and proxy gives every triangle fresnel 0.04, roughness 1, metallic 0, where a2 - 1 == 0
and the GGX terms of device/mcpt_core.hpp are constants.  Here the fixture scenes wear
material_fixtures.PALETTE (19 materials over the range the ABI accepts, non-dyadic roughnesses) and
k_material's merged brdf_sample_wi / brdf_f_pdf are held to the oracle's separate functions bit for
bit: stage by stage on generic and on grazing path states, film by film, and across the two
switches that decide whether a BRDF term is evaluated at all."""
import functools
import os

import numpy as np
import pytest

import material_fixtures as mf
import stage_fixtures as sf
from stage_checks import _check_stage, _same
from test_gpu import film_close

pytestmark = pytest.mark.gpu

N_PATHS = 4096
FILM_W, FILM_H, FILM_SPP = 64, 48, 8


@functools.lru_cache(maxsize=None)
def _scene(cid):
    """(arrays of the fixture scene of config cid, the same wearing the palette)"""
    import mcpt

    a = sf.stage_scene(mcpt, cid).arrays()
    return a, mf.with_palette(a)


@functools.lru_cache(maxsize=None)
def _state(cid, kind):
    import oracle_py

    a, _ = _scene(cid)
    if kind == "generic":
        return sf.material_state(a, oracle_py.trace_closest, cid, N_PATHS)
    return mf.grazing_state(a, oracle_py.trace_closest, N_PATHS, 11, cid)


@pytest.mark.parametrize("kind", ["generic", "grazing"])
@pytest.mark.parametrize("fixed", [False, True], ids=["reference", "fixed"])
@pytest.mark.parametrize("scene", ["c1dir", "c2"])
def test_material_stage_palette_parity(mcpt_mod, oracle, scene, fixed, kind):
    """k_material on palette scenes equals the oracle's or_stage_material in every output field: 4096
    generic paths (every palette row under at least 32 of them, so both lobes of every material are
    drawn but for a 2^-32 chance) and up to 4096 grazing paths (at least 1000 with shading n.wo < 0.02
    and 500 with n.wo < 0: the fmx(..., BRDF_EPS) clamp on every n.wo), in both integrator modes."""
    cid = sf.SCENES[scene]
    a, ap = _scene(cid)
    inp = _state(cid, kind)
    assert len(inp["flags"]) <= N_PATHS
    if kind == "generic":
        rows = mf.rows_hit(a, inp)
        assert rows.min() >= 32, rows
    else:
        ndw = mf.n_dot_wo(a, oracle.trace_closest, inp)
        assert (ndw < 0.02).sum() >= 1000 and (ndw < 0).sum() >= 500, ((ndw < 0.02).sum(), (ndw < 0).sum())
    ref = oracle.stage_material(ap, inp, max_depth=sf.DEPTH, rr_depth=sf.RR, fixed=fixed)
    pt = mcpt_mod.PathTracer(0, mcpt_mod.default_config(spp=sf.SPP, max_depth=sf.DEPTH, rr_depth=sf.RR, fixed=fixed))
    pt.upload_scene(mcpt_mod.desc_from_arrays(ap))
    pt.set_camera(sf.stage_camera(mcpt_mod, cid))
    got = pt.stage("material", inp)
    pt.close()
    _check_stage("material", got, ref, ap, oracle)


def _film_pt(mcpt, ap, cid, fixed=False, slots=1, rr=sf.RR):
    cam = mcpt.config_camera(mcpt.CONFIGS[cid], FILM_W, FILM_H)
    pt = mcpt.PathTracer(0, mcpt.default_config(spp=FILM_SPP, max_depth=sf.DEPTH, rr_depth=rr, tile=64, fixed=fixed))
    pt.upload_scene(mcpt.desc_from_arrays(ap))
    pt.set_camera(cam)
    pt.resize(FILM_W, FILM_H, 64, 64)
    if slots != 1:
        pt.set_path_slots(slots)
    return pt, cam


@pytest.mark.parametrize("slots", [1, 2])
@pytest.mark.parametrize("fixed", [False, True], ids=["reference", "fixed"])
@pytest.mark.parametrize("scene", ["c1dir", "c2"])
def test_film_palette_parity(mcpt_mod, oracle, scene, fixed, slots):
    """Palette scenes rendered whole (64 x 48, 8 spp, depth 5, roulette from 3): with one path slot
    the film's bits and sample counts equal oracle.render's; with two slots only the summation order
    differs, so sample counts are exact and radiance is within the slot tests' 1e-4."""
    cid = sf.SCENES[scene]
    _, ap = _scene(cid)
    pt, cam = _film_pt(mcpt_mod, ap, cid, fixed, slots)
    st = pt.render()
    Ld, smp = pt.film()
    pt.close()
    rL, rs, cnt = oracle.render(ap, cam, FILM_W, FILM_H, FILM_SPP, sf.DEPTH, sf.RR, fixed=fixed)
    assert np.array_equal(smp, rs)
    assert np.all(rs[:-1, :-1] == FILM_SPP)
    if slots == 1:
        assert _same(Ld, rL), f"{int((Ld.view(np.uint32) != rL.view(np.uint32)).sum())} film values differ"
    else:
        ok, nbad = film_close(Ld, rL)
        assert ok, f"{nbad} radiance values differ"
    assert (st.extend_rays, st.shadow_rays, st.vis_rays) == (cnt["extend_rays"], cnt["shadow_rays"], cnt["vis_rays"])


def test_palette_film_same_with_and_without_occluder_cache(mcpt_mod):
    """The occluder cache decides whether k_material evaluates the BRDF-sample term at all (a ray it
    resolves as occluded needs none), which with glossy materials is a term whose f / pdf can be
    large: the config-2 palette film is bit-identical with the cache (default) and without it
    (MCPT_OCC_G=0 at upload)."""
    _, ap = _scene(2)

    def run(env):
        old = os.environ.get("MCPT_OCC_G")
        if env is None:
            os.environ.pop("MCPT_OCC_G", None)
        else:
            os.environ["MCPT_OCC_G"] = env
        try:
            pt, _ = _film_pt(mcpt_mod, ap, 2)
        finally:
            if old is None:
                os.environ.pop("MCPT_OCC_G", None)
            else:
                os.environ["MCPT_OCC_G"] = old
        pt.clear()
        st = pt.render()
        L, smp = pt.film()
        out = (L.copy(), smp.copy(), (st.extend_rays, st.shadow_rays, st.vis_rays), pt.occ_stats())
        pt.close()
        return out

    off, on = run("0"), run(None)
    assert off[3] == (0, False) and on[3][1]
    print(f"any-hit rays {sum(on[2][1:])}, resolved by the cache {on[3][0]}")
    assert on[3][0] > 0
    assert np.array_equal(on[0].view(np.uint32), off[0].view(np.uint32))
    assert np.array_equal(on[1], off[1]) and on[2] == off[2]


@pytest.mark.parametrize("fixed", [False, True], ids=["reference", "fixed"])
def test_palette_film_same_with_and_without_skip_discarded(mcpt_mod, fixed):
    """mcpt_set_skip_discarded skips the continuation sample of a path the next logic pass discards
    (k_material's no_cont branch); with glossy materials that sample's f / pdf ratio can be large.
    The config-2 palette film, its sample counts and its ray counts are the same with the switch on
    and off, and the switch does skip evaluations here."""
    _, ap = _scene(2)
    pt, _ = _film_pt(mcpt_mod, ap, 2, fixed)
    out = []
    for on in (True, False):
        pt.set_skip_discarded(on)
        pt.clear()
        st = pt.render()
        L, s = pt.film()
        out.append((L.copy().view(np.uint32), s.copy(), (st.extend_rays, st.shadow_rays, st.vis_rays), pt.discard_stats()))
    pt.close()
    (La, sa, ca, ka), (Lb, sb, cb, kb) = out
    assert np.array_equal(La, Lb), f"films differ in {(La != Lb).sum()} values"
    assert np.array_equal(sa, sb) and ca == cb
    assert ka["evaluations_not_run"] > 0 and ka["extension_untraced"] > ka["evaluations_not_run"]
    assert (kb["extension_untraced"], kb["evaluations_not_run"]) == (0, 0)
