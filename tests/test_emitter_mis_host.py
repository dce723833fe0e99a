"""MIS between emitter samples and collected emission on the CPU: the reference
loop of tests/emitter_mis_ref.py against emitter_ref's, the symmetry of the two weights, the agreement of
the MIS estimator with collection only on the oracle, and its variance against both other estimators.

32 x 32 on config 2's proxy, seeds as in tests/test_emitter_host.py (independent seeds differ in bits
20..31 only); the seed families are 1 (collection only), 101 (sampled, no MIS) and 201 (MIS)."""
import numpy as np
import pytest

import emission_ref as ER
import emitter_mis_ref as XR
import emitter_ref as MR

W = H = 32
SPP = 16
REND = (slice(0, H - 1), slice(0, W - 1))  # the last row and column are never rendered
f32 = np.float32


def seeds(base):
    return [(base + k) << 20 for k in range(8)]


@pytest.fixture(scope="module")
def c2(mcpt_mod, scene_c2):
    a = ER.black(scene_c2[1])
    nmat = len(a["mat_params"])
    E = ER.table(nmat, {ER.MATS_LIT[0]: (3.0, 2.0, 1.0), ER.MATS_LIT[1]: (0.5, 2.0, 8.0)})
    return dict(a=a, cam=mcpt_mod.config_camera(mcpt_mod.CONFIGS[2], W, H), E=E, nmat=nmat)


@pytest.mark.parametrize("fixed", [False, True])
def test_mis_off_equals_the_sampling_reference(oracle, c2, fixed):
    """mis=False: the new loop is emitter_ref.render bit for bit, sampled and unsampled; and MIS without
    an emitter is not in effect: the plain film."""
    kw = dict(max_depth=5, fixed=fixed, emission=c2["E"])
    for sample in (True, False):
        old = MR.render(oracle, c2["a"], c2["cam"], W, H, 4, sample=sample, **kw)
        new = XR.render(oracle, c2["a"], c2["cam"], W, H, 4, sample=sample, mis=False, **kw)
        assert np.array_equal(new[0].view(np.uint32), old[0].view(np.uint32)) and np.array_equal(new[1], old[1])
        assert new[2] == old[2]
    unsampled = XR.render(oracle, c2["a"], c2["cam"], W, H, 4, sample=False, mis=True, **kw)  # MIS without sampling
    assert np.array_equal(unsampled[0].view(np.uint32), old[0].view(np.uint32))
    none = XR.render(oracle, c2["a"], c2["cam"], W, H, 4, max_depth=5, fixed=fixed, sample=True, mis=True,
                     emission=np.zeros((c2["nmat"], 3), np.float32))
    plain = ER.render(oracle, c2["a"], c2["cam"], W, H, 4, max_depth=5, fixed=fixed)
    assert np.array_equal(none[0].view(np.uint32), plain[0].view(np.uint32))


def test_mis_keeps_paths_and_ray_counts(oracle, c2):
    """MIS changes weights only: samples, every ray count and the emitter rays are those of the sampled
    loop without it, and the film differs."""
    kw = dict(max_depth=5, emission=c2["E"], sample=True)
    off = XR.render(oracle, c2["a"], c2["cam"], W, H, 4, **kw)
    on = XR.render(oracle, c2["a"], c2["cam"], W, H, 4, mis=True, **kw)
    assert np.array_equal(on[1], off[1]) and on[2] == off[2]
    assert int((on[0] != off[0]).any(axis=-1).sum()) > 300


def test_weight_symmetry(oracle, c2):
    """From one shared origin the emitter sample's pdf (point minus origin, dist^2) and the collection
    formula's (the ray's parameter to the triangle's plane, t^2) are the same density, so the two power
    heuristics against one BRDF pdf sum to one: |wE + wC - 1| <= 1e-4 wherever cosl >= 0.01, about ten
    times the 8.5e-6 measured on 200 000 pairs.  50 000 pairs here: random origins in the scene's box,
    table entries by their cdf, uniform points, the BRDF pdf of a random material of the scene for a
    random normal on the direction's side and a random outgoing direction.  At most 2 % of the pairs may
    fall to the cosl condition (0.9 % measured at 200 000).

    This run: max |wE + wC - 1| = 8.9e-06 at cosl >= 0.01 (1.5e-04 over all pairs), 1.05 % of the pairs
    left out."""
    a, E = c2["a"], c2["E"]
    tab = XR.scene_table(a, E)
    rng = np.random.default_rng(20260118)
    N = 50000
    v0a, v1a, v2a = (np.asarray(a[k], np.float32).reshape(-1, 3) for k in ("v0", "v1", "v2"))
    lo = np.minimum(np.minimum(v0a, v1a), v2a).min(0)
    hi = np.maximum(np.maximum(v0a, v1a), v2a).max(0)
    o = (lo + (hi - lo) * rng.random((N, 3))).astype(np.float32)
    k = np.minimum(np.searchsorted(tab["cdf"], rng.random(N).astype(np.float32), side="right"), len(tab["cdf"]) - 1)
    pos = tab["pos"][k]
    v0, e1, e2 = v0a[pos], v1a[pos] - v0a[pos], v2a[pos] - v0a[pos]
    u1, u2 = rng.random(N).astype(np.float32), rng.random(N).astype(np.float32)
    su = np.sqrt(u1)
    p = (v0 + e1 * (su * (f32(1) - u2))[:, None]) + e2 * (su * u2)[:, None]
    dv = p - o
    d2 = MR._dot(dv, dv)
    dist = np.sqrt(d2)
    d = dv / dist[:, None]
    c = MR._cross(e1, e2)
    lc = np.sqrt(MR._dot(c, c))
    cosl = np.abs(MR._dot(c / lc[:, None], d))
    pdf_e = ((tab["pick"][k] / (f32(0.5) * lc)) * d2) / cosl
    # one BRDF pdf per pair
    n = rng.normal(size=(N, 3)).astype(np.float32)
    n /= np.linalg.norm(n, axis=1, keepdims=True).astype(np.float32)
    n = np.where((MR._dot(n, d) < 0)[:, None], -n, n).astype(np.float32)
    wo = rng.normal(size=(N, 3)).astype(np.float32)
    wo /= np.linalg.norm(wo, axis=1, keepdims=True).astype(np.float32)
    wo = np.where((MR._dot(n, wo) < 0)[:, None], -wo, wo).astype(np.float32)
    params = np.asarray(a["mat_params"], np.float32).reshape(-1, 8)[rng.integers(0, c2["nmat"], N)]
    _, pdf_b = XR.brdf_pdf(oracle, params, n, d, wo)
    wE = XR.power_heuristic(pdf_e, pdf_b)
    wC = XR.collect_weight(pdf_b, tab["pick"][k], v0, e1, e2, o, d)
    keep = cosl >= f32(0.01)
    err = np.abs((wE.astype(np.float64) + wC.astype(np.float64)) - 1.0)
    out = 1.0 - float(keep.mean())
    print("weight symmetry: max |wE + wC - 1|", float(err[keep].max()), "at cosl >= 0.01,", float(err.max()),
          "over all pairs; left out", out)
    assert np.isfinite(err[keep]).all() and float(err[keep].max()) <= 1e-4
    assert out <= 0.02


_batches = {}


def batch(oracle, c2, E, kind, mode):
    """8 independent frames' means per pixel, (8, H - 1, W - 1, 3), of one estimator: "col" (collection
    only, seeds 1..), "smp" (sampled, no MIS, 101..) or "mis" (201..).  Rendered once per module."""
    key = (E.tobytes(), kind, mode)
    if key not in _batches:
        kw = dict(fixed=True) if mode == "fixed" else dict(fixed=False, rr_depth=5)
        base = {"col": 1, "smp": 101, "mis": 201}[kind]
        _batches[key] = np.array([XR.render(oracle, c2["a"], c2["cam"], W, H, SPP, emission=E, sample=kind != "col",
                                            mis=kind == "mis", seed=s, **kw)[0][REND] / SPP for s in seeds(base)])
    return _batches[key]


@pytest.mark.parametrize("mode", ["fixed", "reference"])
def test_estimators_agree_on_the_oracle(oracle, c2, mode):
    """Collection only against MIS, 8 independent seeds each, MATS_LIT emissive under a black environment,
    16 spp: the film means per channel differ by less than 4 combined standard errors of the 8-seed batch
    means.  Fixed mode with the default rr_depth; reference mode with rr_depth = max_depth (its unweighted
    roulette biases estimators differently), the scheme of tests/test_emitter_host.py.

    This run: differences of 0.86 / 0.26 / 0.85 combined standard errors per channel in fixed mode and
    1.97 / 0.77 / 0.08 in reference mode."""
    col = batch(oracle, c2, c2["E"], "col", mode).mean(axis=(1, 2))  # (8, 3) film means
    mis = batch(oracle, c2, c2["E"], "mis", mode).mean(axis=(1, 2))
    d = col.mean(0) - mis.mean(0)
    se = np.sqrt(col.var(0, ddof=1) / 8 + mis.var(0, ddof=1) / 8)
    print(mode, "means", col.mean(0), mis.mean(0), "difference / combined se", d / se)
    assert (se > 0).all() and (np.abs(d) <= 4 * se).all()


@pytest.mark.parametrize("material", [5, 8])
def test_mis_variance_with_one_small_emitter(oracle, c2, material):
    """One sphere emissive at radiance 40, fixed mode: the per-pixel variance across the 8 seeds, averaged
    over the film, of the MIS frames is below both the collection-only frames' and the sampled frames'
    without MIS (each ratio < 1).  Both spheres rest on the floor, where area sampling without MIS has
    its 1 / dist^2 singularity and collection alone rarely finds the emitter.

    This run: MIS / collection and MIS / no-MIS 0.058 and 0.37 for material 5, 0.30 and 0.023 for
    material 8 (film-average variances 2.31 / 0.365 / 0.134 and 6.02 / 78.9 / 1.81)."""
    E = ER.table(c2["nmat"], {material: (40.0, 40.0, 40.0)})
    v = {k: float(batch(oracle, c2, E, k, "fixed").var(0, ddof=1).mean()) for k in ("col", "smp", "mis")}
    print("material", material, "film-average variance col / smp / mis", v["col"], v["smp"], v["mis"], "ratios MIS / col",
          v["mis"] / v["col"], "MIS / smp", v["mis"] / v["smp"])
    assert v["mis"] / v["col"] < 1 and v["mis"] / v["smp"] < 1
