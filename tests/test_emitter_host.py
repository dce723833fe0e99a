"""Emitter sampling on the CPU: the reference loop of tests/emitter_ref.py against
emission_ref's, the emitter table's invariants, the agreement of the two estimators on the oracle and
the variance of the sampled frames.  The host table builder itself is tests/native/emitter_table_host.cpp.

Independent seeds differ in bits 20..31 only: rng_key hashes ((pixel << 32) | sample) ^ seed, so seeds
that differ in the low bits permute a pixel's samples and seeds that differ from bit 32 on permute the
pixels, and either leaves a film's mean where it was."""
import os
import subprocess

import numpy as np
import pytest

import emission_ref as ER
import emitter_ref as MR
from conftest import REPO

W = H = 32
SPP = 16  # the agreement and variance frames; see test_estimators_agree_on_the_oracle
REND = (slice(0, H - 1), slice(0, W - 1))  # the last row and column are never rendered


def seeds(base):
    return [(base + k) << 20 for k in range(8)]


@pytest.fixture(scope="module")
def c2(mcpt_mod, scene_c2):
    a = ER.black(scene_c2[1])
    nmat = len(a["mat_params"])
    E = ER.table(nmat, {ER.MATS_LIT[0]: (3.0, 2.0, 1.0), ER.MATS_LIT[1]: (0.5, 2.0, 8.0)})
    return dict(a=a, cam=mcpt_mod.config_camera(mcpt_mod.CONFIGS[2], W, H), E=E, nmat=nmat)


@pytest.mark.parametrize("fixed", [False, True])
def test_off_equals_the_old_reference(oracle, c2, fixed):
    """Sampling off: emitter_ref.render is emission_ref.render bit for bit, with the oracle's film line
    and with the one restated here (mirror), which is what the sampled loop builds on."""
    kw = dict(max_depth=5, fixed=fixed, emission=c2["E"])
    old = ER.render(oracle, c2["a"], c2["cam"], W, H, 4, **kw)
    for mirror in (False, True):
        new = MR.render(oracle, c2["a"], c2["cam"], W, H, 4, mirror=mirror, **kw)
        assert np.array_equal(new[0].view(np.uint32), old[0].view(np.uint32)) and np.array_equal(new[1], old[1])
        assert all(new[2][k] == old[2][k] for k in old[2]) and new[2]["emitter_rays"] == 0
    # switched on without an emissive triangle: inactive, the same film again
    none = MR.render(oracle, c2["a"], c2["cam"], W, H, 4, max_depth=5, fixed=fixed, sample=True,
                     emission=np.zeros((c2["nmat"], 3), np.float32))
    plain = ER.render(oracle, c2["a"], c2["cam"], W, H, 4, max_depth=5, fixed=fixed)
    assert np.array_equal(none[0].view(np.uint32), plain[0].view(np.uint32))


def test_sampling_keeps_paths_and_ray_counts(oracle, c2):
    """The emitter sample draws from slots of its own: samples, the three ray counts and the iteration
    count are those of the unsampled loop; every material evaluation makes one emitter sample."""
    off = MR.render(oracle, c2["a"], c2["cam"], W, H, 4, emission=c2["E"])
    on = MR.render(oracle, c2["a"], c2["cam"], W, H, 4, emission=c2["E"], sample=True)
    assert np.array_equal(on[1], off[1])
    for k in ("extend_rays", "shadow_rays", "vis_rays", "iterations"):
        assert on[2][k] == off[2][k], k
    assert 0 < on[2]["emitter_rays"] <= on[2]["shadow_rays"]
    assert not np.array_equal(on[0], off[0])


def test_table(c2):
    a, E = c2["a"], c2["E"]
    t = MR.scene_table(a, E)
    n = len(t["cdf"])
    mat = np.asarray(a["mat"], np.int32)
    lit = np.isin(mat, ER.MATS_LIT)
    assert n == int(lit.sum()) > 900  # the ceiling's two triangles and the sphere's
    assert (np.diff(t["cdf"]) >= 0).all() and t["cdf"][-1] == np.float32(1)
    assert (np.diff(t["id"].astype(np.int64)) > 0).all()  # ascending scene id
    assert lit[t["pos"]].all()
    # pick: each entry one fp32 rounding of a difference of values <= 1, half an ulp of 1 apiece
    assert abs(float(t["pick"].astype(np.float64).sum()) - 1.0) <= n * 2.0 ** -24
    assert (t["pick"] >= 0).all() and t["pick"][0] == t["cdf"][0]
    # a zero-area triangle of an emissive material and a non-finite weight get no entry
    w = MR.weights(a, E)
    ids = np.asarray(a["tri_id"])
    w2 = w.copy()
    p0, p1 = t["pos"][3], t["pos"][10]
    w2[p0], w2[p1] = 0.0, np.inf
    t2 = MR.build_table(w2, ids)
    assert len(t2["cdf"]) == n - 2 and not np.isin(ids[[p0, p1]], t2["id"]).any() and t2["cdf"][-1] == np.float32(1)
    deg = {k: np.array(a[k], np.float32).reshape(-1, 3).copy() for k in ("v0", "v1", "v2")}
    deg["v1"][p0] = deg["v0"][p0]
    a3 = dict(a)
    a3.update(deg)
    assert MR.weights(a3, E)[p0] == 0 and ids[p0] not in MR.scene_table(a3, E)["id"]
    # any record order gives the same table
    perm = np.random.default_rng(7).permutation(len(w))
    tp = MR.build_table(w[perm], ids[perm])
    for k in ("cdf", "pick", "id"):
        assert np.array_equal(tp[k].view(np.uint32), t[k].view(np.uint32)), k
    assert tp["total"] == t["total"] and np.array_equal(perm[tp["pos"]], t["pos"])
    # nothing emits: empty
    assert len(MR.scene_table(a, np.zeros_like(E))["cdf"]) == 0


def test_native_table_builder():
    """The host builder as a stand-alone program (built by the Makefile, here too if it is not there yet, like
    the other native tests)."""
    subprocess.run(["make", "tests/native/emitter_table_host"], cwd=REPO, check=True, capture_output=True)
    exe = os.path.join(REPO, "tests", "native", "emitter_table_host")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr


def batch(oracle, c2, E, sample, base, **kw):
    """8 independent frames' means per pixel, (8, H - 1, W - 1, 3)."""
    return np.array([MR.render(oracle, c2["a"], c2["cam"], W, H, SPP, emission=E, sample=sample, seed=s, **kw)[0][REND] / SPP
                     for s in seeds(base)])


@pytest.mark.parametrize("mode", ["fixed", "reference"])
def test_estimators_agree_on_the_oracle(oracle, c2, mode):
    """Collection only and sampled, 8 independent seeds each, MATS_LIT emissive under a black environment:
    the film means per channel differ by less than 4 combined standard errors of the 8-seed batch means
    (derived from the runs).  Fixed mode with the default rr_depth; reference mode with rr_depth =
    max_depth, since its unweighted roulette biases the two estimators differently.  16 spp: on the
    reference's own runs the differences were 0.2 / 0.3 / 0.0 (fixed) and 1.8 / 0.1 / 0.3 (reference)
    standard errors, about 25 s for both modes."""
    kw = dict(fixed=True) if mode == "fixed" else dict(fixed=False, rr_depth=5)
    col = batch(oracle, c2, c2["E"], False, 1, **kw).mean(axis=(1, 2))  # (8, 3) film means
    smp = batch(oracle, c2, c2["E"], True, 101, **kw).mean(axis=(1, 2))
    d = col.mean(0) - smp.mean(0)
    se = np.sqrt(col.var(0, ddof=1) / 8 + smp.var(0, ddof=1) / 8)
    print(mode, "means", col.mean(0), smp.mean(0), "difference / combined se", d / se)
    assert (se > 0).all() and (np.abs(d) <= 4 * se).all()


def test_sampled_variance_with_one_small_emitter(oracle, c2):
    """Only the smallest sphere (material 5, radius 0.3) emissive: the per-pixel variance across the 8
    seeds, averaged over the film, of the sampled frames against the collection frames'.

    Measured on the oracle (fixed mode, 32 x 32, these seeds) at the 16 spp of this file: 0.158 for the
    film averages, 0.140 for the per-pixel medians.  The estimate is heavy-tailed, and the film average
    is the statistic that shows it: every sphere rests on the floor, and area sampling without MIS has
    the 1 / dist^2 singularity at the contact, so a single sample can be 600 times its pixel's mean.
    At 8 spp the same seeds gave 1.22 for this sphere and 1.86 / 10.3 / 32.4 / 1.33 for spheres 6 .. 9
    (one such sample each), with the median pixel's ratio at 0.23 - 0.43 (MIS
    between the emitter sample and the collected term is the named follow-up).  The seeds are fixed,
    so the test is deterministic."""
    E = ER.table(c2["nmat"], {5: (40.0, 40.0, 40.0)})
    col = batch(oracle, c2, E, False, 1, fixed=True)
    smp = batch(oracle, c2, E, True, 101, fixed=True)
    vc, vs = col.var(0, ddof=1).mean(axis=-1), smp.var(0, ddof=1).mean(axis=-1)
    ratio = float(vs.mean() / vc.mean())
    print("variance ratio sampled / collection: film average", ratio, "median pixel",
          float(np.median(vs[vc > 0]) / np.median(vc[vc > 0])))
    assert ratio < 1
