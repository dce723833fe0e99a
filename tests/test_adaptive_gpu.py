"""The film's error estimate, the budgets built from it and the adaptive loop on the device (DESIGN.md
section 11; adaptive.hip, mcpt_film_error, mcpt_error_run, mcpt_budget_from_error, render_adaptive)
against the numpy restatement (tests/adaptive_ref.py) and against the films themselves, bit for bit."""
import numpy as np
import pytest

import adaptive_ref as R
from test_sample_budget_gpu import H, TILE, W, camera, composed, film, frame, make_pt

pytestmark = pytest.mark.gpu

f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same(dev, host):
    """Device result against a numpy one: the same bits, where a NaN equals any NaN (the sign and payload
    of a NaN an operation makes are the processor's choice: x86 makes 0xffc00000, gfx950 0x7fc00000)."""
    d, h = np.ascontiguousarray(dev, f32), np.ascontiguousarray(host, f32)
    nd, nh = np.isnan(d), np.isnan(h)
    return np.array_equal(nd, nh) and np.array_equal(d.view(np.uint32)[~nd], h.view(np.uint32)[~nh])


@pytest.fixture(scope="module")
def bare_pt(mcpt_mod):
    """A context without a scene or a film: all mcpt_error_run needs."""
    pt = mcpt_mod.PathTracer(0, mcpt_mod.default_config(spp=1))
    yield pt
    pt.close()


@pytest.mark.parametrize("S", R.SLOTS)
def test_error_run_matches_numpy(mcpt_mod, bare_pt, S):
    Ld, ns = R.make_slots(S)  # the CPU test's inputs (tests/test_adaptive_host.py)
    got = mcpt_mod.error_run(bare_pt, Ld, ns)
    ref = R.film_error(Ld, ns)
    assert same(got, ref), f"{(bits(got) != bits(ref)).sum()} values differ"
    assert bare_pt.adaptive_bytes == 0  # temporary buffers only


def slot_images(pt, S):
    Ls, ns = zip(*(pt.film_slot(k) for k in range(S)))
    return np.stack(Ls), np.stack(ns)


@pytest.mark.parametrize("compact", [False, True], ids=["full", "compact"])
@pytest.mark.parametrize("S,spp", [(4, 6), (3, 7)], ids=["S4spp6", "S3spp7"])
@pytest.mark.parametrize("which", ["c1", "c2", "cube"])
def test_film_error_matches_the_slots(request, mcpt_mod, bare_pt, which, S, spp, compact):
    """Unequal n_k (6 samples over 4 slots, 7 over 3): the device estimate of a real film is the kernel's
    estimate of the slot images, the slot images sum in slot order to the film, and budgets built from
    the estimate equal the restatement's."""
    from test_primary_hits import CAMS
    scene = request.getfixturevalue(CAMS[which][0])[0]
    pt = make_pt(mcpt_mod, scene, camera(mcpt_mod, which), spp, S, False, compact)
    L, s, _ = frame(pt)
    err = pt.film_error()
    Ls, ns = slot_images(pt, S)
    assert len({int(x) for x in ns[:, 0, 0]}) > 1, "the slots were meant to hold unequal counts"
    assert np.array_equal(bits(err), bits(mcpt_mod.error_run(bare_pt, Ls, ns)))
    assert same(err, R.film_error(Ls, ns))
    # the film is the slots summed in slot order
    accL, accn = Ls[0].copy(), ns[0].copy()
    for k in range(1, S):
        accL = (accL + Ls[k]).astype(f32)
        accn = accn + ns[k]
    assert same(L.view(f32), accL) and np.array_equal(accn, s)
    assert np.all(err[:-1, :-1, 2] == min(S, spp)) and np.all(err[:-1, :-1, 3] == spp)
    assert np.all(err[-1, :, 2] == 0) and np.all(err[:, -1, 2] == 0) and np.all(err[-1, :, 0] == -1)
    # budgets, and the counters' readback
    owned = R.rendered_mask(H, W)
    for params in (R.PARAMS, dict(R.PARAMS, target_rel_err=0.01, max_spp=1000, min_spp=0)):
        out = pt.budget_from_error(**params)
        ref, (total, mx, kept) = R.budget(err, owned, **params)
        got = pt.sample_budget()
        assert np.array_equal(got, ref), f"{(got != ref).sum()} budgets differ"
        assert (out["total"], out["max"], out["unchanged"]) == (total, mx, kept)
    pt.close()


def test_film_error_owns_only_its_tiles(mcpt_mod, scene_c2):
    """A context that owns two of the six tiles (one of them in the never-rendered last row): the others
    get K = 0 and budget 0, in both layouts."""
    cam = camera(mcpt_mod, "c2")
    for compact in (False, True):
        pt = make_pt(mcpt_mod, scene_c2[0], cam, 4, 2, False, compact)
        pt.set_tiles([(1, 0), (0, 1)])
        frame(pt)
        err = pt.film_error()
        own = np.zeros((H, W), bool)
        own[0:TILE, TILE:2 * TILE] = True
        own[TILE:, 0:TILE] = True
        ren = own & R.rendered_mask(H, W)
        assert np.all(err[ren][:, 2] == 2) and np.all(err[ren][:, 3] == 4)
        assert np.all(err[~own] == f32([-1, 0, 0, 0]))
        Ls, ns = slot_images(pt, 2)
        assert not ns[:, ~own].any() and same(err, R.film_error(Ls, ns))
        out = pt.budget_from_error(**R.PARAMS)
        ref, (total, mx, kept) = R.budget(err, ren, **R.PARAMS)
        assert np.array_equal(pt.sample_budget(), ref) and (out["total"], out["max"], out["unchanged"]) == (total, mx, kept)
        pt.close()


def test_render_adaptive(mcpt_mod, scene_c1):
    """Config 1 at S = 4, min 4, max 16, two rounds: every rendered pixel ends with exactly its budget,
    and the film is, pixel by pixel, the uniform render at that pixel's budget."""
    S = 4
    pt = make_pt(mcpt_mod, scene_c1[0], camera(mcpt_mod, "c1"), 4, S)
    pt.clear()
    stats, budgets = pt.render_adaptive(target=0.05, min_spp=4, max_spp=16, rounds=2)
    L, s = film(pt)
    m = pt.sample_budget()
    ren = R.rendered_mask(H, W)
    print(f"budgets {budgets}; values {np.unique(m[ren])}; rays {[st.rays for st in stats]}")
    assert np.array_equal(s[ren], m[ren]) and not m[~ren].any() and not s[~ren].any()
    assert m[ren].min() >= 4 and m[ren].max() <= 16
    assert budgets[0]["max"] > 4, "nothing asked for more samples: the loop was not exercised"
    assert budgets[1]["total"] >= budgets[0]["total"]  # budgets never go below the counts
    values = [int(v) for v in np.unique(m[ren])]
    assert len(values) <= 13
    rays_adaptive = pt.ray_counts()["extension"]
    pt.set_sample_budget(None)
    uni = {}
    for v in values:
        pt.set_spp(v)
        uni[v] = frame(pt)[:2]
    wantL, wants = composed(uni, np.where(ren, m, values[0]))
    assert np.array_equal(s[ren], wants[ren])
    assert np.array_equal(L[ren], wantL[ren]), f"{(L[ren] != wantL[ren]).sum()} film values differ"
    assert rays_adaptive > 0
    pt.close()
