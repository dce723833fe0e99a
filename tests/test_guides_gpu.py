"""First-hit guide buffers (mcpt_guides_render / mcpt_guides_read) against the CPU oracle, bit for bit:
guide sample s of a pixel is the camera ray of film sample s (the oracle's wf_generate restatement),
traced by the oracle's closest hit and accumulated in numpy float32 in sample order."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
f32 = np.float32


def make_pt(mcpt, scene, cam, W, H, spp=4, depth=5, tile=64, slots=1):
    pt = mcpt.PathTracer(0, mcpt.default_config(spp=spp, max_depth=depth, tile=tile))
    pt.upload_scene(scene)
    pt.set_camera(cam)
    pt.resize(W, H, tile, tile)
    if slots > 1:
        pt.set_path_slots(slots)
    return pt


def oracle_guides(oracle, arrays, cam, W, H, n):
    """Sums and counts of n guide samples per rendered pixel, as the issue states them."""
    P = W * H
    alb, nrm = np.zeros((P, 3), f32), np.zeros((P, 3), f32)
    dep, cnt = np.zeros(P, f32), np.zeros(P, np.uint32)
    dead = {"flags": np.ones(P, np.uint32), "hit_tri": np.full(P, -1, np.int32), "ray_d": np.zeros((P, 3), f32),
            "beta": np.zeros((P, 4), f32), "nee0": np.zeros((P, 4), f32), "nee1": np.zeros((P, 4), f32),
            "vis": np.zeros((P, 2), np.uint8), "Ld": np.zeros((P, 3), f32)}
    base = arrays["mat_params"][:, :3].astype(f32)
    for s in range(n):
        out = oracle.stage_logic(arrays, cam, W, H, dict(dead, samples=np.full(P, s, np.uint32)), spp=n)
        q = (out["queued"] & 1) != 0
        pos_t, nm, tri = oracle.trace_closest(arrays, out["ray_o"][q], out["ray_d"][q])
        hit = tri >= 0
        mat = nm[:, 3].astype(np.int32)
        a = np.where(hit[:, None], base[np.where(hit, mat, 0)], f32(1)).astype(f32)
        nn = np.where(hit[:, None], nm[:, :3], f32(0)).astype(f32)
        t = np.where(hit, pos_t[:, 3], f32(0)).astype(f32)
        alb[q] = alb[q] + a
        nrm[q] = nrm[q] + nn
        dep[q] = dep[q] + t
        cnt[q] += 1
    return {"albedo": alb.reshape(H, W, 3), "normal": nrm.reshape(H, W, 3), "depth": dep.reshape(H, W),
            "count": cnt.reshape(H, W)}


def assert_same_guides(g, ref):
    for k in ("albedo", "normal", "depth"):
        assert np.array_equal(g[k].view(np.uint32), ref[k].view(np.uint32)), f"{k} sums differ"
    assert np.array_equal(g["count"], ref["count"]), "counts differ"


CASES = {
    "c1_17x13": ("scene_c1", (0.0, 0.0, 4.0), 17, 13, 1e-4, 4),
    "cube_axis_65x49": ("scene_cube", (0.0, 0.0, 3.0), 65, 49, 0.05, 3),  # along -z: the zero-direction column
}


@pytest.mark.parametrize("case", list(CASES))
def test_guides_match_the_oracle(request, mcpt_mod, oracle, case):
    fx, pos, W, H, lens, n = CASES[case]
    scene, arrays = request.getfixturevalue(fx)
    cam = mcpt_mod.make_camera(pos, -90.0, 0.0, aspect=f32(W) / f32(H), lens_radius=lens)
    pt = make_pt(mcpt_mod, scene, cam, W, H)
    pt.render_guides(n)
    g = pt.guides()
    pt.close()
    ref = oracle_guides(oracle, arrays, cam, W, H, n)
    assert_same_guides(g, ref)
    rendered = np.zeros((H, W), bool)
    rendered[:H - 1, :W - 1] = True
    assert np.all(g["count"][rendered] == n) and np.all(g["count"][~rendered] == 0)
    assert np.all(g["albedo"][~rendered] == 0) and np.all(g["depth"][~rendered] == 0)
    assert (g["depth"] > 0).any() and (g["depth"][rendered] == 0).any()  # hits and misses both occur


def test_pinhole_traces_one_sample(mcpt_mod, oracle, scene_c1):
    scene, arrays = scene_c1
    W, H = 17, 13
    cam = mcpt_mod.make_camera((0.0, 0.0, 4.0), -90.0, 0.0, aspect=f32(W) / f32(H), lens_radius=0.0)
    pt = make_pt(mcpt_mod, scene, cam, W, H)
    pt.render_guides(5)
    g = pt.guides()
    pt.close()
    assert g["count"].max() == 1 and g["count"][:H - 1, :W - 1].min() == 1
    assert_same_guides(g, oracle_guides(oracle, arrays, cam, W, H, 1))


def test_chunk_size_changes_no_bit(mcpt_mod, scene_cube):
    """Tiny chunk budgets (100 rays: seven pixel ranges, one sample per chunk; 1397 rays: one pixel
    range, the samples split 2 + 1) against the default (one chunk)."""
    W, H, n = 33, 21, 3
    cam = mcpt_mod.make_camera((0.3, 0.1, 3.0), -90.0, 0.0, aspect=f32(W) / f32(H), lens_radius=0.05)
    out = []
    for budget in (None, "6800", "95000"):
        old = os.environ.pop("MCPT_GUIDE_CHUNK_BYTES", None)
        if budget:
            os.environ["MCPT_GUIDE_CHUNK_BYTES"] = budget
        try:
            pt = make_pt(mcpt_mod, scene_cube[0], cam, W, H)
            pt.render_guides(n)
            out.append(pt.guides())
            pt.close()
        finally:
            os.environ.pop("MCPT_GUIDE_CHUNK_BYTES", None)
            if old is not None:
                os.environ["MCPT_GUIDE_CHUNK_BYTES"] = old
    assert out[0]["count"].max() == n
    assert_same_guides(out[1], out[0])
    assert_same_guides(out[2], out[0])


def test_guides_and_denoise_have_no_side_effects(mcpt_mod, scene_c2):
    """Context A interleaves the guide pass and a denoise with its render; context B only renders."""
    W, H = 64, 48
    cam = mcpt_mod.config_camera(mcpt_mod.CONFIGS[2], W, H)
    a = make_pt(mcpt_mod, scene_c2[0], cam, W, H)
    b = make_pt(mcpt_mod, scene_c2[0], cam, W, H)
    a.iterate(3)
    a.render_guides(4)
    a.denoise()
    a.render()
    b.render()
    La, sa = a.film()
    Lb, sb = b.film()
    ca, cb = a.ray_counts(), b.ray_counts()
    a.close()
    b.close()
    assert np.array_equal(La.view(np.uint32), Lb.view(np.uint32)), "films differ"
    assert np.array_equal(sa, sb) and sa.max() == 4
    assert ca == cb and ca["extension"] > 0


def test_guides_error_codes(mcpt_mod, scene_c1):
    W, H = 17, 13
    cam = mcpt_mod.make_camera((0.0, 0.0, 4.0), -90.0, 0.0, aspect=f32(W) / f32(H))
    pt = make_pt(mcpt_mod, scene_c1[0], cam, W, H)
    with pytest.raises(mcpt_mod.McptError, match="mcpt_guides_render"):
        pt.guides()
    for bad in (0, 2 ** 19 - 256):
        with pytest.raises(mcpt_mod.McptError, match="nsamples"):
            pt.render_guides(bad)
    pt.render_guides(1)
    pt.clear()  # a film clear leaves the guides valid
    assert pt.guides()["count"].max() == 1
    pt.upload_scene(scene_c1[0])  # a scene upload does not
    with pytest.raises(mcpt_mod.McptError, match="mcpt_guides_render"):
        pt.guides()
    pt.close()
