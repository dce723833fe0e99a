"""The a-trous filter's gfx950 kernels (mcpt_denoise_run, mcpt_film_denoise) against the numpy float32
restatement (tests/denoise_ref.py), bit for bit; the film path against mcpt_denoise_run fed the film's
and the guides' means; error codes; and the filter's effect on a 4-spp frame."""
import os

import numpy as np
import pytest

import denoise_ref as R

pytestmark = pytest.mark.gpu
f32 = np.float32

# the host test's shapes plus one full block row and one full block column of the kernels' tiles
SHAPES = R.SHAPES + [(256, 3), (3, 256)]
SIGMA_SETS = {
    "color": dict(R.SIGMAS_OFF, sigma_color=2.0),
    "normal": dict(R.SIGMAS_OFF, sigma_normal=0.5),
    "albedo": dict(R.SIGMAS_OFF, sigma_albedo=0.3),
    "depth": dict(R.SIGMAS_OFF, sigma_depth=0.2),
    "all": R.SIGMAS,
}


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, f32).view(np.uint32), np.ascontiguousarray(b, f32).view(np.uint32))


@pytest.fixture(scope="module")
def ctx(mcpt_mod):
    pt = mcpt_mod.PathTracer(0)  # mcpt_denoise_run needs neither a scene nor a film
    yield pt
    pt.close()


@pytest.fixture(scope="module")
def refs():
    """Inputs and numpy results per (shape, passes, sigma set), computed once."""
    cache = {}

    def get(shape, passes, which):
        key = (shape, passes, which)
        if key not in cache:
            inp = R.make_inputs(*shape)
            cache[key] = (inp, R.denoise(inp["rgb"], inp["albedo"], inp["normal"], inp["depth"], inp["samples"],
                                         passes=passes, **SIGMA_SETS[which]))
        return cache[key]

    return get


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("passes", R.PASSES)
def test_denoise_run_matches_numpy(mcpt_mod, ctx, refs, shape, passes):
    for which in SIGMA_SETS:
        inp, ref = refs(shape, passes, which)
        got = mcpt_mod.denoise_run(ctx, inp["rgb"], inp["albedo"], inp["normal"], inp["depth"], inp["samples"],
                                   passes=passes, **SIGMA_SETS[which])
        assert same_bits(got, ref), f"sigma set {which}"
    inp, _ = refs(shape, passes, "all")
    got = mcpt_mod.denoise_run(ctx, inp["rgb"], inp["albedo"], inp["normal"], inp["depth"], None, passes=passes, **R.SIGMAS)
    assert same_bits(got, R.denoise(inp["rgb"], inp["albedo"], inp["normal"], inp["depth"], None, passes=passes, **R.SIGMAS))


@pytest.mark.parametrize("lds_max", ["0", "1"])
def test_lds_and_direct_kernels_agree(mcpt_mod, ctx, refs, lds_max):
    """MCPT_DENOISE_LDS_MAX moves strides 1 and 2 from the LDS kernel to the direct one: same bits."""
    inp, ref = refs((67, 35), 3, "all")
    os.environ["MCPT_DENOISE_LDS_MAX"] = lds_max
    try:
        got = mcpt_mod.denoise_run(ctx, inp["rgb"], inp["albedo"], inp["normal"], inp["depth"], inp["samples"], passes=3,
                                   **R.SIGMAS)
    finally:
        del os.environ["MCPT_DENOISE_LDS_MAX"]
    assert same_bits(got, ref)


def make_pt(mcpt, scene, cam, W, H, spp, depth, tile=64, slots=1):
    pt = mcpt.PathTracer(0, mcpt.default_config(spp=spp, max_depth=depth, tile=tile))
    pt.upload_scene(scene)
    pt.set_camera(cam)
    pt.resize(W, H, tile, tile)
    if slots > 1:
        pt.set_path_slots(slots)
    return pt


def means(film, guides):
    """Ld / samples and guide sum / count in numpy float32, as the film path forms them."""
    Ld, smp = film
    with np.errstate(all="ignore"):
        rgb = Ld / smp[..., None].astype(f32)
        cnt = guides["count"].astype(f32)
        return rgb, guides["albedo"] / cnt[..., None], guides["normal"] / cnt[..., None], guides["depth"] / cnt, smp


FILM_CASES = {
    "c2_64x48": ("scene_c2", 2, (0.0, 0.0, 3.5), 64, 48),
    "cube_65x49": ("scene_cube", None, (0.3, 0.1, 3.0), 65, 49),
}


@pytest.mark.parametrize("slots", [1, 2])
@pytest.mark.parametrize("case", list(FILM_CASES))
def test_film_denoise_equals_denoise_run_on_the_means(request, mcpt_mod, ctx, case, slots):
    fx, cid, pos, W, H = FILM_CASES[case]
    scene = request.getfixturevalue(fx)[0]
    cam = mcpt_mod.make_camera(pos, -90.0, 0.0, aspect=f32(W) / f32(H))
    pt = make_pt(mcpt_mod, scene, cam, W, H, spp=4, depth=5, slots=slots)
    pt.render()
    pt.render_guides(4)
    pt.denoise()
    got = pt.denoised()
    rgb, al, nm, z, smp = means(pt.film(), pt.guides())
    rgba = pt.tonemap(denoised=True)
    pt.close()
    assert smp.max() == 4
    want = mcpt_mod.denoise_run(ctx, rgb, al, nm, z, smp)  # the defaults
    assert same_bits(got, want)
    assert np.all(got[smp == 0] == 0) and (got[smp > 0] > 0).any()
    # the denoised tonemap is k_tonemap's arithmetic with samples = 1
    with np.errstate(all="ignore"):
        c = got * f32(1.0)
        t = f32(255) * (c / (c + f32(1)))
    exp8 = np.where(np.isfinite(t) & (t >= 0), t, 0).astype(np.uint32).astype(np.uint8)
    assert np.array_equal(rgba[..., :3], exp8) and np.all(rgba[..., 3] == 255)


def test_error_codes_name_the_missing_step(mcpt_mod, scene_c1):
    W, H = 17, 13
    cam = mcpt_mod.make_camera((0.0, 0.0, 4.0), -90.0, 0.0, aspect=f32(W) / f32(H))
    pt = make_pt(mcpt_mod, scene_c1[0], cam, W, H, spp=1, depth=3)
    pt.render()
    with pytest.raises(mcpt_mod.McptError, match="mcpt_guides_render"):  # denoise before guides
        pt.denoise()
    with pytest.raises(mcpt_mod.McptError, match="mcpt_film_denoise"):   # denoised() before a denoise
        pt.denoised()
    with pytest.raises(mcpt_mod.McptError, match="mcpt_film_denoise"):
        pt.tonemap(denoised=True)
    pt.render_guides(1)
    for bad in (0, 9):
        with pytest.raises(mcpt_mod.McptError, match="passes"):
            pt.denoise(passes=bad)
    pt.denoise()
    assert pt.denoised().shape == (H, W, 3)
    other = mcpt_mod.make_camera((0.2, 0.0, 4.0), -90.0, 0.0, aspect=f32(W) / f32(H))
    pt.set_camera(other)  # a different camera: the guides are stale
    with pytest.raises(mcpt_mod.McptError, match="mcpt_guides_render"):
        pt.denoise()
    pt.render_guides(1)
    pt.render()
    pt.denoise()
    pt.resize(W, H, 64, 64)  # a resize drops the guides and the denoised frame
    with pytest.raises(mcpt_mod.McptError, match="mcpt_film_denoise"):
        pt.denoised()
    with pytest.raises(mcpt_mod.McptError, match="mcpt_guides_render"):
        pt.denoise()
    # no samples anywhere: all zeros, not an error
    pt.render_guides(1)
    pt.clear()
    pt.denoise()
    assert np.all(pt.denoised() == 0)
    pt.close()


def test_denoise_lowers_the_error_of_a_4spp_frame(mcpt_mod, scene_c2):
    """Config 2's proxy at 64 x 48: the default-parameter denoised 4-spp frame is closer (MSE) to the
    renderer's own 1024-spp frame than the raw 4-spp frame is.  Only pixels without samples or with a
    non-finite reference value are left out: at most the last row and column plus 1 % of the film
    (the CPU oracle's 1024-spp render of this camera has no non-finite pixel).  Measured on an MI355X:
    MSE raw 1.08389e-4, denoised 2.86204e-5, ratio 0.2641, 111 pixels excluded."""
    W, H = 64, 48
    rc = mcpt_mod.CONFIGS[2]
    cam = mcpt_mod.config_camera(rc, W, H)
    ref_pt = make_pt(mcpt_mod, scene_c2[0], cam, W, H, spp=1024, depth=rc.max_depth)
    ref_pt.render()
    Lr, sr = ref_pt.film()
    ref_pt.close()
    pt = make_pt(mcpt_mod, scene_c2[0], cam, W, H, spp=4, depth=rc.max_depth)
    pt.render()
    pt.render_guides(4)
    pt.denoise()
    den = pt.denoised()
    Ln, sn = pt.film()
    pt.close()
    with np.errstate(all="ignore"):
        ref = Lr / sr[..., None].astype(f32)
        raw = Ln / sn[..., None].astype(f32)
    keep = (sn > 0) & (sr > 0) & np.isfinite(ref).all(axis=2)
    excluded = int((~keep).sum())
    assert excluded <= (W + H - 1) + W * H // 100, excluded
    mse_raw = float(np.mean((raw[keep].astype(np.float64) - ref[keep]) ** 2))
    mse_den = float(np.mean((den[keep].astype(np.float64) - ref[keep]) ** 2))
    print(f"config 2, 64x48, 4 spp against 1024 spp: MSE raw {mse_raw:.6g}, denoised {mse_den:.6g}, "
          f"ratio {mse_den / mse_raw:.4f}; {excluded} pixels excluded")
    assert np.isfinite(mse_raw) and mse_den < mse_raw
