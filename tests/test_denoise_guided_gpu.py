"""The variance-guided a-trous filter's gfx950 kernels (mcpt_denoise_guided_run,
mcpt_film_denoise_guided) against the numpy float32 restatement (tests/denoise_guided_ref.py), bit for
bit in colour and variance; the film path against mcpt_denoise_guided_run fed the film's means, the
guides' means and the squared standard error; scattered-in pixels; side effects; error codes; and the
filter's effect on an 8-spp frame."""
import ctypes as C
import os

import numpy as np
import pytest

import denoise_guided_ref as G
import denoise_ref as R

pytestmark = pytest.mark.gpu
f32 = np.float32

SHAPES = R.SHAPES + [(256, 3), (3, 256)]
PAR = dict(R.SIGMAS, **G.GUIDED)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, f32).view(np.uint32), np.ascontiguousarray(b, f32).view(np.uint32))


@pytest.fixture(scope="module")
def ctx(mcpt_mod):
    pt = mcpt_mod.PathTracer(0)  # mcpt_denoise_guided_run needs neither a scene nor a film
    yield pt
    pt.close()


@pytest.fixture(scope="module")
def refs():
    """Inputs and numpy results per (shape, passes), computed once."""
    cache = {}

    def get(shape, passes):
        key = (shape, passes)
        if key not in cache:
            inp = G.make_inputs(*shape)
            cache[key] = (inp, G.denoise_guided(inp["rgb"], inp["variance"], inp["albedo"], inp["normal"], inp["depth"],
                                                inp["samples"], passes=passes, **PAR))
        return cache[key]

    return get


def run(mcpt, ctx, inp, samples="own", **kw):
    sm = inp["samples"] if isinstance(samples, str) else samples
    return mcpt.denoise_guided_run(ctx, inp["rgb"], inp["variance"], inp["albedo"], inp["normal"], inp["depth"], sm, **kw)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("passes", R.PASSES)
def test_denoise_guided_run_matches_numpy(mcpt_mod, ctx, refs, shape, passes):
    inp, (ref, ref_v) = refs(shape, passes)
    got, got_v = run(mcpt_mod, ctx, inp, passes=passes, **PAR)
    assert same_bits(got, ref), "colour"
    assert same_bits(got_v, ref_v), "variance"


@pytest.mark.parametrize("lds_max", ["0", "1"])
def test_lds_and_direct_kernels_agree(mcpt_mod, ctx, refs, lds_max):
    """MCPT_DENOISE_LDS_MAX moves strides 1 and 2 from the LDS kernel to the direct one: same bits."""
    inp, (ref, ref_v) = refs((67, 35), 3)
    os.environ["MCPT_DENOISE_LDS_MAX"] = lds_max
    try:
        got, got_v = run(mcpt_mod, ctx, inp, passes=3, **PAR)
    finally:
        del os.environ["MCPT_DENOISE_LDS_MAX"]
    assert same_bits(got, ref) and same_bits(got_v, ref_v)


def test_without_a_variance_it_is_the_plain_filter(mcpt_mod, ctx):
    """(a) every variance unknown: mcpt_denoise_run's colours, bit for bit, and no variance."""
    inp = G.make_inputs(67, 35)
    inp["variance"] = np.full((35, 67), -1.0, f32)
    got, got_v = run(mcpt_mod, ctx, inp, passes=3, **PAR)
    want = mcpt_mod.denoise_run(ctx, inp["rgb"], inp["albedo"], inp["normal"], inp["depth"], inp["samples"], passes=3,
                                **R.SIGMAS)
    assert same_bits(got, want) and np.all(got_v == -1)


@pytest.mark.parametrize("k", [-7, 5])
def test_power_of_two_scaling_is_exact_without_eps(mcpt_mod, ctx, k):
    """(b) lum_eps = 0, every variance known: colours x 2^k and variances x 4^k scale the outputs exactly."""
    inp = G.make_inputs(67, 35)
    with np.errstate(all="ignore"):
        inp["variance"] = np.where(inp["variance"] >= 0, inp["variance"], f32(1.5)).astype(f32)  # the zeros stay
    assert (inp["variance"] == 0).any()
    par = dict(PAR, lum_eps=0.0)
    base, base_v = run(mcpt_mod, ctx, inp, passes=3, **par)
    sc = dict(inp, rgb=(inp["rgb"] * f32(2.0 ** k)).astype(f32), variance=(inp["variance"] * f32(4.0 ** k)).astype(f32))
    got, got_v = run(mcpt_mod, ctx, sc, passes=3, **par)
    assert same_bits(got, base * f32(2.0 ** k))
    assert same_bits(got_v, np.where(base_v >= 0, base_v * f32(4.0 ** k), f32(-1)))
    valid = R.planes(inp["rgb"], inp["samples"], inp["normal"], inp["albedo"], inp["depth"])[1]
    assert np.all(np.isfinite(base_v[valid]) & (base_v[valid] >= 0)) and np.all(base_v[~valid] == -1)  # (c)


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


def variance_of(err):
    """The film path's variance input: se^2, -1 where there is no estimate."""
    se = err[..., 0]
    with np.errstate(all="ignore"):
        return np.where(se < 0, f32(-1), se * se).astype(f32)


FILM_CASES = {
    "c2_64x48": ("scene_c2", (0.0, 0.0, 3.5), 64, 48),
    "cube_65x49": ("scene_cube", (0.3, 0.1, 3.0), 65, 49),
}


@pytest.mark.parametrize("slots", [2, 3])
@pytest.mark.parametrize("case", list(FILM_CASES))
def test_film_denoise_guided_equals_the_run_on_the_means(request, mcpt_mod, ctx, case, slots):
    fx, pos, W, H = FILM_CASES[case]
    scene = request.getfixturevalue(fx)[0]
    cam = mcpt_mod.make_camera(pos, -90.0, 0.0, aspect=f32(W) / f32(H))
    pt = make_pt(mcpt_mod, scene, cam, W, H, spp=8, depth=5, slots=slots)
    pt.render()
    pt.render_guides(4)
    pt.denoise_guided()
    got, got_v = pt.denoised(), pt.denoised_variance()
    rgba = pt.tonemap(denoised=True)
    rgb, al, nm, z, smp = means(pt.film(), pt.guides())
    var = variance_of(pt.film_error())
    pt.close()
    assert smp.max() == 8 and (var >= 0).any()
    want, want_v = mcpt_mod.denoise_guided_run(ctx, rgb, var, al, nm, z, smp)  # the defaults
    assert same_bits(got, want) and same_bits(got_v, want_v)
    assert np.all(got[smp == 0] == 0) and np.all(got_v[smp == 0] == -1) and (got_v >= 0).any()
    # the denoised tonemap is k_tonemap's arithmetic with samples = 1
    with np.errstate(all="ignore"):
        c = got * f32(1.0)
        t = f32(255) * (c / (c + f32(1)))
    exp8 = np.where(np.isfinite(t) & (t >= 0), t, 0).astype(np.uint32).astype(np.uint8)
    assert np.array_equal(rgba[..., :3], exp8) and np.all(rgba[..., 3] == 255)


def loaded_hip_runtime():
    """The HIP runtime libmcpt.so runs on, for a device buffer: the copy already mapped into the process
    (opening libamdhip64 by a path of our own could load a second runtime beside it)."""
    with open("/proc/self/maps") as f:
        paths = sorted({line.split()[-1] for line in f if "libamdhip64" in line})
    assert len(paths) == 1, paths
    hip = C.CDLL(paths[0])
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    return hip


def test_scattered_in_pixels_take_the_plain_term(mcpt_mod, ctx, scene_c2):
    """Two contexts with complementary tile sets; B's packed tiles unpacked into A.  A has no slot
    accumulators for B's pixels (K = 0), so they enter the filter without a variance."""
    hip = loaded_hip_runtime()
    W, H, T = 64, 48, 16
    rc = mcpt_mod.CONFIGS[2]
    cam = mcpt_mod.config_camera(rc, W, H)
    every = [(tx, ty) for ty in range(H // T) for tx in range(W // T)]
    mine = [t for i, t in enumerate(every) if i % 2 == 0]
    theirs = [t for t in every if t not in mine]
    pts = []
    for tiles in (mine, theirs):
        pt = make_pt(mcpt_mod, scene_c2[0], cam, W, H, 4, 5, tile=T)
        pt.set_compact_paths(True)
        pt.set_path_slots(2)
        pt.set_tiles(tiles)
        pt.render()
        pts.append(pt)
    a, b = pts
    lib = mcpt_mod.lib()
    n = C.c_uint32()
    assert lib.mcpt_film_pack_tiles(b.h, None, C.byref(n)) == 0 and n.value == len(theirs) * T * T
    buf = C.c_void_p()
    assert hip.hipMalloc(C.byref(buf), C.c_size_t(n.value * 16)) == 0
    assert lib.mcpt_film_pack_tiles(b.h, buf, C.byref(n)) == 0
    xy = np.ascontiguousarray(theirs, np.uint32).reshape(-1, 2)
    assert lib.mcpt_film_unpack_tiles(a.h, buf, xy.ctypes.data_as(C.POINTER(C.c_uint32)), len(theirs)) == 0
    assert lib.mcpt_sync(a.h) == 0 and hip.hipFree(buf) == 0
    a.render_guides(2)
    a.denoise_guided()
    got, got_v = a.denoised(), a.denoised_variance()
    rgb, al, nm, z, smp = means(a.film(), a.guides())
    err = a.film_error()
    for pt in pts:
        pt.close()
    foreign = np.zeros((H, W), bool)
    for tx, ty in theirs:
        foreign[ty * T:(ty + 1) * T, tx * T:(tx + 1) * T] = True
    assert smp[foreign].max() == 4 and np.all(err[foreign][:, 0] == -1) and np.all(err[foreign][:, 2] == 0)
    var = variance_of(err)
    assert np.all(var[foreign] == -1) and (var[~foreign] >= 0).any()
    want, want_v = mcpt_mod.denoise_guided_run(ctx, rgb, var, al, nm, z, smp)
    assert same_bits(got, want) and same_bits(got_v, want_v)
    assert np.all(got_v[foreign] == -1) and (got[foreign] > 0).any()


def test_no_side_effects_on_the_render_and_the_plain_filter(mcpt_mod, scene_c2):
    """Guides and a guided denoise between two halves of a render change nothing the render produces;
    a guided call between two plain denoises of the same film does not change their result."""
    W, H = 64, 48
    rc = mcpt_mod.CONFIGS[2]
    cam = mcpt_mod.config_camera(rc, W, H)
    out = []
    for interleave in (False, True):
        pt = make_pt(mcpt_mod, scene_c2[0], cam, W, H, spp=2, depth=rc.max_depth, slots=2)
        pt.render()
        if interleave:
            pt.render_guides(2)
            pt.denoise_guided()
        pt.set_spp(4)
        pt.render()
        out.append((pt.film(), pt.ray_counts()))
        if interleave:
            pt.denoise()
            d1 = pt.denoised()
            pt.denoise_guided()
            g1 = pt.denoised()
            pt.denoise()
            d2 = pt.denoised()
            assert same_bits(d1, d2) and not same_bits(d1, g1)
        pt.close()
    (f0, r0), (f1, r1) = out
    assert np.array_equal(f0[0].view(np.uint32), f1[0].view(np.uint32)) and np.array_equal(f0[1], f1[1])
    assert f0[1].max() == 4 and r0 == r1 and r0["extension"] > 0


def test_error_codes_name_the_missing_step(mcpt_mod, scene_c1):
    W, H = 17, 13
    cam = mcpt_mod.make_camera((0.0, 0.0, 4.0), -90.0, 0.0, aspect=f32(W) / f32(H))
    pt = make_pt(mcpt_mod, scene_c1[0], cam, W, H, spp=2, depth=3)
    pt.render()
    with pytest.raises(mcpt_mod.McptError, match="mcpt_guides_render"):  # before guides
        pt.denoise_guided()
    pt.render_guides(1)
    with pytest.raises(mcpt_mod.McptError, match="mcpt error -1.*2 path slots"):  # one path slot
        pt.denoise_guided()
    pt.set_path_slots(2)  # (re-allocates the film: the guides go with it)
    pt.render()
    with pytest.raises(mcpt_mod.McptError, match="mcpt_guides_render"):
        pt.denoise_guided()
    pt.render_guides(1)
    for kw, what in ((dict(passes=0), "passes"), (dict(passes=9), "passes"), (dict(sigma_lum=0.0), "sigma_lum"),
                     (dict(sigma_lum=-1.0), "sigma_lum"), (dict(sigma_lum=float("nan")), "sigma_lum"),
                     (dict(lum_eps=-1e-3), "lum_eps")):
        with pytest.raises(mcpt_mod.McptError, match="mcpt error -1.*" + what):
            pt.denoise_guided(**kw)
    pt.denoise()
    with pytest.raises(mcpt_mod.McptError, match="mcpt error -1.*mcpt_film_denoise_guided"):  # variance of a plain denoise
        pt.denoised_variance()
    pt.denoise_guided()
    assert pt.denoised().shape == (H, W, 3) and pt.denoised_variance().shape == (H, W)
    pt.denoise(passes=1)  # ... and again after a plain one follows a guided one
    with pytest.raises(mcpt_mod.McptError, match="mcpt_film_denoise_guided"):
        pt.denoised_variance()
    # paths in flight
    pt.clear()
    assert pt.iterate(1).live_paths > 0
    with pytest.raises(mcpt_mod.McptError, match="mcpt error -1.*in flight"):
        pt.denoise_guided()
    pt.render()
    pt.denoise_guided()
    other = mcpt_mod.make_camera((0.2, 0.0, 4.0), -90.0, 0.0, aspect=f32(W) / f32(H))
    pt.set_camera(other)  # a different camera: the guides are stale
    pt.render()
    with pytest.raises(mcpt_mod.McptError, match="mcpt_guides_render"):
        pt.denoise_guided()
    pt.render_guides(1)
    pt.denoise_guided()
    pt.resize(W, H, 64, 64)  # a resize drops the guides, the denoised frame and its variance
    with pytest.raises(mcpt_mod.McptError, match="mcpt_film_denoise"):
        pt.denoised_variance()
    with pytest.raises(mcpt_mod.McptError, match="mcpt_film_denoise"):
        pt.denoised()
    with pytest.raises(mcpt_mod.McptError, match="mcpt_guides_render"):
        pt.denoise_guided()
    # the run's own argument checks
    inp = G.make_inputs(5, 3)
    with pytest.raises(mcpt_mod.McptError, match="sigma_lum"):
        run(mcpt_mod, pt, inp, sigma_lum=0.0)
    pt.close()


def test_a_refused_guided_call_keeps_the_plain_result(mcpt_mod, scene_c1):
    """Both forms share the context's planes.  A guided call that is refused (bad parameters, paths in
    flight) comes back before it touches them: the plain result stays readable, bit for bit, and the
    guided call that succeeds afterwards gets its variance planes then."""
    W, H = 17, 13
    cam = mcpt_mod.make_camera((0.0, 0.0, 4.0), -90.0, 0.0, aspect=f32(W) / f32(H))
    pt = make_pt(mcpt_mod, scene_c1[0], cam, W, H, spp=2, depth=3, slots=2)
    pt.render()
    pt.render_guides(1)
    pt.denoise()
    d1 = pt.denoised()
    with pytest.raises(mcpt_mod.McptError, match="passes"):
        pt.denoise_guided(passes=0)
    assert same_bits(pt.denoised(), d1)
    pt.clear()
    assert pt.iterate(1).live_paths > 0
    with pytest.raises(mcpt_mod.McptError, match="in flight"):
        pt.denoise_guided()
    assert same_bits(pt.denoised(), d1)
    pt.render()
    pt.denoise_guided()
    assert pt.denoised_variance().shape == (H, W) and pt.denoised().shape == (H, W, 3)
    pt.close()


def test_guided_denoise_beats_the_plain_one_on_an_8spp_frame(mcpt_mod, scene_c2):
    """Config 2's proxy at 64 x 48, 8 spp in 4 path slots, 4 guide samples, against the renderer's own
    1024-spp frame: MSE(guided) < MSE(plain filter at its defaults) < MSE(raw), with the guided filter
    at sigma_lum = 4, lum_eps = 1e-4 (the prototype's row) and again at its defaults.  Only pixels without samples or with a non-finite reference value are left out: at most
    the last row and column plus 1 % of the film.  A numpy prototype on the CPU oracle's frames gave
    4.01e-6 / 2.80e-5 / 5.41e-5 (111 pixels excluded).  Measured on an MI355X: MSE raw 5.40655e-5, plain
    2.79992e-5, guided 4.01389e-6, 111 pixels excluded."""
    W, H = 64, 48
    rc = mcpt_mod.CONFIGS[2]
    cam = mcpt_mod.config_camera(rc, W, H)
    ref_pt = make_pt(mcpt_mod, scene_c2[0], cam, W, H, spp=1024, depth=rc.max_depth)
    ref_pt.render()
    Lr, sr = ref_pt.film()
    ref_pt.close()
    pt = make_pt(mcpt_mod, scene_c2[0], cam, W, H, spp=8, depth=rc.max_depth, slots=4)
    pt.render()
    pt.render_guides(4)
    pt.denoise()
    plain = pt.denoised()
    pt.denoise_guided(**G.GUIDED)
    guided = pt.denoised()
    pt.denoise_guided()
    guided_def = pt.denoised()
    Ln, sn = pt.film()
    pt.close()
    with np.errstate(all="ignore"):
        ref = Lr / sr[..., None].astype(f32)
        raw = Ln / sn[..., None].astype(f32)
    keep = (sn > 0) & (sr > 0) & np.isfinite(ref).all(axis=2)
    excluded = int((~keep).sum())
    assert excluded <= (W + H - 1) + W * H // 100, excluded
    mse_raw, mse_plain, mse_guided, mse_def = (float(np.mean((im[keep].astype(np.float64) - ref[keep]) ** 2))
                                               for im in (raw, plain, guided, guided_def))
    print(f"config 2, 64x48, 8 spp / 4 slots against 1024 spp: MSE raw {mse_raw:.6g}, plain {mse_plain:.6g}, "
          f"guided {mse_guided:.6g}, guided at the defaults {mse_def:.6g}; {excluded} pixels excluded")
    assert np.isfinite(mse_raw) and mse_guided < mse_plain < mse_raw
    assert mse_def < mse_plain
