"""The spatial variance estimate's gfx950 kernel (mcpt_variance_run, mcpt_set_variance_fill) against the
numpy float32 restatement (tests/variance_ref.py), bit for bit; fill-only and exactness properties; the
film paths (mcpt_film_denoise_guided, mcpt_film_temporal) with the fill on against the host-image runs
composed with mcpt_variance_run; scattered-in pixels; off is off; error codes; side effects; and the
effect on one-slot frames."""
import ctypes as C

import numpy as np
import pytest

import denoise_guided_ref as G
import denoise_ref as R
import temporal_ref as T
import variance_ref as V

pytestmark = pytest.mark.gpu
f32 = np.float32

SHAPES = R.SHAPES + [(256, 3), (3, 256)]


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, f32).view(np.uint32), np.ascontiguousarray(b, f32).view(np.uint32))


@pytest.fixture(scope="module")
def ctx(mcpt_mod):
    pt = mcpt_mod.PathTracer(0)  # mcpt_variance_run needs neither a scene nor a film
    yield pt
    pt.close()


def run(mcpt, ctx, inp, known=False, **kw):
    return mcpt.variance_run(ctx, inp["rgb"], inp["albedo"], inp["normal"], inp["depth"], inp["samples"],
                             inp["variance"] if known else None, **kw)


def valid_of(inp):
    return R.planes(inp["rgb"], inp["samples"], inp["normal"], inp["albedo"], inp["depth"])[1]


# ---- 1 .. 3: the kernel against numpy, fill only, exactness ----

@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("radius", V.RADII)
def test_variance_run_matches_numpy(mcpt_mod, ctx, shape, radius):
    """67 x 35 crosses the 32 x 16 tile borders with every halo width."""
    inp = G.make_inputs(*shape)
    got = run(mcpt_mod, ctx, inp, radius=radius, **V.PARAMS)
    assert same_bits(got, V.run_ref(inp, radius=radius, **V.PARAMS))
    assert ctx.variance_ms() > 0


@pytest.mark.parametrize("radius", V.RADII)
def test_fill_only(mcpt_mod, ctx, radius):
    """Known inputs are returned unchanged, invalid pixels give -1, a known result is finite and >= 0,
    and what is filled does not depend on the neighbours' variances."""
    inp = G.make_inputs(67, 35)
    got = run(mcpt_mod, ctx, inp, known=True, radius=radius, **V.PARAMS)
    assert same_bits(got, V.run_ref(inp, known=True, radius=radius, **V.PARAMS))
    valid = valid_of(inp)
    with np.errstate(all="ignore"):
        known = valid & (inp["variance"] >= 0) & (inp["variance"] <= R.FLT_MAX)
    assert known.any() and (valid & ~known).any()
    assert same_bits(got[known], inp["variance"][known])
    assert np.all(got[~valid] == -1)
    assert np.all((got == -1) | (np.isfinite(got) & (got >= 0)))
    alone = run(mcpt_mod, ctx, inp, radius=radius, **V.PARAMS)
    assert same_bits(got[~known], alone[~known]) and (alone[valid] >= 0).sum() > valid.sum() // 2


def test_a_constant_image_has_variance_zero(mcpt_mod, ctx):
    inp = G.make_inputs(67, 35)
    valid = valid_of(inp)
    inp["rgb"] = np.where(valid[..., None], f32([0.7, 1.3, 0.2]), inp["rgb"]).astype(f32)
    for radius in V.RADII:
        got = run(mcpt_mod, ctx, inp, radius=radius, **V.PARAMS)
        assert np.all((got == 0) | (got == -1)) and (got == 0).sum() > valid.sum() // 2 and np.all(got[~valid] == -1)


@pytest.mark.parametrize("k", [-7, 5])
def test_power_of_two_scaling_is_exact(mcpt_mod, ctx, k):
    """rgb x 2^k gives variances x 4^k, bit for bit."""
    inp = G.make_inputs(67, 35)
    base = run(mcpt_mod, ctx, inp, radius=3, **V.PARAMS)
    sc = dict(inp, rgb=(inp["rgb"] * f32(2.0 ** k)).astype(f32))
    got = run(mcpt_mod, ctx, sc, radius=3, **V.PARAMS)
    assert (base > 0).any() and same_bits(got, np.where(base >= 0, base * f32(4.0 ** k), f32(-1)))


# ---- 4 .. 6: the film paths ----

def make_pt(mcpt, scene, cam, W, H, spp, depth, tile=64, slots=1, seed=0x5EED2026):
    pt = mcpt.PathTracer(0, mcpt.default_config(spp=spp, max_depth=depth, tile=tile, seed=seed))
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
    se = err[..., 0]
    with np.errstate(all="ignore"):
        return np.where(se < 0, f32(-1), se * se).astype(f32)


FILM_CASES = {
    "c2_64x48": ("scene_c2", (0.0, 0.0, 3.5), 64, 48),
    "cube_65x49": ("scene_cube", (0.3, 0.1, 3.0), 65, 49),
}


@pytest.mark.parametrize("case", list(FILM_CASES))
def test_one_slot_film_denoise_guided_equals_the_runs_on_the_means(request, mcpt_mod, ctx, case):
    """8 spp in one path slot, fill on: denoise_guided() equals denoise_guided_run fed variance_run's
    output on the film's and the guides' means."""
    fx, pos, W, H = FILM_CASES[case]
    scene = request.getfixturevalue(fx)[0]
    cam = mcpt_mod.make_camera(pos, -90.0, 0.0, aspect=f32(W) / f32(H))
    pt = make_pt(mcpt_mod, scene, cam, W, H, spp=8, depth=5)
    pt.set_variance_fill()
    pt.render()
    pt.render_guides(4)
    pt.denoise_guided()
    got, got_v = pt.denoised(), pt.denoised_variance()
    ms = pt.variance_ms()
    rgb, al, nm, z, smp = means(pt.film(), pt.guides())
    pt.close()
    var = mcpt_mod.variance_run(ctx, rgb, al, nm, z, smp)  # the defaults, nothing known
    assert smp.max() == 8 and (var >= 0).sum() > W * H // 2 and ms > 0
    want, want_v = mcpt_mod.denoise_guided_run(ctx, rgb, var, al, nm, z, smp)
    assert same_bits(got, want) and same_bits(got_v, want_v)
    assert np.all(got_v[smp == 0] == -1) and (got_v >= 0).any()


@pytest.mark.parametrize("case", list(FILM_CASES))
def test_with_slot_estimates_everywhere_the_fill_changes_nothing(request, mcpt_mod, case):
    """8 spp in 2 slots: every pixel with samples has a slot estimate, so fill on and off agree bit for bit."""
    fx, pos, W, H = FILM_CASES[case]
    scene = request.getfixturevalue(fx)[0]
    cam = mcpt_mod.make_camera(pos, -90.0, 0.0, aspect=f32(W) / f32(H))
    pt = make_pt(mcpt_mod, scene, cam, W, H, spp=8, depth=5, slots=2)
    pt.render()
    pt.render_guides(4)
    out = []
    for on in (False, True):
        if on:
            pt.set_variance_fill()
        pt.denoise_guided()
        out.append((pt.denoised(), pt.denoised_variance()))
    rgb, _, _, _, smp = means(pt.film(), pt.guides())
    var = variance_of(pt.film_error())
    pt.close()
    valid = (smp > 0) & np.isfinite(rgb).all(axis=2)
    assert valid.sum() > W * H // 2 and np.all(var[valid] >= 0)
    assert same_bits(out[0][0], out[1][0]) and same_bits(out[0][1], out[1][1])


def loaded_hip_runtime():
    """The HIP runtime libmcpt.so runs on, for a device buffer: the copy already mapped into the process."""
    with open("/proc/self/maps") as f:
        paths = sorted({line.split()[-1] for line in f if "libamdhip64" in line})
    assert len(paths) == 1, paths
    hip = C.CDLL(paths[0])
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    return hip


def test_scattered_in_pixels_get_the_estimate(mcpt_mod, ctx, scene_c2):
    """Two contexts with complementary tile sets; B's packed tiles unpacked into A.  A has no slot
    accumulators for B's pixels: with the fill on they carry the spatial estimate, A's own keep se^2."""
    hip = loaded_hip_runtime()
    W, H, T_ = 64, 48, 16
    rc = mcpt_mod.CONFIGS[2]
    cam = mcpt_mod.config_camera(rc, W, H)
    every = [(tx, ty) for ty in range(H // T_) for tx in range(W // T_)]
    mine = [t for i, t in enumerate(every) if i % 2 == 0]
    theirs = [t for t in every if t not in mine]
    pts = []
    for tiles in (mine, theirs):
        pt = make_pt(mcpt_mod, scene_c2[0], cam, W, H, 4, 5, tile=T_)
        pt.set_compact_paths(True)
        pt.set_path_slots(2)
        pt.set_tiles(tiles)
        pt.render()
        pts.append(pt)
    a, b = pts
    lib = mcpt_mod.lib()
    n = C.c_uint32()
    assert lib.mcpt_film_pack_tiles(b.h, None, C.byref(n)) == 0 and n.value == len(theirs) * T_ * T_
    buf = C.c_void_p()
    assert hip.hipMalloc(C.byref(buf), C.c_size_t(n.value * 16)) == 0
    assert lib.mcpt_film_pack_tiles(b.h, buf, C.byref(n)) == 0
    xy = np.ascontiguousarray(theirs, np.uint32).reshape(-1, 2)
    assert lib.mcpt_film_unpack_tiles(a.h, buf, xy.ctypes.data_as(C.POINTER(C.c_uint32)), len(theirs)) == 0
    assert lib.mcpt_sync(a.h) == 0 and hip.hipFree(buf) == 0
    a.render_guides(2)
    a.set_variance_fill()
    a.denoise_guided()
    got, got_v = a.denoised(), a.denoised_variance()
    rgb, al, nm, z, smp = means(a.film(), a.guides())
    err = a.film_error()
    for pt in pts:
        pt.close()
    foreign = np.zeros((H, W), bool)
    for tx, ty in theirs:
        foreign[ty * T_:(ty + 1) * T_, tx * T_:(tx + 1) * T_] = True
    var = variance_of(err)
    assert smp[foreign].max() == 4 and np.all(var[foreign] == -1) and (var[~foreign] >= 0).any()
    filled = mcpt_mod.variance_run(ctx, rgb, al, nm, z, smp, var)  # where(se known, se^2, the estimate)
    assert same_bits(filled[var >= 0], var[var >= 0])
    want, want_v = mcpt_mod.denoise_guided_run(ctx, rgb, filled, al, nm, z, smp)
    assert same_bits(got, want) and same_bits(got_v, want_v)
    has = foreign & (smp > 0)
    assert (filled[has] >= 0).sum() > 0.9 * has.sum() and np.all(got_v[has & (filled >= 0)] >= 0)


def frame_seed(k):
    return (0x9E3779B97F4A7C15 * (k + 1)) & (2 ** 64 - 1)


def frame(pt, cam, k, guides=2):
    pt.set_camera(cam)
    pt.set_seed(frame_seed(k))
    pt.render()
    pt.render_guides(guides)


def yawed(mcpt, rc, W, H, yaw_off, **kw):
    return mcpt.make_camera(rc.position, rc.yaw + yaw_off, rc.pitch, rc.fovy, aspect=f32(W) / f32(H), **kw)


@pytest.mark.parametrize("cid", [1, 2])
def test_one_slot_temporal_film_path_equals_the_runs_on_the_means(request, mcpt_mod, ctx, cid):
    """Three one-slot 2-spp frames, yawed and reseeded, fill on: each temporal() equals mcpt_temporal_run
    fed that frame's means with mcpt_variance_run's variance and the previous call's planes."""
    W, H = 64, 48
    rc = mcpt_mod.CONFIGS[cid]
    scene = request.getfixturevalue(f"scene_c{cid}")[0]
    cams = [yawed(mcpt_mod, rc, W, H, 1.5 * f) for f in range(3)]
    pt = make_pt(mcpt_mod, scene, cams[0], W, H, spp=2, depth=rc.max_depth)
    pt.set_variance_fill()
    hist, vp_prev = T.empty_history(W, H), mcpt_mod.camera_view_proj(cams[0])
    for f, cam in enumerate(cams):
        frame(pt, cam, 100 + f)
        pt.temporal_accumulate(**T.PARAMS)
        t = pt.temporal()
        rgb, al, nm, z, smp = means(pt.film(), pt.guides())
        var = mcpt_mod.variance_run(ctx, rgb, al, nm, z, smp)
        assert smp.max() == 2 and (var >= 0).sum() > W * H // 8
        col, vl, hcol, hpos, hnrm = mcpt_mod.temporal_run(ctx, rgb, smp, var, t["position"], nm, z, *hist, vp_prev, **T.PARAMS)
        assert same_bits(hcol[..., :3], t["rgb"]) and same_bits(hcol[..., 3], t["nsamples"]), f"frame {f}: colour"
        assert same_bits(hpos[..., 3], t["variance"]) and same_bits(hpos[..., :3], t["position"]), f"frame {f}: variance"
        assert (t["variance"] >= 0).any()
        hist, vp_prev = (hcol, hpos, hnrm), mcpt_mod.camera_view_proj(cam)
    with pytest.raises(mcpt_mod.McptError, match="mcpt_film_denoise"):  # the accumulation used the filter's planes
        pt.denoised()
    pt.temporal_denoise()
    assert (pt.denoised_variance() >= 0).any()
    pt.close()


# ---- 7 .. 9: off is off, error codes, side effects ----

def test_off_is_off_and_the_setting_survives(mcpt_mod, scene_c1):
    W, H = 33, 21
    rc = mcpt_mod.CONFIGS[1]
    pt = make_pt(mcpt_mod, scene_c1[0], yawed(mcpt_mod, rc, W, H, 0.0), W, H, spp=2, depth=3)

    def off_checks():
        pt.render()
        pt.render_guides(1)
        with pytest.raises(mcpt_mod.McptError, match="mcpt error -1.*2 path slots"):
            pt.denoise_guided()
        pt.temporal_accumulate()
        assert np.all(pt.temporal()["variance"] == -1)

    off_checks()  # before the first set_variance_fill
    pt.set_variance_fill(radius=1)
    pt.denoise_guided()
    assert (pt.denoised_variance() >= 0).any()
    pt.temporal_accumulate()
    assert (pt.temporal()["variance"] >= 0).any()
    pt.set_variance_fill(None)
    pt.temporal_reset()
    off_checks()  # ... and again after it is turned off
    # the setting survives a film clear, a seed change, a slot change and a resize
    pt.set_variance_fill()
    pt.clear()
    pt.set_seed(77)
    pt.set_path_slots(2)
    pt.set_path_slots(1)
    pt.resize(W + 1, H + 2, 64, 64)
    pt.render()
    pt.render_guides(1)
    pt.denoise_guided()
    assert (pt.denoised_variance() >= 0).any()
    pt.close()


def test_error_codes_name_the_parameter(mcpt_mod, ctx, scene_c1):
    W, H = 17, 13
    cam = mcpt_mod.make_camera((0.0, 0.0, 4.0), -90.0, 0.0, aspect=f32(W) / f32(H))
    pt = make_pt(mcpt_mod, scene_c1[0], cam, W, H, spp=2, depth=3)
    pt.render()
    pt.render_guides(1)
    pt.set_variance_fill(radius=1)
    pt.denoise_guided()
    d1, v1 = pt.denoised(), pt.denoised_variance()
    bad = ((dict(radius=0), "radius"), (dict(radius=4), "radius"), (dict(sigma_normal=float("nan")), "sigma_normal"),
           (dict(sigma_albedo=float("inf")), "sigma_albedo"), (dict(sigma_depth=float("-inf")), "sigma_depth"),
           (dict(min_neff=0.5), "min_neff"), (dict(min_neff=float("nan")), "min_neff"), (dict(min_neff=float("inf")), "min_neff"))
    inp = G.make_inputs(5, 3)
    for kw, what in bad:
        with pytest.raises(mcpt_mod.McptError, match="mcpt error -1.*" + what):
            pt.set_variance_fill(**kw)
        with pytest.raises(mcpt_mod.McptError, match="mcpt error -1.*" + what):
            run(mcpt_mod, ctx, inp, **kw)
    assert same_bits(pt.denoised(), d1)  # the refused calls touched nothing
    pt.denoise_guided()  # ... and left the previous setting (radius 1) in place
    assert same_bits(pt.denoised(), d1) and same_bits(pt.denoised_variance(), v1)
    pt.set_variance_fill(radius=3, sigma_normal=-1.0, sigma_albedo=0.0)  # sigma <= 0 turns a term off
    pt.denoise_guided()
    assert not same_bits(pt.denoised_variance(), v1)
    lib = mcpt_mod.lib()
    assert lib.mcpt_variance_default_params(None) == -1 and lib.mcpt_set_variance_fill(None, None) == -1
    assert lib.mcpt_debug_variance_ms(None, None) == -1
    assert lib.mcpt_variance_run(pt.h, 2, 2, *([None] * 8)) == -1 and b"null" in lib.mcpt_last_error(pt.h)
    # paths in flight with one slot: refused, and the previous denoised result stays readable
    pt.denoise_guided()
    d2 = pt.denoised()
    pt.clear()
    assert pt.iterate(1).live_paths > 0
    with pytest.raises(mcpt_mod.McptError, match="mcpt error -1.*in flight"):
        pt.denoise_guided()
    with pytest.raises(mcpt_mod.McptError, match="mcpt error -1.*in flight"):
        pt.temporal_accumulate()
    assert same_bits(pt.denoised(), d2)
    with pytest.raises(mcpt_mod.McptError, match="passes"):
        pt.denoise_guided(passes=0)
    assert same_bits(pt.denoised(), d2)
    pt.render()
    pt.denoise_guided()
    pt.close()


def test_no_side_effects_on_the_render(mcpt_mod, scene_c2):
    """A fill-on guided denoise and accumulation between two halves of a one-slot render change nothing
    the render produces."""
    W, H = 64, 48
    rc = mcpt_mod.CONFIGS[2]
    cam = mcpt_mod.config_camera(rc, W, H)
    out = []
    for interleave in (False, True):
        pt = make_pt(mcpt_mod, scene_c2[0], cam, W, H, spp=2, depth=rc.max_depth)
        pt.render()
        if interleave:
            pt.set_variance_fill()
            pt.render_guides(2)
            pt.denoise_guided()
            pt.temporal_accumulate()
        pt.set_spp(4)
        pt.render()
        out.append((pt.film(), pt.ray_counts()))
        pt.close()
    (f0, r0), (f1, r1) = out
    assert np.array_equal(f0[0].view(np.uint32), f1[0].view(np.uint32)) and np.array_equal(f0[1], f1[1])
    assert f0[1].max() == 4 and r0 == r1 and r0["extension"] > 0


# ---- 10, 11: the effect ----

def mse(img, ref, keep):
    return float(np.mean((img[keep].astype(np.float64) - ref[keep]) ** 2))


def reference(mcpt, scene, cam, W, H, rc, spp):
    pt = make_pt(mcpt, scene, cam, W, H, spp=spp, depth=rc.max_depth)
    pt.render()
    L, s = pt.film()
    pt.close()
    with np.errstate(all="ignore"):
        return L / s[..., None].astype(f32), s


def test_fill_makes_the_guided_filter_work_on_a_one_slot_frame(mcpt_mod, scene_c2):
    """Config 2's proxy at 64 x 48, 8 spp in ONE path slot, 4 guide samples, against the renderer's own
    1024-spp frame: with the fill at its defaults MSE(guided) < 0.5 MSE(plain filter at its defaults).
    Only pixels without samples or with a non-finite reference value are left out: at most the last row
    and column plus 1 % of the film (141).  The numpy restatement on the CPU oracle's frames gave
    3.65e-6 against 2.80e-5 at radius 2, min_neff 2 (ratio 0.13, 111 pixels excluded).  Measured on an
    MI355X: MSE raw 5.40655e-5, plain 2.79992e-5, guided 3.61962e-6 at the defaults (radius 1, min_neff 4;
    3.64885e-6 at radius 2, min_neff 2), 111 pixels excluded."""
    W, H = 64, 48
    rc = mcpt_mod.CONFIGS[2]
    cam = mcpt_mod.config_camera(rc, W, H)
    ref, sr = reference(mcpt_mod, scene_c2[0], cam, W, H, rc, 1024)
    pt = make_pt(mcpt_mod, scene_c2[0], cam, W, H, spp=8, depth=rc.max_depth)
    pt.render()
    pt.render_guides(4)
    pt.denoise()
    plain = pt.denoised()
    pt.set_variance_fill()
    pt.denoise_guided()
    guided = pt.denoised()
    Ln, sn = pt.film()
    pt.close()
    with np.errstate(all="ignore"):
        raw = Ln / sn[..., None].astype(f32)
    keep = (sn > 0) & (sr > 0) & np.isfinite(ref).all(axis=2)
    excluded = int((~keep).sum())
    m_raw, m_plain, m_guided = (mse(im, ref, keep) for im in (raw, plain, guided))
    print(f"config 2, 64x48, 8 spp / 1 slot against 1024 spp: MSE raw {m_raw:.6g}, plain {m_plain:.6g}, "
          f"guided with the variance fill {m_guided:.6g}; {excluded} pixels excluded")
    assert excluded <= (W + H - 1) + W * H // 100, excluded
    assert np.isfinite(m_guided) and m_guided < 0.5 * m_plain


def test_fill_makes_temporal_denoise_help_on_a_one_slot_moving_sequence(mcpt_mod, scene_c2):
    """Config 2's proxy at 96 x 64, 8 frames of 2 spp in ONE path slot, the camera yawed +1 degree and
    the seed changed every frame, against the renderer's own 512-spp frame at the last camera.  With the
    fill on, accumulate + temporal_denoise must beat the accumulated frame itself, and the same pipeline
    with the fill off (which filters the accumulated frame with the plain colour term).  The numpy
    restatement on the CPU oracle's frames gave 2.97e-6 (fill on, radius 2, min_neff 2) against 1.55e-5
    (accumulated) and 3.96e-5 (fill off).  Measured on an MI355X: MSE raw 2.10549e-4, accumulated
    1.55157e-5, fill off 3.96463e-5, fill on 3.09894e-6 at the defaults (3.00224e-6 at radius 2,
    min_neff 2)."""
    W, H = 96, 64
    rc = mcpt_mod.CONFIGS[2]
    cams = [yawed(mcpt_mod, rc, W, H, 1.0 * f) for f in range(8)]
    ref, sr = reference(mcpt_mod, scene_c2[0], cams[-1], W, H, rc, 512)
    res = {}
    for on in (False, True):
        pt = make_pt(mcpt_mod, scene_c2[0], cams[0], W, H, spp=2, depth=rc.max_depth)
        if on:
            pt.set_variance_fill()
        for f, cam in enumerate(cams):
            frame(pt, cam, 500 + f)
            pt.temporal_accumulate()
        pt.temporal_denoise()
        res[on] = (pt.denoised(), pt.temporal(), pt.film())
        pt.close()
    (off_dn, off_acc, _), (on_dn, on_acc, (L, s)) = res[False], res[True]
    assert same_bits(off_acc["rgb"], on_acc["rgb"])  # the fill touches variances only
    assert np.all(off_acc["variance"] == -1) and (on_acc["variance"] >= 0).any()
    keep = (s > 0) & (sr > 0) & np.isfinite(ref).all(axis=2)
    assert int((~keep).sum()) <= (W + H - 1) + W * H // 100
    with np.errstate(all="ignore"):
        raw = L / s[..., None].astype(f32)
    m_raw, m_acc, m_off, m_on = (mse(x, ref, keep) for x in (raw, on_acc["rgb"], off_dn, on_dn))
    print(f"config 2, 96x64, 8 x 2 spp / 1 slot, +1 deg per frame, against 512 spp: MSE raw {m_raw:.6g}, accumulated "
          f"{m_acc:.6g}, accumulate + temporal_denoise with the fill off {m_off:.6g}, on {m_on:.6g}")
    assert np.isfinite(m_on) and m_on < m_acc and m_on < m_off
