"""The temporal stage's gfx950 kernel (mcpt_temporal_run, mcpt_film_temporal) against the numpy float32
restatement (tests/temporal_ref.py), bit for bit; the film path against mcpt_temporal_run fed the
film's means, the squared standard error and the guides' means; the world positions against traced
first hits; one path slot; a static view; the seed setter; side effects; error codes; and the effect on
a moving 2-spp sequence."""
import numpy as np
import pytest

import temporal_ref as T

pytestmark = pytest.mark.gpu
f32 = np.float32
NAMES = ("col", "vl", "hcol", "hpos", "hnrm")


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, f32).view(np.uint32), np.ascontiguousarray(b, f32).view(np.uint32))


@pytest.fixture(scope="module")
def ctx(mcpt_mod):
    pt = mcpt_mod.PathTracer(0)  # mcpt_temporal_run needs neither a scene nor a film
    yield pt
    pt.close()


def run(mcpt, ctx, inp, **par):
    par = dict(T.PARAMS, **par)
    return mcpt.temporal_run(ctx, inp["rgb"], inp["samples"], inp["variance"], inp["position"], inp["normal"], inp["depth"],
                             inp["hcol"], inp["hpos"], inp["hnrm"], inp["vp_prev"], **par)


@pytest.mark.parametrize("shape", T.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_temporal_run_matches_numpy(mcpt_mod, ctx, shape):
    inp = T.make_inputs(mcpt_mod, *shape)
    got = run(mcpt_mod, ctx, inp)
    for name, g, r in zip(NAMES, got, T.run_ref(inp)):
        assert same_bits(g, r), name


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


def frame_seed(k):
    """A seed per frame that differs in every bit field: the seed is XORed onto (pixel << 32 | sample
    index), so seeds that differ in their low bits alone (k, k + 1) hand a 2-spp pixel the same two
    samples in the other order, and the frames would repeat each other's noise."""
    return (0x9E3779B97F4A7C15 * (k + 1)) & (2 ** 64 - 1)


def frame(pt, cam, k, guides=2):
    pt.set_camera(cam)
    pt.set_seed(frame_seed(k))
    pt.render()
    pt.render_guides(guides)


def yawed(mcpt, rc, W, H, yaw_off, **kw):
    return mcpt.make_camera(rc.position, rc.yaw + yaw_off, rc.pitch, rc.fovy, aspect=f32(W) / f32(H), **kw)


@pytest.mark.parametrize("cid", [1, 2])
def test_film_path_equals_the_run_on_the_means(request, mcpt_mod, ctx, cid):
    """Three frames (2 spp in 2 slots) with the camera yawed and the seed changed between them: each
    call's accumulated frame equals mcpt_temporal_run fed that frame's film means, se^2, the guides'
    means, the positions read back, and the previous call's planes."""
    W, H = 64, 48
    rc = mcpt_mod.CONFIGS[cid]
    scene = request.getfixturevalue(f"scene_c{cid}")[0]
    cams = [yawed(mcpt_mod, rc, W, H, 1.5 * f) for f in range(3)]
    pt = make_pt(mcpt_mod, scene, cams[0], W, H, spp=2, depth=rc.max_depth, slots=2)
    hist, vp_prev = T.empty_history(W, H), mcpt_mod.camera_view_proj(cams[0])
    gained = []
    for f, cam in enumerate(cams):
        frame(pt, cam, 100 + f)
        pt.temporal_accumulate(**T.PARAMS)
        t = pt.temporal()
        rgb, _, nm, z, smp = means(pt.film(), pt.guides())
        var = variance_of(pt.film_error())
        assert smp.max() == 2 and (var >= 0).any()
        col, vl, hcol, hpos, hnrm = mcpt_mod.temporal_run(ctx, rgb, smp, var, t["position"], nm, z, *hist, vp_prev, **T.PARAMS)
        assert same_bits(hcol[..., :3], t["rgb"]) and same_bits(hcol[..., 3], t["nsamples"]), f"frame {f}: colour"
        assert same_bits(hpos[..., 3], t["variance"]) and same_bits(hpos[..., :3], t["position"]), f"frame {f}: variance"
        gained.append(int((t["nsamples"] > smp).sum()))
        hist, vp_prev = (hcol, hpos, hnrm), mcpt_mod.camera_view_proj(cam)
    pt.close()
    # the first call accumulates nothing; the later ones do wherever there is a surface (config 1's sphere
    # covers a quarter of the film, the sky has no first hit to reproject)
    assert gained[0] == 0 and min(gained[1:]) > W * H // 16, gained


def test_positions_are_the_traced_first_hits(mcpt_mod, oracle, scene_c1):
    """lens_radius = 0: X = o + t d of the pixel's pinhole ray, against mcpt_stage_run's closest hit of
    that ray.  Tolerance: 8 ulp of the largest coordinate magnitude (tp_world is one multiply-add per
    component on the traced t)."""
    scene, arrays = scene_c1
    W, H = 64, 48
    cam = mcpt_mod.make_camera((0.2, 0.1, 4.0), -88.0, 2.0, aspect=f32(W) / f32(H), lens_radius=0.0)
    pt = make_pt(mcpt_mod, scene, cam, W, H, spp=2, depth=3, slots=2)
    pt.render()
    pt.render_guides(1)
    pt.temporal_accumulate()
    pos = pt.temporal()["position"].reshape(-1, 3)
    P = W * H
    dead = {"flags": np.ones(P, np.uint32), "hit_tri": np.full(P, -1, np.int32), "ray_d": np.zeros((P, 3), f32),
            "beta": np.zeros((P, 4), f32), "nee0": np.zeros((P, 4), f32), "nee1": np.zeros((P, 4), f32),
            "vis": np.zeros((P, 2), np.uint8), "Ld": np.zeros((P, 3), f32), "samples": np.zeros(P, np.uint32)}
    out = oracle.stage_logic(arrays, cam, W, H, dead, spp=1)
    q = (out["queued"] & 1) != 0
    hit_p, _, tri = pt.trace_closest(out["ray_o"][q], out["ray_d"][q])
    pt.close()
    hit = tri >= 0
    assert hit.sum() > P // 8 and (~hit).any()
    got, want = pos[q][hit], hit_p[hit, :3]
    tol = 8 * np.spacing(np.abs(want).max(axis=1).astype(f32))
    assert np.all(np.abs(got - want).max(axis=1) <= tol), float(np.abs(got - want).max())
    assert np.all(pos[q][~hit] == 0) and np.all(pos[~q] == 0)


def test_one_slot_has_no_variance_and_filters_like_the_plain_run(mcpt_mod, ctx, scene_c1):
    W, H = 64, 48
    rc = mcpt_mod.CONFIGS[1]
    pt = make_pt(mcpt_mod, scene_c1[0], yawed(mcpt_mod, rc, W, H, 0.0), W, H, spp=2, depth=rc.max_depth)
    for f in range(2):
        frame(pt, yawed(mcpt_mod, rc, W, H, 1.0 * f), 7 + f)
        pt.temporal_accumulate()
    t = pt.temporal()
    sig = dict(passes=3, sigma_color=2.0, sigma_normal=0.5, sigma_albedo=0.3, sigma_depth=0.2)
    pt.temporal_denoise(**sig)
    got, got_v = pt.denoised(), pt.denoised_variance()
    _, al, nm, z, _ = means(pt.film(), pt.guides())
    pt.close()
    assert np.all(t["variance"] == -1) and (t["nsamples"] > 2).any() and np.all(got_v == -1)
    want = mcpt_mod.denoise_run(ctx, t["rgb"], al, nm, z, (t["nsamples"] > 0).astype(np.uint32), **sig)
    assert same_bits(got, want)


def mse(img, ref, keep):
    return float(np.mean((img[keep].astype(np.float64) - ref[keep]) ** 2))


def reference(mcpt, scene, cam, W, H, rc, spp=512):
    pt = make_pt(mcpt, scene, cam, W, H, spp=spp, depth=rc.max_depth)
    pt.render()
    L, s = pt.film()
    pt.close()
    with np.errstate(all="ignore"):
        return L / s[..., None].astype(f32), s


def test_a_static_view_accumulates_like_one_longer_frame(mcpt_mod, scene_c2):
    """Four frames from one camera with four seeds, max_history large: every pixel with a first hit ends
    with N' = 4 s (to the rounding of the tap's sum(w N) / sum(w): four products, three sums and a
    quotient per frame, under 32 ulp in all), a miss keeps N' = s, and the accumulated frame is closer to
    the 512-spp frame than any of the four.  A pinhole: with a lens the guide depth of a silhouette
    pixel depends on the seed, and such a pixel may find its own history inconsistent.  Measured on an
    MI355X: MSE accumulated 5.63199e-5, single frames 2.2465e-4, 2.17552e-4, 2.50832e-4, 2.01261e-4."""
    W, H = 64, 48
    rc = mcpt_mod.CONFIGS[2]
    cam = yawed(mcpt_mod, rc, W, H, 0.0, lens_radius=0.0)
    ref, sr = reference(mcpt_mod, scene_c2[0], cam, W, H, rc)
    pt = make_pt(mcpt_mod, scene_c2[0], cam, W, H, spp=2, depth=rc.max_depth, slots=2)
    single = []
    for f in range(4):
        frame(pt, cam, 31 + f)
        pt.temporal_accumulate(max_history=1e6, alpha_min=0.0)
        L, s = pt.film()
        with np.errstate(all="ignore"):
            single.append(L / s[..., None].astype(f32))
    t = pt.temporal()
    g = pt.guides()
    pt.close()
    with np.errstate(all="ignore"):
        hit = (s > 0) & (g["depth"] / g["count"].astype(f32) > 0)
    assert hit.sum() > W * H // 4
    n4 = 4.0 * s[hit].astype(np.float64)
    assert np.all(np.abs(t["nsamples"][hit] - n4) <= n4 * 32 * 2.0 ** -24)
    assert np.all(t["nsamples"][(s > 0) & ~hit] == s[(s > 0) & ~hit]) and np.all(t["nsamples"][s == 0] == 0)
    keep = (s > 0) & (sr > 0) & np.isfinite(ref).all(axis=2)
    m_acc, m_single = mse(t["rgb"], ref, keep), [mse(x, ref, keep) for x in single]
    print(f"config 2, 64x48, static view, 4 x 2 spp against 512 spp: MSE accumulated {m_acc:.6g}, single frames "
          + ", ".join(f"{m:.6g}" for m in m_single))
    assert np.isfinite(m_acc) and all(m_acc < m for m in m_single)


def test_set_seed_equals_a_fresh_context(mcpt_mod, scene_c1):
    W, H = 64, 48
    rc = mcpt_mod.CONFIGS[1]
    cam = mcpt_mod.config_camera(rc, W, H)
    fresh = make_pt(mcpt_mod, scene_c1[0], cam, W, H, spp=2, depth=rc.max_depth, seed=12345)
    fresh.render()
    want = fresh.film()
    fresh.close()
    pt = make_pt(mcpt_mod, scene_c1[0], cam, W, H, spp=2, depth=rc.max_depth)
    pt.render()
    other = pt.film()
    pt.render_guides(1)
    pt.guides()
    pt.set_seed(12345)
    with pytest.raises(mcpt_mod.McptError, match="mcpt_guides_render"):  # the guides are stale
        pt.guides()
    assert pt.film()[1].max() == 0  # the film was cleared
    pt.render()
    got = pt.film()
    assert same_bits(got[0], want[0]) and np.array_equal(got[1], want[1]) and not same_bits(got[0], other[0])
    pt.clear()
    assert pt.iterate(1).live_paths > 0
    with pytest.raises(mcpt_mod.McptError, match="mcpt error -1.*in flight"):
        pt.set_seed(1)
    pt.render()
    assert same_bits(pt.film()[0], want[0])  # the refused call changed nothing
    pt.close()


def test_no_side_effects_on_the_render_and_the_other_filters(mcpt_mod, scene_c2):
    """Guides, an accumulation and a temporal denoise between two halves of a render change nothing the
    render produces, nor what the two film filters return afterwards; a context that never calls them
    holds no bytes for them."""
    W, H = 64, 48
    rc = mcpt_mod.CONFIGS[2]
    cam = mcpt_mod.config_camera(rc, W, H)
    out = []
    for interleave in (False, True):
        pt = make_pt(mcpt_mod, scene_c2[0], cam, W, H, spp=2, depth=rc.max_depth, slots=2)
        pt.render()
        if interleave:
            pt.render_guides(2)
            pt.temporal_accumulate()
            pt.temporal_denoise()
            assert pt.denoised().shape == (H, W, 3) and pt.temporal_bytes() == W * H * (7 * 16 + 8)
        else:
            assert pt.temporal_bytes() == 0
        pt.set_spp(4)
        pt.render()
        film, rays = pt.film(), pt.ray_counts()
        pt.render_guides(2)
        if interleave:
            pt.temporal_accumulate()
            pt.temporal_denoise()
        pt.denoise()
        plain = pt.denoised()
        pt.denoise_guided()
        out.append((film, rays, plain, pt.denoised(), pt.denoised_variance()))
        if not interleave:
            assert pt.temporal_bytes() == 0
        pt.close()
    (f0, r0, p0, g0, v0), (f1, r1, p1, g1, v1) = out
    assert np.array_equal(f0[0].view(np.uint32), f1[0].view(np.uint32)) and np.array_equal(f0[1], f1[1])
    assert f0[1].max() == 4 and r0 == r1 and r0["extension"] > 0
    assert same_bits(p0, p1) and same_bits(g0, g1) and same_bits(v0, v1)


def test_error_codes_name_the_missing_step(mcpt_mod, ctx, scene_c1):
    W, H = 17, 13
    cam = mcpt_mod.make_camera((0.0, 0.0, 4.0), -90.0, 0.0, aspect=f32(W) / f32(H))
    pt = make_pt(mcpt_mod, scene_c1[0], cam, W, H, spp=2, depth=3, slots=2)
    pt.render()
    with pytest.raises(mcpt_mod.McptError, match="mcpt error -1.*mcpt_film_temporal"):  # read before accumulate
        pt.temporal()
    with pytest.raises(mcpt_mod.McptError, match="mcpt error -1.*mcpt_film_temporal"):
        pt.temporal_denoise()
    with pytest.raises(mcpt_mod.McptError, match="mcpt error -1.*mcpt_guides_render"):  # no guides
        pt.temporal_accumulate()
    pt.render_guides(1)
    for kw, what in ((dict(pos_tol=-1.0), "pos_tol"), (dict(nrm_tol=-0.5), "nrm_tol"), (dict(max_history=-1.0), "max_history"),
                     (dict(alpha_min=-0.1), "alpha_min"), (dict(alpha_min=1.5), "alpha_min"),
                     (dict(pos_tol=float("nan")), "pos_tol"), (dict(nrm_tol=float("inf")), "nrm_tol"),
                     (dict(max_history=float("inf")), "max_history"), (dict(alpha_min=float("nan")), "alpha_min")):
        with pytest.raises(mcpt_mod.McptError, match="mcpt error -1.*" + what):
            pt.temporal_accumulate(**kw)
    with pytest.raises(mcpt_mod.McptError, match="mcpt_film_temporal"):  # none of those accumulated
        pt.temporal()
    lib = mcpt_mod.lib()
    assert lib.mcpt_temporal_default_params(None) == -1 and lib.mcpt_camera_view_proj(None, None) == -1
    assert lib.mcpt_film_temporal(None, None) == -1 and lib.mcpt_temporal_read(None, None, None, None, None) == -1
    assert lib.mcpt_temporal_run(pt.h, 2, 2, *([None] * 16)) == -1 and b"null" in lib.mcpt_last_error(pt.h)
    inp = T.make_inputs(mcpt_mod, 2, 3)
    with pytest.raises(mcpt_mod.McptError, match="alpha_min"):
        run(mcpt_mod, ctx, inp, alpha_min=2.0)
    # paths in flight
    pt.clear()
    assert pt.iterate(1).live_paths > 0
    with pytest.raises(mcpt_mod.McptError, match="mcpt error -1.*in flight"):
        pt.temporal_accumulate()
    pt.render()
    pt.temporal_accumulate()
    first = pt.temporal()
    assert np.array_equal(first["nsamples"], pt.film()[1].astype(f32))
    assert lib.mcpt_temporal_read(pt.h, None, None, None, None) == 0  # every pointer may be NULL
    pt.temporal_denoise(passes=2)
    with pytest.raises(mcpt_mod.McptError, match="mcpt error -1.*passes"):
        pt.temporal_denoise(passes=0)
    # the history survives a film clear, a seed and a camera change ...
    pt.clear()
    assert same_bits(pt.temporal()["rgb"], first["rgb"])
    frame(pt, mcpt_mod.make_camera((0.05, 0.0, 4.0), -90.0, 0.0, aspect=f32(W) / f32(H)), 9, guides=1)
    with pytest.raises(mcpt_mod.McptError, match="mcpt error -1.*mcpt_film_temporal"):  # the frame is another camera's
        pt.temporal_denoise()
    pt.temporal_accumulate()
    assert (pt.temporal()["nsamples"] > 2).any()
    # ... a reset, a scene upload and a resize drop it
    pt.temporal_reset()
    with pytest.raises(mcpt_mod.McptError, match="mcpt_film_temporal"):
        pt.temporal()
    pt.temporal_accumulate()
    assert pt.temporal()["nsamples"].max() == 2
    pt.upload_scene(scene_c1[0])
    with pytest.raises(mcpt_mod.McptError, match="mcpt_film_temporal"):
        pt.temporal()
    pt.render()
    pt.render_guides(1)
    pt.temporal_accumulate()
    assert pt.temporal()["nsamples"].max() == 2 and pt.temporal_bytes() > 0
    pt.resize(W, H, 64, 64)
    assert pt.temporal_bytes() == 0
    with pytest.raises(mcpt_mod.McptError, match="mcpt_film_temporal"):
        pt.temporal()
    pt.close()


def test_accumulation_beats_the_single_frame_filter_on_a_moving_sequence(mcpt_mod, scene_c2):
    """Config 2's proxy at 96 x 64, 8 frames of 2 spp in 2 slots, the camera yawed +1 degree and the
    seed changed every frame, against the renderer's own 512-spp frame at the last camera: accumulate +
    temporal_denoise at the defaults must beat denoise_guided of the last frame alone.  Measured on an
    MI355X: MSE raw 2.10549e-4, accumulated 1.55157e-5, denoise_guided of the last frame 8.48134e-6,
    accumulate + temporal_denoise 2.80074e-6; mean history 7.19 samples."""
    W, H = 96, 64
    rc = mcpt_mod.CONFIGS[2]
    cams = [yawed(mcpt_mod, rc, W, H, 1.0 * f) for f in range(8)]
    ref, sr = reference(mcpt_mod, scene_c2[0], cams[-1], W, H, rc)
    pt = make_pt(mcpt_mod, scene_c2[0], cams[0], W, H, spp=2, depth=rc.max_depth, slots=2)
    for f, cam in enumerate(cams):
        frame(pt, cam, 500 + f)
        pt.temporal_accumulate()
    pt.temporal_denoise()
    temporal = pt.denoised()
    acc = pt.temporal()
    pt.denoise_guided()
    single = pt.denoised()
    L, s = pt.film()
    pt.close()
    with np.errstate(all="ignore"):
        raw = L / s[..., None].astype(f32)
    keep = (s > 0) & (sr > 0) & np.isfinite(ref).all(axis=2)
    assert int((~keep).sum()) <= (W + H - 1) + W * H // 100
    m_raw, m_acc, m_single, m_temporal = (mse(x, ref, keep) for x in (raw, acc["rgb"], single, temporal))
    print(f"config 2, 96x64, 8 x 2 spp / 2 slots, +1 deg per frame, against 512 spp: MSE raw {m_raw:.6g}, accumulated "
          f"{m_acc:.6g}, denoise_guided of the last frame {m_single:.6g}, accumulate + temporal_denoise {m_temporal:.6g}; "
          f"mean history {float(acc['nsamples'][keep].mean()):.3g} samples")
    assert np.isfinite(m_temporal) and m_temporal < m_single
