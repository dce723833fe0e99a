"""numpy float32 restatement of the variance-guided a-trous filter (the guided half of
mc-path-tracer_amd/csrc/device/denoise.hpp): every expression in the header's order, one IEEE rounding
per operation, the shared pieces from denoise_ref.  The host build of the header and the gfx950 kernels
must agree with it bit for bit (tests/test_denoise_guided_host.py, tests/test_denoise_guided_gpu.py)."""
import numpy as np

import denoise_ref as R

f32 = np.float32
GUIDED = dict(sigma_lum=4.0, lum_eps=1e-4)


def luminance(c):
    """mcpt::luminance: in double, rounded once to float32."""
    c = np.asarray(c, f32).astype(np.float64)
    with np.errstate(all="ignore"):
        return (0.299 * c[..., 0] + 0.587 * c[..., 1] + 0.114 * c[..., 2]).astype(f32)


def _window(H, W, oy, ox):
    y0, y1, x0, x1 = max(0, -oy), min(H, H - oy), max(0, -ox), min(W, W - ox)
    if y0 >= y1 or x0 >= x1:
        return None
    return (slice(y0, y1), slice(x0, x1)), (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))


def denoise_guided(rgb, variance, albedo, normal, depth, samples=None, passes=5, sigma_lum=4.0, lum_eps=1e-4,
                   sigma_color=1.0, sigma_normal=0.0, sigma_albedo=0.0, sigma_depth=0.0):
    """The guided filter over (H, W, 3) rgb / albedo / normal and (H, W) variance / depth [/ samples]
    -> ((H, W, 3) colour, (H, W) variance with -1 where unknown)."""
    col, valid, rz = R.planes(rgb, samples, normal, albedo, depth)
    N, A, Z = np.asarray(normal, f32), np.asarray(albedo, f32), np.asarray(depth, f32)
    H, W = valid.shape
    kn, ka, kz = R.dn_k(sigma_normal), R.dn_k(sigma_albedo), R.dn_k(sigma_depth)
    sl, eps = f32(sigma_lum), f32(lum_eps)
    var = np.asarray(variance, f32).reshape(H, W)
    with np.errstate(all="ignore"):
        v = np.where(valid & (var >= f32(0)) & (var <= R.FLT_MAX), var, f32(-1)).astype(f32)
    lum = np.where(valid, luminance(col), f32(0)).astype(f32)
    sc = f32(sigma_color)
    for i in range(passes):
        kc = R.dn_k(sc)
        s = 1 << i
        known = v >= f32(0)
        # prefilter: 3 x 3 at stride 1 over the known variances
        gs, gv = np.zeros((H, W), f32), np.zeros((H, W), f32)
        for dy in range(-1, 2):
            for dx in range(-1, 2):
                win = _window(H, W, dy, dx)
                if win is None:
                    continue
                P, Q = win
                g = f32(0.25) if (dx == 0 and dy == 0) else f32(0.125) if (dx == 0 or dy == 0) else f32(0.0625)
                m = known[P] & known[Q]
                gs[P] = np.where(m, gs[P] + g, gs[P])
                gv[P] = np.where(m, gv[P] + g * v[Q], gv[P])
        with np.errstate(all="ignore"):
            vt = gv / gs
            rcp = (f32(1) / (sl * np.sqrt(vt) + eps)).astype(f32)
        aw = np.zeros((H, W), f32)
        ac = np.zeros((H, W, 3), f32)
        av = np.zeros((H, W), f32)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                win = _window(H, W, dy * s, dx * s)
                if win is None:
                    continue
                P, Q = win
                m = valid[P] & valid[Q]
                with np.errstate(all="ignore"):
                    if dx == 0 and dy == 0:
                        e = np.ones(m.shape, f32)
                    else:
                        dz = Z[P] - Z[Q]
                        xc = np.where(known[P], np.abs(lum[P] - lum[Q]) * rcp[P], kc * R._sq3(col[P], col[Q])).astype(f32)
                        x = ((xc + kn * R._sq3(N[P], N[Q])) + ka * R._sq3(A[P], A[Q])) + (kz * (dz * dz)) * rz[P]
                        e = np.where((x >= f32(0)) & (x <= R.FLT_MAX), R.dexp_neg(x), f32(0)).astype(f32)
                    w = (R.H5[dy] * R.H5[dx]) * e
                    aw[P] = np.where(m, aw[P] + w, aw[P])
                    ac[P] = np.where(m[..., None], ac[P] + w[..., None] * col[Q], ac[P])
                    vq = np.where(v[Q] >= f32(0), v[Q], v[P])
                    av[P] = np.where(m & known[P], av[P] + (w * w) * vq, av[P])
        with np.errstate(all="ignore"):
            col = np.where(valid[..., None], ac / aw[..., None], f32(0)).astype(f32)
            v = np.where(valid & known, av / (aw * aw), f32(-1)).astype(f32)
        lum = np.where(valid, luminance(col), f32(0)).astype(f32)
        sc = sc * f32(0.5)
    return col, v


def make_inputs(W, H, seed=0, dirty=True):
    """denoise_ref.make_inputs plus "variance": uniform in [0, 4]; with dirty=True about 10 % unknown
    (-1), 5 % exactly 0 and 2 % NaN."""
    inp = R.make_inputs(W, H, seed, dirty)
    rng = np.random.default_rng(77000 + 1000 * W + H + seed)
    var = rng.uniform(0.0, 4.0, (H, W)).astype(f32)
    if dirty:
        u = rng.uniform(size=(H, W))
        var[u < 0.10] = -1.0
        var[(u >= 0.10) & (u < 0.15)] = 0.0
        var[(u >= 0.15) & (u < 0.17)] = np.nan
    inp["variance"] = var
    return inp


def heteroscedastic(W=96, H=64, seed=3):
    """A 16-pixel checkerboard of two colours, the right half 5x brighter, with Gaussian noise of
    sigma = 0.02 mean (top half) / 0.3 mean (bottom half) per channel, flat guides, variance = sigma^2.
    The two colours differ in luminance (0.82 against 0.30): the guided term sees luminance only, so a
    board of equal luminances would test that limit and not the noise levels.
    Returns (inputs, clean image)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    a, b = np.array([0.9, 0.8, 0.7]), np.array([0.25, 0.3, 0.4])
    clean = np.where((((xx // 16) + (yy // 16)) % 2 == 0)[..., None], a, b)
    clean = clean * np.where(xx >= W // 2, 5.0, 1.0)[..., None]
    rel = np.where(yy < H // 2, 0.02, 0.3)
    mean = clean.mean(axis=2)
    sigma = rel * mean
    noisy = clean + rng.normal(size=(H, W, 3)) * sigma[..., None]
    inp = {"rgb": noisy.astype(f32), "variance": (sigma * sigma).astype(f32),
           "albedo": np.full((H, W, 3), 0.5, f32), "normal": np.tile(f32([0, 0, 1]), (H, W, 1)),
           "depth": np.full((H, W), 2.0, f32), "samples": np.full((H, W), 4, np.uint32)}
    return inp, clean.astype(f32)
