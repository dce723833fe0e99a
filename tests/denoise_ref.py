"""numpy float32 restatement of the a-trous filter (mc-path-tracer_amd/csrc/device/denoise.hpp): every
expression in the header's order, one IEEE rounding per operation, vectorised over pixels with a loop
over the 25 taps in row-major (dy, dx) order.  The host build of the header and the gfx950 kernels
must agree with it bit for bit (tests/test_denoise_host.py, tests/test_denoise_gpu.py)."""
import numpy as np

f32 = np.float32
LOG2E = f32(1.44269504088896341)
LN2_HI = f32(0.693359375)
LN2_LO = f32(-2.12194440e-4)
EXP_MAX = f32(87.5)
FLT_MIN = f32(1.17549435e-38)
FLT_MAX = f32(3.402823466e+38)
POLY = [f32(v) for v in (-1.52527338e-5, 1.54035304e-4, -1.33335581e-3, 9.61812911e-3, -5.55041087e-2,
                         2.40226507e-1, -6.93147181e-1)]
H5 = {-2: f32(0.0625), -1: f32(0.25), 0: f32(0.375), 1: f32(0.25), 2: f32(0.0625)}

SHAPES = [(1, 1), (5, 3), (33, 9), (67, 35)]  # (W, H)
PASSES = [1, 3, 6]
SIGMAS = dict(sigma_color=2.0, sigma_normal=0.5, sigma_albedo=0.3, sigma_depth=0.2)
SIGMAS_OFF = dict(sigma_color=0.0, sigma_normal=0.0, sigma_albedo=0.0, sigma_depth=0.0)


def dexp_neg(x):
    x = np.asarray(x, f32)
    with np.errstate(all="ignore"):
        ok = x <= EXP_MAX
        pos = x > f32(0)
        xs = np.where(ok & pos, x, f32(1))
        k = (xs * LOG2E + f32(0.5)).astype(np.int32)  # truncation of a positive value
        kf = k.astype(f32)
        r = xs - kf * LN2_HI
        r = r - kf * LN2_LO
        f = r * LOG2E
        p = POLY[0] * f
        for c in POLY[1:]:
            p = p + c
            p = p * f
        p = p + f32(1)
        e = np.ldexp(p, -k).astype(f32)  # p * 2^-k, one rounding
        e = np.where(e < FLT_MIN, f32(0), e)
    return np.where(~ok, f32(0), np.where(~pos, f32(1), e)).astype(f32)


def dn_k(sigma):
    sigma = f32(sigma)
    return f32(1) / (sigma * sigma) if sigma > 0 else f32(0)


def planes(rgb, samples, normal, albedo, depth):
    """dn_planes: colour (H, W, 3) with invalid pixels zeroed, valid (H, W) bool, rz (H, W)."""
    rgb = np.asarray(rgb, f32)
    has = np.ones(rgb.shape[:2], bool) if samples is None else np.asarray(samples) > 0
    with np.errstate(all="ignore"):
        valid = has & np.all(rgb - rgb == 0, axis=2)
        col = np.where(valid[..., None], rgb, f32(0)).astype(f32)
        z = np.asarray(depth, f32)
        z2 = z * z
        rz = f32(1) / np.where(z2 > f32(1e-12), z2, f32(1e-12)).astype(f32)
    return col, valid, rz


def _sq3(a, b):
    d = a - b
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def denoise(rgb, albedo, normal, depth, samples=None, passes=5, sigma_color=1.0, sigma_normal=0.0, sigma_albedo=0.0,
            sigma_depth=0.0):
    """The filter over (H, W, 3) rgb / albedo / normal and (H, W) depth [/ samples] -> (H, W, 3)."""
    col, valid, rz = planes(rgb, samples, normal, albedo, depth)
    N, A, Z = np.asarray(normal, f32), np.asarray(albedo, f32), np.asarray(depth, f32)
    H, W = valid.shape
    kn, ka, kz = dn_k(sigma_normal), dn_k(sigma_albedo), dn_k(sigma_depth)
    sc = f32(sigma_color)
    for i in range(passes):
        kc = dn_k(sc)
        s = 1 << i
        aw = np.zeros((H, W), f32)
        ac = np.zeros((H, W, 3), f32)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                oy, ox = dy * s, dx * s
                y0, y1, x0, x1 = max(0, -oy), min(H, H - oy), max(0, -ox), min(W, W - ox)
                if y0 >= y1 or x0 >= x1:
                    continue
                P = (slice(y0, y1), slice(x0, x1))
                Q = (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))
                m = valid[P] & valid[Q]
                with np.errstate(all="ignore"):
                    if dx == 0 and dy == 0:
                        e = np.ones(m.shape, f32)
                    else:
                        dz = Z[P] - Z[Q]
                        x = ((kc * _sq3(col[P], col[Q]) + kn * _sq3(N[P], N[Q])) + ka * _sq3(A[P], A[Q])) + \
                            (kz * (dz * dz)) * rz[P]
                        e = np.where((x >= f32(0)) & (x <= FLT_MAX), dexp_neg(x), f32(0)).astype(f32)
                    w = (H5[dy] * H5[dx]) * e
                    aw[P] = np.where(m, aw[P] + w, aw[P])
                    ac[P] = np.where(m[..., None], ac[P] + w[..., None] * col[Q], ac[P])
        with np.errstate(all="ignore"):
            col = np.where(valid[..., None], ac / aw[..., None], f32(0)).astype(f32)
        sc = sc * f32(0.5)
    return col


def make_inputs(W, H, seed=0, dirty=True):
    """Random colour in [0.1, 10], guides in two regions (left / right of a slanted edge: orthogonal
    normals, different albedo and depth, each with a little noise); with dirty=True about 10 % of the
    pixels without samples and a few NaN / Inf colours and NaN normals."""
    rng = np.random.default_rng(1000 * W + H + seed)
    rgb = rng.uniform(0.1, 10.0, (H, W, 3)).astype(f32)
    yy, xx = np.mgrid[0:H, 0:W]
    right = (xx + yy // 3) * 2 >= W
    normal = np.where(right[..., None], f32([1, 0, 0]), f32([0, 0, 1])).astype(f32)
    normal = (normal + rng.normal(0, 0.02, (H, W, 3))).astype(f32)
    albedo = (np.where(right[..., None], f32([0.8, 0.2, 0.2]), f32([0.3, 0.7, 0.4])) +
              rng.uniform(-0.02, 0.02, (H, W, 3))).astype(f32)
    depth = (np.where(right, 5.0, 2.0) + rng.uniform(-0.05, 0.05, (H, W))).astype(f32)
    samples = np.full((H, W), 4, np.uint32)
    if dirty:
        samples[rng.uniform(size=(H, W)) < 0.10] = 0
        n = W * H
        for v in (np.nan, np.inf, -np.inf):
            k = rng.integers(0, n, max(1, n // 60))
            rgb.reshape(-1, 3)[k, rng.integers(0, 3, len(k))] = v
        k = rng.integers(0, n, max(1, n // 60))
        normal.reshape(-1, 3)[k, 0] = np.nan
        depth.reshape(-1)[rng.integers(0, n, max(1, n // 100))] = 0.0  # a miss
    return {"rgb": rgb, "albedo": albedo, "normal": normal, "depth": depth, "samples": samples, "right": right}
