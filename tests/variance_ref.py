"""numpy float32 restatement of the spatial variance estimate
(mc-path-tracer_amd/csrc/device/variance.hpp): every expression in the header's order, one IEEE rounding
per operation, the shared pieces from denoise_ref / denoise_guided_ref.  The host build of the header and
the gfx950 kernel must agree with it bit for bit (tests/test_variance_host.py, tests/test_variance_gpu.py)."""
import numpy as np

import denoise_guided_ref as G
import denoise_ref as R

f32 = np.float32
RADII = [1, 2, 3]
PARAMS = dict(sigma_normal=0.5, sigma_albedo=0.3, sigma_depth=0.2, min_neff=2.0)


def variance(rgb, albedo, normal, depth, samples=None, variance=None, radius=2, sigma_normal=0.3, sigma_albedo=0.3,
             sigma_depth=0.1, min_neff=2.0):
    """The estimate over (H, W, 3) rgb / albedo / normal and (H, W) depth [/ samples / known variances]
    -> (H, W) variance: the known inputs, the estimate elsewhere, -1 where unknown."""
    col, valid, rz = R.planes(rgb, samples, normal, albedo, depth)
    N, A, Z = np.asarray(normal, f32), np.asarray(albedo, f32), np.asarray(depth, f32)
    H, W = valid.shape
    kn, ka, kz = R.dn_k(sigma_normal), R.dn_k(sigma_albedo), R.dn_k(sigma_depth)
    if variance is None:
        v0 = np.full((H, W), -1, f32)
    else:
        var = np.asarray(variance, f32).reshape(H, W)
        with np.errstate(all="ignore"):
            v0 = np.where(valid & (var >= f32(0)) & (var <= R.FLT_MAX), var, f32(-1)).astype(f32)  # dn_vl
    lum = np.where(valid, G.luminance(col), f32(0)).astype(f32)
    sw, sww, s1, s2 = (np.zeros((H, W), f32) for _ in range(4))
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            win = G._window(H, W, dy, dx)
            if win is None:
                continue
            P, Q = win
            m = valid[P] & valid[Q]
            with np.errstate(all="ignore"):
                if dx == 0 and dy == 0:
                    e = np.ones(m.shape, f32)
                else:
                    dz = Z[P] - Z[Q]
                    x = ((f32(0) + kn * R._sq3(N[P], N[Q])) + ka * R._sq3(A[P], A[Q])) + (kz * (dz * dz)) * rz[P]
                    e = np.where((x >= f32(0)) & (x <= R.FLT_MAX), R.dexp_neg(x), f32(0)).astype(f32)
                d = lum[Q] - lum[P]
                sw[P] = np.where(m, sw[P] + e, sw[P])
                sww[P] = np.where(m, sww[P] + e * e, sww[P])
                s1[P] = np.where(m, s1[P] + e * d, s1[P])
                s2[P] = np.where(m, s2[P] + e * (d * d), s2[P])
    with np.errstate(all="ignore"):
        mean = s1 / sw
        raw = s2 / sw - mean * mean
        var = np.where(raw > f32(0), raw, f32(0)).astype(f32)
        neff = (sw * sw) / sww
        var = var * (neff / (neff - f32(1)))
        ok = (neff >= f32(min_neff)) & (raw - raw == f32(0)) & (var >= f32(0)) & (var <= R.FLT_MAX)
    est = np.where(ok, var, f32(-1)).astype(f32)
    return np.where(valid, np.where(v0 >= f32(0), v0, est), f32(-1)).astype(f32)


def run_ref(inp, known=False, **par):
    """variance() over a make_inputs dict; known: its "variance" entries count as known."""
    return variance(inp["rgb"], inp["albedo"], inp["normal"], inp["depth"], inp["samples"],
                    inp["variance"] if known else None, **par)
