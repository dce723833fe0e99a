"""numpy float32 restatement of the temporal stage (mc-path-tracer_amd/csrc/device/temporal.hpp): every
expression in the header's order, one IEEE rounding per operation, vectorised over pixels with a loop
over the four corners of the bilinear tap in row-major order.  The host build of the header and the
gfx950 kernel must agree with it bit for bit (tests/test_temporal_host.py, tests/test_temporal_gpu.py)."""
import numpy as np

import denoise_guided_ref as G
import denoise_ref as R

f32 = np.float32
FLT_MAX = R.FLT_MAX
PARAMS = dict(pos_tol=0.2, nrm_tol=0.3, max_history=24.0, alpha_min=0.05)  # the parity tests' (not the defaults)
SHAPES = [(1, 1), (2, 3), (33, 9), (67, 35)]  # (W, H)


def known(v):
    with np.errstate(all="ignore"):
        return (v >= f32(0)) & (v <= FLT_MAX)


def finite(v):
    with np.errstate(all="ignore"):
        return v - v == 0


def sq3(a, b):
    return R._sq3(a, b)


def mat_vec4(m, v0, v1, v2, v3):
    """mcpt::mat_vec4 of the column-major 16-vector m: four (…) arrays."""
    m = np.asarray(m, f32)
    return [((m[r] * v0 + m[4 + r] * v1) + m[8 + r] * v2) + m[12 + r] * v3 for r in range(4)]


def tp_floor(f):
    i = f.astype(np.int32)  # truncation
    return np.where(i.astype(f32) > f, i - 1, i).astype(np.int32)


def pixel(rgb, samples, variance, position, normal, depth):
    """tp_pixel: dict of col (H, W, 3), valid, s, vc, reproj, X, n, z."""
    rgb = np.asarray(rgb, f32)
    sm = np.asarray(samples)
    valid = (sm > 0) & np.all(finite(rgb), axis=2)
    var = np.asarray(variance, f32)
    z = np.asarray(depth, f32)
    with np.errstate(all="ignore"):
        reproj = valid & (z > f32(0)) & (z <= FLT_MAX)
    return {"col": np.where(valid[..., None], rgb, f32(0)).astype(f32), "valid": valid,
            "s": np.where(valid, sm.astype(f32), f32(0)).astype(f32),
            "vc": np.where(valid & known(var), var, f32(-1)).astype(f32), "reproj": reproj,
            "X": np.where(reproj[..., None], np.asarray(position, f32), f32(0)).astype(f32),
            "n": np.where(reproj[..., None], np.asarray(normal, f32), f32(0)).astype(f32),
            "z": np.where(reproj, z, f32(0)).astype(f32)}


def project(vp, p, W, H):
    """tp_project: ok, x0, y0, tx, ty."""
    X = p["X"]
    with np.errstate(all="ignore"):
        c = mat_vec4(vp, X[..., 0], X[..., 1], X[..., 2], f32(1))
        Wf, Hf = f32(W), f32(H)
        fx = ((c[0] / c[3] + f32(1)) * f32(0.5)) * Wf - f32(0.5)
        fy = ((f32(1) - c[1] / c[3]) * f32(0.5)) * Hf - f32(0.5)
        ok = p["reproj"] & (c[3] > f32(0)) & (fx > f32(-1)) & (fx < Wf) & (fy > f32(-1)) & (fy < Hf)
    sx, sy = np.where(ok, fx, f32(0)).astype(f32), np.where(ok, fy, f32(0)).astype(f32)
    x0, y0 = tp_floor(sx), tp_floor(sy)
    return ok, x0, y0, sx - x0.astype(f32), sy - y0.astype(f32)


def temporal(rgb, samples, variance, position, normal, depth, hcol, hpos, hnrm, vp_prev, pos_tol, nrm_tol, max_history,
             alpha_min, detail=False):
    """The stage over (H, W, 3) rgb / position / normal, (H, W) samples / variance / depth and the three
    (H, W, 4) history planes -> col (H, W, 4), vl (H, W, 2), hcol, hpos, hnrm (H, W, 4)."""
    p = pixel(rgb, samples, variance, position, normal, depth)
    H, W = p["valid"].shape
    hcol, hpos, hnrm = (np.asarray(a, f32).reshape(H, W, 4) for a in (hcol, hpos, hnrm))
    pt, nt, mh, am = f32(pos_tol), f32(nrm_tol), f32(max_history), f32(alpha_min)
    ok, x0, y0, tx, ty = project(vp_prev, p, W, H)
    yy, xx = np.mgrid[0:H, 0:W]
    aw = np.zeros((H, W), f32)
    ac = np.zeros((H, W, 3), f32)
    an = np.zeros((H, W), f32)
    av = np.zeros((H, W), f32)
    vknown = np.ones((H, W), bool)
    accepted = []
    with np.errstate(all="ignore"):
        tol = pt * p["z"]
        for k in range(4):
            dx, dy = k & 1, k >> 1
            qx, qy = x0 + dx, y0 + dy
            inside = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
            jx, jy = np.where(inside, qx, xx), np.where(inside, qy, yy)
            hc, hp, hn = hcol[jy, jx], hpos[jy, jx], hnrm[jy, jx]
            w = (tx if dx else f32(1) - tx) * (ty if dy else f32(1) - ty)
            acc = inside & (hc[..., 3] > f32(0)) & (hc[..., 3] <= FLT_MAX) & np.all(finite(hc[..., :3]), axis=2) & \
                (hn[..., 3] > f32(0)) & (sq3(hp[..., :3], p["X"]) <= tol * tol) & (sq3(hn[..., :3], p["n"]) <= nt * nt)
            vk = known(hp[..., 3])
            wa = np.where(acc, w, f32(0)).astype(f32)
            aw = aw + wa
            ac = ac + wa[..., None] * np.where(acc[..., None], hc[..., :3], f32(0)).astype(f32)
            an = an + wa * np.where(acc, hc[..., 3], f32(0)).astype(f32)
            av = av + wa * np.where(acc & vk, hp[..., 3], f32(0)).astype(f32)
            vknown = vknown & (~acc | vk)
            accepted.append(acc)
        h = ac / aw[..., None]
        nh, vh = an / aw, av / aw
        nc = np.where(nh < mh, nh, mh).astype(f32)
        al0 = p["s"] / (nc + p["s"])
        al = np.where(al0 > am, al0, am).astype(f32)
        cb = h + al[..., None] * (p["col"] - h)
        om = f32(1) - al
        vb = (om * om) * vh + (al * al) * p["vc"]
        use = ok & (aw > f32(0)) & np.all(finite(cb), axis=2)
        vo = np.where(use, np.where(vknown & known(p["vc"]) & known(vb), vb, f32(-1)), p["vc"]).astype(f32)
    rgb_o = np.where(use[..., None], cb, p["col"]).astype(f32)
    valid_o = np.where(use, f32(1), p["valid"].astype(f32)).astype(f32)
    col = np.concatenate([rgb_o, valid_o[..., None]], axis=2)
    vl = np.stack([np.where((valid_o != 0) & known(vo), vo, f32(-1)).astype(f32),
                   np.where(valid_o != 0, G.luminance(rgb_o), f32(0)).astype(f32)], axis=2)
    out_hcol = np.concatenate([rgb_o, np.where(use, nc + p["s"], p["s"]).astype(f32)[..., None]], axis=2)
    out_hpos = np.concatenate([p["X"], np.where(p["valid"], vo, f32(-1)).astype(f32)[..., None]], axis=2)
    out_hnrm = np.concatenate([p["n"], p["z"][..., None]], axis=2)
    out = tuple(np.ascontiguousarray(a, f32) for a in (col, vl, out_hcol, out_hpos, out_hnrm))
    if detail:
        return out, {"use": use, "accepted": accepted, "pixel": p, "ok": ok}
    return out


def empty_history(W, H):
    return tuple(np.zeros((H, W, 4), f32) for _ in range(3))


# ---- synthetic frames -------------------------------------------------------------------------------

def pinhole_rays(ivp, W, H):
    """gen_ray_pixel in double (good enough to make test geometry): origins and directions (H, W, 3)."""
    m = np.asarray(ivp, np.float64).reshape(4, 4).T  # column-major -> row-major
    yy, xx = np.mgrid[0:H, 0:W]
    px = 2.0 * ((xx + 0.5) / W) - 1.0
    py = 1.0 - 2.0 * ((yy + 0.5) / H)
    one = np.ones_like(px)
    near = np.stack([px, py, -one, one], axis=-1) @ m.T
    far = np.stack([px, py, one, one], axis=-1) @ m.T
    near, far = near[..., :3] / near[..., 3:], far[..., :3] / far[..., 3:]
    d = far - near
    return near, d / np.linalg.norm(d, axis=-1, keepdims=True)


def planes_frame(ivp, W, H, planes):
    """First hits of the pinhole rays on axis-aligned planes z = const, each (z, x_min, x_max): the
    nearest hit in front of the camera.  -> position (H, W, 3), normal, depth (0 where nothing is hit)."""
    o, d = pinhole_rays(ivp, W, H)
    best = np.full((H, W), np.inf)
    for z, x_min, x_max in planes:
        with np.errstate(all="ignore"):
            t = (z - o[..., 2]) / d[..., 2]
        x = o[..., 0] + t * d[..., 0]
        hit = (t > 0) & (x >= x_min) & (x <= x_max) & (t < best)
        best = np.where(hit, t, best)
    hit = np.isfinite(best)
    t = np.where(hit, best, 0.0)
    pos = np.where(hit[..., None], o + t[..., None] * d, 0.0)
    nrm = np.where(hit[..., None], np.array([0.0, 0.0, 1.0]), 0.0)
    return pos.astype(f32), nrm.astype(f32), t.astype(f32)


def _search_edge(vp, W, H, base, axis, want_fx=None, want_fy=None):
    """Positions near `base` whose projection lands on fx == want_fx (or fy == want_fy) as closely as
    float32 allows: candidates along one coordinate in steps of its ulp, tested with the restatement
    itself.  Returns [(position, side)]: the candidate with the largest coordinate below the target
    (side -1), the one with the smallest above it (+1) and, where the arithmetic can produce the target
    at all (for many film sizes it cannot: ndc + 1 lives on a grid of 2^-23), one exactly on it (0)."""
    k = np.arange(-30000, 30001)
    X = np.tile(np.asarray(base, f32), (len(k), 1))
    X[:, axis] = (X[:, axis] + k * np.spacing(X[:, axis])).astype(f32)
    with np.errstate(all="ignore"):
        c = mat_vec4(vp, X[:, 0], X[:, 1], X[:, 2], f32(1))
        fx = ((c[0] / c[3] + f32(1)) * f32(0.5)) * f32(W) - f32(0.5)
        fy = ((f32(1) - c[1] / c[3]) * f32(0.5)) * f32(H) - f32(0.5)
    f, want = (fx, f32(want_fx)) if want_fx is not None else (fy, f32(want_fy))
    assert np.all(c[3] > 0) and (f < want).any() and (f > want).any()
    out = [(X[np.flatnonzero(f < want)[np.argmax(f[f < want])]], -1), (X[np.flatnonzero(f > want)[np.argmin(f[f > want])]], 1)]
    if (f == want).any():
        out.append((X[np.flatnonzero(f == want)[0]], 0))
    return out


def make_inputs(mcpt, W, H, seed=0, dirty=True):
    """A wall z = 0 seen by two cameras a few degrees apart (VP_prev from mcpt.camera_view_proj of the
    previous one): the current frame's positions, normals and depths from its pinhole rays, the history
    planes from the previous camera's, random colours, counts and variances.  dirty=True mixes in invalid
    pixels, pixels without history, unknown and zero variances, NaN / Inf history colours, positions
    behind the previous camera and outside its film, and positions that project onto row -1, column -1
    and the last row and column: on either side of them and, where float32 can produce the value, exactly
    ("edge": [(pixel, "fx" | "fy", target, side)])."""
    rng = np.random.default_rng(5000 * W + H + seed)
    aspect = f32(W) / f32(H)
    cur = mcpt.make_camera((0.15, 0.05, 4.0), -92.0, 1.0, aspect=aspect, lens_radius=0.0)
    prev = mcpt.make_camera((0.0, 0.0, 4.0), -90.0, 0.0, aspect=aspect, lens_radius=0.0)
    vp = mcpt.camera_view_proj(prev)
    wall = [(0.0, -1e9, 1e9)]
    pos, nrm, z = planes_frame(cur.inv_view_proj, W, H, wall)
    hp, hn, hz = planes_frame(prev.inv_view_proj, W, H, wall)
    nrm = (nrm + rng.normal(0, 0.02, (H, W, 3))).astype(f32)
    hn = (hn + rng.normal(0, 0.02, (H, W, 3))).astype(f32)
    inp = {"rgb": rng.uniform(0.1, 10.0, (H, W, 3)).astype(f32), "samples": rng.integers(1, 5, (H, W)).astype(np.uint32),
           "variance": rng.uniform(0.0, 4.0, (H, W)).astype(f32), "position": pos, "normal": nrm, "depth": z,
           "hcol": np.concatenate([rng.uniform(0.1, 10.0, (H, W, 3)), rng.uniform(1.0, 40.0, (H, W, 1))], axis=2).astype(f32),
           "hpos": np.concatenate([hp, rng.uniform(0.0, 4.0, (H, W, 1))], axis=2).astype(f32),
           "hnrm": np.concatenate([hn, hz[..., None]], axis=2).astype(f32), "vp_prev": vp}
    if not dirty:
        return inp
    n = W * H
    u = rng.uniform(size=(H, W))
    inp["samples"][u < 0.08] = 0                                   # invalid: no samples
    inp["depth"][(u >= 0.08) & (u < 0.12)] = 0.0                   # a miss
    inp["variance"][(u >= 0.12) & (u < 0.22)] = -1.0               # unknown
    inp["variance"][(u >= 0.22) & (u < 0.27)] = 0.0
    inp["variance"][(u >= 0.27) & (u < 0.29)] = np.nan
    u = rng.uniform(size=(H, W))
    inp["hcol"][u < 0.10, 3] = 0.0                                 # no history
    inp["hpos"][(u >= 0.10) & (u < 0.20), 3] = -1.0                # history without a variance
    inp["hpos"][(u >= 0.20) & (u < 0.25), 3] = 0.0
    inp["hnrm"][(u >= 0.25) & (u < 0.30), 3] = 0.0                 # a history pixel that was not reprojectable
    inp["hpos"][(u >= 0.30) & (u < 0.35), 2] += f32(1.5)           # another surface: the position test fails
    inp["hnrm"][(u >= 0.35) & (u < 0.40), :3] = f32([1, 0, 0])     # ... the normal test fails
    flat_rgb, flat_h = inp["rgb"].reshape(-1, 3), inp["hcol"].reshape(-1, 4)
    for v in (np.nan, np.inf, -np.inf):
        k = rng.integers(0, n, max(1, n // 50))
        flat_rgb[k, rng.integers(0, 3, len(k))] = v
        k = rng.integers(0, n, max(1, n // 40))
        flat_h[k, rng.integers(0, 3, len(k))] = v
    flat_pos = inp["position"].reshape(-1, 3)
    for k in rng.integers(0, n, max(1, n // 30)):                  # behind the previous camera
        flat_pos[k] = f32([rng.uniform(-1, 1), rng.uniform(-1, 1), 9.0])
    for k in rng.integers(0, n, max(1, n // 30)):                  # far outside its film
        flat_pos[k] = f32([rng.uniform(20, 30) * rng.choice([-1, 1]), rng.uniform(-1, 1), 0.0])
    if n >= 16:
        # the film's borders: wall points that project onto row -1, column -1, the last row and the last
        # column, on either side of them and, where float32 can, exactly (_search_edge)
        o, d = pinhole_rays(prev.inv_view_proj, 2, 2)
        half_w = float(np.abs(o[0, 0, 0] + (-o[0, 0, 2] / d[0, 0, 2]) * d[0, 0, 0]) * 2.0)   # the wall's half extent
        half_h = half_w / float(aspect)
        targets = [(0, "fx", -1.0, (-half_w * (1 + 1.0 / W), 0.0)), (0, "fx", W - 1.0, (half_w * (1 - 1.0 / W), 0.0)),
                   (1, "fy", -1.0, (0.0, half_h * (1 + 1.0 / H))), (1, "fy", H - 1.0, (0.0, -half_h * (1 - 1.0 / H)))]
        found = [(X, which, want, side) for axis, which, want, (bx, by) in targets
                 for X, side in _search_edge(vp, W, H, (bx, by, 0.0), axis, **{"want_" + which: want})]
        slots = rng.choice(n, len(found), replace=False)
        for k, (X, _, _, _) in zip(slots, found):
            flat_pos[k] = X
            inp["samples"].reshape(-1)[k] = 2
            flat_rgb[k] = f32([1.0, 2.0, 3.0])
            inp["depth"].reshape(-1)[k] = 4.0
        inp["edge"] = [(int(k), which, want, side) for k, (_, which, want, side) in zip(slots, found)]
    return inp


def run_ref(inp, detail=False, **par):
    par = dict(PARAMS, **par)
    return temporal(inp["rgb"], inp["samples"], inp["variance"], inp["position"], inp["normal"], inp["depth"], inp["hcol"],
                    inp["hpos"], inp["hnrm"], inp["vp_prev"], detail=detail, **par)


def disocclusion(mcpt, W=64, H=48, shift=0.5):
    """A near plane (z = 4, x <= 0) in front of a far wall (z = 0), the current camera at (0, 0, 6) and
    the previous one `shift` to its left, both looking down -z.  The current camera sees every far-wall
    point with x > 0.  The previous one does not see the point x if the line from (-shift, 6) to (x, 0)
    crosses z = 4 at x' = x - (x + shift) 4 / 6 <= 0, i.e. x <= 2 shift.  So the pixels the move
    uncovers are the far-wall pixels with 0 < x <= 2 shift (up to the bilinear tap's one-pixel reach,
    which the caller allows for).  Returns (inputs, x of every pixel's hit, hit is on the far wall)."""
    aspect = f32(W) / f32(H)
    cur = mcpt.make_camera((0.0, 0.0, 6.0), -90.0, 0.0, aspect=aspect, lens_radius=0.0)
    prev = mcpt.make_camera((-shift, 0.0, 6.0), -90.0, 0.0, aspect=aspect, lens_radius=0.0)
    scene = [(4.0, -1e9, 0.0), (0.0, -1e9, 1e9)]
    pos, nrm, z = planes_frame(cur.inv_view_proj, W, H, scene)
    hp, hn, hz = planes_frame(prev.inv_view_proj, W, H, scene)
    rng = np.random.default_rng(11)
    inp = {"rgb": rng.uniform(0.1, 2.0, (H, W, 3)).astype(f32), "samples": np.full((H, W), 2, np.uint32),
           "variance": rng.uniform(0.0, 1.0, (H, W)).astype(f32), "position": pos, "normal": nrm, "depth": z,
           "hcol": np.concatenate([rng.uniform(0.1, 2.0, (H, W, 3)), np.full((H, W, 1), 6.0)], axis=2).astype(f32),
           "hpos": np.concatenate([hp, rng.uniform(0.0, 1.0, (H, W, 1))], axis=2).astype(f32),
           "hnrm": np.concatenate([hn, hz[..., None]], axis=2).astype(f32), "vp_prev": mcpt.camera_view_proj(prev)}
    return inp, pos[..., 0].astype(np.float64), pos[..., 2] < 1.0
