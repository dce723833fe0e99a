#!/usr/bin/env python3
"""The denoiser's default sigmas, measured (profiles/denoise_defaults.txt).

Renders BASELINE configs 1 and 2 and the cube scene at 64x48 and 4 spp, denoises each frame with
5 passes and every candidate (sigma_color, sigma_normal, sigma_albedo, sigma_depth), and compares with
the renderer's own 1024-spp frame of the same film: MSE over the pixels that have samples and a finite
reference.  Rows are ranked by the geometric mean over the three scenes of MSE(denoised) / MSE(raw);
the defaults (mcpt_denoise_default_params) are the best row.  A sigma of 0 turns its term off.

--guided sweeps the variance-guided filter's (sigma_lum, lum_eps) instead
(profiles/denoise_guided_defaults.txt): the same scenes and size with 4 path slots, frames at 4 and 16
spp and one render_adaptive frame at its defaults each, five passes, the guide sigmas at their current
defaults, ranked by the geometric mean over the nine frames; the plain filter's row on the same frames
is printed beside it.  The best row is mcpt_denoise_guided_default_params.

--temporal sweeps the temporal stage's (pos_tol, nrm_tol, max_history, alpha_min)
(profiles/temporal_defaults.txt): sequences of 8 frames of the same scenes and size at 2 spp in 2 path
slots, the camera yawed by 0.5 or 2 degrees per frame, a seed per frame; the score is the MSE of the
last frame after accumulation and the guided passes, relative to the guided passes over the last frame
alone, both against the 1024-spp frame at the last camera, ranked by the geometric mean over the six
sequences.  The best row is mcpt_temporal_default_params.

--variance sweeps the spatial variance estimate's (radius, min_neff) and the guided filter's sigma_lum
over it (profiles/variance_defaults.txt): one-slot frames of the same scenes and size at 2, 4, 8 and 16
spp, mcpt_film_denoise_guided with the variance fill on, five passes, lum_eps 0, the guide sigmas at
their defaults, ranked by the geometric mean over the twelve frames; the plain filter's row on the same
frames is printed beside it.  The best row is mcpt_variance_default_params.
"""
import argparse
import itertools
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "mc-path-tracer_amd"))

import mcpt  # noqa: E402

W, H, SPP, REF_SPP, GUIDES, PASSES = 64, 48, 4, 1024, 4, 5
COLOR = (0.0, 0.25, 0.5, 1.0, 2.0, 4.0)
NORMAL = (0.1, 0.3, 1.0)
ALBEDO = (0.05, 0.1, 0.3)
DEPTH = (0.05, 0.1, 0.5)


def scenes():
    for cid in (1, 2):
        rc = mcpt.CONFIGS[cid]
        yield f"config{cid}", mcpt.build_config_scene(cid), mcpt.config_camera(rc, W, H), rc.max_depth
    s = mcpt.Scene()
    s.load_glb(os.path.join(mcpt.ASSET_DIR, "Cube.glb"))
    s.set_env_hdr(os.path.join(mcpt.ASSET_DIR, "HDR_029_Sky_Cloudy_Env.hdr"), 1)
    s.build(8)
    yield "cube", s, mcpt.make_camera((0.3, 0.1, 3.0), -90.0, 0.0, aspect=np.float32(W) / np.float32(H)), 5


def tracer(scene, cam, spp, depth):
    pt = mcpt.PathTracer(0, mcpt.default_config(spp=spp, max_depth=depth, tile=64))
    pt.upload_scene(scene)
    pt.set_camera(cam)
    pt.resize(W, H, 64, 64)
    pt.render()
    return pt


GUIDED_SLOTS = 4
GUIDED_SPP = (4, 16, "adaptive")
SIGMA_LUM = (1.0, 2.0, 4.0, 8.0)
LUM_EPS = (0.0, 1e-6, 1e-4, 1e-2)


def guided(out):
    cands = list(itertools.product(SIGMA_LUM, LUM_EPS))
    frames, raw_mse = [], []
    cols, plain = [], []
    for name, scene, cam, depth in scenes():
        rp = tracer(scene, cam, REF_SPP, depth)
        Lr, sr = rp.film()
        rp.close()
        with np.errstate(all="ignore"):
            ref = Lr / sr[..., None].astype(np.float32)
        for spp in GUIDED_SPP:
            pt = mcpt.PathTracer(0, mcpt.default_config(spp=4 if spp == "adaptive" else spp, max_depth=depth, tile=64))
            pt.upload_scene(scene)
            pt.set_camera(cam)
            pt.resize(W, H, 64, 64)
            pt.set_path_slots(GUIDED_SLOTS)
            if spp == "adaptive":
                pt.render_adaptive()
            else:
                pt.render()
            pt.render_guides(GUIDES)
            Ln, sn = pt.film()
            with np.errstate(all="ignore"):
                raw = Ln / sn[..., None].astype(np.float32)
            keep = (sn > 0) & (sr > 0) & np.isfinite(ref).all(axis=2)
            r64 = ref[keep].astype(np.float64)
            m = float(np.mean((raw[keep] - r64) ** 2))
            frames.append(f"{name}/{spp}")
            raw_mse.append(m)
            pt.denoise(passes=PASSES)
            plain.append(float(np.mean((pt.denoised()[keep] - r64) ** 2)) / m)
            col = []
            for sl, eps in cands:
                pt.denoise_guided(passes=PASSES, sigma_lum=sl, lum_eps=eps)
                col.append(float(np.mean((pt.denoised()[keep] - r64) ** 2)) / m)
            cols.append(col)
            pt.close()
    ratios = np.array(cols).T  # candidate x frame
    gm = lambda r: float(np.exp(np.mean(np.log(r))))  # noqa: E731
    score = np.array([gm(r) for r in ratios])
    order = np.argsort(score)
    d = mcpt.denoise_guided_params()
    lines = [f"# guided denoiser defaults: {W}x{H}, {GUIDED_SLOTS} path slots, {GUIDES} guide samples, {PASSES} passes, "
             f"against {REF_SPP} spp",
             "# frames (scene/spp): " + " ".join(frames),
             "# MSE(raw): " + " ".join(f"{m:.6g}" for m in raw_mse),
             "# columns: sigma_lum lum_eps | MSE(denoised) / MSE(raw) per frame | geometric mean",
             f"# built-in defaults: passes {d.passes}, sigma_lum {d.sigma_lum:g}, lum_eps {d.lum_eps:g}; guide sigmas "
             f"{d.sigma_color:g} {d.sigma_normal:g} {d.sigma_albedo:g} {d.sigma_depth:g}",
             "plain filter   | " + " ".join(f"{r:9.5f}" for r in plain) + f" | {gm(plain):9.5f}"]
    for i in order:
        sl, eps = cands[i]
        mark = "  <- defaults" if abs(sl - d.sigma_lum) < 1e-6 and abs(eps - d.lum_eps) < 1e-9 else ""
        lines.append(f"{sl:5g} {eps:8g} | " + " ".join(f"{r:9.5f}" for r in ratios[i]) + f" | {score[i]:9.5f}{mark}")
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    b = cands[order[0]]
    print(f"best: sigma_lum {b[0]:g} lum_eps {b[1]:g}")


T_FRAMES, T_SPP, T_SLOTS, T_GUIDES = 8, 2, 2, 2
T_YAW = (0.5, 2.0)
POS_TOL = (0.02, 0.05, 0.1, 0.2)
NRM_TOL = (0.25, 0.5, 1.0)
MAX_HISTORY = (4.0, 8.0, 16.0, 32.0, 64.0)
ALPHA_MIN = (0.0, 0.05, 0.1, 0.2, 0.4)


def frame_seed(k):
    """A seed per frame that differs in every bit field (seeds one apart hand a pixel the same samples)."""
    return (0x9E3779B97F4A7C15 * (k + 1)) & (2 ** 64 - 1)


def temporal(out):
    """Sequences of T_FRAMES frames per scene and yaw step; each frame's film means, variances, guide
    means and positions are recorded once from the film path, and every candidate replays the sequence
    through mcpt_temporal_run and filters the last accumulated frame with mcpt_denoise_guided_run."""
    cands = list(itertools.product(POS_TOL, NRM_TOL, MAX_HISTORY, ALPHA_MIN))
    run = mcpt.PathTracer(0)
    names, single_mse, cols = [], [], []
    for name, scene, cam0, depth in scenes():
        rc = {"config1": mcpt.CONFIGS[1], "config2": mcpt.CONFIGS[2]}.get(name)
        pos = rc.position if rc else (0.3, 0.1, 3.0)
        for step in T_YAW:
            cams = [mcpt.make_camera(pos, -90.0 + step * f, rc.pitch if rc else 0.0, aspect=np.float32(W) / np.float32(H))
                    for f in range(T_FRAMES)]
            rp = tracer(scene, cams[-1], REF_SPP, depth)
            Lr, sr = rp.film()
            rp.close()
            pt = mcpt.PathTracer(0, mcpt.default_config(spp=T_SPP, max_depth=depth, tile=64))
            pt.upload_scene(scene)
            pt.set_camera(cams[0])
            pt.resize(W, H, 64, 64)
            pt.set_path_slots(T_SLOTS)
            rec = []
            for f, cam in enumerate(cams):
                pt.set_camera(cam)
                pt.set_seed(frame_seed(f))
                pt.render()
                pt.render_guides(T_GUIDES)
                pt.temporal_accumulate()
                L, s = pt.film()
                g = pt.guides()
                se = pt.film_error()[..., 0]
                with np.errstate(all="ignore"):
                    cnt = g["count"].astype(np.float32)
                    rec.append(dict(rgb=L / s[..., None].astype(np.float32), samples=s,
                                    variance=np.where(se < 0, np.float32(-1), se * se).astype(np.float32),
                                    position=pt.temporal()["position"], normal=g["normal"] / cnt[..., None],
                                    depth=g["depth"] / cnt, albedo=g["albedo"] / cnt[..., None],
                                    vp=mcpt.camera_view_proj(cam)))
            pt.denoise_guided()
            single = pt.denoised()
            pt.close()
            with np.errstate(all="ignore"):
                ref = Lr / sr[..., None].astype(np.float32)
            keep = (rec[-1]["samples"] > 0) & (sr > 0) & np.isfinite(ref).all(axis=2)
            r64 = ref[keep].astype(np.float64)
            m = float(np.mean((single[keep] - r64) ** 2))
            names.append(f"{name}/{step:g}")
            single_mse.append(m)
            col = []
            for pt_, nt, mh, am in cands:
                hist, vp_prev = tuple(np.zeros((H, W, 4), np.float32) for _ in range(3)), rec[0]["vp"]
                for r in rec:
                    c4, vl, *hist = mcpt.temporal_run(run, r["rgb"], r["samples"], r["variance"], r["position"], r["normal"],
                                                      r["depth"], *hist, vp_prev, pos_tol=pt_, nrm_tol=nt, max_history=mh,
                                                      alpha_min=am)
                    vp_prev = r["vp"]
                last = rec[-1]
                den, _ = mcpt.denoise_guided_run(run, c4[..., :3], vl[..., 0], last["albedo"], last["normal"], last["depth"],
                                                 (c4[..., 3] != 0).astype(np.uint32))
                col.append(float(np.mean((den[keep] - r64) ** 2)) / m)
            cols.append(col)
    run.close()
    ratios = np.array(cols).T  # candidate x sequence
    score = np.exp(np.mean(np.log(ratios), axis=1))
    # (candidates whose alpha never differs, e.g. a short max_history under any alpha_min, replay the same
    # frames and tie exactly: a stable sort keeps them in grid order)
    order = np.argsort(score, kind="stable")
    d = mcpt.temporal_params()
    cur = (d.pos_tol, d.nrm_tol, d.max_history, d.alpha_min)
    lines = [f"# temporal defaults: {W}x{H}, sequences of {T_FRAMES} frames, {T_SPP} spp in {T_SLOTS} slots, {T_GUIDES} guide "
             f"samples, a seed per frame, the guided passes at their defaults, against {REF_SPP} spp at the last camera",
             "# sequences (scene/yaw step in degrees): " + " ".join(names),
             "# MSE(denoise_guided of the last frame alone): " + " ".join(f"{m:.6g}" for m in single_mse),
             "# columns: pos_tol nrm_tol max_history alpha_min | MSE(accumulate + temporal_denoise) / MSE(last frame alone) "
             "per sequence | geometric mean",
             f"# built-in defaults: {cur[0]:g} {cur[1]:g} {cur[2]:g} {cur[3]:g}"]
    for i in order:
        c = cands[i]
        mark = "  <- defaults" if all(abs(x - y) < 1e-6 for x, y in zip(c, cur)) else ""
        lines.append(f"{c[0]:5g} {c[1]:5g} {c[2]:5g} {c[3]:5g} | " + " ".join(f"{r:9.5f}" for r in ratios[i]) +
                     f" | {score[i]:9.5f}{mark}")
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[:17]))
    b = cands[order[0]]
    print(f"best: pos_tol {b[0]:g} nrm_tol {b[1]:g} max_history {b[2]:g} alpha_min {b[3]:g}")


V_SPP = (2, 4, 8, 16)
V_RADIUS = (1, 2, 3)
V_MIN_NEFF = (1.5, 2.0, 4.0)
V_SIGMA_LUM = (4.0, 8.0)


def variance(out):
    cands = list(itertools.product(V_RADIUS, V_MIN_NEFF, V_SIGMA_LUM))
    frames, raw_mse, cols, plain = [], [], [], []
    for name, scene, cam, depth in scenes():
        rp = tracer(scene, cam, REF_SPP, depth)
        Lr, sr = rp.film()
        rp.close()
        with np.errstate(all="ignore"):
            ref = Lr / sr[..., None].astype(np.float32)
        for spp in V_SPP:
            pt = tracer(scene, cam, spp, depth)  # one path slot
            pt.render_guides(GUIDES)
            Ln, sn = pt.film()
            with np.errstate(all="ignore"):
                raw = Ln / sn[..., None].astype(np.float32)
            keep = (sn > 0) & (sr > 0) & np.isfinite(ref).all(axis=2)
            r64 = ref[keep].astype(np.float64)
            m = float(np.mean((raw[keep] - r64) ** 2))
            frames.append(f"{name}/{spp}")
            raw_mse.append(m)
            pt.denoise(passes=PASSES)
            plain.append(float(np.mean((pt.denoised()[keep] - r64) ** 2)) / m)
            col = []
            for radius, neff, sl in cands:
                pt.set_variance_fill(radius=radius, min_neff=neff)
                pt.denoise_guided(passes=PASSES, sigma_lum=sl, lum_eps=0.0)
                col.append(float(np.mean((pt.denoised()[keep] - r64) ** 2)) / m)
            cols.append(col)
            pt.close()
    ratios = np.array(cols).T  # candidate x frame
    gm = lambda r: float(np.exp(np.mean(np.log(r))))  # noqa: E731
    score = np.array([gm(r) for r in ratios])
    order = np.argsort(score, kind="stable")
    d, g = mcpt.variance_params(), mcpt.denoise_guided_params()
    lines = [f"# variance estimate defaults: {W}x{H}, one path slot, {GUIDES} guide samples, {PASSES} guided passes with "
             f"lum_eps 0, against {REF_SPP} spp",
             "# frames (scene/spp): " + " ".join(frames),
             "# MSE(raw): " + " ".join(f"{m:.6g}" for m in raw_mse),
             "# columns: radius min_neff sigma_lum | MSE(denoised) / MSE(raw) per frame | geometric mean",
             f"# built-in defaults: radius {d.radius}, min_neff {d.min_neff:g}, guide sigmas {d.sigma_normal:g} "
             f"{d.sigma_albedo:g} {d.sigma_depth:g}; the guided filter's sigma_lum {g.sigma_lum:g}",
             "plain filter     | " + " ".join(f"{r:8.4f}" for r in plain) + f" | {gm(plain):8.4f}"]
    for i in order:
        radius, neff, sl = cands[i]
        mark = "  <- defaults" if radius == d.radius and abs(neff - d.min_neff) < 1e-6 and abs(sl - g.sigma_lum) < 1e-6 else ""
        lines.append(f"{radius:3d} {neff:5g} {sl:5g}  | " + " ".join(f"{r:8.4f}" for r in ratios[i]) + f" | {score[i]:8.4f}{mark}")
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    b = cands[order[0]]
    print(f"best: radius {b[0]} min_neff {b[1]:g} sigma_lum {b[2]:g}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--guided", action="store_true", help="sweep the variance-guided filter's sigma_lum and lum_eps")
    ap.add_argument("--temporal", action="store_true", help="sweep the temporal stage's four parameters")
    ap.add_argument("--variance", action="store_true", help="sweep the spatial variance estimate's radius and min_neff")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.variance:
        return variance(a.out or os.path.join(REPO, "profiles", "variance_defaults.txt"))
    if a.temporal:
        return temporal(a.out or os.path.join(REPO, "profiles", "temporal_defaults.txt"))
    if a.guided:
        return guided(a.out or os.path.join(REPO, "profiles", "denoise_guided_defaults.txt"))
    a.out = a.out or os.path.join(REPO, "profiles", "denoise_defaults.txt")
    cands = list(itertools.product(COLOR, NORMAL, ALBEDO, DEPTH))
    ratios = np.zeros((len(cands), 3))
    raw_mse, names = [], []
    for k, (name, scene, cam, depth) in enumerate(scenes()):
        names.append(name)
        rp = tracer(scene, cam, REF_SPP, depth)
        Lr, sr = rp.film()
        rp.close()
        pt = tracer(scene, cam, SPP, depth)
        pt.render_guides(GUIDES)
        Ln, sn = pt.film()
        with np.errstate(all="ignore"):
            ref = Lr / sr[..., None].astype(np.float32)
            raw = Ln / sn[..., None].astype(np.float32)
        keep = (sn > 0) & (sr > 0) & np.isfinite(ref).all(axis=2)
        r64 = ref[keep].astype(np.float64)
        raw_mse.append(float(np.mean((raw[keep] - r64) ** 2)))
        for i, (sc, sn_, sa, sz) in enumerate(cands):
            pt.denoise(passes=PASSES, sigma_color=sc, sigma_normal=sn_, sigma_albedo=sa, sigma_depth=sz)
            ratios[i, k] = float(np.mean((pt.denoised()[keep] - r64) ** 2)) / raw_mse[-1]
        pt.close()
    score = np.exp(np.mean(np.log(ratios), axis=1))
    order = np.argsort(score)
    d = mcpt.denoise_params()
    cur = (d.sigma_color, d.sigma_normal, d.sigma_albedo, d.sigma_depth)
    lines = [f"# denoiser defaults: {W}x{H}, {SPP} spp + {GUIDES} guide samples, {PASSES} passes, against {REF_SPP} spp",
             "# MSE(raw 4 spp): " + ", ".join(f"{n} {m:.6g}" for n, m in zip(names, raw_mse)),
             "# columns: sigma_color sigma_normal sigma_albedo sigma_depth | MSE(denoised) / MSE(raw): "
             + " ".join(names) + " | geometric mean",
             f"# built-in defaults: passes {d.passes}, sigmas {cur[0]:g} {cur[1]:g} {cur[2]:g} {cur[3]:g}"]
    for i in order:
        c = cands[i]
        mark = "  <- defaults" if all(abs(x - y) < 1e-6 for x, y in zip(c, cur)) else ""
        lines.append(f"{c[0]:5g} {c[1]:5g} {c[2]:5g} {c[3]:5g} | " + " ".join(f"{r:10.6f}" for r in ratios[i]) +
                     f" | {score[i]:10.6f}{mark}")
    text = "\n".join(lines) + "\n"
    with open(a.out, "w") as f:
        f.write(text)
    print("\n".join(lines[:12]))
    b = cands[order[0]]
    print(f"best: sigma_color {b[0]:g} sigma_normal {b[1]:g} sigma_albedo {b[2]:g} sigma_depth {b[3]:g}")


if __name__ == "__main__":
    main()
