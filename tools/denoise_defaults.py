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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--guided", action="store_true", help="sweep the variance-guided filter's sigma_lum and lum_eps")
    ap.add_argument("--out")
    a = ap.parse_args()
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
