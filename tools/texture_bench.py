#!/usr/bin/env python3
"""Cost of base-colour textures (profiles/textures.json).

Config 2 at bench.py's layout (its film, spp and path slots): frames without textures and with one
1024 x 1024 texture on the five walls (materials 0..4; uvs a planar map of the positions, about one
repeat per wall, so neighbouring hits read neighbouring texels), alternating on one context; wall ms per
frame (clear + render) and the shade stage's device ms per iteration (StageStats.ms_shade: k_shade +
k_material).  The two cases run different k_material instantiations (the last template argument), so one
kernel trace of this program separates them:

  rocprofv3 --kernel-trace --stats -d D -o kt --output-format csv -- python3 tools/texture_bench.py
  python3 tools/texture_bench.py --kstats D      # k_material time per launch, per instantiation

The ray counts of the two cases differ beyond rr_depth (the roulette tests a throughput the base colour
has scaled), so the figures come with the material evaluations (= shadow rays) of a frame.

--mr (profiles/textures_mr.json): the same setup with a second 1024 x 1024 image on
the same walls as their metallic-roughness texture (G, B in 64..255: the walls' roughness 1 becomes 0.25
.. 1 per hit, their metallic 0 stays 0), frames with the base-colour set alone and with base + MR alternating on one context: k_material's textured
instantiation against k_material<TexMr, ...> (a name of its own in the trace).  The counts change with the set at
every depth (F_FZERO), so the cost per material evaluation is reported too.

--normal (profiles/textures_nrm.json): --mr's setup with a third 1024 x 1024 image on the
same walls as their normal map (R, G anywhere, B in 128..255, scale 1; tangents from mcpt.tangents_from_uv over
the planar uvs), frames with base + MR and with base + MR + normal alternating on one context:
k_material<TexMr, ...> against k_material<TexNrm, ...>.

--srgb (profiles/textures_srgb.json): --normal's setup with the base-colour image flagged
MCPT_TEX_SRGB, frames with base + MR + normal unflagged and flagged alternating on one context:
k_material<TexNrm, ...> against k_material<TexSrgb, ...> (the decode table a literal array read per lane).  The
frames' spread (min, max) comes with the medians.
Prints one JSON line.
"""
import argparse
import csv
import glob
import json
import os
import re
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "mc-path-tracer_amd"))
sys.path.insert(0, REPO)


def kstats(d):
    """k_material rows of rocprofv3's kernel_stats.csv files under d: calls, total and average ns."""
    out = {}
    for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            m = re.search(r"k_material<(\w+), (\w+), (\w+), (\w+)>", row["Name"])
            r = re.search(r"k_material<(?:\w+::)*TexMr, (\w+), (\w+), (\w+)>", row["Name"])
            n = re.search(r"k_material<(?:\w+::)*TexNrm, (\w+), (\w+), (\w+)>", row["Name"])
            g = re.search(r"k_material<(?:\w+::)*TexSrgb, (\w+), (\w+), (\w+)>", row["Name"])
            if g:
                out["fixed=%s samp=%s mis=%s tex=srgb" % tuple(int(x in ("true", "1")) for x in g.groups())] = {
                    "calls": int(row["Calls"]), "total_ms": float(row["TotalDurationNs"]) / 1e6, "us_per_launch": float(row["AverageNs"]) / 1e3}
                continue
            if n:
                out["fixed=%s samp=%s mis=%s tex=nrm" % tuple(int(x in ("true", "1")) for x in n.groups())] = {
                    "calls": int(row["Calls"]), "total_ms": float(row["TotalDurationNs"]) / 1e6, "us_per_launch": float(row["AverageNs"]) / 1e3}
                continue
            if not (m or r):
                continue
            key = "fixed=%s samp=%s mis=%s tex=%s" % tuple(int(x in ("true", "1")) for x in m.groups()) if m else \
                "fixed=%s samp=%s mis=%s tex=mr" % tuple(int(x in ("true", "1")) for x in r.groups())
            out[key] = {"calls": int(row["Calls"]), "total_ms": float(row["TotalDurationNs"]) / 1e6,
                        "us_per_launch": float(row["AverageNs"]) / 1e3}
    return out


def wall_set(a, size, walls):
    """uvs from the positions (x + 0.37 z, y + 0.61 z) / 2 + 0.5 and one size x size random texture on `walls`."""
    rng = np.random.default_rng(19)
    uv = [(np.stack([v[:, 0] + 0.37 * v[:, 2], v[:, 1] + 0.61 * v[:, 2]], 1) * 0.5 + 0.5).astype(np.float32)
          for v in (np.asarray(a[k], np.float32).reshape(-1, 3) for k in ("v0", "v1", "v2"))]
    img = rng.integers(64, 256, (size, size, 4)).astype(np.uint8)
    mat_tex = np.array([0 if m in walls else -1 for m in range(len(a["mat_params"]))], np.int32)
    return uv, [img], mat_tex


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=None)
    ap.add_argument("--mr", action="store_true", help="base-colour set against base + metallic-roughness (section 20)")
    ap.add_argument("--normal", action="store_true", help="base + MR against base + MR + normal map (section 21)")
    ap.add_argument("--srgb", action="store_true", help="base + MR + normal against the same with the base image flagged sRGB (section 22)")
    ap.add_argument("--kstats", metavar="DIR", default=None, help="summarise a kernel trace of this program and exit")
    a = ap.parse_args()
    if a.kstats:
        print(json.dumps({"k_material": kstats(a.kstats)}))
        return
    import bench
    import mcpt

    rc = mcpt.CONFIGS[2]
    spp, slots = a.spp or rc.spp, bench.BENCH_SLOTS[2]
    scene = mcpt.build_config_scene(2)
    walls = (0, 1, 2, 3, 4)
    uv, imgs, mat_tex = wall_set(scene.arrays(), a.size, walls)
    pt = mcpt.PathTracer(0, mcpt.default_config(spp=spp, max_depth=rc.max_depth))
    a.normal = a.normal or a.srgb
    a.mr = a.mr or a.normal
    if a.mr:  # a second image on the same walls, both index arrays set
        imgs = imgs + [np.random.default_rng(20).integers(64, 256, (a.size, a.size, 4)).astype(np.uint8)]
        mat_mr = np.where(mat_tex >= 0, 1, -1).astype(np.int32)
    if a.normal:  # a third image on the same walls, with tangents from the planar uvs
        nimg = np.random.default_rng(21).integers(0, 256, (a.size, a.size, 4)).astype(np.uint8)
        nimg[..., 2] = np.random.default_rng(22).integers(128, 256, (a.size, a.size)).astype(np.uint8)
        imgs = imgs + [nimg]
        mat_nrm = np.where(mat_tex >= 0, 2, -1).astype(np.int32)
        sa = scene.arrays()
        tans = mcpt.tangents_from_uv(sa["v0"], sa["v1"], sa["v2"], sa["n0"], sa["n1"], sa["n2"], *uv)
    pt.upload_scene(scene)
    pt.set_camera(mcpt.config_camera(rc))
    pt.set_path_slots(slots)
    pt.resize(rc.width, rc.height)

    def case(k):
        if k == "walls_textured":
            pt.set_textures(*uv, imgs, mat_tex)
        elif k == "walls_textured_mr":
            pt.set_textures(*uv, imgs, mat_tex, mat_mr=mat_mr)
        elif k == "walls_textured_mr_nrm":
            pt.set_textures(*uv, imgs, mat_tex, mat_mr=mat_mr, tangents=tans, mat_nrm=mat_nrm)
        elif k == "walls_textured_mr_nrm_srgb":
            pt.set_textures(*uv, imgs, mat_tex, mat_mr=mat_mr, tangents=tans, mat_nrm=mat_nrm, tex_flags=[mcpt.MCPT_TEX_SRGB, 0, 0])
        else:
            pt.set_textures()

    rows = {"walls_textured": [], "walls_textured_mr": []} if a.mr else {"none": [], "walls_textured": []}
    if a.normal:
        rows = {"walls_textured_mr": [], "walls_textured_mr_nrm": []}
    if a.srgb:
        rows = {"walls_textured_mr_nrm": [], "walls_textured_mr_nrm_srgb": []}
    shade = {k: [] for k in rows}
    iters, rays, stats = {}, {}, {}
    for i in range(a.warmup + a.repeats):
        for k in rows:
            case(k)
            stats[k] = pt.texture_stats()
            pt.clear()
            t = time.perf_counter()
            st = pt.render()  # returns after the device has finished
            ms = (time.perf_counter() - t) * 1e3
            rays[k] = [int(st.extend_rays), int(st.shadow_rays), int(st.vis_rays)]
            iters[k] = int(st.iterations)
            if i >= a.warmup:
                rows[k].append(ms)
                shade[k].append(st.ms_shade / max(1, st.iterations))
    pt.close()
    med = lambda v: float(statistics.median(v))
    extra = {}
    if a.mr:  # the counts differ between the two sets: cost per material evaluation (= shadow ray)
        extra["frame_ns_per_material_evaluation"] = {k: 1e6 * med(v) / max(1, rays[k][1]) for k, v in rows.items()}
        extra["shade_stage_ns_per_material_evaluation"] = {k: 1e6 * med(v) * iters[k] / max(1, rays[k][1]) for k, v in shade.items()}
    print(json.dumps({
        "config": 2, "frame": [rc.width, rc.height], "spp": spp, "slots": slots, "repeats": a.repeats,
        "texture": [a.size, a.size], "textured_materials": list(walls), "device": pt.device,
        "ms_per_frame_median": {k: med(v) for k, v in rows.items()},
        "ms_per_frame_all": {k: [round(x, 3) for x in v] for k, v in rows.items()},
        "ms_per_frame_min_max": {k: [round(min(v), 3), round(max(v), 3)] for k, v in rows.items()},
        "shade_stage_ms_per_iteration_median": {k: med(v) for k, v in shade.items()},
        "iterations_per_frame": iters, "rays": rays, "material_evaluations": {k: v[1] for k, v in rays.items()},
        "texture_stats": stats, **extra}))


if __name__ == "__main__":
    main()
