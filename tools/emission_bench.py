#!/usr/bin/env python3
"""Cost of emissive materials (profiles/emission.json).

Config 2 at bench.py's layout (its film, spp and path slots): frames with no emission table and with
one emissive wall (--mat, the ceiling), alternating on one context; wall ms per frame (clear + render)
and the shade stage's device ms per iteration (StageStats.ms_shade: k_shade + k_material).  The two
cases run different k_shade instantiations (the last template argument), so one kernel trace of this
program separates them:

  rocprofv3 --kernel-trace --stats -d D -o kt --output-format csv -- python3 tools/emission_bench.py
  python3 tools/emission_bench.py --kstats D      # k_shade time per launch, per instantiation

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
    """k_shade rows of rocprofv3's kernel_stats.csv files under d: calls, total and average ns."""
    out = {}
    for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            m = re.search(r"k_shade<(\w+), (\w+), (\w+)>", row["Name"])
            if not m:
                continue
            key = "fixed=%s map=%s emit=%s" % tuple(int(x in ("true", "1")) for x in m.groups())
            out[key] = {"calls": int(row["Calls"]), "total_ms": float(row["TotalDurationNs"]) / 1e6,
                        "us_per_launch": float(row["AverageNs"]) / 1e3}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--mat", type=int, default=2, help="the emissive material (config 2: 2 is the ceiling)")
    ap.add_argument("--radiance", type=float, default=8.0)
    ap.add_argument("--spp", type=int, default=None)
    ap.add_argument("--kstats", metavar="DIR", default=None, help="summarise a kernel trace of this program and exit")
    a = ap.parse_args()
    if a.kstats:
        print(json.dumps({"k_shade": kstats(a.kstats)}))
        return
    import bench
    import mcpt

    rc = mcpt.CONFIGS[2]
    spp, slots = a.spp or rc.spp, bench.BENCH_SLOTS[2]
    scene = mcpt.build_config_scene(2)
    pt = mcpt.PathTracer(0, mcpt.default_config(spp=spp, max_depth=rc.max_depth))
    pt.upload_scene(scene)
    pt.set_camera(mcpt.config_camera(rc))
    pt.set_path_slots(slots)
    pt.resize(rc.width, rc.height)
    E = np.zeros((len(scene.arrays()["mat_params"]), 3), np.float32)
    E[a.mat] = a.radiance
    rows = {"none": [], "one_wall": []}
    shade = {k: [] for k in rows}
    rays, lum = {}, {}
    for i in range(a.warmup + a.repeats):
        for k in rows:
            pt.set_emission(E if k == "one_wall" else None)
            pt.clear()
            t = time.perf_counter()
            st = pt.render()  # returns after the device has finished
            ms = (time.perf_counter() - t) * 1e3
            rays[k] = [int(st.extend_rays), int(st.shadow_rays), int(st.vis_rays)]
            if i >= a.warmup:
                rows[k].append(ms)
                shade[k].append(st.ms_shade / max(1, st.iterations))
        if i == 0:
            for k in rows:
                pt.set_emission(E if k == "one_wall" else None)
                pt.clear()
                pt.render()
                Ld, sm = pt.film()
                lum[k] = float((Ld[:-1, :-1].sum(axis=2) / (3.0 * sm[:-1, :-1, None].max())).mean())
    pt.close()
    med = lambda v: float(statistics.median(v))
    print(json.dumps({
        "config": 2, "frame": [rc.width, rc.height], "spp": spp, "slots": slots, "repeats": a.repeats,
        "emissive_material": a.mat, "radiance": a.radiance, "device": pt.device,
        "ms_per_frame_median": {k: med(v) for k, v in rows.items()},
        "ms_per_frame_all": {k: [round(x, 3) for x in v] for k, v in rows.items()},
        "shade_stage_ms_per_iteration_median": {k: med(v) for k, v in shade.items()},
        "rays": rays, "rays_equal": rays["none"] == rays["one_wall"], "mean_radiance": lum}))


if __name__ == "__main__":
    main()
