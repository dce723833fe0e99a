#!/usr/bin/env python3
"""Cost and gain of emitter sampling (profiles/emitter_sampling.json) and of MIS
between its samples and collected emission (--mis; section 18; profiles/emitter_mis.json).

Config 2 at bench.py's layout (its film and path slots) under a black environment with one small sphere
emissive (--mat, radius 0.3): frames with emitter sampling off and on, alternating on one context.
Reports wall ms per frame (clear + render), each frame's mean squared error against a collection-only
frame of --ref-spp samples under another seed, and the spp at which the unsampled render would reach the
sampled frame's error: spp * mse_off / mse_on, the error of either estimator falling as 1 / spp, after
taking the reference frame's own share (mse_off * spp / ref_spp) out of both.  --mis adds a third frame
kind on the same context, emitter sampling with MIS, in the same alternation: its cost is to be read
against the sampled frame of the same run.

Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "mc-path-tracer_amd"))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--mat", type=int, default=5, help="the emissive material (config 2: 5 is the smallest sphere)")
    ap.add_argument("--radiance", type=float, default=40.0)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--ref-spp", type=int, default=1024)
    ap.add_argument("--mis", action="store_true", help="a third frame kind: emitter sampling with MIS (section 18)")
    a = ap.parse_args()
    import bench
    import mcpt

    rc = mcpt.CONFIGS[2]
    slots = bench.BENCH_SLOTS[2]
    scene = mcpt.Scene()
    scene.make_proxy(2)
    scene.set_env_color((0.0, 0.0, 0.0))
    scene.set_emission(a.mat, (a.radiance,) * 3)
    scene.build(**mcpt.DEFAULT_BVH)
    pt = mcpt.PathTracer(0, mcpt.default_config(spp=a.ref_spp, max_depth=rc.max_depth, seed=0xA11CE << 20))
    pt.upload_scene(scene)
    pt.set_camera(mcpt.config_camera(rc))
    pt.set_path_slots(slots)
    pt.resize(rc.width, rc.height)

    def mean_image():
        Ld, sm = pt.film()
        return (Ld[:-1, :-1] / np.maximum(sm[:-1, :-1, None], 1)).astype(np.float64)

    t = time.perf_counter()
    pt.render()
    ref_ms = (time.perf_counter() - t) * 1e3
    ref = mean_image()
    pt.set_seed(0x5EED2026)
    pt.set_spp(a.spp)
    ms = {"off": [], "on": []}
    if a.mis:
        ms["mis"] = []
    mse, erays = {}, {}
    by_prev, prev = {}, None  # --mis: the timed frames of each kind by the kind of the frame before
    for i in range(a.warmup + a.repeats):
        # The frame after the unsampled one allocates and clears the sampling streams inside its render:
        # with --mis the two sampled kinds swap places every round, so each pays that equally often.
        for k in (list(ms) if i % 2 == 0 else ["off"] + list(ms)[:0:-1]):
            pt.set_emitter_sampling(k != "off")
            pt.set_emitter_mis(k == "mis")
            pt.clear()
            t = time.perf_counter()
            pt.render()  # returns after the device has finished
            if i >= a.warmup:
                ms[k].append((time.perf_counter() - t) * 1e3)
                by_prev.setdefault(f"{k}_after_{prev}", []).append(round(ms[k][-1], 3))
            prev = k
            if i == 0:
                mse[k] = float(((mean_image() - ref) ** 2).mean())
                erays[k] = pt.emitter_stats()["emitter_rays"]
    stats = pt.emitter_stats()
    pt.close()
    med = lambda v: float(statistics.median(v))
    ref_share = mse["off"] * a.spp / a.ref_spp  # the reference frame's own error, a collection-only frame's at ref_spp
    on, off = max(mse["on"] - ref_share, 0.0), max(mse["off"] - ref_share, 0.0)
    extra = {}
    if a.mis:
        mis = max(mse["mis"] - ref_share, 0.0)
        extra = {"ms_per_frame_by_previous_kind": by_prev, "mse_without_reference_share_mis": mis,
                 "emitter_rays_per_frame_mis": erays["mis"],
                 "unsampled_spp_for_mis_mse": (a.spp * off / mis) if mis > 0 else None,
                 "sampled_spp_for_mis_mse": (a.spp * on / mis) if mis > 0 else None}
    print(json.dumps({
        "config": 2, "frame": [rc.width, rc.height], "spp": a.spp, "ref_spp": a.ref_spp, "slots": slots,
        "emissive_material": a.mat, "radiance": a.radiance, "repeats": a.repeats, "table_entries": stats["entries"],
        "table_build_ms": stats["build_ms"], "emitter_rays_per_frame": erays["on"],
        "ms_per_frame_median": {k: med(v) for k, v in ms.items()},
        "ms_per_frame_all": {k: [round(x, 3) for x in v] for k, v in ms.items()},
        "reference_frame_ms": ref_ms, "mse": mse, "mse_without_reference_share": {"off": off, "on": on},
        "unsampled_spp_for_sampled_mse": (a.spp * off / on) if on > 0 else None, **extra}))


if __name__ == "__main__":
    main()
