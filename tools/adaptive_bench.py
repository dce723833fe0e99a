#!/usr/bin/env python3
"""Measurements of adaptive sampling (profiles/adaptive.json).

  map      the config-2 frame of bench.py (its film, spp and path slots) with no budget map and with a
           uniform map installed, alternating, wall ms per frame (clear + render)
  kernels  mcpt_film_error and mcpt_budget_from_error on a 1920 x 1080 film at 24 path slots: device
           ms, and bytes per second over their compulsory traffic (error: 20 B per slot and pixel read,
           16 B per pixel written; budget: 16 B read, 4 B written) against the device's measured copy
           ceiling (mcpt_debug_hbm_copy)
  quality  per config (its own film size and bench path slots): the renderer's 1024-spp frame as the
           reference; for every --targets row render_adaptive(target, --min-spp, --max-spp, --rounds),
           then a uniform render at the same total sample count (rounded to whole spp); MSE of the mean
           radiance against the reference over the rendered pixels with finite values, wall ms and rays

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

import mcpt  # noqa: E402


def med(v):
    return float(statistics.median(v))


def tracer(cid, spp, slots, W=None, H=None):
    rc = mcpt.CONFIGS[cid]
    W, H = W or rc.width, H or rc.height
    pt = mcpt.PathTracer(0, mcpt.default_config(spp=spp, max_depth=rc.max_depth))
    pt.upload_scene(mcpt.build_config_scene(cid))
    pt.set_camera(mcpt.config_camera(rc, W, H))
    pt.set_path_slots(slots)
    pt.resize(W, H)
    return pt


def timed_frame(pt):
    pt.clear()
    t = time.perf_counter()
    st = pt.render()
    return (time.perf_counter() - t) * 1e3, st


def map_cost(a, slots):
    rc = mcpt.CONFIGS[2]
    pt = tracer(2, rc.spp, slots)
    rows = {"none": [], "uniform_map": []}
    full = np.full((pt.H, pt.W), rc.spp, np.uint32)
    rays = {}
    for i in range(a.warmup + a.repeats):
        for k in rows:
            pt.set_sample_budget(full if k == "uniform_map" else None)
            ms, st = timed_frame(pt)
            rays[k] = st.rays
            if i >= a.warmup:
                rows[k].append(ms)
    pt.close()
    return {"config": 2, "spp": rc.spp, "slots": slots, "repeats": a.repeats,
            "ms_per_frame_median": {k: med(v) for k, v in rows.items()},
            "ms_per_frame_min": {k: min(v) for k, v in rows.items()},
            "ms_per_frame_all": {k: [round(x, 3) for x in v] for k, v in rows.items()}, "rays": rays}


def kernels(a):
    S, W, H = 24, 1920, 1080
    pt = tracer(2, 2 * S, S, W, H)
    pt.render()
    err_ms, bud_ms = [], []
    for i in range(a.warmup + a.repeats):
        pt.film_error()
        pt.budget_from_error()
        ms = pt.adaptive_ms()
        if i >= a.warmup:
            err_ms.append(ms["error"])
            bud_ms.append(ms["budget"])
    copy = pt.hbm_copy_gbps()
    pt.close()
    px = W * H
    eb, bb = (20 * S + 16) * px, 20 * px
    e, b = med(err_ms), med(bud_ms)
    return {"width": W, "height": H, "slots": S, "repeats": a.repeats, "hbm_copy_gbps": copy,
            "film_error": {"device_ms_median": e, "device_ms_min": min(err_ms), "bytes": eb, "gbps": eb / (e * 1e-3) / 1e9,
                           "share_of_copy": eb / (e * 1e-3) / 1e9 / copy},
            "budget": {"device_ms_median": b, "device_ms_min": min(bud_ms), "bytes": bb, "gbps": bb / (b * 1e-3) / 1e9,
                       "share_of_copy": bb / (b * 1e-3) / 1e9 / copy}}


def mean_image(pt):
    L, s = pt.film()
    with np.errstate(all="ignore"):
        return L.astype(np.float64) / np.maximum(s, 1)[..., None], s


def quality(a, cid, slots):
    pt = tracer(cid, a.ref_spp, slots)
    ms_ref, st = timed_frame(pt)
    ref, s = mean_image(pt)
    ok = (s > 0) & np.isfinite(ref).all(axis=2)

    def mse(img):
        good = ok & np.isfinite(img).all(axis=2)
        d = img[good] - ref[good]
        rel = d / (ref[good] + 0.01)
        return float((d * d).mean()), float((rel * rel).mean()), int(good.sum())

    npx = int((s > 0).sum())
    rows = []
    for target in a.targets:
        pt.clear()
        t = time.perf_counter()
        stats, budgets = pt.render_adaptive(target=target, min_spp=a.min_spp, max_spp=a.max_spp, rounds=a.rounds)
        ms_ad = (time.perf_counter() - t) * 1e3
        img, smp = mean_image(pt)
        total = int(smp.sum())
        m_ad = mse(img)
        hist = {int(v): int(c) for v, c in zip(*np.unique(np.minimum(smp[s > 0], a.max_spp), return_counts=True))}
        n_uni = max(1, int(round(total / npx)))
        pt.set_sample_budget(None)
        pt.set_spp(n_uni)
        ms_un, st_un = timed_frame(pt)
        m_un = mse(mean_image(pt)[0])
        rows.append({"target_rel_err": target, "min_spp": a.min_spp, "max_spp": a.max_spp, "rounds": a.rounds,
                     "adaptive": {"samples": total, "mean_spp": total / npx, "mse": m_ad[0], "rel_mse": m_ad[1],
                                  "wall_ms": ms_ad, "rays": int(sum(x.rays for x in stats)), "budgets": budgets,
                                  "pixels_at_min": hist.get(a.min_spp, 0), "pixels_at_max": hist.get(a.max_spp, 0)},
                     "uniform": {"spp": n_uni, "samples": n_uni * npx, "mse": m_un[0], "rel_mse": m_un[1],
                                 "wall_ms": ms_un, "rays": int(st_un.rays)},
                     "mse_ratio_adaptive_over_uniform": m_ad[0] / m_un[0] if m_un[0] else None,
                     "rel_mse_ratio_adaptive_over_uniform": m_ad[1] / m_un[1] if m_un[1] else None})
    pt.close()
    return {"config": cid, "width": mcpt.CONFIGS[cid].width, "height": mcpt.CONFIGS[cid].height, "slots": slots,
            "reference_spp": a.ref_spp, "reference_wall_ms": ms_ref, "rendered_pixels": npx, "rows": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="map,kernels,quality")
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--configs", type=int, nargs="*", default=[2, 3])
    ap.add_argument("--ref-spp", type=int, default=1024)
    ap.add_argument("--targets", type=float, nargs="*", default=[0.2, 0.1, 0.05, 0.025])
    ap.add_argument("--min-spp", type=int, default=32)
    ap.add_argument("--max-spp", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", help="also write the JSON here")
    a = ap.parse_args()
    import bench

    res = {"tool": "adaptive_bench"}
    what = a.what.split(",")
    if "map" in what:
        res["map"] = map_cost(a, bench.BENCH_SLOTS[2])
    if "kernels" in what:
        res["kernels"] = kernels(a)
    if "quality" in what:
        res["quality"] = [quality(a, c, bench.BENCH_SLOTS[c]) for c in a.configs]
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
