#!/usr/bin/env python3
"""Timing of the preview denoiser on BASELINE config 2 at 1920x1080 (profiles/denoise.json).

Reports the guide pass at 16 samples (mcpt_guides_render) and mcpt_film_denoise at the default
parameters: medians over --repeats timed calls after --warmup untimed ones, device-event times per
pass, and the achieved bytes/s of a pass over its compulsory traffic (64 B per pixel: three planes
read, one written) against the same device's measured copy ceiling (mcpt_debug_hbm_copy).  --ab also
times the passes with strides 1 and 2 moved from the LDS kernel to the direct one
(MCPT_DENOISE_LDS_MAX = 0, 1, 2), alternating the variants within every repeat.  Prints one JSON line.

--guided times the variance-guided filter instead (profiles/denoise_guided.json): the film is rendered
with 4 path slots, and every repeat runs mcpt_film_denoise_guided and mcpt_film_denoise one after the
other, so the plain passes of the same run are the yardstick.  A guided pass moves 80 B per pixel
(the plain pass's 64 B plus the float2 {variance, luminance} plane read and written).
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "mc-path-tracer_amd"))

import mcpt  # noqa: E402


def med(v):
    return float(statistics.median(v))


def guided(a, pt, W, H):
    p, q = mcpt.denoise_params(), mcpt.denoise_guided_params()
    pt.render_guides(a.guide_samples)

    def one(fn, n):
        t = time.perf_counter()
        fn()
        wall = (time.perf_counter() - t) * 1e3
        ms = pt.denoise_ms()
        return wall, ms["prepare"], ms["passes"][:n], pt.adaptive_ms()["error"]

    rows = {"guided": [], "plain": []}
    for i in range(a.warmup + a.repeats):
        for k, fn, n in (("guided", pt.denoise_guided, q.passes), ("plain", pt.denoise, p.passes)):
            r = one(fn, n)
            if i >= a.warmup:
                rows[k].append(r)
    copy_gbps = pt.hbm_copy_gbps()
    px = W * H
    res = {"tool": "denoise_bench --guided", "device": pt.device_name, "config": 2, "width": W, "height": H,
           "film_spp": a.spp, "slots": a.slots, "repeats": a.repeats, "warmup": a.warmup, "hbm_copy_gbps": copy_gbps}
    for k, par, bpp in (("guided", q, 80), ("plain", p, 64)):
        v = rows[k]
        passes_ms = [med([r[2][i] for r in v]) for i in range(par.passes)]
        res[k] = {"params": {f: getattr(par, f) for f, _ in type(par)._fields_},
                  "wall_ms_median": med([r[0] for r in v]), "prepare_ms_median": med([r[1] for r in v]),
                  "pass_ms_median": passes_ms, "passes_ms_total_median": med([sum(r[2]) for r in v]),
                  "bytes_per_pixel_per_pass": bpp,
                  "pass_gbps": [bpp * px / (ms * 1e-3) / 1e9 for ms in passes_ms]}
        res[k]["pass_share_of_copy"] = [x / copy_gbps for x in res[k]["pass_gbps"]]
    res["guided"]["film_error_ms_median"] = med([r[3] for r in rows["guided"]])
    res["guided_over_plain_pass_ms"] = [g / q_ for g, q_ in zip(res["guided"]["pass_ms_median"], res["plain"]["pass_ms_median"])]
    pt.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--guide-samples", type=int, default=16)
    ap.add_argument("--spp", type=int, default=4, help="samples of the film that is filtered")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--ab", action="store_true", help="also time MCPT_DENOISE_LDS_MAX = 0 / 1 / 2")
    ap.add_argument("--guided", action="store_true", help="time the guided passes beside the plain ones")
    ap.add_argument("--slots", type=int, default=4, help="path slots of the film (--guided)")
    ap.add_argument("--out", help="also write the JSON here")
    a = ap.parse_args()
    if a.repeats < 10:
        ap.error("--repeats must be at least 10")
    rc = mcpt.CONFIGS[2]
    W, H = a.width, a.height
    scene = mcpt.build_config_scene(2)
    pt = mcpt.PathTracer(0, mcpt.default_config(spp=a.spp, max_depth=rc.max_depth))
    pt.upload_scene(scene)
    pt.set_camera(mcpt.config_camera(rc, W, H))
    pt.resize(W, H)
    if a.guided:
        pt.set_path_slots(a.slots)
    pt.render()
    p = mcpt.denoise_params()
    if a.guided:
        return guided(a, pt, W, H)

    def guides():
        t = time.perf_counter()
        pt.render_guides(a.guide_samples)  # synchronous
        return (time.perf_counter() - t) * 1e3, pt.denoise_ms()["guides"]

    def denoise():
        t = time.perf_counter()
        pt.denoise()
        wall = (time.perf_counter() - t) * 1e3
        ms = pt.denoise_ms()
        return wall, ms["prepare"], ms["passes"][:p.passes]

    for _ in range(a.warmup):
        guides()
        denoise()
    g = [guides() for _ in range(a.repeats)]
    d = [denoise() for _ in range(a.repeats)]
    passes_ms = [med([r[2][i] for r in d]) for i in range(p.passes)]
    copy_gbps = pt.hbm_copy_gbps()
    px = W * H
    res = {
        "tool": "denoise_bench", "device": pt.device_name, "config": 2, "width": W, "height": H, "film_spp": a.spp,
        "repeats": a.repeats, "warmup": a.warmup,
        "guides": {"samples": a.guide_samples, "wall_ms_median": med([r[0] for r in g]),
                   "device_ms_median": med([r[1] for r in g]), "device_ms_min": min(r[1] for r in g),
                   "rays": (W - 1) * (H - 1) * a.guide_samples},
        "denoise": {"params": {k: getattr(p, k) for k, _ in mcpt.DenoiseParams._fields_},
                    "wall_ms_median": med([r[0] for r in d]), "prepare_ms_median": med([r[1] for r in d]),
                    "pass_ms_median": passes_ms, "passes_ms_total_median": med([sum(r[2]) for r in d]),
                    "bytes_per_pixel_per_pass": 64,
                    "pass_gbps": [64.0 * px / (ms * 1e-3) / 1e9 for ms in passes_ms]},
        "hbm_copy_gbps": copy_gbps,
    }
    res["denoise"]["pass_share_of_copy"] = [x / copy_gbps for x in res["denoise"]["pass_gbps"]]
    if a.ab:
        rows = {k: [] for k in ("0", "1", "2")}
        for i in range(a.warmup + a.repeats):
            for k in rows:
                os.environ["MCPT_DENOISE_LDS_MAX"] = k
                r = denoise()
                if i >= a.warmup:
                    rows[k].append(r[2])
        os.environ.pop("MCPT_DENOISE_LDS_MAX", None)
        res["lds_ab_pass_ms_median"] = {f"lds_max_stride_{k}": [med([r[i] for r in v]) for i in range(p.passes)]
                                        for k, v in rows.items()}
    pt.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
