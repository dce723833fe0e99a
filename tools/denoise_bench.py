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

--temporal times the temporal stage (profiles/temporal.json): 4 spp in 4 path slots, two frames one
degree of yaw apart per repeat, k_temporal's device time on the second (mcpt_debug_temporal_ms), its
compulsory bytes (220 B per pixel: the film, its error plane, the guide sums and the camera records in,
48 B of history in, 72 B of planes out) as a share of the same run's mcpt_debug_hbm_copy ceiling, and the
five guided passes over the accumulated frame measured in the same process.

--variance times the spatial variance estimate (profiles/variance.json): the film in one path slot,
every repeat one mcpt_film_denoise_guided with the variance fill at its defaults; k_variance_spatial's
device time (mcpt_debug_variance_ms) beside the stride-1 guided pass of the same call and the run's
copy ceiling.
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


def temporal(a, pt, W, H):
    """k_temporal on frame B accumulated onto frame A, the camera yawed by --yaw degrees between the two.
    Every repeat renders both frames anew (a seed each), so the history the timed launch gathers from is
    one call old, as in a preview loop; the guided passes then run over the accumulated frame."""
    rc = mcpt.CONFIGS[2]
    q = mcpt.denoise_guided_params()
    aspect = np.float32(W) / np.float32(H)
    cams = [mcpt.make_camera(rc.position, rc.yaw + y, rc.pitch, rc.fovy, aspect=aspect) for y in (0.0, a.yaw)]
    rows = []
    for i in range(a.warmup + a.repeats):
        pt.temporal_reset()
        for k, cam in enumerate(cams):
            pt.set_camera(cam)
            pt.set_seed((0x9E3779B97F4A7C15 * (2 * i + k + 1)) & (2 ** 64 - 1))
            pt.render()
            pt.render_guides(a.guide_samples)
            t = time.perf_counter()
            pt.temporal_accumulate()
            wall = (time.perf_counter() - t) * 1e3
        ms_t = pt.temporal_ms()
        pt.temporal_denoise()
        ms = pt.denoise_ms()
        if i >= a.warmup:
            rows.append((wall, ms_t, ms["prepare"], ms["passes"][:q.passes]))
    copy_gbps = pt.hbm_copy_gbps()
    px = W * H
    gained = float((pt.temporal()["nsamples"] > a.spp).mean())
    bpp = 16 + 4 + 16 + 16 + 16 + 32 + 48 + 72  # Ld, samples, err, two guide sums, camera records; history in; planes out
    t_ms = med([r[1] for r in rows])
    passes_ms = [med([r[3][i] for r in rows]) for i in range(q.passes)]
    res = {"tool": "denoise_bench --temporal", "device": pt.device_name, "config": 2, "width": W, "height": H,
           "film_spp": a.spp, "slots": a.slots, "yaw_deg": a.yaw, "repeats": a.repeats, "warmup": a.warmup,
           "hbm_copy_gbps": copy_gbps, "pixels_with_history": gained,
           "accumulate_wall_ms_median": med([r[0] for r in rows]),
           "temporal": {"params": {f: getattr(mcpt.temporal_params(), f) for f, _ in mcpt.TemporalParams._fields_},
                        "k_temporal_ms_median": t_ms, "k_temporal_ms_min": min(r[1] for r in rows),
                        "bytes_per_pixel": bpp, "gbps": bpp * px / (t_ms * 1e-3) / 1e9,
                        "share_of_copy": bpp * px / (t_ms * 1e-3) / 1e9 / copy_gbps,
                        "device_bytes": pt.temporal_bytes()},
           "guided": {"prepare_ms_median": med([r[2] for r in rows]), "pass_ms_median": passes_ms,
                      "passes_ms_total_median": med([sum(r[3]) for r in rows]), "bytes_per_pixel_per_pass": 80,
                      "pass_share_of_copy": [80 * px / (ms * 1e-3) / 1e9 / copy_gbps for ms in passes_ms]}}
    pt.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


def variance(a, pt, W, H):
    """k_variance_spatial inside a one-slot mcpt_film_denoise_guided with the fill at its defaults: its
    device time beside the stride-1 guided pass of the same call."""
    q, v = mcpt.denoise_guided_params(), mcpt.variance_params()
    pt.render_guides(a.guide_samples)
    pt.set_variance_fill()
    rows = []
    for i in range(a.warmup + a.repeats):
        t = time.perf_counter()
        pt.denoise_guided()
        wall = (time.perf_counter() - t) * 1e3
        ms = pt.denoise_ms()
        if i >= a.warmup:
            rows.append((wall, pt.variance_ms(), ms["prepare"], ms["passes"][:q.passes]))
    known = float((pt.denoised_variance() >= 0).mean())
    copy_gbps = pt.hbm_copy_gbps()
    px = W * H
    # the colour, guide and albedo planes' lines (16 B each; of the colour plane only the valid flag is
    # used), the vl plane read (8 B) and the variance written (4 B)
    bpp = 16 + 16 + 16 + 8 + 4
    v_ms = med([r[1] for r in rows])
    passes_ms = [med([r[3][i] for r in rows]) for i in range(q.passes)]
    res = {"tool": "denoise_bench --variance", "device": pt.device_name, "config": 2, "width": W, "height": H,
           "film_spp": a.spp, "slots": 1, "repeats": a.repeats, "warmup": a.warmup, "hbm_copy_gbps": copy_gbps,
           "pixels_with_a_variance": known,
           "variance": {"params": {f: getattr(v, f) for f, _ in mcpt.VarianceParams._fields_},
                        "k_variance_spatial_ms_median": v_ms, "k_variance_spatial_ms_min": min(r[1] for r in rows),
                        "bytes_per_pixel": bpp, "gbps": bpp * px / (v_ms * 1e-3) / 1e9,
                        "share_of_copy": bpp * px / (v_ms * 1e-3) / 1e9 / copy_gbps},
           "guided": {"wall_ms_median": med([r[0] for r in rows]), "prepare_ms_median_incl_variance": med([r[2] for r in rows]),
                      "pass_ms_median": passes_ms, "bytes_per_pixel_per_pass": 80,
                      "pass_share_of_copy": [80 * px / (ms * 1e-3) / 1e9 / copy_gbps for ms in passes_ms]},
           "variance_over_stride1_pass_ms": v_ms / passes_ms[0]}
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
    ap.add_argument("--temporal", action="store_true", help="time k_temporal and the guided passes after it")
    ap.add_argument("--yaw", type=float, default=1.0, help="degrees of yaw between the two frames (--temporal)")
    ap.add_argument("--variance", action="store_true", help="time k_variance_spatial on a one-slot film")
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
    if a.guided or a.temporal:
        pt.set_path_slots(a.slots)
    if a.temporal:
        return temporal(a, pt, W, H)
    pt.render()
    p = mcpt.denoise_params()
    if a.variance:
        return variance(a, pt, W, H)
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
