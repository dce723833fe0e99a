"""Geometry updates (mcpt_scene_update_geometry) against a fresh upload, and what a
refitted tree costs the traversal against a rebuilt one.

Per config (device-built, PLOC), with a warp of 5 % of the scene's extent per step:
* wall time and the mcpt_debug_geometry_update_ms phases of a refit and of a rebuild, and beside them
  the wall time of a fresh mcpt_scene_upload_gpu_bvh of the same moved scene on a second context of the
  same process -- the three alternating, medians and ranges over REPS rounds after a warm-up round;
* k_trace's per-launch time (device events, over ITERS wavefront iterations) and the wall time of a
  4-spp frame on the refitted tree against the rebuilt one after 1, 8 and 32 accumulated warp steps,
  alternating, medians and ranges over REPS rounds.

usage: python tools/geom_update_bench.py [configs, default 2,4,5] [out.json, default profiles/geom_update.json]"""
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "mc-path-tracer_amd")]
import mcpt  # noqa: E402

F = np.float32
REPS, ITERS, AMP = 5, 12, 0.05
STEPS = (1, 8, 32)


def warp(v, ext, step):
    """One warp step: a wave along y of AMP x the extent, phase by step; a function of the position."""
    out = v.copy()
    out[:, 1] += F(AMP * ext) * np.sin(F(0.7 * step) + F(9.0 / ext) * (v[:, 0] + v[:, 2])).astype(F)
    return out


def stats(xs):
    xs = sorted(xs)
    return {"median": round(xs[len(xs) // 2], 4), "min": round(xs[0], 4), "max": round(xs[-1], 4)}


def moved_desc(scene, verts):
    d = scene.desc()
    d.v0, d.v1, d.v2 = (mcpt.fptr(v) for v in verts)
    d._verts = verts
    return d


def wall(fn, pt):
    pt._ck(mcpt.lib().mcpt_sync(pt.h))
    t = time.perf_counter()
    fn()
    pt._ck(mcpt.lib().mcpt_sync(pt.h))
    return (time.perf_counter() - t) * 1e3


def frame(pt):
    """(wall ms of a cleared 4-spp frame, k_trace ms per launch over ITERS iterations of a second one)."""
    pt.clear()
    ms = wall(pt.render, pt)
    pt.clear()
    st = pt.iterate(ITERS)
    return ms, st.ms_extend / ITERS


def main():
    configs = [int(x) for x in (sys.argv[1] if len(sys.argv) > 1 else "2,4,5").split(",")]
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(REPO, "profiles", "geom_update.json")
    out = []
    for c in configs:
        rc = mcpt.CONFIGS[c]
        scene = mcpt.build_config_scene(c)
        a = scene.arrays()
        base = [np.ascontiguousarray(a[k], F) for k in ("v0", "v1", "v2")]
        allv = np.concatenate(base)
        ext = float((allv.max(axis=0) - allv.min(axis=0)).max())
        cam = mcpt.config_camera(rc)
        pts = []
        for _ in range(2):  # [0]: updated in place; [1]: fresh uploads, then the rebuilt tree
            p = mcpt.PathTracer(0, mcpt.default_config(spp=4, max_depth=rc.max_depth))
            p.upload_scene(scene, gpu_bvh="ploc")
            p.set_camera(cam)
            p.resize(rc.width, rc.height)
            pts.append(p)
        pa, pb = pts
        info = pa.bvh_read()[2]
        r = {"config": c, "tris": int(info["ntri"]), "width": int(info["width"]), "depth": int(info["depth"]),
             "film": [rc.width, rc.height], "amplitude": AMP, "reps": REPS}
        m1 = [warp(v, ext, 1) for v in base]
        d1 = moved_desc(scene, m1)
        rows = {"refit": [], "rebuild": [], "fresh_upload": []}
        phases = {"refit": [], "rebuild": []}
        for rep in range(REPS + 1):  # round 0 warms up
            for mode in ("refit", "rebuild"):
                t = wall(lambda: pa.update_geometry(*m1, mode=mode), pa)
                if rep:
                    rows[mode].append(t)
                    phases[mode].append(pa.geometry_update_ms())
            t = wall(lambda: pb.upload_scene(d1, gpu_bvh="ploc"), pb)
            if rep:
                rows["fresh_upload"].append(t)
        r["wall_ms"] = {k: stats(v) for k, v in rows.items()}
        r["device_ms"] = {k: {ph: stats([x[ph] for x in v]) for ph in v[0]} for k, v in phases.items()}
        r["fresh_upload_build_ms"] = round(pb.last_build_ms, 3)
        # refitted against rebuilt after accumulated steps: pa refits every step, pb rebuilds at the step measured
        pa.upload_scene(scene, gpu_bvh="ploc")
        pa.set_camera(cam)
        cur, quality = base, {}
        for step in range(1, max(STEPS) + 1):
            cur = [warp(v, ext, step) for v in cur]
            pa.update_geometry(*cur)
            if step not in STEPS:
                continue
            pb.update_geometry(*cur, mode="rebuild")
            fr = {"refit": [], "rebuild": []}
            for rep in range(REPS + 1):
                for name, p in (("refit", pa), ("rebuild", pb)):
                    x = frame(p)
                    if rep:
                        fr[name].append(x)
            quality[str(step)] = {n: {"frame_ms": stats([x[0] for x in v]), "trace_ms_per_launch": stats([x[1] for x in v])}
                                  for n, v in fr.items()}
        r["after_steps"] = quality
        print(json.dumps(r), flush=True)
        out.append(r)
        for p in pts:
            p.close()
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    json.dump(out, open(out_path, "w"), indent=1)


if __name__ == "__main__":
    main()
