"""CPU model of the occluder table's complete keys: for sampled any-hit rays of a
BASELINE config, the length of their key's conservative candidate list, from the product's own builder
(device/occ_beam.hpp occ_key_list, compiled for the host as tools/occ_list_model.cpp), and the
ray-weighted share of keys with at most N candidates, split by the rays' outcome (CPU oracle any-hit
trace).  A key with at most kOccWays candidates is complete: its rays leave the traversal.

The rays are path-like but not the renderer's: surface points are drawn by area, each shoots a light ray
(uniform direction, origin p + 0.01 n) and a BRDF visibility ray (cosine-weighted, origin p + 0.001 wi) as
k_material offsets them, and walks on along a cosine-weighted direction for --bounces vertices.  No GPU.
Usage: python tools/occ_list_model.py [--config 2] [--points 20000] [--bounces 2] [--grid 24] [--bins 12]"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "mc-path-tracer_amd"))
sys.path.insert(0, os.path.join(REPO, "oracle"))


def helper():
    exe, src = os.path.join(REPO, "tools", "occ_list_model"), os.path.join(REPO, "tools", "occ_list_model.cpp")
    hdr = os.path.join(REPO, "mc-path-tracer_amd", "csrc", "device", "occ_beam.hpp")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        subprocess.run([hipcc, "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-I" + os.path.join(REPO, "include"),
                        "-I" + os.path.join(REPO, "mc-path-tracer_amd", "csrc"), src, "-o", exe], check=True)
    return exe


def unit(v):
    return v / np.maximum(np.linalg.norm(v, axis=1, keepdims=True), 1e-30)


def cosine_dirs(rng, n):
    """cosine-weighted directions around the unit normals n"""
    u1, u2 = rng.random(len(n)), rng.random(len(n))
    r, ph = np.sqrt(u1), 2 * np.pi * u2
    a = np.where(np.abs(n[:, :1]) > 0.9, np.array([[0.0, 1.0, 0.0]]), np.array([[1.0, 0.0, 0.0]]))
    t = unit(np.cross(a, n))
    b = np.cross(n, t)
    return unit(t * (r * np.cos(ph))[:, None] + b * (r * np.sin(ph))[:, None] + n * np.sqrt(1 - u1)[:, None])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=2)
    ap.add_argument("--points", type=int, default=20000)
    ap.add_argument("--bounces", type=int, default=2)
    ap.add_argument("--grid", type=int, default=24)
    ap.add_argument("--bins", type=int, default=12)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    import mcpt
    import oracle_py

    arr = mcpt.build_config_scene(a.config).arrays()
    v0, v1, v2 = (np.asarray(arr[k], np.float32).reshape(-1, 3) for k in ("v0", "v1", "v2"))
    rng = np.random.default_rng(a.seed)
    nrm = np.cross(v1 - v0, v2 - v0).astype(np.float64)
    area = 0.5 * np.linalg.norm(nrm, axis=1)
    tri = rng.choice(len(v0), a.points, p=area / area.sum())
    s, t = rng.random(a.points), rng.random(a.points)
    fl = s + t > 1
    s[fl], t[fl] = 1 - s[fl], 1 - t[fl]
    p = (v0[tri] + (v1[tri] - v0[tri]) * s[:, None] + (v2[tri] - v0[tri]) * t[:, None]).astype(np.float64)
    n = unit(nrm[tri])
    nth = oracle_py.default_threads()
    ros, rds = [], []
    for b in range(a.bounces + 1):
        ld = unit(rng.normal(size=p.shape))
        wi = cosine_dirs(rng, n)
        ros += [p + 0.01 * n, p + 0.001 * wi]
        rds += [ld, wi]
        if b == a.bounces:
            break
        wo = cosine_dirs(rng, n)
        pos_t, hn, ht = oracle_py.trace_closest(arr, p + 0.001 * n, wo, nthreads=nth)
        hit = ht >= 0
        p, wo = pos_t[hit, :3].astype(np.float64), wo[hit]
        n = unit(hn[hit, :3].astype(np.float64))
        n = np.where((np.sum(n * wo, axis=1) > 0)[:, None], -n, n)  # facing the arriving ray
    ro, rd = np.concatenate(ros).astype(np.float32), np.concatenate(rds).astype(np.float32)
    vis = oracle_py.trace_any(arr, ro, rd, nthreads=nth)
    with tempfile.TemporaryDirectory() as td:
        fi, fo = os.path.join(td, "in.bin"), os.path.join(td, "out.bin")
        with open(fi, "wb") as f:
            np.array([len(arr["nprims"]), len(v0), a.grid, a.bins, len(ro)], np.int32).tofile(f)
            for k in ("bmin", "bmax"):
                np.ascontiguousarray(arr[k], np.float32).tofile(f)
            for k in ("offset", "nprims"):
                np.ascontiguousarray(arr[k], np.int32).tofile(f)
            for x in (v0, v1, v2, ro, rd):
                np.ascontiguousarray(x, np.float32).tofile(f)
        subprocess.run([helper(), fi, fo], check=True)
        cnt = np.fromfile(fo, np.int32)
    print(f"config {a.config}: {len(ro)} any-hit rays, {100.0 * np.mean(vis == 1):.1f} % unoccluded; "
          f"{100.0 * np.mean(cnt == -2):.2f} % outside their key's beam or without a positive culling scale")
    print("| rays | <= 0 | <= 2 | <= 4 | <= 6 | <= 8 |")
    print("|---|---|---|---|---|---|")
    for name, sel in (("unoccluded", vis == 1), ("occluded", vis == 0)):
        c = cnt[sel]
        row = [np.mean((c >= 0) & (c <= k)) if len(c) else 0.0 for k in (0, 2, 4, 6, 8)]
        print(f"| {name} ({len(c)}) | " + " | ".join(f"{x:.3f}" for x in row) + " |")
    bad = int(np.sum((cnt == 0) & (vis == 0)))
    print(f"occluded rays with an empty list: {bad} (must be 0)")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
