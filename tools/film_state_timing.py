#!/usr/bin/env python3
"""Host wall time of the film-state transitions (csrc/film_state.cpp) on a 1920x1080 film: 200 calls of
resize alternating between two film sizes and 200 calls of set_tiles alternating between two tile
subsets, each call synchronous.  Prints one JSON line.  MCPT_LIB selects another build of the library,
so two builds are compared by running this once per build, alternating (one library per process).

    python tools/film_state_timing.py [--calls 200]
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "mc-path-tracer_amd"))

import mcpt  # noqa: E402
from mcpt import parallel  # noqa: E402


def timed(n, call, args):
    t0 = time.perf_counter()
    for i in range(n):
        call(*args[i % 2])
    return (time.perf_counter() - t0) * 1e3 / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    a = ap.parse_args()
    W, H, T = 1920, 1080, 256
    pt = mcpt.PathTracer(0, mcpt.default_config(spp=1, max_depth=2))
    sizes = [(1280, 720, 128, 128), (W, H, T, T)]
    timed(4, pt.resize, sizes)  # warm-up: first allocations
    resize_ms = timed(a.calls, pt.resize, sizes)  # ends at W x H
    subsets = [(parallel.tiles_for_rank(0, 2, W, H, T),), (parallel.tiles_for_rank(1, 3, W, H, T),)]
    timed(4, pt.set_tiles, subsets)
    tiles_ms = timed(a.calls, pt.set_tiles, subsets)
    pt.set_compact_paths(True)
    compact_tiles_ms = timed(a.calls, pt.set_tiles, subsets)  # compact: re-allocates the path state and clears
    pt.close()
    print(json.dumps({"lib": os.environ.get("MCPT_LIB", "libmcpt.so"), "calls": a.calls, "resize_ms_per_call": round(resize_ms, 4),
                      "set_tiles_ms_per_call": round(tiles_ms, 4), "set_tiles_compact_ms_per_call": round(compact_tiles_ms, 4)}))


if __name__ == "__main__":
    main()
