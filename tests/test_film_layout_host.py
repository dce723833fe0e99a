"""The film-state sizing rules (csrc/host/film_layout.hpp) through the stand-alone program
tests/native/film_layout_host.cpp, without a device: every field of every fixed case recomputed here from
the formulas the context has always used, the limits with their messages, and one run of the same
program under the address and undefined-behaviour sanitizers.  No GPU."""
import os
import re
import subprocess

import pytest

from conftest import REPO

CSRC = os.path.join(REPO, "mc-path-tracer_amd", "csrc")
SRC = os.path.join(REPO, "tests", "native", "film_layout_host.cpp")
FLAGS = ["-O2", "-std=c++17", "-Wall", "-I", CSRC, "-I", os.path.join(REPO, "include")]
BLOCK, SHARDS = 256, 64  # kBlock, kShards (kernels.hpp)


def build_exe(path, extra=()):
    subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, *extra, SRC, "-o", path], check=True)
    return path


def run(exe):
    return subprocess.run([exe], check=True, timeout=60, capture_output=True, text=True).stdout


@pytest.fixture(scope="module")
def plain_output(tmp_path_factory):
    return run(build_exe(str(tmp_path_factory.mktemp("film_layout_host") / "film_layout_host")))


def parse(out):
    cases = {}
    for line in out.splitlines():
        name, rest = line.split(" ", 1)
        f = dict(re.findall(r'(\w+)=("[^"]*"|\S+)', rest))
        f = {k: v.strip('"') if v.startswith('"') else v for k, v in f.items()}
        f["in"] = tuple(int(x) for x in f["in"].split(","))
        assert name not in cases
        cases[name] = f
    return cases


def ceil_div(a, b):
    return -(-a // b)


def expected(w, h, tw, th, slots, compact, ntiles, mult):
    """The rules as the context applied them before they had a header of their own."""
    if 0 in (w, h, tw, th):
        return {"size_error": "bad film size"}
    if w * h >= 2 ** 31:
        return {"size_error": "film too large"}
    if tw * th > 2 ** 26:
        return {"size_error": "tile too large"}
    nx, ny = ceil_div(w, tw), ceil_div(h, th)
    if ntiles < 0:
        ntiles = nx * ny
    per_tile = ceil_div(tw * th, BLOCK)
    ext_cap = max(1, ceil_div(ntiles * per_tile * slots, SHARDS)) * BLOCK
    npx = ntiles * tw * th if compact else w * h
    paths = npx * slots
    return {
        "ntiles": ntiles, "nx": nx, "ny": ny, "npix": w * h, "npx": npx, "paths": paths,
        "blocks_per_tile": per_tile * slots, "ext_cap": ext_cap, "any_cap": mult * ext_cap, "queue_need": SHARDS * ext_cap,
        "blk_done_n": slots * nx * ny * per_tile, "sum_planes": int(slots > 1 or bool(compact)),
        "one_tile_cap": max(1, ceil_div(per_tile * slots, SHARDS)) * BLOCK,
        "paths_error": "film too large for the path slots" if paths >= 2 ** 31 else "",
        "emitter_error": "film too large for emitter sampling" if 3 * paths >= 2 ** 32 else "",
    }


def check(out):
    cases = parse(out)
    for name, f in cases.items():
        want = expected(*f["in"])
        got = {k: (v if k.endswith("error") else int(v)) for k, v in f.items() if k != "in"}
        assert got == want, name
    return cases


def test_every_field_of_every_case(plain_output):
    c = check(plain_output)
    assert len(c) == 21
    # the cases by what they are there for (the program's list is fixed)
    assert c["empty_set"]["ext_cap"] == c["empty_set_compact"]["ext_cap"] == "256"  # never 0
    assert c["empty_set_compact"]["npx"] == c["empty_set_compact"]["paths"] == "0"
    assert c["one_pixel"]["in"][:4] == (1, 1, 1, 1) and c["one_pixel"]["blk_done_n"] == "1"
    assert c["ragged"]["in"][:4] == (33, 17, 16, 16) and (c["ragged"]["nx"], c["ragged"]["ny"]) == ("3", "2")
    assert c["slots_256"]["in"][4] == 256
    assert c["mult_2"]["in"][7] == 2 and c["mult_3"]["in"][7] == 3
    assert int(c["mult_3"]["any_cap"]) * 2 == int(c["mult_2"]["any_cap"]) * 3 and c["mult_3"]["ext_cap"] == c["mult_2"]["ext_cap"]
    assert c["compact_subset"]["in"][5] == 1 and 0 < int(c["compact_subset"]["ntiles"]) < 4 * 2
    assert c["compact_subset"]["npx"] == str(3 * 64 * 64) and c["compact_subset"]["npix"] == str(200 * 120)
    # a 32 x 32 tile under 17 slots: 68 blocks, more than the empty tile set's one block per shard holds
    assert int(c["one_tile_17_slots"]["one_tile_cap"]) == 512 > int(c["empty_set"]["ext_cap"])


def test_limits_and_their_messages(plain_output):
    c = check(plain_output)
    assert c["paths_2p31_minus_1"]["paths"] == str(2 ** 31 - 1) and c["paths_2p31_minus_1"]["paths_error"] == ""
    for name in ("paths_2p31", "paths_2p31_compact"):
        assert c[name]["paths"] == str(2 ** 31) and c[name]["paths_error"] == "film too large for the path slots"
    assert 3 * int(c["emitter_below_2p32"]["paths"]) == 2 ** 32 - 1 and c["emitter_below_2p32"]["emitter_error"] == ""
    assert 3 * int(c["emitter_at_2p32"]["paths"]) >= 2 ** 32 > 3 * (int(c["emitter_at_2p32"]["paths"]) - 1)
    assert c["emitter_at_2p32"]["emitter_error"] == "film too large for emitter sampling"
    assert c["emitter_at_2p32"]["paths_error"] == ""
    assert c["film_2p31"]["in"][0] * c["film_2p31"]["in"][1] == 2 ** 31 and c["film_2p31"]["size_error"] == "film too large"
    t = c["tile_2p26"]["in"]
    assert t[2] * t[3] == 2 ** 26 and "size_error" not in c["tile_2p26"] and c["tile_2p26"]["blk_done_n"] == str(2 ** 18)
    t = c["tile_2p26_plus_1"]["in"]
    assert t[2] * t[3] == 2 ** 26 + 1 and c["tile_2p26_plus_1"]["size_error"] == "tile too large"
    assert c["zero_width"]["size_error"] == c["zero_tile"]["size_error"] == "bad film size"


def test_sanitized_build_runs_clean(plain_output, tmp_path):
    """The same program with the address and undefined-behaviour sanitizers on its host code (it has no
    device code), run directly: the same output, no report."""
    san = "-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all".split()
    exe = build_exe(str(tmp_path / "film_layout_host_san"), ["-g", *san])
    assert run(exe) == plain_output
