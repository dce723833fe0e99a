"""tools/kcode_diff.py and the file layout it guards: kernels.hip holds the wavefront
iteration's kernels and no other, and the tool reads every kernel of the built library without a GPU."""
import os
import re
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "mc-path-tracer_amd", "csrc")
ITERATION = {"k_shade", "k_material", "k_primary", "k_trace", "k_accumulate"}


def _kernels(name):
    src = open(os.path.join(CSRC, name)).read()
    return set(re.findall(r"^__global__.*?\bvoid (k_\w+)\(", src, flags=re.M))


def test_kernels_hip_holds_only_the_iteration():
    assert _kernels("kernels.hip") == ITERATION
    moved = _kernels("scene_tables.hip") | _kernels("film.hip")
    assert len(moved) == 18 and not (moved & ITERATION)  # 16 kernel families, k_cull_* counted as three


def test_library_compared_with_itself_is_all_same():
    lib = os.path.join(REPO, "mc-path-tracer_amd", "libmcpt.so")
    tool = os.path.join(REPO, "tools", "kcode_diff.py")
    r = subprocess.run([sys.executable, tool, lib, lib, "mcpt_dev"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert all(l.startswith("same") for l in lines[:-1]) and re.fullmatch(r"(\d+) kernels, \1 same, 0 not", lines[-1])
    for k in ITERATION | {"k_occ_complete", "k_primary_build", "k_copy"}:
        assert any(f"{k}E" in l or f"{k}I" in l for l in lines), k
    # a name no kernel has: nothing compared is not a pass
    r = subprocess.run([sys.executable, tool, lib, lib, "no_such_kernel"], capture_output=True, text=True)
    assert r.returncode == 1
