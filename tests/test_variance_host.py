"""Host build of the spatial variance estimate's arithmetic (device/variance.hpp,
tests/native/variance_host.cpp) against the numpy float32 restatement (tests/variance_ref.py) bit for
bit, with and without known input variances, the properties the specification implies, and one run under
the address and undefined-behaviour sanitizers.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import denoise_guided_ref as G
import denoise_ref as R
import variance_ref as V
from conftest import REPO

f32 = np.float32
SRC = os.path.join(REPO, "tests", "native", "variance_host.cpp")
FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-I", os.path.join(REPO, "mc-path-tracer_amd", "csrc"),
         "-I", os.path.join(REPO, "include")]


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("variance_host") / "variance_host")
    subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, SRC, "-o", exe], check=True)
    return exe


def host_variance(exe, tmp, inp, radius, known=False, use_samples=True, **par):
    H, W = inp["depth"].shape
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as f:
        for k, dt in (("rgb", f32), ("samples", np.uint32), ("variance", f32), ("albedo", f32), ("normal", f32),
                      ("depth", f32)):
            f.write(np.ascontiguousarray(inp[k], dt).tobytes())
    s = [repr(float(f32(par[k]))) for k in ("sigma_normal", "sigma_albedo", "sigma_depth", "min_neff")]
    subprocess.run([exe, str(W), str(H), str(radius), *s, "1" if use_samples else "0", "1" if known else "0", fin, fout],
                   check=True, timeout=120)
    return np.fromfile(fout, f32).reshape(H, W)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, f32).view(np.uint32), np.ascontiguousarray(b, f32).view(np.uint32))


def valid_of(inp):
    return R.planes(inp["rgb"], inp["samples"], inp["normal"], inp["albedo"], inp["depth"])[1]


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("radius", V.RADII)
def test_host_estimate_matches_numpy(host_exe, tmp_path, shape, radius):
    """make_inputs' dirty pixels: no samples, NaN / Inf colours, NaN normals, depth 0."""
    inp = G.make_inputs(*shape)
    got = host_variance(host_exe, str(tmp_path), inp, radius, **V.PARAMS)
    assert same_bits(got, V.run_ref(inp, radius=radius, **V.PARAMS))
    valid = valid_of(inp)
    assert np.all(got[~valid] == -1)
    known = got >= 0
    assert np.all((got == -1) | known) and np.all(np.isfinite(got))
    if shape == (67, 35):
        assert known.sum() > valid.sum() // 2  # the estimate exists on most of a frame


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("radius", V.RADII)
def test_known_variances_come_back_unchanged(host_exe, tmp_path, shape, radius):
    """Fill only: make_inputs' variance plane (about 10 % unknown, 2 % NaN, 5 % zero) as the known part."""
    inp = G.make_inputs(*shape)
    got = host_variance(host_exe, str(tmp_path), inp, radius, known=True, **V.PARAMS)
    assert same_bits(got, V.run_ref(inp, known=True, radius=radius, **V.PARAMS))
    valid = valid_of(inp)
    with np.errstate(all="ignore"):
        known = valid & (inp["variance"] >= 0) & (inp["variance"] <= R.FLT_MAX)
    assert same_bits(got[known], inp["variance"][known])
    assert np.all(got[~valid] == -1)
    # the rest is what the estimate gives without any known variance: it reads no neighbour's variance
    alone = host_variance(host_exe, str(tmp_path), inp, radius, **V.PARAMS)
    assert same_bits(got[~known], alone[~known])


def test_a_constant_image_has_variance_zero(host_exe, tmp_path):
    inp = G.make_inputs(33, 9)
    valid = valid_of(inp)
    inp["rgb"] = np.where(valid[..., None], f32([0.7, 1.3, 0.2]), inp["rgb"]).astype(f32)
    got = host_variance(host_exe, str(tmp_path), inp, 2, **V.PARAMS)
    assert np.all((got == 0) | (got == -1)) and (got == 0).sum() > valid.sum() // 2 and np.all(got[~valid] == -1)


@pytest.mark.parametrize("k", [-7, 5])
def test_power_of_two_scaling_is_exact(host_exe, tmp_path, k):
    inp = G.make_inputs(67, 35)
    base = host_variance(host_exe, str(tmp_path), inp, 3, **V.PARAMS)
    sc = dict(inp, rgb=(inp["rgb"] * f32(2.0 ** k)).astype(f32))
    got = host_variance(host_exe, str(tmp_path), sc, 3, **V.PARAMS)
    assert same_bits(got, np.where(base >= 0, base * f32(4.0 ** k), f32(-1)))


def test_min_neff_gates_the_estimate(host_exe, tmp_path):
    """An isolated pixel (every neighbour invalid) has neff = 1: unknown whatever min_neff is; a larger
    min_neff only removes estimates."""
    inp = G.make_inputs(33, 9, dirty=False)
    inp["samples"][:] = 0
    inp["samples"][4, 10] = 4
    inp["samples"][4:6, 20:22] = 4
    got = host_variance(host_exe, str(tmp_path), inp, 1, **dict(V.PARAMS, min_neff=1.0))
    assert got[4, 10] == -1
    inp = G.make_inputs(33, 9)
    lo = host_variance(host_exe, str(tmp_path), inp, 1, **dict(V.PARAMS, min_neff=1.5))
    hi = host_variance(host_exe, str(tmp_path), inp, 1, **dict(V.PARAMS, min_neff=4.0))
    assert np.all((hi == -1) | (hi == lo)) and (hi >= 0).sum() < (lo >= 0).sum()


def test_sanitized_build_runs_clean(tmp_path):
    """The stand-alone program once more with the address and undefined-behaviour sanitizers on its host
    code (it has no device code), on the 67 x 35 case at the widest radius: same bits, no report."""
    exe = str(tmp_path / "variance_host_san")
    san = "-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all".split()
    subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, "-g", *san, SRC, "-o", exe], check=True)
    inp = G.make_inputs(67, 35)
    got = host_variance(exe, str(tmp_path), inp, 3, known=True, **V.PARAMS)
    assert same_bits(got, V.run_ref(inp, known=True, radius=3, **V.PARAMS))
