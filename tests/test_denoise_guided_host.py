"""Host build of the variance-guided filter's arithmetic (device/denoise.hpp,
tests/native/denoise_guided_host.cpp) against the numpy float32 restatement
(tests/denoise_guided_ref.py) bit for bit, the properties the specification implies, its effect on a
heteroscedastic image, and one run under the address and undefined-behaviour sanitizers.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import denoise_guided_ref as G
import denoise_ref as R
from conftest import REPO

f32 = np.float32
SRC = os.path.join(REPO, "tests", "native", "denoise_guided_host.cpp")
FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-I", os.path.join(REPO, "mc-path-tracer_amd", "csrc"),
         "-I", os.path.join(REPO, "include")]


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("denoise_guided_host") / "denoise_guided_host")
    subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, SRC, "-o", exe], check=True)
    return exe


def host_filter(exe, tmp, inp, passes, use_samples=True, env=None, **par):
    H, W = inp["depth"].shape
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as f:
        for k, dt in (("rgb", f32), ("samples", np.uint32), ("variance", f32), ("albedo", f32), ("normal", f32),
                      ("depth", f32)):
            f.write(np.ascontiguousarray(inp[k], dt).tobytes())
    s = [repr(float(f32(par[k]))) for k in ("sigma_lum", "lum_eps", "sigma_color", "sigma_normal", "sigma_albedo",
                                            "sigma_depth")]
    subprocess.run([exe, str(W), str(H), str(passes), *s, "1" if use_samples else "0", fin, fout], check=True, timeout=120,
                   env=env)
    out = np.fromfile(fout, f32)
    return out[:3 * W * H].reshape(H, W, 3), out[3 * W * H:].reshape(H, W)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, f32).view(np.uint32), np.ascontiguousarray(b, f32).view(np.uint32))


def ref_filter(inp, passes, **par):
    return G.denoise_guided(inp["rgb"], inp["variance"], inp["albedo"], inp["normal"], inp["depth"], inp["samples"],
                            passes=passes, **par)


PAR = dict(R.SIGMAS, **G.GUIDED)


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("passes", R.PASSES)
def test_host_filter_matches_numpy(host_exe, tmp_path, shape, passes):
    inp = G.make_inputs(*shape)
    got, got_v = host_filter(host_exe, str(tmp_path), inp, passes, **PAR)
    ref, ref_v = ref_filter(inp, passes, **PAR)
    assert same_bits(got, ref) and same_bits(got_v, ref_v)
    _, valid, _ = R.planes(inp["rgb"], inp["samples"], inp["normal"], inp["albedo"], inp["depth"])
    with np.errstate(all="ignore"):
        known = valid & (inp["variance"] >= 0) & (inp["variance"] <= R.FLT_MAX)
    assert np.all(got[~valid] == 0)
    # (c) a known variance stays finite and non-negative; an unknown one stays unknown
    assert np.all(np.isfinite(got_v[known]) & (got_v[known] >= 0))
    assert np.all(got_v[~known] == -1)
    # what an invalid pixel's colour or variance holds never reaches a valid pixel (the pixels are kept
    # invalid through their sample count: a finite colour alone would make them valid)
    for junk in (np.nan, 1e30):
        alt = dict(inp)
        alt["samples"] = np.where(valid, inp["samples"], 0).astype(np.uint32)
        alt["rgb"] = np.where(valid[..., None], inp["rgb"], f32(junk)).astype(f32)
        alt["variance"] = np.where(valid, inp["variance"], f32(junk)).astype(f32)
        alt_out, alt_v = host_filter(host_exe, str(tmp_path), alt, passes, **PAR)
        assert same_bits(alt_out[valid], got[valid]) and same_bits(alt_v[valid], got_v[valid])


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_without_a_variance_it_is_the_plain_filter(host_exe, tmp_path, shape):
    """(a) every variance unknown: the plain filter's colours, bit for bit."""
    inp = G.make_inputs(*shape)
    inp["variance"] = np.full(inp["depth"].shape, -1.0, f32)
    for passes in (1, 3):
        got, got_v = host_filter(host_exe, str(tmp_path), inp, passes, **PAR)
        assert same_bits(got, R.denoise(inp["rgb"], inp["albedo"], inp["normal"], inp["depth"], inp["samples"],
                                        passes=passes, **R.SIGMAS))
        assert np.all(got_v == -1)


def all_known(inp):
    """The inputs with every variance known: the unknown and NaN entries replaced, the zeros kept."""
    out = dict(inp)
    with np.errstate(all="ignore"):
        bad = ~(inp["variance"] >= 0)
    out["variance"] = np.where(bad, f32(1.5), inp["variance"]).astype(f32)
    return out


@pytest.mark.parametrize("k", [-7, 5])
def test_power_of_two_scaling_is_exact_without_eps(host_exe, tmp_path, k):
    """(b) lum_eps = 0 and every variance known: colours x 2^k and variances x 4^k scale the outputs
    exactly (a zero variance gives rcp = +Inf: only the centre tap has weight)."""
    inp = all_known(G.make_inputs(67, 35))
    assert (inp["variance"] == 0).any()
    par = dict(PAR, lum_eps=0.0)
    base, base_v = host_filter(host_exe, str(tmp_path), inp, 3, **par)
    sc = dict(inp)
    sc["rgb"] = (inp["rgb"] * f32(2.0 ** k)).astype(f32)
    sc["variance"] = (inp["variance"] * f32(4.0 ** k)).astype(f32)
    got, got_v = host_filter(host_exe, str(tmp_path), sc, 3, **par)
    assert same_bits(got, base * f32(2.0 ** k))
    assert same_bits(got_v, np.where(base_v >= 0, base_v * f32(4.0 ** k), f32(-1)))


def test_a_converged_pixel_is_left_alone(host_exe, tmp_path):
    """Zero variance everywhere with lum_eps = 0: the image comes back unchanged (to the rounding of
    w c / w), with variance 0."""
    inp = G.make_inputs(33, 9, dirty=False)
    inp["variance"] = np.zeros((9, 33), f32)
    got, got_v = host_filter(host_exe, str(tmp_path), inp, 3, **dict(PAR, lum_eps=0.0))
    assert np.all(np.abs(got - inp["rgb"]) <= np.abs(inp["rgb"]) * f32(2.0 ** -22)) and np.all(got_v == 0)


def test_heteroscedastic_image_beats_the_plain_filter(host_exe, tmp_path):
    """A checkerboard with a 5x brightness step and noise of 2 % (top) / 30 % (bottom) of the mean: one
    absolute sigma_color cannot fit both halves and both brightness levels, the variance can."""
    inp, clean = G.heteroscedastic()
    off = dict(sigma_normal=0.0, sigma_albedo=0.0, sigma_depth=0.0)
    guided, _ = host_filter(host_exe, str(tmp_path), inp, 5, sigma_color=2.0, **G.GUIDED, **off)
    unknown = dict(inp, variance=np.full(inp["depth"].shape, -1.0, f32))
    plain, _ = host_filter(host_exe, str(tmp_path), unknown, 5, sigma_color=2.0, **G.GUIDED, **off)
    assert same_bits(plain, R.denoise(inp["rgb"], inp["albedo"], inp["normal"], inp["depth"], inp["samples"], passes=5,
                                      sigma_color=2.0, **off))
    mse = [float(np.mean((a.astype(np.float64) - clean) ** 2)) for a in (inp["rgb"], plain, guided)]
    print(f"heteroscedastic 96x64: MSE raw {mse[0]:.4g}, plain {mse[1]:.4g}, guided {mse[2]:.4g}")
    assert mse[2] < mse[1]


def test_sanitized_build_runs_clean(tmp_path):
    """The stand-alone program once more with the address and undefined-behaviour sanitizers on its host
    code (it has no device code), on the 67 x 35 case: same bits, no report."""
    exe = str(tmp_path / "denoise_guided_host_san")
    san = "-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all".split()
    subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, "-g", *san, SRC, "-o", exe], check=True)
    inp = G.make_inputs(67, 35)
    got, got_v = host_filter(exe, str(tmp_path), inp, 3, **PAR)
    ref, ref_v = ref_filter(inp, 3, **PAR)
    assert same_bits(got, ref) and same_bits(got_v, ref_v)
