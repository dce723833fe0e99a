"""Host build of the temporal stage's arithmetic (device/temporal.hpp, tests/native/temporal_host.cpp)
against the numpy float32 restatement (tests/temporal_ref.py) bit for bit in all five output planes, the
properties the specification implies (empty history, disocclusion, isolation, bounds), and one run
under the address and undefined-behaviour sanitizers.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import temporal_ref as T
from conftest import REPO

f32 = np.float32
SRC = os.path.join(REPO, "tests", "native", "temporal_host.cpp")
FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-I", os.path.join(REPO, "mc-path-tracer_amd", "csrc"),
         "-I", os.path.join(REPO, "include")]
NAMES = ("col", "vl", "hcol", "hpos", "hnrm")


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("temporal_host") / "temporal_host")
    subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, SRC, "-o", exe], check=True)
    return exe


def host_pass(exe, tmp, inp, **par):
    par = dict(T.PARAMS, **par)
    H, W = inp["depth"].shape
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as f:
        for k, dt in (("rgb", f32), ("samples", np.uint32), ("variance", f32), ("position", f32), ("normal", f32),
                      ("depth", f32), ("hcol", f32), ("hpos", f32), ("hnrm", f32), ("vp_prev", f32)):
            f.write(np.ascontiguousarray(inp[k], dt).tobytes())
    s = [repr(float(f32(par[k]))) for k in ("pos_tol", "nrm_tol", "max_history", "alpha_min")]
    subprocess.run([exe, str(W), str(H), *s, fin, fout], check=True, timeout=120)
    out = np.fromfile(fout, f32)
    n = W * H
    parts, o = [], 0
    for k in (4, 2, 4, 4, 4):
        parts.append(out[o:o + k * n].reshape(H, W, k))
        o += k * n
    assert o == out.size
    return tuple(parts)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, f32).view(np.uint32), np.ascontiguousarray(b, f32).view(np.uint32))


def assert_same(got, ref):
    for name, g, r in zip(NAMES, got, ref):
        assert same_bits(g, r), name


@pytest.mark.parametrize("shape", T.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_pass_matches_numpy(mcpt_mod, host_exe, tmp_path, shape):
    inp = T.make_inputs(mcpt_mod, *shape)
    got = host_pass(host_exe, str(tmp_path), inp)
    ref, d = T.run_ref(inp, detail=True)
    assert_same(got, ref)
    if shape[0] * shape[1] >= 16:
        # the inputs do exercise the paths: some pixels use the history, some do not, and the border
        # positions are rejected at and beyond row / column -1, accepted just inside, and tap the last
        # row / column (x0 = W - 1: the right-hand corners lie outside) or the one before
        valid = d["pixel"]["valid"]
        assert d["use"].any() and (valid & ~d["use"]).any() and (~valid).any()
        _, x0, y0, _, _ = T.project(inp["vp_prev"], d["pixel"], *shape)
        assert len(inp["edge"]) >= 8
        for k, which, want, side in inp["edge"]:
            ok, i0 = d["ok"].reshape(-1)[k], (x0 if which == "fx" else y0).reshape(-1)[k]
            if want == -1.0:
                assert ok == (side > 0) and (not ok or i0 == -1)
            else:
                assert ok and i0 == (want - 1 if side < 0 else want)
    # bounds
    col, vl, hcol, hpos, hnrm = got
    p = d["pixel"]
    par = T.PARAMS
    assert np.all(hcol[..., 3] <= f32(par["max_history"]) + p["s"])
    v = hpos[..., 3]
    kn = v != -1
    assert np.all(np.isfinite(v[kn]) & (v[kn] >= 0))
    unknown_tap = np.zeros(p["valid"].shape, bool)
    for k, acc in enumerate(d["accepted"]):
        dx, dy = k & 1, k >> 1
        ok_, x0, y0, _, _ = T.project(inp["vp_prev"], p, *shape)
        jx, jy = np.clip(x0 + dx, 0, shape[0] - 1), np.clip(y0 + dy, 0, shape[1] - 1)
        unknown_tap |= acc & d["use"] & ~T.known(inp["hpos"][jy, jx, 3])
    assert np.all(v[(p["vc"] == -1) | unknown_tap] == -1)
    assert same_bits(vl[..., 0], np.where(col[..., 3] != 0, v, f32(-1)))


@pytest.mark.parametrize("shape", T.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_an_empty_history_passes_the_frame_through(mcpt_mod, host_exe, tmp_path, shape):
    """N = 0 everywhere: the outputs are the current colour and v_c bit for bit, and N' = s."""
    inp = T.make_inputs(mcpt_mod, *shape)
    inp["hcol"][..., 3] = 0.0
    col, vl, hcol, hpos, hnrm = host_pass(host_exe, str(tmp_path), inp)
    p = T.pixel(inp["rgb"], inp["samples"], inp["variance"], inp["position"], inp["normal"], inp["depth"])
    assert same_bits(col[..., :3], p["col"]) and same_bits(col[..., 3], p["valid"].astype(f32))
    assert same_bits(hcol[..., :3], p["col"]) and same_bits(hcol[..., 3], p["s"])
    assert same_bits(hpos[..., 3], p["vc"]) and same_bits(vl[..., 0], p["vc"])
    assert np.array_equal(hcol[..., 3], np.where(p["valid"], inp["samples"], 0).astype(f32))


def test_disocclusion_is_the_uncovered_strip(mcpt_mod, host_exe, tmp_path):
    """A near plane (x <= 0) in front of a far wall, the previous camera 0.5 to the left: the move
    uncovers the far-wall points with 0 < x <= 1 (temporal_ref.disocclusion).  Those pixels leave as
    they came (N' = s, the current colour's bits); every other valid pixel gains history.  One pixel on
    either side of the two borders of the strip is left out of both claims: a bilinear tap reaches one
    pixel, so a pixel next to a border may or may not find an accepted corner."""
    W, H, shift = 64, 48, 0.5
    inp, x, far = T.disocclusion(mcpt_mod, W, H, shift)
    par = dict(pos_tol=0.05, nrm_tol=0.3, max_history=64.0, alpha_min=0.0)
    col, vl, hcol, hpos, hnrm = host_pass(host_exe, str(tmp_path), inp, **par)
    px = 2.0 * 6.0 * np.tan(np.radians(22.5)) * (W / H) / W      # a far-wall pixel's width
    s = inp["samples"].astype(f32)
    uncovered = far & (x > px) & (x <= 2 * shift - px)
    border = (np.abs(x) <= px) | (far & (np.abs(x - 2 * shift) <= px))
    # (the previous camera's film ends before the current one's does: what lies beyond has no history either)
    seen = T.project(inp["vp_prev"], T.pixel(inp["rgb"], inp["samples"], inp["variance"], inp["position"], inp["normal"],
                                             inp["depth"]), W, H)
    inside_prev = seen[0] & (seen[1] >= 0) & (seen[1] < W - 1) & (seen[2] >= 0) & (seen[2] < H - 1)
    assert 0 < uncovered.sum() < W * H // 4
    assert np.all(hcol[uncovered, 3] == s[uncovered])
    assert same_bits(col[uncovered][:, :3], inp["rgb"][uncovered]) and same_bits(hpos[uncovered][:, 3], inp["variance"][uncovered])
    rest = ~uncovered & ~border & inside_prev
    assert rest.sum() > W * H // 2 and np.all(hcol[rest, 3] > s[rest])


def test_what_is_rejected_never_reaches_an_output(mcpt_mod, host_exe, tmp_path):
    """Colour and variance of invalid pixels and of rejected history taps replaced by NaN or 1e30: no
    valid output bit changes."""
    inp = T.make_inputs(mcpt_mod, 67, 35)
    # (history pixels rejected for their NaN / Inf colour are kept rejected through their count, as the
    # invalid pixels below are through theirs: a finite 1e30 alone would make them acceptable)
    inp["hcol"][~np.all(np.isfinite(inp["hcol"][..., :3]), axis=2), 3] = 0.0
    base = host_pass(host_exe, str(tmp_path), inp)
    _, d = T.run_ref(inp, detail=True)
    p = d["pixel"]
    H, W = p["valid"].shape
    ok_, x0, y0, _, _ = T.project(inp["vp_prev"], p, W, H)
    touched = np.zeros((H, W), bool)  # history pixels some accepted corner reads
    for k, acc in enumerate(d["accepted"]):
        qx, qy = x0 + (k & 1), y0 + (k >> 1)
        m = acc & d["use"]
        touched[qy[m], qx[m]] = True
    assert touched.any() and (~touched).any()
    for junk in (np.nan, 1e30):
        alt = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in inp.items()}
        alt["samples"] = np.where(p["valid"], inp["samples"], 0).astype(np.uint32)  # kept invalid by their count
        alt["rgb"][~p["valid"]] = f32(junk)
        alt["variance"][~p["valid"]] = f32(junk)
        alt["hcol"][~touched, :3] = f32(junk)
        alt["hpos"][~touched, 3] = f32(junk)
        got = host_pass(host_exe, str(tmp_path), alt)
        assert_same(got, base)


def test_static_view_weights_like_one_longer_frame(mcpt_mod, host_exe, tmp_path):
    """The same camera twice, unclamped: N' = N + s and c' = h + s / (N + s) (c - h) on the pixels that
    reproject onto themselves."""
    W, H = 33, 9
    inp = T.make_inputs(mcpt_mod, W, H, dirty=False)
    cam = mcpt_mod.make_camera((0.15, 0.05, 4.0), -92.0, 1.0, aspect=f32(W) / f32(H), lens_radius=0.0)
    inp["vp_prev"] = mcpt_mod.camera_view_proj(cam)
    inp["hpos"][..., :3] = inp["position"]
    inp["hnrm"][..., :3] = inp["normal"]
    inp["hnrm"][..., 3] = inp["depth"]
    col, vl, hcol, hpos, hnrm = host_pass(host_exe, str(tmp_path), inp, pos_tol=0.01, max_history=1e6, alpha_min=0.0)
    s = inp["samples"].astype(f32)
    assert np.all(np.abs(hcol[..., 3] - (inp["hcol"][..., 3] + s)) <= 1e-4 * hcol[..., 3])
    want = inp["hcol"][..., :3] + (s / (inp["hcol"][..., 3] + s))[..., None] * (inp["rgb"] - inp["hcol"][..., :3])
    assert np.allclose(col[..., :3], want, rtol=1e-4, atol=1e-5)


def test_sanitized_build_runs_clean(mcpt_mod, tmp_path):
    """The stand-alone program once more with the address and undefined-behaviour sanitizers on its host
    code (it has no device code), on the 67 x 35 case: same bits, no report."""
    exe = str(tmp_path / "temporal_host_san")
    san = "-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all".split()
    subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, "-g", *san, SRC, "-o", exe], check=True)
    inp = T.make_inputs(mcpt_mod, 67, 35)
    assert_same(host_pass(exe, str(tmp_path), inp), T.run_ref(inp))
