"""CPU checks of the env-map family (tests/env_maps.py): what each map reaches, by the
oracle's own tables and draws; the guided CDF search against the plain one in a stand-alone native program
(also built with the host sanitizers); and the host table builder on maps loaded from Radiance files written
here.  The device side of the same maps is tests/test_env_maps_gpu.py."""
import os
import struct
import subprocess

import numpy as np
import pytest

import env_maps as EM
from conftest import REPO
from stage_checks import _same

NDRAW = 20000


@pytest.fixture(scope="module")
def stage_arrays(mcpt_mod):
    """Config 1's stage scene (sphere, HRDI env light and one directional light)."""
    import stage_fixtures as sf

    a = sf.stage_scene(mcpt_mod, 1).arrays()
    assert len(a["dir_params"]) == 1  # two lights: half the choices are the env light
    return a


@pytest.fixture(scope="module")
def stage_flags(stage_arrays, oracle):
    """The flags of the 1024 material-stage paths test_env_maps_gpu.py runs (they do not depend on the map)."""
    import stage_fixtures as sf

    return sf.material_state(stage_arrays, oracle.trace_closest, n=1024)["flags"]


def test_family_is_complete_and_deterministic():
    for name, (W, H) in EM.SIZES.items():
        t = EM.make(name)
        assert t.shape == (H, W, 4) and t.dtype == np.float32 and not t.flags.writeable
    assert (EM.SIZES["odd"][0] * EM.SIZES["odd"][1]) % 4 != 0
    assert EM.SIZES["chunk_2731x3"][0] * EM.SIZES["chunk_2731x3"][1] == 8192 + 1
    assert EM.SIZES["chunk_8192x2"][0] * EM.SIZES["chunk_8192x2"][1] == 2 * 8192
    assert all(W * H < 16 for W, H in (EM.SIZES[k] for k in ("tiny_4x2", "tiny_3x3", "tiny_2x2")))
    for k in ("tiny_4x2", "tiny_3x3", "tiny_2x2", "const"):
        assert (EM.make(k)[..., :3] > 0).all()
    odd = EM.make("odd")
    assert 0.1 < (odd[..., :3] == 0).all(axis=2).mean() < 0.3
    assert (EM.make("negative")[..., :3] < 0).any()
    for k, col in (("sun_first", 0), ("sun_last", 63)):
        t = EM.make(k)
        assert np.count_nonzero(t) == 3 and (t[EM.SUN_ROW, col, :3] == 1e4).all()
    again = EM.make.__wrapped__("bands")
    assert np.array_equal(again, EM.make("bands"))


@pytest.mark.parametrize("name", EM.ACCEPTED)
def test_guide_expectation_from_the_oracle_tables(name):
    """Guides off for `negative` (unsorted rows), `zeros` (NaN marginal) and `w65536` (size), on for the rest:
    the rule of k_env_check and env_guides applied to the oracle's tables."""
    assert EM.guides_expected(name) == (name not in EM.GUIDES_OFF)
    t = EM.tables(name)
    kinds = EM.row_kinds(t)
    if name == "negative":
        assert EM._sorted_finite(t["marginal_y"]) and (kinds == "unsorted").sum() >= 3
        assert t["pdf"].min() < 0  # the map does what it is there for
    if name == "zeros":
        assert all(np.isnan(t[k]).all() for k in ("marginal_y", "conds_y", "pdf"))
    if name == "bands":
        assert (kinds == "nan").sum() == 12  # row 0, rows 11-19 and rows 31-32 of the filtered luminance
        assert np.flatnonzero(kinds == "nan").tolist() == [0] + list(range(11, 20)) + [31, 32]
    if name.startswith("sun"):
        assert (kinds == "nan").sum() == 30
    if name == "w65535":
        assert np.nanmax(t["conds_y"][1]) <= 1.0001  # upper_bound can reach 65535, the last 16-bit value
    print(name, {k: int((kinds == k).sum()) for k in ("nan", "sorted", "unsorted")})


def test_one_row_map_has_nan_tables():
    """H == 1: sin(pi * 0 / 1) = 0 in every term, so the reference's tables are NaN throughout (the upload refuses
    such a map: tests/test_env_maps_gpu.py)."""
    t = EM.tables("chunk_8193x1")
    assert all(np.isnan(t[k]).all() for k in ("marginal_y", "conds_y", "pdf"))


@pytest.mark.parametrize("fixed", [False, True], ids=["reference", "fixed"])
@pytest.mark.parametrize("name", EM.ACCEPTED)
def test_oracle_draws(oracle, stage_arrays, name, fixed):
    """20,000 uniform draws through or_env_dir: every direction is finite (a NaN row sends the search to
    column -1, never to a NaN direction), a draw in a NaN row lands in column -1, and or_env_pdf at a sampled
    direction is finite on the maps whose pdf table is (the reference's own self-check)."""
    W, H = EM.SIZES[name]
    t = EM.tables(name)
    ex, ey = EM.uniform_draws(NDRAW)
    x, y = EM.cells(oracle, t, ex, ey)
    assert x.min() >= -1 and x.max() <= W - 1 and y.min() >= 0 and y.max() <= H - 1
    kinds = EM.row_kinds(t)
    assert (x[kinds[y] == "nan"] == -1).all()
    d, pdf = oracle.env_draws(EM.scene_arrays(stage_arrays, name, given=True), ex, ey, fixed)
    assert np.isfinite(d).all()
    assert np.allclose(np.linalg.norm(d.astype(np.float64), axis=1), 1.0, atol=1e-5)
    if np.isfinite(t["pdf"]).all():
        assert np.isfinite(pdf).all()
    print(f"{name} fixed={fixed}: column -1 in {100 * (x == -1).mean():.1f} % of the draws, "
          f"unsorted rows {100 * (kinds[y] == 'unsorted').mean():.1f} %")
    if name == "tiny_4x2":
        assert (x == -1).all()  # row 0 only
    if name == "zeros":
        assert (x == -1).all() and (y == 0).all()  # y clamped from -1


@pytest.mark.parametrize("name,what,least", [("bands", "col-1", 0.05), ("sun_first", "col-1", 0.50),
                                             ("sun_last", "col-1", 0.50), ("negative", "unsorted", 0.25)])
def test_material_stage_samples_reach_what_the_map_is_for(oracle, stage_flags, name, what, least):
    """Of the env-light samples the 1024-path material stage draws, at least 5 % land in column -1 on `bands`,
    at least 50 % on `sun_*`, and at least 25 % in an unsorted conditional row on `negative`."""
    t = EM.tables(name)
    ex, ey, ids = EM.material_env_draws(oracle, stage_flags)
    assert 400 < len(ids) < 624  # about half of the 1024 light choices
    x, y = EM.cells(oracle, t, ex, ey)
    frac = (x == -1).mean() if what == "col-1" else (EM.row_kinds(t)[y] == "unsorted").mean()
    print(f"{name}: {what} in {100 * frac:.1f} % of {len(ids)} env samples")
    assert frac >= least


# ---------------------------------------------------------------------------------------------
def _write_lists(path):
    lists = []
    for name in EM.ACCEPTED:
        if not EM.guides_expected(name):
            continue
        t = EM.tables(name)
        lists.append(t["marginal_y"])
        lists.extend(t["conds_y"])
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(lists)))
        for v in lists:
            f.write(struct.pack("<i", len(v)))
            f.write(np.ascontiguousarray(v, "<f4").tobytes())
    return len(lists)


@pytest.mark.parametrize("exe", ["env_search_host", "env_search_host_san"])
def test_guided_search_equals_plain_search(tmp_path, exe):
    """upper_bound_guided against upper_bound (device/mcpt_core.hpp, compiled for the host) on the marginal and
    every conditional row of every map whose guides are on, at the bin edges, their float neighbours, 0, the
    largest float below 1 and the CDF's own values with their neighbours; once more under the host's address
    and undefined-behaviour sanitizers (a stand-alone program, run directly)."""
    subprocess.run(["make", f"tests/native/{exe}"], cwd=REPO, check=True, capture_output=True)  # built by `make all`
    path = os.path.join(REPO, "tests", "native", exe)
    n = _write_lists(tmp_path / "lists.bin")
    r = subprocess.run([path, str(tmp_path / "lists.bin")], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    last = r.stdout.strip().splitlines()[-1].split()
    assert last[0] == f"lists={n}" and last[2] == "bad=0" and int(last[1].split("=")[1]) > 3000 * n


# ---------------------------------------------------------------------------------------------
def rgbe_encode(rgb):
    """(H, W, 3) non-negative float32 -> (H, W, 4) uint8 RGBE (Radiance's float2rgbe)."""
    rgb = np.asarray(rgb, np.float64)
    m = rgb.max(axis=2)
    f, e = np.frexp(m)
    with np.errstate(all="ignore"):
        s = np.where(m > 1e-32, f * 256.0 / m, 0.0)
    out = np.zeros(rgb.shape[:2] + (4,), np.uint8)
    out[..., :3] = np.floor(rgb * s[..., None]).astype(np.uint8)
    out[..., 3] = np.where(m > 1e-32, e + 128, 0).astype(np.uint8)
    return out


def rgbe_decode(b):
    """What RGBE bytes hold (stb_image's rgb * 2^(e - 136), 0 when e == 0), with the alpha the loader pads."""
    ex = b[..., 3].astype(np.int32)
    f = np.where(ex > 0, np.ldexp(np.float32(1.0), ex - 136), 0).astype(np.float32)
    out = np.zeros(b.shape, np.float32)
    out[..., :3] = b[..., :3].astype(np.float32) * f[..., None]
    return out


def _rle(chan):
    out, x, n = bytearray(), 0, len(chan)
    while x < n:
        r = 1
        while x + r < n and r < 127 and chan[x + r] == chan[x]:
            r += 1
        if r >= 3:
            out += bytes([128 + r, chan[x]])
            x += r
            continue
        s = x
        while x < n and x - s < 128:
            if x + 2 < n and chan[x] == chan[x + 1] == chan[x + 2]:
                break
            x += 1
        out += bytes([x - s]) + bytes(chan[s:x].tolist())
    return bytes(out)


def write_hdr(path, b, rle):
    H, W = b.shape[:2]
    with open(path, "wb") as f:
        f.write(b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n" + f"-Y {H} +X {W}\n".encode())
        for y in range(H):
            if not rle:
                f.write(b[y].tobytes())
                continue
            f.write(bytes([2, 2, W >> 8, W & 255]))
            for c in range(4):
                f.write(_rle(b[y, :, c]))


@pytest.mark.parametrize("device_tables", [False, True], ids=["host_tables", "device_tables"])
@pytest.mark.parametrize("name,rle", [("odd", True), ("odd", False), ("bands", True), ("tiny_3x3", False)])
def test_host_table_builder_on_maps_loaded_from_hdr(mcpt_mod, oracle, tmp_path, name, rle, device_tables):
    """Scene.set_env_hdr on a Radiance file written here (new-style RLE scanlines, or flat where the map is
    narrower than 8 texels or for variety): the texture is what the RGBE bytes hold (and what the independent
    decoder of tests/test_oracle.py reads from the RLE files), and the host-built tables equal the oracle's
    or_env_build of that texture bit for bit; with device_tables the scene keeps the texture alone."""
    from test_oracle import decode_hdr_py

    b = rgbe_encode(EM.make(name)[..., :3])
    q = rgbe_decode(b)
    assert rle == (rle and b.shape[1] >= 8)
    path = tmp_path / f"{name}.hdr"
    write_hdr(path, b, rle)
    s = mcpt_mod.Scene()
    s.make_proxy(1)
    s.set_env_hdr(path, 1, device_tables=device_tables)
    s.build(8)
    a = s.arrays()
    assert a["env_mode"] == 1 and a["env_tex"].shape == q.shape
    assert np.array_equal(a["env_tex"].view(np.uint32), q.view(np.uint32))
    if rle:
        assert np.array_equal(a["env_tex"][..., :3], decode_hdr_py(path))
    if name == "bands":  # the black bands survive the encoding
        assert (q[10:20] == 0).all() and (q[:, 40:60] == 0).all()
    if device_tables:
        assert all(a["env_" + k].size == 0 for k in ("marginal_y", "conds_y", "pdf"))
        return
    ref = oracle.env_build(q)
    for k in ("marginal_y", "conds_y", "pdf"):
        assert _same(a["env_" + k].reshape(ref[k].shape), ref[k]), k
