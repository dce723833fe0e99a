"""sRGB base colour on the CPU: the decode table of device/srgb_table.hpp against numpy
and libm, the lookup of device/texture.hpp compiled for the host against tests/texture_srgb_ref.py, the reference
against texture_nrm_ref and texture_ref, and the host scene builder's flag.  No GPU."""
import math
import os
import subprocess

import numpy as np
import pytest

import texture_nrm_ref as NR
import texture_ref as TR
import texture_srgb_ref as SR
from conftest import REPO

W, H, SPP = 24, 16, 4
F = np.float32
RAYS = ("extend_rays", "shadow_rays", "vis_rays")


def u32(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def same(f, g):
    return np.array_equal(u32(f[0]), u32(g[0])) and np.array_equal(f[1], g[1]) and all(f[2][k] == g[2][k] for k in RAYS)


def changed(f, g):
    return int((f[0] != g[0]).any(axis=2).sum())


@pytest.fixture(scope="module")
def exe():
    subprocess.run(["make", "tests/native/srgb_table_host"], cwd=REPO, check=True, capture_output=True)  # built by `make all`
    return os.path.join(REPO, "tests", "native", "srgb_table_host")


@pytest.fixture(scope="module")
def c2(mcpt_mod, scene_c2):
    s, a = scene_c2
    g, sets = SR.fixture(a)
    return dict(a=g, cam=mcpt_mod.config_camera(mcpt_mod.CONFIGS[2], W, H), **sets)


_FILM = {}


def film(oracle, c2, which, fixed=False, depth=5):
    key = (which, fixed, depth)
    if key not in _FILM:
        _FILM[key] = SR.render(oracle, c2["a"], c2["cam"], W, H, SPP, max_depth=depth, fixed=fixed, tex=c2[which] if which else None)
    return _FILM[key]


# ---------------------------------------------------------------------------------------------
# 1. the table
def test_table_properties():
    """Strictly increasing, L[0] == 0, L[255] == 1, bytes 0..10 on the linear branch and 11..255 on the power
    branch; libm's double pow gives numpy's 256 floats; and no double value lies nearer than 0.003 ulp to a float
    rounding midpoint (the nearest is byte 70 at 0.004), so the literal does not depend on the libm."""
    L = SR.table()
    assert L.dtype == np.float32 and L[0] == 0 and L[255] == 1 and (np.diff(L) > 0).all()
    x = np.arange(256) / 255.0
    assert x[10] <= 0.04045 < x[11]
    assert np.array_equal(L[:11], (x[:11] / 12.92).astype(F))
    libm = np.array([v / 12.92 if v <= 0.04045 else math.pow((v + 0.055) / 1.055, 2.4) for v in x]).astype(F)
    assert np.array_equal(u32(libm), u32(L))
    d = np.where(x <= 0.04045, x / 12.92, ((x + 0.055) / 1.055) ** 2.4)[1:255]
    lo = d.astype(F)
    ulp = np.spacing(np.minimum(lo, np.nextafter(lo, F(0))).astype(F)).astype(np.float64)  # the binade's spacing
    frac = np.abs(d - lo.astype(np.float64)) / ulp  # 0 .. 0.5: the distance to the float chosen
    near = 0.5 - frac
    k = int(np.argmin(near))
    print(f"nearest to a rounding midpoint: byte {k + 1} at {near[k]:.4f} ulp")
    assert near.min() > 0.003 and k + 1 == 70


def test_the_librarys_table_is_numpys(exe):
    """The 256 literals of device/srgb_table.hpp as the compiled lookup reads them."""
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    got = np.array([int(t, 16) for t in out], np.uint32)
    assert len(got) == 256 and np.array_equal(got, u32(SR.table()))


def _host_lookup(exe, tmp, img, uv, srgb):
    im = np.ascontiguousarray(img, np.uint8)
    uv = np.ascontiguousarray(uv, F).reshape(-1, 2)
    with open(tmp / "in.bin", "wb") as f:
        f.write(np.array([im.shape[1], im.shape[0], srgb, len(uv)], np.int32).tobytes())
        f.write(im.tobytes())
        f.write(uv.tobytes())
    subprocess.run([exe, str(tmp / "in.bin"), str(tmp / "out.bin")], check=True)
    return np.fromfile(tmp / "out.bin", F).reshape(-1, 3)


def special_uvs(rng, n):
    uv = (rng.random((n, 2)) * 6 - 3).astype(F)
    uv[:8] = [[np.nan, 0.3], [0.3, np.nan], [65536.0, 0.2], [0.2, -65536.0], [np.inf, -np.inf], [65535.996, -65535.996], [0.0, 1.0], [-0.0, 0.5]]
    return uv


def test_the_compiled_lookup_equals_the_reference(exe, tmp_path):
    """tex_bilinear_rgba8_srgb on the host against texture_srgb_ref.lookup, bit for bit: decoded and (flag off, and
    through tex_bilinear_rgba8 itself) undecoded, over 1 x 1, 5 x 3 and 8 x 8 images holding bytes 0, 10, 11 and
    255, at random uvs and at NaN and >= 65536 coordinates; and every byte at exact texel centres gives L[c]."""
    rng = np.random.default_rng(2)
    for h, w in ((1, 1), (3, 5), (8, 8)):
        img = rng.integers(0, 256, (h, w, 4)).astype(np.uint8)
        img.reshape(-1)[:4] = [0, 10, 11, 255]
        uv = special_uvs(rng, 600)
        assert np.array_equal(u32(_host_lookup(exe, tmp_path, img, uv, 1)), u32(SR.lookup(img, uv, SR.table())))
        for off in (0, 2):
            assert np.array_equal(u32(_host_lookup(exe, tmp_path, img, uv, off)), u32(TR.lookup(img, uv)))
    img = np.arange(256, dtype=np.uint8).reshape(16, 16, 1).repeat(4, axis=2)
    img[..., 1] = img[..., 0][::-1, ::-1]
    jj, ii = np.meshgrid(np.arange(16), np.arange(16), indexing="ij")
    uv = np.stack([(ii + 0.5) / 16, (jj + 0.5) / 16], -1).reshape(-1, 2).astype(F)
    got = _host_lookup(exe, tmp_path, img, uv, 1)
    L = SR.table()
    assert np.array_equal(u32(got[:, 0]), u32(L[np.arange(256)])) and np.array_equal(u32(got[:, 1]), u32(L[255 - np.arange(256)]))


def test_lookup_under_byte_over_255_is_texture_refs():
    rng = np.random.default_rng(3)
    for h, w in ((1, 1), (3, 5), (8, 8), (6, 7)):
        img = rng.integers(0, 256, (h, w, 4)).astype(np.uint8)
        uv = special_uvs(rng, 500)
        assert np.array_equal(u32(SR.lookup(img, uv, SR.unorm_table())), u32(TR.lookup(img, uv)))
    assert np.array_equal(u32(SR.unorm_table()), u32(TR.texels(np.arange(256, dtype=np.uint8).reshape(1, 256, 1).repeat(3, 2))[0, :, 0]))


# ---------------------------------------------------------------------------------------------
# 2. the reference film
@pytest.mark.parametrize("fixed", [False, True])
def test_without_a_flag_in_use_the_loop_is_texture_nrm_refs(oracle, c2, fixed):
    """No tex_flags, all 0, or a flag on the texture only normal slots use: texture_nrm_ref.render bit for bit."""
    want = NR.render(oracle, c2["a"], c2["cam"], W, H, SPP, fixed=fixed, tex=c2["all"])
    assert same(film(oracle, c2, "all", fixed), want)
    zero = dict(c2["all"], tex_flags=np.zeros(3, np.uint32))
    assert same(SR.render(oracle, c2["a"], c2["cam"], W, H, SPP, fixed=fixed, tex=zero), want)
    assert same(film(oracle, c2, "srgb_unused", fixed), want)


@pytest.mark.parametrize("depth", [5, 2])
@pytest.mark.parametrize("fixed", [False, True])
def test_the_flag_changes_more_than_100_pixels(oracle, c2, fixed, depth):
    """The guard the device tests rely on, for the reference alone (DESIGN.md section 22 records the counts): the
    flag changes the film of the base + MR + normal set, and of the base-only set, in more than 150 of the 384
    pixels, and every film is finite."""
    f = {k: film(oracle, c2, k, fixed, depth) for k in ("all", "srgb", "base", "srgb_base")}
    n_all, n_base = changed(f["srgb"], f["all"]), changed(f["srgb_base"], f["base"])
    print(f"fixed={fixed} depth={depth}: pixels changed by the sRGB flag on base + MR + normal {n_all}, on base only {n_base}")
    assert all(np.isfinite(x[0]).all() for x in f.values())
    assert n_all >= 150 and n_base >= 150


def test_mr_and_normal_lookups_never_decode(oracle, c2):
    """Images 0 and 1 serve as base colours and, on other materials, as MR textures: with both flagged, the
    exploded scene's roughness, metallic and normals are those of the unflagged set, and only the base colours of
    paths on flagged materials differ."""
    import stage_fixtures as sf

    a, flagged, plain = c2["a"], c2["srgb"], c2["all"]
    inp = sf.material_state(a, oracle.trace_closest, 2, 512)
    tri = np.asarray(inp["hit_tri"], np.int32)
    x, y = (f(a, t, tri, inp["ray_o"], inp["ray_d"]) for f, t in ((SR.exploded, flagged), (NR.exploded, plain)))
    for k in ("n0", "n1", "n2"):
        assert np.array_equal(u32(x[k]), u32(y[k]))
    assert np.array_equal(u32(x["mat_params"][:, 3:]), u32(y["mat_params"][:, 3:]))
    on = SR.flagged_materials(flagged, len(a["mat_params"]))[np.asarray(a["mat"])[tri]]
    assert on.any() and (~on).any()
    assert np.array_equal(u32(x["mat_params"][~on, :3]), u32(y["mat_params"][~on, :3]))
    assert (u32(x["mat_params"][on, :3]) != u32(y["mat_params"][on, :3])).any(axis=1).mean() > 0.9
    assert (np.asarray(flagged["mat_mr"])[np.asarray(a["mat"])[tri]] >= 0).any()


# ---------------------------------------------------------------------------------------------
# 3. the host scene builder
def test_scene_builder_carries_the_flag(mcpt_mod):
    s = mcpt_mod.Scene()
    v = [np.array([p], F) for p in ([0, 0, 0], [1, 0, 0], [0, 1, 0])]
    n = [np.array([[0, 0, 1]], F)] * 3
    s.add_mesh(*v, *n)
    s.add_mesh(*v, *n)
    img = np.full((2, 3, 4), 128, np.uint8)
    s.set_texture(0, img)
    assert "tex_flags" not in s.textures()  # an unflagged scene returns the keys it returned before
    s.set_texture(1, img, srgb=True)
    s.set_mr_texture(0, img)
    t = s.textures()
    assert np.array_equal(t["tex_flags"], np.array([0, mcpt_mod.MCPT_TEX_SRGB, 0], np.uint32)) and len(t["textures"]) == 3
    s.set_texture(1, img)  # replaced by an unflagged image
    assert "tex_flags" not in s.textures()
    rc = mcpt_mod.lib().mcpt_scene_set_material_texture_ex(s.h, 0, 3, 2, img.ctypes.data_as(mcpt_mod.C.POINTER(mcpt_mod.C.c_uint8)), 2)
    assert rc == -1


# ---------------------------------------------------------------------------------------------
# 4. the emitter-sampling reference
@pytest.mark.parametrize("mis", [False, True])
def test_render_emitters_without_a_set_is_emitter_mis_refs(oracle, c2, mis):
    """tex=None: emitter_mis_ref.render(sample=True) bit for bit, counts included; and the flagged base + MR set
    changes that film in more than 100 pixels."""
    import emission_ref as ER
    import emitter_mis_ref as XR

    a = ER.black(c2["a"])
    E = ER.table(len(a["mat_params"]), {ER.MATS_LIT[0]: (3.0, 2.0, 1.0), ER.MATS_LIT[1]: (0.5, 2.0, 8.0)})
    want = XR.render(oracle, a, c2["cam"], W, H, SPP, emission=E, sample=True, mis=mis)
    got = SR.render_emitters(oracle, a, c2["cam"], W, H, SPP, None, E, mis=mis)
    assert np.array_equal(u32(got[0]), u32(want[0])) and np.array_equal(got[1], want[1]) and got[2] == want[2]
    flagged = SR.render_emitters(oracle, a, c2["cam"], W, H, SPP, c2["srgb_both"], E, mis=mis)
    stored = SR.render_emitters(oracle, a, c2["cam"], W, H, SPP, c2["both"], E, mis=mis)
    n = changed(flagged, stored)
    print(f"mis={mis}: pixels changed by the sRGB flag under emitter sampling {n}")
    assert n > 100 and np.isfinite(flagged[0]).all()
