"""Base-colour textures on the CPU: the reference of tests/texture_ref.py against the
oracle, and the host scene builder's uvs and textures.  No GPU."""
import ctypes as C
import json
import os
import struct

import numpy as np
import pytest

import texture_ref as TR
from conftest import ASSETS

W, H, SPP = 24, 16, 3
F = np.float32


def u32(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def c2(mcpt_mod, scene_c2):
    s, a = scene_c2
    return dict(scene=s, a=a, cam=mcpt_mod.config_camera(mcpt_mod.CONFIGS[2], W, H))


# ---------------------------------------------------------------------------------------------
# 1. the reference loop
@pytest.mark.parametrize("fixed", [False, True])
def test_the_loop_without_textures_is_the_oracle(oracle, c2, fixed):
    """texture_ref.render with no textures equals oracle.render bit for bit, as the plain loop and over
    the exploded scene (one triangle and one material per path): the exploding itself changes nothing."""
    rLd, rsm, rc = oracle.render(c2["a"], c2["cam"], W, H, SPP, fixed=fixed)
    for explode in (False, True):
        Ld, sm, cnt = TR.render(oracle, c2["a"], c2["cam"], W, H, SPP, fixed=fixed, explode=explode)
        assert np.array_equal(u32(Ld), u32(rLd)) and np.array_equal(sm, rsm), explode
        assert all(cnt[k] == rc[k] for k in ("extend_rays", "shadow_rays", "vis_rays")), explode


def test_a_texture_set_changes_the_reference_film(oracle, c2):
    tex = TR.random_set(c2["a"], sizes=((8, 8),))
    plain, _, pc = TR.render(oracle, c2["a"], c2["cam"], W, H, SPP)
    Ld, sm, cnt = TR.render(oracle, c2["a"], c2["cam"], W, H, SPP, tex=tex)
    changed = (Ld != plain).any(axis=2)
    print("pixels changed by the textures:", int(changed.sum()), "of", (W - 1) * (H - 1))
    assert np.isfinite(Ld).all() and changed.sum() > 100
    # The draws are keyed by (seed, pixel, sample, vertex), so they do not depend on the textures, and
    # neither do the paths up to the roulette.  The roulette tests the throughput, which the base colour
    # scales: beyond rr_depth a darker surface ends paths earlier, in the reference loop as on the device.
    assert cnt != pc
    short = [TR.render(oracle, c2["a"], c2["cam"], W, H, SPP, max_depth=2, tex=t)[2] for t in (None, tex)]
    assert short[0] == short[1]  # no vertex reaches the roulette: the counts are the untextured ones


def test_numpy_uv_reproduces_the_oracles_hit_records(oracle, c2):
    """uv_of restates tri_intersect: on every hit of a bundle of rays it gives or_trace_closest's t and,
    through the interpolation, its twice-normalised normal, bit for bit.  So u, v can be formed in numpy."""
    a = c2["a"]
    rng = np.random.default_rng(7)
    mn, mx = np.asarray(a["bmin"][0], np.float64), np.asarray(a["bmax"][0], np.float64)
    o = ((mn + mx) / 2 + (mx - mn) / 2 * 0.8 * rng.uniform(-1, 1, (4096, 3))).astype(F)
    d = rng.normal(size=(4096, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)
    pt, nm, tri = oracle.trace_closest(a, o, d)
    hit = tri >= 0
    assert hit.sum() > 2000
    ix = np.argsort(a["tri_id"])[tri[hit]]
    u, v, t = TR.uv_of(a, ix, o[hit], d[hit])
    assert np.array_equal(u32(t), u32(pt[hit, 3]))
    assert np.array_equal(u32(TR.hit_normal(a, ix, u, v)), u32(nm[hit, :3]))


def test_texel_quotients_and_lookup_identities():
    """byte / 255: the fp64 product rounded to float32 (device/texture.hpp's unorm8) is numpy's float32
    division for all 256 bytes.  The lookup of a constant image is that constant's texel wherever it is
    0 or 1 (weights that are multiples of 2^-16 and sum to 1), and a texel centre returns its texel."""
    c = np.arange(256)
    assert np.array_equal(u32((c * (1.0 / 255.0)).astype(F)), u32(c.astype(F) / F(255)))
    rng = np.random.default_rng(3)
    uv = (rng.random((512, 2)) * 7 - 3).astype(F)
    img = np.zeros((5, 3, 4), np.uint8)
    img[..., 1] = 255
    assert np.array_equal(TR.lookup(img, uv), np.broadcast_to(F([0, 1, 0]), (512, 3)))
    img = rng.integers(0, 256, (4, 8, 4)).astype(np.uint8)  # power-of-two sizes: the centres are exact
    jj, ii = np.meshgrid(np.arange(4), np.arange(8), indexing="ij")
    centres = np.stack([(ii + 0.5) / 8, (jj + 0.5) / 4], -1).reshape(-1, 2).astype(F)
    assert np.array_equal(u32(TR.lookup(img, centres)), u32(TR.texels(img).reshape(-1, 3)))
    assert np.array_equal(u32(TR.lookup(img, centres + F([3, -2]))), u32(TR.texels(img).reshape(-1, 3)))  # wrap
    bad = F([[np.nan, 0.3], [0.3, np.inf], [65536.0, 0.3], [-70000.0, 0.3]])
    zero = F([[0.0, 0.3], [0.3, 0.0], [0.0, 0.3], [0.0, 0.3]])
    assert np.array_equal(u32(TR.lookup(img, bad)), u32(TR.lookup(img, zero)))


# ---------------------------------------------------------------------------------------------
# 2. the host scene builder
def _glb_texcoords(path):
    """Per triangle corner uvs of a glb's first primitive, read with the standard library."""
    d = open(path, "rb").read()
    jlen = struct.unpack_from("<I", d, 12)[0]
    js = json.loads(d[20:20 + jlen])
    bin0 = 20 + jlen + 8

    def acc(i, dt, ncomp):
        a = js["accessors"][i]
        v = js["bufferViews"][a["bufferView"]]
        off = bin0 + v.get("byteOffset", 0) + a.get("byteOffset", 0)
        assert not v.get("byteStride")
        return np.frombuffer(d, dt, a["count"] * ncomp, off).reshape(a["count"], ncomp)

    pr = js["meshes"][0]["primitives"][0]
    uv = acc(pr["attributes"]["TEXCOORD_0"], np.float32, 2)
    ia = js["accessors"][pr["indices"]]
    idx = acc(pr["indices"], {5123: np.uint16, 5125: np.uint32, 5121: np.uint8}[ia["componentType"]], 1).reshape(-1, 3)
    return uv[idx.astype(np.int64)]  # (ntri, 3, 2)


def test_glb_texcoords_survive_the_build_in_desc_order(mcpt_mod, scene_cube):
    s, a = scene_cube
    want = _glb_texcoords(os.path.join(ASSETS, "Cube.glb"))
    assert len(want) == len(a["mat"]) == 12 and np.ptp(want) > 0.5
    for k in range(3):  # slot i of the desc holds scene triangle tri_id[i]
        assert np.array_equal(a[f"uv{k}"], want[a["tri_id"], k]), k
    uv = s.uv()
    assert all(np.array_equal(uv[k], a[f"uv{k}"]) for k in range(3))
    # a transform bakes positions and normals, not uvs
    t = mcpt_mod.Scene()
    t.load_glb(os.path.join(ASSETS, "Cube.glb"))
    xf = np.eye(4, dtype=F)
    xf[0, 0], xf[3, 1] = 2.0, 0.5
    t.transform(xf)
    t.build(8)
    b = t.arrays()
    for k in range(3):
        assert np.array_equal(b[f"uv{k}"], want[b["tri_id"], k]), k
    assert not np.array_equal(b["v0"][np.argsort(b["tri_id"])], a["v0"][np.argsort(a["tri_id"])])
    assert s.textures() is None  # a glb's embedded images are not decoded


def _quad_scene(mcpt, n_meshes=2):
    q = np.array([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0]], F)
    nn = np.tile(F([0, 0, 1]), (2, 1))
    s = mcpt.Scene()
    for m in range(n_meshes):
        z = F([0, 0, m])
        s.add_mesh(q[[0, 0]] + z, q[[1, 2]] + z, q[[2, 3]] + z, nn, nn, nn, (0.8, 0.8, 0.8))
    return s


def test_set_uv_and_set_texture_round_trip(mcpt_mod):
    s = _quad_scene(mcpt_mod)
    uv = [np.arange(4, dtype=F).reshape(2, 2) / 4 + k for k in range(3)]
    s.set_uv(1, *uv)
    s.build(1)
    a = s.arrays()
    assert np.array_equal(a["mat"][np.argsort(a["tri_id"])], [0, 0, 1, 1])
    inv = np.argsort(a["tri_id"])  # scene triangle -> desc slot; triangles 2, 3 are mesh 1's
    for k in range(3):
        assert not a[f"uv{k}"][inv[:2]].any()  # a mesh added without uvs has zeros
        assert np.array_equal(a[f"uv{k}"][inv[2:]], uv[k])
    s.set_uv(0, *[u + 10 for u in uv])  # on a built scene: the getters follow at once
    b = s.arrays()
    for k in range(3):
        assert np.array_equal(b[f"uv{k}"][inv[:2]], uv[k] + 10) and np.array_equal(b[f"uv{k}"][inv[2:]], uv[k])
    assert s.textures() is None
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (3, 5, 4)).astype(np.uint8)
    s.set_texture(1, img)
    t = s.textures()
    assert np.array_equal(t["mat_tex"], [-1, 0]) and len(t["textures"]) == 1 and np.array_equal(t["textures"][0], img)
    rgb = rng.integers(0, 256, (2, 2, 3)).astype(np.uint8)  # an rgb image gets alpha 255
    s.set_texture(0, rgb)
    t = s.textures()
    assert np.array_equal(t["mat_tex"], [1, 0]) and np.array_equal(t["textures"][1][..., :3], rgb)
    assert (t["textures"][1][..., 3] == 255).all()
    s.set_texture(1, img[:2, :2])  # a material's own texture is replaced in place
    t = s.textures()
    assert np.array_equal(t["mat_tex"], [1, 0]) and np.array_equal(t["textures"][0], img[:2, :2])
    s.set_texture(0, None)
    s.set_texture(1, None)
    assert s.textures() is None


def test_invalid_arguments_are_refused(mcpt_mod):
    lib = mcpt_mod.lib()
    s = _quad_scene(mcpt_mod)
    px = np.zeros((2, 2, 4), np.uint8)
    p8 = px.ctypes.data_as(C.POINTER(C.c_uint8))
    uv = np.zeros((2, 2), F)
    f = uv.ctypes.data_as(C.POINTER(C.c_float))
    for mat in (-1, 2):
        assert lib.mcpt_scene_set_material_texture(s.h, mat, 2, 2, p8) == -1
        assert lib.mcpt_scene_set_mesh_uv(s.h, mat, f, f, f) == -1
    for w, h in ((0, 2), (2, 0), (16385, 1), (1, 16385), (-1, 2)):
        assert lib.mcpt_scene_set_material_texture(s.h, 0, w, h, p8) == -1
    assert lib.mcpt_scene_set_mesh_uv(s.h, 0, f, None, f) == -1
    assert s.textures() is None
    with pytest.raises(mcpt_mod.McptError):
        s.uv()  # not built
    with pytest.raises(ValueError):
        s.set_texture(0, np.zeros((2, 2, 4), np.float32))
