"""Emissive materials on the CPU: the reference loop of tests/emission_ref.py
against the oracle's own render, the properties of the emission term that need no device, the host
scene builder's table and the glb reader's emissiveFactor / KHR_materials_emissive_strength."""
import ctypes as C
import json
import os
import struct

import numpy as np
import pytest

import emission_ref as ER
from conftest import ASSETS

W, H = 24, 16
LIT = (W - 1) * (H - 1)  # 345 rendered pixels: the last row and column never are


@pytest.fixture(scope="module")
def cube_dir(mcpt_mod):
    s = mcpt_mod.Scene()
    s.load_glb(os.path.join(ASSETS, "Cube.glb"))
    s.set_env_hdr(os.path.join(ASSETS, "HDR_029_Sky_Cloudy_Env.hdr"), 1)
    s.add_dir_light((-0.3, -1.0, -0.2), (1.0, 0.9, 0.8), 2.0)
    s.build(8)
    return s.arrays()


@pytest.fixture(scope="module")
def c2_films(mcpt_mod, oracle, scene_c2):
    """Reference films of config 2's proxy under a black environment, computed once per key."""
    a = ER.black(scene_c2[1])
    cam = mcpt_mod.config_camera(mcpt_mod.CONFIGS[2], W, H)
    nmat = len(a["mat_params"])
    cache = {}

    def film(mats, scale=1.0, depth=5, fixed=False):
        key = (tuple(mats), scale, depth, fixed)
        if key not in cache:
            E = ER.table(nmat, {m: np.float32(scale) * np.array((3.0, 2.0, 1.0), np.float32) for m in mats})
            cache[key] = ER.render(oracle, a, cam, W, H, 4, max_depth=depth, fixed=fixed, emission=E if mats else None)
        return cache[key]

    return film


@pytest.mark.parametrize("fixed", [False, True])
@pytest.mark.parametrize("which", ["cube", "c1", "c2"])
def test_loop_without_emission_is_the_oracle_render(mcpt_mod, oracle, cube_dir, scene_c1, scene_c2, which, fixed):
    a, cid, spp = {"cube": (cube_dir, 1, 6), "c1": (scene_c1[1], 1, 4), "c2": (scene_c2[1], 2, 4)}[which]
    cam = mcpt_mod.config_camera(mcpt_mod.CONFIGS[cid], W, H)
    Ld, sm, cnt = ER.render(oracle, a, cam, W, H, spp, fixed=fixed)
    oLd, osm, ocnt = oracle.render(a, cam, W, H, spp, fixed=fixed)
    assert np.array_equal(sm, osm) and sm[:-1, :-1].min() == spp
    assert np.array_equal(Ld.view(np.uint32), oLd.view(np.uint32))
    for k in ("extend_rays", "shadow_rays", "vis_rays", "iterations"):
        assert cnt[k] == ocnt[k], k


@pytest.mark.parametrize("fixed", [False, True])
def test_film_is_linear_in_the_table(c2_films, fixed):
    """Under a black environment every film value is a sum of Le * beta terms: 4 E gives 4 x the film, exactly."""
    Ld1, sm1, c1 = c2_films(ER.MATS_LIT, 1.0, fixed=fixed)
    Ld4, sm4, c4 = c2_films(ER.MATS_LIT, 4.0, fixed=fixed)
    lit = int((Ld1.reshape(-1, 3) != 0).any(axis=1).sum())
    print("lit pixels", lit, "of", LIT)
    assert lit > LIT // 3
    assert np.array_equal((np.float32(4.0) * Ld1).view(np.uint32), Ld4.view(np.uint32))
    assert np.array_equal(sm1, sm4) and c1 == c4  # the paths do not depend on the table


@pytest.mark.parametrize("wall", [0, 3])
def test_indirect_emission_and_the_depth_cap(c2_films, wall):
    """An emissive wall lights pixels that never see it: at a changed pixel whose depth-1 film is zero,
    every primary hit lies on a non-emissive material.  max_depth = 2 cuts the paths at the second
    vertex, which still collects (len == max_depth), so fewer pixels change than at depth 5."""
    none = c2_films((), depth=5)[0].reshape(-1, 3)
    assert not none.any()  # black environment, no light: nothing but emission reaches the film
    d5 = c2_films((wall,), depth=5)[0].reshape(-1, 3)
    d2 = c2_films((wall,), depth=2)[0].reshape(-1, 3)
    d1 = c2_films((wall,), depth=1)[0].reshape(-1, 3)
    ch5, ch2, direct = (d5 != 0).any(axis=1), (d2 != 0).any(axis=1), (d1 != 0).any(axis=1)
    print("wall", wall, "changed at depth 5 / 2 / 1:", int(ch5.sum()), int(ch2.sum()), int(direct.sum()), "of", LIT)
    assert 0 < direct.sum() < LIT
    assert (ch5 & ~direct).any(), "no pixel lit by indirect emission alone"
    assert (ch2 & ~direct).any(), "the len == max_depth vertex collected nothing"
    assert ch2.sum() != ch5.sum() and not (ch2 & ~ch5).any()
    # a path's first two vertices are the same at either depth: depth 5 only adds terms
    assert (d5[ch2] >= d2[ch2]).all()


def write_quad_glb(path, materials):
    """One unit quad (two triangles, POSITION + NORMAL, u16 indices) per entry of `materials`."""
    pos = np.array([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0]], np.float32)
    nrm = np.tile(np.array([0, 0, 1], np.float32), (4, 1))
    idx = np.array([0, 1, 2, 0, 2, 3], np.uint16)
    blob = pos.tobytes() + nrm.tobytes() + idx.tobytes()
    blob += b"\0" * (-len(blob) % 4)
    doc = {
        "asset": {"version": "2.0"}, "scene": 0, "scenes": [{"nodes": list(range(len(materials)))}],
        "nodes": [{"mesh": i, "translation": [3.0 * i, 0, 0]} for i in range(len(materials))],
        "meshes": [{"primitives": [{"attributes": {"POSITION": 0, "NORMAL": 1}, "indices": 2, "material": i, "mode": 4}]}
                   for i in range(len(materials))],
        "materials": materials,
        "buffers": [{"byteLength": len(blob)}],
        "bufferViews": [{"buffer": 0, "byteOffset": 0, "byteLength": 48}, {"buffer": 0, "byteOffset": 48, "byteLength": 48},
                        {"buffer": 0, "byteOffset": 96, "byteLength": 12}],
        "accessors": [{"bufferView": 0, "componentType": 5126, "count": 4, "type": "VEC3", "min": [-1, -1, 0], "max": [1, 1, 0]},
                      {"bufferView": 1, "componentType": 5126, "count": 4, "type": "VEC3"},
                      {"bufferView": 2, "componentType": 5123, "count": 6, "type": "SCALAR"}],
    }
    js = json.dumps(doc).encode()
    js += b" " * (-len(js) % 4)
    with open(path, "wb") as f:
        f.write(struct.pack("<4sII", b"glTF", 2, 12 + 8 + len(js) + 8 + len(blob)))
        f.write(struct.pack("<II", len(js), 0x4E4F534A) + js)
        f.write(struct.pack("<II", len(blob), 0x004E4942) + blob)


def test_glb_emissive_factor_times_strength(mcpt_mod, tmp_path):
    ef, strength = (0.25, 0.5, 0.75), 6.5
    mats = [{"pbrMetallicRoughness": {"baseColorFactor": [0.8, 0.7, 0.6, 1]}, "emissiveFactor": list(ef),
             "extensions": {"KHR_materials_emissive_strength": {"emissiveStrength": strength}}},
            {"pbrMetallicRoughness": {"baseColorFactor": [0.5, 0.5, 0.5, 1]}},
            {"emissiveFactor": [1.0, 0.5, 0.0]}]  # no extension: strength 1
    p = tmp_path / "quads.glb"
    write_quad_glb(p, mats)
    s = mcpt_mod.Scene()
    s.load_glb(p)
    e = s.emission()
    assert e.shape == (3, 3) and e.dtype == np.float32
    assert np.array_equal(e[0], np.array(ef, np.float32) * np.float32(strength))
    assert np.array_equal(e[1], np.zeros(3, np.float32))
    assert np.array_equal(e[2], np.array([1.0, 0.5, 0.0], np.float32))
    s.build(8)
    a = s.arrays()
    assert len(a["mat_params"]) == 3 and sorted(set(a["mat"])) == [0, 1, 2]
    assert np.allclose(a["mat_params"][0, :3], (0.8, 0.7, 0.6))
    # a glb without either leaves every entry zero: emission() is None (the bundled assets)
    p2 = tmp_path / "plain.glb"
    write_quad_glb(p2, [{"pbrMetallicRoughness": {"baseColorFactor": [1, 1, 1, 1]}}])
    s2 = mcpt_mod.Scene()
    s2.load_glb(p2)
    assert s2.emission() is None
    for name in ("Cube.glb", "sphere.glb", "Suzanne.glb"):
        s3 = mcpt_mod.Scene()
        s3.load_glb(os.path.join(ASSETS, name))
        assert s3.emission() is None, name


def test_scene_emission_round_trip_and_rejections(mcpt_mod):
    s = mcpt_mod.Scene()
    s.make_proxy(2)
    assert s.emission() is None
    s.set_emission(2, (8.0, 8.0, 8.0)).set_emission(7, (0.5, 2.0, 8.0))
    e = s.emission()
    nmat = e.shape[0]
    assert np.array_equal(e, ER.table(nmat, {2: (8.0, 8.0, 8.0), 7: (0.5, 2.0, 8.0)}))
    s.build(**mcpt_mod.DEFAULT_BVH)
    assert np.array_equal(s.emission(), e) and len(s.arrays()["mat_params"]) == nmat  # one entry per desc material
    for mat, rgb in ((-1, (1, 1, 1)), (nmat, (1, 1, 1)), (2, (1, -1, 1)), (2, (1, np.nan, 1)), (2, (np.inf, 1, 1))):
        with pytest.raises(mcpt_mod.McptError):
            s.set_emission(mat, rgb)
    assert np.array_equal(s.emission(), e)  # a rejected call changes nothing
    s.set_emission(2, (0, 0, 0)).set_emission(7, (0, 0, 0))
    assert s.emission() is None
    rgb, n = C.POINTER(C.c_float)(), C.c_int32(-1)
    assert mcpt_mod.lib().mcpt_scene_get_emission(s.h, C.byref(rgb), C.byref(n)) == 0 and not rgb and n.value == nmat


def test_entry_points_resolve(mcpt_mod):
    lib = C.CDLL(mcpt_mod.LIB_PATH)
    for name in ("mcpt_set_material_emission", "mcpt_material_emission_read", "mcpt_scene_set_material_emission",
                 "mcpt_scene_get_emission"):
        assert hasattr(lib, name) and name in mcpt_mod.ABI, name
    for cls, names in ((mcpt_mod.Scene, ("set_emission", "emission")), (mcpt_mod.PathTracer, ("set_emission", "emission"))):
        for n in names:
            assert callable(getattr(cls, n)), (cls, n)
    # the desc and the ABI version are what they were: the table travels beside the desc
    assert "emission" not in [f[0] for f in mcpt_mod.SceneDesc._fields_]
