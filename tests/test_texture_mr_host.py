"""Metallic-roughness textures on the CPU: the reference of tests/texture_mr_ref.py
against texture_ref and the oracle, and the host scene builder's MR setter and getter.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import texture_mr_ref as MR
import texture_ref as TR

W, H, SPP = 24, 16, 4
F = np.float32
RAYS = ("extend_rays", "shadow_rays", "vis_rays")


def u32(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def same(f, g):
    return np.array_equal(u32(f[0]), u32(g[0])) and np.array_equal(f[1], g[1]) and all(f[2][k] == g[2][k] for k in RAYS)


@pytest.fixture(scope="module")
def c2(mcpt_mod, scene_c2):
    s, a = scene_c2
    g, both, base, only = MR.fixture(a)
    return dict(a=g, both=both, base=base, only=only, cam=mcpt_mod.config_camera(mcpt_mod.CONFIGS[2], W, H))


_FILM = {}


def film(oracle, c2, which, fixed=False, depth=5):
    key = (which, fixed, depth)
    if key not in _FILM:
        _FILM[key] = MR.render(oracle, c2["a"], c2["cam"], W, H, SPP, max_depth=depth, fixed=fixed, tex=c2[which] if which else None)
    return _FILM[key]


# ---------------------------------------------------------------------------------------------
# 1. the reference
@pytest.mark.parametrize("fixed", [False, True])
def test_without_mr_indices_the_loop_is_texture_refs(oracle, c2, fixed):
    """mat_mr all -1 (and absent): texture_ref.render bit for bit, counts included; no set: the oracle."""
    want = TR.render(oracle, c2["a"], c2["cam"], W, H, SPP, fixed=fixed, tex=c2["base"])
    none = dict(c2["base"], mat_mr=np.full_like(c2["base"]["mat_tex"], -1))
    assert same(MR.render(oracle, c2["a"], c2["cam"], W, H, SPP, fixed=fixed, tex=none), want)
    assert same(film(oracle, c2, "base", fixed), want)
    assert same(film(oracle, c2, None, fixed), oracle.render(c2["a"], c2["cam"], W, H, SPP, fixed=fixed))


@pytest.mark.parametrize("depth", [5, 2])
@pytest.mark.parametrize("fixed", [False, True])
def test_the_mr_set_changes_more_than_100_pixels(oracle, c2, fixed, depth):
    """The guard the device tests rely on, for the reference alone: the MR set changes the film, alone
    and on top of the base-colour set, in more than 100 of the 384 pixels, and every film is finite."""
    f = {k: film(oracle, c2, k, fixed, depth) for k in (None, "base", "both", "only")}
    n_alone = int((f["only"][0] != f[None][0]).any(axis=2).sum())
    n_added = int((f["both"][0] != f["base"][0]).any(axis=2).sum())
    print(f"fixed={fixed} depth={depth}: pixels changed by the MR set alone {n_alone}, added to the base set {n_added}; "
          f"extension rays none {f[None][2]['extend_rays']} base {f['base'][2]['extend_rays']} both {f['both'][2]['extend_rays']}")
    assert all(np.isfinite(x[0]).all() for x in f.values())
    assert n_alone > 100 and n_added > 100


def test_extension_rays_depend_on_the_mr_set_below_the_roulette(oracle, c2):
    """max_depth 2 < rr_depth: no roulette, yet a lower roughness and a higher metallic end more
    continuation samples with f == 0 or pdf == 0 (F_FZERO), so fewer extension rays follow; the base-colour
    set alone changes no count there."""
    n, b, m = (film(oracle, c2, k, depth=2)[2]["extend_rays"] for k in (None, "base", "both"))
    assert n == b and m != n, (n, b, m)


def _masked(a, tex, masks):
    """Constant MR images whose G, B are 0 or 255 per material, and the arrays with those columns zeroed."""
    nmat = len(a["mat_params"])
    sizes = [(1, 1), (3, 5), (8, 8)]
    imgs = [np.broadcast_to(np.array([91, 255 * masks[m][0], 255 * masks[m][1], 77], np.uint8), sizes[m % 3] + (4,)).copy()
            for m in range(nmat)]
    t = dict(tex, textures=imgs, mat_tex=np.full(nmat, -1, np.int32), mat_mr=np.arange(nmat, dtype=np.int32))
    z = dict(a, mat_params=np.asarray(a["mat_params"], F).copy())
    z["mat_params"][:, 6:8] *= np.asarray(masks, F)
    return t, z


@pytest.mark.parametrize("fixed", [False, True])
def test_constant_images_are_channel_masks(oracle, c2, fixed):
    """Constant MR images with G, B in {0, 255}: the film of the same scene with those columns of mat_params
    zeroed, bit for bit (the weights are multiples of 2^-16 that sum to 1 and multiply 0 or 1; a zeroed
    roughness meets the same clamp either way).  All 255: the film without an MR set."""
    a = c2["a"]
    nmat = len(a["mat_params"])
    masks = [((1 + m % 3) & 1, (1 + m % 3) >> 1 & 1) for m in range(nmat)]  # (1,0), (0,1), (1,1) in turn
    t, z = _masked(a, c2["both"], masks)
    got = MR.render(oracle, a, c2["cam"], W, H, SPP, fixed=fixed, tex=t)
    want = oracle.render(z, c2["cam"], W, H, SPP, fixed=fixed)
    plain = film(oracle, c2, None, fixed)
    assert same(got, want) and not np.array_equal(u32(got[0]), u32(plain[0]))
    white, _ = _masked(a, c2["both"], [(1, 1)] * nmat)
    assert same(MR.render(oracle, a, c2["cam"], W, H, SPP, fixed=fixed, tex=white), plain)


# ---------------------------------------------------------------------------------------------
# 2. the host scene builder
def _quad_scene(mcpt, n_meshes=3):
    q = np.array([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0]], F)
    nn = np.tile(F([0, 0, 1]), (2, 1))
    s = mcpt.Scene()
    for m in range(n_meshes):
        z = F([0, 0, m])
        s.add_mesh(q[[0, 0]] + z, q[[1, 2]] + z, q[[2, 3]] + z, nn, nn, nn, (0.8, 0.8, 0.8))
    return s


def test_set_mr_texture_round_trip(mcpt_mod):
    s = _quad_scene(mcpt_mod)
    assert s.textures() is None
    rng = np.random.default_rng(6)
    a, b, c = (rng.integers(0, 256, hw + (4,)).astype(np.uint8) for hw in ((3, 5), (2, 2), (1, 4)))
    s.set_mr_texture(1, a)  # a scene with only an MR texture: the list holds it, no base-colour index is set
    t = s.textures()
    assert np.array_equal(t["mat_tex"], [-1, -1, -1]) and np.array_equal(t["mat_mr"], [-1, 0, -1])
    assert len(t["textures"]) == 1 and np.array_equal(t["textures"][0], a)
    s.set_texture(1, b)  # the same material's base colour: independent, a second image
    s.set_mr_texture(2, c[..., :3])  # an rgb image gets alpha 255
    t = s.textures()
    assert np.array_equal(t["mat_tex"], [-1, 1, -1]) and np.array_equal(t["mat_mr"], [-1, 0, 2])
    assert np.array_equal(t["textures"][1], b) and np.array_equal(t["textures"][2][..., :3], c[..., :3])
    assert (t["textures"][2][..., 3] == 255).all()
    s.set_mr_texture(1, a[:2, :3])  # a material's own MR texture is replaced in place
    t = s.textures()
    assert np.array_equal(t["mat_mr"], [-1, 0, 2]) and np.array_equal(t["textures"][0], a[:2, :3]) and len(t["textures"]) == 3
    s.set_mr_texture(1, None)  # detach: the base-colour texture of the material stays
    t = s.textures()
    assert np.array_equal(t["mat_tex"], [-1, 1, -1]) and np.array_equal(t["mat_mr"], [-1, -1, 2])
    s.set_texture(1, None)
    assert np.array_equal(s.textures()["mat_mr"], [-1, -1, 2])  # an MR texture alone keeps the list
    s.set_mr_texture(2, None)
    assert s.textures() is None


def test_a_scene_without_mr_returns_what_it_did(mcpt_mod):
    lib = mcpt_mod.lib()
    s = _quad_scene(mcpt_mod, 2)
    mr, n = C.POINTER(C.c_int32)(), C.c_int32(0)
    assert lib.mcpt_scene_get_material_mr(s.h, C.byref(mr), C.byref(n)) == 0 and n.value == 2 and [mr[0], mr[1]] == [-1, -1]
    img = np.random.default_rng(8).integers(0, 256, (3, 5, 4)).astype(np.uint8)
    s.set_texture(1, img)
    t = s.textures()
    assert np.array_equal(t["mat_tex"], [-1, 0]) and len(t["textures"]) == 1 and np.array_equal(t["textures"][0], img)
    assert np.array_equal(t["mat_mr"], [-1, -1])
    assert lib.mcpt_scene_get_material_mr(s.h, C.byref(mr), C.byref(n)) == 0 and [mr[0], mr[1]] == [-1, -1]


def test_invalid_arguments_are_refused(mcpt_mod):
    lib = mcpt_mod.lib()
    s = _quad_scene(mcpt_mod, 2)
    px = np.zeros((2, 2, 4), np.uint8)
    p8 = px.ctypes.data_as(C.POINTER(C.c_uint8))
    for mat in (-1, 2):
        assert lib.mcpt_scene_set_material_mr_texture(s.h, mat, 2, 2, p8) == -1
        assert lib.mcpt_scene_set_material_mr_texture(s.h, mat, 2, 2, None) == -1
    for w, h in ((0, 2), (2, 0), (16385, 1), (1, 16385), (-1, 2)):
        assert lib.mcpt_scene_set_material_mr_texture(s.h, 0, w, h, p8) == -1
    assert lib.mcpt_scene_set_material_mr_texture(None, 0, 2, 2, p8) == -1
    mr, n = C.POINTER(C.c_int32)(), C.c_int32(0)
    assert lib.mcpt_scene_get_material_mr(s.h, None, C.byref(n)) == -1 and lib.mcpt_scene_get_material_mr(s.h, C.byref(mr), None) == -1
    assert lib.mcpt_scene_get_material_mr(None, C.byref(mr), C.byref(n)) == -1
    assert s.textures() is None
    with pytest.raises(ValueError):
        s.set_mr_texture(0, np.zeros((2, 2, 4), np.float32))
