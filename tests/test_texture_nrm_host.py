"""Normal-map textures on the CPU: the reference of tests/texture_nrm_ref.py against
texture_mr_ref and the oracle, mcpt.tangents_from_uv against its numpy float64 restatement, and the host
scene builder's normal setter and getters.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import texture_mr_ref as MR
import texture_nrm_ref as NR

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
    g, sets = NR.fixture(a)
    return dict(a=g, cam=mcpt_mod.config_camera(mcpt_mod.CONFIGS[2], W, H), **sets)


_FILM = {}


def film(oracle, c2, which, fixed=False, depth=5):
    key = (which, fixed, depth)
    if key not in _FILM:
        _FILM[key] = NR.render(oracle, c2["a"], c2["cam"], W, H, SPP, max_depth=depth, fixed=fixed, tex=c2[which] if which else None)
    return _FILM[key]


def changed(f, g):
    return int((f[0] != g[0]).any(axis=2).sum())


# ---------------------------------------------------------------------------------------------
# 1. the reference
@pytest.mark.parametrize("fixed", [False, True])
def test_without_normal_indices_the_loop_is_texture_mr_refs(oracle, c2, fixed):
    """mat_nrm all -1 (tangents and scales given) or absent: texture_mr_ref.render bit for bit, counts included."""
    want = MR.render(oracle, c2["a"], c2["cam"], W, H, SPP, fixed=fixed, tex=c2["both"])
    none = dict(c2["all"], mat_nrm=np.full_like(c2["all"]["mat_nrm"], -1))
    assert same(NR.render(oracle, c2["a"], c2["cam"], W, H, SPP, fixed=fixed, tex=none), want)
    assert same(film(oracle, c2, "both", fixed), want)


@pytest.mark.parametrize("depth", [5, 2])
@pytest.mark.parametrize("fixed", [False, True])
def test_the_normal_set_changes_more_than_100_pixels(oracle, c2, fixed, depth):
    """The guard the device tests rely on, for the reference alone: the normal maps change the film, on top of
    the base + MR set and alone, in more than 100 of the 384 pixels, and every film is finite."""
    f = {k: film(oracle, c2, k, fixed, depth) for k in (None, "both", "all", "nrm")}
    n_added, n_alone = changed(f["all"], f["both"]), changed(f["nrm"], f[None])
    print(f"fixed={fixed} depth={depth}: pixels changed by the normal maps added to base + MR {n_added}, alone {n_alone}; "
          f"extension rays both {f['both'][2]['extend_rays']} all {f['all'][2]['extend_rays']}")
    assert all(np.isfinite(x[0]).all() for x in f.values())
    assert n_added > 100 and n_alone > 100


def test_extension_rays_depend_on_the_normal_set_below_the_roulette(oracle, c2):
    """max_depth 2 < rr_depth: no roulette, yet another normal ends other continuation samples."""
    b, m = (film(oracle, c2, k, depth=2)[2]["extend_rays"] for k in ("both", "all"))
    assert m != b, (b, m)


@pytest.mark.parametrize("depth", [5, 2])
@pytest.mark.parametrize("fixed", [False, True])
def test_scale_0_and_blue_255_is_the_identity(oracle, c2, fixed, depth):
    """A normal image whose B is 255 everywhere (R, G, A arbitrary) at scale 0: c.x = c.y = +-0 and c.z = 1,
    so m_i = N_i and the film is the one without normal maps bit for bit, counts included.  Byte 128 is not
    0.5 (128 / 255 = 0.50196...), so a "flat" (128, 128, 255) map at a non-zero scale is no identity."""
    assert changed(film(oracle, c2, "all", fixed, depth), film(oracle, c2, "both", fixed, depth)) > 100
    full = c2["all"]
    flat = full["textures"][-1].copy()
    flat[..., 2] = 255
    t = dict(full, textures=full["textures"][:-1] + [flat], nrm_scale=np.zeros_like(full["nrm_scale"]))
    assert same(NR.render(oracle, c2["a"], c2["cam"], W, H, SPP, max_depth=depth, fixed=fixed, tex=t), film(oracle, c2, "both", fixed, depth))
    if depth == 5 and not fixed:  # ... and the flat map at its own scales is none
        t = dict(full, textures=full["textures"][:-1] + [np.broadcast_to(np.array([128, 128, 255, 9], np.uint8), (2, 2, 4)).copy()])
        assert not same(NR.render(oracle, c2["a"], c2["cam"], W, H, SPP, fixed=fixed, tex=t), film(oracle, c2, "both", fixed, depth))


# ---------------------------------------------------------------------------------------------
# 2. tangents
def _bits(ts):
    return [u32(t) for t in ts]


def test_tangents_equal_the_restatement_on_the_fixture(mcpt_mod, c2):
    a, t = c2["a"], c2["all"]
    got = mcpt_mod.tangents_from_uv(a["v0"], a["v1"], a["v2"], a["n0"], a["n1"], a["n2"], t["uv0"], t["uv1"], t["uv2"])
    for g, w in zip(got, (t["tan0"], t["tan1"], t["tan2"])):
        assert np.array_equal(u32(g), u32(w))
        assert np.isfinite(g).all() and np.allclose(np.linalg.norm(g[:, :3].astype(np.float64), axis=1), 1, atol=1e-6)
        assert set(np.unique(g[:, 3])) <= {-1.0, 1.0}
    assert (got[0][:, 3] < 0).any() and (got[0][:, 3] > 0).any()  # random uvs: both handednesses occur


def test_tangents_hand_made_cases(mcpt_mod):
    """Zero determinant (collinear uvs), uv-degenerate (all three uvs equal), Tt parallel to N_i, a non-finite
    uv, a zero normal, and a regular triangle with its mirror image in uv: the C function equals the
    restatement bit for bit on all, the fallback is the stated one, and the mirrored triangle flips s."""
    p0, p1, p2 = F([0, 0, 0]), F([1, 0, 0]), F([0, 1, 0])
    z, x = F([0, 0, 1]), F([1, 0, 0])
    rows = [
        # v0 v1 v2, n0 n1 n2, uv0 uv1 uv2
        (p0, p1, p2, z, z, z, (0, 0), (1, 0), (0, 1)),              # regular: T = +x, s = +1
        (p0, p1, p2, z, z, z, (0, 0), (1, 0), (0, -1)),             # mirrored in v: s = -1
        (p0, p1, p2, z, z, z, (1, 0), (0, 0), (1, 1)),              # mirrored in u: T = -x, s = -1
        (p0, p1, p2, z, z, z, (0, 0), (1, 1), (2, 2)),              # zero determinant: fallback
        (p0, p1, p2, z, z, z, (0.25, 0.5), (0.25, 0.5), (0.25, 0.5)),  # uv-degenerate: fallback
        (p0, p1, p2, x, z, F([0.6, 0, 0.8]), (0, 0), (1, 0), (0, 1)),   # Tt = +x parallel to N_0: fallback at corner 0 only
        (p0, p1, p2, z, z, z, (0, 0), (np.inf, 0), (0, 1)),         # non-finite uv: fallback
        (p0, p1, p2, F([0, 0, 0]), F([0.5, 0.5, 0.7071]), F([0, -1, 0]), (0, 0), (0, 0), (0, 0)),  # fallbacks: zero normal, tie, -y
        (F([0.3, -1.2, 2.0]), F([1.7, 0.1, 2.5]), F([-0.4, 0.9, 3.1]), F([0.1, 0.2, 0.97]), F([0.0, 0.6, 0.8]), F([-0.3, 0.1, 0.95]),
         (0.13, 0.71), (0.92, 0.33), (0.41, -0.27)),               # generic
    ]
    arr = [np.array([r[k] for r in rows], F) for k in range(9)]
    got = mcpt_mod.tangents_from_uv(*arr)
    want = NR.tangents_from_uv(*arr)
    for g, w in zip(got, want):
        assert np.array_equal(u32(g), u32(w)), (g, w)
    t0 = got[0]
    assert np.array_equal(t0[0], [1, 0, 0, 1]) and np.array_equal(t0[1], [1, 0, 0, -1]) and np.array_equal(t0[2], [-1, 0, 0, -1])
    # the fallback for N = +z: the smallest component's axis is x (the first of the tie x, y): cross(z, x) = +y
    for k in (3, 4, 6):
        assert all(np.array_equal(t[k], [0, 1, 0, 1]) for t in got), k
    assert np.array_equal(got[0][5], [0, 0, 1, 1])  # N = +x: axis y (first of the tie y, z), cross(x, y) = +z
    assert np.array_equal(got[1][5], [1, 0, 0, 1])  # the other corners keep the regular tangent
    assert np.array_equal(got[0][7], [1, 0, 0, 1])  # a zero normal: (1, 0, 0)
    assert np.array_equal(got[2][7], [0, 0, 1, 1])  # N = -y: axis x, cross(-y, x) = +z
    assert np.isfinite(np.concatenate(got)).all()


def test_tangents_refuse_null_arrays(mcpt_mod):
    lib = mcpt_mod.lib()
    a = np.zeros(4, F)
    p = a.ctypes.data_as(C.POINTER(C.c_float))
    assert lib.mcpt_tangents_from_uv(1, *([p] * 11), None) == -1
    assert lib.mcpt_tangents_from_uv(1, None, *([p] * 11)) == -1
    assert lib.mcpt_tangents_from_uv(-1, *([p] * 12)) == -1
    assert lib.mcpt_tangents_from_uv(0, *([None] * 12)) == 0
    with pytest.raises(ValueError):
        mcpt_mod.tangents_from_uv(*[np.zeros((2, 3), F)] * 6, *[np.zeros((1, 2), F)] * 3)


# ---------------------------------------------------------------------------------------------
# 3. the host scene builder
def _quad_scene(mcpt, n_meshes=3):
    q = np.array([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0]], F)
    nn = np.tile(F([0, 0, 1]), (2, 1))
    s = mcpt.Scene()
    for m in range(n_meshes):
        z = F([0, 0, m])
        s.add_mesh(q[[0, 0]] + z, q[[1, 2]] + z, q[[2, 3]] + z, nn, nn, nn, (0.8, 0.8, 0.8))
    return s


def test_set_normal_texture_round_trip(mcpt_mod):
    s = _quad_scene(mcpt_mod)
    assert s.textures() is None
    rng = np.random.default_rng(6)
    a, b, c = (rng.integers(0, 256, hw + (4,)).astype(np.uint8) for hw in ((3, 5), (2, 2), (1, 4)))
    s.set_normal_texture(1, a, scale=0.75)  # a scene with only a normal map: the list holds it
    t = s.textures()
    assert np.array_equal(t["mat_tex"], [-1, -1, -1]) and np.array_equal(t["mat_mr"], [-1, -1, -1])
    assert np.array_equal(t["mat_nrm"], [-1, 0, -1]) and np.array_equal(t["nrm_scale"], F([1, 0.75, 1]))
    assert len(t["textures"]) == 1 and np.array_equal(t["textures"][0], a)
    s.set_texture(1, b)
    s.set_mr_texture(1, c)
    s.set_normal_texture(2, c[..., :3])  # an rgb image gets alpha 255; the default scale is 1
    t = s.textures()
    assert np.array_equal(t["mat_tex"], [-1, 1, -1]) and np.array_equal(t["mat_mr"], [-1, 2, -1]) and np.array_equal(t["mat_nrm"], [-1, 0, 3])
    assert np.array_equal(t["textures"][3][..., :3], c[..., :3]) and (t["textures"][3][..., 3] == 255).all()
    assert np.array_equal(t["nrm_scale"], F([1, 0.75, 1]))
    s.set_normal_texture(1, a[:2, :3], scale=-2.0)  # a material's own normal map is replaced in place, with its scale
    t = s.textures()
    assert np.array_equal(t["mat_nrm"], [-1, 0, 3]) and np.array_equal(t["textures"][0], a[:2, :3]) and len(t["textures"]) == 4
    assert np.array_equal(t["nrm_scale"], F([1, -2, 1]))
    s.set_normal_texture(1, None)  # detach: the material's other textures stay, the scale is 1 again
    t = s.textures()
    assert np.array_equal(t["mat_tex"], [-1, 1, -1]) and np.array_equal(t["mat_nrm"], [-1, -1, 3]) and np.array_equal(t["nrm_scale"], F([1, 1, 1]))
    s.set_normal_texture(2, None)
    t = s.textures()
    assert "mat_nrm" not in t and "nrm_scale" not in t and np.array_equal(t["mat_mr"], [-1, 2, -1])  # as before normal maps
    s.set_texture(1, None)
    s.set_mr_texture(1, None)
    assert s.textures() is None


def test_scene_tangents_are_the_function_over_the_built_scene(mcpt_mod):
    s = _quad_scene(mcpt_mod, 2)
    rng = np.random.default_rng(3)
    for m in range(2):
        s.set_uv(m, *(rng.random((2, 2)).astype(F) for _ in range(3)))
    with pytest.raises(mcpt_mod.McptError):
        s.tangents()  # not built
    s.build()
    a = s.arrays()
    want = NR.tangents_from_uv(a["v0"], a["v1"], a["v2"], a["n0"], a["n1"], a["n2"], *s.uv())
    got = s.tangents()
    assert all(np.array_equal(u32(g), u32(w)) for g, w in zip(got, want)) and got[0].shape == (4, 4)


def test_invalid_arguments_are_refused(mcpt_mod):
    lib = mcpt_mod.lib()
    s = _quad_scene(mcpt_mod, 2)
    px = np.zeros((2, 2, 4), np.uint8)
    p8 = px.ctypes.data_as(C.POINTER(C.c_uint8))
    L = lib.mcpt_scene_set_material_normal_texture
    for mat in (-1, 2):
        assert L(s.h, mat, 2, 2, p8, 1.0) == -1 and L(s.h, mat, 2, 2, None, 1.0) == -1
    for w, h in ((0, 2), (2, 0), (16385, 1), (1, 16385), (-1, 2)):
        assert L(s.h, 0, w, h, p8, 1.0) == -1
    for bad in (np.inf, -np.inf, np.nan):
        assert L(s.h, 0, 2, 2, p8, bad) == -1
    assert L(None, 0, 2, 2, p8, 1.0) == -1
    mn, sc, n = C.POINTER(C.c_int32)(), C.POINTER(C.c_float)(), C.c_int32(0)
    G = lib.mcpt_scene_get_material_normal
    assert G(s.h, None, C.byref(sc), C.byref(n)) == -1 and G(s.h, C.byref(mn), None, C.byref(n)) == -1
    assert G(s.h, C.byref(mn), C.byref(sc), None) == -1 and G(None, C.byref(mn), C.byref(sc), C.byref(n)) == -1
    assert G(s.h, C.byref(mn), C.byref(sc), C.byref(n)) == 0 and n.value == 2 and [mn[0], mn[1]] == [-1, -1] and [sc[0], sc[1]] == [1, 1]
    t = [C.POINTER(C.c_float)() for _ in range(3)]
    T = lib.mcpt_scene_get_tangents
    assert T(s.h, C.byref(t[0]), C.byref(t[1]), C.byref(t[2]), C.byref(n)) == -1  # not built
    assert T(None, C.byref(t[0]), C.byref(t[1]), C.byref(t[2]), C.byref(n)) == -1
    assert T(s.h, None, C.byref(t[1]), C.byref(t[2]), C.byref(n)) == -1
    assert s.textures() is None
    with pytest.raises(ValueError):
        s.set_normal_texture(0, np.zeros((2, 2, 4), np.float32))
