"""The film, path-stream and ray-queue state of a context under chains of transitions.

Every case applies a chain of film-state transitions (resize, path slots, layout, tile set, one-tile
steps, pack / unpack, emitter sampling) to one context, renders, and compares the film (Ld bit for bit,
samples) and ray_counts() with a fresh context created directly in the chain's final configuration.
Rejected calls raise McptError with a fixed message and leave the film as it was.

Config 1's scene, films of at most 96 x 80 with 16 x 16 or 32 x 32 tiles (ragged grids), 2 spp, depth 3."""
import ctypes as C

import numpy as np
import pytest

from mcpt import parallel

pytestmark = pytest.mark.gpu
SPP, DEPTH = 2, 3
E_INVALID = -1  # MCPT_E_INVALID (include/mcpt.h)


def u32(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def cam_c1(mcpt, W, H):
    return mcpt.config_camera(mcpt.CONFIGS[1], W, H)


def fresh(mcpt, scene, cam, W, H, T, slots=1, compact=False, tiles=None, E=None, sample=False):
    """A context created directly in a configuration (slots and layout are recorded before the film exists)."""
    pt = mcpt.PathTracer(0, mcpt.default_config(spp=SPP, max_depth=DEPTH, tile=T))
    pt.set_path_slots(slots)
    pt.set_compact_paths(compact)
    pt.upload_scene(scene)
    if E is not None:
        pt.set_emission(E)
    if sample:
        pt.set_emitter_sampling(True)
    pt.set_camera(cam)
    pt.resize(W, H, T, T)
    if tiles is not None:
        pt.set_tiles(tiles)
    return pt


def state(pt):
    Ld, s = pt.film()
    return Ld.copy(), s.copy(), pt.ray_counts()


def frame(pt):
    pt.render()
    return state(pt)


def same(a, b):
    return np.array_equal(u32(a[0]), u32(b[0])) and np.array_equal(a[1], b[1]) and a[2] == b[2]


def fresh_frame(mcpt, *args, **kw):
    pt = fresh(mcpt, *args, **kw)
    f = frame(pt)
    pt.close()
    return f


def raises(mcpt, msg, fn, *args):
    with pytest.raises(mcpt.McptError) as e:
        fn(*args)
    assert str(e.value) == f"mcpt error {E_INVALID}: {msg}"


def pack_to_device(mcpt, pt, ntiles, T):
    """pt's tile-set pixels packed into a device buffer of the HIP runtime libmcpt.so runs on (the copy
    already mapped into the process) -> (hip, buffer)."""
    with open("/proc/self/maps") as f:
        paths = sorted({line.split()[-1] for line in f if "libamdhip64" in line})
    assert len(paths) == 1, paths
    hip = C.CDLL(paths[0])
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    lib, n, buf = mcpt.lib(), C.c_uint32(), C.c_void_p()
    assert lib.mcpt_film_pack_tiles(pt.h, None, C.byref(n)) == 0 and n.value == ntiles * T * T
    assert hip.hipMalloc(C.byref(buf), C.c_size_t(n.value * 16)) == 0
    assert lib.mcpt_film_pack_tiles(pt.h, buf, C.byref(n)) == 0
    return hip, buf


def subset(W, H, T, seed=3):
    """A strict subset of the tile grid (rank 1 of 3) in scrambled order."""
    mine = parallel.tiles_for_rank(1, 3, W, H, T)
    return [mine[i] for i in np.random.default_rng(seed).permutation(len(mine))]


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("compact", [False, True])
def test_resize_chain(mcpt_mod, scene_c1, compact):
    """Small -> render -> larger with another tile size -> back: the queues shrink and regrow."""
    sc = scene_c1[0]
    pt = fresh(mcpt_mod, sc, cam_c1(mcpt_mod, 40, 24), 40, 24, 16, compact=compact)
    small = frame(pt)
    assert small[1].sum() > 0
    assert same(small, fresh_frame(mcpt_mod, sc, cam_c1(mcpt_mod, 40, 24), 40, 24, 16, compact=compact))
    pt.set_camera(cam_c1(mcpt_mod, 96, 80))
    pt.resize(96, 80, 32, 32)
    assert same(frame(pt), fresh_frame(mcpt_mod, sc, cam_c1(mcpt_mod, 96, 80), 96, 80, 32, compact=compact))
    pt.set_camera(cam_c1(mcpt_mod, 40, 24))
    pt.resize(40, 24, 16, 16)
    assert same(frame(pt), small)
    pt.close()


def test_slots_chain_full_layout(mcpt_mod, scene_c1):
    """set_path_slots 1 -> 3 -> 1 in the full layout, a render at each."""
    sc, W, H, T = scene_c1[0], 72, 40, 16
    cam = cam_c1(mcpt_mod, W, H)
    pt = fresh(mcpt_mod, sc, cam, W, H, T)
    one = frame(pt)
    pt.set_path_slots(3)
    assert not pt.film()[1].any()  # cleared
    assert same(frame(pt), fresh_frame(mcpt_mod, sc, cam, W, H, T, slots=3))
    pt.set_path_slots(1)
    assert same(frame(pt), one)
    assert same(one, fresh_frame(mcpt_mod, sc, cam, W, H, T))
    pt.close()


def test_compact_on_and_off_chain(mcpt_mod, scene_c1):
    """compact on -> a scrambled strict subset -> 2 slots -> every tile -> compact off."""
    sc, W, H, T = scene_c1[0], 72, 40, 16
    cam = cam_c1(mcpt_mod, W, H)
    sub = subset(W, H, T)
    nx, ny = parallel.tile_grid(W, H, T)
    assert 0 < len(sub) < nx * ny
    pt = fresh(mcpt_mod, sc, cam, W, H, T)
    pt.render()
    pt.set_compact_paths(True)
    assert not pt.film()[1].any()
    pt.set_tiles(sub)
    assert same(frame(pt), fresh_frame(mcpt_mod, sc, cam, W, H, T, compact=True, tiles=sub))
    pt.set_path_slots(2)  # keeps the tile set
    assert same(frame(pt), fresh_frame(mcpt_mod, sc, cam, W, H, T, slots=2, compact=True, tiles=sub))
    pt.set_tiles(None)
    assert same(frame(pt), fresh_frame(mcpt_mod, sc, cam, W, H, T, slots=2, compact=True))
    pt.set_compact_paths(False)
    assert same(frame(pt), fresh_frame(mcpt_mod, sc, cam, W, H, T, slots=2))
    pt.close()


@pytest.mark.parametrize("compact", [False, True])
def test_empty_tile_set_chain(mcpt_mod, scene_c1, compact):
    """An empty tile set renders nothing; one tile set after it is stepped like a fresh context's."""
    sc, W, H, T = scene_c1[0], 40, 24, 16
    cam = cam_c1(mcpt_mod, W, H)
    pt = fresh(mcpt_mod, sc, cam, W, H, T, compact=compact)
    pt.set_tiles([])
    st = pt.render()
    assert st.extend_rays == 0
    Ld, s, rays = state(pt)
    assert not s.any() and not Ld.any() and not any(rays.values())
    pt.set_tiles([(2, 1)])  # the ragged corner tile
    ref = fresh(mcpt_mod, sc, cam, W, H, T, compact=compact, tiles=[(2, 1)])
    for _ in range(3):
        pt.step(2, 1)
        ref.step(2, 1)
    got = state(pt)
    assert got[1].sum() > 0 and same(got, state(ref))
    pt.close()
    ref.close()


def test_one_tile_step_with_a_full_tile_set(mcpt_mod, scene_c1):
    """step(tx, ty) beside a full tile set (the one-tile buffer), then a render over the set."""
    sc, W, H, T = scene_c1[0], 72, 40, 16
    cam = cam_c1(mcpt_mod, W, H)
    pt = fresh(mcpt_mod, sc, cam, W, H, T)
    pt.set_path_slots(2)
    pt.set_path_slots(1)
    ref = fresh(mcpt_mod, sc, cam, W, H, T)
    for _ in range(3):
        pt.step(4, 2)
        ref.step(4, 2)
    got = state(pt)
    own = np.zeros((H, W), bool)
    own[2 * T:, 4 * T:] = True  # the ragged corner tile
    assert got[1][own].any() and not got[1][~own].any()
    assert same(got, state(ref))
    assert same(frame(pt), frame(ref))
    pt.close()
    ref.close()


def test_one_tile_step_swaps_an_empty_tile_set(mcpt_mod, scene_c1):
    """With 17 slots a 32 x 32 tile's 68 blocks need more per-shard queue capacity than the empty
    tile set's queues have: the step swaps the tile set for the tile and restores it."""
    sc, W, H, T, S = scene_c1[0], 96, 80, 32, 17
    cam = cam_c1(mcpt_mod, W, H)
    pt = fresh(mcpt_mod, sc, cam_c1(mcpt_mod, 40, 24), 40, 24, 16, slots=S)
    pt.set_camera(cam)
    pt.resize(W, H, T, T)
    pt.set_tiles([])
    ref = fresh(mcpt_mod, sc, cam, W, H, T, slots=S)  # full tile set: the one-tile buffer
    for _ in range(3):
        pt.step(2, 2)
        ref.step(2, 2)
    got = state(pt)
    assert got[1].sum() > 0 and same(got, state(ref))
    st = pt.render()  # the empty set is back
    assert st.extend_rays == 0 and same(state(pt), got)
    pt.set_tiles(None)
    assert same(frame(pt), frame(ref))
    pt.close()
    ref.close()


@pytest.mark.parametrize("compact", [False, True])
def test_pack_unpack_clear(mcpt_mod, scene_c1, compact):
    """A rank's tiles packed and unpacked into a root that renders the others: the whole frame; a clear
    empties the unpacked pixels too."""
    sc, W, H, T = scene_c1[0], 72, 40, 16
    cam = cam_c1(mcpt_mod, W, H)
    full = fresh_frame(mcpt_mod, sc, cam, W, H, T, slots=2)
    mine = parallel.tiles_for_rank(1, 3, W, H, T)
    nx, ny = parallel.tile_grid(W, H, T)
    others = [(x, y) for y in range(ny) for x in range(nx) if (x, y) not in mine]
    src = fresh(mcpt_mod, sc, cam, W, H, T, slots=2, compact=compact, tiles=mine)
    root = fresh(mcpt_mod, sc, cam, W, H, T, slots=2, compact=compact, tiles=others)
    src.render()
    root.render()
    lib = mcpt_mod.lib()
    hip, buf = pack_to_device(mcpt_mod, src, len(mine), T)
    xy = np.ascontiguousarray(mine, np.uint32).reshape(-1, 2)
    assert lib.mcpt_film_unpack_tiles(root.h, buf, xy.ctypes.data_as(C.POINTER(C.c_uint32)), len(mine)) == 0
    assert lib.mcpt_sync(root.h) == 0 and hip.hipFree(buf) == 0
    Ld, s = root.film()
    assert np.array_equal(u32(Ld), u32(full[0])) and np.array_equal(s, full[1])
    root.clear()
    Ld, s = root.film()
    assert not s.any() and not Ld.any()
    src.close()
    root.close()


# ---------------------------------------------------------------------------------------------
def emitter_scene(mcpt):
    """Twelve triangles in five meshes (one material each): floor, back wall, side wall, a pyramid and
    a quad lamp facing down, under a dim sky.  The lamp's material is the emissive one."""
    def quad(a, b, c, d):
        return np.float32([[a, b, c], [a, c, d]])

    def mesh(s, tris, rgb):
        tris = np.float32(tris)
        n = np.cross(tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0])
        n = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)
        s.add_mesh(tris[:, 0], tris[:, 1], tris[:, 2], n, n, n, rgb)

    s = mcpt.Scene()
    mesh(s, quad((-2, 0, 2), (2, 0, 2), (2, 0, -2), (-2, 0, -2)), (0.7, 0.7, 0.7))
    mesh(s, quad((-2, 0, -2), (2, 0, -2), (2, 3, -2), (-2, 3, -2)), (0.6, 0.3, 0.3))
    mesh(s, quad((-2, 0, 2), (-2, 0, -2), (-2, 3, -2), (-2, 3, 2)), (0.3, 0.6, 0.3))
    apex, base = (0.3, 1.1, -0.4), [(-0.3, 0, 0.2), (0.9, 0, 0.2), (0.9, 0, -1.0), (-0.3, 0, -1.0)]
    mesh(s, [[base[k], base[(k + 1) % 4], apex] for k in range(4)], (0.4, 0.4, 0.8))
    mesh(s, quad((-0.6, 2.5, 0.4), (-0.6, 2.5, -0.8), (0.6, 2.5, -0.8), (0.6, 2.5, 0.4)), (0.8, 0.8, 0.8))
    s.set_env_color((0.05, 0.06, 0.08), 1.0)
    s.build(4)
    E = np.zeros((5, 3), np.float32)
    E[4] = (6.0, 5.0, 4.0)
    return s, E


def emitter_cam(mcpt, W, H):
    return mcpt.make_camera((0.2, 1.2, 4.0), aspect=np.float32(W) / np.float32(H))


@pytest.mark.parametrize("compact", [False, True])
def test_emitter_sampling_chain(mcpt_mod, compact):
    """The any-hit queues hold 3 rays per evaluation while emitter sampling is active: the switch
    combined with a change of tile set, path slots and film size, and back to 2."""
    mcpt = mcpt_mod
    sc, E = emitter_scene(mcpt)
    assert len(sc.arrays()["mat"]) == 12
    W, H, T = 64, 48, 16
    cam = emitter_cam(mcpt, W, H)
    pt = fresh(mcpt, sc, cam, W, H, T, compact=compact)
    plain = frame(pt)
    pt.set_emission(E)
    lit = frame(pt)
    assert not np.array_equal(u32(lit[0]), u32(plain[0]))
    pt.set_emitter_sampling(True)
    assert pt.emitter_stats()["active"]
    third = frame(pt)
    assert pt.emitter_stats()["emitter_rays"] > 0
    assert not np.array_equal(u32(third[0]), u32(lit[0]))
    assert same(third, fresh_frame(mcpt, sc, cam, W, H, T, compact=compact, E=E, sample=True))
    sub = subset(W, H, T)
    pt.set_tiles(sub)
    pt.set_path_slots(2)  # compact: keeps the subset; full: back to every tile
    assert same(frame(pt), fresh_frame(mcpt, sc, cam, W, H, T, slots=2, compact=compact, E=E, sample=True,
                                       tiles=sub if compact else None))
    W2, H2, T2 = 96, 80, 32
    cam2 = emitter_cam(mcpt, W2, H2)
    pt.set_camera(cam2)
    pt.resize(W2, H2, T2, T2)
    pt.set_emitter_sampling(False)
    assert not pt.emitter_stats()["active"]
    last = frame(pt)
    assert pt.emitter_stats()["emitter_rays"] == 0
    assert same(last, fresh_frame(mcpt, sc, cam2, W2, H2, T2, slots=2, compact=compact, E=E))
    pt.close()


# ---------------------------------------------------------------------------------------------
def test_rejections_keep_the_film_compact(mcpt_mod, scene_c1):
    """Compact layout: a duplicate tile, a tile out of range, a step outside the tile set and an unpack
    into an own tile are rejected with their messages; the film stays."""
    sc, W, H, T = scene_c1[0], 72, 40, 16
    sub = subset(W, H, T)
    other = next(t for t in [(0, 0), (1, 0)] if t not in sub)
    pt = fresh(mcpt_mod, sc, cam_c1(mcpt_mod, W, H), W, H, T, slots=2, compact=True, tiles=sub)
    before = frame(pt)
    assert before[1].sum() > 0
    raises(mcpt_mod, "compact paths: a tile is listed twice", pt.set_tiles, [sub[0], sub[1], sub[0]])
    assert same(state(pt), before)
    raises(mcpt_mod, "tile out of range", pt.set_tiles, [sub[0], (5, 0)])  # the grid is 5 x 3
    raises(mcpt_mod, "tile out of range", pt.set_tiles, [(0, 3)])
    raises(mcpt_mod, "tile out of range", pt.step, 5, 0)
    assert same(state(pt), before)
    raises(mcpt_mod, "compact paths: the tile is not in the tile set", pt.step, *other)
    assert same(state(pt), before)
    xy = np.ascontiguousarray([other, sub[0]], np.uint32)
    lib = mcpt_mod.lib()
    junk = C.c_void_p(16)  # never read: the tiles are checked first
    rc = lib.mcpt_film_unpack_tiles(pt.h, junk, xy.ctypes.data_as(C.POINTER(C.c_uint32)), 2)
    assert rc == E_INVALID and lib.mcpt_last_error(pt.h).decode() == "unpack into one of the context's own tiles"
    xy = np.ascontiguousarray([other, (0, 3)], np.uint32)
    rc = lib.mcpt_film_unpack_tiles(pt.h, junk, xy.ctypes.data_as(C.POINTER(C.c_uint32)), 2)
    assert rc == E_INVALID and lib.mcpt_last_error(pt.h).decode() == "tile out of range"
    assert same(state(pt), before)
    assert same(frame(pt), before)  # the film was complete: nothing more to render
    pt.close()


def test_rejections_keep_the_film_full_layout(mcpt_mod, scene_c1):
    """Full layout: a tile out of range, an unpack into an own tile and a tile set naming an unpacked
    tile are rejected with their messages; the film stays."""
    sc, W, H, T = scene_c1[0], 72, 40, 16
    cam = cam_c1(mcpt_mod, W, H)
    mine = parallel.tiles_for_rank(1, 3, W, H, T)
    nx, ny = parallel.tile_grid(W, H, T)
    others = [(x, y) for y in range(ny) for x in range(nx) if (x, y) not in mine]
    src = fresh(mcpt_mod, sc, cam, W, H, T, tiles=mine)
    root = fresh(mcpt_mod, sc, cam, W, H, T, tiles=others)
    src.render()
    root.render()
    lib = mcpt_mod.lib()
    hip, buf = pack_to_device(mcpt_mod, src, len(mine), T)
    uptr = C.POINTER(C.c_uint32)
    before = state(root)
    xy = np.ascontiguousarray([mine[0], others[0]], np.uint32)
    rc = lib.mcpt_film_unpack_tiles(root.h, buf, xy.ctypes.data_as(uptr), 2)
    assert rc == E_INVALID and lib.mcpt_last_error(root.h).decode() == "unpack into one of the context's own tiles"
    assert same(state(root), before)
    raises(mcpt_mod, "tile out of range", root.set_tiles, [(0, 0), (nx, 0)])
    assert same(state(root), before)
    xy = np.ascontiguousarray(mine, np.uint32).reshape(-1, 2)
    assert lib.mcpt_film_unpack_tiles(root.h, buf, xy.ctypes.data_as(uptr), len(mine)) == 0
    assert lib.mcpt_sync(root.h) == 0 and hip.hipFree(buf) == 0
    whole = state(root)
    ref = fresh_frame(mcpt_mod, sc, cam, W, H, T)
    assert np.array_equal(u32(whole[0]), u32(ref[0])) and np.array_equal(whole[1], ref[1])
    raises(mcpt_mod, "a tile of the set holds pixels unpacked from another context: clear the film first",
           root.set_tiles, [others[0], mine[0]])
    raises(mcpt_mod, "a tile of the set holds pixels unpacked from another context: clear the film first",
           root.set_tiles, None)
    assert same(state(root), whole)
    assert same(frame(root), whole)  # the tile set is still the root's own
    root.clear()
    root.set_tiles(None)  # accepted after the clear
    assert same(frame(root), ref)
    src.close()
    root.close()
