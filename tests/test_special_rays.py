"""Axis-aligned, nearly axis-aligned and non-finite rays (tests/special_rays.py) against the oracle.

Rays with a non-finite inverse direction component take k_trace's second box test, slab() (the
reference's sign-selected test, where a NaN product passes), and a chain of special cases around it:
cull_iota's -inf / -FLT_MAX / overflowing values, keep_box's NaN margin, the 4-wide sort's NaN keys,
the occluder cache's `fin` test, the complete keys' direction intervals that touch zero and k_shade's
ray_misses_scene.  No other generator of the suite makes a zero direction component.

CPU tests: the model of the product's traversal (oracle/trav_model.c, modes 0 and 2) against the
oracle on these rays, and the conditions on the generator (so that a weakened generator fails).
GPU tests: k_trace (closest and any hit) against the oracle, bit for bit, on every scene, tree and
kernel variant; films of the floor scene under axis-aligned directional lights against the oracle's
render, with every upload variant of the occluder cache, the complete keys and the primary table.

A NaN slab product lets a box pass for a ray that misses the box's ancestors, so on a few of these
rays the reference traversal's answer depends on the tree.  The GPU tests
therefore give the oracle the tree the device holds (special_rays.tree_arrays of the read-back tree)
and compare every ray with that, and they check that the oracle on the scene's own desc tree differs
from it only on rays with a NaN product.
"""
import os

import numpy as np
import pytest

import bvh_ref as R
import refit_ref as RF
import special_rays as SR
from test_cull import floor_scene, same_as_oracle, scaled_scene

F = np.float32
N_CPU = 200000
N_GPU = 120000
N_PLANES = 40000
SCENES = ["floor", "c2", "c2_x1e3", "c2_x1e-3", "cube"]
SMALL = ["one", "coincident300"]
_SCENES, _REF = {}, {}


def scene(mcpt_mod, request, name):
    """(Scene, arrays) by name, built once per session."""
    if name not in _SCENES:
        if name == "cube":
            _SCENES[name] = request.getfixturevalue("scene_cube")
        else:
            if name == "floor":
                s = floor_scene(mcpt_mod)
            elif name.startswith("c2"):
                s = scaled_scene(mcpt_mod, 2, float(name[4:]) if "_x" in name else 1.0)
            elif name == "one":
                s = R.scene_of(mcpt_mod, R.random_tris(1, size=0.5))
            elif name == "coincident300":
                s = R.scene_of(mcpt_mod, R.coincident_tris(300))
            else:
                raise KeyError(name)
            _SCENES[name] = (s, s.arrays())
    return _SCENES[name]


def reference(oracle, key, a, n, seed, planes=None):
    """Rays and the oracle's answers for them, computed once per key and shared: (ro, rd, cls,
    (pos_t, normal, triangle, visibility))."""
    if key not in _REF:
        ro, rd, cls = SR.special_rays(a, n, seed, planes)
        th = oracle.default_threads()
        op_, on, ot = oracle.trace_closest(a, ro, rd, nthreads=th)
        ov = oracle.trace_any(a, ro, rd, nthreads=th)
        for x in (ro, rd, cls, op_, on, ot, ov):
            x.setflags(write=False)
        _REF[key] = (ro, rd, cls, (op_, on, ot, ov))
    return _REF[key]


def with_env(env, fn):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# ---- CPU: the generator's conditions and the traversal model ---------------------------------
def check_generator(name, a, ro, rd, cls, ot, ov, hits=True):
    """The conditions a weakened generator would miss; returns the ON_PLANE NaN-product share."""
    nf = SR.nonfinite_inverse(rd)
    for c in (SR.ZERO1, SR.ZERO2, SR.ON_PLANE, SR.SUBNORMAL):
        assert (cls == c).sum() > 0 and nf[cls == c].all(), SR.CLASS_NAMES[c]
    assert (cls == SR.TINY).sum() > 0 and not nf[cls == SR.TINY].any()
    zeros = (rd == 0).sum(axis=1)
    assert (zeros[cls == SR.ZERO1] == 1).all() and (zeros[cls == SR.ZERO2] == 2).all()
    neg = np.signbit(rd) & (rd == 0)
    for c in (SR.ZERO1, SR.ZERO2, SR.ON_PLANE):  # both signs of zero, in comparable parts
        k = cls == c
        share = neg[k].sum() / (rd[k] == 0).sum()
        assert 0.4 < share < 0.6, (SR.CLASS_NAMES[c], share)
    sub = rd[cls == SR.SUBNORMAL]
    assert (sub != 0).all() and (np.abs(sub) < F(1.1754944e-38)).any(axis=1).all()
    on = cls == SR.ON_PLANE
    nan_share = float(SR.nan_product(ro[on], rd[on], a["bmin"], a["bmax"]).mean())
    assert nan_share >= 0.9, nan_share
    over = SR.iota_overflows(rd) & (cls == SR.TINY)
    assert over.sum() >= 1000, over.sum()
    sc = cls == SR.SCALED
    n2 = (rd[sc].astype(np.float64) ** 2).sum(axis=1)
    lim = 1.0 + 1.0 / 512.0
    assert ((n2 > lim) & (n2 < lim * (1 + 2.0 ** -7))).sum() > 100 and ((n2 <= lim) & (n2 > 0.99)).sum() > 100
    assert (n2 < 1e-4).any() and (n2 > 1e4).any()
    if len(a["v0"]) <= SR.NONFINITE_TRIS:
        k = cls == SR.NONFINITE
        assert 1000 <= k.sum() <= SR.NONFINITE_MAX
        assert np.isnan(ro[k]).any() and np.isinf(ro[k]).any() and np.isnan(rd[k]).any() and np.isinf(rd[k]).any()
        allzero = (rd[k] == 0).all(axis=1)
        assert allzero.any() and (np.signbit(rd[k][allzero]).any(axis=1) & ~np.signbit(rd[k][allzero]).all(axis=1)).any()
    if hits:
        for nm, cnt, hit, occ in SR.class_shares(cls, ot, ov):
            if nm != "nonfinite":
                assert hit >= 0.5, (name, nm, hit)
                assert 0.0 < occ < 1.0, (name, nm, occ)
    return nan_share


@pytest.mark.parametrize("name", SCENES)
def test_model_equals_oracle_on_special_rays(mcpt_mod, oracle, request, name):
    """The model of the product's traversal without culling (mode 0) and under the product's rule (mode
    2) against the oracle on 200,000 special rays: closest triangle, t bits and visibility bit for bit;
    and the generator's conditions on the same rays."""
    _, a = scene(mcpt_mod, request, name)
    ro, rd, cls, (op_, on, ot, ov) = reference(oracle, (name, N_CPU, 1), a, N_CPU, 1)
    nan_share = check_generator(name, a, ro, rd, cls, ot, ov, hits=name != "cube")
    m = oracle.model_margins(a)
    assert m["contained"]
    for mode in (0, 2):
        tri, t, vis, _ = oracle.model_trace(a, ro, rd, mode, m, nthreads=oracle.default_threads())
        assert np.array_equal(tri, ot), f"mode {mode}: {(tri != ot).sum()} closest hits differ"
        assert np.array_equal(t.view(np.uint32), op_[:, 3].view(np.uint32)), f"mode {mode}: t differs"
        assert np.array_equal(vis, ov), f"mode {mode}: {(vis != ov).sum()} visibilities differ"
    print(f"{name}: {len(ro)} rays, hit/occluded {SR.format_shares(cls, ot, ov)}, NaN-product share {nan_share:.3f}, "
          f"{int((SR.iota_overflows(rd) & (cls == SR.TINY)).sum())} tiny rays with an overflowing scale, 0 differ")


def test_planes_argument_and_small_scenes(mcpt_mod, oracle, request):
    """special_rays takes its on-plane coordinates from `planes` when given, and works on a single
    triangle (the root a leaf) and on coincident triangles (flat, equal boxes)."""
    _, a = scene(mcpt_mod, request, "floor")
    pl = F([[0.125, 0.375, -0.625], [1.5, 2.5, 3.5]])
    ro, rd, cls = SR.special_rays(a, 20000, 3, planes=pl)
    k = cls == SR.ON_PLANE
    zero = rd[k] == 0
    assert np.isin(ro[k][zero], pl).all()
    assert SR.nan_product(ro[k], rd[k], pl, pl).all()
    for name in SMALL:
        _, b = scene(mcpt_mod, request, name)
        ro, rd, cls = SR.special_rays(b, 20000, 5)
        assert len(ro) == 20000 and set(np.unique(cls)) == set(range(7))
        k = cls == SR.ON_PLANE
        assert np.isin(ro[k][rd[k] == 0], np.concatenate([b["v0"], b["v1"], b["v2"]])).all()
        assert SR.nan_product(ro[k], rd[k], b["bmin"], b["bmax"]).mean() > 0.5  # (a middle vertex is no box plane)


@pytest.mark.parametrize("width", [2, 4])
@pytest.mark.parametrize("builder", ["ploc", "lbvh"])
def test_answers_belong_to_the_tree_on_nan_product_rays(mcpt_mod, oracle, request, builder, width):
    """The floor scene under the reference builders' PLOC and LBVH trees (tests/bvh_ref.py), as pair
    trees and collapsed to 4-wide nodes, through SR.tree_arrays: the oracle's answers differ from the
    ones under the scene's SAH desc tree only on rays with a NaN slab product, and the traversal
    model (modes 0 and 2) equals the oracle under every tree.  Ray 29576 of the batch the GPU tests
    use is such a ray: direction (0, -inf, -0), origin on a vertex's x coordinate, accepted at t = -0
    on triangles 181 and 237; the SAH tree reaches both (181, the lower id, wins), the PLOC tree only
    237 -- which is what k_trace returns on its PLOC tree."""
    _, a = scene(mcpt_mod, request, "floor")
    ro, rd, cls, ref_a = reference(oracle, ("floor", N_GPU, 2), a, N_GPU, 2)
    t = R.BUILDERS[builder](a["v0"], a["v1"], a["v2"])
    b = SR.tree_arrays(a, t["nodes"], R.tri_records(a, 3)[t["order"]], R.ref_info(t, len(a["v0"]), width=width))
    assert np.isinf(b["bmin"]).any() == (width == 4)
    ref_b = oracle_trace(oracle, b, ro, rd)
    dep = check_tree_dependent(a, b, ro, rd, ref_a, ref_b)
    if builder == "ploc":
        assert np.array_equal(rd[29576], F([0.0, -np.inf, -0.0])) and ref_a[2][29576] == 181 and ref_b[2][29576] == 237
    m = oracle.model_margins(b)
    assert m["contained"]
    for mode in (0, 2):
        tri, tt, vis, _ = oracle.model_trace(b, ro, rd, mode, m, nthreads=oracle.default_threads())
        assert np.array_equal(tri, ref_b[2]) and np.array_equal(vis, ref_b[3]), mode
        assert np.array_equal(tt.view(np.uint32), ref_b[0][:, 3].view(np.uint32)), mode
    print(f"floor, {builder} tree, width {width}: {dep} of {len(ro)} answers belong to the tree")


# ---- GPU: k_trace ----------------------------------------------------------------------------
def trace(pt, ro, rd):
    gp, gn, gt = pt.trace_closest(ro, rd)
    return gp, gn, gt, pt.trace_any(ro, rd)


def oracle_trace(oracle, a, ro, rd):
    th = oracle.default_threads()
    return oracle.trace_closest(a, ro, rd, nthreads=th) + (oracle.trace_any(a, ro, rd, nthreads=th),)


def differing(x, y):
    """Rays on which two (pos_t, normal, triangle, visibility) results differ in any bit."""
    out = np.zeros(len(x[2]), bool)
    for u, v in zip(x, y):
        dt = np.uint32 if u.dtype.itemsize == 4 else np.uint8
        out |= (np.ascontiguousarray(u).view(dt) != np.ascontiguousarray(v).view(dt)).reshape(len(out), -1).any(axis=1)
    return out


def check_tree_dependent(a, b, ro, rd, ref_a, ref_b):
    """Rays on which the oracle's answers under two trees (arrays a and b) of one scene differ have a
    NaN slab product against a box of one of them: a box that passes although the ray misses its
    ancestors, so what the reference's traversal reaches belongs to the tree.  Returns their number."""
    dep = differing(ref_a, ref_b)
    boxes = (np.concatenate([a["bmin"].reshape(-1, 3), b["bmin"].reshape(-1, 3)]),
             np.concatenate([a["bmax"].reshape(-1, 3), b["bmax"].reshape(-1, 3)]))
    assert SR.nan_product(ro[dep], rd[dep], *boxes).all(), f"{int(dep.sum())} rays depend on the tree without a NaN product"
    return int(dep.sum())


def check_on_device_tree(pt, oracle, a, ro, rd, cls, ref_a, what):
    """k_trace against the oracle on the tree the device holds (SR.tree_arrays of the read-back tree):
    every ray, bit for bit -- triangle index, position and t, normal, visibility.  The oracle on the
    scene's own desc tree differs from that only on rays check_tree_dependent() accepts; on every other
    ray the product so equals it too.  Prints the shares; returns the arrays of the device's tree."""
    got = trace(pt, ro, rd)
    b = SR.tree_arrays(a, *pt.bvh_read())
    ref_b = oracle_trace(oracle, b, ro, rd)
    same_as_oracle(got, ref_b)
    dep = check_tree_dependent(a, b, ro, rd, ref_a, ref_b)
    on = cls == SR.ON_PLANE
    share = float(SR.nan_product(ro[on], rd[on], b["bmin"], b["bmax"]).mean())
    print(f"{what}: {len(ro)} rays, hit/occluded {SR.format_shares(cls, ref_b[2], ref_b[3])}, NaN-product share "
          f"{share:.3f}, 0 differ from the oracle on the device's tree, {dep} answers belong to the tree")
    return b, share


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES + SMALL)
def test_gpu_special_rays_default_upload(mcpt_mod, oracle, request, name):
    """mcpt_stage_run EXTEND and SHADOW under the default upload against the oracle: triangle index,
    position and t bits, normal bits, visibility.  c2_x1e3 has no bounded triangle (every margin
    infinite), c2_x1e-3 only bounded ones; `one` is a root leaf."""
    s, a = scene(mcpt_mod, request, name)
    ro, rd, cls, ref = reference(oracle, (name, N_GPU, 2), a, N_GPU, 2)
    pt = mcpt_mod.PathTracer(0)
    pt.upload_scene(s)
    try:
        check_on_device_tree(pt, oracle, a, ro, rd, cls, ref, name)
    finally:
        pt.close()


def without_containment(a):
    """The arrays with an interior node's box shrunk by a fifth per side (as
    test_bvh_without_containment_disables_cull_and_cache does): the upload turns the culls and the
    occluder cache off (cull_ok = 0), and the oracle traverses the same boxes."""
    b = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in a.items()}
    n = int(np.nonzero(b["nprims"] == 0)[0][1])
    lo, hi = b["bmin"].reshape(-1, 3)[n].copy(), b["bmax"].reshape(-1, 3)[n].copy()
    b["bmin"].reshape(-1, 3)[n] = lo + F(0.2) * (hi - lo)
    b["bmax"].reshape(-1, 3)[n] = hi - F(0.2) * (hi - lo)
    return b


VARIANTS = {
    "layout0": ({"MCPT_SIBLING_LAYOUT": "0"}, False), "layout1": ({"MCPT_SIBLING_LAYOUT": "1"}, False),
    "layout2": ({"MCPT_SIBLING_LAYOUT": "2"}, False), "layout3": ({"MCPT_SIBLING_LAYOUT": "3"}, False),
    "width4": ({"MCPT_BVH_WIDTH": "4"}, False), "width4_ploc": ({"MCPT_BVH_WIDTH": "4"}, "ploc"),
    "ploc": ({}, "ploc"), "lbvh": ({}, "lbvh"), "tiny_stack": ({}, False), "no_containment": ({}, False),
}
READ_BACK = ("width4", "width4_ploc", "ploc", "lbvh")


@pytest.mark.gpu
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", ["floor", "c2"])
def test_gpu_special_rays_tree_and_kernel_variants(mcpt_mod, oracle, request, name, variant):
    """The same comparison under every node numbering, 4-wide nodes (host- and device-built), both
    device builders, the 2-entry LDS stack (spill entries) and a caller tree without containment.
    For the device-built and 4-wide trees a second batch takes its on-plane origins from the planes
    of the tree as read back, and at least 0.9 of its on-plane rays have a NaN product there."""
    s, a = scene(mcpt_mod, request, name)
    env, gpu_bvh = VARIANTS[variant]
    key, up = (name, N_GPU, 2), s
    if variant == "no_containment":
        a = without_containment(a)
        key, up = (name, N_GPU, 2, variant), mcpt_mod.desc_from_arrays(a)
    ro, rd, cls, ref = reference(oracle, key, a, N_GPU, 2)
    pt = mcpt_mod.PathTracer(0)
    try:
        with_env(env, lambda: pt.upload_scene(up, gpu_bvh=gpu_bvh))
        if variant == "tiny_stack":
            pt.set_tiny_lds_stack(True)
        info = pt.bvh_read()[2]
        assert info["width"] == (4 if "width4" in variant else 2) and bool(info["gpu_built"]) == bool(gpu_bvh)
        if variant.startswith("layout"):
            assert info["layout"] == int(variant[-1])
        check_on_device_tree(pt, oracle, a, ro, rd, cls, ref, f"{name} {variant}")
        if variant in READ_BACK:
            ro2, rd2, cls2 = SR.special_rays(a, N_PLANES, 7, SR.tree_planes(pt.bvh_read()[0]))
            _, share = check_on_device_tree(pt, oracle, a, ro2, rd2, cls2, oracle_trace(oracle, a, ro2, rd2),
                                            f"{name} {variant}, read-back planes")
            assert share >= 0.9, share
    finally:
        pt.close()


@pytest.mark.gpu
def test_gpu_special_rays_after_a_refit(mcpt_mod, oracle, request):
    """update_geometry (refit) of the floor scene with moved vertices; the rays take their planes from
    the moved mesh and the oracle traces the moved arrays."""
    s, a = scene(mcpt_mod, request, "floor")
    m = RF.refitted_desc_arrays(a)
    ro, rd, cls, ref = reference(oracle, ("floor moved", N_GPU, 4), m, N_GPU, 4)
    pt = mcpt_mod.PathTracer(0)
    try:
        pt.upload_scene(s)
        before = pt.trace_closest(ro, rd)[2]
        pt.update_geometry(m["v0"], m["v1"], m["v2"])
        assert not np.array_equal(before, pt.trace_closest(ro, rd)[2])  # the mesh did move
        _, share = check_on_device_tree(pt, oracle, m, ro, rd, cls, ref, "floor after a refit")
        assert share >= 0.9, share
    finally:
        pt.close()


# ---- GPU: films under axis-aligned directional lights -------------------------------------------
LIGHTS = {"up": (0.0, 1.0, 0.0), "up_negative_zeros": (-0.0, 1.0, -0.0), "along_x": (1.0, 0.0, 0.0),
          "unnormalised_z": (0.0, 0.0, -3.0)}
FW = FH = 48
SPP, DEPTH = 4, 3
FILM_VARIANTS = [("default", {}, False, 1), ("occ_g0", {"MCPT_OCC_G": "0"}, False, 1),
                 ("occ_complete0", {"MCPT_OCC_COMPLETE": "0"}, False, 1), ("primary_hits0", {"MCPT_PRIMARY_HITS": "0"}, False, 1),
                 ("width4", {"MCPT_BVH_WIDTH": "4"}, False, 1), ("ploc", {}, "ploc", 1), ("two_slots", {}, False, 2)]
_LIT = {}


def lit_scene(mcpt_mod, light):
    if light not in _LIT:
        s = floor_scene(mcpt_mod, env=(0.1, 0.1, 0.1), light=LIGHTS[light] if light else None)
        _LIT[light] = (s, s.arrays())
    return _LIT[light]


def film_ctx(mcpt_mod, s, env, gpu_bvh, slots, fixed):
    """A context with the scene uploaded under `env` (MCPT_PRIMARY_HITS is read at creation, the others at upload)."""
    def make():
        pt = mcpt_mod.PathTracer(0, mcpt_mod.default_config(spp=SPP, max_depth=DEPTH, fixed=fixed))
        pt.upload_scene(s, gpu_bvh=gpu_bvh)
        return pt

    pt = with_env(env, make)
    pt.set_camera(mcpt_mod.make_camera((0.5, 2.0, 4.0)))
    if slots != 1:
        pt.set_path_slots(slots)
    pt.resize(FW, FH)
    return pt


@pytest.mark.gpu
@pytest.mark.parametrize("fixed", [False, True], ids=["reference", "fixed"])
@pytest.mark.parametrize("light", list(LIGHTS))
def test_gpu_films_under_axis_aligned_lights(mcpt_mod, oracle, light, fixed):
    """The queued path (k_shade's ray_misses_scene and prefiltered sets, the occluder cache, the
    complete keys, the primary table) with every shadow ray of the frame axis-aligned: the film of
    the floor scene under one directional light equals the oracle's render (sample counts equal,
    radiance within film_close) for every upload variant, and the one-slot variants equal each other
    bit for bit."""
    from test_gpu import film_close

    s, a = lit_scene(mcpt_mod, light)
    cam = mcpt_mod.make_camera((0.5, 2.0, 4.0))
    ref_Ld, ref_smp, _ = oracle.render(a, cam, FW, FH, spp=SPP, max_depth=DEPTH, fixed=fixed)
    dark_Ld, _, _ = oracle.render(lit_scene(mcpt_mod, None)[1], cam, FW, FH, spp=SPP, max_depth=DEPTH, fixed=fixed)
    lit = int((ref_Ld.sum(axis=2) > 2.0 * dark_Ld.sum(axis=2)).sum())
    if light != "unnormalised_z":
        assert lit > 0  # the light reaches the film
    first, line = None, []
    for vname, env, gpu_bvh, slots in FILM_VARIANTS:
        pt = film_ctx(mcpt_mod, s, env, gpu_bvh, slots, fixed)
        pt.render()
        Ld, smp = pt.film()
        rays, occ = pt.ray_counts(), pt.occ_stats()
        pt.close()
        assert np.array_equal(smp, ref_smp), vname
        ok, nbad = film_close(Ld, ref_Ld)
        assert ok, f"{vname}: {nbad} radiance values differ from the oracle"
        if vname == "default":
            first = Ld.copy()
            assert occ[1] and rays["any_hit"] > 0
            assert rays["any_hit_traversed"] > 0  # the cache has not swallowed the class
        elif slots == 1:
            assert np.array_equal(Ld.view(np.uint32), first.view(np.uint32)), f"{vname} differs from the default upload"
        if vname == "occ_g0":
            assert not occ[1]
        line.append(f"{vname} {rays['any_hit_traversed']}/{rays['any_hit']}")
    print(f"{light} fixed={fixed}: {lit} pixels above twice the unlit film; any-hit rays traversed/all: {', '.join(line)}")


@pytest.mark.gpu
@pytest.mark.parametrize("light", list(LIGHTS))
def test_gpu_any_hit_rays_of_the_lit_floor_are_axis_aligned(mcpt_mod, oracle, light):
    """The any-hit rays the shading stage makes on the lit floor scene: the material stage over paths at
    the camera's first hits gives the light and BSDF visibility rays and says which it queued.  (The
    library does not retain the any-hit queue of a film iteration: mcpt_debug_queue_rays(which = 1)
    reports that, so the rays come from mcpt_stage_run MATERIAL, the same kernel on the same paths.)
    At least a third of them have two exactly zero direction components, the oracle's any-hit trace
    returns both outcomes on those, every queued ray equals the oracle's bit for bit, and every ray
    the stage resolved in place (ray_misses_scene) is unoccluded for the oracle."""
    from stage_checks import _same

    s, a = lit_scene(mcpt_mod, light)
    rng = np.random.default_rng(9)
    n = 4096
    o = np.tile(F([0.5, 2.0, 4.0]), (n, 1))
    tgt = np.stack([rng.uniform(-2.5, 3.0, n), rng.uniform(0.0, 1.0, n), rng.uniform(-3.0, 2.0, n)], axis=1)
    d = tgt - o
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)
    tri = oracle.trace_closest(a, o, d)[2]
    k = tri >= 0
    assert k.sum() > 3000
    inv = np.argsort(a["tri_id"])  # scene triangle id -> array index
    n = int(k.sum())
    beta = np.zeros((n, 4), F)
    beta[:, :3] = rng.uniform(0.05, 1.0, (n, 3))
    sidx = rng.integers(0, SPP, n).astype(np.uint32)
    state = {"flags": (np.uint32(1) << np.uint32(1)) | (sidx << np.uint32(13)), "hit_tri": inv[tri[k]].astype(np.int32),
             "ray_o": o[k], "ray_d": d[k], "beta": beta}
    ref = oracle.stage_material(a, state, max_depth=DEPTH, rr_depth=3)
    pt = mcpt_mod.PathTracer(0, mcpt_mod.default_config(spp=SPP, max_depth=DEPTH))
    pt.upload_scene(s)
    pt.set_camera(mcpt_mod.make_camera((0.5, 2.0, 4.0)))
    got = pt.stage("material", state)
    pt.close()
    q = got["queued"]
    ros, rds = [], []
    for bit, vk, o_k, d_k in ((4, 0, "light_o", "light_d"), (8, 1, "bvis_o", "bvis_d")):
        drawn = ~np.isnan(ref[o_k][:, 0])
        qd = (q & bit) > 0
        assert not qd[~drawn].any()
        assert _same(got[o_k][qd], ref[o_k][qd]) and _same(got[d_k][qd], ref[d_k][qd])
        res = drawn & ~qd  # resolved in place: the product says visible
        assert np.all(got["vis"][res, vk] == 1)
        if res.any():
            assert np.all(oracle.trace_any(a, ref[o_k][res], ref[d_k][res]) == 1)
        ros.append(ref[o_k][drawn]), rds.append(ref[d_k][drawn])
    ro, rd = np.concatenate(ros), np.concatenate(rds)
    two = (rd == 0).sum(axis=1) == 2
    assert two.mean() >= 1.0 / 3.0, two.mean()
    vis = oracle.trace_any(a, ro[two], rd[two])
    assert (vis == 0).any() and (vis == 1).any()
    print(f"{light}: {len(ro)} any-hit rays, {two.mean():.3f} with two zero direction components, "
          f"{(vis == 0).mean():.3f} of those occluded, {int(((q & 12) > 0).sum())} paths queued one")
