"""Primary hits from the per-pixel candidate table (kernels.hip k_primary,
scene_tables.hip k_primary_build): the table decides only which primary rays skip the traversal, never a hit, so films,
sample counts and ray counts with it and with MCPT_PRIMARY_HITS=0 are bit-identical."""
import os
import subprocess

import numpy as np
import pytest

from conftest import REPO

W, H, SPP, DEPTH = 64, 48, 8, 5


def make_pt(mcpt, scene, cam, w=W, h=H, env=None, slots=1, tiny=False):
    """A context rendering `scene` from `cam`; env: variables set while it is created and the scene
    uploaded (MCPT_PRIMARY_HITS is read at creation, MCPT_BVH_WIDTH at upload)."""
    env = env or {}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        pt = mcpt.PathTracer(0, mcpt.default_config(spp=SPP, max_depth=DEPTH, tile=64))
        pt.upload_scene(scene)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    pt.set_camera(cam)
    pt.resize(w, h, 64, 64)
    pt.set_path_slots(slots)
    if tiny:
        pt.set_tiny_lds_stack(True)
    return pt


def frame(pt):
    pt.clear()
    pt.render()
    L, s = pt.film()
    return L.copy().view(np.uint32), s.copy(), pt.ray_counts(), pt.primary_stats()


def on_off(mcpt, scene, cam, w=W, h=H, env=None, tiny=False):
    off_env = dict(env or {}, MCPT_PRIMARY_HITS="0")
    pts = make_pt(mcpt, scene, cam, w, h, env, tiny=tiny), make_pt(mcpt, scene, cam, w, h, off_env, tiny=tiny)
    on, off = frame(pts[0]), frame(pts[1])
    for p in pts:
        p.close()
    assert off[3]["lists"] == 0 and off[3]["resolved"] == 0 and off[3]["builds"] == 0
    assert np.array_equal(on[0], off[0]), "films differ"
    assert np.array_equal(on[1], off[1]), "sample counts differ"
    assert on[2]["extension"] == off[2]["extension"]
    # every ray the table resolved is one the traversal did not see, and nothing else changed
    assert off[2]["extension_traversed"] - on[2]["extension_traversed"] == on[3]["resolved"]
    assert on[2]["any_hit"] == off[2]["any_hit"]
    return on, off


# (scene fixture, camera position, yaw, pitch): inside / outside the root box, and exactly along -z
CAMS = {
    "c1": ("scene_c1", (0.0, 0.0, 4.0), -90.0, 0.0),          # config 1's sphere, from outside (along -z)
    "c2": ("scene_c2", (0.0, 0.0, 3.5), -90.0, 0.0),          # the config-2 proxy, inside its closed box
    "c2_tilt": ("scene_c2", (0.4, 0.3, 3.0), -97.0, -6.0),
    "cube": ("scene_cube", (0.3, 0.1, 3.0), -90.0, 0.0),      # axis-aligned faces and NaN frames, from outside
    "cube_in": ("scene_cube", (0.1, 0.05, 0.2), -60.0, 20.0),  # inside the cube (and its root box)
    "cube_axis": ("scene_cube", (0.0, 0.0, 3.0), -90.0, 0.0),  # looking exactly along -z at the face centre
}


@pytest.mark.gpu
@pytest.mark.parametrize("lens", [1e-4, 0.0, 0.05])
@pytest.mark.parametrize("which", list(CAMS))
def test_on_off_bit_identity(request, mcpt_mod, which, lens):
    fx, pos, yaw, pitch = CAMS[which]
    scene = request.getfixturevalue(fx)[0]
    cam = mcpt_mod.make_camera(pos, yaw, pitch, aspect=np.float32(W) / np.float32(H), lens_radius=lens)
    on, _ = on_off(mcpt_mod, scene, cam)
    st = on[3]
    print(f"{which} lens {lens}: lists {st['lists']} overflow {st['overflow']} resolved {st['resolved']} "
          f"of {on[2]['extension']} extension rays, build {st['build_ms']:.3f} ms")
    assert st["lists"] + st["overflow"] == W * H and st["builds"] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("lens", [1e-4, 0.0])
def test_zero_direction_column(mcpt_mod, scene_cube, lens):
    """An odd film under a camera looking exactly along -z: the centre column and row have NDC 0, so
    their rays have a zero direction component (a non-finite inverse: such rays are traversed)."""
    cam = mcpt_mod.make_camera((0.0, 0.0, 3.0), -90.0, 0.0, aspect=np.float32(65) / np.float32(49), lens_radius=lens)
    on_off(mcpt_mod, scene_cube[0], cam, 65, 49)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["width4", "tiny_stack"])
def test_on_off_traversal_variants(mcpt_mod, scene_c2, variant):
    cam = mcpt_mod.config_camera(mcpt_mod.CONFIGS[2], W, H)
    env = {"MCPT_BVH_WIDTH": "4"} if variant == "width4" else None
    on, _ = on_off(mcpt_mod, scene_c2[0], cam, env=env, tiny=variant == "tiny_stack")
    assert on[3]["resolved"] > 0


@pytest.mark.gpu
def test_not_vacuous(mcpt_mod, scene_c2):
    """Config 2, default lens.  The first iteration generates one primary ray per rendered pixel (the
    last column and row are never rendered); with a pinhole camera and the table off, the rays it queues
    for the traversal are exactly the rendered pixels whose pinhole ray enters the root box (k_shade
    resolves the others in place).  With the table, the lists must resolve the primary rays of at least
    half of those pixels, and over the frame the traversal sees exactly the resolved rays fewer.  The
    bound is on the rays the first iteration resolves, not on primary_stats' "lists": that count includes
    the empty lists of pixels outside the root box, which would satisfy "half the pixels" on their own."""
    rc = mcpt_mod.CONFIGS[2]
    cam = mcpt_mod.config_camera(rc, W, H)
    assert abs(cam.lens_radius - 1e-4) < 1e-9
    pin = mcpt_mod.make_camera(rc.position, rc.yaw, rc.pitch, rc.fovy, aspect=np.float32(W) / np.float32(H), lens_radius=0.0)
    ref = make_pt(mcpt_mod, scene_c2[0], pin, env={"MCPT_PRIMARY_HITS": "0"})
    ref.clear()
    ref.iterate(1)
    entering = ref.ray_counts()["extension_traversed"]
    ref.close()
    pt = make_pt(mcpt_mod, scene_c2[0], cam)
    pt.clear()
    pt.iterate(1)
    first = pt.primary_stats()
    pt.close()
    print(f"config 2: {entering} of the {(W - 1) * (H - 1)} rendered pixels' pinhole rays enter the root box; lists {first['lists']}, "
          f"overflow {first['overflow']} of {W * H} pixels; first iteration resolved {first['resolved']}")
    assert entering > 0 and first["resolved"] * 2 >= entering
    on, off = on_off(mcpt_mod, scene_c2[0], cam)
    assert on[3]["resolved"] > 0
    assert off[2]["extension_traversed"] - on[2]["extension_traversed"] == on[3]["resolved"]


@pytest.mark.gpu
def test_invalidation(mcpt_mod, scene_c2, scene_cube):
    """Camera, scene and film size each rebuild the table (the frame equals a fresh context's); a film
    clear alone does not (the build counter stays)."""
    cam_a = mcpt_mod.config_camera(mcpt_mod.CONFIGS[2], W, H)
    cam_b = mcpt_mod.make_camera((0.4, 0.3, 3.0), -97.0, -6.0, aspect=np.float32(W) / np.float32(H))

    def fresh(scene, cam, w, h):
        p = make_pt(mcpt_mod, scene, cam, w, h)
        f = frame(p)
        p.close()
        return f

    pt = make_pt(mcpt_mod, scene_c2[0], cam_a)
    f0 = frame(pt)
    assert f0[3]["builds"] == 1
    f1 = frame(pt)  # a film clear alone
    assert f1[3]["builds"] == 1 and np.array_equal(f0[0], f1[0]) and f1[3]["resolved"] == f0[3]["resolved"]
    steps = [("camera", scene_c2[0], cam_b, W, H), ("scene", scene_cube[0], cam_b, W, H), ("film size", scene_cube[0], cam_b, 80, 40)]
    builds = 1
    for what, scene, cam, w, h in steps:
        if what == "camera":
            pt.set_camera(cam)
        elif what == "scene":
            pt.upload_scene(scene)
        else:
            pt.resize(w, h, 64, 64)
        got, ref = frame(pt), fresh(scene, cam, w, h)
        builds += 1
        assert got[3]["builds"] == builds, what
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), what
        # (which any-hit rays the occluder cache resolves depends on racy stores; the totals do not)
        assert all(got[2][k] == ref[2][k] for k in ("extension", "extension_traversed", "any_hit")), what
        assert (got[3]["lists"], got[3]["overflow"], got[3]["resolved"]) == (ref[3]["lists"], ref[3]["overflow"], ref[3]["resolved"]), what
    pt.close()


def test_primary_beam_host():
    """The interval bound on the CPU (tests/native/primary_beam.cpp, built by the Makefile like the other
    native test): gen_ray_lens's origin, direction and inverse direction lie inside the pixel's intervals
    for random cameras, pixels and lens draws; a box the beam provably misses fails the ray's slab test; a
    triangle it sees back-facing is rejected."""
    subprocess.run(["make", "tests/native/primary_beam"], cwd=REPO, check=True, capture_output=True)
    r = subprocess.run([os.path.join(REPO, "tests", "native", "primary_beam")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "bad=0" in r.stdout
