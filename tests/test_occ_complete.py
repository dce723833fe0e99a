"""Complete keys of the any-hit occluder table (device/occ_beam.hpp, scene_tables.hip
k_occ_complete, kernels.hip occ_hit1): an entry that lists every triangle a ray of its key can be accepted on resolves
such a ray either way, so films, sample counts and ray totals with the lists and with MCPT_OCC_COMPLETE=0
are bit-identical, and the rays the lists resolve are exactly the rays that leave the traversal.

The accounting.  Of the any-hit rays that are not resolved where they are made, each is either traversed
(any_hit_traversed), resolved as occluded by a table entry (any_hit_occluder_cache; this includes the
"occluded" count of occ_complete_stats) or resolved as unoccluded by a complete entry ("unoccluded").  Which
occluded rays the recorded occluders catch depends on racy stores and differs between any two contexts, on
or off, so the traversed counts alone are not comparable; the rays that needed the traversal or a recorded
occluder are:  traversed + cache - occluded(complete).  With the lists that number is the number without
them minus the rays resolved from complete entries (unoccluded + occluded), which is what is asserted."""
import os
import subprocess

import numpy as np
import pytest

from conftest import REPO

W, H, SPP, DEPTH = 64, 48, 8, 5


def make_pt(mcpt, scene, cam, env=None, slots=1, fixed=False):
    """A context rendering `scene` from `cam`; env: variables set while the scene is uploaded
    (MCPT_OCC_COMPLETE and MCPT_BVH_WIDTH are read at upload)."""
    env = env or {}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        pt = mcpt.PathTracer(0, mcpt.default_config(spp=SPP, max_depth=DEPTH, tile=64, fixed=fixed))
        pt.upload_scene(scene)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    pt.set_camera(cam)
    pt.resize(W, H, 64, 64)
    pt.set_path_slots(slots)
    return pt


def frame(pt):
    pt.clear()
    pt.render()
    L, s = pt.film()
    return dict(L=L.copy().view(np.uint32), s=s.copy(), rays=pt.ray_counts(), done=pt.occ_complete_stats())


def needed(f):
    """any-hit rays that needed the traversal or a recorded occluder"""
    return f["rays"]["any_hit_traversed"] + f["rays"]["any_hit_occluder_cache"] - f["done"]["occluded"]


# (scene fixture, camera position, yaw, pitch) as in test_primary_hits.py; None: config 2's own camera
CAMS = {
    "c1": ("scene_c1", (0.0, 0.0, 4.0), -90.0, 0.0),
    "c2": ("scene_c2", (0.0, 0.0, 3.5), -90.0, 0.0),
    "c2_tilt": ("scene_c2", (0.4, 0.3, 3.0), -97.0, -6.0),
    "c2_config": ("scene_c2", None, 0.0, 0.0),
    "cube": ("scene_cube", (0.3, 0.1, 3.0), -90.0, 0.0),
    "cube_in": ("scene_cube", (0.1, 0.05, 0.2), -60.0, 20.0),
    "cube_axis": ("scene_cube", (0.0, 0.0, 3.0), -90.0, 0.0),
}


@pytest.mark.gpu
@pytest.mark.parametrize("width", ["pair", "width4"])
@pytest.mark.parametrize("fixed", [False, True], ids=["reference", "fixed"])
@pytest.mark.parametrize("slots", [1, 4])
@pytest.mark.parametrize("which", list(CAMS))
def test_on_off_bit_identity(request, mcpt_mod, which, slots, fixed, width):
    fx, pos, yaw, pitch = CAMS[which]
    scene = request.getfixturevalue(fx)[0]
    if pos is None:
        cam = mcpt_mod.config_camera(mcpt_mod.CONFIGS[2], W, H)
    else:
        cam = mcpt_mod.make_camera(pos, yaw, pitch, aspect=np.float32(W) / np.float32(H))
    env = {"MCPT_BVH_WIDTH": "4"} if width == "width4" else {}
    pt_on = make_pt(mcpt_mod, scene, cam, env, slots, fixed)
    pt_off = make_pt(mcpt_mod, scene, cam, dict(env, MCPT_OCC_COMPLETE="0"), slots, fixed)
    on, off, on2 = frame(pt_on), frame(pt_off), frame(pt_on)
    pt_on.close()
    pt_off.close()
    d = on["done"]
    print(f"{which} slots {slots} {'fixed' if fixed else 'reference'} {width}: complete keys {d['keys']} built in "
          f"{d['build_ms']:.2f} ms; of {on['rays']['any_hit']} any-hit rays {d['unoccluded']} resolved unoccluded, "
          f"{d['occluded']} occluded from complete entries; traversed {on['rays']['any_hit_traversed']} on, "
          f"{off['rays']['any_hit_traversed']} off; recorded-occluder hits {on['rays']['any_hit_occluder_cache']} on, "
          f"{off['rays']['any_hit_occluder_cache']} off; second frame {on2['done']['unoccluded']} / {on2['done']['occluded']}")
    assert off["done"]["keys"] == 0 and off["done"]["unoccluded"] == 0 and off["done"]["occluded"] == 0
    assert np.array_equal(on["L"], off["L"]), "films differ"
    assert np.array_equal(on["s"], off["s"]), "sample counts differ"
    for k in ("extension", "extension_traversed", "any_hit"):
        assert on["rays"][k] == off["rays"][k], k
    assert d["occluded"] <= on["rays"]["any_hit_occluder_cache"]
    # every ray a complete entry resolved is one that left the traversal, and nothing else changed
    assert needed(on) == needed(off) - (d["unoccluded"] + d["occluded"])
    if which == "c2_config":
        assert d["keys"] > 0 and d["unoccluded"] + d["occluded"] > 0
    # a second frame: the film clear restored the table (the complete lists with it)
    assert np.array_equal(on2["L"], on["L"]) and np.array_equal(on2["s"], on["s"])
    for k in ("extension", "extension_traversed", "any_hit"):
        assert on2["rays"][k] == on["rays"][k], k
    assert on2["done"]["keys"] == d["keys"]
    assert needed(on2) == needed(off) - (on2["done"]["unoccluded"] + on2["done"]["occluded"])
    assert (on2["done"]["unoccluded"] > 0) == (d["unoccluded"] > 0)


def test_occ_beam_host():
    """The candidate lists on the CPU (tests/native/occ_beam.cpp, built by the Makefile like the other native
    tests): for a cube, a sphere in a box and a triangle soup, every triangle the scalar acceptance takes for a
    ray of a key's beam is in the key's list whenever the key is complete; at least 1000 rays per scene are
    checked and at least half of the cube's sampled keys are complete (the program fails otherwise)."""
    subprocess.run(["make", "tests/native/occ_beam"], cwd=REPO, check=True, capture_output=True)
    r = subprocess.run([os.path.join(REPO, "tests", "native", "occ_beam")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "bad=0" in r.stdout and "VACUOUS" not in r.stdout
