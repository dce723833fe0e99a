"""Continuation rays the next logic pass is certain to discard (kernels.hip
k_shade / k_material, mcpt_set_skip_discarded): the switch decides only which rays are made, never a
result, so films, sample counts and ray counts with it on and off are bit-identical, and both equal the
oracle's.

What discard_stats counts: every extension ray that was counted but not made, whether or not it would
have entered the scene's box (a marked record has no continuation direction to test).  The rays among
them that a switch-off run resolves in place -- which the traversal never saw anyway -- are counted by
that switch-off run ("doomed_in_place"), so the traversal's saving is the difference of the two."""
import numpy as np
import pytest

from test_primary_hits import CAMS, H, SPP, W

pytestmark = pytest.mark.gpu

# (max_depth, rr_depth): the default; roulette from the first bounce on, where the throughput is
# still (1,1,1); roulette never (only the depth rule); depth and roulette at adjacent vertices; the
# first evaluation being the last bounce; no bounce at all
PAIRS = [(5, 3), (5, 0), (3, 5), (2, 1), (1, 3), (0, 3)]
SCENES = ["c2", "cube", "c1"]  # config 2's camera inside the closed box; NaN frames; a sphere from outside


def camera(mcpt, which):
    if which == "c2":
        return mcpt.config_camera(mcpt.CONFIGS[2], W, H)
    _, pos, yaw, pitch = CAMS[which]
    return mcpt.make_camera(pos, yaw, pitch, aspect=np.float32(W) / np.float32(H))


def make_pt(mcpt, scene, cam, depth, rr, fixed=False, slots=1):
    pt = mcpt.PathTracer(0, mcpt.default_config(spp=SPP, max_depth=depth, rr_depth=rr, tile=64, fixed=fixed))
    pt.upload_scene(scene)
    pt.set_camera(cam)
    pt.resize(W, H, 64, 64)
    pt.set_path_slots(slots)
    return pt


def frame(pt, on):
    pt.set_skip_discarded(on)
    pt.clear()
    st = pt.render()
    L, s = pt.film()
    return dict(L=L.copy().view(np.uint32), s=s.copy(), rays=pt.ray_counts(), skip=pt.discard_stats(),
                st=(st.extend_rays, st.shadow_rays, st.vis_rays), live=st.live_paths)


def on_off(pt):
    on, off = frame(pt, True), frame(pt, False)
    print(f"on {on['rays']} {on['skip']} stages {on['st']}\noff {off['rays']} {off['skip']} stages {off['st']}")
    assert on["live"] == 0 and off["live"] == 0
    assert np.array_equal(on["L"], off["L"]), f"films differ in {(on['L'] != off['L']).sum()} values"
    assert np.array_equal(on["s"], off["s"]), "sample counts differ"
    assert np.all(on["s"][:-1, :-1] == SPP) and np.all(on["s"][-1] == 0) and np.all(on["s"][:, -1] == 0)
    assert on["rays"]["extension"] == off["rays"]["extension"] and on["rays"]["any_hit"] == off["rays"]["any_hit"]
    assert on["st"] == off["st"]
    # the switch-off run makes every ray and skips no evaluation; the switch-on run resolves none of
    # the discarded paths' rays in place (it does not make them)
    assert (off["skip"]["extension_untraced"], off["skip"]["any_hit_untraced"], off["skip"]["evaluations_not_run"]) == (0, 0, 0)
    assert on["skip"]["doomed_in_place"] == 0
    # the traversal's saving: the rays not made, minus those a switch-off run resolves in place
    assert (off["rays"]["extension_traversed"] - on["rays"]["extension_traversed"]
            == on["skip"]["extension_untraced"] - off["skip"]["doomed_in_place"])
    # an evaluation not run is one extension ray, one light ray and at most one BRDF visibility ray
    ev = on["skip"]["evaluations_not_run"]
    assert ev <= on["skip"]["extension_untraced"] and ev <= on["skip"]["any_hit_untraced"] <= 2 * ev
    return on, off


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"d{p[0]}rr{p[1]}")
@pytest.mark.parametrize("fixed", [False, True], ids=["reference", "fixed"])
@pytest.mark.parametrize("slots", [1, 2])
@pytest.mark.parametrize("which", SCENES)
def test_on_off_bit_identity(request, mcpt_mod, which, slots, fixed, pair):
    depth, rr = pair
    scene = request.getfixturevalue(CAMS[which][0])[0]
    cam = camera(mcpt_mod, which)
    if depth == 0:
        # no bounce at all is not a configuration of the product (mcpt_create: max_depth 1..200), with
        # or without the switch: a len-1 path needs its primary hit for the background either way
        with pytest.raises(mcpt_mod.McptError):
            make_pt(mcpt_mod, scene, cam, depth, rr, fixed, slots)
        return
    pt = make_pt(mcpt_mod, scene, cam, depth, rr, fixed, slots)
    on, _ = on_off(pt)
    pt.close()
    sk = on["skip"]
    roulette = sk["extension_untraced"] - sk["evaluations_not_run"]
    if rr >= depth:  # no vertex <= max_depth is beyond rr_depth: the depth rule alone
        assert roulette == 0


@pytest.mark.parametrize("pair", [(5, 3), (1, 3), (5, 0)], ids=lambda p: f"d{p[0]}rr{p[1]}")
def test_against_oracle(mcpt_mod, oracle, scene_c2, pair):
    depth, rr = pair
    cam = camera(mcpt_mod, "c2")
    pt = make_pt(mcpt_mod, scene_c2[0], cam, depth, rr)
    on = frame(pt, True)
    pt.close()
    rL, rs, cnt = oracle.render(scene_c2[1], cam, W, H, SPP, depth, rr)
    want = (cnt["extend_rays"], cnt["shadow_rays"], cnt["vis_rays"])
    nbad = int((on["L"] != np.ascontiguousarray(rL, np.float32).view(np.uint32)).sum())
    print(f"{pair}: {nbad} film values differ from the oracle; rays {on['st']} oracle {want}; {on['skip']}")
    assert np.array_equal(on["s"], rs)
    assert nbad == 0
    assert on["st"] == want


def test_not_vacuous(mcpt_mod, scene_c2):
    """Config 2's camera at the default (5, 3): the rays not made are at least a tenth of the
    extension rays a switch-off run traverses (the oracle counts 24.9 % of the non-primary extension
    rays at 480x270, 8 spp; the share does not depend on resolution, and a tenth leaves room for the
    small film's pixel mix).  At (3, 5) no vertex reaches the roulette: the depth rule alone."""
    cam = camera(mcpt_mod, "c2")
    pt = make_pt(mcpt_mod, scene_c2[0], cam, 5, 3)
    on, off = on_off(pt)
    pt.close()
    sk = on["skip"]
    print(f"(5,3): untraced {sk['extension_untraced']} of {off['rays']['extension_traversed']} traversed with the switch off")
    assert sk["extension_untraced"] * 10 >= off["rays"]["extension_traversed"]
    assert sk["extension_untraced"] > sk["evaluations_not_run"] > 0  # both rules fire
    pt = make_pt(mcpt_mod, scene_c2[0], cam, 3, 5)
    on, _ = on_off(pt)
    pt.close()
    sk = on["skip"]
    assert sk["extension_untraced"] - sk["evaluations_not_run"] == 0 and sk["evaluations_not_run"] > 0


@pytest.mark.parametrize("fixed", [False, True], ids=["reference", "fixed"])
@pytest.mark.parametrize("slots", [1, 2])
def test_mid_frame_toggle(mcpt_mod, scene_c2, slots, fixed):
    """Half the frame's iterations with the switch on, the rest with it off (and the other way round):
    the film is the all-off film.  A marked record or an early termination leaves no state the other
    setting misreads."""
    cam = camera(mcpt_mod, "c2")
    pt = make_pt(mcpt_mod, scene_c2[0], cam, 5, 3, fixed, slots)
    off = frame(pt, False)
    # paths that start together end together: samples per slot x (max_depth + 1) iterations at most
    half = (SPP // slots) * 6 // 2
    for first in (True, False):
        pt.set_skip_discarded(first)
        pt.clear()
        st = pt.iterate(half)
        assert st.live_paths > 0, "the frame was over before the toggle"
        pt.set_skip_discarded(not first)
        st = pt.render()
        L, s = pt.film()
        assert st.live_paths == 0
        assert np.array_equal(L.view(np.uint32), off["L"]), f"first half {'on' if first else 'off'}: films differ"
        assert np.array_equal(s, off["s"])
        rays = pt.ray_counts()
        assert rays["extension"] == off["rays"]["extension"] and rays["any_hit"] == off["rays"]["any_hit"]
    pt.close()
