"""Per-pixel sample budgets and "continue rendering" (mcpt_set_sample_budget,
mcpt_set_spp; k_shade's map instantiation).  Every check rests on the composition property: samples are
keyed by (pixel, sample index) and pixels never share an accumulator, so pixel p under budget map m is
pixel p of a uniform render at spp = m[p] with the same path slots, bit for bit.

Film 33 x 17 with 16 x 16 tiles: partial tiles, a 256-pixel block that straddles rows, and the
never-rendered last row and column."""
import os

import numpy as np
import pytest

from test_primary_hits import CAMS

pytestmark = pytest.mark.gpu

W, H, TILE, DEPTH = 33, 17, 16, 5
SCENES = ["c1", "c2", "cube"]  # a sphere from outside; inside config 2's closed room; NaN frames
VALUES = (0, 1, 2, 5, 8)
MAX_SPP = 2 ** 19 - 256


def camera(mcpt, which):
    if which == "c2":
        return mcpt.config_camera(mcpt.CONFIGS[2], W, H)
    _, pos, yaw, pitch = CAMS[which]
    return mcpt.make_camera(pos, yaw, pitch, aspect=np.float32(W) / np.float32(H))


def make_pt(mcpt, scene, cam, spp, slots=1, fixed=False, compact=False, env=None):
    env = env or {}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        pt = mcpt.PathTracer(0, mcpt.default_config(spp=spp, max_depth=DEPTH, tile=TILE, fixed=fixed))
        pt.upload_scene(scene)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    pt.set_camera(cam)
    pt.set_path_slots(slots)
    if compact:
        pt.set_compact_paths(True)
    pt.resize(W, H, TILE, TILE)
    return pt


def film(pt):
    L, s = pt.film()
    return L.copy().view(np.uint32), s.copy()


def counts(pt):
    """The ray counts that do not depend on which any-hit rays the occluder cache caught (its table is
    filled by racing waves): the cache only moves any-hit rays between 'traversed' and 'resolved by the
    cache', so their sum is the deterministic figure."""
    r = pt.ray_counts()
    return (r["extension"], r["extension_traversed"], r["any_hit"], r["any_hit_traversed"] + r["any_hit_occluder_cache"])


def frame(pt):
    pt.clear()
    st = pt.render()
    assert st.live_paths == 0
    return film(pt) + (counts(pt),)


def budget_map(seed=11):
    return np.random.default_rng(seed).choice(np.array(VALUES, np.uint32), size=(H, W))


def uniform_films(pt, values):
    """{v: (Ld bits, samples)} of uniform renders at spp = v on pt (no map installed)."""
    out = {}
    pt.set_sample_budget(None)
    for v in values:
        pt.set_spp(v)
        out[v] = frame(pt)[:2]
    return out


def composed(uni, m):
    L = np.zeros((H, W, 3), np.uint32)
    s = np.zeros((H, W), np.uint32)
    for v, (Lv, sv) in uni.items():
        L[m == v] = Lv[m == v]
        s[m == v] = sv[m == v]
    return L, s


@pytest.mark.parametrize("fixed", [False, True], ids=["reference", "fixed"])
@pytest.mark.parametrize("compact", [False, True], ids=["full", "compact"])
@pytest.mark.parametrize("slots", [1, 3])
@pytest.mark.parametrize("which", SCENES)
def test_uniform_map_is_no_map(request, mcpt_mod, which, slots, compact, fixed):
    scene = request.getfixturevalue(CAMS[which][0])[0]
    spp = 5
    pt = make_pt(mcpt_mod, scene, camera(mcpt_mod, which), spp, slots, fixed, compact)
    assert pt.adaptive_bytes == 0
    plain = frame(pt)
    pt.set_sample_budget(np.full((H, W), spp, np.uint32))
    mapped = frame(pt)
    assert np.array_equal(pt.sample_budget(), np.full((H, W), spp, np.uint32))
    pt.close()
    print(f"{which} S={slots}: rays {plain[2]} / {mapped[2]}")
    assert np.array_equal(plain[0], mapped[0]), f"films differ in {(plain[0] != mapped[0]).sum()} values"
    assert np.array_equal(plain[1], mapped[1])
    assert np.all(plain[1][:-1, :-1] == spp) and not plain[1][-1].any() and not plain[1][:, -1].any()
    assert plain[2] == mapped[2]


@pytest.mark.parametrize("variant", ["skip_off", "primary_off"])
@pytest.mark.parametrize("fixed", [False, True], ids=["reference", "fixed"])
@pytest.mark.parametrize("slots", [1, 2, 3])
@pytest.mark.parametrize("which", SCENES)
def test_composition(request, mcpt_mod, which, slots, fixed, variant):
    scene = request.getfixturevalue(CAMS[which][0])[0]
    env = {"MCPT_PRIMARY_HITS": "0"} if variant == "primary_off" else None
    pt = make_pt(mcpt_mod, scene, camera(mcpt_mod, which), 8, slots, fixed, env=env)
    if variant == "skip_off":
        pt.set_skip_discarded(False)
    m = budget_map()
    uni = uniform_films(pt, [v for v in VALUES if v])
    uni[0] = (np.zeros((H, W, 3), np.uint32), np.zeros((H, W), np.uint32))
    pt.set_sample_budget(m)
    L, s, _ = frame(pt)
    pt.close()
    wantL, wants = composed(uni, m)
    assert np.array_equal(s, wants)
    assert np.array_equal(s[:-1, :-1], m[:-1, :-1]) and not s[-1].any() and not s[:, -1].any()
    assert np.array_equal(L, wantL), f"{(L != wantL).sum()} film values differ from the uniform renders"


@pytest.mark.parametrize("fixed", [False, True], ids=["reference", "fixed"])
def test_composition_against_the_oracle(mcpt_mod, oracle, scene_c2, fixed):
    """S = 1: expected[p] = the oracle's uniform film at spp = m[p], pixel p (bit for bit on config 2's
    room, as tests/test_skip_discarded.py compares it)."""
    cam = camera(mcpt_mod, "c2")
    m = budget_map()
    pt = make_pt(mcpt_mod, scene_c2[0], cam, 8, 1, fixed)
    pt.set_sample_budget(m)
    L, s, _ = frame(pt)
    pt.close()
    uni = {0: (np.zeros((H, W, 3), np.uint32), np.zeros((H, W), np.uint32))}
    for v in VALUES[1:]:
        rL, rs, _ = oracle.render(scene_c2[1], cam, W, H, v, DEPTH, 3, tile=TILE, fixed=fixed)
        uni[v] = (np.ascontiguousarray(rL, np.float32).view(np.uint32), rs)
    wantL, wants = composed(uni, m)
    assert np.array_equal(s, wants)
    assert np.array_equal(L, wantL), f"{(L != wantL).sum()} film values differ from the oracle"


@pytest.mark.parametrize("compact", [False, True], ids=["full", "compact"])
@pytest.mark.parametrize("slots", [1, 3])
def test_continuation(mcpt_mod, scene_c2, slots, compact):
    cam = camera(mcpt_mod, "c2")
    pt = make_pt(mcpt_mod, scene_c2[0], cam, 8, slots, False, compact)
    direct8 = frame(pt)
    # 3 spp, then on to 8 on the same film: a direct 8-spp frame, rays included
    pt.set_spp(3)
    three = frame(pt)
    assert np.all(three[1][:-1, :-1] == 3)
    pt.set_spp(8)
    st = pt.render()
    assert st.live_paths == 0 and st.extend_rays > 0, "the finished frame's state kept the new samples out"
    assert np.array_equal(film(pt)[0], direct8[0]) and np.array_equal(film(pt)[1], direct8[1])
    assert counts(pt) == direct8[2]
    # the same with a map raised after render() has returned (stale block-done flags and idle word)
    m = budget_map()
    uni = uniform_films(pt, [v for v in VALUES if v])
    uni[0] = (np.zeros((H, W, 3), np.uint32), np.zeros((H, W), np.uint32))
    low = np.minimum(m, 2).astype(np.uint32)
    pt.set_sample_budget(low)
    lowf = frame(pt)
    assert np.array_equal(lowf[1][:-1, :-1], low[:-1, :-1])
    pt.set_sample_budget(m)
    st = pt.render()
    assert st.live_paths == 0 and st.extend_rays > 0
    L, s = film(pt)
    wantL, wants = composed(uni, m)
    assert np.array_equal(s, wants) and np.array_equal(L, wantL)
    # lowering budgets below the counts changes nothing and traces nothing
    pt.set_sample_budget(low)
    st = pt.render()
    assert st.rays == 0 and st.live_paths == 0
    L2, s2 = film(pt)
    assert np.array_equal(L2, L) and np.array_equal(s2, s)
    # a film clear keeps the map (so do slot, tile-set and layout changes) ...
    pt.clear()
    assert np.array_equal(pt.sample_budget(), low)
    pt.set_path_slots(2)
    pt.set_tiles([(0, 0), (2, 1)])
    pt.set_compact_paths(not compact)
    assert np.array_equal(pt.sample_budget(), low)
    pt.set_tiles(None)
    st = pt.render()
    assert np.array_equal(film(pt)[1][:-1, :-1], low[:-1, :-1])
    # ... and a resize drops it
    pt.resize(W, H, TILE, TILE)
    with pytest.raises(mcpt_mod.McptError):
        pt.sample_budget()
    assert pt.adaptive_bytes == 0
    pt.render()
    assert np.all(film(pt)[1][:-1, :-1] == 8)
    pt.close()


def test_rejections(mcpt_mod, scene_c2):
    cam = camera(mcpt_mod, "c2")
    pt = make_pt(mcpt_mod, scene_c2[0], cam, 8, 1)
    m = budget_map()
    pt.set_sample_budget(m)
    # a too-large entry
    bad = m.copy()
    bad[3, 4] = MAX_SPP + 1
    with pytest.raises(mcpt_mod.McptError, match="mcpt error -1"):
        pt.set_sample_budget(bad)
    assert np.array_equal(pt.sample_budget(), m)
    ok = m.copy()
    ok[3, 4] = MAX_SPP  # the largest count is accepted (and put back: nothing is rendered with it)
    pt.set_sample_budget(ok)
    pt.set_sample_budget(m)
    with pytest.raises(mcpt_mod.McptError, match="mcpt error -1"):
        pt.set_spp(MAX_SPP + 1)
    with pytest.raises(mcpt_mod.McptError, match="mcpt error -1"):
        pt.set_spp(-1)
    # paths in flight
    pt.clear()
    st = pt.iterate(1)
    assert st.live_paths > 0
    with pytest.raises(mcpt_mod.McptError, match="mcpt error -1"):
        pt.set_sample_budget(np.full((H, W), 2, np.uint32))
    with pytest.raises(mcpt_mod.McptError, match="mcpt error -1"):
        pt.set_sample_budget(None)
    with pytest.raises(mcpt_mod.McptError, match="mcpt error -1"):
        pt.set_spp(4)
    with pytest.raises(mcpt_mod.McptError, match="mcpt error -1"):
        pt.budget_from_error()
    assert np.array_equal(pt.sample_budget(), m) and pt.cfg.spp == 8
    # the error estimate needs two slots (and a finished iteration)
    with pytest.raises(mcpt_mod.McptError, match="mcpt error -1"):
        pt.film_error()
    pt.render()
    with pytest.raises(mcpt_mod.McptError, match="mcpt error -1"):
        pt.film_error()
    assert np.array_equal(pt.sample_budget(), m)
    assert np.array_equal(film(pt)[1][:-1, :-1], m[:-1, :-1])  # and the frame still finishes under the map
    pt.close()


def test_isolation(mcpt_mod, scene_c2):
    """A context that never calls the adaptive functions holds no memory for them, whatever else it
    does; the first call that needs a buffer allocates that buffer only."""
    cam = camera(mcpt_mod, "c2")
    pt = make_pt(mcpt_mod, scene_c2[0], cam, 2, 2)
    frame(pt)
    pt.set_tiles([(0, 0)])
    pt.set_compact_paths(True)
    pt.set_tiles(None)
    frame(pt)
    pt.set_spp(3)             # a scalar: no memory
    pt.set_sample_budget(None)
    assert pt.adaptive_bytes == 0
    pt.set_sample_budget(np.ones((H, W), np.uint32))
    assert pt.adaptive_bytes == 4 * W * H
    pt.close()
