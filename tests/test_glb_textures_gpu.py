"""A textured glb on the device: tests/glb_fixtures.py's room through
Scene.load_glb(flags=MCPT_GLB_AS_AUTHORED) and PathTracer.upload_scene at 24 x 16, 4 spp, against the same file
dressed by hand through the setters and against tests/texture_srgb_ref.py, bit for bit."""
import numpy as np
import pytest

import glb_fixtures as GF
import texture_srgb_ref as SR

pytestmark = pytest.mark.gpu
W, H, SPP = 24, 16, 4
F = np.float32
RAYS = ("extend_rays", "shadow_rays", "vis_rays")
LIGHT = (-0.2, 0.3, 1.0)  # a directional light through the room's opening: most pixels on the textured walls are lit


def u32(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def film_of(mcpt, scene, cam):
    p = mcpt.PathTracer(0, mcpt.default_config(spp=SPP))
    p.upload_scene(scene)
    p.set_camera(cam)
    p.resize(W, H)
    st = p.render()
    Ld, sm = p.film()
    out = (Ld.copy(), sm.copy(), tuple(int(getattr(st, k)) for k in RAYS), p.texture_stats(), p.textures())
    p.close()
    return out


def test_a_textured_glb_renders_as_authored(mcpt_mod, oracle, tmp_path):
    meshes, mats, px, png = GF.room()
    path = tmp_path / "room.glb"
    path.write_bytes(GF.write(meshes, mats, png))
    s = mcpt_mod.Scene()
    s.load_glb(path, flags=mcpt_mod.MCPT_GLB_AS_AUTHORED)
    s.add_dir_light(LIGHT, (1.0, 1.0, 1.0), 3.0)
    s.build()
    rep = s.glb_report()
    assert rep == {"images_decoded": 4, "images_skipped": 0, "slots_attached": 6, "slots_skipped": 0, "lines": []}
    cam = mcpt_mod.make_camera((0.0, 0.0, 2.4), aspect=F(W) / F(H))
    got = film_of(mcpt_mod, s, cam)
    st, inst = got[3], got[4]
    assert st["in_effect"] and st["srgb_in_effect"] and st["nrm_in_effect"] and st["mr_in_effect"]
    assert (st["textured_materials"], st["mr_materials"], st["nrm_materials"], st["srgb_materials"]) == (4, 1, 1, 4)
    assert len(inst["textures"]) == 4 and [int(f) for f in inst["tex_flags"]] == [1, 1, 0, 1]

    # the same file without flags, its factors and textures set by hand: the same film
    hand = mcpt_mod.Scene()
    hand.load_glb(path, flags=mcpt_mod.MCPT_GLB_PBR_FACTORS)
    hand.set_texture(0, px[0], srgb=True), hand.set_mr_texture(0, px[1]), hand.set_normal_texture(0, px[2], scale=0.75)
    hand.set_texture(1, px[3], srgb=True), hand.set_texture(2, px[3], srgb=True), hand.set_texture(4, px[1], srgb=True)
    hand.add_dir_light(LIGHT, (1.0, 1.0, 1.0), 3.0)
    hand.build()
    p = mcpt_mod.PathTracer(0, mcpt_mod.default_config(spp=SPP))
    p.upload_scene(hand)
    t = hand.textures()  # (the hand-built scene's tangents come from its uvs: install the authored ones)
    p.set_textures(*hand.uv(), t["textures"], t["mat_tex"], mat_mr=t["mat_mr"], tangents=s.tangents(), mat_nrm=t["mat_nrm"],
                   nrm_scale=t["nrm_scale"], tex_flags=t["tex_flags"])
    p.set_camera(cam)
    p.resize(W, H)
    p.render()
    hLd, hsm = p.film()
    p.close()
    assert np.array_equal(u32(got[0]), u32(hLd)) and np.array_equal(got[1], hsm)

    # ... and the reference loop's, with exact ray counts
    a, t = s.arrays(), s.textures()
    uv, tans = s.uv(), s.tangents()
    tex = dict(uv0=uv[0], uv1=uv[1], uv2=uv[2], textures=t["textures"], mat_tex=t["mat_tex"], mat_mr=t["mat_mr"], mat_nrm=t["mat_nrm"],
               nrm_scale=t["nrm_scale"], tan0=tans[0], tan1=tans[1], tan2=tans[2], tex_flags=t["tex_flags"])
    rLd, rsm, rc = SR.render(oracle, a, cam, W, H, SPP, tex=tex)
    stored = SR.render(oracle, a, cam, W, H, SPP, tex=dict(tex, tex_flags=None))
    n = int((rLd != stored[0]).any(axis=2).sum())
    print("pixels the sRGB flags change in the reference film:", n)
    assert n > 100
    assert np.array_equal(got[1], rsm) and np.array_equal(u32(got[0]), u32(rLd)) and got[2] == tuple(rc[k] for k in RAYS)
