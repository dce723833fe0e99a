"""glb material import on the CPU (mcpt_scene_load_glb_ex): tests/glb_fixtures.py's room
loaded as authored against a scene built by hand from the same arrays with add_mesh and the setters, the flags
one by one, and every case that cannot be honoured with its counts and its line in the report.  No GPU."""
import os

import numpy as np
import pytest

import glb_fixtures as GF
import png_fixtures as PF

F = np.float32
GEOMETRY = ("v0", "v1", "v2", "n0", "n1", "n2", "mat", "tri_id")


def u32(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def room(tmp_path_factory):
    meshes, mats, px, png = GF.room()
    path = tmp_path_factory.mktemp("glb") / "room.glb"
    path.write_bytes(GF.write(meshes, mats, png))
    return dict(path=path, meshes=meshes, mats=mats, px=px, png=png)


def load(mcpt, path, flags, build=True):
    s = mcpt.Scene()
    s.load_glb(path, flags=flags)
    if build:
        s.build()
    return s


def hand_arrays(room):
    """Per mesh (v0, v1, v2, n0, n1, n2, uv0, uv1, uv2, base rgb): the triangles as the loader must make them, in
    numpy float32.  A node matrix M moves a position to M p (the fixture's mirror: x -> -x + 0.25, exact) and a
    normal to normalize(transpose(inverse(M)) n), which for the mirror negates x; every normal is then
    n * (1 / sqrt((x x + y y) + z z)), glm's normalize."""
    out = []
    for m, mat in zip(room["meshes"], (0, 1, 1, 2, 3, None)):
        pos, nrm, uv = (np.asarray(m[k], F) for k in ("pos", "nrm", "uv"))
        if m.get("matrix") is not None:
            assert list(m["matrix"]) == GF.MIRROR
            pos = (pos * F([-1, 1, 1]) + F([0.25, 0, 0])).astype(F)
            nrm = (nrm * F([-1, 1, 1])).astype(F)
        d = ((nrm[:, 0] * nrm[:, 0] + nrm[:, 1] * nrm[:, 1]) + nrm[:, 2] * nrm[:, 2]).astype(F)
        nrm = (nrm * (F(1) / np.sqrt(d))[:, None]).astype(F)
        idx = np.asarray(m["idx"]).reshape(-1, 3)
        pbr = room["mats"][mat]["pbrMetallicRoughness"] if mat is not None else {}
        base = pbr.get("baseColorFactor", [1, 1, 1, 1])[:3]
        out.append(tuple(a[idx[:, k]] for a in (pos, nrm, uv) for k in range(3)) + (base,))
    return out


def by_hand(mcpt, room, srgb=True):
    """A scene built from the fixture's arrays with add_mesh, set_uv and the texture setters as the file authors
    them (materials in add order: back wall 0, floor 1, ceiling 2, left 3, right 4, quad 5)."""
    s = mcpt.Scene()
    for k, (v0, v1, v2, n0, n1, n2, uv0, uv1, uv2, base) in enumerate(hand_arrays(room)):
        s.add_mesh(v0, v1, v2, n0, n1, n2, base_rgb=base)
        s.set_uv(k, uv0, uv1, uv2)
    px = room["px"]
    s.set_texture(0, px[0], srgb=srgb)
    s.set_mr_texture(0, px[1])
    s.set_normal_texture(0, px[2], scale=0.75)
    s.set_texture(1, px[3], srgb=srgb)
    s.set_texture(2, px[3], srgb=srgb)
    s.set_texture(4, px[1], srgb=srgb)
    s.build()
    return s


def slot_images(t, key):
    """Per material the image of its slot `key`, or None."""
    return [None if k < 0 else t["textures"][k] for k in t[key]]


def same_images(a, b):
    return len(a) == len(b) and all((x is None and y is None) or (x is not None and y is not None and np.array_equal(x, y)) for x, y in zip(a, b))


def test_as_authored_equals_the_scene_dressed_by_hand(mcpt_mod, room):
    got, hand = load(mcpt_mod, room["path"], mcpt_mod.MCPT_GLB_AS_AUTHORED), by_hand(mcpt_mod, room)
    ga, ha = got.arrays(), hand.arrays()
    for k in GEOMETRY:
        assert np.array_equal(ga[k], ha[k]), k
    assert all(np.array_equal(u32(x), u32(y)) for x, y in zip(got.uv(), hand.uv()))
    gp, hp = np.asarray(ga["mat_params"]).reshape(-1, 8), np.asarray(ha["mat_params"]).reshape(-1, 8)
    assert np.array_equal(u32(gp[:, :6]), u32(hp[:, :6]))
    # the factors as authored, glTF's defaults 1 and 1 (the quad has no material at all)
    want = np.array([[0.6, 0.5], [1.0, 0.0], [1.0, 0.0], [0.3, 1.0], [0.8, 0.25], [1.0, 1.0]], F)
    assert np.array_equal(u32(gp[:, 6:8]), u32(want)) and np.array_equal(hp[:, 6:8], np.tile(F([1, 0]), (6, 1)))
    gt, ht = got.textures(), hand.textures()
    for key in ("mat_tex", "mat_mr", "mat_nrm"):
        assert same_images(slot_images(gt, key), slot_images(ht, key)), key
    assert np.array_equal(u32(gt["nrm_scale"]), u32(ht["nrm_scale"])) and gt["nrm_scale"][0] == F(0.75)
    # one glTF image is one entry, however many slots use it: four images, and image 1 serves two slots
    assert len(gt["textures"]) == 4 and len(ht["textures"]) == 6
    assert gt["mat_mr"][0] == gt["mat_tex"][4] and gt["mat_tex"][1] == gt["mat_tex"][2]
    # the flags: every image a base-colour slot uses, and only those (image 1 is MR on material 0 and base on 4)
    base_used = set(int(k) for k in gt["mat_tex"] if k >= 0)
    assert [int(f) for f in gt["tex_flags"]] == [1 if k in base_used else 0 for k in range(4)]
    assert gt["tex_flags"][gt["mat_nrm"][0]] == 0
    rep = got.glb_report()
    assert rep == {"images_decoded": 4, "images_skipped": 0, "slots_attached": 6, "slots_skipped": 0, "lines": []}


def test_authored_tangents_follow_the_node_and_the_rest_come_from_the_uvs(mcpt_mod, room):
    """The back wall's TANGENTs under its mirroring node: T' = normalize(M3 T) (here x negated) and s' = -s (det
    < 0); every other triangle keeps mcpt_tangents_from_uv's."""
    got, hand = load(mcpt_mod, room["path"], mcpt_mod.MCPT_GLB_TEXTURES), by_hand(mcpt_mod, room)
    a = got.arrays()
    tid, mat = np.asarray(a["tri_id"]), np.asarray(a["mat"])
    back = mat == 0
    assert back.sum() == 2
    t = np.asarray(room["meshes"][0]["tan"], F)
    v = (t[:, :3] * F([-1, 1, 1])).astype(F)
    d = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
    want = np.concatenate([v * (F(1) / np.sqrt(d))[:, None], -t[:, 3:4]], 1).astype(F)
    idx = np.asarray(room["meshes"][0]["idx"]).reshape(-1, 3)
    gt, ht = got.tangents(), hand.tangents()
    for i in np.flatnonzero(back):
        for k in range(3):
            assert np.array_equal(u32(gt[k][i]), u32(want[idx[tid[i]][k]])), (i, k)
    for k in range(3):
        assert np.array_equal(u32(gt[k][~back]), u32(ht[k][~back]))
        assert not np.array_equal(u32(gt[k][back]), u32(ht[k][back]))


@pytest.mark.parametrize("name", ["room", "Cube.glb"])
def test_flags_0_is_load_glb(mcpt_mod, room, name):
    path = room["path"] if name == "room" else os.path.join(mcpt_mod.ASSET_DIR, name)
    a, b = mcpt_mod.Scene(), mcpt_mod.Scene()
    a.load_glb(path)
    assert mcpt_mod.lib().mcpt_scene_load_glb_ex(b.h, str(path).encode(), None, 0) == 0
    a.build(), b.build()
    x, y = a.arrays(), b.arrays()
    assert set(x) == set(y)
    for k in x:
        assert np.array_equal(np.asarray(x[k]), np.asarray(y[k])), k
    assert a.textures() is None and b.textures() is None
    assert all(np.array_equal(p, q) for p, q in zip(a.uv(), b.uv())) and all(np.array_equal(p, q) for p, q in zip(a.tangents(), b.tangents()))
    assert b.glb_report()["slots_attached"] == 0
    assert mcpt_mod.lib().mcpt_scene_load_glb_ex(b.h, str(path).encode(), None, 8) == -1


def test_each_flag_changes_only_its_own_fields(mcpt_mod, room):
    M = mcpt_mod
    plain = load(M, room["path"], 0)
    pa = plain.arrays()
    f = load(M, room["path"], M.MCPT_GLB_PBR_FACTORS)
    fa = f.arrays()
    assert f.textures() is None and all(np.array_equal(u32(p), u32(q)) for p, q in zip(f.tangents(), plain.tangents()))
    assert np.array_equal(np.asarray(fa["mat_params"]).reshape(-1, 8)[:, :6], np.asarray(pa["mat_params"]).reshape(-1, 8)[:, :6])
    assert not np.array_equal(np.asarray(fa["mat_params"]), np.asarray(pa["mat_params"]))
    t = load(M, room["path"], M.MCPT_GLB_TEXTURES)
    assert np.array_equal(np.asarray(t.arrays()["mat_params"]), np.asarray(pa["mat_params"]))
    tt = t.textures()
    assert "tex_flags" not in tt and len(tt["textures"]) == 4 and (tt["mat_nrm"] >= 0).sum() == 1
    s = load(M, room["path"], M.MCPT_GLB_SRGB)  # alone: no texture is attached, so nothing carries the flag
    assert s.textures() is None and np.array_equal(np.asarray(s.arrays()["mat_params"]), np.asarray(pa["mat_params"]))
    ts = load(M, room["path"], M.MCPT_GLB_TEXTURES | M.MCPT_GLB_SRGB).textures()
    assert "tex_flags" in ts and same_images(slot_images(ts, "mat_tex"), slot_images(tt, "mat_tex"))
    for x in (f, t, s):
        for k in GEOMETRY:
            assert np.array_equal(x.arrays()[k], pa[k]), k


def unhonoured(room):
    """name -> (glb bytes, word of the report line, images skipped, slots skipped): material 1's base-colour slot
    (image 3) is the one that cannot be honoured."""
    meshes, mats, png = room["meshes"], room["mats"], room["png"]

    def variant(info=None, image=None, samplers=None, textures=None):
        m = [dict(x) for x in mats]
        pbr = dict(m[1]["pbrMetallicRoughness"])
        pbr["baseColorTexture"] = dict(pbr["baseColorTexture"], **(info or {}))
        m[1]["pbrMetallicRoughness"] = pbr
        ims = list(png)
        if image is not None:
            ims[3] = image
        return GF.write(meshes, m, ims, samplers=samplers, textures=textures)

    tex = lambda **k: [{"source": 0}, {"source": 1}, {"source": 2}, dict({"source": 3}, **k)]
    bad_png = png[3][:-20] + bytes([png[3][-20] ^ 1]) + png[3][-19:]
    return {
        "jpeg": (variant(image={"mimeType": "image/jpeg", "_payload": b"\xff\xd8\xff\xe0" + bytes(32)}), "image/jpeg", 1, 2),
        "uri": (variant(image={"uri": "wall.png"}), "uri", 1, 2),
        "texCoord": (variant(info={"texCoord": 1}), "texCoord", 0, 2),
        "transform": (variant(info={"extensions": {"KHR_texture_transform": {"scale": [2, 2]}}}), "KHR_texture_transform", 0, 2),
        "clamp": (variant(samplers=[{"wrapS": 33071}], textures=tex(sampler=0)), "REPEAT", 0, 2),
        "mirror T": (variant(samplers=[{"wrapT": 33648, "wrapS": 10497}], textures=tex(sampler=0)), "REPEAT", 0, 2),
        "refused png": (variant(image=bad_png), "png:", 1, 2),
        "texture index": (variant(info={"index": 9}), "out of range", 0, 2),
        "image index": (variant(textures=tex(source=7)), "out of range", 0, 2),
        "sampler index": (variant(samplers=[{}], textures=tex(sampler=3)), "out of range", 0, 2),
    }


@pytest.mark.parametrize("name", ["jpeg", "uri", "texCoord", "transform", "clamp", "mirror T", "refused png", "texture index",
                                  "image index", "sampler index"])
def test_what_cannot_be_honoured_leaves_the_slot_empty(mcpt_mod, room, tmp_path, name):
    data, word, im_skipped, slots_skipped = unhonoured(room)[name]
    (tmp_path / "v.glb").write_bytes(data)
    s = load(mcpt_mod, tmp_path / "v.glb", mcpt_mod.MCPT_GLB_AS_AUTHORED)  # the load is MCPT_OK
    t, rep = s.textures(), s.glb_report()
    print(name, rep)
    assert list(t["mat_tex"][[1, 2]]) == [-1, -1] and t["mat_tex"][0] >= 0 and t["mat_tex"][4] >= 0  # floor and ceiling share material 1
    p = np.asarray(s.arrays()["mat_params"]).reshape(-1, 8)
    assert np.array_equal(p[1, 6:8], F([1, 0]))  # the factors still apply
    assert rep["images_skipped"] == im_skipped and rep["slots_skipped"] == slots_skipped
    assert rep["images_decoded"] == 3 and rep["slots_attached"] == 4 and len(t["textures"]) == 3
    lines = [l for l in rep["lines"] if l.startswith("material 1 baseColorTexture")]
    assert len(lines) == 2 and all(word in l for l in lines), rep["lines"]


def test_a_repeat_sampler_with_filters_is_honoured(mcpt_mod, room, tmp_path):
    tex = [{"source": j, "sampler": 0} for j in range(4)]
    data = GF.write(room["meshes"], room["mats"], room["png"], samplers=[{"wrapS": 10497, "magFilter": 9728, "minFilter": 9987}], textures=tex)
    (tmp_path / "s.glb").write_bytes(data)
    rep = load(mcpt_mod, tmp_path / "s.glb", mcpt_mod.MCPT_GLB_AS_AUTHORED).glb_report()
    assert rep["slots_attached"] == 6 and rep["slots_skipped"] == 0


def test_setters_leave_the_other_slots_of_a_shared_image(mcpt_mod, room):
    """After an as-authored load image 1 is material 0's MR texture and material 4's base colour, and image 3 the
    base colour of materials 1 and 2: a setter on one of those slots appends a texture and the other slot keeps
    its image; a slot that alone uses its entry is replaced in place."""
    s = load(mcpt_mod, room["path"], mcpt_mod.MCPT_GLB_AS_AUTHORED, build=False)
    px = room["px"]
    new = np.full((2, 2, 4), 9, np.uint8)
    s.set_texture(4, new)  # shared with material 0's MR slot
    s.set_texture(2, new, srgb=True)  # shared with material 1's base slot
    t = s.textures()
    assert len(t["textures"]) == 6 and t["mat_tex"][4] == 4 and t["mat_tex"][2] == 5
    assert np.array_equal(t["textures"][t["mat_mr"][0]], px[1]) and np.array_equal(t["textures"][t["mat_tex"][1]], px[3])
    assert np.array_equal(t["textures"][4], new) and np.array_equal(t["textures"][5], new)
    assert [int(f) for f in t["tex_flags"]] == [1, 1, 0, 1, 0, 1]  # the kept entries keep their flags
    s.set_normal_texture(0, new, scale=2.0)  # material 0 alone uses image 2: replaced in place
    s.set_texture(4, px[0])  # ... and material 4 alone uses entry 4 now
    t = s.textures()
    assert len(t["textures"]) == 6 and t["mat_nrm"][0] == 2 and np.array_equal(t["textures"][2], new)
    assert t["mat_tex"][4] == 4 and np.array_equal(t["textures"][4], px[0])
    assert np.array_equal(t["textures"][t["mat_mr"][0]], px[1]) and np.array_equal(t["textures"][t["mat_tex"][0]], px[0])


@pytest.mark.parametrize("bad", ["zero", "nan", "handedness"])
def test_a_degenerate_tangent_falls_back_to_the_uvs(mcpt_mod, room, tmp_path, bad):
    """One bad vertex (a zero tangent, a NaN, a handedness that is not +-1): the primitive takes the uv-derived
    tangents, every texture stays attached, the report names it, and the tangents are finite (the texture set's
    install refuses non-finite ones)."""
    meshes = [dict(m) for m in room["meshes"]]
    t = np.array(meshes[0]["tan"], F)
    if bad == "zero":
        t[2, :3] = 0
    elif bad == "nan":
        t[1, 0] = np.nan
    else:
        t[3, 3] = 0.5
    meshes[0]["tan"] = t
    (tmp_path / "t.glb").write_bytes(GF.write(meshes, room["mats"], room["png"]))
    s = load(mcpt_mod, tmp_path / "t.glb", mcpt_mod.MCPT_GLB_AS_AUTHORED)
    rep = s.glb_report()
    assert rep["slots_attached"] == 6 and rep["slots_skipped"] == 0 and (s.textures()["mat_nrm"] >= 0).sum() == 1
    assert len(rep["lines"]) == 1 and rep["lines"][0].startswith("material 0 TANGENT") and "degenerate" in rep["lines"][0]
    plain = load(mcpt_mod, tmp_path / "t.glb", 0)
    for g, w in zip(s.tangents(), plain.tangents()):
        assert np.isfinite(g).all() and np.array_equal(u32(g), u32(w))
