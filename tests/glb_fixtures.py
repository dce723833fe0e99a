"""glb files from arrays, written with json and struct: the inputs of tests/test_glb_textures_host.py and
tests/test_glb_textures_gpu.py.

write(meshes, materials, images, samplers=None, textures=None) -> bytes.  A mesh is a dict {"pos", "nrm": (nv, 3),
"uv": (nv, 2) or None, "tan": (nv, 4) or None, "idx": (ntri * 3,) uint32, "material": index or None, "matrix":
16 floats column-major or None}; each becomes one node with one single-primitive mesh.  A material is a glTF
material dict as it goes into the JSON.  An image is PNG bytes (embedded, image/png), or a dict that goes into the
JSON as it is (a uri, another mimeType) with an optional "_payload" of bytes to embed.  textures defaults to one
per image, {"source": j}.

room() is the fixture the two test files share: a five-wall room plus a quad, four materials."""
import json
import struct

import numpy as np

import png_fixtures as PF

F = np.float32


def write(meshes, materials, images, samplers=None, textures=None):
    bin_ = bytearray()
    views, accessors = [], []

    def view(data):
        while len(bin_) % 4:
            bin_.append(0)
        views.append({"buffer": 0, "byteOffset": len(bin_), "byteLength": len(data)})
        bin_.extend(data)
        return len(views) - 1

    def accessor(a, ctype, kind):
        a = np.ascontiguousarray(a)
        acc = {"bufferView": view(a.tobytes()), "componentType": ctype, "count": int(a.shape[0]), "type": kind}
        if kind == "VEC3" and ctype == 5126:
            acc["min"], acc["max"] = a.min(0).tolist(), a.max(0).tolist()
        accessors.append(acc)
        return len(accessors) - 1

    nodes, jmeshes = [], []
    for m in meshes:
        attrs = {"POSITION": accessor(np.asarray(m["pos"], F), 5126, "VEC3"), "NORMAL": accessor(np.asarray(m["nrm"], F), 5126, "VEC3")}
        if m.get("uv") is not None:
            attrs["TEXCOORD_0"] = accessor(np.asarray(m["uv"], F), 5126, "VEC2")
        if m.get("tan") is not None:
            attrs["TANGENT"] = accessor(np.asarray(m["tan"], F), 5126, "VEC4")
        prim = {"attributes": attrs, "indices": accessor(np.asarray(m["idx"], np.uint32), 5125, "SCALAR")}
        if m.get("material") is not None:
            prim["material"] = int(m["material"])
        jmeshes.append({"primitives": [prim]})
        node = {"mesh": len(jmeshes) - 1}
        if m.get("matrix") is not None:
            node["matrix"] = [float(x) for x in m["matrix"]]
        nodes.append(node)
    jimages = []
    for im in images:
        if isinstance(im, (bytes, bytearray)):
            jimages.append({"bufferView": view(im), "mimeType": "image/png"})
        else:
            d = {k: v for k, v in im.items() if k != "_payload"}
            if "_payload" in im:
                d["bufferView"] = view(im["_payload"])
            jimages.append(d)
    doc = {"asset": {"version": "2.0"}, "scene": 0, "scenes": [{"nodes": list(range(len(nodes)))}], "nodes": nodes,
           "meshes": jmeshes, "accessors": accessors, "bufferViews": views, "materials": materials}
    if jimages:
        doc["images"] = jimages
        doc["textures"] = textures if textures is not None else [{"source": j} for j in range(len(jimages))]
    if samplers:
        doc["samplers"] = samplers
    while len(bin_) % 4:
        bin_.append(0)
    doc["buffers"] = [{"byteLength": len(bin_)}]
    js = json.dumps(doc).encode()
    js += b" " * (-len(js) % 4)
    body = struct.pack("<II", len(js), 0x4E4F534A) + js + struct.pack("<II", len(bin_), 0x004E4942) + bytes(bin_)
    return struct.pack("<4sII", b"glTF", 2, 12 + len(body)) + body


def quad(p0, eu, ev, n, uv_scale=1.0):
    """Two triangles over p0, p0 + eu, p0 + eu + ev, p0 + ev with normal n and uvs (0, 0) .. (uv_scale, uv_scale)."""
    p0, eu, ev = (np.asarray(x, F) for x in (p0, eu, ev))
    pos = np.stack([p0, p0 + eu, p0 + eu + ev, p0 + ev]).astype(F)
    uv = (np.array([[0, 0], [1, 0], [1, 1], [0, 1]], F) * F(uv_scale) + F(0.125)).astype(F)
    return dict(pos=pos, nrm=np.tile(np.asarray(n, F), (4, 1)), uv=uv, idx=np.array([0, 1, 2, 0, 2, 3], np.uint32))


MIRROR = [-1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0, 0.25, 0, 0, 1.0]  # x -> -x + 0.25: det < 0


def images(seed=3):
    """(arrays, PNG bytes): four random RGBA images; the normal image's B lies in 128..255."""
    rng = np.random.default_rng(seed)
    px = [rng.integers(0, 256, (h, w, 4)).astype(np.uint8) for h, w in ((8, 8), (5, 3), (6, 7), (4, 4))]
    px[2][..., 2] = rng.integers(128, 256, px[2].shape[:2]).astype(np.uint8)
    return px, [PF.write(p, 6, 8, filters=(4, 1, 3, 0, 2)) for p in px]


def room():
    """(meshes, materials, image arrays, PNG bytes).  Five walls of a unit room and a quad inside it.  Materials:
    0 base (image 0) + MR (image 1) + normal (image 2, scale 0.75), on the back wall, which has authored TANGENTs
         and sits under a mirroring node matrix;
    1 base only (image 3), no TANGENT: floor and ceiling;
    2 untextured with factors: the left wall;
    3 base = image 1, the image material 0 uses as its MR texture: the right wall; the quad has no material."""
    h = 1.0
    walls = [quad([-h, -h, -h], [2 * h, 0, 0], [0, 2 * h, 0], [0, 0, 1], 2.0),   # back
             quad([-h, -h, h], [2 * h, 0, 0], [0, 0, -2 * h], [0, 1, 0], 1.5),   # floor
             quad([-h, h, -h], [2 * h, 0, 0], [0, 0, 2 * h], [0, -1, 0], 1.5),   # ceiling
             quad([-h, -h, h], [0, 0, -2 * h], [0, 2 * h, 0], [1, 0, 0], 1.0),   # left
             quad([h, -h, -h], [0, 0, 2 * h], [0, 2 * h, 0], [-1, 0, 0], 3.0),   # right
             quad([-0.4, -0.2, 0.1], [0.8, 0, 0.1], [0, 0.7, 0.2], [0, -0.2747211, 0.9615239], 1.0)]
    rng = np.random.default_rng(5)
    t = rng.normal(size=(4, 3))
    t[:, 2] = 0  # in the back wall's plane
    t /= np.linalg.norm(t, axis=1)[:, None]
    walls[0]["tan"] = np.concatenate([t, np.array([[1], [-1], [1], [-1]])], 1).astype(F)
    walls[0]["matrix"] = MIRROR
    walls[0]["idx"] = np.array([0, 2, 1, 0, 3, 2], np.uint32)  # (the mirror flips the winding: authored reversed, it faces the room)
    for w, m in zip(walls, (0, 1, 1, 2, 3, None)):
        w["material"] = m
    mats = [{"name": "all", "pbrMetallicRoughness": {"baseColorFactor": [0.9, 0.8, 0.7, 1.0], "roughnessFactor": 0.6, "metallicFactor": 0.5,
                                                     "baseColorTexture": {"index": 0}, "metallicRoughnessTexture": {"index": 1}},
             "normalTexture": {"index": 2, "scale": 0.75}},
            {"name": "base", "pbrMetallicRoughness": {"baseColorTexture": {"index": 3}, "metallicFactor": 0.0}},
            {"name": "plain", "pbrMetallicRoughness": {"baseColorFactor": [0.2, 0.5, 0.9, 1.0], "roughnessFactor": 0.3}},
            {"name": "shared", "pbrMetallicRoughness": {"baseColorTexture": {"index": 1}, "roughnessFactor": 0.8, "metallicFactor": 0.25}}]
    px, png = images()
    return walls, mats, px, png
