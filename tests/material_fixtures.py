"""Glossy and metallic materials for the parity tests (DESIGN.md "Parity tests").

Every scene the loaders and proxies build carries one material point: fresnel 0.04, roughness 1,
metallic 0, where a2 - 1 == 0 and most of the GGX arithmetic is constant.  PALETTE spreads the
material space the ABI accepts over a scene's triangles, and grazing_state aims rays along the
surfaces so the n.wo clamps are exercised.  The roughnesses are non-dyadic on purpose: for 0.5,
0.25 and the like r*r, (r*r)*(r*r) and ((r*r)*r)*r are all exact, so two orders of the a2 product
round alike and a swapped order would go unnoticed."""
import numpy as np

import stage_fixtures as sf

ROUGHNESS = (1.0, 0.73, 0.37, 0.11, 0.01)
METALLIC = (0.0, 0.37, 1.0)
# rows: base rgb, fresnel rgb, roughness, metallic
PALETTE = np.array(
    [[0.8, 0.6, 0.2, 0.04, 0.04, 0.04, r, m] for r in ROUGHNESS for m in METALLIC] + [
        [0.0, 0.0, 0.0, 0.04, 0.5, 0.9, 0.3, 0.0],    # black base, coloured fresnel
        [0.9, 0.0, 0.4, 0.0, 0.0, 0.0, 0.3, 1.0],     # zero fresnel, full metal
        [0.5, 0.5, 0.5, 0.04, 0.04, 0.04, 0.0, 0.0],  # roughness 0: load_mat clamps to BRDF_EPS
        [0.5, 0.5, 0.5, 0.04, 0.04, 0.04, 1.5, 0.3],  # beyond the sliders: a2 - 1 > 0
    ], np.float32)
assert PALETTE.shape == (19, 8)


def with_palette(arrays):
    """A copy of a scene's arrays with PALETTE as its materials, triangle id t wearing row t % 19
    (by id, so the assignment does not depend on the BVH order)."""
    b = dict(arrays)
    b["mat_params"] = PALETTE.copy()
    b["mat"] = (np.asarray(arrays["tri_id"], np.int64) % len(PALETTE)).astype(np.int32)
    return b


def rows_hit(arrays, state):
    """Paths per palette row of a material-stage input on with_palette(arrays)."""
    return np.bincount(with_palette(arrays)["mat"][state["hit_tri"]], minlength=len(PALETTE))


def n_dot_wo(arrays, trace_closest, state):
    """Shading n . wo of every path of a material-stage input (the oracle's interpolated normal)."""
    _, nm, tri = trace_closest(arrays, state["ray_o"], state["ray_d"])
    assert np.all(tri >= 0)
    return -(nm[:, :3].astype(np.float64) * state["ray_d"].astype(np.float64)).sum(1)


def grazing_state(arrays, trace_closest, n, seed, cid=1):
    """Material-stage input (stage_fixtures.material_state's form) of rays that skim the surface:
    from a random point p of a random triangle, the direction d = normalize(-u - ng * delta) with u
    a unit vector in the triangle's plane, ng its geometric normal on the side of its first vertex
    normal and delta in U(0, 0.03); the ray starts 0.5 (config 1) or 0.05 (config 2) back along d.
    The candidates the oracle finds a hit for are kept (nearly all of n).  Where the interpolated
    normal leans away from the facet, n . wo falls below BRDF_EPS or below zero."""
    rng = np.random.default_rng(seed)
    a = arrays
    T = len(a["mat"])
    ti = rng.integers(0, T, n)
    v0, v1, v2 = (np.asarray(a[k], np.float64)[ti] for k in ("v0", "v1", "v2"))
    bary = rng.dirichlet((1.0, 1.0, 1.0), n)
    p = bary[:, :1] * v0 + bary[:, 1:2] * v1 + bary[:, 2:] * v2
    e1, e2 = v1 - v0, v2 - v0
    ng = np.cross(e1, e2)
    ng /= np.linalg.norm(ng, axis=1, keepdims=True)
    ng *= np.where((ng * np.asarray(a["n0"], np.float64)[ti]).sum(1) < 0, -1.0, 1.0)[:, None]
    t1 = e1 / np.linalg.norm(e1, axis=1, keepdims=True)
    t2 = np.cross(ng, t1)
    ang = rng.uniform(0.0, 2.0 * np.pi, (n, 1))
    u = np.cos(ang) * t1 + np.sin(ang) * t2
    d = -u - ng * rng.uniform(0.0, 0.03, (n, 1))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = p - d * (0.5 if cid == 1 else 0.05)
    ro, rd = o.astype(np.float32), d.astype(np.float32)
    _, _, tri = trace_closest(a, ro, rd)
    k = tri >= 0
    inv = np.argsort(a["tri_id"])  # scene triangle id -> array index
    ro, rd, hit = ro[k], rd[k], inv[tri[k]].astype(np.int32)
    m = len(hit)
    ln = rng.integers(1, sf.DEPTH + 1, m).astype(np.uint32)
    sidx = rng.integers(0, sf.SPP, m).astype(np.uint32)
    beta = np.zeros((m, 4), np.float32)
    beta[:, :3] = rng.uniform(0.05, 1.0, (m, 3))
    return {"flags": (ln << 1) | (sidx << 13), "hit_tri": hit, "ray_o": ro, "ray_d": rd, "beta": beta}
