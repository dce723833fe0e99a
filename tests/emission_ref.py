"""Reference for emissive materials: the wavefront loop over the oracle's own
stages (or_stage_logic, or_stage_material, or_trace_any, or_trace_closest), with the one line the
oracle lacks: a path the logic stage lets continue into the material stage collects the emission of
the surface it hit, weighted by the throughput the logic stage stores for it,

    Ld[cont] += E[mat[hit_tri[cont]]] * beta_out[cont, :3]          (float32)

With emission=None the loop is oracle.render, bit for bit (tests/test_emission_host.py)."""
import numpy as np

MATS_LIT = (2, 7)  # config 2's proxy: the ceiling and one of the spheres
HASVIS = np.uint32(1 << 12)  # mcpt_path_view flags: a BRDF visibility ray was made (non-delta light)


def table(nmat, entries):
    """(nmat, 3) float32 table from {material id: rgb}."""
    e = np.zeros((nmat, 3), np.float32)
    for m, rgb in entries.items():
        e[m] = rgb
    return e


def black(arrays):
    """The scene's arrays under a black Color environment (every radiance then comes from emission)."""
    a = dict(arrays)
    a["env_mode"] = 0
    a["env_color"] = np.zeros(3, np.float32)
    a["env_ls"] = np.float32(1.0)
    return a


def emission_line(Ld, cont, hit_tri, beta_out, mat, emission):
    """The numpy line: Ld of the continuing paths += E[mat[hit_tri]] * beta_out[:, :3], in float32."""
    E = np.asarray(emission, np.float32)
    Ld[cont] = Ld[cont] + E[mat[hit_tri[cont]]] * beta_out[cont, :3]
    return Ld


def render(oracle, arrays, cam, W, H, spp, max_depth=5, rr_depth=3, seed=0x5EED2026, fixed=False, emission=None):
    """Returns (Ld[H, W, 3], samples[H, W], counters) like oracle.render, plus per-material emission."""
    n = W * H
    kw = dict(max_depth=max_depth, rr_depth=rr_depth, seed=seed, fixed=fixed)
    mat = np.asarray(arrays["mat"], np.int32)
    inv = np.argsort(arrays["tri_id"])  # scene triangle id -> position in the scene's triangle arrays
    st = {"flags": np.ones(n, np.uint32), "samples": np.zeros(n, np.uint32), "hit_tri": np.full(n, -1, np.int32),
          "ray_o": np.zeros((n, 3), np.float32), "ray_d": np.zeros((n, 3), np.float32),
          "beta": np.zeros((n, 4), np.float32), "nee0": np.zeros((n, 4), np.float32),
          "nee1": np.zeros((n, 4), np.float32), "vis": np.zeros((n, 2), np.uint8), "Ld": np.zeros((n, 3), np.float32)}
    cnt = {"extend_rays": 0, "shadow_rays": 0, "vis_rays": 0, "iterations": 0}
    while True:
        out = oracle.stage_logic(arrays, cam, W, H, st, spp, **kw)
        cont, gen = (out["queued"] & 2) != 0, (out["queued"] & 1) != 0
        for k in ("flags", "samples", "ray_o", "ray_d", "beta", "Ld"):
            st[k] = out[k]
        if emission is not None:
            emission_line(st["Ld"], cont, st["hit_tri"], st["beta"], mat, emission)
        if not cont.any() and not gen.any():
            break
        cnt["iterations"] += 1
        if cont.any():
            # or_stage_material keys its draws by the array index as the pixel: the whole film goes in,
            # non-continuing paths with a dummy triangle, and only the continuing rows come back
            ms = dict(st)
            ms["hit_tri"] = np.where(cont, st["hit_tri"], 0).astype(np.int32)
            m = oracle.stage_material(arrays, ms, **kw)
            for k in ("flags", "ray_o", "ray_d", "beta", "nee0", "nee1"):
                st[k][cont] = m[k][cont]
            st["vis"][cont, 0] = oracle.trace_any(arrays, m["light_o"][cont], m["light_d"][cont])
            # A delta light has no BRDF visibility ray (or_stage_material writes NaN for it): the flags'
            # has-visibility bit says so.  (The ray's own direction can be NaN too, from the reference's
            # NaN frame at an axis-aligned normal, and is then still a ray that is traced and counted.)
            has = cont & ((m["flags"] & HASVIS) != 0)
            st["vis"][cont, 1] = 0
            st["vis"][has, 1] = oracle.trace_any(arrays, m["bvis_o"][has], m["bvis_d"][has])
            cnt["shadow_rays"] += int(cont.sum())
            cnt["vis_rays"] += int(has.sum())
        ext = cont | gen
        _, _, tri = oracle.trace_closest(arrays, st["ray_o"][ext], st["ray_d"][ext])
        st["hit_tri"][ext] = np.where(tri >= 0, inv[np.maximum(tri, 0)], -1).astype(np.int32)
        cnt["extend_rays"] += int(ext.sum())
    return st["Ld"].reshape(H, W, 3), st["samples"].reshape(H, W), cnt
