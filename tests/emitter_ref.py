"""Reference for emitter sampling: the wavefront loop of tests/emission_ref.py
over the oracle's own stages, plus

  * the emitter table in numpy (weights in float32 by the sampling arithmetic's own expressions, the
    running sum in float64 in scene-id order),
  * one emitter sample per material evaluation in numpy float32, with the oracle's own or_rand,
    or_upper_bound and or_brdf_eval (ctypes) and or_trace_closest's t < tmax as the shadow result,
  * the logic pass's film line with the emitter term: or_stage_logic adds (acc * beta) to the film
    itself and has no third term, so for the paths that take the MIS sum (alive, 1 < len <= max_depth)
    the film is formed here as logic_core forms it (mis_accumulate's order, then + nee2 where the
    emitter ray was unoccluded, then acc * beta, then the add), from the same inputs.

With sample=False the loop is emission_ref.render, bit for bit (mirror=True: with the film line
formed here all the same, which checks the restatement against the oracle's own).
"""
import ctypes as C

import numpy as np

from emission_ref import HASVIS, MATS_LIT, black, emission_line, table  # noqa: F401  (re-exported)

SL_EMIT_PICK, SL_EMIT_U, SL_EMIT_V = 4096, 4097, 4098
F_DEAD, F_CONDL, F_CONDB = np.uint32(1), np.uint32(1 << 9), np.uint32(1 << 10)
f32 = np.float32
_f = C.POINTER(C.c_float)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def luminance(c):
    """mcpt_core.hpp luminance: the weighted sum in float64, rounded once."""
    c = np.asarray(c, np.float32).astype(np.float64)
    return (0.299 * c[..., 0] + 0.587 * c[..., 1] + 0.114 * c[..., 2]).astype(np.float32)


def weights(arrays, emission):
    """area * luminance(Le[mat]) per triangle of the scene's arrays (their order), float32; 0 where the
    material does not emit."""
    v0, v1, v2 = (np.asarray(arrays[k], np.float32).reshape(-1, 3) for k in ("v0", "v1", "v2"))
    E = np.asarray(emission, np.float32)[np.asarray(arrays["mat"], np.int32)]
    c = _cross(v1 - v0, v2 - v0)
    with np.errstate(all="ignore"):
        area = f32(0.5) * np.sqrt(_dot(c, c))
        w = area * luminance(E)
    return np.where((E != 0).any(axis=1), w, f32(0)).astype(np.float32)


def build_table(w, ids):
    """The emitter table from per-triangle weights and scene ids, in any order: dict of cdf, pick
    (float32), id (uint32, ascending), pos (index into w / ids) and total (float64)."""
    w = np.asarray(w, np.float32)
    ids = np.asarray(ids).astype(np.uint32)
    keep = np.flatnonzero((w > 0) & np.isfinite(w))
    keep = keep[np.argsort(ids[keep], kind="stable")]
    if not len(keep):
        z = np.zeros(0, np.float32)
        return {"cdf": z, "pick": z.copy(), "id": np.zeros(0, np.uint32), "pos": keep, "total": 0.0}
    prefix = np.cumsum(w[keep].astype(np.float64))  # serial, in id order
    total = prefix[-1]
    cdf = (prefix / total).astype(np.float32)
    cdf[-1] = f32(1)
    pick = cdf.copy()
    pick[1:] = cdf[1:] - cdf[:-1]
    return {"cdf": cdf, "pick": pick, "id": ids[keep], "pos": keep, "total": float(total)}


def scene_table(arrays, emission):
    ids = arrays["tri_id"] if "tri_id" in arrays and len(arrays["tri_id"]) else np.arange(len(arrays["mat"]))
    return build_table(weights(arrays, emission), ids)


def emitter_sample(oracle, arrays, tab, emission, pix, sidx, ln, so, n, wo, hit_mat, seed):
    """One emitter sample per row: (cE[k, 3], valid[k], ldir[k, 3], tmax[k]) in float32."""
    L = oracle.lib()
    k = len(pix)
    Ne = len(tab["cdf"])
    cdf = np.ascontiguousarray(tab["cdf"], np.float32)
    cp = cdf.ctypes.data_as(_f)
    pick_i = np.zeros(k, np.int64)
    u1, u2 = np.zeros(k, np.float32), np.zeros(k, np.float32)
    for j in range(k):
        a = (int(seed), int(pix[j]), int(sidx[j]), int(ln[j]))
        pick_i[j] = min(L.or_upper_bound(cp, Ne, L.or_rand(*a, SL_EMIT_PICK)), Ne - 1)
        u1[j] = L.or_rand(*a, SL_EMIT_U)
        u2[j] = L.or_rand(*a, SL_EMIT_V)
    pos = tab["pos"][pick_i]
    v0, v1, v2 = (np.asarray(arrays[q], np.float32).reshape(-1, 3)[pos] for q in ("v0", "v1", "v2"))
    e1, e2 = v1 - v0, v2 - v0  # the record's edges as stored
    with np.errstate(all="ignore"):
        su = np.sqrt(u1)
        p = (v0 + e1 * (su * (f32(1) - u2))[:, None]) + e2 * (su * u2)[:, None]
        dv = p - so
        d2 = _dot(dv, dv)
        dist = np.sqrt(d2)
        ldir = dv / dist[:, None]
        c = _cross(e1, e2)
        lc = np.sqrt(_dot(c, c))
        area = f32(0.5) * lc
        nc = np.where((lc == 0)[:, None], c, c / lc[:, None])
        cosl = np.abs(_dot(nc, ldir))
        pdf = ((tab["pick"][pick_i] / area) * d2) / cosl
        params = np.ascontiguousarray(np.asarray(arrays["mat_params"], np.float32).reshape(-1, 8)[hit_mat])
        f = np.zeros((k, 3), np.float32)
        out = np.zeros(8, np.float32)
        nn, ww, ll = (np.ascontiguousarray(x, np.float32) for x in (n, wo, ldir))
        for j in range(k):
            L.or_brdf_eval(params[j].ctypes.data_as(_f), nn[j].ctypes.data_as(_f), ll[j].ctypes.data_as(_f),
                           ww[j].ctypes.data_as(_f), out.ctypes.data_as(_f))
            f[j] = out[0:3] + out[3:6]
        Le = np.asarray(emission, np.float32)[np.asarray(arrays["mat"], np.int32)[pos]]
        cE = (f * Le) / pdf[:, None]
        valid = (dist > 0) & (cosl > 0) & (pdf > 0) & (pdf < np.inf) & np.isfinite(cE).all(axis=1)
        tmax = dist * f32(0.999)
    cE = np.where(valid[:, None], cE, f32(0)).astype(np.float32)
    return cE, valid, ldir.astype(np.float32), tmax.astype(np.float32)


def film_line(Ld, take, B, fl, n0, n1, vis, n2=None, ve=None):
    """logic_core's film update for the paths `take`: acc (mis_accumulate's order, then the emitter term),
    acc * beta, film + that.  Float32 throughout."""
    acc = np.zeros((len(fl), 3), np.float32)
    mL = ((fl & F_CONDL) != 0) & (vis[:, 0] != 0)
    acc = np.where(mL[:, None], acc + n0[:, :3], acc)
    mB = ((fl & HASVIS) != 0) & (vis[:, 1] != 0) & ((fl & F_CONDB) != 0)
    acc = np.where(mB[:, None], acc + n1[:, :3], acc)
    if n2 is not None:
        acc = np.where((ve != 0)[:, None], acc + n2[:, :3], acc)
    with np.errstate(all="ignore"):
        add = acc * B
        return np.where(take[:, None], Ld + add, Ld).astype(np.float32)


def render(oracle, arrays, cam, W, H, spp, max_depth=5, rr_depth=3, seed=0x5EED2026, fixed=False, emission=None,
           sample=False, mirror=False):
    """(Ld[H, W, 3], samples[H, W], counters).  sample: emitter sampling on (active only with a non-empty
    table, as on the device); counters["emitter_rays"]: valid emitter samples."""
    n = W * H
    kw = dict(max_depth=max_depth, rr_depth=rr_depth, seed=seed, fixed=fixed)
    mat = np.asarray(arrays["mat"], np.int32)
    inv = np.argsort(arrays["tri_id"])  # scene triangle id -> position in the scene's triangle arrays
    tab = scene_table(arrays, emission) if (sample and emission is not None) else None
    active = tab is not None and len(tab["cdf"]) > 0
    own_film = active or mirror
    yy, xx = np.divmod(np.arange(n), W)
    rendered = (xx < W - 1) & (yy < H - 1)
    st = {"flags": np.ones(n, np.uint32), "samples": np.zeros(n, np.uint32), "hit_tri": np.full(n, -1, np.int32),
          "ray_o": np.zeros((n, 3), np.float32), "ray_d": np.zeros((n, 3), np.float32),
          "beta": np.zeros((n, 4), np.float32), "nee0": np.zeros((n, 4), np.float32),
          "nee1": np.zeros((n, 4), np.float32), "vis": np.zeros((n, 2), np.uint8), "Ld": np.zeros((n, 3), np.float32)}
    nee2, ve = np.zeros((n, 4), np.float32), np.zeros(n, np.uint8)
    nrm = np.zeros((n, 3), np.float32)
    cnt = {"extend_rays": 0, "shadow_rays": 0, "vis_rays": 0, "iterations": 0, "emitter_rays": 0}
    while True:
        fl_in = st["flags"].copy()
        len_in = (fl_in >> np.uint32(1)) & np.uint32(0xFF)
        if own_film:
            alive = rendered & ((fl_in & F_DEAD) == 0) & ((fl_in >> np.uint32(13)) < np.uint32(spp))
            take = alive & (len_in > 1) & (len_in <= max_depth)
            Ld_mis = film_line(st["Ld"], take, st["beta"][:, :3], fl_in, st["nee0"], st["nee1"], st["vis"],
                               nee2 if active else None, ve if active else None)
        out = oracle.stage_logic(arrays, cam, W, H, st, spp, **kw)
        cont, gen = (out["queued"] & 2) != 0, (out["queued"] & 1) != 0
        for k in ("flags", "samples", "ray_o", "ray_d", "beta", "Ld"):
            st[k] = out[k]
        if own_film:
            st["Ld"] = np.where(take[:, None], Ld_mis, st["Ld"])  # (a len > 1 path has no other film term)
        if emission is not None:
            emission_line(st["Ld"], cont & (len_in == 1) if active else cont, st["hit_tri"], st["beta"], mat, emission)
        if not cont.any() and not gen.any():
            break
        cnt["iterations"] += 1
        if cont.any():
            ms = dict(st)
            ms["hit_tri"] = np.where(cont, st["hit_tri"], 0).astype(np.int32)
            wo = -st["ray_d"]  # the direction the path arrived by (before the material stage replaces it)
            m = oracle.stage_material(arrays, ms, **kw)
            for k in ("flags", "ray_o", "ray_d", "beta", "nee0", "nee1"):
                st[k][cont] = m[k][cont]
            st["vis"][cont, 0] = oracle.trace_any(arrays, m["light_o"][cont], m["light_d"][cont])
            has = cont & ((m["flags"] & HASVIS) != 0)
            st["vis"][cont, 1] = 0
            st["vis"][has, 1] = oracle.trace_any(arrays, m["bvis_o"][has], m["bvis_d"][has])
            cnt["shadow_rays"] += int(cont.sum())
            cnt["vis_rays"] += int(has.sum())
            if active:
                ci = np.flatnonzero(cont)
                cE, valid, ldir, tmax = emitter_sample(oracle, arrays, tab, emission, ci, fl_in[ci] >> np.uint32(13), len_in[ci],
                                                       m["light_o"][ci], nrm[ci], wo[ci], mat[st["hit_tri"][ci]], seed)
                nee2[ci, :3] = cE
                ve[ci] = 0
                vi = ci[valid]
                if len(vi):
                    pos_t, _, tri = oracle.trace_closest(arrays, m["light_o"][vi], ldir[valid])
                    ve[vi] = ~((tri >= 0) & (pos_t[:, 3] < tmax[valid]))
                cnt["emitter_rays"] += int(valid.sum())
        ext = cont | gen
        _, nm, tri = oracle.trace_closest(arrays, st["ray_o"][ext], st["ray_d"][ext])
        st["hit_tri"][ext] = np.where(tri >= 0, inv[np.maximum(tri, 0)], -1).astype(np.int32)
        nrm[ext] = nm[:, :3]
        cnt["extend_rays"] += int(ext.sum())
    return st["Ld"].reshape(H, W, 3), st["samples"].reshape(H, W), cnt
