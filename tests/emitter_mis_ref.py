"""Reference for MIS between emitter samples and collected emission: the loop of
tests/emitter_ref.py's render with a `mis` argument, in numpy float32 over the oracle's own stages.

With mis=True (and sampling active)
  * the emitter sample carries its weight: wE = power_heuristic(pdf_e, pdf_be), cE = ((f Le) wE) / pdf_e,
    pdf_be the BRDF's pdf of the sampled direction ((out[7] + out[6]) * 0.5f of or_brdf_eval),
  * pdf_s, the same pdf for the continuation direction the material stage stored, rides in nee2.w,
  * a continuing path collects at every length again; at len >= 2, where the surface emits, with
    wC = power_heuristic(pdf_s, pdf_c), pdf_c the emitter sample's solid-angle pdf for the point hit, from
    the continuation ray as stored and the hit triangle's v0, e1, e2 (collect_weight),
  * pick_rec: the table's pick by position in the scene's triangle arrays, 0 elsewhere.

With mis=False the loop is emitter_ref.render, bit for bit (tests/test_emitter_mis_host.py)."""
import ctypes as C

import numpy as np

import emitter_ref as MR
from emitter_ref import (HASVIS, SL_EMIT_PICK, SL_EMIT_U, SL_EMIT_V, F_DEAD, _cross, _dot, _f, f32, film_line,  # noqa: F401
                         scene_table)


def power_heuristic(f, g):
    """mcpt_core.hpp power_heuristic in float32: (f f) / (f f + g g)."""
    f, g = np.asarray(f, np.float32), np.asarray(g, np.float32)
    with np.errstate(all="ignore"):
        return ((f * f) / (f * f + g * g)).astype(np.float32)


def brdf_pdf(oracle, params, n, wi, wo):
    """brdf_f_pdf's pdf per row: (diff_get_pdf + spec_get_pdf) * 0.5f from or_brdf_eval; also f (fs + fd)."""
    L = oracle.lib()
    k = len(params)
    out = np.zeros(8, np.float32)
    pdf, f = np.zeros(k, np.float32), np.zeros((k, 3), np.float32)
    pp, nn, ii, oo = (np.ascontiguousarray(x, np.float32) for x in (params, n, wi, wo))
    for j in range(k):
        L.or_brdf_eval(pp[j].ctypes.data_as(_f), nn[j].ctypes.data_as(_f), ii[j].ctypes.data_as(_f),
                       oo[j].ctypes.data_as(_f), out.ctypes.data_as(_f))
        f[j] = out[0:3] + out[3:6]
        pdf[j] = (out[7] + out[6]) * f32(0.5)
    return f, pdf


def pick_by_record(tab, ntri):
    """pick_rec: the table's pick at the entries' positions in the scene's triangle arrays, 0 elsewhere."""
    p = np.zeros(ntri, np.float32)
    p[tab["pos"]] = tab["pick"]
    return p


def area_pdf(pick, v0, e1, e2, o, d):
    """The emitter sample's solid-angle pdf for the point where the ray (o, d) meets the triangle's plane,
    and cosl: k_shade's expressions."""
    with np.errstate(all="ignore"):
        c = _cross(e1, e2)
        lc = np.sqrt(_dot(c, c))
        area = f32(0.5) * lc
        t = _dot(v0 - o, c) / _dot(d, c)
        d2 = t * t
        nc = np.where((lc == 0)[:, None], c, c / lc[:, None])
        cosl = np.abs(_dot(nc, d))
        return (((pick / area) * d2) / cosl).astype(np.float32), cosl.astype(np.float32)


def collect_weight(pdf_s, pick, v0, e1, e2, o, d):
    """wC per row: power_heuristic(pdf_s, pdf_c); 1 where pdf_c is not a finite number > 0 or the weight
    is not in [0, 1]."""
    pdf_c, _ = area_pdf(pick, v0, e1, e2, o, d)
    w = power_heuristic(pdf_s, pdf_c)
    with np.errstate(all="ignore"):
        bad = ~((pdf_c > 0) & (pdf_c < np.inf)) | ~((w >= 0) & (w <= 1))
    return np.where(bad, f32(1), w).astype(np.float32)


def emitter_sample(oracle, arrays, tab, emission, pix, sidx, ln, so, n, wo, hit_mat, seed, mis):
    """emitter_ref.emitter_sample with the weight folded in when mis: (cE, valid, ldir, tmax)."""
    if not mis:
        return MR.emitter_sample(oracle, arrays, tab, emission, pix, sidx, ln, so, n, wo, hit_mat, seed)
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
    e1, e2 = v1 - v0, v2 - v0
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
        params = np.asarray(arrays["mat_params"], np.float32).reshape(-1, 8)[hit_mat]
        f, pdf_be = brdf_pdf(oracle, params, n, ldir, wo)
        Le = np.asarray(emission, np.float32)[np.asarray(arrays["mat"], np.int32)[pos]]
        wE = power_heuristic(pdf, pdf_be)
        cE = ((f * Le) * wE[:, None]) / pdf[:, None]
        valid = (dist > 0) & (cosl > 0) & (pdf > 0) & (pdf < np.inf) & np.isfinite(cE).all(axis=1)
        tmax = dist * f32(0.999)
    cE = np.where(valid[:, None], cE, f32(0)).astype(np.float32)
    return cE, valid, ldir.astype(np.float32), tmax.astype(np.float32)


def collect(Ld, cont, len_in, hit_tri, beta_out, mat, emission, pick_rec, pdf_s, arrays, ray_o, ray_d):
    """The weighted collection of the continuing paths: where the surface emits,
    Ld += (Le * beta) * w, w = 1 at len 1 and collect_weight at len >= 2; elsewhere the film keeps its bits."""
    E = np.asarray(emission, np.float32)
    ci = np.flatnonzero(cont)
    ci = ci[(E[mat[hit_tri[ci]]] != 0).any(axis=1)]
    if not len(ci):
        return Ld
    pos = hit_tri[ci]
    v0, v1, v2 = (np.asarray(arrays[q], np.float32).reshape(-1, 3)[pos] for q in ("v0", "v1", "v2"))
    w = collect_weight(pdf_s[ci], pick_rec[pos], v0, v1 - v0, v2 - v0, ray_o[ci], ray_d[ci])
    w = np.where(len_in[ci] == 1, f32(1), w).astype(np.float32)
    with np.errstate(all="ignore"):
        Ld[ci] = Ld[ci] + (E[mat[pos]] * beta_out[ci, :3]) * w[:, None]
    return Ld


def render(oracle, arrays, cam, W, H, spp, max_depth=5, rr_depth=3, seed=0x5EED2026, fixed=False, emission=None,
           sample=False, mirror=False, mis=False):
    """emitter_ref.render with mis: (Ld[H, W, 3], samples[H, W], counters).  MIS is in effect only while
    sampling is active (a non-empty table), as on the device."""
    n = W * H
    kw = dict(max_depth=max_depth, rr_depth=rr_depth, seed=seed, fixed=fixed)
    mat = np.asarray(arrays["mat"], np.int32)
    inv = np.argsort(arrays["tri_id"])
    tab = scene_table(arrays, emission) if (sample and emission is not None) else None
    active = tab is not None and len(tab["cdf"]) > 0
    mis = bool(mis and active)
    pick_rec = pick_by_record(tab, len(mat)) if mis else None
    params_all = np.asarray(arrays["mat_params"], np.float32).reshape(-1, 8)
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
            st["Ld"] = np.where(take[:, None], Ld_mis, st["Ld"])
        if emission is not None:
            if mis:  # (a continuing path's ray_o / ray_d are still the ray that found the hit)
                collect(st["Ld"], cont, len_in, st["hit_tri"], st["beta"], mat, emission, pick_rec, nee2[:, 3], arrays,
                        st["ray_o"], st["ray_d"])
            else:
                MR.emission_line(st["Ld"], cont & (len_in == 1) if active else cont, st["hit_tri"], st["beta"], mat, emission)
        if not cont.any() and not gen.any():
            break
        cnt["iterations"] += 1
        if cont.any():
            ms = dict(st)
            ms["hit_tri"] = np.where(cont, st["hit_tri"], 0).astype(np.int32)
            wo = -st["ray_d"]
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
                hm = mat[st["hit_tri"][ci]]
                cE, valid, ldir, tmax = emitter_sample(oracle, arrays, tab, emission, ci, fl_in[ci] >> np.uint32(13), len_in[ci],
                                                       m["light_o"][ci], nrm[ci], wo[ci], hm, seed, mis)
                nee2[ci, :3] = cE
                if mis:  # pdf_s of the continuation direction the material stage stored
                    nee2[ci, 3] = brdf_pdf(oracle, params_all[hm], nrm[ci], m["ray_d"][ci], wo[ci])[1]
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
