// temporal.hpp -- arithmetic of the temporal stage of the preview denoiser:
// reprojection of the previous accumulated frame onto the current one and their blend, SVGF's temporal
// half (Schied et al., "Spatiotemporal Variance-Guided Filtering", HPG 2017, sections 4.1 and 4.2)
// with the history length counted in samples.
//
// __host__ __device__ in the style of denoise.hpp: add / mul / IEEE div / correctly rounded sqrt /
// comparisons only, one rounding per operation under the project's flags, no libm, float -> int by
// truncation plus a compare.  The host build and the gfx950 kernel (temporal.hip) agree bit for bit;
// tests/temporal_ref.py restates every expression below in numpy float32, in the same order.
//
// History planes (float4 per pixel), written by one call and gathered by the next:
//   hcol  (r, g, b, N)      accumulated colour; N: accumulated sample count, 0 = no history
//   hpos  (X.x, X.y, X.z, v)  world position of the first hit; v: variance of the mean luminance, -1 unknown
//   hnrm  (n.x, n.y, n.z, z)  mean guide normal and depth; z = 0: the pixel was not reprojectable and
//                             no later tap accepts it
// Output planes for the spatial passes: colour (r, g, b, valid) and vl (dn_vl), as denoise.hpp's.
#pragma once
#include "denoise.hpp"

namespace mcpt {

constexpr float TP_FLT_MAX = 3.402823466e+38f;

struct TemporalParams {
    float pos_tol;      // a tap is consistent if |X_q - X| <= pos_tol * z
    float nrm_tol;      // ... and |n_q - n| <= nrm_tol
    float max_history;  // the history's sample count is clamped to this before the blend
    float alpha_min;    // lower bound of the current frame's weight
};

// World position of a pixel's first hit from its pinhole ray (o, d) and its mean guide depth z.  With
// a lens the guide rays start on the lens and aim at pFocal, so their mean is the centre-of-lens ray:
// eye = iv (0, 0, 0, 1) / w, X = eye + z normalize(pFocal - eye).
MCPT_HD V3 tp_eye(const CamView& c) {
    float e[4];
    mat_vec4(c.iv, 0.f, 0.f, 0.f, 1.f, e);
    return v3(e[0], e[1], e[2]) / e[3];
}
MCPT_HD V3 tp_world_focal(const CamView& c, V3 pFocal, float z) {
    const V3 eye = tp_eye(c);
    return eye + normalize(pFocal - eye) * z;
}
MCPT_HD V3 tp_world(const CamView& c, V3 o, V3 d, float z) {
    if (c.lens_radius > 0.f) return tp_world_focal(c, gen_ray_focal(c, o, d), z);
    return o + d * z;
}

// The current frame's pixel.  col: dn_planes' colour entry; s: its sample count; vc: the variance of
// its mean luminance or -1; reproj: it has a first hit to reproject (a valid colour and a depth that is
// a finite number > 0: a miss, and a pixel without guide samples, whose means are 0 / 0, have none).
// X, n, z are zero where !reproj.
struct TpPixel {
    float4 col;
    float s, vc;
    V3 X, n;
    float z;
    bool reproj;
};
MCPT_HD bool tp_known(float v) { return v >= 0.f && v <= TP_FLT_MAX; }
MCPT_HD TpPixel tp_pixel(float r, float g, float b, bool has_samples, float s, float var, V3 X, V3 n, float z) {
    TpPixel p;
    const bool valid = has_samples && dn_finite(r) && dn_finite(g) && dn_finite(b);
    p.col = valid ? make_float4(r, g, b, 1.f) : make_float4(0.f, 0.f, 0.f, 0.f);
    p.s = valid ? s : 0.f;
    p.vc = (valid && tp_known(var)) ? var : -1.f;
    p.reproj = valid && z > 0.f && z <= TP_FLT_MAX;
    p.X = p.reproj ? X : v3(0.f, 0.f, 0.f);
    p.n = p.reproj ? n : v3(0.f, 0.f, 0.f);
    p.z = p.reproj ? z : 0.f;
    return p;
}

// Projection into the previous frame: clip = VP_prev (X, 1); pixel coordinates of the pixel centres'
// grid; (x0, y0) = floor, (tx, ty) = the fractions.  ok = false: behind the previous camera, outside
// -1 < fx < W, -1 < fy < H (no corner of the tap would lie inside the film), or not a number.
struct TpProj {
    bool ok;
    int x0, y0;
    float tx, ty;
};
MCPT_HD int tp_floor(float f) {  // |f| < 2^31
    const int i = (int)f;
    return (float)i > f ? i - 1 : i;
}
MCPT_HD TpProj tp_project(const float* vp, const TpPixel& p, int W, int H) {
    float c[4];
    mat_vec4(vp, p.X.x, p.X.y, p.X.z, 1.f, c);
    const float Wf = (float)W, Hf = (float)H;
    const float fx = ((c[0] / c[3] + 1.f) * 0.5f) * Wf - 0.5f;
    const float fy = ((1.f - c[1] / c[3]) * 0.5f) * Hf - 0.5f;
    TpProj q;
    q.ok = p.reproj && c[3] > 0.f && fx > -1.f && fx < Wf && fy > -1.f && fy < Hf;
    const float sx = q.ok ? fx : 0.f, sy = q.ok ? fy : 0.f;
    q.x0 = tp_floor(sx);
    q.y0 = tp_floor(sy);
    q.tx = sx - (float)q.x0;
    q.ty = sy - (float)q.y0;
    return q;
}
// Corner k = 0 .. 3 of the bilinear tap, row-major: its offset and its weight
MCPT_HD int tp_corner_dx(int k) { return k & 1; }
MCPT_HD int tp_corner_dy(int k) { return k >> 1; }
MCPT_HD float tp_corner_w(const TpProj& q, int k) {
    const float wx = (k & 1) ? q.tx : 1.f - q.tx, wy = (k >> 1) ? q.ty : 1.f - q.ty;
    return wx * wy;
}

// The accepted corners' sums.  A corner is accepted if it lies inside the film (`in`), holds a history
// (a sample count that is a finite number > 0, a finite colour, a depth > 0) and is consistent with the
// pixel in position and normal.  Its values are selected, not branched on: a rejected corner adds
// zeros, so what it holds never reaches the sums.
struct TpAcc {
    float w, r, g, b, n, v;
    bool vknown;  // every accepted corner's variance is known
};
MCPT_HD void tp_tap(const TemporalParams& k, const TpPixel& p, float w, bool in, const float4& hc, const float4& hp,
                    const float4& hn, TpAcc& a) {
    const float tol = k.pos_tol * p.z;
    const bool acc = in && hc.w > 0.f && hc.w <= TP_FLT_MAX && dn_finite(hc.x) && dn_finite(hc.y) && dn_finite(hc.z) &&
                     hn.w > 0.f && dn_sq3(hp.x, hp.y, hp.z, p.X.x, p.X.y, p.X.z) <= tol * tol &&
                     dn_sq3(hn.x, hn.y, hn.z, p.n.x, p.n.y, p.n.z) <= k.nrm_tol * k.nrm_tol;
    const bool vk = tp_known(hp.w);
    const float wa = acc ? w : 0.f;
    a.w = a.w + wa;
    a.r = a.r + wa * (acc ? hc.x : 0.f);
    a.g = a.g + wa * (acc ? hc.y : 0.f);
    a.b = a.b + wa * (acc ? hc.z : 0.f);
    a.n = a.n + wa * (acc ? hc.w : 0.f);
    a.v = a.v + wa * ((acc && vk) ? hp.w : 0.f);
    a.vknown = a.vknown && (!acc || vk);
}

// The blend and the five plane entries of the pixel.  The history is used if the projection is ok, the
// accepted weights sum to more than 0 and the blended colour is finite; else the pixel is a
// disocclusion and leaves as it came: c' = c, N' = s, v' = v_c.
struct TpOut {
    float4 col;
    float2 vl;
    float4 hcol, hpos, hnrm;
};
MCPT_HD TpOut tp_blend(const TemporalParams& k, const TpPixel& p, const TpProj& q, const TpAcc& a) {
    const float hr = a.r / a.w, hg = a.g / a.w, hb = a.b / a.w;
    const float nh = a.n / a.w, vh = a.v / a.w;
    const float nc = nh < k.max_history ? nh : k.max_history;
    const float al0 = p.s / (nc + p.s);
    const float al = al0 > k.alpha_min ? al0 : k.alpha_min;
    const float cr = hr + al * (p.col.x - hr), cg = hg + al * (p.col.y - hg), cb = hb + al * (p.col.z - hb);
    const float om = 1.f - al;
    const float vb = (om * om) * vh + (al * al) * p.vc;
    const bool use = q.ok && a.w > 0.f && dn_finite(cr) && dn_finite(cg) && dn_finite(cb);
    const bool valid = p.col.w != 0.f;
    const float vo = use ? ((a.vknown && tp_known(p.vc) && tp_known(vb)) ? vb : -1.f) : p.vc;
    TpOut o;
    o.col = use ? make_float4(cr, cg, cb, 1.f) : p.col;
    o.vl = dn_vl(o.col, vo);
    o.hcol = make_float4(o.col.x, o.col.y, o.col.z, use ? nc + p.s : p.s);
    o.hpos = make_float4(p.X.x, p.X.y, p.X.z, valid ? vo : -1.f);
    o.hnrm = make_float4(p.n.x, p.n.y, p.n.z, p.z);
    return o;
}

// Host form over W x H planes (the kernel's parity reference; tests/native/temporal_host.cpp): cur = the
// current frame's pixels, hcol / hpos / hnrm = the previous call's planes, vp = VP_prev (column-major)
inline void temporal_pass_host(const TemporalParams& k, int W, int H, const float* vp, const TpPixel* cur,
                               const float4* hcol, const float4* hpos, const float4* hnrm, float4* out_col, float2* out_vl,
                               float4* out_hcol, float4* out_hpos, float4* out_hnrm) {
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            const size_t i = (size_t)y * W + x;
            const TpPixel& p = cur[i];
            const TpProj q = tp_project(vp, p, W, H);
            TpAcc a{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, true};
            for (int c = 0; c < 4; c++) {
                const int qx = q.x0 + tp_corner_dx(c), qy = q.y0 + tp_corner_dy(c);
                const bool in = qx >= 0 && qx < W && qy >= 0 && qy < H;
                const size_t j = in ? (size_t)qy * W + (size_t)qx : i;
                tp_tap(k, p, tp_corner_w(q, c), in, hcol[j], hpos[j], hnrm[j], a);
            }
            const TpOut o = tp_blend(k, p, q, a);
            out_col[i] = o.col;
            out_vl[i] = o.vl;
            out_hcol[i] = o.hcol;
            out_hpos[i] = o.hpos;
            out_hnrm[i] = o.hnrm;
        }
}

// VP = inverse(inv_view_proj), column-major like its input: cofactors in double, rounded once
inline void tp_view_proj(const float* ivp, float* out16) {
    double m[16], inv[16];
    for (int i = 0; i < 16; i++) m[i] = (double)ivp[i];
    inv[0] = m[5] * m[10] * m[15] - m[5] * m[11] * m[14] - m[9] * m[6] * m[15] + m[9] * m[7] * m[14] + m[13] * m[6] * m[11] - m[13] * m[7] * m[10];
    inv[4] = -m[4] * m[10] * m[15] + m[4] * m[11] * m[14] + m[8] * m[6] * m[15] - m[8] * m[7] * m[14] - m[12] * m[6] * m[11] + m[12] * m[7] * m[10];
    inv[8] = m[4] * m[9] * m[15] - m[4] * m[11] * m[13] - m[8] * m[5] * m[15] + m[8] * m[7] * m[13] + m[12] * m[5] * m[11] - m[12] * m[7] * m[9];
    inv[12] = -m[4] * m[9] * m[14] + m[4] * m[10] * m[13] + m[8] * m[5] * m[14] - m[8] * m[6] * m[13] - m[12] * m[5] * m[10] + m[12] * m[6] * m[9];
    inv[1] = -m[1] * m[10] * m[15] + m[1] * m[11] * m[14] + m[9] * m[2] * m[15] - m[9] * m[3] * m[14] - m[13] * m[2] * m[11] + m[13] * m[3] * m[10];
    inv[5] = m[0] * m[10] * m[15] - m[0] * m[11] * m[14] - m[8] * m[2] * m[15] + m[8] * m[3] * m[14] + m[12] * m[2] * m[11] - m[12] * m[3] * m[10];
    inv[9] = -m[0] * m[9] * m[15] + m[0] * m[11] * m[13] + m[8] * m[1] * m[15] - m[8] * m[3] * m[13] - m[12] * m[1] * m[11] + m[12] * m[3] * m[9];
    inv[13] = m[0] * m[9] * m[14] - m[0] * m[10] * m[13] - m[8] * m[1] * m[14] + m[8] * m[2] * m[13] + m[12] * m[1] * m[10] - m[12] * m[2] * m[9];
    inv[2] = m[1] * m[6] * m[15] - m[1] * m[7] * m[14] - m[5] * m[2] * m[15] + m[5] * m[3] * m[14] + m[13] * m[2] * m[7] - m[13] * m[3] * m[6];
    inv[6] = -m[0] * m[6] * m[15] + m[0] * m[7] * m[14] + m[4] * m[2] * m[15] - m[4] * m[3] * m[14] - m[12] * m[2] * m[7] + m[12] * m[3] * m[6];
    inv[10] = m[0] * m[5] * m[15] - m[0] * m[7] * m[13] - m[4] * m[1] * m[15] + m[4] * m[3] * m[13] + m[12] * m[1] * m[7] - m[12] * m[3] * m[5];
    inv[14] = -m[0] * m[5] * m[14] + m[0] * m[6] * m[13] + m[4] * m[1] * m[14] - m[4] * m[2] * m[13] - m[12] * m[1] * m[6] + m[12] * m[2] * m[5];
    inv[3] = -m[1] * m[6] * m[11] + m[1] * m[7] * m[10] + m[5] * m[2] * m[11] - m[5] * m[3] * m[10] - m[9] * m[2] * m[7] + m[9] * m[3] * m[6];
    inv[7] = m[0] * m[6] * m[11] - m[0] * m[7] * m[10] - m[4] * m[2] * m[11] + m[4] * m[3] * m[10] + m[8] * m[2] * m[7] - m[8] * m[3] * m[6];
    inv[11] = -m[0] * m[5] * m[11] + m[0] * m[7] * m[9] + m[4] * m[1] * m[11] - m[4] * m[3] * m[9] - m[8] * m[1] * m[7] + m[8] * m[3] * m[5];
    inv[15] = m[0] * m[5] * m[10] - m[0] * m[6] * m[9] - m[4] * m[1] * m[10] + m[4] * m[2] * m[9] + m[8] * m[1] * m[6] - m[8] * m[2] * m[5];
    const double det = m[0] * inv[0] + m[1] * inv[4] + m[2] * inv[8] + m[3] * inv[12];
    for (int i = 0; i < 16; i++) out16[i] = (float)(inv[i] / det);
}

}  // namespace mcpt
