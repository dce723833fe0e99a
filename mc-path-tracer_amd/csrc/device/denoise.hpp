// denoise.hpp -- arithmetic of the edge-avoiding a-trous wavelet filter (Dammertz, Sewtz, Hanika,
// Lensch: "Edge-Avoiding A-Trous Wavelet Transform for fast Global Illumination Filtering", HPG 2010)
// over the film and its first-hit guide buffers (albedo, normal, depth).
//
// __host__ __device__, add / mul / IEEE div only, one rounding per operation under the project's
// flags (-ffp-contract=off, correctly rounded division): the host build and the gfx950 kernels
// (denoise.hip) agree bit for bit, as with mcpt_core.hpp.  tests/denoise_ref.py restates every
// expression below in numpy float32, in the same order.
//
// Planes (float4 per pixel):
//   colour  (r, g, b, valid)   valid = 1: the pixel has samples and a finite colour; 0: skipped as a
//                              tap and written as (0, 0, 0, 0)
//   guide   (nx, ny, nz, z)    mean first-hit normal and depth
//   albedo  (r, g, b, rz)      mean first-hit albedo; rz = 1 / max(z * z, 1e-12)
#pragma once
#include "mcpt_core.hpp"

namespace mcpt {

// exp(-x) for x >= 0 without libm: k = nearest integer to x log2(e), r = x - k ln 2 in two exact
// steps (Cody-Waite: k <= 126 has 7 bits, LN2_HI 10, and x - k LN2_HI cancels exactly), f = r log2(e)
// in [-1/2, 1/2], 2^-f by the degree-7 Taylor polynomial of exp(-f ln 2) (remainder < 2^-27), and
// 2^-k built as an exponent field.  Exactly 1 at 0; 0 where the result would be subnormal (and for
// x > 87.5, a NaN included), so no subnormal is ever produced; a negative x saturates at 1.
constexpr float DN_LOG2E = 1.44269504088896341f;
constexpr float DN_LN2_HI = 0.693359375f;         // 355 / 512
constexpr float DN_LN2_LO = -2.12194440e-4f;      // ln 2 - LN2_HI
constexpr float DN_EXP_MAX = 87.5f;               // exp(-87.5) < 2^-126
constexpr float DN_FLT_MIN = 1.17549435e-38f;     // 2^-126
MCPT_HD float dexp_neg(float x) {
    if (!(x <= DN_EXP_MAX)) return 0.f;
    if (!(x > 0.f)) return 1.f;
    const int k = (int)(x * DN_LOG2E + 0.5f);     // truncation: the operand is positive
    const float kf = (float)k;
    float r = x - kf * DN_LN2_HI;
    r = r - kf * DN_LN2_LO;
    const float f = r * DN_LOG2E;
    float p = -1.52527338e-5f * f;                // (-ln 2)^n / n!, n = 7 .. 1
    p = p + 1.54035304e-4f;
    p = p * f;
    p = p + -1.33335581e-3f;
    p = p * f;
    p = p + 9.61812911e-3f;
    p = p * f;
    p = p + -5.55041087e-2f;
    p = p * f;
    p = p + 2.40226507e-1f;
    p = p * f;
    p = p + -6.93147181e-1f;
    p = p * f;
    p = p + 1.f;
    const float scale = __builtin_bit_cast(float, (uint32_t)(127 - k) << 23);  // 2^-k, k in 0..126
    const float e = p * scale;
    return e < DN_FLT_MIN ? 0.f : e;
}

// One pass: taps at stride 2^i, k = 1 / (sigma * sigma) per term (0: the term is off)
struct DenoisePass {
    float kc, kn, ka, kz;
    int stride;
};
MCPT_HD float dn_k(float sigma) { return sigma > 0.f ? 1.f / (sigma * sigma) : 0.f; }
// the B3 spline taps h = {1/16, 1/4, 3/8, 1/4, 1/16} (exact, and so are their products)
MCPT_HD float dn_h(int d) { return d == 0 ? 0.375f : (d == 1 || d == -1) ? 0.25f : 0.0625f; }

MCPT_HD bool dn_finite(float v) { return v - v == 0.f; }
MCPT_HD float dn_rz(float z) {
    const float z2 = z * z;
    return 1.f / (z2 > 1e-12f ? z2 : 1e-12f);
}
// The three planes of a pixel from its mean colour, whether it has samples, and its mean guides
MCPT_HD void dn_planes(float r, float g, float b, bool has_samples, float nx, float ny, float nz, float z, float ar,
                       float ag, float ab, float4& col, float4& gd, float4& al) {
    const bool valid = has_samples && dn_finite(r) && dn_finite(g) && dn_finite(b);
    col = valid ? make_float4(r, g, b, 1.f) : make_float4(0.f, 0.f, 0.f, 0.f);
    gd = make_float4(nx, ny, nz, z);
    al = make_float4(ar, ag, ab, dn_rz(z));
}

struct DnAcc {
    float w, r, g, b;
    float v;  // the guided form's variance sum (the plain form leaves it alone)
};
MCPT_HD float dn_sq3(float ax, float ay, float az, float bx, float by, float bz) {
    const float dx = ax - bx, dy = ay - by, dz = az - bz;
    return (dx * dx + dy * dy) + dz * dz;
}
// The plain colour term of a tap: kc |C(p) - C(q)|^2
MCPT_HD float dn_xc(const DenoisePass& k, const float4& cp, const float4& cq) {
    return k.kc * dn_sq3(cp.x, cp.y, cp.z, cq.x, cq.y, cq.z);
}
// Edge-stopping factor of a tap q != p, given its colour term xc: exp(-(xc + the normal, albedo and
// depth terms)); an exponent that is not a finite number >= 0 gives 0.  (aq.w is not looked at.)
MCPT_HD float dn_edge(const DenoisePass& k, float xc, const float4& gp, const float4& ap, const float4& gq,
                      const float4& aq) {
    const float dn = dn_sq3(gp.x, gp.y, gp.z, gq.x, gq.y, gq.z);
    const float da = dn_sq3(ap.x, ap.y, ap.z, aq.x, aq.y, aq.z);
    const float dz = gp.w - gq.w;
    const float x = ((xc + k.kn * dn) + k.ka * da) + (k.kz * (dz * dz)) * ap.w;
    return (x >= 0.f && x <= 3.402823466e+38f) ? dexp_neg(x) : 0.f;
}
// Weight of tap q = p + stride (dx, dy) of a valid pixel p, given its colour term xc (dn_xc, or the
// guided form's).  The centre's exponent is 0 by definition (its xc is not looked at).
MCPT_HD float dn_weight(const DenoisePass& k, int dx, int dy, float xc, const float4& gp, const float4& ap,
                        const float4& gq, const float4& aq) {
    float e = 1.f;
    if (dx != 0 || dy != 0) e = dn_edge(k, xc, gp, ap, gq, aq);
    return (dn_h(dy) * dn_h(dx)) * e;
}
MCPT_HD void dn_add(float w, const float4& cq, DnAcc& acc) {
    acc.w = acc.w + w;
    acc.r = acc.r + w * cq.x;
    acc.g = acc.g + w * cq.y;
    acc.b = acc.b + w * cq.z;
}
// The plain tap; cq.w != 0 (the caller skips invalid taps and taps outside the film)
MCPT_HD void dn_tap(const DenoisePass& k, int dx, int dy, const float4& cp, const float4& gp, const float4& ap,
                    const float4& cq, const float4& gq, const float4& aq, DnAcc& acc) {
    dn_add(dn_weight(k, dx, dy, dn_xc(k, cp, cq), gp, ap, gq, aq), cq, acc);
}
MCPT_HD float4 dn_finish(const DnAcc& acc) { return make_float4(acc.r / acc.w, acc.g / acc.w, acc.b / acc.w, 1.f); }

// ---- variance-guided form ----
// SVGF's spatial filter (Schied et al., HPG 2017, section 4.4): the a-trous filter above with the
// colour term replaced by |l(p) - l(q)| / (sigma_lum sqrt(prefiltered variance of p) + lum_eps), and
// the variance of the pixel's mean luminance filtered along with the colour.  Beside the three planes
// a pixel carries (float2)
//   vl  (v, l)   v: variance of its mean luminance, -1 where unknown (always -1 for an invalid pixel);
//                l = luminance(colour), evaluated once per pixel and pass (0 for an invalid pixel)
// A pixel without a variance takes the plain filter's colour term, so with every variance unknown the
// colours are dn_tap's bit for bit.  Beside add / mul / div this part takes one correctly rounded square
// root per pixel and pass, and luminance() computes in double (tests/denoise_guided_ref.py restates it).
//
// The guided part of a pass: the colour term's two parameters and the vl planes, vl -> out_vl in
// ping-pong beside the colour
struct DenoiseVar {
    float sigma_lum, lum_eps;
    const float2* vl;
    float2* out_vl;
};
MCPT_HD bool dn_known(float v) { return v >= 0.f; }
MCPT_HD float2 dn_vl(const float4& col, float var) {
    const bool valid = col.w != 0.f;
    return make_float2(valid && var >= 0.f && var <= 3.402823466e+38f ? var : -1.f,
                       valid ? luminance(V3{col.x, col.y, col.z}) : 0.f);
}
// Prefilter of a pixel with a known variance: the 3 x 3 Gaussian {1/4, 1/8, 1/16} over the neighbours
// at stride 1 (whatever the pass) whose variance is known, row-major; the caller skips the others
struct DnPre {
    float gs, gv;
};
MCPT_HD void dn_pre_tap(int dx, int dy, float vr, DnPre& a) {
    const float g = (dx == 0 && dy == 0) ? 0.25f : (dx == 0 || dy == 0) ? 0.125f : 0.0625f;
    a.gs = a.gs + g;
    a.gv = a.gv + g * vr;
}
// 1 / (sigma_lum sqrt(vt) + lum_eps); vt = 0 with lum_eps = 0 gives +Inf, which leaves only the centre tap
MCPT_HD float dn_pre_rcp(const DenoiseVar& k, const DnPre& a) {
    const float vt = a.gv / a.gs;
    return 1.f / (k.sigma_lum * __builtin_sqrtf(vt) + k.lum_eps);
}
// dn_tap with the variance: known = dn_known(vlp.x), rcp = dn_pre_rcp of p (any finite value
// otherwise).  Both colour terms and the variance sum are evaluated whatever `known` is and selected,
// so the kernels' taps stay free of branches; acc.v of a pixel without a variance is never used.
MCPT_HD void dn_tap_guided(const DenoisePass& k, int dx, int dy, bool known, float rcp, const float4& cp, const float2& vlp,
                           const float4& gp, const float4& ap, const float4& cq, const float2& vlq, const float4& gq,
                           const float4& aq, DnAcc& acc) {
    const float xl = __builtin_fabsf(vlp.y - vlq.y) * rcp;
    const float xp = dn_xc(k, cp, cq);
    const float w = dn_weight(k, dx, dy, known ? xl : xp, gp, ap, gq, aq);
    dn_add(w, cq, acc);
    acc.v = acc.v + (w * w) * (dn_known(vlq.x) ? vlq.x : vlp.x);
}
// The vl of a filtered pixel: col = dn_finish(acc)
MCPT_HD float2 dn_finish_vl(const DnAcc& acc, bool known, const float4& col) {
    return make_float2(known ? acc.v / (acc.w * acc.w) : -1.f, luminance(V3{col.x, col.y, col.z}));
}

// Host form of one pass over W x H planes, guided where v != nullptr (the kernels' parity reference;
// tests/native/denoise_host.cpp, denoise_guided_host.cpp)
inline void denoise_pass_host(const DenoisePass& k, int W, int H, const float4* col, const float4* gd, const float4* al,
                              float4* out, const DenoiseVar* v = nullptr) {
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            const size_t p = (size_t)y * W + x;
            const float4 cp = col[p];
            if (cp.w == 0.f) {
                out[p] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (v) v->out_vl[p] = make_float2(-1.f, 0.f);
                continue;
            }
            float2 vlp = make_float2(-1.f, 0.f);
            bool known = false;
            float rcp = 0.f;
            if (v) {
                vlp = v->vl[p];
                known = dn_known(vlp.x);
            }
            if (known) {
                DnPre pre{0.f, 0.f};
                for (int dy = -1; dy <= 1; dy++)
                    for (int dx = -1; dx <= 1; dx++) {
                        const int rx = x + dx, ry = y + dy;
                        if (rx < 0 || rx >= W || ry < 0 || ry >= H) continue;
                        const float vr = v->vl[(size_t)ry * W + (size_t)rx].x;
                        if (dn_known(vr)) dn_pre_tap(dx, dy, vr, pre);
                    }
                rcp = dn_pre_rcp(*v, pre);
            }
            DnAcc acc{0.f, 0.f, 0.f, 0.f, 0.f};
            for (int dy = -2; dy <= 2; dy++)
                for (int dx = -2; dx <= 2; dx++) {
                    const long qx = (long)x + (long)dx * k.stride, qy = (long)y + (long)dy * k.stride;
                    if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
                    const size_t q = (size_t)qy * W + (size_t)qx;
                    if (col[q].w == 0.f) continue;
                    if (v) dn_tap_guided(k, dx, dy, known, rcp, cp, vlp, gd[p], al[p], col[q], v->vl[q], gd[q], al[q], acc);
                    else dn_tap(k, dx, dy, cp, gd[p], al[p], col[q], gd[q], al[q], acc);
                }
            out[p] = dn_finish(acc);
            if (v) v->out_vl[p] = dn_finish_vl(acc, known, out[p]);
        }
}

// The guided pass by its own name and parameter struct (tests/native/denoise_guided_host.cpp)
struct DenoiseGuidedPass {
    DenoisePass k;            // k.kc: the fallback term of a pixel without a variance
    float sigma_lum, lum_eps;
};
inline void denoise_guided_pass_host(const DenoiseGuidedPass& k, int W, int H, const float4* col, const float2* vl,
                                     const float4* gd, const float4* al, float4* out, float2* out_vl) {
    const DenoiseVar v{k.sigma_lum, k.lum_eps, vl, out_vl};
    denoise_pass_host(k.k, W, H, col, gd, al, out, &v);
}

}  // namespace mcpt
