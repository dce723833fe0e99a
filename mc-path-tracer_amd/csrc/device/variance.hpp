// variance.hpp -- arithmetic of the spatial variance estimate: a variance of
// the mean luminance for pixels that have none from the path slots, SVGF's spatial fallback (Schied et
// al., "Spatiotemporal Variance-Guided Filtering", HPG 2017, section 4.2): luminance moments over a
// (2R + 1)^2 window, edge-stopped by the guides.
//
// __host__ __device__ in the style of denoise.hpp: add / mul / IEEE div only, one rounding per
// operation under the project's flags.  The host build and the gfx950 kernel (variance.hip) agree bit
// for bit; tests/variance_ref.py restates every expression below in numpy float32, in the same order.
//
// Over the planes of denoise.hpp.  Of a valid pixel p without a known variance, the taps q = p + (dx, dy),
// |dx|, |dy| <= R, row-major, skipping taps outside the image and invalid ones:
//   e = 1 at the centre, else dn_edge with a zero colour term (the filter's normal, albedo and depth terms)
//   d = l(q) - l(p);  sw += e;  sww += e e;  s1 += e d;  s2 += e (d d)
// The moments are shifted by the centre's luminance: a constant window gives exactly 0, and there is
// no E[l^2] - E[l]^2 cancellation on converged pixels.  Then
//   m = s1 / sw;  var = max(s2 / sw - m m, 0);  neff = (sw sw) / sww;  var = var (neff / (neff - 1))
// and the variance is known if neff >= min_neff and var is a finite number >= 0 (a NaN anywhere falls
// to "unknown", -1).  A pixel whose variance is known keeps it; an invalid pixel stays at -1.
#pragma once
#include "denoise.hpp"

namespace mcpt {

struct VariancePass {
    float kn, ka, kz;  // dn_k of the three guide sigmas (0: the term is off)
    float min_neff;
    int radius;
};
// The edge term's parameters as the filter's struct: no colour term, stride 1
MCPT_HD DenoisePass vr_edge_pass(const VariancePass& k) { return DenoisePass{0.f, k.kn, k.ka, k.kz, 1}; }

struct VrAcc {
    float sw, sww, s1, s2;
};
// One tap; e: its edge weight, lp / lq: the luminances of the centre and the tap
MCPT_HD void vr_tap(float e, float lp, float lq, VrAcc& a) {
    const float d = lq - lp;
    a.sw = a.sw + e;
    a.sww = a.sww + e * e;
    a.s1 = a.s1 + e * d;
    a.s2 = a.s2 + e * (d * d);
}
MCPT_HD float vr_finish(const VariancePass& k, const VrAcc& a) {
    const float m = a.s1 / a.sw;
    const float raw = a.s2 / a.sw - m * m;
    float var = raw > 0.f ? raw : 0.f;
    const float neff = (a.sw * a.sw) / a.sww;
    var = var * (neff / (neff - 1.f));
    // (the clamp would turn a NaN of overflowed moments into 0: raw itself must be a finite number)
    return (neff >= k.min_neff && dn_finite(raw) && var >= 0.f && var <= 3.402823466e+38f) ? var : -1.f;
}

// Host form over W x H planes, in place on vl's variances (the kernel's parity reference;
// tests/native/variance_host.cpp).  Only variances are written and none is read from a neighbour, so
// the order of the pixels does not matter.
inline void variance_pass_host(const VariancePass& k, int W, int H, const float4* col, const float4* gd, const float4* al,
                               float2* vl) {
    const DenoisePass ek = vr_edge_pass(k);
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            const size_t p = (size_t)y * W + x;
            if (col[p].w == 0.f || dn_known(vl[p].x)) continue;
            VrAcc acc{0.f, 0.f, 0.f, 0.f};
            for (int dy = -k.radius; dy <= k.radius; dy++)
                for (int dx = -k.radius; dx <= k.radius; dx++) {
                    const int qx = x + dx, qy = y + dy;
                    if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
                    const size_t q = (size_t)qy * W + (size_t)qx;
                    if (col[q].w == 0.f) continue;
                    const float e = (dx == 0 && dy == 0) ? 1.f : dn_edge(ek, 0.f, gd[p], al[p], gd[q], al[q]);
                    vr_tap(e, vl[p].y, vl[q].y, acc);
                }
            vl[p].x = vr_finish(k, acc);
        }
}

}  // namespace mcpt
