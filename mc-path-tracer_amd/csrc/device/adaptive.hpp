// adaptive.hpp -- arithmetic of adaptive sampling: the film's error estimate from the path slots'
// accumulators and the per-pixel sample budget built from it.
//
// __host__ __device__, add / mul / IEEE div and sqrt only, one rounding per operation under the
// project's flags (-ffp-contract=off, correctly rounded division and square root): the host build and
// the gfx950 kernels (adaptive.hip) agree bit for bit, as with denoise.hpp.  tests/adaptive_ref.py
// restates every expression below in numpy float32, in the same order.
//
// Path slot k of a pixel accumulates the pixel's samples k, k + S, k + 2S, ... into its own (Ld_k,
// n_k): the slot means are S estimates of the pixel from disjoint sample sets, so their spread is a
// standard error of their mean, and the hot kernels pay nothing for it.
#pragma once
#include "mcpt_core.hpp"

namespace mcpt {

// Slot k's accumulator of one pixel is Ld[k * stride + i], n[k * stride + i], k < slots.  Over the
// slots with n_k > 0, in ascending order (K of them):
//   y_k  = luminance(Ld_k) / (float)n_k
//   ybar = (((y_0 + y_1) + y_2) + ...) / (float)K
//   s2   = (((d_0 d_0 + d_1 d_1) + ...) / (float)(K - 1),  d_k = y_k - ybar
//   se   = sqrt(s2 / (float)K)
// Result {se, ybar, (float)K, (float)n}, n = sum of n_k (exact: < 2^24).  K < 2: no estimate, se = -1
// (K = 0: ybar = 0).  Non-finite sums propagate into ybar and se.
MCPT_HD float err_slot_mean(const float4& L, uint32_t n) { return luminance(V3{L.x, L.y, L.z}) / (float)n; }
MCPT_HD float4 film_error_pixel(const float4* Ld, const uint32_t* ns, size_t stride, size_t i, int slots) {
    float sum = 0.f;
    uint32_t K = 0, n = 0;
    for (int k = 0; k < slots; k++) {
        const uint32_t nk = ns[(size_t)k * stride + i];
        if (nk == 0) continue;
        sum = sum + err_slot_mean(Ld[(size_t)k * stride + i], nk);
        K++;
        n += nk;
    }
    if (K == 0) return make_float4(-1.f, 0.f, 0.f, 0.f);
    const float ybar = sum / (float)K;
    if (K < 2) return make_float4(-1.f, ybar, (float)K, (float)n);
    float ss = 0.f;
    for (int k = 0; k < slots; k++) {
        const uint32_t nk = ns[(size_t)k * stride + i];
        if (nk == 0) continue;
        const float d = err_slot_mean(Ld[(size_t)k * stride + i], nk) - ybar;
        ss = ss + d * d;
    }
    const float s2 = ss / (float)(K - 1);
    return make_float4(__builtin_sqrtf(s2 / (float)K), ybar, (float)K, (float)n);
}

// Budget of a pixel from its estimate e = {se, ybar, K, n} (mcpt_sample_budget_params; tau > 0,
// lum_floor >= 0, min_spp <= max_spp).  With lo = max(n, min_spp):
//   not owned (another context's pixel, or the never-rendered last row / column)   0
//   se < 0 (no estimate)                                                           lo
//   r = se / (ybar + lum_floor) not finite (a NaN pixel cannot converge)           n
//   r <= tau                                                                       lo
//   want = n ((r / tau) (r / tau)) as  e.w * (q * q), q = r / tau
//   !(want < (float)max_spp)  (an overflow to +Inf included)                       max(max_spp, lo)
//   else max(ceil(want), lo); the ceiling is t = (uint32_t)want, plus 1 where (float)t < want --
//   want is positive and below max_spp <= 2^19 - 256, so the conversion is exact and in range.
struct BudgetParams {
    float tau, lum_floor;
    uint32_t min_spp, max_spp;
};
MCPT_HD bool err_finite(float v) { return v - v == 0.f; }
MCPT_HD uint32_t budget_pixel(const float4& e, bool owned, const BudgetParams& p) {
    if (!owned) return 0u;
    const uint32_t n = (uint32_t)e.w;
    const uint32_t lo = n > p.min_spp ? n : p.min_spp;
    if (e.x < 0.f) return lo;
    const float r = e.x / (e.y + p.lum_floor);
    if (!err_finite(r)) return n;
    if (r <= p.tau) return lo;
    const float q = r / p.tau;
    const float want = e.w * (q * q);
    if (!(want < (float)p.max_spp)) return p.max_spp > lo ? p.max_spp : lo;
    const uint32_t t = (uint32_t)want;
    const uint32_t c = t + ((float)t < want ? 1u : 0u);
    return c > lo ? c : lo;
}

}  // namespace mcpt
