// denoise_guided.hip -- gfx950 kernels of the variance-guided a-trous filter (device/denoise.hpp,
// DESIGN.md section 12): the counterparts of denoise.hip's k_denoise_lds / k_denoise_direct /
// k_denoise_prep_*, which stay as they are.
//
// On top of the plain filter's three float4 planes a pixel carries a float2 {variance of its mean
// luminance or -1, luminance}, in ping-pong like the colour: 80 B of compulsory traffic per pixel and
// pass against 64 B.  A tap is 56 B, so the LDS tiles are 36 x 20 x 56 B = 39.4 KiB (stride 1) and
// 40 x 24 x 56 B = 52.5 KiB (stride 2): 4 / 3 blocks per CU of the 160 KiB, under the 64 KiB static
// limit.  The 3 x 3 variance prefilter is at stride 1 in every pass: in the LDS kernels its halo of 1
// lies inside the 2-stride halo, in the direct kernel it is nine adjacent reads of the float2 plane.
// An invalid pixel's variance is -1 by construction (dn_vl, dn_finish_guided's callers), so the
// prefilter needs the float2 plane only.  The reciprocal of the colour term is computed once per pixel.
// As in denoise.hip the LDS and the direct kernels run the same tap sequence per pixel: same bits.
#include "kernels.hpp"

#include "device/denoise.hpp"

namespace mcpt_dev {

using namespace mcpt;

constexpr int kDgTileW = 32, kDgTileH = 16;  // as denoise.hip: 256 threads, two rows each

template <int S>
__global__ __launch_bounds__(256) void k_denoise_guided_lds(DenoiseGuidedArgs a) {
    constexpr int LW = kDgTileW + 4 * S, LH = kDgTileH + 4 * S;
    __shared__ float4 s_col[LW * LH];
    __shared__ float4 s_gd[LW * LH];
    __shared__ float4 s_al[LW * LH];
    __shared__ float2 s_vl[LW * LH];
    const int x0 = (int)blockIdx.x * kDgTileW, y0 = (int)blockIdx.y * kDgTileH;
    for (int i = (int)threadIdx.x; i < LW * LH; i += 256) {
        const int lx = i % LW, ly = i / LW;
        const int gx = x0 - 2 * S + lx, gy = y0 - 2 * S + ly;
        float4 c = make_float4(0.f, 0.f, 0.f, 0.f), g = c, al = c;  // outside the film: an invalid tap
        float2 vl = make_float2(-1.f, 0.f);
        if (gx >= 0 && gx < a.W && gy >= 0 && gy < a.H) {
            const size_t q = (size_t)gy * (size_t)a.W + (size_t)gx;
            c = a.col[q];
            g = a.gd[q];
            al = a.al[q];
            vl = a.vl[q];
        }
        s_col[i] = c;
        s_gd[i] = g;
        s_al[i] = al;
        s_vl[i] = vl;
    }
    __syncthreads();
    const int tx = (int)threadIdx.x % kDgTileW, ty0 = (int)threadIdx.x / kDgTileW;
    for (int ty = ty0; ty < kDgTileH; ty += 256 / kDgTileW) {
        const int x = x0 + tx, y = y0 + ty;
        if (x >= a.W || y >= a.H) continue;
        const int lp = (ty + 2 * S) * LW + tx + 2 * S;
        const float4 cp = s_col[lp];
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
        float2 ov = make_float2(-1.f, 0.f);
        if (cp.w != 0.f) {
            const float4 gp = s_gd[lp], ap = s_al[lp];
            const float2 vlp = s_vl[lp];
            const bool known = dn_known(vlp.x);
            float rcp = 0.f;
            if (known) {
                DnPre pre{0.f, 0.f};
#pragma unroll
                for (int dy = -1; dy <= 1; dy++)
#pragma unroll
                    for (int dx = -1; dx <= 1; dx++) {
                        const float vr = s_vl[lp + dy * LW + dx].x;
                        if (dn_known(vr)) dn_pre_tap(dx, dy, vr, pre);
                    }
                rcp = dn_pre_rcp(a.k, pre);
            }
            DnAccV acc{0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int dy = -2; dy <= 2; dy++)
#pragma unroll
                for (int dx = -2; dx <= 2; dx++) {
                    const int lq = lp + dy * S * LW + dx * S;
                    const float4 cq = s_col[lq];
                    if (cq.w == 0.f) continue;
                    dn_tap_guided(a.k, dx, dy, known, rcp, cp, vlp, gp, ap, cq, s_vl[lq], s_gd[lq], s_al[lq], acc);
                }
            dn_finish_guided(acc, known, o, ov);
        }
        const size_t p = (size_t)y * (size_t)a.W + (size_t)x;
        a.out[p] = o;
        a.out_vl[p] = ov;
    }
}

__global__ __launch_bounds__(256) void k_denoise_guided_direct(DenoiseGuidedArgs a) {
    const int x = (int)blockIdx.x * 64 + (int)threadIdx.x % 64, y = (int)blockIdx.y * 4 + (int)threadIdx.x / 64;
    if (x >= a.W || y >= a.H) return;
    const size_t p = (size_t)y * (size_t)a.W + (size_t)x;
    const float4 cp = a.col[p];
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    float2 ov = make_float2(-1.f, 0.f);
    if (cp.w != 0.f) {
        const float4 gp = a.gd[p], ap = a.al[p];
        const float2 vlp = a.vl[p];
        const bool known = dn_known(vlp.x);
        float rcp = 0.f;
        if (known) {
            // the nine reads at clamped coordinates, issued together; a neighbour outside the film counts as unknown
            float vr[9];
#pragma unroll
            for (int dy = -1; dy <= 1; dy++)
#pragma unroll
                for (int dx = -1; dx <= 1; dx++) {
                    const int rx = x + dx, ry = y + dy;
                    const bool in = rx >= 0 && rx < a.W && ry >= 0 && ry < a.H;
                    const float v = a.vl[in ? (size_t)ry * (size_t)a.W + (size_t)rx : p].x;
                    vr[(dy + 1) * 3 + dx + 1] = in ? v : -1.f;
                }
            DnPre pre{0.f, 0.f};
#pragma unroll
            for (int dy = -1; dy <= 1; dy++)
#pragma unroll
                for (int dx = -1; dx <= 1; dx++)
                    if (dn_known(vr[(dy + 1) * 3 + dx + 1])) dn_pre_tap(dx, dy, vr[(dy + 1) * 3 + dx + 1], pre);
            rcp = dn_pre_rcp(a.k, pre);
        }
        const int S = a.k.k.stride;
        DnAccV acc{0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int dy = -2; dy <= 2; dy++) {
            const int qy = y + dy * S;
            if (qy < 0 || qy >= a.H) continue;
#pragma unroll
            for (int dx = -2; dx <= 2; dx++) {
                const int qx = x + dx * S;
                if (qx < 0 || qx >= a.W) continue;
                const size_t q = (size_t)qy * (size_t)a.W + (size_t)qx;
                const float4 cq = a.col[q];
                if (cq.w == 0.f) continue;
                dn_tap_guided(a.k, dx, dy, known, rcp, cp, vlp, gp, ap, cq, a.vl[q], a.gd[q], a.al[q], acc);
            }
        }
        dn_finish_guided(acc, known, o, ov);
    }
    a.out[p] = o;
    a.out_vl[p] = ov;
}

void launch_denoise_guided_pass(const DenoiseGuidedArgs& a, int lds_max_stride, hipStream_t s) {
    if (a.W <= 0 || a.H <= 0) return;
    const dim3 tg((unsigned)((a.W + kDgTileW - 1) / kDgTileW), (unsigned)((a.H + kDgTileH - 1) / kDgTileH));
    if (a.k.k.stride == 1 && lds_max_stride >= 1) hipLaunchKernelGGL(k_denoise_guided_lds<1>, tg, dim3(256), 0, s, a);
    else if (a.k.k.stride == 2 && lds_max_stride >= 2) hipLaunchKernelGGL(k_denoise_guided_lds<2>, tg, dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL(k_denoise_guided_direct, dim3((unsigned)((a.W + 63) / 64), (unsigned)((a.H + 3) / 4)), dim3(256), 0, s,
                           a);
}

// The planes as k_denoise_prep_film / k_denoise_prep_images form them, plus {variance, luminance}
__global__ void k_denoise_guided_prep_film(DenoiseGuidedPrepArgs g) {
    const DenoisePrepArgs& a = g.base;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const float4 L = a.Ld[i];
    const uint32_t ns = a.samples[i];
    const float s = (float)ns;
    const float4 ga = a.g_alb[i], gn = a.g_nz[i];
    const float cnt = ga.w;
    float4 col, gd, al;
    dn_planes(L.x / s, L.y / s, L.z / s, ns > 0, gn.x / cnt, gn.y / cnt, gn.z / cnt, gn.w / cnt, ga.x / cnt, ga.y / cnt,
              ga.z / cnt, col, gd, al);
    a.col[i] = col;
    a.gd[i] = gd;
    a.al[i] = al;
    const float se = g.err[i].x;
    g.vl[i] = dn_vl(col, (se >= 0.f && dn_finite(se)) ? se * se : -1.f);
}
__global__ void k_denoise_guided_prep_images(DenoiseGuidedPrepArgs g) {
    const DenoisePrepArgs& a = g.base;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    float4 col, gd, al;
    dn_planes(a.rgb[3 * (size_t)i], a.rgb[3 * (size_t)i + 1], a.rgb[3 * (size_t)i + 2], a.samples ? a.samples[i] > 0 : true,
              a.normal[3 * (size_t)i], a.normal[3 * (size_t)i + 1], a.normal[3 * (size_t)i + 2], a.depth[i],
              a.albedo[3 * (size_t)i], a.albedo[3 * (size_t)i + 1], a.albedo[3 * (size_t)i + 2], col, gd, al);
    a.col[i] = col;
    a.gd[i] = gd;
    a.al[i] = al;
    g.vl[i] = dn_vl(col, g.variance[i]);
}
void launch_denoise_guided_prep(const DenoiseGuidedPrepArgs& a, hipStream_t s) {
    if (!a.base.n) return;
    if (a.base.Ld) hipLaunchKernelGGL(k_denoise_guided_prep_film, dim3((a.base.n + 255) / 256), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(k_denoise_guided_prep_images, dim3((a.base.n + 255) / 256), dim3(256), 0, s, a);
}

}  // namespace mcpt_dev
