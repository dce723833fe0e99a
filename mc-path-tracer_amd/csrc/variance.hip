// variance.hip -- gfx950 kernel of the spatial variance estimate (device/variance.hpp, DESIGN.md
// section 14): fills the variances the path slots did not give, once per frame, between the filter's
// plane set-up and its first pass.
//
// k_variance_spatial<R> is tiled as k_denoise_lds is: a block stages its 32 x 16 tile with a halo of R
// in LDS and every tap is served from there.  A tap needs its luminance, whether it is valid, its guide
// float4 and its albedo rgb: 36 B in three arrays (the albedo array's w holds the colour plane's valid
// flag; the centre's 1 / z^2 is one global read per pixel), so the widest tile, R = 3, is
// 38 x 22 x 36 B = 29.4 KiB.  The halo costs 1.2 / 1.4 / 1.6 global reads per pixel and plane.
//
// The kernel works in place on the vl plane: a thread reads its neighbours' luminances and guides and
// its own variance, and writes only its own variance.  The luminances and variances are read and
// written as single floats of the float2 plane, so no load ever covers a variance another thread stores.
#include "kernels.hpp"

#include "device/variance.hpp"

namespace mcpt_dev {

using namespace mcpt;

constexpr int kVrTileW = 32, kVrTileH = 16;  // pixels per block; 256 threads, two rows each (as the filter's)

template <int R>
__global__ __launch_bounds__(256) void k_variance_spatial(VarianceArgs a) {
    constexpr int LW = kVrTileW + 2 * R, LH = kVrTileH + 2 * R;
    __shared__ float4 s_gd[LW * LH];
    __shared__ float4 s_al[LW * LH];  // albedo rgb, valid
    __shared__ float s_l[LW * LH];
    const float* colf = (const float*)a.col;
    float* vlf = (float*)a.vl;
    const int x0 = (int)blockIdx.x * kVrTileW, y0 = (int)blockIdx.y * kVrTileH;
    for (int i = (int)threadIdx.x; i < LW * LH; i += 256) {
        const int lx = i % LW, ly = i / LW;
        const int gx = x0 - R + lx, gy = y0 - R + ly;
        float4 g = make_float4(0.f, 0.f, 0.f, 0.f), al = g;  // outside the image: an invalid tap
        float l = 0.f;
        if (gx >= 0 && gx < a.W && gy >= 0 && gy < a.H) {
            const size_t q = (size_t)gy * (size_t)a.W + (size_t)gx;
            g = a.gd[q];
            al = a.al[q];
            al.w = colf[4 * q + 3];
            l = vlf[2 * q + 1];
        }
        s_gd[i] = g;
        s_al[i] = al;
        s_l[i] = l;
    }
    __syncthreads();
    const DenoisePass ek = vr_edge_pass(a.k);
    const int tx = (int)threadIdx.x % kVrTileW, ty0 = (int)threadIdx.x / kVrTileW;
    for (int ty = ty0; ty < kVrTileH; ty += 256 / kVrTileW) {
        const int x = x0 + tx, y = y0 + ty;
        if (x >= a.W || y >= a.H) continue;
        const int lp = (ty + R) * LW + tx + R;
        float4 ap = s_al[lp];
        if (ap.w == 0.f) continue;  // an invalid pixel stays at -1
        const size_t p = (size_t)y * (size_t)a.W + (size_t)x;
        if (dn_known(vlf[2 * p])) continue;  // fill only
        ap.w = a.al[p].w;
        const float4 gp = s_gd[lp];
        const float l0 = s_l[lp];
        VrAcc acc{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int dy = -R; dy <= R; dy++)
#pragma unroll
            for (int dx = -R; dx <= R; dx++) {
                const int lq = lp + dy * LW + dx;
                const float4 aq = s_al[lq];
                if (aq.w == 0.f) continue;
                const float e = (dx == 0 && dy == 0) ? 1.f : dn_edge(ek, 0.f, gp, ap, s_gd[lq], aq);
                vr_tap(e, l0, s_l[lq], acc);
            }
        vlf[2 * p] = vr_finish(a.k, acc);
    }
}

void launch_variance_spatial(const VarianceArgs& a, hipStream_t s) {
    if (a.W <= 0 || a.H <= 0) return;
    const dim3 tg((unsigned)((a.W + kVrTileW - 1) / kVrTileW), (unsigned)((a.H + kVrTileH - 1) / kVrTileH));
    if (a.k.radius == 1) hipLaunchKernelGGL(k_variance_spatial<1>, tg, dim3(256), 0, s, a);
    else if (a.k.radius == 2) hipLaunchKernelGGL(k_variance_spatial<2>, tg, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(k_variance_spatial<3>, tg, dim3(256), 0, s, a);
}

}  // namespace mcpt_dev
