// temporal.hip -- gfx950 kernels of the temporal stage of the preview denoiser (device/temporal.hpp,
// DESIGN.md section 13).
//
// k_temporal<FILM>: one thread per pixel, blocks of 64 x 4 pixels.  A pixel forms its current-frame
// record (from the film, the film error, the guide sums and the camera records, or from caller images),
// projects its first hit into the previous frame and gathers the 2 x 2 bilinear tap from the three
// history planes.  Neighbouring pixels reproject onto neighbouring history pixels, so the gather of a
// wave covers about the wave's own footprint shifted by the motion: the compulsory traffic is the
// three history planes once (48 B), the current frame (about 60 B from the film) and the five planes
// written (72 B).  The twelve tap loads are issued together, at clamped addresses, before any test:
// the consistency tests and the sums then select, so the tap has no branch and no dependent load.
#include "kernels.hpp"

#include "device/temporal.hpp"

namespace mcpt_dev {

using namespace mcpt;

template <bool FILM>
__global__ __launch_bounds__(256) void k_temporal(TemporalArgs a) {
    const int x = (int)blockIdx.x * 64 + (int)threadIdx.x % 64, y = (int)blockIdx.y * 4 + (int)threadIdx.x / 64;
    if (x >= a.W || y >= a.H) return;
    const size_t i = (size_t)y * (size_t)a.W + (size_t)x;
    TpPixel p;
    if constexpr (FILM) {
        const float4 L = a.Ld[i];
        const uint32_t ns = a.samples[i];
        const float s = (float)ns;
        const float4 gn = a.g_nz[i];
        const float cnt = a.g_alb[i].w;  // the guide sample count
        const float z = gn.w / cnt;
        float var = -1.f;
        if (a.err) {
            const float se = a.err[i].x;
            var = (se >= 0.f && dn_finite(se)) ? se * se : -1.f;
        }
        if (a.vfill && !(var >= 0.f)) var = a.vfill[i].x;  // no slot estimate: the spatial one (or -1)
        const float4 cp = a.cam_px[i], cd = a.cam_dir[i];
        // (the camera table holds pFocal for a lens and the pinhole origin otherwise: k_cam_table)
        const V3 X = a.cam.lens_radius > 0.f ? tp_world_focal(a.cam, v3(cp.x, cp.y, cp.z), z)
                                             : v3(cp.x, cp.y, cp.z) + v3(cd.x, cd.y, cd.z) * z;
        p = tp_pixel(L.x / s, L.y / s, L.z / s, ns > 0, s, var, X, v3(gn.x / cnt, gn.y / cnt, gn.z / cnt), z);
    } else {
        const uint32_t ns = a.samples[i];
        p = tp_pixel(a.rgb[3 * i], a.rgb[3 * i + 1], a.rgb[3 * i + 2], ns > 0, (float)ns, a.variance[i],
                     v3(a.position[3 * i], a.position[3 * i + 1], a.position[3 * i + 2]),
                     v3(a.normal[3 * i], a.normal[3 * i + 1], a.normal[3 * i + 2]), a.depth[i]);
    }
    const TpProj q = tp_project(a.vp_prev, p, a.W, a.H);
    float4 hc[4], hp[4], hn[4];
    bool in[4];
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const int qx = q.x0 + tp_corner_dx(c), qy = q.y0 + tp_corner_dy(c);
        in[c] = qx >= 0 && qx < a.W && qy >= 0 && qy < a.H;
        const size_t j = in[c] ? (size_t)qy * (size_t)a.W + (size_t)qx : i;
        hc[c] = a.hcol[j];
        hp[c] = a.hpos[j];
        hn[c] = a.hnrm[j];
    }
    TpAcc acc{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, true};
#pragma unroll
    for (int c = 0; c < 4; c++) tp_tap(a.k, p, tp_corner_w(q, c), in[c], hc[c], hp[c], hn[c], acc);
    const TpOut o = tp_blend(a.k, p, q, acc);
    a.col[i] = o.col;
    a.vl[i] = o.vl;
    a.out_hcol[i] = o.hcol;
    a.out_hpos[i] = o.hpos;
    a.out_hnrm[i] = o.hnrm;
}

void launch_temporal(const TemporalArgs& a, hipStream_t s) {
    if (a.W <= 0 || a.H <= 0) return;
    const dim3 g((unsigned)((a.W + 63) / 64), (unsigned)((a.H + 3) / 4));
    if (a.Ld) hipLaunchKernelGGL(k_temporal<true>, g, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(k_temporal<false>, g, dim3(256), 0, s, a);
}

__global__ void k_temporal_prep(TemporalPrepArgs a) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const float4 ga = a.g_alb[i], gn = a.g_nz[i];
    const float cnt = ga.w;
    float4 col, gd, al;
    dn_planes(0.f, 0.f, 0.f, true, gn.x / cnt, gn.y / cnt, gn.z / cnt, gn.w / cnt, ga.x / cnt, ga.y / cnt, ga.z / cnt, col, gd,
              al);
    a.col[i] = a.tcol[i];
    a.vl[i] = a.tvl[i];
    a.gd[i] = gd;
    a.al[i] = al;
}
void launch_temporal_prep(const TemporalPrepArgs& a, hipStream_t s) {
    if (a.n) hipLaunchKernelGGL(k_temporal_prep, dim3((a.n + 255) / 256), dim3(256), 0, s, a);
}

}  // namespace mcpt_dev
