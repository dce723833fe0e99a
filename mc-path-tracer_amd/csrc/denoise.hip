// denoise.hip -- gfx950 kernels of the preview denoiser: the first-hit guide pass (camera rays of the
// film's samples, accumulated per pixel) and the edge-avoiding a-trous filter (device/denoise.hpp).
//
// The filter is one launch per pass over three float4 planes (colour + valid, normal + depth,
// albedo + 1/z^2) with two colour planes in ping-pong: 64 B of compulsory traffic per pixel and
// pass.  Each pixel reads 25 taps x 3 planes, so what a pass costs is set by where the 75 float4
// reads per pixel are served from:
//   strides 1 and 2 (k_denoise_lds): a block stages its 32 x 16 tile with the 2-stride halo in LDS
//     (36 x 20 / 40 x 24 pixels x 48 B = 34 / 45 KiB, 4 / 3 blocks per CU) and every tap is a
//     ds_read_b128; the halo costs 1.4 / 1.9 global reads per pixel and plane instead of 25;
//   wider strides (k_denoise_direct): the taps of a block's pixels share no cache lines (a row of
//     taps is `stride` pixels apart), a halo tile would be 3x the tile and more at stride 4, so
//     the taps are read from memory directly, guides only for valid taps.
// Both run the same tap sequence per pixel (row-major over dy, dx), so the results are the same
// bits; MCPT_DENOISE_LDS_MAX (0, 1 or 2: the widest stride that takes the LDS kernel) is an A/B knob.
//
// Every kernel here is one template over `Guided`.  The variance-guided form
// adds, under `if constexpr`, a float2 plane {variance of the pixel's mean luminance or -1, luminance}
// in ping-pong like the colour: 80 B of compulsory traffic per pixel and pass against 64 B.  A tap is
// then 56 B, so the LDS tiles are 36 x 20 x 56 B = 39.4 KiB (stride 1) and 40 x 24 x 56 B = 52.5 KiB
// (stride 2): still 4 / 3 blocks per CU of the 160 KiB, under the 64 KiB static limit.  Its 3 x 3
// variance prefilter is at stride 1 in every pass: in the LDS kernels its halo of 1 lies inside the
// 2-stride halo, in the direct kernel it is nine adjacent reads of the float2 plane.  An invalid
// pixel's variance is -1 by construction (dn_vl, dn_finish_vl's callers), so the prefilter needs the
// float2 plane only.  The reciprocal of the colour term is computed once per pixel.  The plain
// instantiations hold none of this: they take DenoiseArgs, and their tiles have no float2 array.
#include <type_traits>

#include "kernels.hpp"

#include "device/denoise.hpp"

namespace mcpt_dev {

using namespace mcpt;

constexpr int kDnTileW = 32, kDnTileH = 16;  // pixels per block; 256 threads, two rows each

template <bool Guided>
using DnArgs = std::conditional_t<Guided, DenoiseGuidedArgs, DenoiseArgs>;
template <bool Guided>
using DnPrepArgs = std::conditional_t<Guided, DenoiseGuidedPrepArgs, DenoisePrepArgs>;

template <bool Guided, int S>
__global__ __launch_bounds__(256) void k_denoise_lds(DnArgs<Guided> a) {
    constexpr int LW = kDnTileW + 4 * S, LH = kDnTileH + 4 * S;
    __shared__ float4 s_col[LW * LH];
    __shared__ float4 s_gd[LW * LH];
    __shared__ float4 s_al[LW * LH];
    __shared__ float2 s_vl[Guided ? LW * LH : 1];  // (never referenced, so not allocated, when plain)
    const int x0 = (int)blockIdx.x * kDnTileW, y0 = (int)blockIdx.y * kDnTileH;
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
            if constexpr (Guided) vl = a.v.vl[q];
        }
        s_col[i] = c;
        s_gd[i] = g;
        s_al[i] = al;
        if constexpr (Guided) s_vl[i] = vl;
    }
    __syncthreads();
    const int tx = (int)threadIdx.x % kDnTileW, ty0 = (int)threadIdx.x / kDnTileW;
    for (int ty = ty0; ty < kDnTileH; ty += 256 / kDnTileW) {
        const int x = x0 + tx, y = y0 + ty;
        if (x >= a.W || y >= a.H) continue;
        const int lp = (ty + 2 * S) * LW + tx + 2 * S;
        const float4 cp = s_col[lp];
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
        float2 ov = make_float2(-1.f, 0.f);
        if (cp.w != 0.f) {
            const float4 gp = s_gd[lp], ap = s_al[lp];
            float2 vlp = ov;
            bool known = false;
            float rcp = 0.f;
            if constexpr (Guided) {
                vlp = s_vl[lp];
                known = dn_known(vlp.x);
                if (known) {
                    DnPre pre{0.f, 0.f};
#pragma unroll
                    for (int dy = -1; dy <= 1; dy++)
#pragma unroll
                        for (int dx = -1; dx <= 1; dx++) {
                            const float vr = s_vl[lp + dy * LW + dx].x;
                            if (dn_known(vr)) dn_pre_tap(dx, dy, vr, pre);
                        }
                    rcp = dn_pre_rcp(a.v, pre);
                }
            }
            DnAcc acc{0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int dy = -2; dy <= 2; dy++)
#pragma unroll
                for (int dx = -2; dx <= 2; dx++) {
                    const int lq = lp + dy * S * LW + dx * S;
                    const float4 cq = s_col[lq];
                    if (cq.w == 0.f) continue;
                    if constexpr (Guided)
                        dn_tap_guided(a.k, dx, dy, known, rcp, cp, vlp, gp, ap, cq, s_vl[lq], s_gd[lq], s_al[lq], acc);
                    else dn_tap(a.k, dx, dy, cp, gp, ap, cq, s_gd[lq], s_al[lq], acc);
                }
            o = dn_finish(acc);
            if constexpr (Guided) ov = dn_finish_vl(acc, known, o);
        }
        const size_t p = (size_t)y * (size_t)a.W + (size_t)x;
        a.out[p] = o;
        if constexpr (Guided) a.v.out_vl[p] = ov;
    }
}

template <bool Guided>
__global__ __launch_bounds__(256) void k_denoise_direct(DnArgs<Guided> a) {
    const int x = (int)blockIdx.x * 64 + (int)threadIdx.x % 64, y = (int)blockIdx.y * 4 + (int)threadIdx.x / 64;
    if (x >= a.W || y >= a.H) return;
    const size_t p = (size_t)y * (size_t)a.W + (size_t)x;
    const float4 cp = a.col[p];
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    float2 ov = make_float2(-1.f, 0.f);
    if (cp.w != 0.f) {
        const float4 gp = a.gd[p], ap = a.al[p];
        float2 vlp = ov;
        bool known = false;
        float rcp = 0.f;
        if constexpr (Guided) {
            vlp = a.v.vl[p];
            known = dn_known(vlp.x);
            if (known) {
                // the nine reads at clamped coordinates, issued together; a neighbour outside the film counts as unknown
                float vr[9];
#pragma unroll
                for (int dy = -1; dy <= 1; dy++)
#pragma unroll
                    for (int dx = -1; dx <= 1; dx++) {
                        const int rx = x + dx, ry = y + dy;
                        const bool in = rx >= 0 && rx < a.W && ry >= 0 && ry < a.H;
                        const float v = a.v.vl[in ? (size_t)ry * (size_t)a.W + (size_t)rx : p].x;
                        vr[(dy + 1) * 3 + dx + 1] = in ? v : -1.f;
                    }
                DnPre pre{0.f, 0.f};
#pragma unroll
                for (int dy = -1; dy <= 1; dy++)
#pragma unroll
                    for (int dx = -1; dx <= 1; dx++)
                        if (dn_known(vr[(dy + 1) * 3 + dx + 1])) dn_pre_tap(dx, dy, vr[(dy + 1) * 3 + dx + 1], pre);
                rcp = dn_pre_rcp(a.v, pre);
            }
        }
        const int S = a.k.stride;
        DnAcc acc{0.f, 0.f, 0.f, 0.f, 0.f};
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
                if constexpr (Guided) dn_tap_guided(a.k, dx, dy, known, rcp, cp, vlp, gp, ap, cq, a.v.vl[q], a.gd[q], a.al[q], acc);
                else dn_tap(a.k, dx, dy, cp, gp, ap, cq, a.gd[q], a.al[q], acc);
            }
        }
        o = dn_finish(acc);
        if constexpr (Guided) ov = dn_finish_vl(acc, known, o);
    }
    a.out[p] = o;
    if constexpr (Guided) a.v.out_vl[p] = ov;
}

template <bool Guided>
static void launch_pass(const DnArgs<Guided>& a, int lds_max_stride, hipStream_t s) {
    const dim3 tg((unsigned)((a.W + kDnTileW - 1) / kDnTileW), (unsigned)((a.H + kDnTileH - 1) / kDnTileH));
    if (a.k.stride == 1 && lds_max_stride >= 1) hipLaunchKernelGGL((k_denoise_lds<Guided, 1>), tg, dim3(256), 0, s, a);
    else if (a.k.stride == 2 && lds_max_stride >= 2) hipLaunchKernelGGL((k_denoise_lds<Guided, 2>), tg, dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL(k_denoise_direct<Guided>, dim3((unsigned)((a.W + 63) / 64), (unsigned)((a.H + 3) / 4)), dim3(256), 0,
                           s, a);
}
void launch_denoise_pass(const DenoiseGuidedArgs& a, int lds_max_stride, hipStream_t s) {
    if (a.W <= 0 || a.H <= 0) return;
    if (a.v.vl) launch_pass<true>(a, lds_max_stride, s);
    else launch_pass<false>(a, lds_max_stride, s);
}

// The filter's planes from the film and the guide sums (mcpt_film_denoise): colour = Ld / samples
// per channel (k_tonemap's division), guides = sum / count; guided: variance = se se of the film's
// error plane
template <bool Guided>
__global__ void k_denoise_prep_film(DnPrepArgs<Guided> a) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const float4 L = a.Ld[i];
    const uint32_t ns = a.samples[i];
    const float s = (float)ns;
    const float4 ga = a.g_alb[i], gn = a.g_nz[i];
    const float cnt = ga.w;  // the guide sample count (exact: < 2^19)
    float4 col, gd, al;
    dn_planes(L.x / s, L.y / s, L.z / s, ns > 0, gn.x / cnt, gn.y / cnt, gn.z / cnt, gn.w / cnt, ga.x / cnt, ga.y / cnt,
              ga.z / cnt, col, gd, al);
    a.col[i] = col;
    a.gd[i] = gd;
    a.al[i] = al;
    if constexpr (Guided) {
        const float se = a.err ? a.err[i].x : -1.f;
        a.vl[i] = dn_vl(col, (se >= 0.f && dn_finite(se)) ? se * se : -1.f);
    }
}
// ... and from caller images of means (mcpt_denoise_run): rgb / normal / albedo 3 floats per pixel,
// depth 1, samples optional (nullptr: every pixel has samples); guided: a variance per pixel
template <bool Guided>
__global__ void k_denoise_prep_images(DnPrepArgs<Guided> a) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    float4 col, gd, al;
    dn_planes(a.rgb[3 * (size_t)i], a.rgb[3 * (size_t)i + 1], a.rgb[3 * (size_t)i + 2], a.samples ? a.samples[i] > 0 : true,
              a.normal[3 * (size_t)i], a.normal[3 * (size_t)i + 1], a.normal[3 * (size_t)i + 2], a.depth[i],
              a.albedo[3 * (size_t)i], a.albedo[3 * (size_t)i + 1], a.albedo[3 * (size_t)i + 2], col, gd, al);
    a.col[i] = col;
    a.gd[i] = gd;
    a.al[i] = al;
    if constexpr (Guided) a.vl[i] = dn_vl(col, a.variance ? a.variance[i] : -1.f);
}
template <bool Guided>
static void launch_prep(const DnPrepArgs<Guided>& a, hipStream_t s) {
    if (a.Ld) hipLaunchKernelGGL(k_denoise_prep_film<Guided>, dim3((a.n + 255) / 256), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(k_denoise_prep_images<Guided>, dim3((a.n + 255) / 256), dim3(256), 0, s, a);
}
void launch_denoise_prep(const DenoiseGuidedPrepArgs& a, hipStream_t s) {
    if (!a.n) return;
    if (a.vl) launch_prep<true>(a, s);
    else launch_prep<false>(a, s);
}

// ---- first-hit guides ----
// Rays of one chunk: ray (s - s0) * np + (p - p0) is film sample s of pixel p, the camera ray k_shade
// generates for it (the pixel's camera record + gen_ray_lens keyed by (seed, pixel, s); with a pinhole
// every sample's ray is the record's).  Pixels the renderer never renders (last column and row) get a
// zero direction, which the traversal resolves as a miss; k_guide_accum skips them.
__global__ void k_guide_rays(GuideArgs a) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.np * a.ns) return;
    const uint32_t pix = a.p0 + i % a.np, sidx = a.s0 + i / a.np;
    const int x = (int)(pix % (uint32_t)a.W), y = (int)(pix / (uint32_t)a.W);
    V3 o = v3(0.f, 0.f, 0.f), d = o;
    if (x < a.W - 1 && y < a.H - 1) {
        const float4 cp = a.cam_px[pix];
        o = v3(cp.x, cp.y, cp.z);
        if (a.cam.lens_radius > 0.f) {
            const Rng r0{rng_key(a.seed, pix, sidx), 0u};
            gen_ray_lens(a.cam, o, r0, o, d);
        } else {
            const float4 cd = a.cam_dir[pix];
            d = v3(cd.x, cd.y, cd.z);
        }
    }
    a.ro[i] = make_float4(o.x, o.y, o.z, 0.f);
    a.rd[i] = make_float4(d.x, d.y, d.z, 0.f);
}
// One thread per pixel adds the chunk's samples in ascending order (the chunks of a pixel arrive in
// ascending sample order too, so the sums do not depend on the chunking): albedo = the material's base
// colour, hit_record's normal and t; a miss adds albedo 1, normal 0, depth 0.
__global__ void k_guide_accum(GuideArgs a) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= a.np) return;
    const uint32_t pix = a.p0 + j;
    const int x = (int)(pix % (uint32_t)a.W), y = (int)(pix / (uint32_t)a.W);
    if (!(x < a.W - 1 && y < a.H - 1)) return;
    float4 ga = a.g_alb[pix], gn = a.g_nz[pix];
    for (uint32_t s = 0; s < a.ns; s++) {
        const size_t i = (size_t)s * a.np + j;
        const float4 hn = a.hit_n[i];
        const int mat = __float_as_int(hn.w);
        V3 al = v3(1.f, 1.f, 1.f), n = v3(0.f, 0.f, 0.f);
        float t = 0.f;
        if (mat >= 0) {
            const float* m = a.mats + 8 * (size_t)mat;
            al = v3(m[0], m[1], m[2]);
            n = v3(hn.x, hn.y, hn.z);
            t = a.hit_p[i].w;
        }
        ga = make_float4(ga.x + al.x, ga.y + al.y, ga.z + al.z, ga.w + 1.f);
        gn = make_float4(gn.x + n.x, gn.y + n.y, gn.z + n.z, gn.w + t);
    }
    a.g_alb[pix] = ga;
    a.g_nz[pix] = gn;
}
void launch_guide_rays(const GuideArgs& a, hipStream_t s) {
    const uint32_t n = a.np * a.ns;
    if (n) hipLaunchKernelGGL(k_guide_rays, dim3((n + 255) / 256), dim3(256), 0, s, a);
}
void launch_guide_accum(const GuideArgs& a, hipStream_t s) {
    if (a.np) hipLaunchKernelGGL(k_guide_accum, dim3((a.np + 255) / 256), dim3(256), 0, s, a);
}

}  // namespace mcpt_dev
