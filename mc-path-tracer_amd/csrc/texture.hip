// texture.hip -- base-colour textures: the kernels beside k_material's textured
// instantiations (kernels.hip).  The arithmetic is device/texture.hpp's.
//   k_tex_sample       the lookup alone over caller uv pairs (mcpt_texture_sample_run)
//   k_tex_uv_records   the per-triangle uv stream in record order (install, MCPT_GEOM_REBUILD)
//   k_guide_accum_tex  the guide pass's accumulation with the textured albedo
// Normal maps:
//   k_tex_tangent_records  the per-triangle tangent stream in record order, beside k_tex_uv_records
//   k_guide_accum_nrm      k_guide_accum_tex with the mapped normal as the normal guide
// sRGB base colour:
//   k_tex_sample_srgb      k_tex_sample with the texels decoded through the table
//   k_guide_accum_srgb     k_guide_accum_nrm with the decoded base colour as the albedo guide
#include "device/scene_dev.hpp"

namespace mcpt_dev {

__global__ __launch_bounds__(256) void k_tex_sample(const uint32_t* tex, int w, int h, const float2* uv, float* out,
                                                    uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float2 c = uv[i];
    const V3 t = mcpt::tex_bilinear_rgba8(tex, w, h, c.x, c.y);
    out[3 * (size_t)i + 0] = t.x;
    out[3 * (size_t)i + 1] = t.y;
    out[3 * (size_t)i + 2] = t.z;
}
void launch_tex_sample(const uint32_t* tex, int w, int h, const float2* uv, float* out_rgb, uint32_t n, hipStream_t s) {
    if (n) hipLaunchKernelGGL(k_tex_sample, dim3((n + 255u) / 256u), dim3(256), 0, s, tex, w, h, uv, out_rgb, n);
}

__global__ __launch_bounds__(256) void k_tex_uv_records(const float2* uv0, const float2* uv1, const float2* uv2,
                                                        const uint32_t* order, float2* out, uint32_t ntri) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= ntri) return;
    uint32_t t = order ? order[p] : p;
    if (t >= ntri) t = p;  // (an order array is a permutation of 0 .. ntri - 1: never taken)
    out[3 * (size_t)p + 0] = uv0[t];
    out[3 * (size_t)p + 1] = uv1[t];
    out[3 * (size_t)p + 2] = uv2[t];
}
void launch_tex_uv_records(const float2* uv0, const float2* uv1, const float2* uv2, const uint32_t* order, float2* out,
                           uint32_t ntri, hipStream_t s) {
    if (ntri) hipLaunchKernelGGL(k_tex_uv_records, dim3((ntri + 255u) / 256u), dim3(256), 0, s, uv0, uv1, uv2, order, out, ntri);
}

__global__ __launch_bounds__(256) void k_tex_tangent_records(const float4* tan0, const float4* tan1, const float4* tan2,
                                                             const uint32_t* order, float4* out, uint32_t ntri) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= ntri) return;
    uint32_t t = order ? order[p] : p;
    if (t >= ntri) t = p;  // (an order array is a permutation of 0 .. ntri - 1: never taken)
    out[3 * (size_t)p + 0] = tan0[t];
    out[3 * (size_t)p + 1] = tan1[t];
    out[3 * (size_t)p + 2] = tan2[t];
}
void launch_tex_tangent_records(const float4* tan0, const float4* tan1, const float4* tan2, const uint32_t* order, float4* out,
                                uint32_t ntri, hipStream_t s) {
    if (ntri)
        hipLaunchKernelGGL(k_tex_tangent_records, dim3((ntri + 255u) / 256u), dim3(256), 0, s, tan0, tan1, tan2, order, out, ntri);
}

// k_guide_accum (denoise.hip) with the hit record rebuilt here, so that the texture coordinate is at
// hand: one thread per pixel adds the chunk's samples in ascending order; a miss adds albedo 1, normal
// 0, depth 0.
__global__ __launch_bounds__(256) void k_guide_accum_tex(GuideTexArgs b) {
    const GuideArgs& a = b.g;
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= a.np) return;
    const uint32_t pix = a.p0 + j;
    const int x = (int)(pix % (uint32_t)a.W), y = (int)(pix / (uint32_t)a.W);
    if (!(x < a.W - 1 && y < a.H - 1)) return;
    float4 ga = a.g_alb[pix], gn = a.g_nz[pix];
    for (uint32_t s = 0; s < a.ns; s++) {
        const size_t i = (size_t)s * a.np + j;
        const int tri = b.rec[i];
        V3 al = v3(1.f, 1.f, 1.f), n = v3(0.f, 0.f, 0.f);
        float t = 0.f;
        if (tri >= 0 && (uint32_t)tri < b.scene.ntri) {
            V3 pos;
            int mat;
            float tu, tv;
            hit_record_t<true>(b.scene, b.tex.uv, xyz(a.ro[i]), xyz(a.rd[i]), tri, pos, n, mat, t, tu, tv);
            const float* m = a.mats + 8 * (size_t)mat;
            al = mcpt::tex_base(b.tex, mat, v3(m[0], m[1], m[2]), tu, tv);
        }
        ga = make_float4(ga.x + al.x, ga.y + al.y, ga.z + al.z, ga.w + 1.f);
        gn = make_float4(gn.x + n.x, gn.y + n.y, gn.z + n.z, gn.w + t);
    }
    a.g_alb[pix] = ga;
    a.g_nz[pix] = gn;
}
void launch_guide_accum_tex(const GuideTexArgs& a, hipStream_t s) {
    if (a.g.np) hipLaunchKernelGGL(k_guide_accum_tex, dim3((a.g.np + 255) / 256), dim3(256), 0, s, a);
}

// k_guide_accum_tex under a normal-mapped set (section 21): the hit record is hit_record_n, so the normal
// guide accumulates the mapped normal and the denoiser's edge stop sees the mapped detail.  Albedo, depth
// and count as k_guide_accum_tex.
__global__ __launch_bounds__(256) void k_guide_accum_nrm(GuideTexArgs b) {
    const GuideArgs& a = b.g;
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= a.np) return;
    const uint32_t pix = a.p0 + j;
    const int x = (int)(pix % (uint32_t)a.W), y = (int)(pix / (uint32_t)a.W);
    if (!(x < a.W - 1 && y < a.H - 1)) return;
    float4 ga = a.g_alb[pix], gn = a.g_nz[pix];
    for (uint32_t s = 0; s < a.ns; s++) {
        const size_t i = (size_t)s * a.np + j;
        const int tri = b.rec[i];
        V3 al = v3(1.f, 1.f, 1.f), n = v3(0.f, 0.f, 0.f);
        float t = 0.f;
        if (tri >= 0 && (uint32_t)tri < b.scene.ntri) {
            V3 pos;
            int mat;
            float tu, tv;
            hit_record_n(b.scene, b.tex, xyz(a.ro[i]), xyz(a.rd[i]), tri, pos, n, mat, t, tu, tv);
            const float* m = a.mats + 8 * (size_t)mat;
            al = mcpt::tex_base(b.tex, mat, v3(m[0], m[1], m[2]), tu, tv);
        }
        ga = make_float4(ga.x + al.x, ga.y + al.y, ga.z + al.z, ga.w + 1.f);
        gn = make_float4(gn.x + n.x, gn.y + n.y, gn.z + n.z, gn.w + t);
    }
    a.g_alb[pix] = ga;
    a.g_nz[pix] = gn;
}
void launch_guide_accum_nrm(const GuideTexArgs& a, hipStream_t s) {
    if (a.g.np) hipLaunchKernelGGL(k_guide_accum_nrm, dim3((a.g.np + 255) / 256), dim3(256), 0, s, a);
}

// The lookup alone with every texel decoded through the sRGB table (section 22)
__global__ __launch_bounds__(256) void k_tex_sample_srgb(const uint32_t* tex, int w, int h, const float2* uv, float* out,
                                                         uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float2 c = uv[i];
    const V3 t = mcpt::tex_bilinear_rgba8_srgb(tex, w, h, c.x, c.y, true);
    out[3 * (size_t)i + 0] = t.x;
    out[3 * (size_t)i + 1] = t.y;
    out[3 * (size_t)i + 2] = t.z;
}
void launch_tex_sample_srgb(const uint32_t* tex, int w, int h, const float2* uv, float* out_rgb, uint32_t n, hipStream_t s) {
    if (n) hipLaunchKernelGGL(k_tex_sample_srgb, dim3((n + 255u) / 256u), dim3(256), 0, s, tex, w, h, uv, out_rgb, n);
}

// k_guide_accum_nrm under a set with an sRGB-flagged base-colour texture (section 22): the albedo guide
// accumulates the colour k_material<TexSrgb, ...> shades with.  The hit record is hit_record_n as at level 4 (a
// material without a normal map keeps its normals by selection); normal, depth and count as k_guide_accum_nrm.
__global__ __launch_bounds__(256) void k_guide_accum_srgb(GuideTexArgs b) {
    const GuideArgs& a = b.g;
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= a.np) return;
    const uint32_t pix = a.p0 + j;
    const int x = (int)(pix % (uint32_t)a.W), y = (int)(pix / (uint32_t)a.W);
    if (!(x < a.W - 1 && y < a.H - 1)) return;
    float4 ga = a.g_alb[pix], gn = a.g_nz[pix];
    for (uint32_t s = 0; s < a.ns; s++) {
        const size_t i = (size_t)s * a.np + j;
        const int tri = b.rec[i];
        V3 al = v3(1.f, 1.f, 1.f), n = v3(0.f, 0.f, 0.f);
        float t = 0.f;
        if (tri >= 0 && (uint32_t)tri < b.scene.ntri) {
            V3 pos;
            int mat;
            float tu, tv;
            hit_record_n(b.scene, b.tex, xyz(a.ro[i]), xyz(a.rd[i]), tri, pos, n, mat, t, tu, tv);
            const float* m = a.mats + 8 * (size_t)mat;
            al = mcpt::tex_base_srgb(b.tex, mat, v3(m[0], m[1], m[2]), tu, tv);
        }
        ga = make_float4(ga.x + al.x, ga.y + al.y, ga.z + al.z, ga.w + 1.f);
        gn = make_float4(gn.x + n.x, gn.y + n.y, gn.z + n.z, gn.w + t);
    }
    a.g_alb[pix] = ga;
    a.g_nz[pix] = gn;
}
void launch_guide_accum_srgb(const GuideTexArgs& a, hipStream_t s) {
    if (a.g.np) hipLaunchKernelGGL(k_guide_accum_srgb, dim3((a.g.np + 255) / 256), dim3(256), 0, s, a);
}

}  // namespace mcpt_dev
