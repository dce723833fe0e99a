// texture.hpp -- base-colour textures: the arithmetic the textured
// instantiations of k_material and the guide pass, the host-image sampler (mcpt_texture_sample_run)
// and tests/texture_ref.py share.  Host and device, like mcpt_core.hpp.
//
//   tc    = (u * uv1 + v * uv2) + w * uv0        per component, fp32, this order (Triangle.cu:79)
//   texel = (float)c / 255.0f                     correctly rounded (cudaReadModeNormalizedFloat)
//   T     = tex_bilinear's arithmetic over the rgb of four RGBA8 texels: wrap addressing, 8-bit
//           fractional weights, the sum order, a coordinate that is NaN or >= 65536 in magnitude
//           counts as 0 (mcpt_core.hpp; dTexture.cu:107-117)
//   base  = base_factor * T                       one fp32 multiply per channel (the glTF rule)
//
// Row 0 of a texture is v in [0, 1 / H): glTF's orientation, no flip.  Texels are used as stored:
// no sRGB decode (the reference's texture objects have none).  Alpha is ignored.
//
// Metallic-roughness textures (tex_mr below) use the same tc and the same lookup:
//   T     = tex_bilinear_rgba8(MR texture of the material, tc)     over rgb, unchanged
//   rough = fmx(rough_factor * T.y, BRDF_EPS)   one fp32 multiply, then load_mat's clamp (G channel)
//   metal = metal_factor * T.z                  one fp32 multiply (B channel)
// rough_factor is the raw mat_params[6], not load_mat's clamped value.  R and A are ignored.  The two
// textures of a material are independent: either, both or none, of any two sizes.
#pragma once
#include "device/mcpt_core.hpp"

namespace mcpt {

// What the textured kernels see of an installed set (mcpt_set_material_textures); uv == nullptr: none.
struct TexView {
    const float2* uv;       // 3 per triangle record (uv0, uv1, uv2), in record order like DevScene::tri_sh
    const uint32_t* atlas;  // every texture's RGBA8 texels (r in the low byte), row-major, one after the other
    const int4* mat;        // per material {first texel in the atlas, w, h, texture index}; w == 0: untextured
    // Metallic-roughness entries (section 20) live in the same allocation, in front of the base-colour
    // ones and mirrored: material m's is mat[-1 - m], the same four words.  Only k_material's MR
    // instantiations read them, and only a set with an MR-textured material launches those.
};

// c / 255 rounded to nearest fp32, c = 0..255.  The fp64 product is within 2^-52 of the quotient,
// and no quotient k / 255 lies that close to the midpoint of two floats (255 = 2^8 - 1: the
// expansion repeats with period 8), so the second rounding gives the quotient's own;
// tests/test_texture_host.py compares all 256 with numpy's float32 division.
MCPT_HD float unorm8(uint32_t c) { return (float)((double)c * (1.0 / 255.0)); }
MCPT_HD V3 rgb8(uint32_t t) { return v3(unorm8(t & 255u), unorm8((t >> 8) & 255u), unorm8((t >> 16) & 255u)); }

// tex_bilinear (mcpt_core.hpp) over a W x H RGBA8 image: the same statements with the texel decode in
// place of the float4 fetch.  Four 4-byte gathers; W, H in 1..16384, so every index fits an int.
MCPT_HD V3 tex_bilinear_rgba8(const uint32_t* tex, int W, int H, float u, float v) {
    if (!(__builtin_fabsf(u) < 65536.f)) u = 0.f;
    if (!(__builtin_fabsf(v) < 65536.f)) v = 0.f;
    float x = u * (float)W - 0.5f;
    float y = v * (float)H - 0.5f;
    float fx = __builtin_floorf(x), fy = __builtin_floorf(y);
    float ax = q8(x - fx), ay = q8(y - fy);
    int i0 = wrapi((int)fx, W), i1 = wrapi((int)fx + 1, W);
    int j0 = wrapi((int)fy, H), j1 = wrapi((int)fy + 1, H);
    const uint32_t c00 = tex[j0 * W + i0], c10 = tex[j0 * W + i1];
    const uint32_t c01 = tex[j1 * W + i0], c11 = tex[j1 * W + i1];
    const V3 t00 = rgb8(c00), t10 = rgb8(c10), t01 = rgb8(c01), t11 = rgb8(c11);
    float bx = 1.f - ax, by = 1.f - ay;
    float w00 = bx * by, w10 = ax * by, w01 = bx * ay, w11 = ax * ay;
    V3 o;
    o.x = ((w00 * t00.x + w10 * t10.x) + w01 * t01.x) + w11 * t11.x;
    o.y = ((w00 * t00.y + w10 * t10.y) + w01 * t01.y) + w11 * t11.y;
    o.z = ((w00 * t00.z + w10 * t10.z) + w01 * t01.z) + w11 * t11.z;
    return o;
}

// The texture coordinate of a hit with Moller-Trumbore u, v and w = (1 - u) - v, one component
MCPT_HD float tex_coord(float u, float v, float w, float c0, float c1, float c2) { return (u * c1 + v * c2) + w * c0; }

// The shaded base colour of material `mat` at texture coordinate (tu, tv): base_factor * T, or
// base_factor itself for an untextured material
MCPT_HD V3 tex_base(const TexView& t, int mat, V3 base_factor, float tu, float tv) {
    const int4 e = t.mat[mat];
    if (e.y <= 0) return base_factor;
    return base_factor * tex_bilinear_rgba8(t.atlas + e.x, e.y, e.z, tu, tv);
}

// The shaded roughness and metallic of material `mat` at (tu, tv): (rough_factor, metal_factor) times the
// G and B channels of its MR texture, the roughness clamped as load_mat clamps it; the clamped factor and
// the metallic factor for a material without one.  rough_factor is the raw mat_params[6].
MCPT_HD void tex_mr(const TexView& t, int mat, float rough_factor, float metal_factor, float tu, float tv, float& rough,
                    float& metal) {
    const int4 e = t.mat[-1 - mat];
    rough = fmx(rough_factor, BRDF_EPS);
    metal = metal_factor;
    if (e.y <= 0) return;
    const V3 T = tex_bilinear_rgba8(t.atlas + e.x, e.y, e.z, tu, tv);
    rough = fmx(rough_factor * T.y, BRDF_EPS);
    metal = metal_factor * T.z;
}

}  // namespace mcpt
