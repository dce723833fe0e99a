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
// Row 0 of a texture is v in [0, 1 / H): glTF's orientation, no flip.  Texels are used as stored
// (the reference's texture objects have no sRGB decode) unless the texture is flagged MCPT_TEX_SRGB and read
// as a base colour (section 22, below).  Alpha is ignored.
//
// Metallic-roughness textures (tex_mr below) use the same tc and the same lookup:
//   T     = tex_bilinear_rgba8(MR texture of the material, tc)     over rgb, unchanged
//   rough = fmx(rough_factor * T.y, BRDF_EPS)   one fp32 multiply, then load_mat's clamp (G channel)
//   metal = metal_factor * T.z                  one fp32 multiply (B channel)
// rough_factor is the raw mat_params[6], not load_mat's clamped value.  R and A are ignored.  The two
// textures of a material are independent: either, both or none, of any two sizes.
//
// Normal-map textures (tex_nrm_coeffs and tex_nrm_vertex below) perturb the three
// vertex normals N_i of the hit's record before the hit record interpolates them, with the record's vertex
// tangents (T_i, s_i), i = 0, 1, 2, at the same tc and through the same lookup.  All fp32, this order:
//   t   = tex_bilinear_rgba8(normal texture of the material, tc)     over rgb, unchanged
//   c.x = (2 * t.x - 1) * scale    c.y = (2 * t.y - 1) * scale    c.z = 2 * t.z - 1     (glTF: z is "up")
//   B_i = cross(N_i, T_i) * s_i                                       glTF's bitangent
//   m_i = (T_i * c.x + B_i * c.y) + N_i * c.z                         per vertex
//   nrm = normalize(normalize((m_1 * u + m_2 * v) + m_0 * w))         the hit record's own two lines, on m_i
// Interpolation is linear, so this is the usual perturbation of the interpolated frame.  glTF's inner
// normalize(c) is left out: a common positive scalar that the hit record's normalisation removes.  A
// material without a normal texture keeps m_i = N_i by selection, not by arithmetic.  Texels are used as
// stored; alpha is ignored.  nrm stands for the hit record's normal everywhere the material stage reads it
// (frames, f and pdf, the emitter sample, the ray origins' offsets): there is no separate geometric normal.
//
// sRGB base colour (srgb_to_linear, tex_bilinear_rgba8_srgb and tex_base_srgb below): a
// base-colour lookup of a texture flagged MCPT_TEX_SRGB is tex_bilinear_rgba8's arithmetic with
//   texel = L[c]                                  in place of c / 255
// L the 256 floats of device/srgb_table.hpp: decode before the filter (the glTF rule).  MR and normal lookups
// never decode, whatever the texture's flag.  Alpha is ignored.
#pragma once
#include "device/mcpt_core.hpp"

namespace mcpt {

// What the textured kernels see of an installed set (mcpt_set_material_textures); uv == nullptr: none.
struct TexView {
    const float2* uv;       // 3 per triangle record (uv0, uv1, uv2), in record order like DevScene::tri_sh
    const uint32_t* atlas;  // every texture's RGBA8 texels (r in the low byte), row-major, one after the other
    const int4* mat;        // per material {first texel in the atlas, w, h, texture index}; w == 0: untextured
    // (section 22) the fourth word of a base-colour entry also carries kTexEntrySrgb for a texture flagged
    // MCPT_TEX_SRGB; only the sRGB kernels read it, and only a set with such a material launches those.
    // Metallic-roughness entries (section 20) live in the same allocation, in front of the base-colour
    // ones and mirrored: material m's is mat[-1 - m], the same four words.  Only k_material's MR
    // instantiations read them, and only a set with an MR-textured material launches those.
    // Normal maps (section 21) add no field either.  The tangent stream, three float4 {T.xyz, s} per
    // record in record order, lies behind the uv stream in its allocation, at uv + tex_tan_offset(ntri)
    // (ntri: DevScene::ntri).  Material m's normal entry {first texel, w, h, scale bits} lies in front of
    // the atlas in its allocation, mirrored: ((const int4*)atlas)[-1 - m]; w == 0: no normal map.  Only the
    // normal-map kernels read either, and only a set with a normal-mapped material launches those.
};
// The tangent stream's place behind the 3 ntri float2 of the uv stream, in float2 units (16-byte aligned)
MCPT_HD size_t tex_tan_offset(uint32_t ntri) { return (3 * (size_t)ntri + 1) & ~(size_t)1; }

// c / 255 rounded to nearest fp32, c = 0..255.  The fp64 product is within 2^-52 of the quotient,
// and no quotient k / 255 lies that close to the midpoint of two floats (255 = 2^8 - 1: the
// expansion repeats with period 8), so the second rounding gives the quotient's own;
// tests/test_texture_host.py compares all 256 with numpy's float32 division.
MCPT_HD float unorm8(uint32_t c) { return (float)((double)c * (1.0 / 255.0)); }
MCPT_HD V3 rgb8(uint32_t t) { return v3(unorm8(t & 255u), unorm8((t >> 8) & 255u), unorm8((t >> 16) & 255u)); }

// L[c], c = 0..255 (section 22): the linear value of the sRGB-encoded byte c, a literal table (one 4-byte
// load per channel through the vector cache on the device; the table is 1 KiB)
MCPT_HD float srgb_to_linear(uint32_t c) {
    static constexpr float L[256] = {
#include "device/srgb_table.hpp"
    };
    return L[c & 255u];
}
// A texel's rgb: L[c] per channel where `srgb`, else rgb8 (selection per texel, after one gather)
MCPT_HD V3 rgb8_srgb(uint32_t t, bool srgb) {
    if (!srgb) return rgb8(t);
    return v3(srgb_to_linear(t & 255u), srgb_to_linear((t >> 8) & 255u), srgb_to_linear((t >> 16) & 255u));
}

// tex_bilinear (mcpt_core.hpp) over a W x H RGBA8 image: the same statements with the texel decode in
// place of the float4 fetch.  Four 4-byte gathers; W, H in 1..16384, so every index fits an int.
// SRGB: the decode is rgb8_srgb(c, srgb) (section 22); without it `srgb` is not read.
template <bool SRGB>
MCPT_HD V3 tex_bilinear_rgba8_t(const uint32_t* tex, int W, int H, float u, float v, [[maybe_unused]] bool srgb) {
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
    V3 t00, t10, t01, t11;
    if constexpr (SRGB) {
        t00 = rgb8_srgb(c00, srgb), t10 = rgb8_srgb(c10, srgb), t01 = rgb8_srgb(c01, srgb), t11 = rgb8_srgb(c11, srgb);
    } else {
        t00 = rgb8(c00), t10 = rgb8(c10), t01 = rgb8(c01), t11 = rgb8(c11);
    }
    float bx = 1.f - ax, by = 1.f - ay;
    float w00 = bx * by, w10 = ax * by, w01 = bx * ay, w11 = ax * ay;
    V3 o;
    o.x = ((w00 * t00.x + w10 * t10.x) + w01 * t01.x) + w11 * t11.x;
    o.y = ((w00 * t00.y + w10 * t10.y) + w01 * t01.y) + w11 * t11.y;
    o.z = ((w00 * t00.z + w10 * t10.z) + w01 * t01.z) + w11 * t11.z;
    return o;
}
MCPT_HD V3 tex_bilinear_rgba8(const uint32_t* tex, int W, int H, float u, float v) {
    return tex_bilinear_rgba8_t<false>(tex, W, H, u, v, false);
}
MCPT_HD V3 tex_bilinear_rgba8_srgb(const uint32_t* tex, int W, int H, float u, float v, bool srgb) {
    return tex_bilinear_rgba8_t<true>(tex, W, H, u, v, srgb);
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
// tex_base under a set with an sRGB-flagged base-colour texture (section 22): the flag rides in the entry's
// fourth word, which holds the texture index (below 2^30) and which no other lookup reads
constexpr int kTexEntrySrgb = 1 << 30;
MCPT_HD V3 tex_base_srgb(const TexView& t, int mat, V3 base_factor, float tu, float tv) {
    const int4 e = t.mat[mat];
    if (e.y <= 0) return base_factor;
    return base_factor * tex_bilinear_rgba8_srgb(t.atlas + e.x, e.y, e.z, tu, tv, (e.w & kTexEntrySrgb) != 0);
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

// The tangent-space coefficients c of material `mat` at (tu, tv) from its normal texture (section 21, the
// head of this file); false for a material without one (the caller then keeps N_i: selection).
MCPT_HD bool tex_nrm_coeffs(const TexView& t, int mat, float tu, float tv, V3& c) {
    const int4 e = reinterpret_cast<const int4*>(t.atlas)[-1 - mat];
    if (e.y <= 0) return false;
    const V3 T = tex_bilinear_rgba8(t.atlas + e.x, e.y, e.z, tu, tv);
    const float scale = __builtin_bit_cast(float, e.w);
    c.x = (2.f * T.x - 1.f) * scale;
    c.y = (2.f * T.y - 1.f) * scale;
    c.z = 2.f * T.z - 1.f;
    return true;
}
// m_i of one vertex: normal N, tangent T with handedness s, coefficients c
MCPT_HD V3 tex_nrm_vertex(V3 N, V3 T, float s, V3 c) {
    const V3 B = cross(N, T) * s;
    return (T * c.x + B * c.y) + N * c.z;
}

}  // namespace mcpt
