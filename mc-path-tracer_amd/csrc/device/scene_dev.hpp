// scene_dev.hpp -- the device helpers that more than one of kernels.hip (the wavefront iteration),
// scene_tables.hip (tables built at upload, camera change or film resize) and film.hip (film and
// debug utilities) uses.  A helper with one user stays in that user's file.  Device code only: the
// host models of occ_coords (tests/native/occ_beam.cpp, tools/occ_list_model.cpp) keep copies.
#pragma once
#include "device/mcpt_core.hpp"
#include "device/texture.hpp"
#include "kernels.hpp"

namespace mcpt_dev {

using mcpt::V3;
using mcpt::v3;

__device__ inline V3 xyz(float4 a) { return v3(a.x, a.y, a.z); }
// the xyz of a float4 element with one dwordx3 load (one VGPR fewer than the float4)
__device__ inline V3 ld3f4(const float4* p) {
    const float* f = reinterpret_cast<const float*>(p);
    return v3(f[0], f[1], f[2]);
}
__device__ inline float4 f4(V3 v, float w) { return make_float4(v.x, v.y, v.z, w); }

#ifndef MCPT_OCC_LAYOUT
#define MCPT_OCC_LAYOUT 0  // occluder-table key order (occ_index): 0 origin-cell major, 1 direction-bin major
#endif
constexpr int kEnd = -1;  // not a valid leaf: offset + count <= ntri < 2^24

// Hit record of ray (o, d) on triangle tri, as dTriangle::hit builds it
// (Triangle.cu:66-92): Moller-Trumbore t/u/v, the interpolated normal
// normalised twice (identity transform), position o + t d, material id.
// TEX (base-colour textures): also the hit's texture coordinate (tu, tv) from the
// record's three uvs (uvs: TexView::uv), fetched with the other loads.
template <bool TEX>
__device__ inline void hit_record_t(const DevScene& sc, const float2* uvs, V3 o, V3 d, int tri, V3& pos, V3& nrm, int& mat,
                                    float& t_out, float& tu, float& tv) {
    const float4* tp = sc.tri + kTriF4 * tri;
    const float4 w0 = tp[0], w1 = tp[1], w2 = tp[2];
    const float4* sp4 = sc.tri_sh + 3 * tri;
    const float4 s0 = sp4[0], s1 = sp4[1], s2 = sp4[2];
    [[maybe_unused]] float2 c0, c1, c2;
    if constexpr (TEX) {
        const float2* up = uvs + 3 * (size_t)tri;
        c0 = up[0], c1 = up[1], c2 = up[2];
        __asm__ volatile("" ::"v"(c0.x), "v"(c0.y), "v"(c1.x), "v"(c1.y), "v"(c2.x), "v"(c2.y));
    }
    // All six loads in one round trip: the compiler otherwise issues the vertex load after
    // the determinant test and the shading record after the whole test (three serialised
    // fetches; the hit is known to exist, so every value is used).
    __asm__ volatile("" ::"v"(w0.x), "v"(w0.y), "v"(w0.z), "v"(w0.w), "v"(w1.x), "v"(w1.y), "v"(w1.z), "v"(w1.w),
                     "v"(w2.x), "v"(s0.x), "v"(s0.y), "v"(s0.z), "v"(s0.w), "v"(s1.x), "v"(s1.y), "v"(s1.z),
                     "v"(s1.w), "v"(s2.x), "v"(s2.y));
    float t, u, v;
    tri_test(o, d, v3(w0.x, w0.y, w0.z), v3(w0.w, w1.x, w1.y), v3(w1.z, w1.w, w2.x), t, u, v);
    const V3 n0 = v3(s0.x, s0.y, s0.z), n1 = v3(s0.w, s1.x, s1.y), n2 = v3(s1.z, s1.w, s2.x);
    const float w = (1.f - u) - v;
    nrm = normalize((n1 * u + n2 * v) + n0 * w);  // Triangle.cu:76
    nrm = normalize(nrm);                          // identity transform, :82
    pos = o + d * t;                               // :86
    mat = __float_as_int(s2.y);                    // material id bits
    t_out = t;
    if constexpr (TEX) {
        tu = mcpt::tex_coord(u, v, w, c0.x, c1.x, c2.x);  // Triangle.cu:79
        tv = mcpt::tex_coord(u, v, w, c0.y, c1.y, c2.y);
    }
}
// hit_record_t<true> under normal maps (device/texture.hpp): the material's normal
// texture is looked up at the hit's texture coordinate, the three vertex normals are perturbed with the
// record's vertex tangents (a material without a normal map keeps them: selection), and the hit record's own
// two normalisation lines run on the result.
// Registers decide the order of the loads.  k_material's sampling instantiations sit at the 128 VGPRs of four
// waves per SIMD, and whatever this function holds across the lookup's two dependent fetches (the material's
// entry, then four gathers) comes on top of what the kernel holds across the function.  With the nine normal
// words or the twelve tangent words held there, however the tangent loads were placed (with the record's
// other loads, behind the triangle test, behind the lookup), those instantiations spilled 6 VGPRs.  So the
// first round trip fetches the vertices, the uvs and the material id only, and a second one behind the lookup
// fetches the normals, from lines the first has just brought in, and the tangents together.
__device__ inline void hit_record_n(const DevScene& sc, const mcpt::TexView& tex, V3 o, V3 d, int tri, V3& pos, V3& nrm,
                                    int& mat, float& t_out, float& tu, float& tv) {
    const float4* tp = sc.tri + kTriF4 * tri;
    const float4 w0 = tp[0], w1 = tp[1], w2 = tp[2];
    const float4* sp4 = sc.tri_sh + 3 * tri;
    const float mat_bits = reinterpret_cast<const float*>(sp4)[9];  // (n2.z, mat, -, -): the material id
    const float2* up = tex.uv + 3 * (size_t)tri;
    const float2 c0 = up[0], c1 = up[1], c2 = up[2];
    __asm__ volatile("" ::"v"(c0.x), "v"(c0.y), "v"(c1.x), "v"(c1.y), "v"(c2.x), "v"(c2.y));
    __asm__ volatile("" ::"v"(w0.x), "v"(w0.y), "v"(w0.z), "v"(w0.w), "v"(w1.x), "v"(w1.y), "v"(w1.z), "v"(w1.w),
                     "v"(w2.x), "v"(mat_bits));
    float t, u, v;
    tri_test(o, d, v3(w0.x, w0.y, w0.z), v3(w0.w, w1.x, w1.y), v3(w1.z, w1.w, w2.x), t, u, v);
    const float w = (1.f - u) - v;
    mat = __float_as_int(mat_bits);
    tu = mcpt::tex_coord(u, v, w, c0.x, c1.x, c2.x);  // Triangle.cu:79
    tv = mcpt::tex_coord(u, v, w, c0.y, c1.y, c2.y);
    V3 c = v3(0.f, 0.f, 0.f);
    const bool mapped = mcpt::tex_nrm_coeffs(tex, mat, tu, tv, c);
    int tri2 = tri;
    __asm__ volatile("" : "+v"(tri2) : "v"(c.x), "v"(c.y), "v"(c.z));  // the second round trip waits for the lookup
    const float4* sq4 = sc.tri_sh + 3 * tri2;
    const float4 s0 = sq4[0], s1 = sq4[1];
    const float s2x = reinterpret_cast<const float*>(sq4)[8];
    V3 n0 = v3(s0.x, s0.y, s0.z), n1 = v3(s0.w, s1.x, s1.y), n2 = v3(s1.z, s1.w, s2x);
    if (mapped) {
        const float4* gp = reinterpret_cast<const float4*>(tex.uv + mcpt::tex_tan_offset(sc.ntri)) + 3 * (size_t)tri2;
        const float4 g0 = gp[0], g1 = gp[1], g2 = gp[2];
        n0 = mcpt::tex_nrm_vertex(n0, xyz(g0), g0.w, c);
        n1 = mcpt::tex_nrm_vertex(n1, xyz(g1), g1.w, c);
        n2 = mcpt::tex_nrm_vertex(n2, xyz(g2), g2.w, c);
    }
    nrm = normalize((n1 * u + n2 * v) + n0 * w);  // Triangle.cu:76, on m_i
    nrm = normalize(nrm);                          // identity transform, :82
    pos = o + d * t;                               // :86
    t_out = t;
}
__device__ inline void hit_record(const DevScene& sc, V3 o, V3 d, int tri, V3& pos, V3& nrm, int& mat, float& t_out) {
    float tu, tv;
    hit_record_t<false>(sc, nullptr, o, d, tri, pos, nrm, mat, t_out, tu, tv);
}

// The occluder table's key of a ray (the cache itself: kernels.hip).  Here, with the knob, because
// k_occ_probes and k_occ_complete (scene_tables.hip) decode a key by the inverse of occ_index.
// (cx, cy, cz): the origin cell; dirbin = (face B + ub) B + vb: the direction bin
__device__ inline void occ_coords(const DevScene& sc, V3 o, V3 d, uint32_t& cx, uint32_t& cy, uint32_t& cz, uint32_t& face,
                                  uint32_t& ub, uint32_t& vb) {
    const float gm = (float)(sc.occ_g - 1), bm = (float)(sc.occ_b - 1), hb = 0.5f * (float)sc.occ_b;
    // fmaxf(NaN, 0) = 0: a NaN coordinate falls in cell / bin 0
    cx = (uint32_t)__builtin_fminf(__builtin_fmaxf((o.x - sc.root_mn[0]) * sc.occ_inv[0], 0.f), gm);
    cy = (uint32_t)__builtin_fminf(__builtin_fmaxf((o.y - sc.root_mn[1]) * sc.occ_inv[1], 0.f), gm);
    cz = (uint32_t)__builtin_fminf(__builtin_fmaxf((o.z - sc.root_mn[2]) * sc.occ_inv[2], 0.f), gm);
    const float ax = __builtin_fabsf(d.x), ay = __builtin_fabsf(d.y), az = __builtin_fabsf(d.z);
    float u, v, m;
    if (ax >= ay && ax >= az) {
        face = d.x < 0.f ? 1u : 0u; u = d.y; v = d.z; m = ax;
    } else if (ay >= az) {
        face = d.y < 0.f ? 3u : 2u; u = d.x; v = d.z; m = ay;
    } else {
        face = d.z < 0.f ? 5u : 4u; u = d.x; v = d.y; m = az;
    }
    const float r = hb * __builtin_amdgcn_rcpf(m);  // cube-map coordinates in [-1, 1] -> [0, B)
    ub = (uint32_t)__builtin_fminf(__builtin_fmaxf(u * r + hb, 0.f), bm);
    vb = (uint32_t)__builtin_fminf(__builtin_fmaxf(v * r + hb, 0.f), bm);
}
// The key's coordinates in one word for k_material's membership test (occ_member2): dirbin | cx << 15 |
// cy << 20 | cz << 25; dirbin < 6 * 64^2 < 2^15 always, the cells fit for occ_g <= 32 (the upload
// builds complete keys, the only users, for no larger grid)
__device__ inline uint32_t occ_index(const DevScene& sc, V3 o, V3 d, uint32_t* packed = nullptr) {
    uint32_t cx, cy, cz, face, ub, vb;
    occ_coords(sc, o, d, cx, cy, cz, face, ub, vb);
    const uint32_t G = (uint32_t)sc.occ_g, B = (uint32_t)sc.occ_b;
    if (packed) *packed = ((face * B + ub) * B + vb) | cx << 15 | cy << 20 | cz << 25;
    // one table cell per key (hashing the keys into a 2^21- or 2^23-cell table measured 43 % / 60 %
    // of config 2's any-hit rays resolved against 72 % direct: the keys that occur collide heavily)
#if MCPT_OCC_LAYOUT == 1
    // direction major: lanes whose rays share a direction bin and lie in neighbouring origin cells
    // (along x) read one 128-B line (A/B knob)
    return (((face * B + ub) * B + vb) * G + cz) * G * G + cy * G + cx;
#else
    return ((((cz * G + cy) * G + cx) * 6u + face) * B + ub) * B + vb;
#endif
}

}  // namespace mcpt_dev
