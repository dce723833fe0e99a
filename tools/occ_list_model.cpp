// Candidate-list lengths of any-hit rays' table keys, from the product's own list builder
// (device/occ_beam.hpp occ_key_list) on the CPU.  Driven by tools/occ_list_model.py, which writes the
// input file: int32 {nnodes, ntri, G, B, nrays}, then the host BVH (bmin, bmax: 3 floats per node;
// offset, nprims: int32 per node; children of an interior node i are i + 1 and offset[i]), the
// triangles in leaf order (v0, v1, v2: 3 floats each) and the rays (o, d: 3 floats each).  Writes one
// int32 per ray to the output file: the key's candidate count (0 .. 8), -1 for a longer list (or the
// builder's box budget), -2 for a ray the key's beam does not contain or whose culling scale is not
// positive (such a ray is traversed whatever its key holds).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>

#include "device/occ_beam.hpp"

using namespace mcpt;

struct In {
    int nnodes, ntri, G, B, nrays;
    std::vector<float> bmin, bmax, v0, v1, v2, ro, rd;
    std::vector<int> offset, nprims;
};
static std::vector<float4> g_nodes, g_recs;
static std::vector<float> g_tw;
static float g_p = 0.f;

static int build(const In& in, int i, float& w) {
    if (in.nprims[i] > 0) {
        if (in.nprims[i] > 8) { fprintf(stderr, "leaf of %d triangles\n", in.nprims[i]); exit(2); }
        w = 0.f;
        for (int t = in.offset[i]; t < in.offset[i] + in.nprims[i]; t++) w = std::fmax(w, g_tw[t]);
        return (int)(0x80000000u | ((uint32_t)(in.nprims[i] - 1) << 24) | (uint32_t)in.offset[i]);
    }
    const int me = (int)(g_nodes.size() / 4), c[2] = {i + 1, in.offset[i]};
    g_nodes.resize(g_nodes.size() + 4);
    float cw[2];
    int r[2];
    for (int k = 0; k < 2; k++) r[k] = build(in, c[k], cw[k]);
    for (int a = 0; a < 3; a++)
        g_nodes[4 * me + a] = make_float4(in.bmin[3 * c[0] + a], in.bmin[3 * c[1] + a], in.bmax[3 * c[0] + a], in.bmax[3 * c[1] + a]);
    g_nodes[4 * me + 3] = make_float4(__builtin_bit_cast(float, r[0]), __builtin_bit_cast(float, r[1]), cw[0], cw[1]);
    w = std::fmax(cw[0], cw[1]);
    return me;
}

template <class T>
static void rd(FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short input\n"); exit(2); }
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    In in;
    int h[5];
    if (fread(h, 4, 5, f) != 5) return 2;
    in.nnodes = h[0]; in.ntri = h[1]; in.G = h[2]; in.B = h[3]; in.nrays = h[4];
    rd(f, in.bmin, 3 * (size_t)in.nnodes); rd(f, in.bmax, 3 * (size_t)in.nnodes);
    rd(f, in.offset, (size_t)in.nnodes); rd(f, in.nprims, (size_t)in.nnodes);
    rd(f, in.v0, 3 * (size_t)in.ntri); rd(f, in.v1, 3 * (size_t)in.ntri); rd(f, in.v2, 3 * (size_t)in.ntri);
    rd(f, in.ro, 3 * (size_t)in.nrays); rd(f, in.rd, 3 * (size_t)in.nrays);
    fclose(f);
    for (int t = 0; t < in.ntri; t++) {
        const float* a = &in.v0[3 * t];
        const V3 e1 = v3(in.v1[3 * t] - a[0], in.v1[3 * t + 1] - a[1], in.v1[3 * t + 2] - a[2]);
        const V3 e2 = v3(in.v2[3 * t] - a[0], in.v2[3 * t + 1] - a[1], in.v2[3 * t + 2] - a[2]);
        g_recs.push_back(make_float4(a[0], a[1], a[2], e1.x));
        g_recs.push_back(make_float4(e1.y, e1.z, e2.x, e2.y));
        g_recs.push_back(make_float4(e2.z, 0.f, 0.f, 0.f));
        double far;
        g_tw.push_back(cull_to_float_up(cull_tri_margin(e1, e2, &far)));
        if (far > 0.0) g_p = std::fmax(g_p, cull_to_float_up(far));
    }
    OccTree tr{};
    float w = 0.f;
    tr.root_ref = build(in, 0, w);
    tr.nodes = g_nodes.data();
    tr.tri = g_recs.data();
    tr.tri_f4 = 3;
    tr.ntri = (uint32_t)in.ntri;
    tr.root_w = w;
    tr.cull_p = g_p;
    std::vector<float4> dirs((size_t)6 * in.B * in.B * kOccDirF4);
    occ_dir_table(in.B, dirs.data());
    OccGrid g;
    float inv[3];
    for (int k = 0; k < 3; k++) {
        tr.root_mn[k] = g.mn[k] = in.bmin[k];
        tr.root_mx[k] = in.bmax[k];
        const float ext = in.bmax[k] - in.bmin[k];
        inv[k] = (float)in.G / ext;
        g.cell[k] = ext / (float)in.G;
    }
    g.g = in.G;
    g.b = in.B;
    g.dir = dirs.data();
    std::map<uint64_t, int> memo;  // key -> list length
    std::vector<int> out((size_t)in.nrays);
    const float gm = (float)(in.G - 1), bm = (float)(in.B - 1), hb = 0.5f * (float)in.B;
    for (int r = 0; r < in.nrays; r++) {
        const V3 o = v3(in.ro[3 * r], in.ro[3 * r + 1], in.ro[3 * r + 2]), d = v3(in.rd[3 * r], in.rd[3 * r + 1], in.rd[3 * r + 2]);
        // device/scene_dev.hpp occ_coords (an exact reciprocal for the device's rcp: the membership test decides)
        uint32_t c[3];
        const float oo[3] = {o.x, o.y, o.z};
        for (int k = 0; k < 3; k++) c[k] = (uint32_t)std::fmin(std::fmax((oo[k] - g.mn[k]) * inv[k], 0.f), gm);
        const float ax = std::fabs(d.x), ay = std::fabs(d.y), az = std::fabs(d.z);
        uint32_t face;
        float u, v, m;
        if (ax >= ay && ax >= az) { face = d.x < 0.f ? 1u : 0u; u = d.y; v = d.z; m = ax; }
        else if (ay >= az) { face = d.y < 0.f ? 3u : 2u; u = d.x; v = d.z; m = ay; }
        else { face = d.z < 0.f ? 5u : 4u; u = d.x; v = d.y; m = az; }
        const float rr = hb * (1.f / m);
        const uint32_t ub = (uint32_t)std::fmin(std::fmax(u * rr + hb, 0.f), bm), vb = (uint32_t)std::fmin(std::fmax(v * rr + hb, 0.f), bm);
        const uint32_t dirbin = (face * in.B + ub) * in.B + vb;
        const V3 iv = v3(1.f / d.x, 1.f / d.y, 1.f / d.z);
        const float io = std::fmax(std::fmax(std::fabs(iv.x), std::fabs(iv.y)), std::fabs(iv.z)) * kCullSlackF;
        const bool pos = io < HUGE_VALF && d.x * d.x + d.y * d.y + d.z * d.z <= kCullNormMax && io * g_p <= 1.f;
        if (!pos || !occ_member(g, c[0], c[1], c[2], dirbin, o, d)) { out[r] = -2; continue; }
        const uint64_t key = (((uint64_t)c[2] * in.G + c[1]) * in.G + c[0]) * 6u * in.B * in.B + dirbin;
        auto it = memo.find(key);
        if (it == memo.end()) {
            uint32_t list[8];
            it = memo.emplace(key, occ_key_list(tr, occ_key_beam(g, c[0], c[1], c[2], dirbin), 8, list)).first;
        }
        out[r] = it->second;
    }
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    fwrite(out.data(), 4, out.size(), f);
    fclose(f);
    return 0;
}
