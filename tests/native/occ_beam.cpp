// Host check of the occluder table's complete candidate lists (device/occ_beam.hpp).  For three scenes
// -- a cube, a tessellated sphere in a box, a random triangle soup, each under a child-pair tree built
// here with the culling margins of mcpt_core.hpp -- it draws table keys and rays that pass the key's
// membership test (occ_member): origins inside the cell and on its faces, directions inside the bin,
// on its edges and on face diagonals, zero and tiny components, lengths 0.5 .. 1.001.  Every ray with a
// finite inverse direction and a positive culling scale is then tested against every triangle with the
// scalar acceptance of the traversal (the leaf box's slab test on the fp32 products, tri_test_t, 0 <= t
// < K_HUGE): an accepted triangle must be in the key's list whenever the key is complete.
// Prints "bad=N"; exits 1 when N != 0, when a scene checked fewer than 1000 rays or when fewer than half
// of the cube's sampled keys are complete.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <vector>

#include "device/occ_beam.hpp"

using namespace mcpt;

static uint64_t g_s = 0x0CCBEA11ull;
static double urand() {
    g_s = splitmix64(g_s);
    return (double)(g_s >> 11) * (1.0 / 9007199254740992.0);
}
static double srand1() { return 2.0 * urand() - 1.0; }

struct Tri { float v0[3], e1[3], e2[3]; };
static Tri make_tri(const double* a, const double* b, const double* c) {
    Tri t;
    for (int k = 0; k < 3; k++) {
        t.v0[k] = (float)a[k];
        t.e1[k] = (float)b[k] - t.v0[k];
        t.e2[k] = (float)c[k] - t.v0[k];
    }
    return t;
}
static void quad(std::vector<Tri>& out, const double* a, const double* b, const double* c, const double* d) {
    out.push_back(make_tri(a, b, c));
    out.push_back(make_tri(a, c, d));
}
// an axis-aligned box of half extent h around the origin, n x n quads per face; outward = true: faces
// seen from outside
static void add_box(std::vector<Tri>& out, double h, bool outward, int n) {
    for (int ax = 0; ax < 3; ax++)
        for (int sg = -1; sg <= 1; sg += 2)
            for (int i = 0; i < n; i++)
                for (int j = 0; j < n; j++) {
                    const int u = (ax + 1) % 3, v = (ax + 2) % 3;
                    const double u0 = -h + 2 * h * i / n, u1 = -h + 2 * h * (i + 1) / n, v0 = -h + 2 * h * j / n, v1 = -h + 2 * h * (j + 1) / n;
                    double p[4][3];
                    const double cu[4] = {u0, u1, u1, u0}, cv[4] = {v0, v0, v1, v1};
                    for (int k = 0; k < 4; k++) { p[k][ax] = sg * h; p[k][u] = cu[k]; p[k][v] = cv[k]; }
                    // (u, v, ax) is right-handed: counter-clockwise in (u, v) faces +ax
                    if ((sg > 0) == outward) quad(out, p[0], p[1], p[2], p[3]);
                    else quad(out, p[0], p[3], p[2], p[1]);
                }
}
static void add_sphere(std::vector<Tri>& out, double r, int nu, int nv) {
    auto pt = [&](int i, int j, double* p) {
        const double th = M_PI * j / nv, ph = 2.0 * M_PI * i / nu;
        p[0] = r * std::sin(th) * std::cos(ph); p[1] = r * std::cos(th); p[2] = r * std::sin(th) * std::sin(ph);
    };
    for (int j = 0; j < nv; j++)
        for (int i = 0; i < nu; i++) {
            double a[3], b[3], c[3], d[3];
            pt(i, j, a); pt(i + 1, j, b); pt(i + 1, j + 1, c); pt(i, j + 1, d);
            if (j > 0) out.push_back(make_tri(a, b, c));
            if (j < nv - 1) out.push_back(make_tri(a, c, d));
        }
}

// A child-pair tree over the triangles (median splits of the centroids; leaves of up to leaf_max
// triangles), in the device layout occ_key_list walks, with each child's margin = the largest W'_T
// under it.  Boxes contain v0, v0 + e1, v0 + e2 as the floats tri_test sees them.
struct Scene {
    std::vector<Tri> tris;        // in leaf order
    std::vector<float4> nodes, recs;
    std::vector<float> leaf_mn, leaf_mx;  // per triangle: its leaf's box
    std::vector<float> tw;
    OccTree tree;
};
struct Box { float mn[3], mx[3]; };
static Box tri_box(const Tri& t) {
    Box b;
    for (int k = 0; k < 3; k++) {
        const float p[3] = {t.v0[k], t.v0[k] + t.e1[k], t.v0[k] + t.e2[k]};
        b.mn[k] = std::min(p[0], std::min(p[1], p[2]));
        b.mx[k] = std::max(p[0], std::max(p[1], p[2]));
    }
    return b;
}
static int build_rec(Scene& s, std::vector<int>& idx, int lo, int hi, const std::vector<Tri>& src, int leaf_max, Box& box,
                     float& w) {
    box = tri_box(src[idx[lo]]);
    for (int i = lo + 1; i < hi; i++) {
        const Box b = tri_box(src[idx[i]]);
        for (int k = 0; k < 3; k++) { box.mn[k] = std::min(box.mn[k], b.mn[k]); box.mx[k] = std::max(box.mx[k], b.mx[k]); }
    }
    if (hi - lo <= leaf_max) {
        const int off = (int)s.tris.size();
        w = 0.f;
        for (int i = lo; i < hi; i++) {
            const Tri& t = src[idx[i]];
            double far;
            const float tw = cull_to_float_up(cull_tri_margin(v3(t.e1[0], t.e1[1], t.e1[2]), v3(t.e2[0], t.e2[1], t.e2[2]), &far));
            if (far > 0.0) s.tree.cull_p = std::max(s.tree.cull_p, cull_to_float_up(far));
            w = std::max(w, tw);
            s.tris.push_back(t);
            for (int k = 0; k < 3; k++) { s.leaf_mn.push_back(box.mn[k]); s.leaf_mx.push_back(box.mx[k]); }
        }
        return (int)(0x80000000u | ((uint32_t)(hi - lo - 1) << 24) | (uint32_t)off);
    }
    int ax = 0;
    for (int k = 1; k < 3; k++) if (box.mx[k] - box.mn[k] > box.mx[ax] - box.mn[ax]) ax = k;
    auto cen = [&](int i) { const Box b = tri_box(src[i]); return b.mn[ax] + b.mx[ax]; };
    std::sort(idx.begin() + lo, idx.begin() + hi, [&](int a, int b) { return cen(a) < cen(b); });
    const int mid = (lo + hi) / 2, me = (int)(s.nodes.size() / 4);
    s.nodes.resize(s.nodes.size() + 4);
    Box b0, b1;
    float w0, w1;
    const int r0 = build_rec(s, idx, lo, mid, src, leaf_max, b0, w0), r1 = build_rec(s, idx, mid, hi, src, leaf_max, b1, w1);
    s.nodes[4 * me + 0] = make_float4(b0.mn[0], b1.mn[0], b0.mx[0], b1.mx[0]);
    s.nodes[4 * me + 1] = make_float4(b0.mn[1], b1.mn[1], b0.mx[1], b1.mx[1]);
    s.nodes[4 * me + 2] = make_float4(b0.mn[2], b1.mn[2], b0.mx[2], b1.mx[2]);
    s.nodes[4 * me + 3] = make_float4(__builtin_bit_cast(float, r0), __builtin_bit_cast(float, r1), w0, w1);
    w = std::max(w0, w1);
    return me;
}
static void build(Scene& s, const std::vector<Tri>& src, int leaf_max) {
    std::vector<int> idx(src.size());
    for (size_t i = 0; i < src.size(); i++) idx[i] = (int)i;
    s.tree = OccTree{};
    Box root;
    float w;
    s.tree.root_ref = build_rec(s, idx, 0, (int)src.size(), src, leaf_max, root, w);
    for (const Tri& t : s.tris) {
        s.recs.push_back(make_float4(t.v0[0], t.v0[1], t.v0[2], t.e1[0]));
        s.recs.push_back(make_float4(t.e1[1], t.e1[2], t.e2[0], t.e2[1]));
        s.recs.push_back(make_float4(t.e2[2], 0.f, 0.f, 0.f));
    }
    s.tree.nodes = s.nodes.data();
    s.tree.tri = s.recs.data();
    s.tree.tri_f4 = 3;
    s.tree.ntri = (uint32_t)s.tris.size();
    for (int k = 0; k < 3; k++) { s.tree.root_mn[k] = root.mn[k]; s.tree.root_mx[k] = root.mx[k]; }
    s.tree.root_w = w;
}

// kernels.hip cull_iota (cull_ok scenes)
static float cull_iota(float cull_p, V3 d, V3 inv) {
    const float ax = std::fabs(inv.x), ay = std::fabs(inv.y), az = std::fabs(inv.z);
    if (!(ax < HUGE_VALF && ay < HUGE_VALF && az < HUGE_VALF)) return -HUGE_VALF;
    const float n2 = d.x * d.x + d.y * d.y + d.z * d.z;
    if (!(n2 <= kCullNormMax)) return -3.4028235e38f;
    const float io = std::fmax(std::fmax(ax, ay), az) * kCullSlackF;
    return io * cull_p <= 1.f ? io : -io;
}

struct Tally { long keys = 0, complete = 0, drawn = 0, checked = 0, accepted = 0, listed = 0, bad = 0; };

// grid: the origin cells' box (the scene's root box scaled by grow about its centre)
static Tally run(const char* name, Scene& s, int G, int B, double grow, int nkeys, int nrays, int ways) {
    Tally t;
    std::vector<float4> dirs((size_t)6 * B * B * kOccDirF4);
    occ_dir_table(B, dirs.data());
    OccGrid g;
    for (int k = 0; k < 3; k++) {
        const double c = 0.5 * ((double)s.tree.root_mn[k] + s.tree.root_mx[k]), h = 0.5 * ((double)s.tree.root_mx[k] - s.tree.root_mn[k]) * grow;
        g.mn[k] = (float)(c - h);
        g.cell[k] = (float)(2.0 * h / G);
    }
    g.g = G;
    g.b = B;
    g.dir = dirs.data();
    const double hb = 0.5 * B;
    for (int ki = 0; ki < nkeys; ki++) {
        const uint32_t c[3] = {(uint32_t)(urand() * G), (uint32_t)(urand() * G), (uint32_t)(urand() * G)};
        const uint32_t face = (uint32_t)(urand() * 6), ub = (uint32_t)(urand() * B), vb = (uint32_t)(urand() * B);
        const uint32_t dirbin = (face * B + ub) * B + vb;
        const Beam beam = occ_key_beam(g, c[0], c[1], c[2], dirbin);
        uint32_t list[8];
        const int n = occ_key_list(s.tree, beam, ways, list);
        t.keys++;
        if (n < 0) continue;
        t.complete++;
        t.listed += n;
        for (int ri = 0; ri < nrays; ri++) {
            // origin: inside the cell, or with coordinates on its faces
            float o[3];
            const Iv civ[3] = {beam.o.x, beam.o.y, beam.o.z};
            for (int k = 0; k < 3; k++) {
                const double f = urand();
                const int mode = (int)(urand() * 6);
                o[k] = mode == 0 ? civ[k].lo : mode == 1 ? civ[k].hi : (float)(civ[k].lo + f * ((double)civ[k].hi - civ[k].lo));
            }
            // direction: cube-map coordinates in the bin (inside, on its edges, on the face diagonal,
            // exactly 0 or tiny where the bin allows), scaled to a length in 0.5 .. 1.001
            double a[2];
            const uint32_t bb[2] = {ub, vb};
            for (int k = 0; k < 2; k++) {
                const double lo = (bb[k] - hb) / hb, hi = (bb[k] + 1.0 - hb) / hb;
                const int mode = (int)(urand() * 8);
                a[k] = mode == 0 ? lo : mode == 1 ? hi : mode == 2 ? 0.0 : mode == 3 ? 1e-30 * srand1() : mode == 4 ? 1e-7 * srand1()
                                                                                                          : lo + urand() * (hi - lo);
            }
            if ((int)(urand() * 8) == 0) a[1] = a[0];                 // the face diagonal
            if ((int)(urand() * 16) == 0) a[0] = a[0] < 0 ? -1.0 : 1.0;  // the cube's edge: a tie of the major axis
            const int lm = (int)(urand() * 6);
            const double len = lm == 0 ? 0.5 + 0.501 * urand() : lm == 1 ? 1.001 : lm == 2 ? 1.0 + 1e-4 * srand1() : 1.0;
            const double m = len / std::sqrt(1.0 + a[0] * a[0] + a[1] * a[1]);
            const int major = (int)(face >> 1), ua = major == 0 ? 1 : 0, va = major == 2 ? 1 : 2;
            float d[3];
            d[major] = (float)((face & 1u) ? -m : m);
            d[ua] = (float)(a[0] * m);
            d[va] = (float)(a[1] * m);
            const V3 ro = v3(o[0], o[1], o[2]), rd = v3(d[0], d[1], d[2]);
            t.drawn++;
            if (!occ_member(g, c[0], c[1], c[2], dirbin, ro, rd)) continue;
            const V3 inv = v3(1.f / rd.x, 1.f / rd.y, 1.f / rd.z);
            if (!(cull_iota(s.tree.cull_p, rd, inv) > 0.f)) continue;  // (finite inverse included)
            t.checked++;
            for (uint32_t k = 0; k < s.tree.ntri; k++) {
                // pair_slab's arithmetic for the triangle's leaf box
                const float* mn = &s.leaf_mn[3 * k];
                const float* mx = &s.leaf_mx[3 * k];
                const float ax = (mn[0] - ro.x) * inv.x, bx = (mx[0] - ro.x) * inv.x;
                const float ay = (mn[1] - ro.y) * inv.y, by = (mx[1] - ro.y) * inv.y;
                const float az = (mn[2] - ro.z) * inv.z, bz = (mx[2] - ro.z) * inv.z;
                const float t0 = fmaxf(fmaxf(fminf(ax, bx), fminf(ay, by)), fminf(az, bz));
                const float t1 = fminf(fminf(fmaxf(ax, bx), fmaxf(ay, by)), fmaxf(az, bz));
                if (!(t0 <= t1)) continue;
                const Tri& tr = s.tris[k];
                float th;
                if (!tri_test_t(ro, rd, v3(tr.v0[0], tr.v0[1], tr.v0[2]), v3(tr.e1[0], tr.e1[1], tr.e1[2]),
                                v3(tr.e2[0], tr.e2[1], tr.e2[2]), th))
                    continue;
                if (th < 0.f || !(th < K_HUGE)) continue;
                t.accepted++;
                bool in_list = false;
                for (int j = 0; j < n; j++) in_list = in_list || list[j] == k;
                if (!in_list) t.bad++;
            }
        }
    }
    printf("%s: ntri=%u cull_p=%g keys=%ld complete=%ld listed=%ld rays_drawn=%ld rays_checked=%ld accepted=%ld bad=%ld\n", name, s.tree.ntri, (double)s.tree.cull_p, t.keys, t.complete,
           t.listed, t.drawn, t.checked, t.accepted, t.bad);
    return t;
}

int main() {
    long bad = 0;
    bool vacuous = false;
    {
        std::vector<Tri> src;
        add_box(src, 0.5, true, 1);
        Scene s;
        build(s, src, 1);
        // origin cells over the cube and a margin around it: rays from inside and from outside
        const Tally t = run("cube", s, 6, 12, 1.5, 1500, 32, 2);
        bad += t.bad;
        vacuous = vacuous || t.checked < 1000 || 2 * t.complete < t.keys;
    }
    {
        std::vector<Tri> src;
        add_box(src, 1.0, false, 2);  // a closed room seen from inside
        add_sphere(src, 0.3, 16, 8);
        Scene s;
        build(s, src, 2);
        const Tally t = run("sphere_in_box", s, 8, 12, 1.0, 6000, 48, 2);
        bad += t.bad;
        vacuous = vacuous || t.checked < 1000;
        // (the same scene with four ways: longer lists, the same guarantee)
        const Tally t4 = run("sphere_in_box_4way", s, 8, 12, 1.0, 2000, 32, 4);
        bad += t4.bad;
    }
    {
        std::vector<Tri> src;
        for (int i = 0; i < 300; i++) {
            double a[3], b[3], c[3];
            const double sz = i % 7 == 0 ? 0.15 : 0.05;
            for (int k = 0; k < 3; k++) { a[k] = 0.7 * srand1(); b[k] = a[k] + sz * srand1(); c[k] = a[k] + sz * srand1(); }
            if (i % 11 == 0) b[0] = c[0] = a[0];  // in an axis plane
            src.push_back(make_tri(a, b, c));
        }
        Scene s;
        build(s, src, 1);  // single-triangle leaf boxes
        const Tally t = run("soup", s, 6, 12, 1.0, 6000, 32, 2);
        bad += t.bad;
        vacuous = vacuous || t.checked < 1000;
    }
    printf("bad=%ld%s\n", bad, vacuous ? " VACUOUS" : "");
    return bad || vacuous ? 1 : 0;
}
