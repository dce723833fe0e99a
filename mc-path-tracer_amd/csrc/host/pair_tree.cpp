// pair_tree.cpp -- see pair_tree.hpp
#include "pair_tree.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <utility>

namespace mcpt_host {
namespace {

constexpr float kFltMax = 3.402823466e+38f;

float as_float(int r) {
    float f;
    memcpy(&f, &r, 4);
    return f;
}

// One pair node: SoA boxes per axis (min child 0, min child 1, max child 0, max child 1), then the
// refs; .z / .w of q[3] are the children's culling margins (launch_cull_margins)
void emit_pair(float4* q, const float* a0, const float* b0, const float* a1, const float* b1, int r0, int r1) {
    q[0] = make_float4(a0[0], a1[0], b0[0], b1[0]);
    q[1] = make_float4(a0[1], a1[1], b0[1], b1[1]);
    q[2] = make_float4(a0[2], a1[2], b0[2], b1[2]);
    q[3] = make_float4(as_float(r0), as_float(r1), 0.f, 0.f);
}

// Every node of the desc's BVH; pair_of: the depth-first pair numbering of the interior nodes (the
// array's own order: parent next to its first child, layout 0), npair of them
bool validate_bvh(const mcpt_scene_desc& d, std::vector<int>& pair_of, int& npair, std::string& err) {
    const int N = d.nnodes;
    pair_of.assign(N, -1);
    npair = 0;
    for (int i = 0; i < N; i++) {
        if (d.nprims[i] == 0) {
            if (i + 1 >= N || d.offset[i] <= i || d.offset[i] >= N) { err = "bad BVH child offset"; return false; }
            pair_of[i] = npair++;
        } else {
            if (d.nprims[i] < 0 || d.nprims[i] > 8) { err = "leaf with more than 8 primitives"; return false; }
            if (d.offset[i] < 0 || d.offset[i] + d.nprims[i] > d.ntri) { err = "bad leaf range"; return false; }
        }
    }
    return true;
}

// Layout 3 (line pairs): every 128-B line holds a node and its larger-area interior child (a node
// without one leaves the line's second half as a pad node that nothing references), lines in
// depth-first order.  Modelled on config 4 (tools/trav_study.py): distinct lines per ray 28.5 -> 25.5,
// L2 misses per ray unchanged (4.77 -> 4.79); measured on the GPU before it becomes anyone's default.
// false (pair_of and npair as they were): the input is not a tree, see number_siblings.
bool number_line_pairs(const mcpt_scene_desc& d, std::vector<int>& pair_of, int& npair, std::vector<uint8_t>& is_pad) {
    const int N = d.nnodes;
    auto area = [&](int i) {
        float e[3];
        for (int k = 0; k < 3; k++) e[k] = std::fmax(d.bmax[3 * i + k] - d.bmin[3 * i + k], 0.f);
        return (double)e[0] * e[1] + (double)e[1] * e[2] + (double)e[2] * e[0];
    };
    auto inner = [&](int i, int out[2]) {
        int n = 0;
        for (int ch : {i + 1, d.offset[i]})
            if (d.nprims[ch] == 0) out[n++] = ch;
        return n;
    };
    std::vector<int> po(N, -1), st{0};
    int next = 0;
    bool tree = true;
    while (tree && !st.empty()) {
        const int i = st.back();
        st.pop_back();
        if (po[i] >= 0) { tree = false; break; }
        next += next & 1;  // a line starts with a head
        po[i] = next++;
        int ks[2], rest[3], nr = 0;
        const int nk = inner(i, ks);
        if (nk > 0) {
            const int cb = nk == 2 && area(ks[1]) > area(ks[0]) ? ks[1] : ks[0];
            if (po[cb] >= 0) { tree = false; break; }
            po[cb] = next++;  // the head's line partner
            for (int k = 0; k < nk; k++)
                if (ks[k] != cb) rest[nr++] = ks[k];
            int gk[2];
            const int ng = inner(cb, gk);
            for (int k = 0; k < ng; k++) rest[nr++] = gk[k];
        }
        // the larger-area subtree comes next (popped first)
        std::sort(rest, rest + nr, [&](int x, int y) { return area(x) < area(y); });
        for (int k = 0; k < nr; k++) st.push_back(rest[k]);
    }
    int reached = 0;
    for (int i = 0; i < N; i++) reached += d.nprims[i] == 0 && po[i] >= 0;
    if (!tree || reached != npair) return false;
    is_pad.assign(next, 1);
    for (int i = 0; i < N; i++)
        if (d.nprims[i] == 0) is_pad[po[i]] = 0;
    pair_of.swap(po);
    npair = next;  // pads included
    return true;
}

// Sibling-contiguous numbering for trees that stay in L2: the interior children of a node get
// consecutive pair indices (one 128-B line holds both, so a popped far child is often already
// cached), level by level (layout 2, breadth-first: the hot top levels share lines) or depth-first
// by sibling pairs (layout 1).  Measured against plain depth-first numbering (layout 0) on config 2
// (4.8 K pairs): k_trace 0.808 -> 0.786 (1) -> 0.781 ms (2); configs 3-5 (0.1-2 M pairs, beyond L2)
// run 1-2 % slower with 1 or 2, so they keep 0.  Layout only: hits are unchanged (tested).
// The walk from the root must reach every interior node exactly once (a tree); a shared child (a DAG,
// which validate_bvh accepts and layout 0 traverses correctly) or an unreachable node would give two
// nodes one pair index, so such inputs keep layout 0: false, pair_of as it was.
bool number_siblings(const mcpt_scene_desc& d, int layout, std::vector<int>& pair_of, int npair) {
    std::vector<int> po(pair_of);
    std::vector<uint8_t> seen(d.nnodes, 0);
    int next = 0;
    po[0] = next++;
    seen[0] = 1;
    bool tree = true;
    std::vector<int> st{0};  // layout 1: stack (depth-first by sibling pairs); 2: FIFO (breadth-first)
    size_t head = 0;
    while (tree && (layout == 2 ? head < st.size() : !st.empty())) {
        int i;
        if (layout == 2) {
            i = st[head++];
        } else {
            i = st.back();
            st.pop_back();
        }
        const int ch[2] = {i + 1, d.offset[i]};
        for (int k = 0; k < 2 && tree; k++) {
            if (d.nprims[ch[k]] != 0) continue;
            if (seen[ch[k]]) tree = false;  // reached twice
            seen[ch[k]] = 1;
            po[ch[k]] = next++;
        }
        if (layout == 2) {
            for (int k = 0; k < 2; k++)
                if (d.nprims[ch[k]] == 0) st.push_back(ch[k]);
        } else {
            for (int k = 1; k >= 0; k--)
                if (d.nprims[ch[k]] == 0) st.push_back(ch[k]);
        }
    }
    if (!tree || next != npair) return false;  // else every interior node reached exactly once: a permutation
    pair_of.swap(po);
    return true;
}

// the vertex union of triangles t0 .. t0 + n - 1 (g_init_BVH_triangle_info)
void tri_box(const mcpt_scene_desc& d, int t0, int n, float mn[3], float mx[3]) {
    for (int k = 0; k < 3; k++) { mn[k] = kFltMax; mx[k] = -kFltMax; }
    for (int t = t0; t < t0 + n; t++)
        for (const float* v : {d.v0 + 3 * (size_t)t, d.v1 + 3 * (size_t)t, d.v2 + 3 * (size_t)t})
            for (int k = 0; k < 3; k++) { mn[k] = std::fmin(mn[k], v[k]); mx[k] = std::fmax(mx[k], v[k]); }
}

// A leaf with several triangles becomes a small subtree of pair nodes whose leaves hold one triangle
// each, boxed by its own bounds.  A triangle then counts only if the line passes the leaf box and its
// own box -- BVHAccel's one-triangle-leaf semantics -- so results do not depend on how a builder
// grouped triangles (Moller-Trumbore alone can accept a grazing line just outside a triangle's box).
// The oracle applies the same own-box test to multi-triangle leaves.
// xn: the expansion pairs so far, numbered from npair on; returns the ref of triangles t0 .. t0 + n - 1.
int expand_leaf(const mcpt_scene_desc& d, int t0, int n, int npair, std::vector<float4>& xn) {
    if (n == 1) return (int)(0x80000000u | (uint32_t)t0);
    const int m = n / 2;
    const int me = npair + (int)(xn.size() / 4);
    xn.resize(xn.size() + 4);
    const int r0 = expand_leaf(d, t0, m, npair, xn), r1 = expand_leaf(d, t0 + m, n - m, npair, xn);
    float a0[3], b0[3], a1[3], b1[3];
    tri_box(d, t0, m, a0, b0);
    tri_box(d, t0 + m, n - m, a1, b1);
    emit_pair(&xn[(size_t)(me - npair) * 4], a0, b0, a1, b1, r0, r1);
    return me;
}

// depth of the tree = the most pair nodes on a root-to-leaf path (a bound on stack pushes, and the
// passes launch_cull_margins needs): a desc leaf adds the levels of its own expansion (halving, so
// ceil(log2 nprims)) to its own depth -- not the deepest expansion anywhere to the deepest leaf
int tree_depth(const mcpt_scene_desc& d) {
    int depth = 0;
    if (d.nnodes == 0) return depth;
    std::vector<std::pair<int, int>> st{{0, 0}};
    while (!st.empty()) {
        auto [n, dd] = st.back();
        st.pop_back();
        if (d.nprims[n] == 0) { st.push_back({n + 1, dd + 1}); st.push_back({d.offset[n], dd + 1}); continue; }
        int lv = 0;  // extra levels under this desc leaf
        while ((1 << lv) < d.nprims[n]) lv++;
        depth = std::max(depth, dd + lv);
    }
    return depth;
}

// Conservative culling (mcpt_core.hpp "conservative box culling") holds for a box that contains its
// triangles: a caller BVH whose node boxes miss some of their subtree's vertices is traversed without
// culling (contained false).  The occluder cache also needs every box inside its parent's (occ_test
// tests a leaf box in place of its ancestors): nested.
void containment(const mcpt_scene_desc& d, bool& contained, bool& nested) {
    const int N = d.nnodes;
    contained = nested = true;
    std::vector<float> lo(3 * (size_t)N, kFltMax), hi(3 * (size_t)N, -kFltMax);
    for (int i = N - 1; i >= 0; i--) {  // children follow their parent (offset[i] > i, i + 1)
        float* l = &lo[3 * (size_t)i];
        float* h = &hi[3 * (size_t)i];
        if (d.nprims[i] > 0) {
            for (int t = d.offset[i]; t < d.offset[i] + d.nprims[i]; t++)
                for (const float* v : {d.v0 + 3 * (size_t)t, d.v1 + 3 * (size_t)t, d.v2 + 3 * (size_t)t})
                    for (int k = 0; k < 3; k++) { l[k] = std::fmin(l[k], v[k]); h[k] = std::fmax(h[k], v[k]); }
        } else {
            for (int ch : {i + 1, d.offset[i]}) {
                for (int k = 0; k < 3; k++) {
                    l[k] = std::fmin(l[k], lo[3 * (size_t)ch + k]);
                    h[k] = std::fmax(h[k], hi[3 * (size_t)ch + k]);
                    if (!(d.bmin[3 * (size_t)ch + k] >= d.bmin[3 * (size_t)i + k]) ||
                        !(d.bmax[3 * (size_t)ch + k] <= d.bmax[3 * (size_t)i + k]))
                        nested = false;
                }
            }
        }
        for (int k = 0; k < 3; k++)
            if (!(l[k] >= d.bmin[3 * (size_t)i + k]) || !(h[k] <= d.bmax[3 * (size_t)i + k])) contained = false;
    }
    nested = nested && contained;
}

}  // namespace

bool validate_desc(const mcpt_scene_desc& d, bool needs_bvh, std::string& err) {
    auto fail = [&](const char* m) { err = m; return false; };
    if (d.ntri < 0 || d.nnodes < 0 || d.nmat < 0 || d.ndir < 0) return fail("negative sizes");
    if (d.ntri >= (1 << 24)) return fail("more than 2^24 triangles");
    if (d.ntri > 0 && d.nnodes == 0 && needs_bvh) return fail("triangles without BVH");
    for (int32_t i = 0; i < d.ntri; i++)
        if (d.mat[i] < 0 || d.mat[i] >= d.nmat) return fail("material id out of range");
    if (d.env_mode == 1) {
        // tables: all three given (host build), or none (built on the device from env_tex)
        const int given = !!d.env_marginal_y + !!d.env_conds_y + !!d.env_pdf;
        if (!d.env_tex || d.env_w < 2 || d.env_h < 2 || (given != 0 && given != 3))
            return fail("HRDI env light without texture or with partial tables");
        if ((int64_t)d.env_w * d.env_h >= ((int64_t)1 << 31)) return fail("env map too large");
    }
    return true;
}

bool build_pair_tree(const mcpt_scene_desc& d, int layout_request, PairTree& out, std::string& err) {
    out = PairTree{};
    std::vector<int> pair_of;
    int npair = 0;
    if (!validate_desc(d, true, err) || !validate_bvh(d, pair_of, npair, err)) return false;
    const int N = d.nnodes;
    int layout = (size_t)npair * 64 <= ((size_t)2 << 20) ? 2 : 0;
    if (layout_request >= 0 && layout_request <= 3) layout = layout_request;
    std::vector<uint8_t> is_pad;  // layout 3: pair indices that are pads
    const bool renumbered = N > 0 && d.nprims[0] == 0 && layout != 0 &&
                            (layout == 3 ? number_line_pairs(d, pair_of, npair, is_pad) : number_siblings(d, layout, pair_of, npair));
    out.layout = renumbered ? layout : 0;
    std::vector<float4> xn;  // expansion pairs, appended after the desc's pairs
    std::vector<int> leaf_ref(N, 0);
    for (int i = 0; i < N; i++)
        if (d.nprims[i] != 0) leaf_ref[i] = expand_leaf(d, d.offset[i], d.nprims[i], npair, xn);
    auto ref_of = [&](int j) -> int { return d.nprims[j] == 0 ? pair_of[j] : leaf_ref[j]; };
    std::vector<float4>& pn = out.pairs;
    pn.assign((size_t)npair * 4, make_float4(0.f, 0.f, 0.f, 0.f));
    for (size_t k = 0; k < is_pad.size(); k++)
        if (is_pad[k]) pn[4 * k + 3] = make_float4(as_float(-1), as_float(-1), 0.f, 0.f);  // kEnd: no child (never referenced)
    for (int i = 0; i < N; i++) {
        if (d.nprims[i] != 0) continue;
        const int c0 = i + 1, c1 = d.offset[i];
        emit_pair(&pn[(size_t)pair_of[i] * 4], d.bmin + 3 * c0, d.bmax + 3 * c0, d.bmin + 3 * c1, d.bmax + 3 * c1, ref_of(c0),
                  ref_of(c1));
    }
    pn.insert(pn.end(), xn.begin(), xn.end());
    out.root_ref = N > 0 ? ref_of(0) : 0;
    out.depth = tree_depth(d);
    if (out.depth > mcpt_dev::kMaxStack) { err = "BVH deeper than the 64-entry traversal stack"; return false; }
    if (N > 0) containment(d, out.contained, out.nested);
    return true;
}

void pack_records(const mcpt_scene_desc& d, std::vector<float4>& tri, std::vector<float4>& sh) {
    constexpr int kTriF4 = mcpt_dev::kTriF4;
    tri.assign((size_t)d.ntri * kTriF4, make_float4(0.f, 0.f, 0.f, 0.f));
    sh.resize((size_t)d.ntri * 3);
    for (int32_t i = 0; i < d.ntri; i++) {
        mcpt::V3 p0 = mcpt::ld3(d.v0, i), p1 = mcpt::ld3(d.v1, i), p2 = mcpt::ld3(d.v2, i);
        mcpt::V3 e1 = p1 - p0, e2 = p2 - p0;  // Triangle.cu:13-14
        tri[kTriF4 * i + 0] = make_float4(p0.x, p0.y, p0.z, e1.x);
        tri[kTriF4 * i + 1] = make_float4(e1.y, e1.z, e2.x, e2.y);
        // triangle id: the traversal's tie-break key and the API's triangle id
        tri[kTriF4 * i + 2] = make_float4(e2.z, as_float(d.tri_id ? d.tri_id[i] : i), 0.f, 0.f);
        mcpt::V3 n0 = mcpt::ld3(d.n0, i), n1 = mcpt::ld3(d.n1, i), n2 = mcpt::ld3(d.n2, i);
        sh[3 * i + 0] = make_float4(n0.x, n0.y, n0.z, n1.x);
        sh[3 * i + 1] = make_float4(n1.y, n1.z, n2.x, n2.y);
        sh[3 * i + 2] = make_float4(n2.z, as_float(d.mat[i]), 0.f, 0.f);
    }
}

// Collapse a child-pair BVH into 4-wide nodes (DevScene::width 4): every 4-wide node
// is a pair node at even depth; its slots are the children of its two children
// (a leaf child takes one slot itself).  Boxes are copied, never recomputed, so
// every leaf box is the pair tree's (and the reference builder's) exact box.
// Breadth-first numbering keeps the top levels together.  Returns the new root
// ref and the largest number of stack pushes along any root-to-leaf path.
// src: per slot the (pair node, child) it copies, 2 * node + child (kQuadNoSrc: an empty slot) -- the
// map a geometry update regathers the boxes and margins through (k_quad_regather).
int pairs_to_quads(const std::vector<float4>& pn, int root_ref, std::vector<float4>& qn, int& new_root, int& max_push,
                   std::vector<uint32_t>& src) {
    using mcpt_dev::kQuadNoSrc;
    qn.clear();
    src.clear();
    max_push = 0;
    if (root_ref < 0) { new_root = root_ref; return 0; }
    auto ref_at = [&](int p, int k) { int r; memcpy(&r, k ? &pn[4 * p + 3].y : &pn[4 * p + 3].x, 4); return r; };
    auto comp = [](const float4& v, int k) { return k == 0 ? v.x : k == 1 ? v.y : k == 2 ? v.z : v.w; };
    std::vector<int> quad_of(pn.size() / 4, -1), order;
    std::vector<int> push_depth;  // pushes accumulated on the path to each quad node
    order.push_back(root_ref);
    quad_of[root_ref] = 0;
    push_depth.push_back(0);
    for (size_t h = 0; h < order.size(); h++) {
        const int p = order[h];
        struct Slot { float mn[3], mx[3], w; int ref; uint32_t src; };  // w: the child's culling margin (q3.z / q3.w)
        Slot sl[4];
        int n = 0;
        for (int k = 0; k < 2; k++) {
            const int r = ref_at(p, k);
            if (r < 0) {  // leaf child of the pair node: its box is in p
                for (int a = 0; a < 3; a++) { sl[n].mn[a] = comp(pn[4 * p + a], k); sl[n].mx[a] = comp(pn[4 * p + a], 2 + k); }
                sl[n].w = comp(pn[4 * p + 3], 2 + k);
                sl[n].src = 2u * (uint32_t)p + (uint32_t)k;
                sl[n++].ref = r;
            } else {      // interior child: take its two children
                for (int j = 0; j < 2; j++) {
                    for (int a = 0; a < 3; a++) { sl[n].mn[a] = comp(pn[4 * r + a], j); sl[n].mx[a] = comp(pn[4 * r + a], 2 + j); }
                    sl[n].w = comp(pn[4 * r + 3], 2 + j);
                    sl[n].src = 2u * (uint32_t)r + (uint32_t)j;
                    sl[n++].ref = ref_at(r, j);
                }
            }
        }
        const int pd = push_depth[h] + (n - 1);
        max_push = std::max(max_push, pd);
        for (int k = 0; k < n; k++) {
            if (sl[k].ref >= 0) {
                const int g = sl[k].ref;
                if (quad_of[g] < 0) {
                    quad_of[g] = (int)order.size();
                    order.push_back(g);
                    push_depth.push_back(pd);
                }
                sl[k].ref = quad_of[g];
            }
        }
        float4 q[8];
        float* f = reinterpret_cast<float*>(q);
        for (int i = 0; i < 32; i++) f[i] = 0.f;
        for (int k = 0; k < 4; k++) {
            const bool used = k < n;
            for (int a = 0; a < 3; a++) {
                f[(2 * a) * 4 + k] = used ? sl[k].mn[a] : 0.f;      // mn.a[k]
                f[(2 * a + 1) * 4 + k] = used ? sl[k].mx[a] : 0.f;  // mx.a[k]
            }
            int r = used ? sl[k].ref : -1;  // kEnd: empty slot
            memcpy(&f[6 * 4 + k], &r, 4);
            f[7 * 4 + k] = used ? sl[k].w : 0.f;  // margins (float4 7)
        }
        qn.insert(qn.end(), q, q + 8);
        for (int k = 0; k < 4; k++) src.push_back(k < n ? sl[k].src : kQuadNoSrc);
    }
    new_root = 0;
    return 0;
}

}  // namespace mcpt_host
