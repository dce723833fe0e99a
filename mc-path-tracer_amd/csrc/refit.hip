// refit.hip -- geometry update of an uploaded scene (mcpt_scene_update_geometry).
//
// New vertex positions for the triangles that are already on the device: the intersection (and
// shading) records are rewritten in place through the upload's storage order, and the child-pair
// tree that is already there gets new boxes and culling margins without a change of topology:
//   1. k_geom_records: records (v0, e1 = v1 - v0, e2 = v2 - v0; the same float32 operations as the
//      upload's host loop) and each record's vertex box (exact min / max, as k_prim_boxes);
//   2. k_cull_tri (scene_tables.hip) gives every record its margin W'_T and the far coefficient P;
//   3. k_refit_reset: every leaf child's box (the union of its records' boxes) and margin; every
//      interior child's words start empty (box +inf / -inf, margin 0);
//   4. k_refit_pass x (depth + 2): an interior child's box and margin are the union / maximum of
//      that node's two stored children.  Bottom-up Jacobi passes in the style of k_cull_pairs and
//      k_bounds_pass: every word moves monotonically (min down, max up) from the empty value to its
//      subtree's exact value, so a word read before or after its own update in the same pass is
//      either way on the near side of the fixed point, which height + 1 passes reach.  min and max
//      are exact: no schedule can change a bit.  Boxes and margins share the passes: a node is read
//      and written once per pass;
//   5. k_refit_root: the root box and its margin from the root node (or the root leaf's records);
//   6. k_quad_regather (4-wide scenes): every slot of the 4-wide nodes copies its (pair node, child)
//      box and margin again through the slot -> source map the upload stored; refs and numbering
//      stay.
// Plain streaming kernels: 64-B pair nodes moved as four float4, one thread per node.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.hpp"

namespace mcpt_dev {

namespace {

constexpr int kB = 256;
constexpr int kNone = -1;  // kEnd: "no child" (pad nodes of layout 3)

__global__ void k_geom_records(GeomRecordsArgs a) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.ntri) return;
    const size_t p = a.order ? a.order[i] : i;
    const float ax = a.v0[3 * p], ay = a.v0[3 * p + 1], az = a.v0[3 * p + 2];
    const float bx = a.v1[3 * p], by = a.v1[3 * p + 1], bz = a.v1[3 * p + 2];
    const float cx = a.v2[3 * p], cy = a.v2[3 * p + 1], cz = a.v2[3 * p + 2];
    float4* r = a.tri + kTriF4 * (size_t)i;
    const float4 keep = r[2];  // .y: the triangle id
    r[0] = make_float4(ax, ay, az, bx - ax);
    r[1] = make_float4(by - ay, bz - az, cx - ax, cy - ay);
    r[2] = make_float4(cz - az, keep.y, keep.z, keep.w);
    if (a.n0) {
        float4* h = a.sh + 3 * (size_t)i;
        const float4 hk = h[2];  // .y: the material
        h[0] = make_float4(a.n0[3 * p], a.n0[3 * p + 1], a.n0[3 * p + 2], a.n1[3 * p]);
        h[1] = make_float4(a.n1[3 * p + 1], a.n1[3 * p + 2], a.n2[3 * p], a.n2[3 * p + 1]);
        h[2] = make_float4(a.n2[3 * p + 2], hk.y, hk.z, hk.w);
    }
    if (a.box) {
        a.box[2 * (size_t)i] = make_float4(fminf(fminf(ax, bx), cx), fminf(fminf(ay, by), cy), fminf(fminf(az, bz), cz), 0.f);
        a.box[2 * (size_t)i + 1] = make_float4(fmaxf(fmaxf(ax, bx), cx), fmaxf(fmaxf(ay, by), cy), fmaxf(fmaxf(az, bz), cz), 0.f);
    }
}

// box and margin of the leaf `ref` (records off .. off + cnt - 1)
__device__ inline void leaf_words(int ref, const float4* __restrict__ box, const float* __restrict__ tw, uint32_t ntri,
                                  float mn[3], float mx[3], float& w) {
    const uint32_t off = (uint32_t)ref & 0xffffffu, cnt = (((uint32_t)ref >> 24) & 7u) + 1u;
    mn[0] = mn[1] = mn[2] = INFINITY;
    mx[0] = mx[1] = mx[2] = -INFINITY;
    w = 0.f;
    for (uint32_t t = off; t < off + cnt && t < ntri; t++) {
        const float4 a = box[2 * (size_t)t], b = box[2 * (size_t)t + 1];
        mn[0] = fminf(mn[0], a.x); mn[1] = fminf(mn[1], a.y); mn[2] = fminf(mn[2], a.z);
        mx[0] = fmaxf(mx[0], b.x); mx[1] = fmaxf(mx[1], b.y); mx[2] = fmaxf(mx[2], b.z);
        w = fmaxf(w, tw[t]);
    }
}

__device__ inline void put_child(float4 q[4], int k, const float mn[3], const float mx[3], float w) {
    float* f = reinterpret_cast<float*>(q);
    for (int a = 0; a < 3; a++) { f[4 * a + k] = mn[a]; f[4 * a + 2 + k] = mx[a]; }
    f[12 + 2 + k] = w;
}

__global__ void k_refit_reset(float4* __restrict__ nodes, uint32_t npairs, const float4* __restrict__ box,
                              const float* __restrict__ tw, uint32_t ntri) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npairs) return;
    float4* nd = nodes + 4 * (size_t)i;
    float4 q[4] = {nd[0], nd[1], nd[2], nd[3]};
    const int ref[2] = {__float_as_int(q[3].x), __float_as_int(q[3].y)};
    if (ref[0] == kNone && ref[1] == kNone) return;  // a pad node stays as it is
#pragma unroll
    for (int k = 0; k < 2; k++) {
        float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY}, w = 0.f;
        if (ref[k] == kNone) continue;
        if (ref[k] < 0) leaf_words(ref[k], box, tw, ntri, mn, mx, w);
        put_child(q, k, mn, mx, w);
    }
    nd[0] = q[0]; nd[1] = q[1]; nd[2] = q[2]; nd[3] = q[3];
}

__global__ void k_refit_pass(float4* __restrict__ nodes, uint32_t npairs) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npairs) return;
    float4* nd = nodes + 4 * (size_t)i;
    const float4 q3 = nd[3];
    const int ref[2] = {__float_as_int(q3.x), __float_as_int(q3.y)};
    const bool in0 = ref[0] >= 0 && (uint32_t)ref[0] < npairs, in1 = ref[1] >= 0 && (uint32_t)ref[1] < npairs;
    if (!in0 && !in1) return;  // leaf children only: final since the reset
    float4 q[4] = {nd[0], nd[1], nd[2], q3};
#pragma unroll
    for (int k = 0; k < 2; k++) {
        if (!(k ? in1 : in0)) continue;
        const float4* c = nodes + 4 * (size_t)ref[k];
        const float4 c0 = c[0], c1 = c[1], c2 = c[2], c3 = c[3];
        const float mn[3] = {fminf(c0.x, c0.y), fminf(c1.x, c1.y), fminf(c2.x, c2.y)};
        const float mx[3] = {fmaxf(c0.z, c0.w), fmaxf(c1.z, c1.w), fmaxf(c2.z, c2.w)};
        put_child(q, k, mn, mx, fmaxf(c3.z, c3.w));
    }
    nd[0] = q[0]; nd[1] = q[1]; nd[2] = q[2]; nd[3] = q[3];
}

// out[0..2] root box min, [3..5] max, [6] the root's margin
__global__ void k_refit_root(const float4* __restrict__ nodes, uint32_t npairs, int root_ref,
                             const float4* __restrict__ box, const float* __restrict__ tw, uint32_t ntri,
                             float* __restrict__ out) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    float mn[3], mx[3], w;
    if (root_ref >= 0) {
        if ((uint32_t)root_ref >= npairs) return;
        const float4* c = nodes + 4 * (size_t)root_ref;
        const float4 c0 = c[0], c1 = c[1], c2 = c[2], c3 = c[3];
        mn[0] = fminf(c0.x, c0.y); mn[1] = fminf(c1.x, c1.y); mn[2] = fminf(c2.x, c2.y);
        mx[0] = fmaxf(c0.z, c0.w); mx[1] = fmaxf(c1.z, c1.w); mx[2] = fmaxf(c2.z, c2.w);
        w = fmaxf(c3.z, c3.w);
    } else {
        leaf_words(root_ref, box, tw, ntri, mn, mx, w);
    }
    for (int a = 0; a < 3; a++) { out[a] = mn[a]; out[3 + a] = mx[a]; }
    out[6] = w;
}

// 4-wide node i: mn.x[4], mx.x[4], mn.y[4], mx.y[4], mn.z[4], mx.z[4], refs[4], margins[4]; slot k
// copies child (src & 1) of pair node (src >> 1), src = kQuadNoSrc: an empty slot
__global__ void k_quad_regather(float4* __restrict__ quads, uint32_t nquads, const uint32_t* __restrict__ src,
                                const float4* __restrict__ pairs, uint32_t npairs) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nquads) return;
    const uint4 s4 = reinterpret_cast<const uint4*>(src)[i];
    const uint32_t s[4] = {s4.x, s4.y, s4.z, s4.w};
    float4 o[8];
    float* f = reinterpret_cast<float*>(o);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        float v[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};  // mn.x mx.x mn.y mx.y mn.z mx.z margin
        if (s[k] != kQuadNoSrc && (s[k] >> 1) < npairs) {
            const float4* c = pairs + 4 * (size_t)(s[k] >> 1);
            const float4 c0 = c[0], c1 = c[1], c2 = c[2], c3 = c[3];
            const bool hi = s[k] & 1u;
            v[0] = hi ? c0.y : c0.x; v[1] = hi ? c0.w : c0.z;
            v[2] = hi ? c1.y : c1.x; v[3] = hi ? c1.w : c1.z;
            v[4] = hi ? c2.y : c2.x; v[5] = hi ? c2.w : c2.z;
            v[6] = hi ? c3.w : c3.z;
        }
#pragma unroll
        for (int a = 0; a < 6; a++) f[4 * a + k] = v[a];
        f[28 + k] = v[6];
    }
    float4* q = quads + 8 * (size_t)i;
#pragma unroll
    for (int a = 0; a < 6; a++) q[a] = o[a];
    q[7] = o[7];  // q[6], the refs, stays
}

}  // namespace

void launch_geom_records(const GeomRecordsArgs& a, hipStream_t s) {
    if (a.ntri == 0) return;
    hipLaunchKernelGGL(k_geom_records, dim3((a.ntri + kB - 1) / kB), dim3(kB), 0, s, a);
}

void launch_refit(float4* nodes, uint32_t npairs, int root_ref, int passes, const float4* box, const float* tri_w,
                  uint32_t ntri, float* out7, hipStream_t s) {
    if (npairs) {
        const dim3 g((npairs + kB - 1) / kB);
        hipLaunchKernelGGL(k_refit_reset, g, dim3(kB), 0, s, nodes, npairs, box, tri_w, ntri);
        for (int p = 0; p < passes; p++) hipLaunchKernelGGL(k_refit_pass, g, dim3(kB), 0, s, nodes, npairs);
    }
    hipLaunchKernelGGL(k_refit_root, dim3(1), dim3(64), 0, s, nodes, npairs, root_ref, box, tri_w, ntri, out7);
}

void launch_quad_regather(float4* quads, uint32_t nquads, const uint32_t* src, const float4* pairs, uint32_t npairs,
                          hipStream_t s) {
    if (nquads == 0) return;
    hipLaunchKernelGGL(k_quad_regather, dim3((nquads + kB - 1) / kB), dim3(kB), 0, s, quads, nquads, src, pairs, npairs);
}

}  // namespace mcpt_dev
