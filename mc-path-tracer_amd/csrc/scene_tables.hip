// scene_tables.hip -- the kernels that build tables at scene upload, on a camera change or on a film
// resize, each with its launcher: occluder records, probes and complete keys, culling margins, the
// primary-hit candidate table, the camera records and the env light's tables.  None runs in a
// wavefront iteration (kernels.hip).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device/mcpt_core.hpp"
#include "device/primary_beam.hpp"
#include "device/scene_dev.hpp"
#include "kernels.hpp"

using namespace mcpt;

namespace mcpt_dev {

__global__ void k_occ_records(DevScene sc, uint32_t nnodes, float4* out) {  // see launch_occ_records
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    auto put = [&](int ref, float mnx, float mny, float mnz, float mxx, float mxy, float mxz, float w) {
        if (ref >= 0 || ref == kEnd) return;
        const uint32_t off = (uint32_t)ref & 0xffffffu, cnt = (((uint32_t)ref >> 24) & 7u) + 1u;
        for (uint32_t k = off; k < off + cnt && k < sc.ntri; k++) {
            const float4* tr = sc.tri + kTriF4 * (size_t)k;  // (v0.xyz, e1.x) (e1.yz, e2.xy) (e2.z, ...)
            const float4 a = tr[0], b = tr[1], c = tr[2];
            float4* o = out + kOccRecF4 * (size_t)k;
            o[0] = make_float4(mnx, mny, mnz, w);  // .w: the leaf's culling margin
            o[1] = make_float4(mxx, mxy, mxz, a.x);
            o[2] = make_float4(a.y, a.z, a.w, b.x);
            o[3] = make_float4(b.y, b.z, b.w, c.x);
        }
    };
    if (i == 0 && sc.root_ref < 0)  // the whole tree is one leaf: its box is the root box
        put(sc.root_ref, sc.root_mn[0], sc.root_mn[1], sc.root_mn[2], sc.root_mx[0], sc.root_mx[1], sc.root_mx[2],
            sc.root_w);
    if (i >= nnodes) return;
    if (sc.width == 4) {  // mn.x[4], mx.x[4], mn.y[4], mx.y[4], mn.z[4], mx.z[4], refs[4], margins[4]
        const float4* nd = sc.nodes + 8 * (size_t)i;
        const float4 mnx = nd[0], mxx = nd[1], mny = nd[2], mxy = nd[3], mnz = nd[4], mxz = nd[5], rf = nd[6], wq = nd[7];
        const float* a0 = &mnx.x; const float* a1 = &mxx.x; const float* b0 = &mny.x;
        const float* b1 = &mxy.x; const float* c0 = &mnz.x; const float* c1 = &mxz.x; const float* r = &rf.x;
        const float* w = &wq.x;
        for (int k = 0; k < 4; k++) put(__float_as_int(r[k]), a0[k], b0[k], c0[k], a1[k], b1[k], c1[k], w[k]);
    } else {  // per axis (mn0, mn1, mx0, mx1), then (ref0, ref1, margin0, margin1)
        const float4* nd = sc.nodes + 4 * (size_t)i;
        const float4 q0 = nd[0], q1 = nd[1], q2 = nd[2], q3 = nd[3];
        put(__float_as_int(q3.x), q0.x, q1.x, q2.x, q0.z, q1.z, q2.z, q3.z);
        put(__float_as_int(q3.y), q0.y, q1.y, q2.y, q0.w, q1.w, q2.w, q3.w);
    }
}
void launch_occ_records(const DevScene& sc, uint32_t nnodes, float4* rec, hipStream_t s) {
    hipLaunchKernelGGL(k_occ_records, dim3(nnodes / 256 + 1), dim3(256), 0, s, sc, nnodes, rec);
}

// One probe ray per occluder-table key (the pre-fill at upload, scene_upload.cpp): from the centre of
// the key's origin cell along the centre of its direction bin, so that occ_index maps the probe back
// to its own key.  Tracing the probes as any-hit rays records an occluder in every key whose probe
// is occluded -- a property of the scene alone, like the BVH.
__global__ void k_occ_probes(DevScene sc, float4* ro, float4* rd, uint32_t nkeys) {
    const uint32_t key = blockIdx.x * blockDim.x + threadIdx.x;
    if (key >= nkeys) return;
    const uint32_t G = (uint32_t)sc.occ_g, B = (uint32_t)sc.occ_b;
    uint32_t t = key, cx, cy, cz, face, ub, vb;
#if MCPT_OCC_LAYOUT == 1
    cx = t % G; t /= G; cy = t % G; t /= G; cz = t % G; t /= G; vb = t % B; t /= B; ub = t % B; face = t / B;
#else
    vb = t % B; t /= B; ub = t % B; t /= B; face = t % 6u; t /= 6u; cx = t % G; t /= G; cy = t % G; cz = t / G;
#endif
    const uint32_t c[3] = {cx, cy, cz};
    float o[3];
    for (int k = 0; k < 3; k++)
        o[k] = sc.occ_inv[k] > 0.f ? sc.root_mn[k] + ((float)c[k] + 0.5f) / sc.occ_inv[k] : sc.root_mn[k];
    const float hb = 0.5f * (float)B;
    const float u = ((float)ub + 0.5f) / hb - 1.f, v = ((float)vb + 0.5f) / hb - 1.f;
    const float sg = (face & 1u) ? -1.f : 1.f;
    float d[3];
    if (face < 2u) { d[0] = sg; d[1] = u; d[2] = v; }
    else if (face < 4u) { d[0] = u; d[1] = sg; d[2] = v; }
    else { d[0] = u; d[1] = v; d[2] = sg; }
    const float inv_n = 1.f / __builtin_sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    ro[key] = make_float4(o[0], o[1], o[2], 0.f);
    rd[key] = make_float4(d[0] * inv_n, d[1] * inv_n, d[2] * inv_n, 0.f);
}
void launch_occ_probes(const DevScene& sc, float4* ro, float4* rd, uint32_t nkeys, hipStream_t s) {
    if (nkeys == 0) return;
    hipLaunchKernelGGL(k_occ_probes, dim3((nkeys + 255) / 256), dim3(256), 0, s, sc, ro, rd, nkeys);
}

// Complete keys (device/occ_beam.hpp): one thread per table key walks the child-pair tree with the
// key's beam; a key with at most kOccWays candidates gets them as marked words (the rest of its ways
// the marked empty word), every other key keeps what the pre-fill left.
__global__ void k_occ_complete(DevScene sc, mcpt::OccTree tree, uint32_t nkeys, uint32_t* ndone) {
    const uint32_t key = blockIdx.x * blockDim.x + threadIdx.x;
    bool done = false;
    if (key < nkeys) {
        const uint32_t G = (uint32_t)sc.occ_g, B = (uint32_t)sc.occ_b;
        uint32_t t = key, cx, cy, cz, face, ub, vb;
#if MCPT_OCC_LAYOUT == 1
        cx = t % G; t /= G; cy = t % G; t /= G; cz = t % G; t /= G; vb = t % B; t /= B; ub = t % B; face = t / B;
#else
        vb = t % B; t /= B; ub = t % B; t /= B; face = t % 6u; t /= 6u; cx = t % G; t /= G; cy = t % G; cz = t / G;
#endif
        const mcpt::OccGrid g{{sc.root_mn[0], sc.root_mn[1], sc.root_mn[2]}, {sc.occ_cell[0], sc.occ_cell[1], sc.occ_cell[2]},
                              sc.occ_g, sc.occ_b, sc.occ_dir};
        const mcpt::Beam b = mcpt::occ_key_beam(g, cx, cy, cz, (face * B + ub) * B + vb);
        uint32_t list[kOccWays];
        const int n = mcpt::occ_key_list(tree, b, (int)kOccWays, list);
        if (n >= 0) {
            done = true;
            for (uint32_t w = 0; w < kOccWays; w++)
                sc.occ[(size_t)key * kOccWays + w] = (int)w < n ? (mcpt::kOccDoneBit | list[w]) : mcpt::kOccDoneNone;
        }
    }
    const uint32_t cnt = (uint32_t)__popcll(__ballot(done));
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(ndone, cnt);
}
void launch_occ_complete(const DevScene& sc, const mcpt::OccTree& tree, uint32_t nkeys, uint32_t* ndone, hipStream_t s) {
    if (nkeys == 0) return;
    hipLaunchKernelGGL(k_occ_complete, dim3((nkeys + 255) / 256), dim3(256), 0, s, sc, tree, nkeys, ndone);
}

// Culling margins (mcpt_core.hpp "conservative box culling").  k_cull_tri: W'_T of every triangle
// record (float, rounded up) and the far coefficient P (positive floats order as their bits).
__global__ void k_cull_tri(const float4* tri, uint32_t ntri, float* tw, uint32_t* pmax, int plane) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ntri) return;
    const float4* r = tri + kTriF4 * (size_t)i;
    const float4 r0 = r[0], r1 = r[1], r2 = r[2];
    double far;
    tw[i] = cull_to_float_up(cull_tri_margin(v3(r0.w, r1.x, r1.y), v3(r1.z, r1.w, r2.x), &far, plane != 0));
    if (far > 0.0) atomicMax(pmax, __float_as_uint(cull_to_float_up(far)));
}
// One bottom-up pass over child-pair nodes: each child's word (q3.z / q3.w) = the largest W'_T
// under it -- its triangles for a leaf, the child node's two words for an interior child.  Words
// start at 0 and only grow toward the subtree maxima, so a word read before or after its own
// update in the same pass is either way a lower bound, and depth + 1 passes reach the fixed point.
__global__ void k_cull_pairs(float4* nodes, uint32_t npairs, const float* tw, uint32_t ntri) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npairs) return;
    const float4 q3 = nodes[4 * (size_t)i + 3];
    float w[2];
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const int ref = __float_as_int(k ? q3.y : q3.x);
        float v = 0.f;
        if (ref >= 0) {
            const float4 c = nodes[4 * (size_t)ref + 3];
            v = __builtin_fmaxf(c.z, c.w);
        } else if (ref != kEnd) {
            const uint32_t off = (uint32_t)ref & 0xffffffu, cnt = (((uint32_t)ref >> 24) & 7u) + 1u;
            for (uint32_t t = off; t < off + cnt && t < ntri; t++) v = __builtin_fmaxf(v, tw[t]);
        }
        w[k] = v;
    }
    nodes[4 * (size_t)i + 3] = make_float4(q3.x, q3.y, w[0], w[1]);
}
__global__ void k_cull_zero(float4* nodes, uint32_t npairs) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npairs) return;
    float4 q3 = nodes[4 * (size_t)i + 3];
    q3.z = q3.w = 0.f;
    nodes[4 * (size_t)i + 3] = q3;
}
void launch_cull_tri(const float4* tri, uint32_t ntri, float* tri_w, uint32_t* pmax, bool plane, hipStream_t s) {
    if (ntri) hipLaunchKernelGGL(k_cull_tri, dim3((ntri + 255) / 256), dim3(256), 0, s, tri, ntri, tri_w, pmax, plane ? 1 : 0);
}
void launch_cull_margins(float4* nodes, uint32_t npairs, const float4* tri, uint32_t ntri, float* tri_w,
                         uint32_t* pmax, int passes, bool plane, hipStream_t s) {
    launch_cull_tri(tri, ntri, tri_w, pmax, plane, s);
    if (!npairs) return;
    hipLaunchKernelGGL(k_cull_zero, dim3((npairs + 255) / 256), dim3(256), 0, s, nodes, npairs);
    for (int p = 0; p < passes; p++)
        hipLaunchKernelGGL(k_cull_pairs, dim3((npairs + 255) / 256), dim3(256), 0, s, nodes, npairs, tri_w, ntri);
}

// The candidate list of every pixel: a beam traversal of the BVH, one thread per pixel.  A subtree
// is skipped when the beam provably fails its box (each ancestor box contains its leaf boxes); a
// leaf's triangles are listed unless the whole beam sees them back-facing.  More than kPrimK
// candidates, or no bound: the pixel gets no list.
__global__ __launch_bounds__(64) void k_primary_build(PrimaryBuildArgs a) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (uint32_t)a.W * (uint32_t)a.H) return;
    const DevScene& sc = a.scene;
    const V3 cp = ld3f4(a.cam_px + i);
    const Beam b = a.cam.lens_radius > 0.f ? beam_lens(a.cam, cp) : beam_point(cp, ld3f4(a.cam_dir + i));
    uint32_t ids[kPrimK];
    int sid[kPrimK];
    int n = 0;
    bool over = !b.ok;
    if (!over) {
        const BeamInv iv = beam_inv(b);
        int stack[kMaxStack];
        int sp = 0;
        if (!beam_misses_box(b, iv, sc.root_mn[0], sc.root_mn[1], sc.root_mn[2], sc.root_mx[0], sc.root_mx[1], sc.root_mx[2]))
            stack[sp++] = sc.root_ref;
        while (sp > 0 && !over) {
            const int ref = stack[--sp];
            if (ref == kEnd) continue;
            if (ref < 0) {  // leaf: 0x80000000 | (count - 1) << 24 | offset
                const uint32_t off = (uint32_t)ref & 0xffffffu, cnt = (((uint32_t)ref >> 24) & 7u) + 1u;
                for (uint32_t k = off; k < off + cnt && k < sc.ntri && !over; k++) {
                    const float4* tr = sc.tri + kTriF4 * (size_t)k;
                    const float4 w0 = tr[0], w1 = tr[1], w2 = tr[2];
                    if (beam_backfacing(b, v3(w0.w, w1.x, w1.y), v3(w1.z, w1.w, w2.x))) continue;
                    if (n == kPrimK) { over = true; break; }
                    const int s = __float_as_int(w2.y);  // scene id: the list is kept in its order
                    int j = n++;
                    for (; j > 0 && sid[j - 1] > s; j--) { sid[j] = sid[j - 1]; ids[j] = ids[j - 1]; }
                    sid[j] = s;
                    ids[j] = k;
                }
                continue;
            }
            float mn[3][4], mx[3][4];
            int rf[4];
            int nch;
            if (sc.width == 4) {
                const float4* nd = sc.nodes + 8 * (size_t)ref;
                const float4 q[7] = {nd[0], nd[1], nd[2], nd[3], nd[4], nd[5], nd[6]};
                for (int ax = 0; ax < 3; ax++) {
                    mn[ax][0] = q[2 * ax].x; mn[ax][1] = q[2 * ax].y; mn[ax][2] = q[2 * ax].z; mn[ax][3] = q[2 * ax].w;
                    mx[ax][0] = q[2 * ax + 1].x; mx[ax][1] = q[2 * ax + 1].y; mx[ax][2] = q[2 * ax + 1].z; mx[ax][3] = q[2 * ax + 1].w;
                }
                rf[0] = __float_as_int(q[6].x); rf[1] = __float_as_int(q[6].y);
                rf[2] = __float_as_int(q[6].z); rf[3] = __float_as_int(q[6].w);
                nch = 4;
            } else {
                const float4* nd = sc.nodes + 4 * (size_t)ref;
                const float4 q[4] = {nd[0], nd[1], nd[2], nd[3]};
                for (int ax = 0; ax < 3; ax++) {
                    mn[ax][0] = q[ax].x; mn[ax][1] = q[ax].y; mx[ax][0] = q[ax].z; mx[ax][1] = q[ax].w;
                }
                rf[0] = __float_as_int(q[3].x); rf[1] = __float_as_int(q[3].y);
                nch = 2;
            }
            for (int k = 0; k < nch; k++) {
                if (rf[k] == kEnd) continue;
                if (beam_misses_box(b, iv, mn[0][k], mn[1][k], mn[2][k], mx[0][k], mx[1][k], mx[2][k])) continue;
                if (sp == kMaxStack) { over = true; break; }
                stack[sp++] = rf[k];
            }
        }
    }
    uint32_t* lp = a.list + (size_t)kPrimLine * i;
    for (int k = 0; k < kPrimK; k++) lp[k] = (!over && k < n) ? ids[k] : 0u;
    a.cnt[i] = over ? (uint8_t)0 : (uint8_t)(n + 1);
    const uint64_t mo = __ballot(over), ml = __ballot(!over);
    if ((threadIdx.x & 63) == 0) {
        if (ml) atomicAdd(a.stats + 0, (uint32_t)__popcll(ml));
        if (mo) atomicAdd(a.stats + 1, (uint32_t)__popcll(mo));
    }
}
void launch_primary_build(const PrimaryBuildArgs& a, hipStream_t s) {
    const uint32_t n = (uint32_t)a.W * (uint32_t)a.H;
    if (n) hipLaunchKernelGGL(k_primary_build, dim3((n + 63) / 64), dim3(64), 0, s, a);
}

// Camera records of a W x H film: gen_ray_pixel of every pixel (ShadeArgs::cam_px / cam_dir)
__global__ void k_cam_table(mcpt::CamView cam, int W, int H, float4* px, float4* dir) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (uint32_t)W * (uint32_t)H) return;
    const int x = (int)(i % (uint32_t)W), y = (int)(i / (uint32_t)W);
    V3 o, d;
    gen_ray_pixel(cam, W, H, x, y, o, d);
    px[i] = f4(cam.lens_radius > 0.f ? gen_ray_focal(cam, o, d) : o, 0.f);
    dir[i] = f4(d, 0.f);
}
void launch_cam_table(const mcpt::CamView& cam, int W, int H, float4* px, float4* dir, hipStream_t s) {
    const uint32_t n = (uint32_t)W * (uint32_t)H;
    if (n) hipLaunchKernelGGL(k_cam_table, dim3((n + 255) / 256), dim3(256), 0, s, cam, W, H, px, dir);
}

// The env texture's device copy takes the pdf table into its alpha plane (EnvView::tex)
__global__ void k_env_pack(float4* tex, const float* __restrict__ pdf, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) tex[i].w = pdf[i];
}
void launch_env_pack(float4* tex, const float* pdf, size_t n, hipStream_t s) {
    if (n) hipLaunchKernelGGL(k_env_pack, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, tex, pdf, n);
}

// Light-sample table of an HRDI env light (EnvView::ltab / lrow / lcol): entry (y, x + 1)
// holds env_L / env_pdf at the direction env_dir returns for cell (x, y) -- computed by the
// very functions the per-sample path calls, so the values are the same -- and the row /
// column tables the direction's two factors (spherical_theta / spherical_phi of the cell's
// v / u, the arithmetic of spherical_direction).
template <bool FIXED>
__global__ void k_env_table(EnvView e, float4* out, float2* row, float2* col) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int W1 = e.w + 1;
    if (i < e.h) {
        float st, ct;
        spherical_theta(env_cell_v<FIXED>(e, i), st, ct);
        row[i] = make_float2(st, ct);
    }
    if (i < W1) {
        const int x = i - 1;
        float sp, cp;
        spherical_phi(env_cell_u<FIXED>(e, FIXED && x < 0 ? 0 : x), sp, cp);
        col[i] = make_float2(sp, cp);
    }
    if (i >= W1 * e.h) return;
    const int y = i / W1, x = i - y * W1 - 1;
    const V3 d = env_cell_dir<FIXED>(e, FIXED && x < 0 ? 0 : x, y);
    V3 L;
    float pdf;
    env_L_pdf<FIXED>(e, d, L, pdf);
    out[i] = make_float4(L.x, L.y, L.z, pdf);
}
void launch_env_table(const EnvView& e, bool fixed_mode, float4* out, float2* row, float2* col, hipStream_t s) {
    const int n = (e.w + 1) * e.h;
    if (fixed_mode) hipLaunchKernelGGL(k_env_table<true>, dim3((n + 255) / 256), dim3(256), 0, s, e, out, row, col);
    else hipLaunchKernelGGL(k_env_table<false>, dim3((n + 255) / 256), dim3(256), 0, s, e, out, row, col);
}

}  // namespace mcpt_dev
