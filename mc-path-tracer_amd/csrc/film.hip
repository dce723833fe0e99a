// film.hip -- film and debug utility kernels, each with its launcher: clear, slot resolve, tonemap,
// tile pack / unpack, the stage harness's hit records, and the quotient and HBM-copy probes.  None
// runs in a wavefront iteration (kernels.hip).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device/mcpt_core.hpp"
#include "device/scene_dev.hpp"
#include "kernels.hpp"

using namespace mcpt;

namespace mcpt_dev {

__global__ void k_clear(ClearArgs a) {  // g_clear_dfilm (wavefront_kernels.cu:55-66)
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    a.flags[i] = F_DEAD | ((i / a.npx) << F_SIDX_SHIFT);  // dead, next sample: the slot's first
    a.samples[i] = 0;
    a.Ld[i] = make_float4(0.f, 0.f, 0.f, 0.f);
}
void launch_clear(const ClearArgs& a, hipStream_t s) {
    if (a.n == 0) return;  // an empty tile set (compact layout): nothing to launch, no zero-sized grid
    hipLaunchKernelGGL(k_clear, dim3((a.n + 255) / 256), dim3(256), 0, s, a);
}

__global__ void k_resolve(ResolveArgs a) {  // film = sum of the path slots' accumulators, in slot order
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    uint32_t o = i;  // the pixel
    if (a.tiles) {   // compact layout: accumulator i is pixel li of tile-set tile ti
        const uint32_t tpx = (uint32_t)(a.tile_w * a.tile_h), ti = i / tpx, li = i - ti * tpx;
        const int2 t = a.tiles[ti];
        const uint32_t x = (uint32_t)t.x * a.tile_w + li % (uint32_t)a.tile_w, y = (uint32_t)t.y * a.tile_h + li / (uint32_t)a.tile_w;
        if (x >= (uint32_t)a.W || y >= (uint32_t)a.H) return;
        o = y * (uint32_t)a.W + x;
    }
    float4 L = a.Ld[i];
    uint32_t n = a.samples[i];
    for (int k = 1; k < a.slots; k++) {
        const float4 l = a.Ld[(size_t)k * a.n + i];
        L = make_float4(L.x + l.x, L.y + l.y, L.z + l.z, 0.f);
        n += a.samples[(size_t)k * a.n + i];
    }
    a.out_Ld[o] = L;
    a.out_samples[o] = n;
}
void launch_resolve(const ResolveArgs& a, hipStream_t s) {
    if (a.n == 0) return;
    hipLaunchKernelGGL(k_resolve, dim3((a.n + 255) / 256), dim3(256), 0, s, a);
}

__global__ void k_tonemap(TonemapArgs a) {  // draw_to_surface (wavefront_kernels.cu:6-40)
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    float4 L = a.Ld[i];
    float s = (float)a.samples[i];
    V3 c = v3(L.x / s, L.y / s, L.z / s);
    c = c * a.exposure;
    c = v3(c.x / (c.x + 1.0f), c.y / (c.y + 1.0f), c.z / (c.z + 1.0f));
    float cc[3] = {255 * c.x, 255 * c.y, 255 * c.z};
    uchar4 o;
    unsigned char b[3];
    for (int k = 0; k < 3; k++) {
        float v = cc[k];
        b[k] = (v == v && v >= 0.f && v < 4294967296.f) ? (unsigned char)(unsigned int)v : (unsigned char)0;
    }
    o.x = b[0]; o.y = b[1]; o.z = b[2]; o.w = 255;
    a.out[i] = o;
}
void launch_tonemap(const TonemapArgs& a, hipStream_t s) {
    if (a.n == 0) return;
    hipLaunchKernelGGL(k_tonemap, dim3((a.n + 255) / 256), dim3(256), 0, s, a);
}

__global__ void k_pack(PackArgs a) {  // tile-set pixels -> packed 16 B/px (for the RCCL gather)
    const int tile_px = a.tile_w * a.tile_h;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (uint32_t)(a.ntiles * tile_px)) return;
    const int tile = i / tile_px, li = i % tile_px;
    int2 t = a.tiles[tile];
    int x = t.x * a.tile_w + li % a.tile_w, y = t.y * a.tile_h + li / a.tile_w;
    float4 o = make_float4(0.f, 0.f, 0.f, __uint_as_float(0u));
    if (x < a.W && y < a.H) {
        uint32_t pid = (uint32_t)y * a.W + x;
        float4 L = a.Ld[pid];
        o = make_float4(L.x, L.y, L.z, __uint_as_float(a.samples[pid]));
    }
    a.out[i] = o;
}
void launch_pack(const PackArgs& a, hipStream_t s) {
    uint32_t n = (uint32_t)(a.ntiles * a.tile_w * a.tile_h);
    if (n == 0) return;
    hipLaunchKernelGGL(k_pack, dim3((n + 255) / 256), dim3(256), 0, s, a);
}

__global__ void k_unpack(UnpackArgs a) {  // packed 16 B/px of a tile set -> film accumulators (mcpt_gather)
    const int tile_px = a.tile_w * a.tile_h;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (uint32_t)(a.ntiles * tile_px)) return;
    const int tile = i / tile_px, li = i % tile_px;
    const int2 t = a.tiles[tile];
    const int x = t.x * a.tile_w + li % a.tile_w, y = t.y * a.tile_h + li / a.tile_w;
    if (x >= a.W || y >= a.H) return;
    const uint32_t pid = (uint32_t)y * a.W + x;
    const float4 v = a.in[i];
    a.Ld[pid] = make_float4(v.x, v.y, v.z, 0.f);
    a.samples[pid] = __float_as_uint(v.w);
}
void launch_unpack(const UnpackArgs& a, hipStream_t s) {
    const uint32_t n = (uint32_t)(a.ntiles * a.tile_w * a.tile_h);
    if (n) hipLaunchKernelGGL(k_unpack, dim3((n + 255) / 256), dim3(256), 0, s, a);
}

__global__ void k_hit_record(HitRecordArgs a) {  // stage_run(EXTEND) outputs
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const int tri = a.tri[i];
    if (tri < 0) {
        a.hit_p[i] = make_float4(0.f, 0.f, 0.f, K_HUGE);
        a.hit_n[i] = make_float4(0.f, 0.f, 0.f, __int_as_float(-1));
        a.scene_tri[i] = -1;
        return;
    }
    a.scene_tri[i] = __float_as_int(a.scene.tri[kTriF4 * tri + 2].y);  // storage position -> scene index
    V3 pos, nrm;
    int mat;
    float t;
    hit_record(a.scene, xyz(a.ro[i]), xyz(a.rd[i]), tri, pos, nrm, mat, t);
    a.hit_p[i] = make_float4(pos.x, pos.y, pos.z, t);
    a.hit_n[i] = make_float4(nrm.x, nrm.y, nrm.z, __int_as_float(mat));
}
void launch_hit_record(const HitRecordArgs& a, hipStream_t s) {
    if (a.n == 0) return;
    hipLaunchKernelGGL(k_hit_record, dim3((a.n + 255) / 256), dim3(256), 0, s, a);
}

__global__ void k_quot(const float* a, const float* b, float* out, uint32_t n) {  // mcpt_debug_quot
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float q0, q1, q2;
    quot3(a[i], 1.0f, -a[i], b[i], q0, q1, q2);
    out[i] = q0;
}
void launch_quot(const float* a, const float* b, float* out, uint32_t n, hipStream_t s) {
    if (n) hipLaunchKernelGGL(k_quot, dim3((n + 255) / 256), dim3(256), 0, s, a, b, out, n);
}

// HBM copy ceiling (mcpt_debug_hbm_copy; SURVEY.md 8(d) "re-measure a STREAM-copy ceiling"): one
// dwordx4 per lane, one pass (a block per 256 float4).  tools/hbm/copy_sweep.hip measured the
// variants: one-pass grids reach 6.25-6.39 TB/s on 1-4 GiB, persistent grid-stride loops
// 4.5-5.0 TB/s whatever the unroll or cache policy.
__global__ __launch_bounds__(256) void k_copy(const float4* __restrict__ src, float4* __restrict__ dst, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[i];
}
void launch_copy(const float4* src, float4* dst, size_t n, hipStream_t s) {
    if (n) hipLaunchKernelGGL(k_copy, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src, dst, n);
}

}  // namespace mcpt_dev
