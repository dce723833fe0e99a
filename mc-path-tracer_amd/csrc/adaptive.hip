// adaptive.hip -- gfx950 kernels of adaptive sampling (device/adaptive.hpp): the film's error estimate
// from the path slots' accumulators, the sample budget built from it, and one slot's accumulators as
// an image.  One thread per film pixel, each a streaming pass: k_film_error reads the pixel's S
// accumulators (16 B + 4 B each) twice -- the mean, then the deviations; the second read of a line is
// served by the cache -- and writes 16 B; k_budget reads 16 B and writes 4 B.
#include <algorithm>

#include "kernels.hpp"

#include "device/adaptive.hpp"

namespace mcpt_dev {

using namespace mcpt;

// The accumulator index of film pixel o = y W + x, or false where the pixel is not the context's
__device__ inline bool own_index(const OwnMap& m, uint32_t o, uint32_t x, uint32_t y, size_t& i) {
    i = o;
    if (!m.own) return true;
    const uint32_t tw = (uint32_t)m.tile_w, th = (uint32_t)m.tile_h;
    const uint32_t ntx = ((uint32_t)m.W + tw - 1) / tw;
    const uint32_t tx = x / tw, ty = y / th;
    const int32_t place = m.own[ty * ntx + tx];
    if (place < 0) return false;
    if (m.compact) i = (size_t)place * (size_t)(tw * th) + (size_t)((y - ty * th) * tw + (x - tx * tw));
    return true;
}

__global__ __launch_bounds__(256) void k_film_error(FilmErrorArgs a) {
    const uint32_t o = blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= (uint32_t)a.m.W * (uint32_t)a.m.H) return;
    const uint32_t y = o / (uint32_t)a.m.W, x = o - y * (uint32_t)a.m.W;
    size_t i;
    float4 e = make_float4(-1.f, 0.f, 0.f, 0.f);  // not the context's pixel: K = 0
    if (own_index(a.m, o, x, y, i)) e = film_error_pixel(a.Ld, a.samples, a.stride, i, a.slots);
    a.out[o] = e;
}

// A bounded grid (launch_budget): every block strides over the film and adds its sum, maximum and
// count with one atomic each.  One block per 256 pixels meant 24K atomics on three words for a 1080p
// film, which serialise at roughly 90 per microsecond (kernels.hpp, kShards): 0.28 ms for a kernel
// that moves 41 MB.
__global__ __launch_bounds__(256) void k_budget(BudgetArgs a) {
    const uint32_t npix = (uint32_t)a.m.W * (uint32_t)a.m.H, step = gridDim.x * blockDim.x;
    unsigned long long sum = 0;
    uint32_t mx = 0, kept = 0;
    for (uint32_t o = blockIdx.x * blockDim.x + threadIdx.x; o < npix; o += step) {
        const uint32_t y = o / (uint32_t)a.m.W, x = o - y * (uint32_t)a.m.W;
        size_t i;
        // the last column and row are never rendered (k_shade)
        const bool owned = own_index(a.m, o, x, y, i) && x + 1 < (uint32_t)a.m.W && y + 1 < (uint32_t)a.m.H;
        const float4 e = a.err[o];
        const uint32_t b = budget_pixel(e, owned, a.p);
        kept += (owned && b == (uint32_t)e.w) ? 1u : 0u;
        a.budget[o] = b;
        sum += b;
        mx = b > mx ? b : mx;
    }
    __shared__ unsigned long long s_sum[4];
    __shared__ uint32_t s_max[4], s_kept[4];
    for (int off = 32; off > 0; off >>= 1) {
        sum += __shfl_xor(sum, off);
        mx = max(mx, (uint32_t)__shfl_xor(mx, off));
        kept += __shfl_xor(kept, off);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        s_sum[wave] = sum;
        s_max[wave] = mx;
        s_kept[wave] = kept;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0, k = 0, m = 0;
        for (int w = 0; w < 4; w++) {
            t += s_sum[w];
            k += s_kept[w];
            m = s_max[w] > m ? s_max[w] : m;
        }
        if (t) atomicAdd(a.cnt + 0, t);
        if (m) atomicMax(a.cnt + 1, m);
        if (k) atomicAdd(a.cnt + 2, k);
    }
}

__global__ __launch_bounds__(256) void k_slot_image(SlotImageArgs a) {
    const uint32_t o = blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= (uint32_t)a.m.W * (uint32_t)a.m.H) return;
    const uint32_t y = o / (uint32_t)a.m.W, x = o - y * (uint32_t)a.m.W;
    size_t i;
    float4 L = make_float4(0.f, 0.f, 0.f, 0.f);
    uint32_t n = 0;
    if (own_index(a.m, o, x, y, i)) {
        L = a.Ld[i];
        n = a.samples[i];
    }
    a.out_Ld[o] = L;
    a.out_samples[o] = n;
}

static unsigned pixel_blocks(const OwnMap& m) { return (unsigned)(((size_t)m.W * (size_t)m.H + 255) / 256); }
void launch_film_error(const FilmErrorArgs& a, hipStream_t s) {
    if (a.m.W <= 0 || a.m.H <= 0) return;
    hipLaunchKernelGGL(k_film_error, dim3(pixel_blocks(a.m)), dim3(256), 0, s, a);
}
void launch_budget(const BudgetArgs& a, hipStream_t s) {
    if (a.m.W <= 0 || a.m.H <= 0) return;
    hipLaunchKernelGGL(k_budget, dim3(std::min(pixel_blocks(a.m), 1024u)), dim3(256), 0, s, a);
}
void launch_slot_image(const SlotImageArgs& a, hipStream_t s) {
    if (a.m.W <= 0 || a.m.H <= 0) return;
    hipLaunchKernelGGL(k_slot_image, dim3(pixel_blocks(a.m)), dim3(256), 0, s, a);
}

}  // namespace mcpt_dev
