// emitter.hip -- emitter sampling's setup kernel: one weight per triangle record,
// from which the host builds the emitter table (host/emitter_table.cpp).  The per-vertex sampling itself
// is part of k_material (kernels.hip).
#include "kernels.hpp"

namespace mcpt_dev {

// weight[r] = area * luminance(Le[mat]) of record r, the area by the expressions k_material's emitter
// sample evaluates (so pick / area there is the density this weight stands for); 0 for a material that
// does not emit.  id[r]: the record's scene triangle id (the table's order).
__global__ __launch_bounds__(256) void k_emitter_weights(const float4* tri, const float4* tri_sh, const float4* emis,
                                                         uint32_t ntri, float* weight, uint32_t* id) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= ntri) return;
    const float4 w0 = tri[(size_t)kTriF4 * r], w1 = tri[(size_t)kTriF4 * r + 1], w2 = tri[(size_t)kTriF4 * r + 2];
    const mcpt::V3 e1 = mcpt::v3(w0.w, w1.x, w1.y), e2 = mcpt::v3(w1.z, w1.w, w2.x);
    const int mat = __float_as_int(tri_sh[3 * (size_t)r + 2].y);
    const float4 le = emis[mat];
    float w = 0.f;
    if (le.x != 0.f || le.y != 0.f || le.z != 0.f) {
        const mcpt::V3 c = mcpt::cross(e1, e2);
        const float area = 0.5f * __builtin_sqrtf(mcpt::dot(c, c));
        w = area * mcpt::luminance(mcpt::v3(le.x, le.y, le.z));
    }
    weight[r] = w;
    id[r] = (uint32_t)__float_as_int(w2.y);
}

void launch_emitter_weights(const DevScene& sc, const float4* emis, float* weight, uint32_t* id, hipStream_t s) {
    if (!sc.ntri) return;
    hipLaunchKernelGGL(k_emitter_weights, dim3((sc.ntri + 255u) / 256u), dim3(256), 0, s, sc.tri, sc.tri_sh, emis, sc.ntri,
                       weight, id);
}

}  // namespace mcpt_dev
