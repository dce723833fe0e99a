// emitter.hip -- emitter sampling's setup kernels: one weight per triangle record, from which the host
// builds the emitter table (host/emitter_table.cpp), and the table's pick
// probability keyed by record for the MIS collection weight (section 18).  The per-vertex sampling itself
// is part of k_material, the collection weight of k_shade (kernels.hip).
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

// pick_rec[ent[k].x] = entry k's pick probability: the emitter table keyed by
// triangle record, for the collection weight of a path that hits an emitter (k_shade's MIS
// instantiation).  The array is cleared first, so a record that is no entry reads 0.  Entries have
// distinct records: no two threads write one word.
__global__ __launch_bounds__(256) void k_emitter_pick_rec(const uint2* ent, uint32_t n, float* pick_rec, uint32_t ntri) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const uint2 e = ent[k];
    if (e.x < ntri) pick_rec[e.x] = __uint_as_float(e.y);
}

void launch_emitter_pick_rec(const uint2* ent, uint32_t n, float* pick_rec, uint32_t ntri, hipStream_t s) {
    if (!ntri) return;
    (void)hipMemsetAsync(pick_rec, 0, (size_t)ntri * sizeof(float), s);  // (an error surfaces at the caller's check)
    if (!n) return;
    hipLaunchKernelGGL(k_emitter_pick_rec, dim3((n + 255u) / 256u), dim3(256), 0, s, ent, n, pick_rec, ntri);
}

}  // namespace mcpt_dev
