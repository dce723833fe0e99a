// emitter_table.hpp -- the emitter table of emitter sampling, built on the host
// from one weight per triangle record.  Host only: no HIP runtime call, so it compiles and is tested
// as a stand-alone program (tests/native/emitter_table_host.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace mcpt_host {

// One entry per emissive triangle, in ascending scene triangle id (not record position: a host tree, a
// device-built tree, a refit and a rebuild order their records differently and give the same table).
struct EmitterTable {
    std::vector<float> cdf;     // cdf[k] = (float)(sum of weights 0..k / total), the last entry exactly 1
    std::vector<float> pick;    // cdf[k] - cdf[k - 1] in fp32 (cdf[-1] = 0): the probability k is chosen with
    std::vector<uint32_t> id;   // scene triangle id
    std::vector<uint32_t> rec;  // the triangle's record index in the uploaded scene
    double total = 0.0;         // sum of the weights, fp64, in id order
    bool same(const EmitterTable& o) const { return cdf == o.cdf && pick == o.pick && id == o.id && rec == o.rec; }
};

// weight[r], id[r]: record r's area * luminance(Le) and scene triangle id.  Records whose weight is
// zero, negative or not finite get no entry.  The running sum is serial fp64 in id order, so numpy's
// cumsum over float64 reproduces it bit for bit.
void build_emitter_table(const float* weight, const uint32_t* id, size_t nrec, EmitterTable& out);

}  // namespace mcpt_host
