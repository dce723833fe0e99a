// emitter_table.cpp -- see emitter_table.hpp.  Setup code, not the hot path.
#include "host/emitter_table.hpp"

#include <algorithm>
#include <cmath>

namespace mcpt_host {

void build_emitter_table(const float* weight, const uint32_t* id, size_t nrec, EmitterTable& out) {
    out = EmitterTable{};
    std::vector<uint32_t> keep;
    for (size_t r = 0; r < nrec; r++)
        if (weight[r] > 0.f && std::isfinite(weight[r])) keep.push_back((uint32_t)r);
    // by scene id; equal ids (a caller's duplicate) keep their record order
    std::stable_sort(keep.begin(), keep.end(), [id](uint32_t a, uint32_t b) { return id[a] < id[b]; });
    const size_t n = keep.size();
    if (!n) return;
    std::vector<double> prefix(n);
    double sum = 0.0;
    for (size_t k = 0; k < n; k++) {
        sum += (double)weight[keep[k]];
        prefix[k] = sum;
    }
    out.total = sum;
    out.cdf.resize(n);
    out.pick.resize(n);
    out.id.resize(n);
    out.rec.resize(n);
    for (size_t k = 0; k < n; k++) {
        out.cdf[k] = k + 1 == n ? 1.f : (float)(prefix[k] / sum);
        out.pick[k] = k ? out.cdf[k] - out.cdf[k - 1] : out.cdf[k];
        out.id[k] = id[keep[k]];
        out.rec[k] = keep[k];
    }
}

}  // namespace mcpt_host
