// Host build of the culling margins k_cull_tri computes (device/mcpt_core.hpp cull_tri_margin and
// cull_to_float_up are host/device): the arbiter between the device's margin words and the oracle's
// restatement (oracle/trav_model.c or_model_margins).  Compiled and run by tests/test_bvh_ref_host.py
// with hipcc (host code) -ffp-contract=off.
//   cull_margin_host IN OUT: IN holds n triangles as 9 floats (v0, v1, v2); OUT gets n floats W'_T and
//   one more, the far coefficient P -- from the edges as the triangle records store them (float32
//   v1 - v0, v2 - v0), exactly k_cull_tri's inputs.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "device/mcpt_core.hpp"

using namespace mcpt;

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<float> v;
    float buf[9];
    while (std::fread(buf, sizeof(float), 9, f) == 9) v.insert(v.end(), buf, buf + 9);
    std::fclose(f);
    const size_t n = v.size() / 9;
    std::vector<float> out(n + 1);
    uint32_t pmax = 0;  // positive floats order as their bits (k_cull_tri's atomicMax)
    for (size_t i = 0; i < n; i++) {
        const float* p = &v[9 * i];
        const V3 e1 = v3(p[3] - p[0], p[4] - p[1], p[5] - p[2]), e2 = v3(p[6] - p[0], p[7] - p[1], p[8] - p[2]);
        double far;
        out[i] = cull_to_float_up(cull_tri_margin(e1, e2, &far, true));
        if (far > 0.0) {
            const float pf = cull_to_float_up(far);
            uint32_t pb;
            std::memcpy(&pb, &pf, 4);
            if (pb > pmax) pmax = pb;
        }
    }
    std::memcpy(&out[n], &pmax, 4);
    f = std::fopen(argv[2], "wb");
    if (!f) return 2;
    const bool ok = std::fwrite(out.data(), sizeof(float), n + 1, f) == n + 1;
    return std::fclose(f) == 0 && ok ? 0 : 2;
}
