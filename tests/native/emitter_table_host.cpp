// emitter_table_host.cpp -- the emitter table builder (csrc/host/emitter_table.cpp, DESIGN.md section
// 17) as a stand-alone CPU program: the table's invariants on generated weights, the exclusion rule and
// the independence of the record order.  Exit status 0 and "ok" on success.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <numeric>
#include <vector>

#include "host/emitter_table.hpp"

using mcpt_host::EmitterTable;

static int fails = 0;
#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);    \
            fails++;                                               \
        }                                                          \
    } while (0)

static uint32_t lcg(uint32_t& s) { return s = s * 1664525u + 1013904223u; }

static void invariants(const EmitterTable& t, const std::vector<float>& w, const std::vector<uint32_t>& id) {
    const size_t n = t.cdf.size();
    CHECK(t.pick.size() == n && t.id.size() == n && t.rec.size() == n);
    size_t want = 0;
    for (float x : w) want += x > 0.f && std::isfinite(x);
    CHECK(n == want);
    if (!n) return;
    CHECK(t.cdf[n - 1] == 1.f);
    double psum = 0.0;
    for (size_t k = 0; k < n; k++) {
        CHECK(t.rec[k] < w.size());
        CHECK(id[t.rec[k]] == t.id[k]);
        CHECK(w[t.rec[k]] > 0.f && std::isfinite(w[t.rec[k]]));
        if (k) CHECK(t.id[k] > t.id[k - 1] && t.cdf[k] >= t.cdf[k - 1]);
        CHECK(t.pick[k] == (k ? t.cdf[k] - t.cdf[k - 1] : t.cdf[k]));
        psum += (double)t.pick[k];
    }
    // each pick is one fp32 rounding of a difference of values <= 1: half an ulp of 1 per entry
    CHECK(std::fabs(psum - 1.0) <= (double)n * 0x1p-24);
}

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    {  // nothing emits
        std::vector<float> w = {0.f, 0.f, -1.f, nan, inf};
        std::vector<uint32_t> id = {0, 1, 2, 3, 4};
        EmitterTable t;
        mcpt_host::build_emitter_table(w.data(), id.data(), w.size(), t);
        CHECK(t.cdf.empty() && t.total == 0.0);
        mcpt_host::build_emitter_table(nullptr, nullptr, 0, t);
        CHECK(t.cdf.empty());
    }
    {  // a small table by hand: ids out of record order, excluded records between
        std::vector<float> w = {2.f, 0.f, 1.f, nan, 1.f};
        std::vector<uint32_t> id = {7, 1, 3, 4, 0};
        EmitterTable t;
        mcpt_host::build_emitter_table(w.data(), id.data(), w.size(), t);
        invariants(t, w, id);
        CHECK(t.cdf.size() == 3 && t.total == 4.0);
        if (t.cdf.size() == 3) {
            CHECK(t.id[0] == 0 && t.id[1] == 3 && t.id[2] == 7);
            CHECK(t.rec[0] == 4 && t.rec[1] == 2 && t.rec[2] == 0);
            CHECK(t.cdf[0] == 0.25f && t.cdf[1] == 0.5f && t.cdf[2] == 1.f);
            CHECK(t.pick[0] == 0.25f && t.pick[1] == 0.25f && t.pick[2] == 0.5f);
        }
    }
    // generated weights over many sizes, and the same records permuted: the same table but for rec
    uint32_t s = 12345u;
    for (size_t n : {1u, 2u, 3u, 63u, 64u, 65u, 1000u, 4097u}) {
        std::vector<float> w(n);
        std::vector<uint32_t> id(n);
        for (size_t i = 0; i < n; i++) {
            const uint32_t r = lcg(s) >> 8;
            w[i] = (r & 7u) == 0 ? 0.f : (float)(r >> 3) * 0x1p-12f;  // one in eight does not emit
            id[i] = (uint32_t)i;
        }
        if (n > 2) w[n / 2] = inf;
        EmitterTable a;
        mcpt_host::build_emitter_table(w.data(), id.data(), n, a);
        invariants(a, w, id);
        std::vector<uint32_t> perm(n);
        std::iota(perm.begin(), perm.end(), 0u);
        for (size_t i = n - 1; i > 0; i--) std::swap(perm[i], perm[lcg(s) % (i + 1)]);
        std::vector<float> wp(n);
        std::vector<uint32_t> idp(n);
        for (size_t i = 0; i < n; i++) { wp[i] = w[perm[i]]; idp[i] = id[perm[i]]; }
        EmitterTable b;
        mcpt_host::build_emitter_table(wp.data(), idp.data(), n, b);
        invariants(b, wp, idp);
        CHECK(a.cdf == b.cdf && a.pick == b.pick && a.id == b.id && a.total == b.total);
        for (size_t k = 0; k < b.rec.size() && k < a.rec.size(); k++) CHECK(perm[b.rec[k]] == a.rec[k]);
    }
    if (fails) return 1;
    printf("ok\n");
    return 0;
}
