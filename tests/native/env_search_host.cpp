// Host check of the env light's guided CDF search (device/mcpt_core.hpp upper_bound_guided) against the
// plain bisection it replaces (upper_bound), on lists read from a file: int32 count, then per list int32 n
// and n floats.  Per list the guide is built as k_env_guides builds it (16-bit entries,
// guide[k] = upper_bound(list, n, k / kEnvGuide)), and the two searches are compared at up to 4096 values:
// the bin edges k / kEnvGuide with their float neighbours, 0, the largest float below 1, 1 itself (a
// rand_float() that rounds up), and distinct list values with their neighbours.  Prints
// "lists=L values=V bad=N" and exits 1 if any answer differs.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "device/mcpt_core.hpp"

using namespace mcpt;

static constexpr size_t kCap = 4096;

static void push(std::vector<float>& v, float x) {
    if (x >= 0.f && x <= 1.f && v.size() < kCap) v.push_back(x);
}
static void push3(std::vector<float>& v, float x) {
    push(v, std::nextafterf(x, -1.f));
    push(v, x);
    push(v, std::nextafterf(x, 2.f));
}

// wrapi against the mathematical i mod n, far enough on both sides that its i % n fallback (|i| >= 2n) runs:
// no caller reaches it on the device (tex_bilinear is handed spherical_map's u, v in [0, 1] and the upload
// refuses maps one texel wide or high), so the texture's documented wrap for |u| < 65536 is checked here.
static long long check_wrapi() {
    long long bad = 0;
    for (int n : {1, 2, 3, 4, 13, 37, 512, 65535, 65536})
        for (int64_t i = -5 * (int64_t)n - 3; i <= 5 * (int64_t)n + 3; i += (n > 4096 ? 257 : 1)) {
            const int64_t want = ((i % n) + n) % n;
            if (wrapi((int)i, n) != (int)want) {
                if (bad < 10) std::printf("wrapi(%lld, %d) = %d, not %lld\n", (long long)i, n, wrapi((int)i, n), (long long)want);
                bad++;
            }
        }
    return bad;
}

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: %s lists.bin\n", argv[0]); return 2; }
    if (const long long wb = check_wrapi()) { std::printf("wrapi bad=%lld\n", wb); return 1; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    int32_t count = 0;
    if (std::fread(&count, 4, 1, f) != 1 || count < 0) { std::fprintf(stderr, "bad header\n"); return 2; }
    long long values = 0, bad = 0;
    std::vector<float> list, vals;
    std::vector<uint16_t> guide(kEnvGuide + 1);
    for (int32_t l = 0; l < count; l++) {
        int32_t n = 0;
        if (std::fread(&n, 4, 1, f) != 1 || n < 1 || n > 65535) { std::fprintf(stderr, "bad list %d\n", l); return 2; }
        list.resize((size_t)n);
        if (std::fread(list.data(), 4, (size_t)n, f) != (size_t)n) { std::fprintf(stderr, "truncated list %d\n", l); return 2; }
        for (int k = 0; k <= kEnvGuide; k++)
            guide[(size_t)k] = (uint16_t)upper_bound(list.data(), n, (float)k / (float)kEnvGuide);
        vals.clear();
        push(vals, 0.f);
        push(vals, std::nextafterf(1.f, 0.f));
        push(vals, 1.f);
        for (int k = 0; k < kEnvGuide; k++) push3(vals, (float)k / (float)kEnvGuide);
        // distinct list values, evenly strided so that the cap keeps both ends of the list
        std::vector<float> distinct;
        for (int i = 0; i < n; i++)
            if (list[(size_t)i] == list[(size_t)i] && (distinct.empty() || list[(size_t)i] != distinct.back()))
                distinct.push_back(list[(size_t)i]);
        const size_t room = (kCap - vals.size()) / 3;
        const size_t step = room ? (distinct.size() + room - 1) / room : 0;
        for (size_t i = 0; step && i < distinct.size(); i += step) push3(vals, distinct[i]);
        if (!distinct.empty()) push3(vals, distinct.back());
        for (float v : vals) {
            const int a = upper_bound(list.data(), n, v);
            const int b = upper_bound_guided(list.data(), guide.data(), v);
            values++;
            if (a != b) {
                if (bad < 10) std::printf("list %d (n=%d) val=%.9g: upper_bound=%d guided=%d\n", l, n, (double)v, a, b);
                bad++;
            }
        }
    }
    std::fclose(f);
    std::printf("lists=%d values=%lld bad=%lld\n", count, values, bad);
    return bad ? 1 : 0;
}
