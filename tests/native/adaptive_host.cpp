// Host build of adaptive sampling's arithmetic (device/adaptive.hpp) for tests/test_adaptive_host.py:
//   adaptive_host error S N in.bin out.bin
//       in.bin: Ld (S * N * 3 float32, slot-major), n (S * N uint32); writes film_error_pixel of the N
//       pixels (4 N float32)
//   adaptive_host budget N tau_bits floor_bits min_spp max_spp in.bin out.bin
//       in.bin: estimates (4 N float32), owned (N bytes); tau and lum_floor as float32 bit patterns;
//       writes budget_pixel of the N pixels (N uint32)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "device/adaptive.hpp"

static bool read_all(FILE* f, void* p, size_t bytes) { return fread(p, 1, bytes, f) == bytes; }
static bool write_file(const char* path, const void* p, size_t bytes) {
    FILE* f = fopen(path, "wb");
    if (!f) return false;
    const bool ok = fwrite(p, 1, bytes, f) == bytes;
    return fclose(f) == 0 && ok;
}
static float from_bits(const char* s) {
    const uint32_t u = (uint32_t)strtoul(s, nullptr, 10);
    float f;
    memcpy(&f, &u, 4);
    return f;
}

int main(int argc, char** argv) {
    if (argc == 6 && !strcmp(argv[1], "error")) {
        const int S = atoi(argv[2]);
        const long N = atol(argv[3]);
        if (S < 1 || S > 256 || N < 1) return 2;
        const size_t n = (size_t)N;
        std::vector<float> rgb(3 * n * S);
        std::vector<uint32_t> ns(n * S);
        FILE* f = fopen(argv[4], "rb");
        if (!f) return 3;
        const bool rd = read_all(f, rgb.data(), 4 * rgb.size()) && read_all(f, ns.data(), 4 * ns.size());
        fclose(f);
        if (!rd) return 3;
        std::vector<float4> Ld(n * S), out(n);
        for (size_t i = 0; i < n * S; i++) Ld[i] = make_float4(rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2], 0.f);
        for (size_t i = 0; i < n; i++) out[i] = mcpt::film_error_pixel(Ld.data(), ns.data(), n, i, S);
        return write_file(argv[5], out.data(), out.size() * sizeof(float4)) ? 0 : 3;
    }
    if (argc == 9 && !strcmp(argv[1], "budget")) {
        const long N = atol(argv[2]);
        if (N < 1) return 2;
        const size_t n = (size_t)N;
        const mcpt::BudgetParams p{from_bits(argv[3]), from_bits(argv[4]), (uint32_t)strtoul(argv[5], nullptr, 10),
                                   (uint32_t)strtoul(argv[6], nullptr, 10)};
        std::vector<float4> e(n);
        std::vector<unsigned char> owned(n);
        FILE* f = fopen(argv[7], "rb");
        if (!f) return 3;
        const bool rd = read_all(f, e.data(), n * sizeof(float4)) && read_all(f, owned.data(), n);
        fclose(f);
        if (!rd) return 3;
        std::vector<uint32_t> out(n);
        for (size_t i = 0; i < n; i++) out[i] = mcpt::budget_pixel(e[i], owned[i] != 0, p);
        return write_file(argv[8], out.data(), 4 * n) ? 0 : 3;
    }
    fprintf(stderr, "usage: adaptive_host error S N in.bin out.bin | budget N tau_bits floor_bits min max in.bin out.bin\n");
    return 2;
}
