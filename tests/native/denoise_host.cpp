// Host build of the denoiser's arithmetic (device/denoise.hpp) for tests/test_denoise_host.py:
//   denoise_host exp N out.bin
//       dexp_neg over the grid x_i = 100 i / (N - 1), i < N (float32), then a few values past the
//       underflow point; writes x and dexp_neg(x) as float32 pairs
//   denoise_host filter W H passes sc sn sa sz use_samples in.bin out.bin
//       in.bin: rgb (3n float32), samples (n uint32), albedo (3n), normal (3n), depth (n); runs the
//       passes with denoise_pass_host and writes the filtered rgb (3n float32)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "device/denoise.hpp"

static bool read_all(FILE* f, void* p, size_t bytes) { return fread(p, 1, bytes, f) == bytes; }

int main(int argc, char** argv) {
    if (argc == 4 && !strcmp(argv[1], "exp")) {
        const long N = atol(argv[2]);
        if (N < 2) return 2;
        std::vector<float> out;
        for (long i = 0; i < N; i++) {
            const float x = (float)(100.0 * (double)i / (double)(N - 1));
            out.push_back(x);
            out.push_back(mcpt::dexp_neg(x));
        }
        for (float x : {87.3f, 87.33654f, 87.4f, 87.5f, 88.f, 104.f, 1e3f, 1e30f, __builtin_huge_valf()}) {
            out.push_back(x);
            out.push_back(mcpt::dexp_neg(x));
        }
        FILE* f = fopen(argv[3], "wb");
        if (!f) return 3;
        const bool ok = fwrite(out.data(), sizeof(float), out.size(), f) == out.size();
        return (fclose(f) == 0 && ok) ? 0 : 3;
    }
    if (argc == 12 && !strcmp(argv[1], "filter")) {
        const int W = atoi(argv[2]), H = atoi(argv[3]), passes = atoi(argv[4]);
        const float sc0 = (float)atof(argv[5]), sn = (float)atof(argv[6]), sa = (float)atof(argv[7]), sz = (float)atof(argv[8]);
        const bool use_samples = atoi(argv[9]) != 0;
        if (W < 1 || H < 1 || passes < 1 || passes > 8) return 2;
        const size_t n = (size_t)W * H;
        std::vector<float> rgb(3 * n), al(3 * n), nm(3 * n), z(n);
        std::vector<uint32_t> sm(n);
        FILE* f = fopen(argv[10], "rb");
        if (!f) return 3;
        const bool rd = read_all(f, rgb.data(), 12 * n) && read_all(f, sm.data(), 4 * n) && read_all(f, al.data(), 12 * n) &&
                        read_all(f, nm.data(), 12 * n) && read_all(f, z.data(), 4 * n);
        fclose(f);
        if (!rd) return 3;
        std::vector<float4> col[2] = {std::vector<float4>(n), std::vector<float4>(n)}, gd(n), ap(n);
        for (size_t i = 0; i < n; i++)
            mcpt::dn_planes(rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2], use_samples ? sm[i] > 0 : true, nm[3 * i], nm[3 * i + 1],
                            nm[3 * i + 2], z[i], al[3 * i], al[3 * i + 1], al[3 * i + 2], col[0][i], gd[i], ap[i]);
        int src = 0;
        float sc = sc0;
        for (int i = 0; i < passes; i++) {
            const mcpt::DenoisePass k{mcpt::dn_k(sc), mcpt::dn_k(sn), mcpt::dn_k(sa), mcpt::dn_k(sz), 1 << i};
            mcpt::denoise_pass_host(k, W, H, col[src].data(), gd.data(), ap.data(), col[src ^ 1].data());
            src ^= 1;
            sc = sc * 0.5f;
        }
        std::vector<float> out(3 * n);
        for (size_t i = 0; i < n; i++) { out[3 * i] = col[src][i].x; out[3 * i + 1] = col[src][i].y; out[3 * i + 2] = col[src][i].z; }
        f = fopen(argv[11], "wb");
        if (!f) return 3;
        const bool ok = fwrite(out.data(), sizeof(float), out.size(), f) == out.size();
        return (fclose(f) == 0 && ok) ? 0 : 3;
    }
    fprintf(stderr, "usage: denoise_host exp N out.bin | filter W H passes sc sn sa sz use_samples in.bin out.bin\n");
    return 2;
}
