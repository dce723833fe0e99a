// Host build of the variance-guided filter's arithmetic (device/denoise.hpp) for
// tests/test_denoise_guided_host.py:
//   denoise_guided_host W H passes sl eps sc sn sa sz use_samples in.bin out.bin
//       in.bin: rgb (3n float32), samples (n uint32), variance (n), albedo (3n), normal (3n), depth (n);
//       runs the passes with denoise_guided_pass_host and writes the filtered rgb (3n float32) and
//       the filtered variances (n float32, -1 where unknown)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "device/denoise.hpp"

static bool read_all(FILE* f, void* p, size_t bytes) { return fread(p, 1, bytes, f) == bytes; }

int main(int argc, char** argv) {
    if (argc != 13) {
        fprintf(stderr, "usage: denoise_guided_host W H passes sl eps sc sn sa sz use_samples in.bin out.bin\n");
        return 2;
    }
    const int W = atoi(argv[1]), H = atoi(argv[2]), passes = atoi(argv[3]);
    const float sl = (float)atof(argv[4]), eps = (float)atof(argv[5]), sc0 = (float)atof(argv[6]), sn = (float)atof(argv[7]),
                sa = (float)atof(argv[8]), sz = (float)atof(argv[9]);
    const bool use_samples = atoi(argv[10]) != 0;
    if (W < 1 || H < 1 || passes < 1 || passes > 8) return 2;
    const size_t n = (size_t)W * H;
    std::vector<float> rgb(3 * n), var(n), al(3 * n), nm(3 * n), z(n);
    std::vector<uint32_t> sm(n);
    FILE* f = fopen(argv[11], "rb");
    if (!f) return 3;
    const bool rd = read_all(f, rgb.data(), 12 * n) && read_all(f, sm.data(), 4 * n) && read_all(f, var.data(), 4 * n) &&
                    read_all(f, al.data(), 12 * n) && read_all(f, nm.data(), 12 * n) && read_all(f, z.data(), 4 * n);
    fclose(f);
    if (!rd) return 3;
    std::vector<float4> col[2] = {std::vector<float4>(n), std::vector<float4>(n)}, gd(n), ap(n);
    std::vector<float2> vl[2] = {std::vector<float2>(n), std::vector<float2>(n)};
    for (size_t i = 0; i < n; i++) {
        mcpt::dn_planes(rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2], use_samples ? sm[i] > 0 : true, nm[3 * i], nm[3 * i + 1],
                        nm[3 * i + 2], z[i], al[3 * i], al[3 * i + 1], al[3 * i + 2], col[0][i], gd[i], ap[i]);
        vl[0][i] = mcpt::dn_vl(col[0][i], var[i]);
    }
    int src = 0;
    float sc = sc0;
    for (int i = 0; i < passes; i++) {
        const mcpt::DenoiseGuidedPass k{{mcpt::dn_k(sc), mcpt::dn_k(sn), mcpt::dn_k(sa), mcpt::dn_k(sz), 1 << i}, sl, eps};
        mcpt::denoise_guided_pass_host(k, W, H, col[src].data(), vl[src].data(), gd.data(), ap.data(), col[src ^ 1].data(),
                                       vl[src ^ 1].data());
        src ^= 1;
        sc = sc * 0.5f;
    }
    std::vector<float> out(4 * n);
    for (size_t i = 0; i < n; i++) {
        out[3 * i] = col[src][i].x;
        out[3 * i + 1] = col[src][i].y;
        out[3 * i + 2] = col[src][i].z;
        out[3 * n + i] = vl[src][i].x;
    }
    f = fopen(argv[12], "wb");
    if (!f) return 3;
    const bool ok = fwrite(out.data(), sizeof(float), out.size(), f) == out.size();
    return (fclose(f) == 0 && ok) ? 0 : 3;
}
