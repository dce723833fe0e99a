// Host build of the spatial variance estimate's arithmetic (device/variance.hpp) for
// tests/test_variance_host.py:
//   variance_host W H radius sn sa sz min_neff use_samples use_variance in.bin out.bin
//       in.bin: rgb (3n float32), samples (n uint32), variance (n), albedo (3n), normal (3n), depth (n);
//       forms the planes (use_variance = 0: no variance is known), runs variance_pass_host and writes
//       the variances (n float32, -1 where unknown)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "device/variance.hpp"

static bool read_all(FILE* f, void* p, size_t bytes) { return fread(p, 1, bytes, f) == bytes; }

int main(int argc, char** argv) {
    if (argc != 12) {
        fprintf(stderr, "usage: variance_host W H radius sn sa sz min_neff use_samples use_variance in.bin out.bin\n");
        return 2;
    }
    const int W = atoi(argv[1]), H = atoi(argv[2]), radius = atoi(argv[3]);
    const float sn = (float)atof(argv[4]), sa = (float)atof(argv[5]), sz = (float)atof(argv[6]), min_neff = (float)atof(argv[7]);
    const bool use_samples = atoi(argv[8]) != 0, use_variance = atoi(argv[9]) != 0;
    if (W < 1 || H < 1 || radius < 1 || radius > 3) return 2;
    const size_t n = (size_t)W * H;
    std::vector<float> rgb(3 * n), var(n), al(3 * n), nm(3 * n), z(n);
    std::vector<uint32_t> sm(n);
    FILE* f = fopen(argv[10], "rb");
    if (!f) return 3;
    const bool rd = read_all(f, rgb.data(), 12 * n) && read_all(f, sm.data(), 4 * n) && read_all(f, var.data(), 4 * n) &&
                    read_all(f, al.data(), 12 * n) && read_all(f, nm.data(), 12 * n) && read_all(f, z.data(), 4 * n);
    fclose(f);
    if (!rd) return 3;
    std::vector<float4> col(n), gd(n), ap(n);
    std::vector<float2> vl(n);
    for (size_t i = 0; i < n; i++) {
        mcpt::dn_planes(rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2], use_samples ? sm[i] > 0 : true, nm[3 * i], nm[3 * i + 1],
                        nm[3 * i + 2], z[i], al[3 * i], al[3 * i + 1], al[3 * i + 2], col[i], gd[i], ap[i]);
        vl[i] = mcpt::dn_vl(col[i], use_variance ? var[i] : -1.f);
    }
    const mcpt::VariancePass k{mcpt::dn_k(sn), mcpt::dn_k(sa), mcpt::dn_k(sz), min_neff, radius};
    mcpt::variance_pass_host(k, W, H, col.data(), gd.data(), ap.data(), vl.data());
    std::vector<float> out(n);
    for (size_t i = 0; i < n; i++) out[i] = vl[i].x;
    f = fopen(argv[11], "wb");
    if (!f) return 3;
    const bool ok = fwrite(out.data(), sizeof(float), out.size(), f) == out.size();
    return (fclose(f) == 0 && ok) ? 0 : 3;
}
