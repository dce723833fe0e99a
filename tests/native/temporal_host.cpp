// Host build of the temporal stage's arithmetic (device/temporal.hpp) for tests/test_temporal_host.py:
//   temporal_host W H pos_tol nrm_tol max_history alpha_min in.bin out.bin
//       in.bin: rgb (3n float32), samples (n uint32), variance (n), position (3n), normal (3n), depth (n),
//       hcol (4n), hpos (4n), hnrm (4n), VP_prev (16, column-major); runs temporal_pass_host and writes
//       col (4n float32), vl (2n), and the new hcol, hpos, hnrm (4n each)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "device/temporal.hpp"

static bool read_all(FILE* f, void* p, size_t bytes) { return fread(p, 1, bytes, f) == bytes; }
static bool write_all(FILE* f, const void* p, size_t bytes) { return fwrite(p, 1, bytes, f) == bytes; }

int main(int argc, char** argv) {
    if (argc != 9) {
        fprintf(stderr, "usage: temporal_host W H pos_tol nrm_tol max_history alpha_min in.bin out.bin\n");
        return 2;
    }
    const int W = atoi(argv[1]), H = atoi(argv[2]);
    const mcpt::TemporalParams k{(float)atof(argv[3]), (float)atof(argv[4]), (float)atof(argv[5]), (float)atof(argv[6])};
    if (W < 1 || H < 1) return 2;
    const size_t n = (size_t)W * H;
    std::vector<float> rgb(3 * n), var(n), pos(3 * n), nm(3 * n), z(n);
    std::vector<uint32_t> sm(n);
    std::vector<float4> hcol(n), hpos(n), hnrm(n);
    float vp[16];
    FILE* f = fopen(argv[7], "rb");
    if (!f) return 3;
    const bool rd = read_all(f, rgb.data(), 12 * n) && read_all(f, sm.data(), 4 * n) && read_all(f, var.data(), 4 * n) &&
                    read_all(f, pos.data(), 12 * n) && read_all(f, nm.data(), 12 * n) && read_all(f, z.data(), 4 * n) &&
                    read_all(f, hcol.data(), 16 * n) && read_all(f, hpos.data(), 16 * n) && read_all(f, hnrm.data(), 16 * n) &&
                    read_all(f, vp, sizeof(vp));
    fclose(f);
    if (!rd) return 3;
    std::vector<mcpt::TpPixel> cur(n);
    for (size_t i = 0; i < n; i++)
        cur[i] = mcpt::tp_pixel(rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2], sm[i] > 0, (float)sm[i], var[i],
                                mcpt::v3(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]),
                                mcpt::v3(nm[3 * i], nm[3 * i + 1], nm[3 * i + 2]), z[i]);
    std::vector<float4> col(n), ohc(n), ohp(n), ohn(n);
    std::vector<float2> vl(n);
    mcpt::temporal_pass_host(k, W, H, vp, cur.data(), hcol.data(), hpos.data(), hnrm.data(), col.data(), vl.data(), ohc.data(),
                             ohp.data(), ohn.data());
    f = fopen(argv[8], "wb");
    if (!f) return 3;
    const bool ok = write_all(f, col.data(), 16 * n) && write_all(f, vl.data(), 8 * n) && write_all(f, ohc.data(), 16 * n) &&
                    write_all(f, ohp.data(), 16 * n) && write_all(f, ohn.data(), 16 * n);
    return (fclose(f) == 0 && ok) ? 0 : 3;
}
