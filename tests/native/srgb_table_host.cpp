// Host reader of the sRGB decode (device/texture.hpp) for tests/test_texture_srgb_host.py.
//   srgb_table_host                 prints the 256 table entries' bit patterns, one hex word per line
//   srgb_table_host IN OUT          the lookup over a file: int32 w, h, srgb, n, then w * h RGBA8 texels and n
//                                   float uv pairs; writes 3 n floats, tex_bilinear_rgba8_srgb(..., srgb != 0)
//                                   (srgb == 2: tex_bilinear_rgba8 itself, the unflagged entry point)
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "device/texture.hpp"

int main(int argc, char** argv) {
    if (argc == 1) {
        for (uint32_t c = 0; c < 256; c++) {
            const float v = mcpt::srgb_to_linear(c);
            uint32_t b;
            std::memcpy(&b, &v, 4);
            std::printf("%08x\n", b);
        }
        return 0;
    }
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hd[4];
    if (std::fread(hd, 4, 4, f) != 4 || hd[0] < 1 || hd[0] > 16384 || hd[1] < 1 || hd[1] > 16384 || hd[3] < 0 || hd[3] > (1 << 24)) return 2;
    std::vector<uint32_t> tex((size_t)hd[0] * hd[1]);
    std::vector<float> uv(2 * (size_t)hd[3]), out(3 * (size_t)hd[3]);
    if (std::fread(tex.data(), 4, tex.size(), f) != tex.size() || std::fread(uv.data(), 4, uv.size(), f) != uv.size()) return 2;
    std::fclose(f);
    for (int32_t i = 0; i < hd[3]; i++) {
        const mcpt::V3 t = hd[2] == 2 ? mcpt::tex_bilinear_rgba8(tex.data(), hd[0], hd[1], uv[2 * i], uv[2 * i + 1])
                                      : mcpt::tex_bilinear_rgba8_srgb(tex.data(), hd[0], hd[1], uv[2 * i], uv[2 * i + 1], hd[2] != 0);
        out[3 * i] = t.x, out[3 * i + 1] = t.y, out[3 * i + 2] = t.z;
    }
    f = std::fopen(argv[2], "wb");
    if (!f || std::fwrite(out.data(), 4, out.size(), f) != out.size()) return 2;
    std::fclose(f);
    return 0;
}
