// The PNG reader (host/png_read.cpp) over damaged files, as a stand-alone CPU program for
// tests/test_png_read_host.py, which also builds and runs it under the host's address and undefined-behaviour
// sanitizers.  Usage: png_read_host SEED CASES FILE...
// Every FILE must decode.  Then the decoder is fed every prefix of the file, and CASES copies of it with one
// byte changed: byte k mod size in turn, xor a non-zero value drawn from SEED.  Each case must either decode
// (MCPT_OK, any pixels) or be refused with MCPT_E_IO, a reason, and the output buffer, w and h untouched.
// Prints "files=F prefixes=P flips=N decoded=D refused=R bad=B" and exits 1 if bad != 0.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mcpt.h"

static uint64_t rng_state;
static uint32_t rng() {  // splitmix64's output function over a counter
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (uint32_t)((z ^ (z >> 31)) >> 32);
}

static long long decoded = 0, refused = 0, bad = 0;

// One damaged input; cap bytes of output as the intact file needs
static void feed(const uint8_t* d, size_t n, size_t cap) {
    std::vector<uint8_t> out(cap, 0xA5);
    int32_t w = -7, h = -9;
    // (an empty prefix is given as a valid pointer with n == 0: NULL data is MCPT_E_INVALID by contract)
    static const uint8_t none = 0;
    const int rc = mcpt_image_read_png_memory(n ? d : &none, n, &w, &h, out.data(), cap);
    if (rc == MCPT_OK) {
        decoded++;
        if (w < 1 || h < 1 || (size_t)w * (size_t)h * 4 > cap) bad++;
        return;
    }
    bool clean = w == -7 && h == -9;
    for (size_t i = 0; clean && i < cap; i++) clean = out[i] == 0xA5;
    // a flipped IHDR may ask for a larger image than the buffer holds: MCPT_E_INVALID, nothing written either
    const bool ok = (rc == MCPT_E_IO && mcpt_image_read_png_error()[0] != 0) || rc == MCPT_E_INVALID;
    if (ok && clean) refused++;
    else {
        if (bad < 10) std::printf("bad case: rc=%d clean=%d n=%zu\n", rc, (int)clean, n);
        bad++;
    }
}

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    rng_state = std::strtoull(argv[1], nullptr, 0);
    const long cases = std::atol(argv[2]);
    long long prefixes = 0, flips = 0;
    for (int a = 3; a < argc; a++) {
        FILE* f = std::fopen(argv[a], "rb");
        if (!f) return 2;
        std::vector<uint8_t> d;
        uint8_t buf[4096];
        size_t got;
        while ((got = std::fread(buf, 1, sizeof buf, f)) > 0) d.insert(d.end(), buf, buf + got);
        std::fclose(f);
        int32_t w = 0, h = 0;
        if (mcpt_image_read_png_memory(d.data(), d.size(), &w, &h, nullptr, 0) != MCPT_OK) {
            std::printf("%s: the intact file's header is refused: %s\n", argv[a], mcpt_image_read_png_error());
            return 1;
        }
        const size_t cap = (size_t)w * (size_t)h * 4;
        std::vector<uint8_t> px(cap);
        if (mcpt_image_read_png_memory(d.data(), d.size(), &w, &h, px.data(), cap) != MCPT_OK) {
            std::printf("%s: the intact file is refused: %s\n", argv[a], mcpt_image_read_png_error());
            return 1;
        }
        for (size_t n = 0; n < d.size(); n++, prefixes++) {
            std::vector<uint8_t> p(d.begin(), d.begin() + n);  // (its own allocation: a read past n is a sanitizer error)
            feed(p.data(), n, cap);
        }
        for (long k = 0; k < cases; k++, flips++) {
            std::vector<uint8_t> p(d);
            uint8_t x = (uint8_t)rng();
            if (!x) x = 0x80;
            p[(size_t)k % p.size()] ^= x;
            feed(p.data(), p.size(), cap);
        }
    }
    std::printf("files=%d prefixes=%lld flips=%lld decoded=%lld refused=%lld bad=%lld\n", argc - 3, prefixes, flips, decoded, refused, bad);
    return bad ? 1 : 0;
}
