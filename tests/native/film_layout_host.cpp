// film_layout_host.cpp -- the film-state sizing rules (csrc/host/film_layout.hpp) as a stand-alone host
// program: a fixed list of cases, one output line each with the inputs and every field of the layout, or
// the rejection's message.  tests/test_film_layout_host.py recomputes the fields.  No device.
#include <cinttypes>
#include <cstdio>

#include "host/film_layout.hpp"

struct Case {
    const char* name;
    uint32_t w, h, tw, th, slots;
    int compact;
    uint64_t ntiles;  // ~0: every tile of the grid
    uint32_t mult;
};

static const Case kCases[] = {
    {"empty_set", 96, 80, 32, 32, 1, 0, 0, 2},
    {"empty_set_compact", 96, 80, 32, 32, 3, 1, 0, 3},
    {"one_pixel", 1, 1, 1, 1, 1, 0, ~0ull, 2},
    {"ragged", 33, 17, 16, 16, 1, 0, ~0ull, 2},
    {"ragged_3_slots", 33, 17, 16, 16, 3, 0, ~0ull, 3},
    {"slots_256", 96, 80, 16, 16, 256, 0, ~0ull, 2},
    {"mult_2", 1920, 1080, 256, 256, 8, 0, ~0ull, 2},
    {"mult_3", 1920, 1080, 256, 256, 8, 0, ~0ull, 3},
    {"compact_subset", 200, 120, 64, 64, 3, 1, 3, 2},
    {"compact_subset_mult_3", 72, 40, 16, 16, 2, 1, 5, 3},
    {"one_tile_17_slots", 96, 80, 32, 32, 17, 0, 1, 2},
    {"paths_2p31_minus_1", 2147483647u, 1, 256, 256, 1, 0, 0, 2},
    {"paths_2p31", 1u << 30, 1, 256, 256, 2, 0, 0, 2},
    {"paths_2p31_compact", 4096, 4096, 8192, 8192, 32, 1, 1, 2},
    {"emitter_below_2p32", 1431655765u, 1, 256, 256, 1, 0, 0, 3},
    {"emitter_at_2p32", 1431655766u, 1, 256, 256, 1, 0, 0, 3},
    {"film_2p31", 1u << 16, 1u << 15, 256, 256, 1, 0, 0, 2},
    {"tile_2p26", 64, 64, 8192, 8192, 1, 0, ~0ull, 2},
    {"tile_2p26_plus_1", 64, 64, 5, 13421773, 1, 0, ~0ull, 2},
    {"zero_width", 0, 8, 16, 16, 1, 0, 0, 2},
    {"zero_tile", 8, 8, 16, 0, 1, 0, 0, 2},
};

int main() {
    for (const Case& k : kCases) {
        printf("%s in=%u,%u,%u,%u,%u,%d,%" PRId64 ",%u", k.name, k.w, k.h, k.tw, k.th, k.slots, k.compact, (int64_t)k.ntiles, k.mult);
        if (const char* e = film_size_error(k.w, k.h, k.tw, k.th)) {
            printf(" size_error=\"%s\"\n", e);
            continue;
        }
        const uint64_t grid = (uint64_t)((k.w + k.tw - 1) / k.tw) * ((k.h + k.th - 1) / k.th);
        const FilmLayout L = film_layout(k.w, k.h, k.tw, k.th, k.slots, k.compact != 0, (size_t)(k.ntiles == ~0ull ? grid : k.ntiles), k.mult);
        const char* pe = path_count_error(L.npx, L.slots);
        const char* ee = emitter_paths_error(L.paths);
        printf(" ntiles=%zu nx=%u ny=%u npix=%zu npx=%zu paths=%zu blocks_per_tile=%u ext_cap=%u any_cap=%u queue_need=%zu"
               " blk_done_n=%zu sum_planes=%d one_tile_cap=%u paths_error=\"%s\" emitter_error=\"%s\"\n",
               L.ntiles, L.nx, L.ny, L.npix, L.npx, L.paths, L.blocks_per_tile, L.ext_cap, L.any_cap, L.queue_need, L.blk_done_n,
               L.sum_planes ? 1 : 0, one_tile_capacity(k.tw, k.th, k.slots), pe ? pe : "", ee ? ee : "");
    }
    return 0;
}
