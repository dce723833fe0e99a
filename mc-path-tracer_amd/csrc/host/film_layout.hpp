// film_layout.hpp -- the sizing rules of the film, the path streams and the ray queues as pure host
// functions (no HIP call): what a film size, tile size, path-slot count, layout, tile set and any-hit
// multiplier make of the tile grid, the path count, the per-shard queue capacities and the k_shade
// block flags, and the limits with their messages.  film_state.cpp allocates from a FilmLayout; the
// iteration and the tables read it (tests/native/film_layout_host.cpp checks it without a device).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "kernels.hpp"

struct FilmLayout {
    // what it was computed from
    uint32_t W = 0, H = 0, tile_w = 0, tile_h = 0, slots = 1;
    bool compact = false;
    size_t ntiles = 0;      // tiles in the tile set
    uint32_t any_mult = 2;  // any-hit rays per material evaluation (3 with emitter sampling active)
    // what follows from it
    uint32_t nx = 0, ny = 0;  // tile grid of the film
    size_t npix = 0;          // W * H
    size_t npx = 0;           // pixels the path state covers: the film's, or in the compact layout the tile set's
    size_t paths = 0;         // slots * npx
    uint32_t blocks_per_tile = 0;       // k_shade blocks of one tile over its slots
    uint32_t ext_cap = 0, any_cap = 0;  // per-shard queue capacities
    size_t queue_need = 0;              // extension-queue entries (kShards * ext_cap)
    size_t blk_done_n = 0;              // k_shade block done flags: slots x film tiles x blocks per tile
    bool sum_planes = false;            // the W x H planes of the slot sums exist (slots > 1 or compact)
};

// Per-shard queue capacity for nblocks k_shade blocks: shard = block mod kShards, and a block pushes at most
// one ray per thread.  Never 0: an empty tile set keeps queues of one block per shard.
inline uint32_t shard_capacity(uint32_t nblocks) {
    return std::max<uint32_t>(1, (nblocks + mcpt_dev::kShards - 1) / mcpt_dev::kShards) * mcpt_dev::kBlock;
}
// ... that one tile needs (mcpt_wavefront_step's one-tile set)
inline uint32_t one_tile_capacity(uint32_t tile_w, uint32_t tile_h, uint32_t slots) {
    return shard_capacity((uint32_t)mcpt_dev::shade_blocks_per_tile((int)(tile_w * tile_h), (int)slots));
}

// nullptr, or why a film of this size and tile size is rejected
inline const char* film_size_error(uint32_t w, uint32_t h, uint32_t tw, uint32_t th) {
    if (w == 0 || h == 0 || tw == 0 || th == 0) return "bad film size";
    if ((uint64_t)w * h >= (1ull << 31)) return "film too large";
    if ((uint64_t)tw * th > (1ull << 26)) return "tile too large";
    return nullptr;
}

// The layout of an accepted film size (film_size_error)
inline FilmLayout film_layout(uint32_t w, uint32_t h, uint32_t tw, uint32_t th, uint32_t slots, bool compact, size_t ntiles,
                              uint32_t any_mult) {
    FilmLayout L;
    L.W = w, L.H = h, L.tile_w = tw, L.tile_h = th, L.slots = slots;
    L.compact = compact;
    L.ntiles = ntiles;
    L.any_mult = any_mult;
    L.nx = (w + tw - 1) / tw;
    L.ny = (h + th - 1) / th;
    L.npix = (size_t)w * h;
    L.npx = compact ? ntiles * (size_t)tw * th : L.npix;
    L.paths = L.npx * slots;
    L.blocks_per_tile = (uint32_t)mcpt_dev::shade_blocks_per_tile((int)(tw * th), (int)slots);
    L.ext_cap = shard_capacity((uint32_t)ntiles * L.blocks_per_tile);
    L.any_cap = any_mult * L.ext_cap;
    L.queue_need = (size_t)mcpt_dev::kShards * L.ext_cap;
    L.blk_done_n = slots * ((size_t)L.nx * L.ny) * (size_t)mcpt_dev::shade_blocks_per_tile((int)(tw * th), 1);
    L.sum_planes = slots > 1 || compact;
    return L;
}

// nullptr, or why the path state of npx pixels and this many slots is rejected (path indices are 31 bits)
inline const char* path_count_error(size_t npx, uint32_t slots) {
    return (uint64_t)npx * slots >= (1ull << 31) ? "film too large for the path slots" : nullptr;
}
// ... and why emitter sampling's 3-bytes-per-path any-hit results are
inline const char* emitter_paths_error(size_t paths) {
    return 3 * (uint64_t)paths >= (1ull << 32) ? "film too large for emitter sampling" : nullptr;
}
