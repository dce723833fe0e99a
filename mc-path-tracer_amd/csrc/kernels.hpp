// kernels.hpp -- device data layout shared by the .hip files and the host runtime (runtime.cpp).
//
// HBM layout (P = slots * W*H paths; slot 0 is the reference's one path per pixel, path_id ==
// pixel_id, wavefront_kernels.cu:108,114).  The reference's Paths is an array-of-structs with a
// 128-B Isect and a 32-B dRay per path (Wavefront.cuh:8-26); here every field is a separate
// 16-B-aligned stream so a wave64 access is one coalesced 1 KiB dwordx4 transaction.  (Records
// that pack a path's fields together -- 32-B rays, 64-B {beta, nee0, nee1, Ld} -- move fewer HBM
// bytes on the sparse accesses but cost more lines per wave instruction, and measured slower:
// k_material 248 -> 302 ms, k_shade 139 -> 193 ms per three config-2 frames)
//   ray_o/ray_d   float4 [P]    extension ray (xyz, pad)
//   hit_tri       i32    [P]    closest triangle of the extension ray (-1 = miss); the hit
//                               record (isect) is rebuilt from it where it is consumed
//   sray_o/sray_d float4 [2Q]   any-hit rays at their any-queue position (Q = queue entries,
//                               allocated with the queues): written densely by k_material after
//                               its block push, read densely by k_trace; the queue entry itself
//                               holds the result index 2p (light sample) / 2p+1 (BRDF visibility).
//   beta          float4 [P]    throughput, (f_sample/pdf_sample).x
//   nee0 / nee1   float4 [P]    precomputed light / BRDF MIS terms, ratio .y / .z
//   flags         u32    [P]    dead, len, MIS condition bits, the path's sample index (bits 13..31)
//   vis           u8     [2P]   any-hit results ([3P] while emitter sampling is active: the emitter
//                               ray of path p at 2P + p)
//   nee2          float4 [P]    the emitter sample's term (only while emitter sampling is active); .w: 0, or
//                               with MIS (section 18) the pdf of the continuation direction
//   samples       u32    [P]    film sample count (dFilm.samples)
//   Ld            float4 [P]    film radiance (dFilm.Ld)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device/adaptive.hpp"
#include "device/denoise.hpp"
#include "device/mcpt_core.hpp"
#include "device/occ_beam.hpp"
#include "device/temporal.hpp"
#include "device/texture.hpp"
#include "device/variance.hpp"

namespace mcpt_dev {

constexpr int kBlock = 256;
constexpr int kTraceBlock = 64;  // one wave per traversal block
#ifndef MCPT_LDS_STACK
#define MCPT_LDS_STACK 8
#endif
constexpr int kLdsStack = MCPT_LDS_STACK;  // traversal stack entries per lane kept in LDS (deeper: scratch)
#ifndef MCPT_LDS_STACK_DEEP
#define MCPT_LDS_STACK_DEEP 10
#endif
constexpr int kLdsStackDeep = MCPT_LDS_STACK_DEEP;  // the same for trees deeper than kDeepTree levels
constexpr int kLdsStackTiny = 2;  // test instantiation (mcpt_debug_tiny_lds_stack): pushes beyond 2 go to scratch
#ifndef MCPT_DEEP_TREE
#define MCPT_DEEP_TREE 20
#endif
constexpr int kDeepTree = MCPT_DEEP_TREE;  // stack pushes beyond which the deep-stack k_trace runs
constexpr int kMaxStack = 64;  // total (reference: int nodesToVisit[64], Triangle.cu:161)

enum : uint32_t {
    F_DEAD = 1u,
    F_LEN_SHIFT = 1,        // bits 1..8
    F_CONDL = 1u << 9,      // light-sample MIS term valid (w > 0 && pdf > 0)
    F_CONDB = 1u << 10,     // BRDF-sample MIS term valid when visible
    F_FZERO = 1u << 11,     // f_sample == 0 || pdf_sample == 0
    F_HASVIS = 1u << 12,    // non-delta light: a BRDF visibility ray was traced
    F_SIDX_SHIFT = 13       // bits 13..31: the sample index the path renders (RNG key); a dead
                            // path's next one (k_shade derives the film's sample count from it)
};
constexpr uint32_t kMaxSpp = 1u << (32 - F_SIDX_SHIFT);  // sample indices must fit the flags word
constexpr int kRecLenShift = 24;  // material record word 2: sample index (< kMaxSpp) | len << 24 (len < 256)
static_assert(kMaxSpp <= (1u << kRecLenShift), "sample index and len share a record word");
// Material record word 2, "no continuation" (between the sample index and len): the next logic pass is
// certain to end the path by Russian roulette, so k_material evaluates no continuation sample
// (ShadeArgs::skip)
constexpr uint32_t kRecNoCont = 1u << 23;
static_assert(kMaxSpp <= kRecNoCont && kRecNoCont < (1u << kRecLenShift), "the mark lies between sample index and len");

// k_shade blocks: kBlock consecutive pixels of one path slot; slot k's blocks follow slot k-1's
__host__ __device__ constexpr int shade_blocks_per_tile(int tile_px, int slots) {
    return (tile_px + kBlock - 1) / kBlock * slots;
}

// BVH node width of the traversal, per scene (DevScene::width): width 2, child-pair
// nodes, 4 x float4 (per axis (mn0, mn1, mx0, mx1), then refs); width 4, 8 x float4:
// mn.x[4], mx.x[4], mn.y[4], mx.y[4], mn.z[4], mx.z[4], refs[4] (kEnd = empty), pad.
// float4 per triangle intersection record: 3 (48 B, packed) or 4 (64 B: a record never
// straddles two 64-B halves of a cache line; MCPT_TRI_F4)
#ifndef MCPT_TRI_F4
#define MCPT_TRI_F4 3
#endif
constexpr int kTriF4 = MCPT_TRI_F4;

struct DevScene {
    const float4* nodes;    // BVH nodes (width children each: 4 or 8 float4)
    const float4* tri;      // kTriF4 x float4: (v0.xyz, e1.x) (e1.yz, e2.xy) (e2.z, id, -, -) [pad]; id = tri_id bits
    const float4* tri_sh;   // 3 x float4: (n0.xyz, n1.x) (n1.yz, n2.xy) (n2.z, mat, -, -)
    float root_mn[3], root_mx[3];
    int root_ref;           // >= 0 pair node, < 0 leaf (0x80000000 | (count-1)<<24 | offset)
    int depth;              // bound on stack pushes of the uploaded tree: picks the k_trace instantiation
    int width;              // node width: 2 (child pairs) or 4 (quads)
    int nlights;            // 1 + ndir (Scene.cu:370-388)
    const float* mats;      // 8 floats per material
    const float* dirs;      // 7 floats per directional light
    mcpt::EnvView env;
    // Any-hit occluder cache: occ[kOccWays i + w] is a triangle record
    // that occluded an any-hit ray of cell i (origin cell of the root box x direction bin), or
    // kOccEmpty; occ_rec[kOccRecF4 t ..] is triangle t's occluder record: the box of the BVH leaf
    // that holds it with that leaf's culling margin, and the triangle (v0, e1, e2), 64 B.
    // k_material tests an any-hit ray against its cell's triangle under that leaf box first:
    // a hit there is one the traversal would find too, so the ray is resolved as occluded.
    // occ == nullptr: off.
    uint32_t* occ;
    // The lookup gate, kOccGateWords words kept with the table (all reset at upload and with the film): [0] skip: k_material skips the lookups while nonzero; k_accumulate
    // sets it to [1] after an iteration whose lookups resolved under 1 in kOccMinRate of the rays
    // tested and counts it down one per iteration; k_trace records occluders only while it is <= 1,
    // so the next lookups meet a fresh table.  [1] backoff: 15, 31, 63, ... 255 after consecutive
    // failed lookup iterations, 0 while they pay.  [2] warm: set by the first iteration that traced
    // any-hit rays (and so recorded occluders into the table the film clear emptied); k_material
    // looks nothing up before it.  (Round 6: the lookups against the empty table used to be judged,
    // which closed the gate for the frame's biggest iterations, 2-4 -- at N = 8 most of a rank's
    // frame.)
    uint32_t* occ_gate;
    const float4* occ_rec;
    uint32_t ntri;
    int occ_g, occ_b;       // origin cells per axis, direction bins per face coordinate
    float occ_inv[3];       // occ_g / root box extent, per axis
    // Complete keys (device/occ_beam.hpp): an entry whose words all carry
    // kOccDoneBit holds every triangle a ray of the key's beam can be accepted on, so k_material
    // resolves such a ray either way.  occ_dir: the direction-bin table of the keys' beams (OccGrid::dir;
    // nullptr: no complete keys, MCPT_OCC_COMPLETE=0), occ_cell the origin cells' extent per axis.
    const float4* occ_dir;
    float occ_cell[3];
    // Conservative culling (mcpt_core.hpp "conservative box culling"): every node holds each
    // child's margin W (pair nodes: q3.z / q3.w; 4-wide nodes: float4 7; occ_rec[4t].w), P is the
    // scene's far coefficient, root_w the root box's margin.  cull_ok = 0 (a caller BVH whose boxes
    // do not contain their triangles, or MCPT_CULL=0): nothing is culled.
    float cull_p, root_w;
    int cull_ok;
};
// "0" at upload: no complete keys (A/B runs, tests).  As with kPrimaryHitsEnv below, bench.py has no entry
// for it and stamps a run that sets it as an unknown knob, i.e. not the product.
constexpr char kOccCompleteEnv[] = "MCPT_OCC_COMPLETE";
constexpr uint32_t kOccEmpty = 0xffffffffu;
#ifndef MCPT_OCC_WAYS
#define MCPT_OCC_WAYS 2  // 4: 16-B entries, measured and not kept (tools/experiments/INDEX.md, occ_ways4.patch)
#endif
constexpr uint32_t kOccWays = MCPT_OCC_WAYS;  // entries per cell: k_trace writes way tri mod kOccWays, k_material tests all
static_assert(kOccWays == 2 || kOccWays == 4, "an entry is one 8-B or 16-B load");
                                      // (1 way resolved 52 % of config 2's any-hit rays, 2 ways 64 %)
constexpr uint32_t kOccGateWords = 3;  // DevScene::occ_gate
constexpr uint32_t kOccMinRate = 10;  // lookups pay when >= 1 in kOccMinRate resolves a ray (see occ_skip)
__host__ __device__ constexpr size_t occ_entries(int g, int b) { return (size_t)g * g * g * 6 * b * b * kOccWays; }

struct DevPaths {
    float4 *ray_o, *ray_d, *sray_o, *sray_d, *beta, *nee0, *nee1, *Ld;
    int32_t* hit_tri;  // closest hit of the extension ray (-1: none); k_shade rebuilds the hit record
    uint32_t *flags, *samples;
    uint8_t* vis;
};

// Queue counters and statistics are sharded over kShards cache lines (one
// shard per k_shade block mod kShards): a single counter word serialises at
// roughly 90 atomics per microsecond, which is what ~24K pushes and ~100K
// statistics adds per iteration would otherwise cost.
constexpr int kShards = 64;
constexpr int kMaxParts = kShards;  // k_trace work partitions (at most one per queue shard)
enum : int { C_EXT = 0, C_ANY = 1, C_VIS = 2, C_STATS = 3, C_EXT_RAYS = 9, C_ANY_RAYS = 10, C_MAT = 11, C_OCC = 12,
              C_OCC_TRY = 13, C_PH = 14, C_SKIP_INPLACE = 25, C_PRIM = 26, C_PRIM_RAYS = 27, C_SKIP_EXT = 28,
              C_SKIP_ANY = 29, C_SKIP_MAT = 30, C_OCC_DONE_VIS = 31, C_OCC_DONE_OCC = 32, C_WORDS = 64 };
// C_STATS..+5; C_OCC / C_OCC_TRY: any-hit rays resolved by / tested against the occluder cache;
// C_PH..+kPhaseWords-1: k_trace's loop-phase counts (counting build, PH_*); C_PRIM: primary-queue
// pushes (k_shade -> k_primary), C_PRIM_RAYS: primary rays resolved from the candidate table
// C_SKIP_EXT / C_SKIP_ANY / C_SKIP_MAT: extension rays, any-hit rays and material evaluations of
// paths the next logic pass discards, counted as rays but not made (ShadeArgs::skip);
// C_SKIP_INPLACE: with the switch off, such paths' extension rays that were resolved in place
// C_OCC_DONE_VIS / C_OCC_DONE_OCC: any-hit rays resolved from complete entries of the occluder table as
// unoccluded (counted as rays only: neither traversed nor in C_OCC) / as occluded (also part of C_OCC)
// k_trace loop-phase counts of the counting instantiation (mcpt_debug_trace_profile), per wave summed:
enum : int {
    PH_TRIPS = 0,          // loop trips with a ray in the wave
    PH_REFILLS = 1,        // refill events
    PH_REFILL_LANES = 2,   // lanes handed a ray by them
    PH_NODE_ITERS = 3,     // node-phase wave iterations (per trip: the most steps any lane took, <= kNodeSteps)
    PH_TRI_PHASES = 4,     // triangle phases run
    PH_TRI_LANES = 5,      // lanes that tested a triangle in them
    PH_TRIP_NODE = 6,      // lanes with node work at a trip's start
    PH_TRIP_LEAF = 7,      // lanes holding a parked leaf at a trip's start
    PH_TRIP_IDLE = 8,      // lanes without a ray at a trip's start (after the refill)
    PH_FINISH_TRIPS = 9,   // trips in which at least one lane finished its ray
    PH_POP_ITERS = 10,     // node-phase wave iterations in which at least one lane popped the stack
    kPhaseWords = 11
};
struct CounterBlock {
    uint32_t shard[kShards][C_WORDS];  // [0] ext pushes [1] any-hit pushes [2] vis rays [3..8] traversal stats [9,10] rays [11] material pushes
    uint32_t last_ext, last_live;
    uint32_t trace_short;  // k_trace launches that left a partition's rays untraced (k_accumulate; must stay 0)
    uint32_t idle;         // set by k_accumulate after an iteration with no ray: the tile set is complete, so
                           // the remaining iterations of the call skip their kernels (run_iterations resets it)
    uint32_t pad[28];
    uint32_t last_ext_shard[kShards];  // per-shard extension pushes of the last iteration
    uint32_t grab[kMaxParts][C_WORDS];  // k_trace ray hand-out, one counter line per partition
    unsigned long long tot_ext, tot_any, tot_vis, tot_occ;
    unsigned long long tot_stats[6];
    unsigned long long tot_ext_q, tot_any_q;  // rays queued to k_trace (the rest were resolved in place)
    unsigned long long tot_phase[kPhaseWords];  // k_trace loop-phase counts (PH_*; counting build only)
    unsigned long long tot_prim;  // primary rays resolved from the candidate table (part of tot_ext)
    unsigned long long tot_skip[4];  // C_SKIP_EXT, C_SKIP_ANY, C_SKIP_MAT, C_SKIP_INPLACE
    unsigned long long tot_done[2];  // C_OCC_DONE_VIS, C_OCC_DONE_OCC
    // emitter rays made (k_material's sampling instantiation, one word per queue shard; they are pushed
    // onto the any-hit queue, so tot_any_q includes them, and are no part of tot_any)
    unsigned long long tot_emit[kShards];
};
static_assert(C_PH + kPhaseWords <= C_SKIP_INPLACE, "counter words overlap");

// Primary-hit candidate table: per film pixel one 64-B line of up to
// kPrimK triangle record indices in ascending scene-id order, and a byte prim_cnt[pixel]: 0 = no list
// (overflow, or no bound: the pixel's rays are traversed), n + 1 = a list of n candidates.
constexpr char kPrimaryHitsEnv[] = "MCPT_PRIMARY_HITS";  // "0" at context creation: the table is off
constexpr int kPrimLine = 16;           // u32 per pixel
constexpr int kPrimK = kPrimLine;       // candidates per pixel

struct ShadeArgs {
    DevScene scene;
    mcpt::CamView cam;
    DevPaths p;
    const int2* tiles;
    int ntiles, tile_w, tile_h, W, H;
    int spp, max_depth, rr_depth;
    int slots;  // path slots per pixel (paths in flight per pixel; slot k runs samples k, k + slots, ...)
    float slots_rcp;  // RN32(1 / slots) (k_shade's udiv_small)
    // Path index of a pixel: slot * npx + its index within the slot.  Full layout (compact 0): npx =
    // W * H and the index is the pixel id (the reference's path_id = pixel_id, wavefront_kernels.cu:
    // 108,114).  Compact layout (mcpt_set_compact_paths): the path state covers only the context's tile
    // set, npx = tile-set tiles * tile pixels and the index is set_tile * tile_w * tile_h + the pixel's
    // index in its tile, where set_tile = tile_base[t] for launch tile t (nullptr: t itself, the launch
    // runs the whole set in its order).
    uint32_t npx;
    int compact;
    const int* tile_base;
    uint64_t seed;
    uint32_t *ext_q, *any_q;
    // material queue (continuing paths, k_shade -> k_material, ext_cap per shard): dense records
    // {pid, pixel, sample index | len << kRecLenShift, hit_tri} + the updated throughput, so
    // k_material reads its per-path inputs from k_shade's coalesced loads instead of gathering them
    // again at pid (the pixel keys its RNG draws: the path index need not be the pixel id)
    uint4* mat_rec;
    float4* mat_beta;
    uint32_t ext_cap, any_cap;  // per-shard queue capacity
    CounterBlock* cnt;
    // k_shade block done flags, per (slot, film tile, block of the tile): set once every path of
    // the block is dead with its last sample finished, so later launches skip the block's loads
    // (cleared with the film; nullptr: off)
    uint8_t* blk_done;
    uint32_t shade_vblocks;  // k_shade: shading blocks of the launch (launch_shade sets it and the grid)
    // Per-pixel camera records of the W x H film (k_cam_table; gen_ray_pixel of every pixel): the
    // pixel's focal point (thin lens) or pinhole origin in cam_px, the pinhole direction in cam_dir
    const float4* cam_px;
    const float4* cam_dir;
    // Primary-hit candidate table (nullptr: off) and the primary queue {path, pixel} of generated
    // rays that k_primary resolves from it (ext_cap entries per shard, counter C_PRIM)
    const uint8_t* prim_cnt;
    const uint32_t* prim_list;
    uint2* prim_q;
    // 1 (mcpt_set_skip_discarded, the default): a continuing path whose next logic pass is certain to
    // end it makes no extension ray (Russian roulette: k_shade marks its record kRecNoCont in
    // reference mode, k_material decides in fixed mode) or ends at once without its material
    // evaluation (the next vertex lies beyond max_depth).  The rays are counted as the reference
    // traces them.  0: every stage as the reference runs it (mcpt_stage_run always)
    int skip;
    // Per-pixel sample budget of the W x H film (mcpt_set_sample_budget; nullptr: none).  Where it is
    // installed, launch_shade runs k_shade's map instantiation, which reads budget[pixel] in place of
    // spp; the no-map instantiation never looks at this field.
    const uint32_t* budget;
    // Emitted radiance per material id (mcpt_set_material_emission), xyz of a
    // float4 each; nullptr: no table, or one without a non-zero entry.  Where it is set, launch_shade
    // runs k_shade's emission instantiation; the others never look at this field.
    const float4* emis;
    // Emitter sampling (mcpt_set_emitter_sampling), set only while it is active
    // (switched on and a non-empty emitter table): launch_shade then runs the sampling instantiations
    // of k_shade and k_material; the others never look at these fields.  emit_cdf / emit_ent: the
    // emitter table on the device, emit_n entries in scene-id order, an entry {record index, pick
    // probability bits}.  nee2: the emitter sample's term per path; its visibility byte is
    // p.vis[emit_vis0 + path] (emit_vis0 = 2P: k_trace's finish writes at the index in o.w as ever).
    // Made emitter rays are counted per queue shard in cnt->tot_emit.
    const float* emit_cdf;
    const uint2* emit_ent;
    int emit_n;
    uint32_t emit_vis0;
    float4* nee2;
    // MIS between the emitter sample and collected emission (mcpt_set_emitter_mis),
    // set only while it is in effect (emitter sampling active and the switch on): launch_shade then
    // runs the MIS instantiations; the others never look at this field.  pick_rec[r]: the emitter
    // table's pick probability of triangle record r, 0 for a record that is no entry.
    const float* pick_rec;
    // Base-colour textures (mcpt_set_material_textures), set only while a set with
    // a textured material is installed (tex.uv != nullptr): launch_shade then runs k_material's textured
    // instantiations; the others never look at this field, and k_shade has none.
    mcpt::TexView tex;
};
// k_primary_build: the table of a W x H film.  stats: [0] pixels with a list, [1] overflow pixels.
struct PrimaryBuildArgs {
    DevScene scene;
    mcpt::CamView cam;
    int W, H;
    const float4 *cam_px, *cam_dir;
    uint8_t* cnt;
    uint32_t* list;
    uint32_t* stats;
};

// One ray set of a trace launch: rays ro/rd[rid] for queue entries
// queue[s * shard_cap + k], k < count of shard s.
struct TraceSet {
    const float4 *ro, *rd;
    const uint32_t* queue;      // nullptr => identity
    const uint32_t* count_ptr;  // device count of shard s at count_ptr[s * C_WORDS] (nullptr => count)
    uint32_t count;
    uint32_t shard_cap;         // queue entries per shard
    uint32_t* stats;            // optional: shard s counters at stats[s * C_WORDS + 0..2] (nodes, tests, hits)
    uint32_t* ray_steps;        // optional per-queue-entry node fetches + triangle tests (diagnostics)
    int prefiltered;            // 1: every ray has a valid direction and enters the root box (k_shade checked)
    int ray_at_slot;            // 1: the ray of queue position k is ro/rd[k] (dense); queue[k] is only the
                                //    result index.  0: the ray is ro/rd[queue[k]]
};
struct TraceArgs {
    DevScene scene;
    TraceSet set[2];            // [0] closest hit -> hit_tri, [1] any hit -> vis
    int nshards;
    int32_t* hit_tri;           // closest-hit output: triangle index or -1
    uint8_t* vis;               // any-hit output: 1 = unoccluded
    uint32_t refill_min;        // refill when at least this many lanes are idle (set by launch_trace)
    uint32_t tri_min;           // run the triangle phase when this many lanes hold a leaf (set by launch_trace)
    uint32_t nparts;            // work partitions (default: the device's XCDs; set by launch_trace)
    uint32_t ndies;             // XCDs of the device (set by launch_trace)
    uint32_t* grab;             // nparts chunk counters, C_WORDS apart, zero at launch (k_accumulate resets)
    const uint32_t* idle;       // optional: nonzero = the tile set is complete, exit at once (CounterBlock::idle)
    int tiny_stack;             // host side: launch the kLdsStackTiny instantiation (mcpt_debug_tiny_lds_stack)
    uint32_t* phase;            // counting build: loop-phase counts of shard s at phase[s * C_WORDS + PH_*] (or nullptr)
};

struct HitRecordArgs { DevScene scene; const float4 *ro, *rd; const int32_t* tri; float4 *hit_p, *hit_n; int32_t* scene_tri; uint32_t n; };
struct ClearArgs { uint32_t* flags; uint32_t* samples; float4* Ld; uint32_t n, npx; };  // n = npx * slots
// n accumulators per slot.  tiles == nullptr: n = W * H pixels in pixel order (full layout); else the
// compact layout's order (tile-set tile i's pixels at i * tile_w * tile_h, row by row), scattered to
// out[y * W + x] for the pixels inside the W x H film
struct ResolveArgs {
    const float4* Ld; const uint32_t* samples; float4* out_Ld; uint32_t* out_samples; uint32_t n; int slots;
    const int2* tiles; int tile_w, tile_h, W, H;
};
struct TonemapArgs { const float4* Ld; const uint32_t* samples; uchar4* out; float exposure; uint32_t n; };
struct PackArgs { const float4* Ld; const uint32_t* samples; const int2* tiles; int ntiles, tile_w, tile_h, W, H; float4* out; };
struct UnpackArgs { const float4* in; const int2* tiles; int ntiles, tile_w, tile_h, W, H; float4* Ld; uint32_t* samples; };

// Launch geometry of one device (mcpt_create): persistent grids from the occupancy
// calculator and the device's XCD count, with environment overrides for sweeps.
struct LaunchGeom {
    uint32_t trace_waves[2][2];  // k_trace grid (waves) per [node width 2/4][LDS stack normal/deep];
                                 // at most 28 waves per CU (MCPT_TRACE_WAVES overrides)
    uint32_t trace_parts;    // k_trace work partitions, MCPT_TRACE_PARTS (1..kMaxParts)
    uint32_t ndies;          // XCDs
    uint32_t mat_blocks[2];  // k_material grid [reference mode, fixed mode]
    uint32_t mat_blocks_samp[2];  // ... of its emitter-sampling instantiations
    uint32_t prim_blocks;    // k_primary grid (resident blocks, a multiple of the shard count)
    uint32_t shade_grid;     // k_shade grid cap (resident blocks x MCPT_SHADE_GRID; 0: one block per shading block)
    uint32_t refill_min, tri_min;  // MCPT_REFILL_MIN, MCPT_TRI_MIN
};

// ---- wavefront iteration (kernels.hip) ----
int launch_geometry(int device, LaunchGeom& g);  // device must be current
// tex_level: 2 the installed texture set has a metallic-roughness textured material:
// with a.tex set, k_material<TexMr, ...> in place of k_material's textured instantiation; 3 it has a
// normal-mapped one (section 21): k_material<TexNrm, ...>; 4 a material's base-colour texture is flagged
// MCPT_TEX_SRGB (section 22): k_material<TexSrgb, ...>.  Below 2 a.tex alone decides.
void launch_shade(const ShadeArgs& a, int nblocks, const LaunchGeom& g, bool fixed_mode, int tex_level, hipStream_t s);
void launch_shade_stage(bool material_stage, const ShadeArgs& a, int nblocks, const LaunchGeom& g, bool fixed_mode,
                        int tex_level, hipStream_t s);
void launch_primary(const ShadeArgs& a, const LaunchGeom& g, hipStream_t s);  // k_primary: after k_shade, before k_trace
void launch_trace(const TraceArgs& a, const LaunchGeom& g, hipStream_t s);
void launch_accumulate(CounterBlock* c, uint32_t nparts, uint32_t* occ_gate, hipStream_t s);
int shade_sections(unsigned long long* out, int n, int reset);  // -DMCPT_DIAG_SHADE builds (else 0)

// ---- emitter sampling (emitter.hip) ----
// k_emitter_weights: per triangle record r of the scene, weight[r] = area * luminance(Le[material]) with
// the sampling arithmetic's own area (0.5 sqrt(dot(c, c)), c = cross(e1, e2) of the record as stored),
// 0 for a non-emissive material, and id[r] = the record's scene triangle id.
void launch_emitter_weights(const DevScene& sc, const float4* emis, float* weight, uint32_t* id, hipStream_t s);
// k_emitter_pick_rec: pick_rec[r] = the pick probability of the emitter table's
// entry whose record is r, 0 for every other of the ntri records.  ent: the table's n device entries
// {record index, pick bits}.
void launch_emitter_pick_rec(const uint2* ent, uint32_t n, float* pick_rec, uint32_t ntri, hipStream_t s);

// ---- scene tables (scene_tables.hip) ----
// Occluder records (DevScene::occ_rec): for each triangle record t, {leaf mn, margin} {leaf mx,
// v0.x} {v0.yz, e1.xy} {e1.z, e2} of the leaf that holds it (nodes: nnodes nodes of the given
// width; a root that is itself a leaf gets the root box)
constexpr int kOccRecF4 = 4;
void launch_occ_records(const DevScene& sc, uint32_t nnodes, float4* rec, hipStream_t s);
void launch_occ_probes(const DevScene& sc, float4* ro, float4* rd, uint32_t nkeys, hipStream_t s);
// Complete keys: every key of sc.occ whose candidate list (occ_key_list over the child-pair tree
// `tree`) has at most kOccWays triangles gets the list, marked (kOccDoneBit); *ndone += their number
void launch_occ_complete(const DevScene& sc, const mcpt::OccTree& tree, uint32_t nkeys, uint32_t* ndone, hipStream_t s);
// Culling margins of a child-pair tree (mcpt_core.hpp cull_*): tri_w[t] = W'_T of record t,
// *pmax = the far coefficient P's bits (max), then `passes` bottom-up passes writing every
// child's subtree maximum into q3.z / q3.w (passes >= tree depth + 1 reach the fixed point).
// plane: the axis-plane bound (cull_plane_b) where it applies (false: the general bound only).
void launch_cull_margins(float4* nodes, uint32_t npairs, const float4* tri, uint32_t ntri, float* tri_w,
                         uint32_t* pmax, int passes, bool plane, hipStream_t s);
// Its first step alone: tri_w and *pmax (max) from the records (the refit fuses the passes with its boxes)
void launch_cull_tri(const float4* tri, uint32_t ntri, float* tri_w, uint32_t* pmax, bool plane, hipStream_t s);
void launch_primary_build(const PrimaryBuildArgs& a, hipStream_t s);
void launch_cam_table(const mcpt::CamView& cam, int W, int H, float4* px, float4* dir, hipStream_t s);
// tex[i].w = pdf[i], i < n (EnvView::tex: the pdf in the texture's alpha plane)
void launch_env_pack(float4* tex, const float* pdf, size_t n, hipStream_t s);
void launch_env_table(const mcpt::EnvView& e, bool fixed_mode, float4* out, float2* row, float2* col, hipStream_t s);

// ---- film (film.hip) ----
void launch_clear(const ClearArgs& a, hipStream_t s);
void launch_resolve(const ResolveArgs& a, hipStream_t s);
void launch_tonemap(const TonemapArgs& a, hipStream_t s);
void launch_pack(const PackArgs& a, hipStream_t s);
void launch_unpack(const UnpackArgs& a, hipStream_t s);
void launch_hit_record(const HitRecordArgs& a, hipStream_t s);
void launch_quot(const float* a, const float* b, float* out, uint32_t n, hipStream_t s);
void launch_copy(const float4* src, float4* dst, size_t n, hipStream_t s);

// ---- geometry update (refit.hip) ----
// k_geom_records: record i of tri (and of sh where n0 is given) from vertices order[i] (nullptr: i) of
// the v / n arrays (device, 3 floats per triangle); the id and material words stay.  box (or nullptr):
// 2 x float4 per record, its vertices' exact min / max.
struct GeomRecordsArgs {
    uint32_t ntri;
    const uint32_t* order;
    const float *v0, *v1, *v2, *n0, *n1, *n2;
    float4 *tri, *sh, *box;
};
void launch_geom_records(const GeomRecordsArgs& a, hipStream_t s);
// Boxes and margins of the child-pair tree `nodes` for new records, topology kept: leaf children from
// box / tri_w (k_geom_records, launch_cull_tri), interior children in `passes` bottom-up passes
// (passes >= tree depth + 1 reach the fixed point; pad nodes stay).  out7 (device): the root box's
// min, max and margin.
void launch_refit(float4* nodes, uint32_t npairs, int root_ref, int passes, const float4* box, const float* tri_w,
                  uint32_t ntri, float* out7, hipStream_t s);
// The boxes and margins of nquads 4-wide nodes again from the pair tree: slot k of node i copies child
// (src[4 i + k] & 1) of pair node (src[4 i + k] >> 1); kQuadNoSrc: an empty slot.  Refs stay.
constexpr uint32_t kQuadNoSrc = 0xffffffffu;
void launch_quad_regather(float4* quads, uint32_t nquads, const uint32_t* src, const float4* pairs, uint32_t npairs,
                          hipStream_t s);

// HRDI tables on the device (env_build.hip), bit-identical to the host build: scratch holds
// env_build_scratch_floats(W, H) floats; W * H < 2^31.
size_t env_build_scratch_floats(int W, int H);
void launch_env_build(const float4* tex, int W, int H, float* scratch, float* marginal_y, float* conds_y,
                      float* pdf, hipStream_t s);
// CDF check (*bad |= 1 unless the guides are valid) + the env_cell search guides
void launch_env_guides(const float* marginal_y, const float* conds_y, int W, int H, uint16_t* gm, uint16_t* gc,
                       uint32_t* bad, hipStream_t s);

// GPU linear BVH (bvh_build.hip).  Inputs: host vertex arrays (3 floats per
// triangle each) and the device triangle / shading records in scene order.
// verts_on_device: v0 / v1 / v2 are device arrays (a geometry update's rebuild), used in place.
struct LbvhInput { int ntri; const float *v0, *v1, *v2; const float4 *d_tri, *d_sh; bool verts_on_device = false; };
struct LbvhOutput {
    float4 *nodes = nullptr, *tri = nullptr, *tri_sh = nullptr;  // hipMalloc'ed, owned by the caller
    uint32_t* order = nullptr;  // likewise: order[p] = the input triangle stored at record p (Morton order)
    int nnodes = 0, root_ref = 0, depth = 0, rounds = 0;
    float root_mn[3], root_mx[3];
};
// PLOC cluster record: subtree height (low 8 bits, saturated at 255) and the subtree's
// interior-node count (bits 8..31).  Unsigned with logical shifts: a count below 2^24 (every
// scene mcpt_scene_upload accepts) packs and unpacks exactly (tests/native/core_identities.cpp).
__host__ __device__ constexpr uint32_t ploc_pack(uint32_t height, uint32_t count) {
    return (height < 255u ? height : 255u) | (count << 8);
}
__host__ __device__ constexpr uint32_t ploc_height(uint32_t h) { return h & 0xffu; }
__host__ __device__ constexpr uint32_t ploc_count(uint32_t h) { return h >> 8; }
// the record of a merge of clusters a and b
__host__ __device__ constexpr uint32_t ploc_merge(uint32_t a, uint32_t b) {
    return ploc_pack((ploc_height(a) > ploc_height(b) ? ploc_height(a) : ploc_height(b)) + 1u,
                     ploc_count(a) + ploc_count(b) + 1u);
}
int build_lbvh(const LbvhInput& in, LbvhOutput& out, hipStream_t s);
int build_ploc(const LbvhInput& in, LbvhOutput& out, hipStream_t s);

// ---- preview denoiser (denoise.hip) ----
// Its two switches, for A/B runs and tests; neither changes a result.  (As with kPrimaryHitsEnv, bench.py
// has no entry for them and stamps a run that sets one as an unknown knob, i.e. not the product.)
constexpr char kDenoiseLdsEnv[] = "MCPT_DENOISE_LDS_MAX";     // 0 / 1 / 2: the widest stride that takes the LDS kernel
constexpr char kGuideChunkEnv[] = "MCPT_GUIDE_CHUNK_BYTES";   // the guide pass's temporary-buffer budget
// One a-trous pass over W x H planes: col -> out (the two colour planes ping-pong), gd / al read only
struct DenoiseArgs {
    mcpt::DenoisePass k;
    int W, H;
    const float4 *col, *gd, *al;
    float4* out;
};
// The filter's planes of n pixels.  Ld != nullptr: from the film (Ld, samples) and the guide sums
// g_alb (albedo rgb, sample count) / g_nz (normal xyz, depth); else from caller images of means (rgb,
// normal, albedo: 3 floats per pixel; depth 1; samples may be nullptr: every pixel has samples)
struct DenoisePrepArgs {
    const float4* Ld; const uint32_t* samples; const float4 *g_alb, *g_nz;
    const float *rgb, *normal, *albedo, *depth;
    float4 *col, *gd, *al; uint32_t n;
};
// One chunk of the guide pass: pixels p0 .. p0 + np of the W x H film, film samples s0 .. s0 + ns;
// ray (s - s0) * np + (p - p0).  k_guide_rays writes ro / rd, k_guide_accum adds the chunk's hit
// records (hit_p.w = t, hit_n = normal and material bits, as k_hit_record writes them) to the sums.
struct GuideArgs {
    mcpt::CamView cam;
    const float4 *cam_px, *cam_dir;
    int W, H;
    uint64_t seed;
    uint32_t p0, np, s0, ns;
    float4 *ro, *rd;
    const float4 *hit_p, *hit_n;
    const float* mats;
    float4 *g_alb, *g_nz;
};
// The variance-guided form: beside the colour planes a float2 plane {variance
// of the mean luminance or -1, luminance} in ping-pong (v.vl -> v.out_vl).  The plain kernels take
// the DenoiseArgs part alone.
struct DenoiseGuidedArgs : DenoiseArgs {
    mcpt::DenoiseVar v;
};
// Its planes: DenoisePrepArgs' plus vl, from the film's error plane err {se, mean, K, n} (with Ld:
// variance = se se, unknown where se < 0 or not finite, and everywhere where err is nullptr) or from a
// caller image of variances (nullptr: none is known)
struct DenoiseGuidedPrepArgs : DenoisePrepArgs {
    const float4* err;
    const float* variance;
    float2* vl;
};
// Both launch the guided kernels where the vl plane is set and the plain ones where it is nullptr
void launch_denoise_pass(const DenoiseGuidedArgs& a, int lds_max_stride, hipStream_t s);
void launch_denoise_prep(const DenoiseGuidedPrepArgs& a, hipStream_t s);
void launch_guide_rays(const GuideArgs& a, hipStream_t s);
void launch_guide_accum(const GuideArgs& a, hipStream_t s);

// ---- base-colour textures (texture.hip) ----
// k_guide_accum_tex: k_guide_accum while textures are installed.  It rebuilds the chunk's hit records
// itself (rays a.ro / a.rd, triangle record rec[i] or -1: k_hit_record's arithmetic) and adds
// tex_base at the hit's texture coordinate as the albedo; normal, depth and count as k_guide_accum.
struct GuideTexArgs {
    GuideArgs g;
    DevScene scene;
    mcpt::TexView tex;
    const int32_t* rec;
};
void launch_guide_accum_tex(const GuideTexArgs& a, hipStream_t s);
// k_guide_accum_nrm (section 21): k_guide_accum_tex whose hit record is hit_record_n, so the normal guide
// accumulates the mapped normal; the albedo guide is unchanged.  Launched only under a normal-mapped set.
void launch_guide_accum_nrm(const GuideTexArgs& a, hipStream_t s);
// k_guide_accum_srgb (section 22): k_guide_accum_nrm whose albedo is tex_base_srgb, the decoded colour.
// Launched only under a set with a material whose base-colour texture is flagged MCPT_TEX_SRGB.
void launch_guide_accum_srgb(const GuideTexArgs& a, hipStream_t s);
// k_tex_sample: out[i] = tex_bilinear_rgba8(tex, w, h, uv[i]) for n uv pairs (mcpt_texture_sample_run)
void launch_tex_sample(const uint32_t* tex, int w, int h, const float2* uv, float* out_rgb, uint32_t n, hipStream_t s);
// k_tex_sample_srgb (section 22): the same over tex_bilinear_rgba8_srgb(..., true) (mcpt_texture_sample_run_ex
// with MCPT_TEX_SRGB)
void launch_tex_sample_srgb(const uint32_t* tex, int w, int h, const float2* uv, float* out_rgb, uint32_t n, hipStream_t s);
// k_tex_uv_records: the uv stream in record order: out[3 p + k] = uv_k[order[p]] (order == nullptr: p),
// uv0 / uv1 / uv2 in desc order
void launch_tex_uv_records(const float2* uv0, const float2* uv1, const float2* uv2, const uint32_t* order, float2* out,
                           uint32_t ntri, hipStream_t s);
// k_tex_tangent_records (section 21): the tangent stream in record order: out[3 p + k] = tan_k[order[p]],
// tan0 / tan1 / tan2 {T.xyz, s} in desc order
void launch_tex_tangent_records(const float4* tan0, const float4* tan1, const float4* tan2, const uint32_t* order, float4* out,
                                uint32_t ntri, hipStream_t s);

// ---- adaptive sampling (adaptive.hip) ----
// Which accumulator holds a film pixel.  own == nullptr: every pixel is the caller's and pixel o's
// accumulator is o (mcpt_error_run).  Else own[film tile] < 0: not the context's (outside its tile
// set, or scattered in from another context); >= 0: the tile's place in the compact layout's order
// (accumulator = place * tile pixels + the pixel's index in its tile), ignored in the full layout
// (accumulator = pixel id).
struct OwnMap {
    const int32_t* own;
    int compact, tile_w, tile_h, W, H;
};
// k_film_error: out[o] = film_error_pixel of film pixel o over `slots` accumulators `stride` apart
struct FilmErrorArgs {
    const float4* Ld; const uint32_t* samples; size_t stride; int slots;
    OwnMap m;
    float4* out;
};
// k_budget: budget[o] = budget_pixel(err[o]); cnt[0] += the budgets, cnt[1] = max, cnt[2] += pixels of
// the context whose budget equals their sample count
struct BudgetArgs {
    const float4* err;
    OwnMap m;
    mcpt::BudgetParams p;
    uint32_t* budget;
    unsigned long long* cnt;
};
// k_slot_image: one slot's accumulators as W x H images (zero where the pixel is not the context's)
struct SlotImageArgs {
    const float4* Ld; const uint32_t* samples;  // the slot's first accumulator
    OwnMap m;
    float4* out_Ld; uint32_t* out_samples;
};
void launch_film_error(const FilmErrorArgs& a, hipStream_t s);
void launch_budget(const BudgetArgs& a, hipStream_t s);
void launch_slot_image(const SlotImageArgs& a, hipStream_t s);

// ---- temporal accumulation (temporal.hip) ----
// k_temporal over a W x H frame: the previous call's history planes hcol / hpos / hnrm and VP_prev in,
// the colour and vl planes for the spatial passes and the new history planes out.  The current frame
// comes from the film (Ld != nullptr: Ld / samples, err {se, ...} or nullptr without an estimate, the
// guide sums and the camera records) or from caller images of means (rgb / position / normal 3 floats
// per pixel, variance / depth 1, samples).  vfill (film form only; nullptr: none): a vl plane of the
// current film frame whose variance a pixel takes where err gives it none.
struct TemporalArgs {
    int W, H;
    mcpt::TemporalParams k;
    float vp_prev[16];
    const uint32_t* samples;
    const float4 *Ld, *err, *g_alb, *g_nz, *cam_px, *cam_dir;
    mcpt::CamView cam;
    const float *rgb, *variance, *position, *normal, *depth;
    const float4 *hcol, *hpos, *hnrm;
    float4* col;
    float2* vl;
    float4 *out_hcol, *out_hpos, *out_hnrm;
    const float2* vfill;
};
// The spatial passes' planes of n pixels from an accumulated frame: its colour and vl planes copied, the
// guide and albedo planes from the guide sums as k_denoise_prep_film forms them
struct TemporalPrepArgs {
    const float4* tcol; const float2* tvl; const float4 *g_alb, *g_nz;
    float4 *col, *gd, *al; float2* vl; uint32_t n;
};
void launch_temporal(const TemporalArgs& a, hipStream_t s);
void launch_temporal_prep(const TemporalPrepArgs& a, hipStream_t s);

// ---- spatial variance estimate (variance.hip) ----
// k_variance_spatial over the filter's planes of a W x H image, in place on vl: a valid pixel whose
// variance is unknown gets the estimate (or stays unknown); col, gd, al and the luminances are read only
struct VarianceArgs {
    mcpt::VariancePass k;  // k.radius: 1 .. 3
    int W, H;
    const float4 *col, *gd, *al;
    float2* vl;
};
void launch_variance_spatial(const VarianceArgs& a, hipStream_t s);

}  // namespace mcpt_dev
