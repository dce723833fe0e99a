// runtime_internal.hpp -- what runtime.cpp (context, camera, lighting tables, render loop), film_state.cpp
// (tile set, ray queues, film and path state, film readers), scene_upload.cpp (scene upload and geometry
// update), postprocess.cpp (guides, denoise, adaptive sampling, temporal accumulation) and stage_run.cpp
// (per-stage parity harness, debug entries) share: the device context behind the mcpt_* C ABI, the
// owners of its state, its error helpers and a few host helpers.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "host/emitter_table.hpp"
#include "host/film_layout.hpp"
#include "kernels.hpp"
#include "mcpt.h"

using namespace mcpt_dev;

namespace mcpt_host {
void set_global_error(const std::string& e);
const char* global_error();
}  // namespace mcpt_host

// Owner of one hipMalloc'd array of T: move-only, freed exactly once (reset(), or the destructor).
template <class T>
class DevBuf {
    T* p_ = nullptr;
    size_t n_ = 0;  // elements

public:
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr, o.n_ = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            reset();
            std::swap(p_, o.p_);
            std::swap(n_, o.n_);
        }
        return *this;
    }
    ~DevBuf() { reset(); }
    void reset() {
        if (p_) (void)hipFree(p_);
        p_ = nullptr;
        n_ = 0;
    }
    // A buffer of at least count elements: one that is large enough is kept (contents too), else it is
    // replaced.  false: the allocation failed and the buffer is empty (hipGetLastError has the cause).
    bool ensure(size_t count) {
        if (p_ && n_ >= count) return true;
        reset();
        if (hipMalloc((void**)&p_, std::max<size_t>(count * sizeof(T), 16)) != hipSuccess) {
            p_ = nullptr;
            return false;
        }
        n_ = count;
        return true;
    }
    size_t size() const { return n_; }
    size_t bytes() const { return p_ ? std::max<size_t>(n_ * sizeof(T), 16) : 0; }  // as allocated
    T* get() const { return p_; }
    operator T*() const { return p_; }
    T* operator->() const { return p_; }
};

// Owner of one hipHostMalloc'd (pinned) array of T, as DevBuf is of device memory
template <class T>
class PinnedBuf {
    T* p_ = nullptr;

public:
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf&) = delete;
    PinnedBuf& operator=(const PinnedBuf&) = delete;
    PinnedBuf(PinnedBuf&& o) noexcept : p_(o.p_) { o.p_ = nullptr; }
    PinnedBuf& operator=(PinnedBuf&& o) noexcept {
        if (this != &o) {
            reset();
            std::swap(p_, o.p_);
        }
        return *this;
    }
    ~PinnedBuf() { reset(); }
    void reset() {
        if (p_) (void)hipHostFree(p_);
        p_ = nullptr;
    }
    bool alloc(size_t count) {  // false: the allocation failed and the buffer is empty
        reset();
        if (hipHostMalloc((void**)&p_, count * sizeof(T)) != hipSuccess) p_ = nullptr;
        return p_ != nullptr;
    }
    T* get() const { return p_; }
    operator T*() const { return p_; }
    T* operator->() const { return p_; }
};

// What a view-dependent product was built for.  Each product stores the key of its build and names
// the fields it depends on when it compares that key with the context's current one.
struct ViewKey {
    enum : unsigned { SCENE = 1, SEED = 2, SIZE = 4, CAM = 8 };
    uint64_t scene_gen = 0, seed = 0;
    uint32_t W = 0, H = 0;
    mcpt::CamView cam{};
    bool same(const ViewKey& o, unsigned fields) const {
        return (!(fields & SCENE) || scene_gen == o.scene_gen) && (!(fields & SEED) || seed == o.seed) &&
               (!(fields & SIZE) || (W == o.W && H == o.H)) && (!(fields & CAM) || memcmp(&cam, &o.cam, sizeof(cam)) == 0);
    }
};

// Per-pixel camera records (cam_table): valid for the film size and camera of `key`
struct CamTable {
    DevBuf<float4> tab;  // pixel records, then directions
    ViewKey key;
    bool ok = false;
};

// Primary-hit candidate table (prim_table): built for (scene upload, camera, film size); a film
// clear keeps it.  Best-effort: any failure leaves it off and the primary rays are traversed.
// (MCPT_PRIMARY_HITS=0: off, for A/B runs and tests.  bench.py has no entry for the switch and
// stamps a run that sets it as an unknown knob, i.e. not the product.)
struct PrimTable {
    bool on = [] { const char* e = getenv(kPrimaryHitsEnv); return !(e && e[0] == '0' && e[1] == 0); }();
    DevBuf<uint8_t> cnt;
    DevBuf<uint32_t> list, stats;  // stats: k_primary_build's two counters
    DevBuf<uint2> q;
    bool ok = false;      // the table is valid for `key`
    bool failed = false;  // the build for `key` failed: not retried until the key changes
    ViewKey key;
    uint64_t builds = 0;            // table builds so far
    uint32_t lists = 0, over = 0;   // the current table: pixels with a list / overflow pixels
    float build_ms = 0.f;           // the last build
    void release() {  // the buffers go; key, failed and the counts stay
        cnt.reset(), list.reset(), stats.reset(), q.reset();
        ok = false;
    }
};

// Preview denoiser.  Guide sums of the W x H film: alb (albedo rgb, sample
// count), nz (normal xyz, depth), allocated by the first mcpt_guides_render, valid for the (scene
// upload, seed, camera) of `key`.  Freed with the film.
struct Guides {
    DevBuf<float4> alb, nz;
    bool ok = false;
    ViewKey key;
};
// The filter's planes of the film (two colour planes in ping-pong, guides, albedo), allocated by the
// first mcpt_film_denoise[_guided] (denoise_planes_ensure); result: the colour plane that holds the
// last result (-1: none).  Variance-guided form: the {variance, luminance}
// planes in ping-pong beside col, allocated by the first guided call; guided: result is a guided
// result, whose variances are vl[result].  Freed with the film.
struct Denoise {
    DevBuf<float4> col[2], gd, al;
    DevBuf<float2> vl[2];
    int result = -1;
    bool guided = false;
};
// Adaptive sampling, all keyed by film pixel and allocated by the first call
// that needs them: budget, the per-pixel sample budget k_shade reads in place of cfg.spp while
// budget_on (budget_max: its largest entry, which sizes mcpt_render's batches); err4, the last
// mcpt_film_error result {se, mean, K, n} (err_ok); own_map, the film tiles' ownership (OwnMap) as
// of the last call that used it; bud_cnt, k_budget's three counters.  Film clears, slot, tile-set
// and layout changes keep them; mcpt_film_resize frees them.
struct Adaptive {
    DevBuf<uint32_t> budget;
    bool budget_on = false;
    uint32_t budget_max = 0;
    DevBuf<float4> err4;
    bool err_ok = false;
    DevBuf<int32_t> own_map;
    DevBuf<unsigned long long> bud_cnt;
    size_t bytes() const { return budget.bytes() + err4.bytes() + own_map.bytes() + bud_cnt.bytes(); }  // mcpt_debug_adaptive_bytes
};
// Temporal accumulation, allocated by the first mcpt_film_temporal: two sets
// of history planes {hcol, hpos, hnrm} in ping-pong (a call gathers from one and writes the other;
// set: the one that holds the last accumulated frame), that frame's colour and vl planes for the
// spatial passes, and its camera in `key` (ok: there is such a frame).  Film clears, seed, camera and
// slot changes keep them; a scene upload and mcpt_temporal_reset forget the frame, mcpt_film_resize
// frees everything.
struct Temporal {
    DevBuf<float4> h[2][3], col;
    DevBuf<float2> vl;
    int set = 0;
    bool ok = false;
    ViewKey key;
    size_t bytes() const {  // mcpt_debug_temporal_bytes
        size_t b = col.bytes() + vl.bytes();
        for (const auto& s : h)
            for (const auto& p : s) b += p.bytes();
        return b;
    }
};
// Device times of the last launches (mcpt_debug_*_ms).  Kept apart from the state above: the *_run
// entry points time launches over temporaries, and a time outlives the buffers it was measured on.
struct StageMs {
    float guides = 0.f, dn[9] = {};    // the last guide pass / filter set-up and passes
    float err = 0.f, budget = 0.f;     // the last k_film_error / k_budget
    float tp = 0.f;                    // the last k_temporal
    float var = 0.f;                   // the last k_variance_spatial
};
// Spatial variance estimate: the mcpt_set_variance_fill setting.  It holds no
// buffer and belongs to no film size, so nothing resets it.
struct VarianceFill {
    bool on = false;
    mcpt_variance_params p{};
};

// Emissive materials (mcpt_set_material_emission): the installed table, 3 floats
// per material of the uploaded scene on the host (empty: none installed) and a float4 per material on
// the device, and how many materials have a non-zero entry.  Only a table with one reaches the kernels
// (dev_table()): without, the context launches what it launched before.  Keyed by material id, so a
// geometry update keeps it; a scene upload drops it.
struct Emission {
    std::vector<float> rgb;
    DevBuf<float4> tab;
    int32_t lit = 0;
    const float4* dev_table() const { return lit > 0 ? tab.get() : nullptr; }
    void drop() {
        rgb.clear();
        lit = 0;
    }
};

// Base-colour textures (mcpt_set_material_textures): the installed set on the host
// (uvs in desc order, 2 floats per triangle and corner; the textures' sizes, first texels and the atlas;
// the per-material index) and on the device: the uv stream in record order, the atlas and the per-material
// {first texel, w, h, index}.  Only a set with a textured material reaches the kernels (view()): without,
// the context launches what it launched before.  The uv stream follows the record order, so a rebuild
// permutes it again (textures_reorder); a scene upload drops the set.
// Metallic-roughness textures (section 20): mat_mr indexes the same texture list (all -1 where the caller
// gave none); d_mat holds 2 nmat entries, the MR ones in front and mirrored (material m's at nmat - 1 - m),
// the base-colour ones behind, where view().mat points (device/texture.hpp TexView).  A set with an
// MR-textured material launches k_material<TexMr, ...>.
// Normal maps (section 21): tan[k] holds corner k's {T.xyz, s}, 4 floats per triangle in desc order (empty:
// the caller gave none), mat_nrm indexes the same texture list (all -1 where absent), nrm_scale one float
// per material (all 1 where absent); nrm_fields records whether the caller gave any of the three, which is
// what the read-back reports.  On the device the tangent stream lies behind the uv stream in d_uv, at
// mcpt::tex_tan_offset(ntri) float2, in record order (textures_reorder permutes both), and the materials'
// normal entries {first texel, w, h, scale bits} lie in front of the atlas in d_atlas, mirrored (material
// m's at word 4 (nmat - 1 - m)): view().atlas points behind them.  No kernel argument grows.  A set with a
// normal-mapped material launches k_material<TexNrm, ...> and k_guide_accum_nrm.
struct Textures {
    std::vector<float> uv[3], tan[3], nrm_scale;
    std::vector<int32_t> tw, th, mat_tex, mat_mr, mat_nrm;
    std::vector<uint32_t> first;  // texture k's first texel in the atlas
    std::vector<uint32_t> flags;  // per texture MCPT_TEX_* (section 22); empty: the caller gave none (all 0)
    std::vector<uint32_t> atlas;
    DevBuf<float2> d_uv, d_stage;  // [3 ntri] record order (+ the tangent stream); [3 ntri] desc order, the permutation's input
    DevBuf<float4> d_tstage;       // [3 ntri] tangents in desc order, the permutation's input
    DevBuf<uint32_t> d_atlas;      // 4 nmat words of normal entries, then the texels
    DevBuf<int4> d_mat;
    int32_t textured = 0;      // materials with a base-colour texture
    int32_t textured_mr = 0;   // materials with a metallic-roughness texture
    int32_t textured_nrm = 0;  // materials with a normal map
    int32_t textured_srgb = 0;  // materials whose base-colour texture is flagged MCPT_TEX_SRGB (section 22)
    bool nrm_fields = false;   // the caller gave tangents, mat_nrm or nrm_scale
    bool dev_ok = false;       // the device arrays stand for the current record order
    bool installed() const { return !mat_tex.empty(); }
    // some material shades through a lookup
    bool shaded() const { return textured > 0 || textured_mr > 0 || textured_nrm > 0; }
    // k_material's texture level while the set is in effect (launch_shade)
    int level() const { return textured_srgb > 0 ? 4 : textured_nrm > 0 ? 3 : textured_mr > 0 ? 2 : 1; }
    mcpt::TexView view() const {
        if (!(shaded() && dev_ok)) return mcpt::TexView{nullptr, nullptr, nullptr};
        return mcpt::TexView{d_uv.get(), d_atlas.get() + 4 * mat_tex.size(), d_mat.get() + mat_tex.size()};
    }
    size_t bytes() const {
        return installed() ? d_uv.bytes() + d_stage.bytes() + d_tstage.bytes() + d_atlas.bytes() + d_mat.bytes() : 0;
    }
    void drop() {
        for (auto& u : uv) u.clear();
        for (auto& t : tan) t.clear();
        tw.clear(), th.clear(), mat_tex.clear(), mat_mr.clear(), mat_nrm.clear(), nrm_scale.clear(), first.clear(), flags.clear(), atlas.clear();
        d_uv.reset(), d_stage.reset(), d_tstage.reset(), d_atlas.reset(), d_mat.reset();
        textured = textured_mr = textured_nrm = textured_srgb = 0;
        nrm_fields = false;
        dev_ok = false;
    }
};

// Emitter sampling (mcpt_set_emitter_sampling): the switch, the emitter table
// of the uploaded scene under the installed emission (host copy and device arrays) and the two per-path
// streams the sampling instantiations use.  Active = switched on and a non-empty table; only then do the
// streams exist and the kernels differ.  The table is rebuilt (emitter_table_refresh) while the switch is
// on whenever the emission table or the geometry changes; a scene upload drops it.
struct EmitterSampling {
    bool on = false;
    mcpt_host::EmitterTable tab;
    DevBuf<float> cdf;
    DevBuf<uint2> ent;     // {record index, pick bits} per entry
    DevBuf<float4> nee2;   // [P]
    DevBuf<uint8_t> vis;   // [3P]: the any-hit results with the emitter rays' third part
    size_t paths = 0;      // P the streams were last sized (and zeroed) for
    float build_ms = 0.f;  // the last table build: weights kernel, readback, host table, upload
    // MIS between emitter samples and collected emission (mcpt_set_emitter_mis):
    // the switch, and the table's pick keyed by triangle record, which follows the table's life and
    // exists only while MIS is in effect (pick_ok: built for the current table and record order).
    bool mis = false;
    DevBuf<float> pick_rec;  // [ntri]
    bool pick_ok = false;
    bool active() const { return on && !tab.cdf.empty(); }
    bool mis_active() const { return mis && active(); }
    void drop_pick() {
        pick_rec.reset();
        pick_ok = false;
    }
    void drop_table() {
        tab = mcpt_host::EmitterTable{};
        drop_pick();
    }
    void drop_streams() {
        nee2.reset();
        vis.reset();
        paths = 0;
    }
};

// The upload-time environment knobs as the last upload read them (read_upload_env, scene_upload.cpp;
// a geometry update takes them from here and never calls getenv)
struct UploadKnobs {
    bool cull_off = false;     // MCPT_CULL=0
    bool plane = true;         // MCPT_CULL_PLANE
    int width = 0;             // MCPT_BVH_WIDTH (0: by tree size)
    int layout = -1;           // MCPT_SIBLING_LAYOUT (-1: by tree size)
    int occ_g = 24, occ_b = 12;                     // MCPT_OCC_G / MCPT_OCC_B
    bool occ_complete = true, occ_prefill = true;   // MCPT_OCC_COMPLETE / MCPT_OCC_PREFILL
    bool env_guides = true;    // MCPT_ENV_GUIDES
};

inline void free_list(std::vector<void*>& v) {
    for (void* q : v)
        if (q) (void)hipFree(q);
    v.clear();
}

// The uploaded scene (scene_upload.cpp): every device array of it, what the kernels see of it, and what
// the last upload or geometry update (mcpt_scene_update_geometry) found out about
// it.  bufs owns every array below and in dev, so the pointers live exactly as long as their arrays:
// reset() frees all of them and value-initialises every field.
struct SceneState {
    std::vector<void*> bufs;
    DevScene dev{};
    bool ok = false;       // dev is complete: false during an upload or update and after a failed one
    int32_t ntri = 0;      // triangles of the uploaded scene
    int32_t nmat = 0;      // ... and its materials
    UploadKnobs knobs;
    bool gpu_upload = false;  // uploaded by mcpt_scene_upload_gpu_bvh
    // the child-pair tree (mcpt_debug_bvh_read): the array launch_cull_margins wrote, which a 4-wide
    // upload collapses from
    const float4* pair_nodes = nullptr;
    uint32_t pair_count = 0;
    int pair_root = 0, pair_depth = 0, ploc_rounds = 0;
    int node_layout = 0;   // pair-node numbering the upload used (mcpt_debug_node_layout)
    bool pair_gpu_built = false;
    bool cull_ok = true, nest_ok = true;  // boxes contain their triangles / nest (PairTree)
    float4* bvh_nodes = nullptr;          // the device builder's node array (also when it holds no node)
    uint32_t* order = nullptr;            // record p holds desc triangle order[p] (nullptr: identity)
    float4 *desc_tri = nullptr, *desc_sh = nullptr;  // records in desc order (device-built scenes: the builders' input)
    float4* quads = nullptr;              // the 4-wide nodes (DevScene::nodes of a width-4 scene)
    uint32_t* quad_src = nullptr;         // per 4-wide slot the (pair node, child) it copies (kQuadNoSrc: empty)
    uint32_t nquads = 0;
    // occluder cache
    size_t occ_entries_n = 0;       // table entries (DevScene::occ; + kOccGateWords gate words)
    uint32_t* occ_init = nullptr;   // the table as the pre-fill and complete keys left it (film clears restore it); nullptr: empty
    uint64_t occ_done_keys = 0;     // complete keys (device/occ_beam.hpp) and their build's ms
    float occ_done_ms = 0.f;
    float4* occ_rec = nullptr;      // DevScene::occ_rec
    float4* occ_dir = nullptr;      // the complete keys' direction-bin table
    // environment light
    bool env_device_built = false;  // the HRDI tables were built on the device (env_build.hip)
    bool env_guides = false;        // env_cell uses the search guides
    float build_ms = 0.f;           // the GPU BVH build (mcpt_scene_upload_gpu_bvh, MCPT_GEOM_REBUILD)
    float env_build_ms = 0.f;       // the device build of the HRDI tables
    // a geometry update's scratch, kept between updates
    DevBuf<float> stage;            // the host entry's vertex (and normal) arrays
    DevBuf<float4> box;             // per record its vertex box
    DevBuf<float> tri_w, out;       // per record W'_T; {root box, root margin, P bits}
    float update_ms[8] = {};        // mcpt_debug_geometry_update_ms

    void reset() {
        free_list(bufs);
        *this = SceneState{};
    }
    // hipFree one array of the scene, drop it from bufs and null the pointer
    template <class T>
    void release(T*& p) {
        auto it = std::find(bufs.begin(), bufs.end(), (const void*)p);
        if (it != bufs.end()) {
            (void)hipFree(*it);
            bufs.erase(it);
        }
        p = nullptr;
    }
};

// ---- what the wavefront iteration runs on (film_state.cpp) ----

// The ray queues of the tile set: extension and any-hit path indices and the material records per shard,
// and the any-hit rays at their queue positions (k_material stores them there, so the path streams'
// sray_o / sray_d point here).  Re-allocated only when the need grows or the any-hit multiplier changes.
struct RayQueues {
    DevBuf<uint32_t> ext, any, mat;     // mat: MatRec + beta per extension-queue entry (8 words)
    DevBuf<float4> any_ray;             // o [mult * alloc], then d
    uint32_t ext_cap = 0, any_cap = 0;  // per-shard capacities of the current tile set
    size_t need = 0;                    // ... and its extension-queue entries (kShards * ext_cap <= alloc)
    size_t alloc = 0;                   // entries ext is allocated for (any holds mult times as many)
    uint32_t mult = 0;                  // any-hit rays per material evaluation the queues are allocated for
    bool ready() const { return ext && any && mat && any_ray; }
    bool fits(const FilmLayout& L) const { return L.queue_need <= alloc && L.any_mult == mult; }
    void release() {
        ext.reset(), any.reset(), mat.reset(), any_ray.reset();
        alloc = 0;
    }
    // The capacities of L; queues that do not fit it are released and allocated anew (the caller has
    // synchronised the stream).  false: an allocation failed and all four are empty.
    bool ensure(const FilmLayout& L) {
        ext_cap = L.ext_cap;
        any_cap = L.any_cap;
        need = L.queue_need;
        if (fits(L)) return true;
        release();
        const size_t m = L.any_mult;
        if (!ext.ensure(need) || !any.ensure(m * need) || !mat.ensure(need * 8) || !any_ray.ensure(2 * m * need)) {
            release();
            return false;
        }
        alloc = need;
        mult = L.any_mult;
        return true;
    }
    // any-hit rays, indexed by any-queue position (kShards * any_cap = mult * need entries)
    float4* sray_o() const { return any_ray; }
    float4* sray_d() const { return any_ray ? any_ray + (size_t)mult * alloc : nullptr; }
};

// -1, or the index of tile t in v
inline int tile_index(const std::vector<int2>& v, int2 t) {
    for (size_t i = 0; i < v.size(); i++)
        if (v[i].x == t.x && v[i].y == t.y) return (int)i;
    return -1;
}

// The tile set the iterations run over (device and host copy; the device array only grows) and
// mcpt_wavefront_step's one-tile set: device + pinned staging, 16 B each (the tile, then its index in
// the tile set, ShadeArgs::tile_base).
struct TileSet {
    DevBuf<int2> dev;
    std::vector<int2> host;
    DevBuf<int2> step;
    PinnedBuf<int2> step_h;
    int index_of(int2 t) const { return tile_index(host, t); }
    // every tile of the film's grid, row by row
    static std::vector<int2> all(const FilmLayout& L) {
        std::vector<int2> t;
        for (uint32_t y = 0; y < L.ny; y++)
            for (uint32_t x = 0; x < L.nx; x++) t.push_back(make_int2((int)x, (int)y));
        return t;
    }
    // n (x, y) pairs as tiles of the grid -> out.  Returns n, or the index of the first pair outside
    // the grid: out then holds the tiles before it.
    static uint32_t parse(const uint32_t* xy, uint32_t n, const FilmLayout& L, std::vector<int2>& out) {
        out.clear();
        for (uint32_t i = 0; i < n; i++) {
            if (xy[2 * i] >= L.nx || xy[2 * i + 1] >= L.ny) return i;
            out.push_back(make_int2((int)xy[2 * i], (int)xy[2 * i + 1]));
        }
        return n;
    }
};

// The film: the path streams (slots x npx paths), the k_shade block done flags and, with more than one
// slot or in the compact layout, the W x H planes of the slot sums -- allocated together for one
// layout (alloc_film_state), exact sizes.  allocated: the film exists (the mcpt_film_* entries' test).
struct FilmState {
    FilmLayout L{};  // what the buffers were last allocated for (the tile set's capacities of now: RayQueues)
    bool allocated = false;
    DevBuf<float4> ray_o, ray_d, beta, nee0, nee1, Ld;
    DevBuf<int32_t> hit_tri;
    DevBuf<uint32_t> flags, samples;
    DevBuf<uint8_t> vis;          // [2 paths]
    DevBuf<uint8_t> blk_done;     // ShadeArgs::blk_done
    DevBuf<float4> sum_Ld;        // slots > 1 or compact: the film, W x H (sum of the slot accumulators)
    DevBuf<uint32_t> sum_samples;
    // tiles holding pixels scattered in from another context (mcpt_film_unpack_tiles, mcpt_gather)
    // since the last film clear: the full layout's slot 0 holds them, so they may not become own
    // tiles before a clear (their sample count restarts from the flags word while Ld accumulates)
    std::vector<int2> unpacked;

    size_t pixels() const { return allocated ? L.npix : 0; }  // W * H of an allocated film, else 0
    void release() {
        // (in the order alloc allocates them)
        ray_o.reset(), ray_d.reset(), hit_tri.reset(), beta.reset(), nee0.reset(), nee1.reset(), Ld.reset();
        flags.reset(), samples.reset(), vis.reset(), blk_done.reset(), sum_Ld.reset(), sum_samples.reset();
        allocated = false;
    }
    // Everything released, then allocated for layout l.  false: an allocation failed (hipGetLastError
    // has the cause) and everything is released.
    bool alloc(const FilmLayout& l) {
        release();
        L = l;
        const size_t P = l.paths;
        const bool ok = ray_o.ensure(P) && ray_d.ensure(P) && hit_tri.ensure(P) && beta.ensure(P) && nee0.ensure(P) &&
                        nee1.ensure(P) && Ld.ensure(P) && flags.ensure(P) && samples.ensure(P) && vis.ensure(2 * P) &&
                        blk_done.ensure(l.blk_done_n) && (!l.sum_planes || (sum_Ld.ensure(l.npix) && sum_samples.ensure(l.npix)));
        if (!ok) release();
        return ok;
    }
    // The path streams as the kernels take them; the any-hit rays live with the queues
    DevPaths paths(const RayQueues& q) const {
        DevPaths p{};
        p.ray_o = ray_o, p.ray_d = ray_d, p.sray_o = q.sray_o(), p.sray_d = q.sray_d();
        p.beta = beta, p.nee0 = nee0, p.nee1 = nee1, p.Ld = Ld;
        p.hit_tri = hit_tri;
        p.flags = flags, p.samples = samples;
        p.vis = vis;
        return p;
    }
};

struct mcpt_ctx;
// The counter block: on the device, its pinned staging copy, and the host copy of the totals after the
// last call (valid: totals_ok; refresh reads them back when they are not).
struct Counters {
    DevBuf<CounterBlock> dev;
    PinnedBuf<CounterBlock> host;
    CounterBlock totals{};
    bool totals_ok = false;
    unsigned long long phase_base[kPhaseWords] = {};  // mcpt_debug_trace_profile's reset point
    int refresh(mcpt_ctx* c);  // device -> host -> totals, one stream synchronisation
};

struct mcpt_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    mcpt_config cfg{};
    char devname[256] = {0};
    int num_cu = 0;
    LaunchGeom geom{};             // persistent grids and k_trace partitions of this device
    uint32_t trace_parts_default = 1;
    SceneState scene;
    Emission em;
    EmitterSampling es;
    Textures tx;
    bool has_scene_before = false;  // set at the start of a re-upload
    // traversal work counters (mcpt_set_work_counters): k_trace's counting instantiation, whose six
    // per-lane counters cost the fast one its spill-free registers -- off by default
    bool count_work = getenv("MCPT_WORK_COUNTERS") != nullptr;
    // mcpt_set_skip_discarded: paths the next logic pass is certain to end make no extension ray
    // (ShadeArgs::skip); results and ray counts are the same either way
    bool skip_discarded = true;
    // camera
    mcpt::CamView cam{};
    bool has_cam = false;
    CamTable cam_tab;
    PrimTable prim;
    uint64_t scene_gen = 0;  // scene uploads so far
    // Film observes camera and scene (Film::update -> clear(), Film.cu:278-281; notified by
    // Camera::update, Camera.cu:207, and Scene::notify, Scene.cu:534-545): a change marks the
    // film stale and the next iteration clears it first (unless MCPT_FLAG_NO_AUTO_CLEAR).
    bool film_stale = false;
    // film + paths: the settings here, the buffers in their owners
    uint32_t W = 0, H = 0, tile_w = 256, tile_h = 256;
    uint32_t slots = 1;  // path slots per pixel (mcpt_set_path_slots); path state holds slots * npx paths
    // Path layout (mcpt_set_compact_paths).  Full: npx = W * H, path index = slot * npx + pixel id.  Compact:
    // the path state covers the tile set only, npx = tile-set tiles x tile pixels (ShadeArgs::npx).
    bool compact = false;
    uint32_t any_mult = 2;  // any-hit rays per material evaluation wanted: 3 with emitter sampling active
    bool blk_done_off = getenv("MCPT_NO_BLOCK_DONE") != nullptr;  // A/B switch: every block runs
    TileSet tiles;
    RayQueues queues;
    FilmState film;
    Counters cnt;
    std::vector<hipEvent_t> events;
    // scratch of one call (TmpScope; the stage runs)
    std::vector<void*> tmp_bufs;
    float last_stage_ms = 0.f;
    int gpu_bvh_builder = MCPT_GPU_BVH_PLOC;  // mcpt_set_gpu_bvh_builder
    bool tiny_stack = false;  // mcpt_debug_tiny_lds_stack: k_trace with a 2-entry LDS stack (tests)
    // film post-processing (postprocess.cpp)
    Guides guides;
    Denoise dn;
    Adaptive ad;
    Temporal tp;
    VarianceFill vf;
    StageMs ms;

    ViewKey view() const { return ViewKey{scene_gen, cfg.seed, W, H, cam}; }
    // The layout of the settings above over a tile set of ntiles tiles
    FilmLayout layout(size_t ntiles) const { return film_layout(W, H, tile_w, tile_h, slots, compact, ntiles, any_mult); }
    // The owners' device memory goes while the device is current and the stream still exists (mcpt_destroy)
    void release_buffers() {
        scene.reset();
        free_list(tmp_bufs);
        tiles = TileSet{}, queues = RayQueues{}, film = FilmState{}, cnt = Counters{};
        cam_tab = CamTable{}, prim.release(), em = Emission{}, es = EmitterSampling{}, tx.drop();
        guides = Guides{}, dn = Denoise{}, ad = Adaptive{}, tp = Temporal{};
    }
};

inline int set_err(mcpt_ctx* c, int rc, const std::string& msg) {
    if (c) c->err = msg;
    mcpt_host::set_global_error(msg);
    return rc;
}
#define HIPCHK(c, x)                                                                          \
    do {                                                                                      \
        hipError_t e_ = (x);                                                                  \
        if (e_ != hipSuccess)                                                                 \
            return set_err((c), MCPT_E_HIP, std::string(#x) + ": " + hipGetErrorString(e_));  \
    } while (0)

template <class T>
int dalloc(mcpt_ctx* c, std::vector<void*>& list, T** out, size_t count) {
    void* q = nullptr;
    size_t bytes = std::max<size_t>(count * sizeof(T), 16);
    hipError_t e = hipMalloc(&q, bytes);
    if (e != hipSuccess) return set_err(c, MCPT_E_NOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
    list.push_back(q);
    *out = (T*)q;
    return MCPT_OK;
}
template <class T>
int dupload(mcpt_ctx* c, std::vector<void*>& list, T** out, const T* src, size_t count) {
    int rc = dalloc(c, list, out, count);
    if (rc) return rc;
    if (count) HIPCHK(c, hipMemcpy(*out, src, count * sizeof(T), hipMemcpyHostToDevice));
    return MCPT_OK;
}
// The temporaries of one call (dalloc / dupload into c->tmp_bufs): the list starts empty and is freed
// on every return.
struct TmpScope {
    std::vector<void*>& L;
    explicit TmpScope(mcpt_ctx* c) : L(c->tmp_bufs) { free_list(L); }
    ~TmpScope() { free_list(L); }
    TmpScope(const TmpScope&) = delete;
    TmpScope& operator=(const TmpScope&) = delete;
};

inline int Counters::refresh(mcpt_ctx* c) {
    totals_ok = false;
    HIPCHK(c, hipMemcpyAsync(host, dev, sizeof(CounterBlock), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    totals = *host;
    totals_ok = true;
    return MCPT_OK;
}

// Defined in runtime.cpp (C++ linkage: `extern "C++"` where they stand inside its extern "C" block)
hipEvent_t ev(mcpt_ctx* c, size_t i);
int check_ready(mcpt_ctx* c);
// The emitter table again from the current scene and emission (nothing while the switch is off or no
// scene stands).  A table that differs bitwise from the previous one marks the film stale and drops the
// temporal history.
int emitter_table_refresh(mcpt_ctx* c);
int cam_table(mcpt_ctx* c, uint32_t W, uint32_t H, const float4** px, const float4** dir);
// Defined in scene_upload.cpp: the installed texture set's uv stream again in the scene's current record
// order (nothing without a set); MCPT_GEOM_REBUILD calls it after the new tree is adopted.
int textures_reorder(mcpt_ctx* c);
// Defined in film_state.cpp
// The tile set t: queues sized for it (RayQueues::ensure), the tiles uploaded.  The film state stays.
int set_tiles_internal(mcpt_ctx* c, const std::vector<int2>& t);
int film_view(mcpt_ctx* c, const float4** Ld, const uint32_t** samples);
// n float4 of a device plane to the host: the xyz as 3 floats per element and / or the w (nullptr: not wanted)
int read_plane(mcpt_ctx* c, const float4* d, size_t n, float* xyz, float* w);
// k_tonemap over a W x H colour plane and its per-pixel sample counts (nullptr: 1 everywhere) -> out
int tonemap_rgba8(mcpt_ctx* c, const float4* col, const uint32_t* samples, float exposure, uint8_t* out);
