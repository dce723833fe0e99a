// runtime.cpp -- device context behind the mcpt_* C ABI (include/mcpt.h).
//
// Replaces the reference's orchestration: PathTracer (PathTracer.cpp:112-187),
// Film device state (Film.cu:121-276) and wavefront_pathtrace
// (wavefront_kernels.cu:377-442).
// Differences by design: one stream, no host sync or managed-memory counter
// readback between stages (counts stay on the device and the trace kernels are
// persistent), a whole tile set per iteration instead of one 256x256 tile, and
// error codes instead of exit(99).  The tile set, the ray queues, the film state and the film's
// readers are film_state.cpp; the film's post-processing entry points (guides, denoise, adaptive
// sampling, temporal accumulation) are postprocess.cpp; scene upload and geometry update are
// scene_upload.cpp; the per-stage parity harness (mcpt_stage_run) and the
// mcpt_debug_* entries beyond the counter reads below are stage_run.cpp.
#include <chrono>
#include <cstdio>

#include "runtime_internal.hpp"

extern "C" {

const char* mcpt_last_error(const mcpt_ctx* c) { return c ? c->err.c_str() : mcpt_host::global_error(); }

int mcpt_create(int device, const mcpt_config* cfg, mcpt_ctx** out) {
    if (!out) return set_err(nullptr, MCPT_E_INVALID, "out is null");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return set_err(nullptr, MCPT_E_NODEVICE, "no HIP device visible (the backend has no CPU fallback)");
    if (device < 0 || device >= n) return set_err(nullptr, MCPT_E_INVALID, "device index out of range");
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess)
        return set_err(nullptr, MCPT_E_HIP, "hipGetDeviceProperties failed");
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return set_err(nullptr, MCPT_E_NODEVICE, std::string("device is ") + prop.gcnArchName + ", code objects are gfx950 only");
    mcpt_ctx* c = new mcpt_ctx();
    c->device = device;
    c->num_cu = prop.multiProcessorCount;
    snprintf(c->devname, sizeof(c->devname), "%s (%s, %d CUs)", prop.name, prop.gcnArchName, prop.multiProcessorCount);
    if (cfg) c->cfg = *cfg;
    else { c->cfg.seed = 0x5EED2026ull; c->cfg.spp = 16; c->cfg.max_depth = 5; c->cfg.rr_depth = 3; c->cfg.tile_w = 256; c->cfg.tile_h = 256; }
    // a dead path's flags word holds its next sample index, up to spp - 1 + 256 path slots
    if (c->cfg.max_depth < 1 || c->cfg.max_depth > 200 || c->cfg.spp < 0 || (uint32_t)c->cfg.spp > kMaxSpp - 256) {
        delete c;
        return set_err(nullptr, MCPT_E_INVALID, "bad config (max_depth 1..200, spp 0..2^19-256)");
    }
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
        delete c;
        return set_err(nullptr, MCPT_E_HIP, "stream creation failed");
    }
    if (!c->cnt.dev.ensure(1) || !c->cnt.host.alloc(1)) {
        delete c;
        return set_err(nullptr, MCPT_E_NOMEM, "counter allocation failed");
    }
    (void)hipMemset(c->cnt.dev, 0, sizeof(CounterBlock));
    if (launch_geometry(device, c->geom) != 0) {
        mcpt_destroy(c);
        return set_err(nullptr, MCPT_E_HIP, "occupancy query failed");
    }
    c->trace_parts_default = c->geom.trace_parts;
    *out = c;
    return MCPT_OK;
}

void mcpt_destroy(mcpt_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    c->release_buffers();  // every owner's memory goes while the device is current and the stream exists
    for (auto e : c->events) (void)hipEventDestroy(e);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

int mcpt_device_name(mcpt_ctx* c, char* buf, int32_t len) {
    if (!c || !buf || len <= 0) return MCPT_E_INVALID;
    snprintf(buf, (size_t)len, "%s", c->devname);
    return MCPT_OK;
}

int mcpt_debug_ray_counts(const mcpt_ctx* c, uint64_t* out) {
    if (!c || !out) return MCPT_E_INVALID;
    const CounterBlock& t = c->cnt.totals;
    const bool ok = c->cnt.totals_ok;
    out[0] = ok ? t.tot_ext : 0;    // extension rays (queued + resolved in place)
    out[1] = ok ? t.tot_ext_q : 0;  // extension rays k_trace traversed
    out[2] = ok ? t.tot_any : 0;    // shadow + BRDF visibility rays
    out[3] = ok ? t.tot_any_q : 0;  // any-hit rays k_trace traversed
    // (emitter rays share the any-hit queue and are no rays of the reference: mcpt_debug_emitter_stats)
    for (int k = 0; ok && k < kShards; k++) out[3] -= t.tot_emit[k];
    out[4] = ok ? t.tot_occ : 0;    // any-hit rays the occluder cache resolved in k_material
    return MCPT_OK;
}
int mcpt_debug_primary_stats(const mcpt_ctx* c, double* out4) {
    if (!c || !out4) return MCPT_E_INVALID;
    out4[0] = c->prim.ok ? (double)c->prim.lists : 0.0;
    out4[1] = c->prim.ok ? (double)c->prim.over : 0.0;
    out4[2] = c->cnt.totals_ok ? (double)c->cnt.totals.tot_prim : 0.0;
    out4[3] = (double)c->prim.build_ms;
    return (int)std::min<uint64_t>(c->prim.builds, 0x7fffffffull);
}
int mcpt_debug_discard_stats(const mcpt_ctx* c, uint64_t* out4) {
    if (!c || !out4) return MCPT_E_INVALID;
    for (int k = 0; k < 4; k++) out4[k] = c->cnt.totals_ok ? c->cnt.totals.tot_skip[k] : 0;
    return MCPT_OK;
}
int mcpt_debug_occ_complete_stats(const mcpt_ctx* c, double* out4) {
    if (!c || !out4) return MCPT_E_INVALID;
    out4[0] = (double)c->scene.occ_done_keys;
    out4[1] = c->cnt.totals_ok ? (double)c->cnt.totals.tot_done[0] : 0.0;
    out4[2] = c->cnt.totals_ok ? (double)c->cnt.totals.tot_done[1] : 0.0;
    out4[3] = (double)c->scene.occ_done_ms;
    return MCPT_OK;
}
int mcpt_debug_occ_stats(const mcpt_ctx* c, uint64_t* resolved, int32_t* enabled) {
    if (!c) return MCPT_E_INVALID;
    if (resolved) *resolved = c->cnt.totals_ok ? c->cnt.totals.tot_occ : 0;
    if (enabled) *enabled = c->scene.dev.occ != nullptr;
    return MCPT_OK;
}

int mcpt_camera_set(mcpt_ctx* c, const mcpt_camera* cam) {
    if (!c || !cam) return set_err(c, MCPT_E_INVALID, "null argument");
    mcpt::CamView nc = c->cam;
    memcpy(nc.ivp, cam->inv_view_proj, sizeof(nc.ivp));
    memcpy(nc.iv, cam->inv_view, sizeof(nc.iv));
    nc.lens_radius = cam->lens_radius;
    nc.focal = cam->focal;
    if (c->has_cam && memcmp(&nc, &c->cam, sizeof(nc)) != 0) c->film_stale = true;
    c->cam = nc;
    c->has_cam = true;
    return MCPT_OK;
}

// The emission table of the uploaded scene's materials.  What the film depends on
// is the table's values, an absent table counting as zeros: a call that changes them is a change of the
// lighting, seen by the film as a camera change is, and by the temporal history as a scene change.
int mcpt_set_material_emission(mcpt_ctx* c, int32_t nmat, const float* rgb) {
    if (!c) return MCPT_E_INVALID;
    if (!c->scene.ok) return set_err(c, MCPT_E_INVALID, "no scene uploaded");
    Emission& em = c->em;
    const size_t n = 3 * (size_t)c->scene.nmat;
    std::vector<float> now(n, 0.f);
    if (rgb) {
        if (nmat != c->scene.nmat) return set_err(c, MCPT_E_INVALID, "nmat differs from the uploaded scene's");
        for (size_t i = 0; i < n; i++)
            if (!(rgb[i] >= 0.f) || !(rgb[i] <= 3.402823466e+38f))
                return set_err(c, MCPT_E_INVALID, "emission must be finite and >= 0");
        now.assign(rgb, rgb + n);
    }
    const std::vector<float> was = em.rgb.empty() ? std::vector<float>(n, 0.f) : em.rgb;
    const bool changed = n && memcmp(was.data(), now.data(), n * sizeof(float)) != 0;
    if (changed || (rgb && em.rgb.empty())) {
        std::vector<float4> t4(c->scene.nmat);
        int32_t lit = 0;
        for (int32_t m = 0; m < c->scene.nmat; m++) {
            t4[m] = make_float4(now[3 * m], now[3 * m + 1], now[3 * m + 2], 0.f);
            lit += now[3 * m] != 0.f || now[3 * m + 1] != 0.f || now[3 * m + 2] != 0.f;
        }
        HIPCHK(c, hipSetDevice(c->device));
        HIPCHK(c, hipStreamSynchronize(c->stream));  // no launch in flight reads the old table
        if (!em.tab.ensure(t4.size())) {
            em.drop();
            return set_err(c, MCPT_E_NOMEM, "hipMalloc: emission table");
        }
        em.lit = 0;  // (a failed copy leaves a table the kernels never read)
        if (!t4.empty()) HIPCHK(c, hipMemcpy(em.tab, t4.data(), t4.size() * sizeof(float4), hipMemcpyHostToDevice));
        em.lit = lit;
    }
    if (rgb) em.rgb = now;
    else em.drop();
    if (changed) {
        c->film_stale = true;
        c->tp.ok = false;  // the history's colours belong to the old lighting
        return emitter_table_refresh(c);  // emitter sampling's table follows the emission (section 17)
    }
    return MCPT_OK;
}

int mcpt_material_emission_read(mcpt_ctx* c, float* rgb, int32_t* nmat) {
    if (!c || !nmat) return set_err(c, MCPT_E_INVALID, "null argument");
    const Emission& em = c->em;
    *nmat = (int32_t)(em.rgb.size() / 3);
    if (em.rgb.empty()) return 0;
    if (rgb) memcpy(rgb, em.rgb.data(), em.rgb.size() * sizeof(float));
    return em.lit;
}

// ---- emitter sampling ----
// The any-hit queue holds two rays per material evaluation, three while emitter sampling is active:
// the queues are re-sized for the current tile set when that changes.
static int emitter_queues(mcpt_ctx* c) {
    const uint32_t mult = c->es.active() ? 3u : 2u;
    if (c->any_mult == mult || !c->film.allocated) {
        c->any_mult = mult;
        return MCPT_OK;
    }
    c->any_mult = mult;
    return set_tiles_internal(c, std::vector<int2>(c->tiles.host));
}

// pick_rec: the table's pick keyed by triangle record, from the device entries of
// the current table, while MIS is in effect; dropped otherwise.  It follows the table: rebuilt with
// every table build (the record order may have changed) and when the MIS switch turns on.
static int emitter_pick_refresh(mcpt_ctx* c) {
    EmitterSampling& es = c->es;
    const uint32_t ntri = c->scene.ok ? c->scene.dev.ntri : 0u;
    if (!es.mis_active() || !ntri) {
        es.drop_pick();
        return MCPT_OK;
    }
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));  // no launch in flight reads the old array
    es.pick_ok = false;
    if (!es.pick_rec.ensure(ntri)) {
        es.drop_pick();
        return set_err(c, MCPT_E_NOMEM, "hipMalloc: emitter pick table");
    }
    launch_emitter_pick_rec(es.ent, (uint32_t)es.tab.cdf.size(), es.pick_rec, ntri, c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    es.pick_ok = true;
    return MCPT_OK;
}

extern "C++" int emitter_table_refresh(mcpt_ctx* c) {
    EmitterSampling& es = c->es;
    if (!es.on || !c->scene.ok) return MCPT_OK;
    const bool was_active = es.active();
    mcpt_host::EmitterTable now;
    es.build_ms = 0.f;
    es.pick_ok = false;  // (belongs to the entries about to be replaced; emitter_pick_refresh below)
    const float4* emis = c->em.dev_table();
    const uint32_t ntri = c->scene.dev.ntri;
    HIPCHK(c, hipSetDevice(c->device));
    if (emis && ntri) {
        TmpScope tmp(c);
        float* dw = nullptr;
        uint32_t* did = nullptr;
        int rc;
        if ((rc = dalloc(c, tmp.L, &dw, ntri)) || (rc = dalloc(c, tmp.L, &did, ntri))) return rc;
        const auto t0 = std::chrono::steady_clock::now();
        launch_emitter_weights(c->scene.dev, emis, dw, did, c->stream);
        HIPCHK(c, hipGetLastError());
        std::vector<float> w(ntri);
        std::vector<uint32_t> id(ntri);
        HIPCHK(c, hipMemcpyAsync(w.data(), dw, ntri * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(id.data(), did, ntri * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        mcpt_host::build_emitter_table(w.data(), id.data(), ntri, now);
        const size_t n = now.cdf.size();
        if (n) {
            std::vector<uint2> ent(n);
            for (size_t k = 0; k < n; k++) {
                uint32_t bits;
                memcpy(&bits, &now.pick[k], sizeof(bits));
                ent[k] = make_uint2(now.rec[k], bits);
            }
            if (!es.cdf.ensure(n) || !es.ent.ensure(n)) {
                es.drop_table();
                return set_err(c, MCPT_E_NOMEM, "hipMalloc: emitter table");
            }
            // (the stream is idle: no launch in flight reads the old arrays)
            HIPCHK(c, hipMemcpy(es.cdf, now.cdf.data(), n * sizeof(float), hipMemcpyHostToDevice));
            HIPCHK(c, hipMemcpy(es.ent, ent.data(), n * sizeof(uint2), hipMemcpyHostToDevice));
        }
        es.build_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    // The record indices are the tree's business: the film depends on the entries' triangles and values
    const bool changed = !(now.cdf == es.tab.cdf && now.pick == es.tab.pick && now.id == es.tab.id);
    es.tab = std::move(now);
    if (changed || was_active != es.active()) {
        c->film_stale = true;
        c->tp.ok = false;
    }
    if (!es.active()) es.drop_streams();
    if (int rc = emitter_pick_refresh(c)) return rc;
    return emitter_queues(c);
}

int mcpt_set_emitter_sampling(mcpt_ctx* c, int32_t on) {
    if (!c) return MCPT_E_INVALID;
    EmitterSampling& es = c->es;
    if (es.on == (on != 0)) return MCPT_OK;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    es.on = on != 0;
    // the switch itself changes the estimator: the film restarts, as with a change of the emission
    c->film_stale = true;
    c->tp.ok = false;
    if (es.on) return emitter_table_refresh(c);
    es.drop_table();
    es.drop_streams();
    return emitter_queues(c);
}

// ---- MIS between emitter samples and collected emission ----
int mcpt_set_emitter_mis(mcpt_ctx* c, int32_t on) {
    if (!c) return MCPT_E_INVALID;
    EmitterSampling& es = c->es;
    if (es.mis == (on != 0)) return MCPT_OK;
    es.mis = on != 0;
    if (!es.active()) return MCPT_OK;  // takes effect with sampling, whose own changes restart the film
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    // the estimator changes: the film restarts, as with mcpt_set_emitter_sampling
    c->film_stale = true;
    c->tp.ok = false;
    return emitter_pick_refresh(c);
}

int mcpt_debug_emitter_mis(const mcpt_ctx* c) {
    if (!c) return MCPT_E_INVALID;
    return c->es.mis_active() ? 1 : 0;
}

int mcpt_emitter_table_read(mcpt_ctx* c, float* cdf, float* pick, uint32_t* tri_id, int32_t* n) {
    if (!c || !n) return set_err(c, MCPT_E_INVALID, "null argument");
    const mcpt_host::EmitterTable& t = c->es.tab;
    *n = (int32_t)t.cdf.size();
    if (cdf && *n) memcpy(cdf, t.cdf.data(), t.cdf.size() * sizeof(float));
    if (pick && *n) memcpy(pick, t.pick.data(), t.pick.size() * sizeof(float));
    if (tri_id && *n) memcpy(tri_id, t.id.data(), t.id.size() * sizeof(uint32_t));
    return MCPT_OK;
}

static unsigned long long emit_rays(const mcpt_ctx* c) {
    unsigned long long s = 0;
    if (c->cnt.totals_ok)
        for (int k = 0; k < kShards; k++) s += c->cnt.totals.tot_emit[k];
    return s;
}

int mcpt_debug_emitter_stats(const mcpt_ctx* c, double* out4) {
    if (!c || !out4) return MCPT_E_INVALID;
    out4[0] = (double)c->es.tab.cdf.size();
    out4[1] = c->es.tab.total;
    out4[2] = (double)emit_rays(c);
    out4[3] = (double)c->es.build_ms;
    return c->es.active() ? 1 : 0;
}

extern "C++" hipEvent_t ev(mcpt_ctx* c, size_t i) {
    while (c->events.size() <= i) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return nullptr;
        c->events.push_back(e);
    }
    return c->events[i];
}

// The camera records of a W x H film under the current camera (k_cam_table: gen_ray_pixel of every
// pixel, 32 B each), rebuilt on the context's stream when the film size or the camera changed.
extern "C++" int cam_table(mcpt_ctx* c, uint32_t W, uint32_t H, const float4** px, const float4** dir) {
    const size_t n = (size_t)W * H;
    CamTable& t = c->cam_tab;
    ViewKey key = c->view();
    key.W = W;
    key.H = H;
    if (!(t.ok && t.key.same(key, ViewKey::SIZE | ViewKey::CAM))) {
        if (2 * n > t.tab.size()) {
            HIPCHK(c, hipStreamSynchronize(c->stream));
            t.ok = false;
            if (!t.tab.ensure(2 * n)) return set_err(c, MCPT_E_NOMEM, "camera table allocation failed");
        }
        launch_cam_table(c->cam, (int)W, (int)H, t.tab, t.tab + n, c->stream);
        HIPCHK(c, hipGetLastError());
        t.key = key;
        t.ok = true;
    }
    *px = t.tab;
    *dir = t.tab + n;
    return MCPT_OK;
}

// The primary-hit candidate table of the W x H film under the current scene and camera
// (k_primary_build over the camera records), built on the context's stream when one of the three
// changed; a film clear leaves it alone.  Best-effort: when a precondition is missing (no leaf-box
// records: MCPT_PRIMARY_HITS=0, or boxes that do not nest), or an allocation or the launch fails, sa's
// table pointers stay null and the primary rays are traversed as before.  Never an error.
static void prim_table(mcpt_ctx* c, ShadeArgs& sa) {
    sa.prim_cnt = nullptr;
    sa.prim_list = nullptr;
    sa.prim_q = nullptr;
    PrimTable& t = c->prim;
    if (!t.on || !c->scene.dev.occ_rec || !c->scene.nest_ok || c->scene.ntri == 0) return;
    const uint32_t W = c->W, H = c->H;
    const size_t n = (size_t)W * H;
    const ViewKey key = c->view();
    const bool same = t.key.same(key, ViewKey::SCENE | ViewKey::SIZE | ViewKey::CAM);
    if (same && t.failed) return;
    const size_t qn = c->queues.need;
    auto fail = [&]() {
        (void)hipGetLastError();
        (void)hipStreamSynchronize(c->stream);
        t.release();
        t.failed = true;
        t.lists = t.over = 0;
    };
    if (!same) {
        t.key = key;
        t.failed = false;
        t.ok = false;
    }
    if (!t.ok) {
        if (n > t.cnt.size() || !t.stats) {
            (void)hipStreamSynchronize(c->stream);
            t.release();
            if (!t.cnt.ensure(n) || !t.list.ensure(n * kPrimLine) || !t.stats.ensure(4)) return fail();
        }
        PrimaryBuildArgs ba{};
        ba.scene = c->scene.dev;
        ba.cam = c->cam;
        ba.W = (int)W;
        ba.H = (int)H;
        ba.cam_px = sa.cam_px;
        ba.cam_dir = sa.cam_dir;
        ba.cnt = t.cnt;
        ba.list = t.list;
        ba.stats = t.stats;
        hipEvent_t e0 = nullptr, e1 = nullptr;
        uint32_t st[2] = {0, 0};
        float ms = 0.f;
        const bool ok = hipEventCreate(&e0) == hipSuccess && hipEventCreate(&e1) == hipSuccess &&
                        hipMemsetAsync(t.stats, 0, 16, c->stream) == hipSuccess &&
                        hipEventRecord(e0, c->stream) == hipSuccess &&
                        (launch_primary_build(ba, c->stream), hipGetLastError() == hipSuccess) &&
                        hipEventRecord(e1, c->stream) == hipSuccess &&
                        hipMemcpyAsync(st, t.stats, sizeof(st), hipMemcpyDeviceToHost, c->stream) == hipSuccess &&
                        hipStreamSynchronize(c->stream) == hipSuccess && hipEventElapsedTime(&ms, e0, e1) == hipSuccess;
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
        if (!ok) return fail();
        t.ok = true;
        t.builds++;
        t.lists = st[0];
        t.over = st[1];
        t.build_ms = ms;
    }
    if (qn > t.q.size()) {  // the primary queue follows the ray queues' capacity (RayQueues::ensure)
        (void)hipStreamSynchronize(c->stream);
        if (!t.q.ensure(qn)) return fail();
    }
    sa.prim_cnt = t.cnt;
    sa.prim_list = t.list;
    sa.prim_q = t.q;
}

extern "C++" int check_ready(mcpt_ctx* c) {
    if (!c) return MCPT_E_INVALID;
    if (!c->scene.ok) return set_err(c, MCPT_E_INVALID, "no scene uploaded");
    if (!c->has_cam) return set_err(c, MCPT_E_INVALID, "no camera set");
    if (!c->film.allocated) return set_err(c, MCPT_E_INVALID, "film not allocated");
    if (!c->queues.ready())  // a failed (re)allocation left none
        return set_err(c, MCPT_E_NOMEM, "ray queues not allocated");
    return MCPT_OK;
}

// One wavefront iteration over the current tile set: shade -> extend -> any-hit.
static int enqueue_iteration(mcpt_ctx* c, size_t evbase, bool timing, const int2* tiles, int ntiles, const int* tile_base) {
    const FilmState& f = c->film;
    const RayQueues& q = c->queues;
    CounterBlock* const cnt = c->cnt.dev;
    ShadeArgs sa;
    sa.scene = c->scene.dev;
    sa.cam = c->cam;
    sa.p = f.paths(q);
    sa.tiles = tiles;
    sa.ntiles = ntiles;
    sa.tile_w = (int)c->tile_w;
    sa.tile_h = (int)c->tile_h;
    sa.W = (int)c->W;
    sa.H = (int)c->H;
    sa.spp = c->cfg.spp;
    sa.max_depth = c->cfg.max_depth;
    sa.rr_depth = c->cfg.rr_depth;
    sa.seed = c->cfg.seed;
    sa.slots = (int)c->slots;
    sa.slots_rcp = 1.0f / (float)c->slots;
    sa.npx = (uint32_t)f.L.npx;
    sa.compact = c->compact ? 1 : 0;
    sa.tile_base = tile_base;
    sa.ext_q = q.ext;
    sa.any_q = q.any;
    sa.mat_rec = reinterpret_cast<uint4*>(q.mat.get());
    sa.mat_beta = reinterpret_cast<float4*>(q.mat.get()) + q.need;
    sa.ext_cap = q.ext_cap;
    sa.any_cap = q.any_cap;
    sa.cnt = cnt;
    sa.blk_done = c->blk_done_off ? nullptr : f.blk_done.get();
    sa.skip = c->skip_discarded ? 1 : 0;
    sa.budget = c->ad.budget_on ? c->ad.budget.get() : nullptr;
    sa.emis = c->em.dev_table();
    // emitter sampling (section 17): its table and streams only while it is active (run_iterations sized them)
    const bool samp = c->es.active() && sa.emis && c->es.nee2.get() && c->es.vis.get();
    sa.emit_cdf = samp ? c->es.cdf.get() : nullptr;
    sa.emit_ent = samp ? c->es.ent.get() : nullptr;
    sa.emit_n = samp ? (int)c->es.tab.cdf.size() : 0;
    sa.emit_vis0 = samp ? (uint32_t)(2 * c->es.paths) : 0u;
    sa.nee2 = samp ? c->es.nee2.get() : nullptr;
    // ... and MIS (section 18) only while it is in effect, with pick_rec of the current table
    if (samp && c->es.mis && !(c->es.pick_ok && c->es.pick_rec.get()))
        return set_err(c, MCPT_E_INVALID, "emitter MIS: no pick table for the current emitter table");
    sa.pick_rec = samp && c->es.mis ? c->es.pick_rec.get() : nullptr;
    if (samp) sa.p.vis = c->es.vis;  // 3P bytes: the emitter rays' results behind the two of every path
    // base-colour textures (section 19): only a set with a textured material, in the current record order
    // (a metallic-roughness textured material counts as well: section 20)
    if (c->tx.shaded() && !c->tx.dev_ok)
        return set_err(c, MCPT_E_INVALID, "textures: no uv stream for the current record order");
    sa.tex = c->tx.view();
    if (int rc = cam_table(c, c->W, c->H, &sa.cam_px, &sa.cam_dir)) return rc;
    prim_table(c, sa);
    const int bpt = (int)f.L.blocks_per_tile;
    if (timing) HIPCHK(c, hipEventRecord(ev(c, evbase + 0), c->stream));
    if (sa.ntiles > 0)
        launch_shade(sa, sa.ntiles * bpt, c->geom, (c->cfg.flags & MCPT_FLAG_FIXED) != 0, c->tx.level(), c->stream);
    if (timing) HIPCHK(c, hipEventRecord(ev(c, evbase + 1), c->stream));
    // primary rays with a candidate list (part of the extend stage's time)
    if (sa.ntiles > 0) launch_primary(sa, c->geom, c->stream);
    // extension (closest hit) and any-hit rays in one persistent launch
    TraceArgs ta{};
    ta.scene = c->scene.dev;
    ta.nshards = kShards;
    TraceSet& e = ta.set[0];
    e.ro = sa.p.ray_o;
    e.rd = sa.p.ray_d;
    e.queue = q.ext;
    e.count_ptr = &cnt->shard[0][C_EXT];
    e.shard_cap = q.ext_cap;
    e.stats = c->count_work ? &cnt->shard[0][C_STATS] : nullptr;  // mcpt_set_work_counters
    e.prefiltered = 1;  // k_shade queues only rays that enter the root box
    TraceSet& v = ta.set[1];
    v.ro = sa.p.sray_o;
    v.rd = sa.p.sray_d;
    v.queue = q.any;
    v.count_ptr = &cnt->shard[0][C_ANY];
    v.shard_cap = q.any_cap;
    v.stats = c->count_work ? &cnt->shard[0][C_STATS + 3] : nullptr;
    v.prefiltered = 1;
    v.ray_at_slot = 1;  // k_material stores the any-hit rays at their queue positions
    ta.phase = c->count_work ? &cnt->shard[0][C_PH] : nullptr;  // loop-phase counts (mcpt_debug_trace_profile)
    ta.hit_tri = sa.p.hit_tri;
    ta.vis = sa.p.vis;
    ta.grab = &cnt->grab[0][0];  // reset by k_accumulate below
    ta.idle = &cnt->idle;
    ta.tiny_stack = c->tiny_stack ? 1 : 0;
    launch_trace(ta, c->geom, c->stream);
    if (timing) HIPCHK(c, hipEventRecord(ev(c, evbase + 2), c->stream));
    launch_accumulate(cnt, c->geom.trace_parts, c->scene.dev.occ ? c->scene.dev.occ_gate : nullptr, c->stream);
    HIPCHK(c, hipGetLastError());
    return MCPT_OK;
}

// n iterations over a tile set (the context's, or one tile for mcpt_wavefront_step).  One
// host synchronisation per call: the counter totals before the call are the host copy the
// previous call (or the film clear) left.
static int run_iterations(mcpt_ctx* c, uint32_t n, mcpt_stage_stats* st, const int2* tiles = nullptr, int ntiles = -1,
                          const int* tile_base = nullptr) {
    int rc = check_ready(c);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    if (c->film_stale && !(c->cfg.flags & MCPT_FLAG_NO_AUTO_CLEAR) && (rc = mcpt_film_clear(c))) return rc;
    if (c->es.active()) {
        // Emitter sampling's per-path streams (section 17), allocated like nee0 for the current path
        // count and only while sampling is active: the emitter terms, and the any-hit results with a
        // third byte per path (the film's own two-byte array rests meanwhile).
        EmitterSampling& es = c->es;
        const size_t paths = c->film.L.paths;
        if (es.paths != paths || !es.nee2.get() || !es.vis.get()) {
            if (const char* e = emitter_paths_error(paths)) return set_err(c, MCPT_E_INVALID, e);
            HIPCHK(c, hipStreamSynchronize(c->stream));
            es.drop_streams();
            if (!es.nee2.ensure(paths) || !es.vis.ensure(3 * paths)) {
                es.drop_streams();
                return set_err(c, MCPT_E_NOMEM, "hipMalloc: emitter sampling streams");
            }
            HIPCHK(c, hipMemset(es.nee2, 0, paths * sizeof(float4)));
            HIPCHK(c, hipMemset(es.vis, 0, 3 * paths));
            es.paths = paths;
        }
    }
    if (!tiles) {
        tiles = c->tiles.dev;
        ntiles = (int)c->tiles.host.size();
    }
    if (!c->cnt.totals_ok && (rc = c->cnt.refresh(c))) return rc;
    const CounterBlock before = c->cnt.totals;
    // iterations after one that traced no ray skip their kernels (k_accumulate sets the flag):
    // mcpt_render's last batch of 32 no longer pays full launches for the finished film
    HIPCHK(c, hipMemsetAsync(&c->cnt.dev->idle, 0, sizeof(uint32_t), c->stream));
    for (uint32_t i = 0; i < n; i++) {
        // events for at most the first 4096 iterations of a call
        bool timing = i < 4096;
        if ((rc = enqueue_iteration(c, (size_t)3 * i, timing, tiles, ntiles, tile_base))) {
            c->cnt.totals_ok = false;
            return rc;
        }
    }
    if ((rc = c->cnt.refresh(c))) return rc;
    const CounterBlock& after = c->cnt.totals;
    if (after.trace_short != before.trace_short)  // k_accumulate's drain check (never expected)
        return set_err(c, MCPT_E_HIP, "k_trace left queued rays untraced in " +
                                          std::to_string(after.trace_short - before.trace_short) + " launch(es)");
    if (st) {
        memset(st, 0, sizeof(*st));
        st->extend_rays = after.tot_ext - before.tot_ext;
        st->vis_rays = after.tot_vis - before.tot_vis;
        st->shadow_rays = (after.tot_any - before.tot_any) - st->vis_rays;
        st->iterations = n;
        st->live_paths = after.last_live;
        st->ext_nodes = after.tot_stats[0] - before.tot_stats[0];
        st->ext_tests = after.tot_stats[1] - before.tot_stats[1];
        st->ext_hits = after.tot_stats[2] - before.tot_stats[2];
        st->any_nodes = after.tot_stats[3] - before.tot_stats[3];
        st->any_tests = after.tot_stats[4] - before.tot_stats[4];
        st->any_hits = after.tot_stats[5] - before.tot_stats[5];
        uint32_t tn = std::min<uint32_t>(n, 4096);
        for (uint32_t i = 0; i < tn; i++) {
            float a = 0, b = 0;
            HIPCHK(c, hipEventElapsedTime(&a, c->events[3 * i + 0], c->events[3 * i + 1]));
            HIPCHK(c, hipEventElapsedTime(&b, c->events[3 * i + 1], c->events[3 * i + 2]));
            st->ms_shade += a;
            st->ms_extend += b;  // extension + any-hit rays: one k_trace launch (ms_shadow stays 0)
        }
        st->ms_total = st->ms_shade + st->ms_extend + st->ms_shadow;
    }
    return MCPT_OK;
}

int mcpt_iterate(mcpt_ctx* c, uint32_t n, mcpt_stage_stats* st) { return run_iterations(c, n, st); }

int mcpt_wavefront_step(mcpt_ctx* c, uint32_t tx, uint32_t ty, mcpt_stage_stats* st) {
    int rc = check_ready(c);
    if (rc) return rc;
    if (tx >= c->film.L.nx || ty >= c->film.L.ny) return set_err(c, MCPT_E_INVALID, "tile out of range");
    TileSet& ts = c->tiles;
    // compact layout: the tile's paths are those of its place in the tile set
    const int base = c->compact ? ts.index_of(make_int2((int)tx, (int)ty)) : 0;
    if (base < 0) return set_err(c, MCPT_E_INVALID, "compact paths: the tile is not in the tile set");
    // The one-tile set goes through its own small buffer (pinned staging, stream-ordered
    // copy): the context's tile set and queues stay as they are when their per-shard queue
    // capacity covers one tile, which it does unless the tile set is empty.
    if (c->queues.ext_cap >= one_tile_capacity(c->tile_w, c->tile_h, c->slots)) {
        if (!ts.step || !ts.step_h) {
            HIPCHK(c, hipSetDevice(c->device));
            if (!ts.step.ensure(2) || !ts.step_h.alloc(2))
                return set_err(c, MCPT_E_HIP, std::string("step tile allocation failed: ") + hipGetErrorString(hipGetLastError()));
        }
        ts.step_h.get()[0] = make_int2((int)tx, (int)ty);  // the previous call's copy has completed
        ts.step_h.get()[1] = make_int2(base, 0);
        HIPCHK(c, hipMemcpyAsync(ts.step, ts.step_h, 2 * sizeof(int2), hipMemcpyHostToDevice, c->stream));
        return run_iterations(c, 1, st, ts.step, 1, reinterpret_cast<const int*>(ts.step.get() + 1));
    }
    std::vector<int2> saved = ts.host;
    if ((rc = set_tiles_internal(c, {make_int2((int)tx, (int)ty)}))) return rc;
    rc = run_iterations(c, 1, st);
    int rc2 = set_tiles_internal(c, saved);
    return rc ? rc : rc2;
}

// acc += one batch: rays, iterations, work counts and times add up, the live paths are the last batch's
static void add(mcpt_stage_stats& acc, const mcpt_stage_stats& one) {
    acc.extend_rays += one.extend_rays, acc.shadow_rays += one.shadow_rays, acc.vis_rays += one.vis_rays;
    acc.iterations += one.iterations;
    acc.ms_shade += one.ms_shade, acc.ms_extend += one.ms_extend, acc.ms_shadow += one.ms_shadow, acc.ms_total += one.ms_total;
    acc.live_paths = one.live_paths;
    acc.ext_nodes += one.ext_nodes, acc.ext_tests += one.ext_tests, acc.ext_hits += one.ext_hits;
    acc.any_nodes += one.any_nodes, acc.any_tests += one.any_tests, acc.any_hits += one.any_hits;
}

int mcpt_render(mcpt_ctx* c, mcpt_stage_stats* st) {
    int rc = check_ready(c);
    if (rc) return rc;
    mcpt_stage_stats acc{}, one{};
    // the largest sample count in force: the budget map's maximum where one is installed
    const uint64_t spp = c->ad.budget_on ? (uint64_t)c->ad.budget_max : (uint64_t)c->cfg.spp;
    const uint64_t cap = (spp + 1) * (uint64_t)(c->cfg.max_depth + 2) + 16;
    uint64_t done = 0;
    // Iterations per batch (one host synchronisation each).  Once the film is done, the rest of a
    // batch are no-op launches (~24 us per iteration, mostly dispatching k_shade's grid), so the
    // first batch is sized to the expected frame -- samples per path slot x (max depth + 1)
    // iterations, the lockstep schedule of paths that all start together -- and later ones are
    // short.  (Config 2 at N = 8: 12 iterations of work ran in a batch of 32.)
    const uint64_t expect = ((spp + c->slots - 1) / c->slots) * (uint64_t)(c->cfg.max_depth + 1);
    for (;;) {
        const uint32_t batch = (uint32_t)std::min<uint64_t>(64, std::max<uint64_t>(8, expect > done ? expect - done : 0));
        if ((rc = run_iterations(c, batch, &one))) return rc;
        add(acc, one);
        done += one.iterations;
        if (one.live_paths == 0 || done > cap) break;
    }
    if (st) *st = acc;
    if (acc.live_paths != 0) return set_err(c, MCPT_E_INVALID, "render did not converge within the iteration cap");
    return MCPT_OK;
}

int mcpt_sync(mcpt_ctx* c) {
    if (!c) return MCPT_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MCPT_OK;
}

int mcpt_set_work_counters(mcpt_ctx* c, int32_t on) {
    if (!c) return MCPT_E_INVALID;
    c->count_work = on != 0;
    return MCPT_OK;
}

int mcpt_set_skip_discarded(mcpt_ctx* c, int32_t on) {
    if (!c) return MCPT_E_INVALID;
    c->skip_discarded = on != 0;  // read per iteration (enqueue_iteration): may change between calls
    return MCPT_OK;
}

int mcpt_set_trace_partitions(mcpt_ctx* c, uint32_t nparts) {
    if (!c || nparts > (uint32_t)kMaxParts)
        return set_err(c, MCPT_E_INVALID, "trace partitions must be 0 (device default) .. " + std::to_string(kMaxParts));
    c->geom.trace_parts = nparts ? nparts : c->trace_parts_default;
    return MCPT_OK;
}

}  // extern "C"
