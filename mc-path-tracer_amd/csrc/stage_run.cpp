// stage_run.cpp -- the per-stage parity harness (mcpt_stage_run) and the mcpt_debug_* entries that do
// more than read context state.  Test and diagnostics paths over the product's kernels: the context,
// the film and the render loop are runtime.cpp.
#include "runtime_internal.hpp"

// mcpt_stage_run(LOGIC | GENERATE | MATERIAL): the product's shading kernels (k_shade: wf_logic
// + wf_generate; k_material: light choice + wf_mat_mix) over caller path state of n paths in
// scratch device buffers -- the per-stage parity harness of SURVEY.md 8(b) / section 4 item 2.
// The context's film, queues and counters are not touched.
static int stage_run_paths(mcpt_ctx* c, int stage, const mcpt_path_view* in, mcpt_path_view* out, uint32_t n) {
    const bool mat = stage == MCPT_STAGE_MATERIAL, gen = stage == MCPT_STAGE_GENERATE;
    if (!in || !out) return set_err(c, MCPT_E_INVALID, "stage needs in->paths and out->paths");
    uint32_t W = n, H = 1;
    if (!mat) {
        W = in->film_w;
        H = in->film_h;
        if (!c->has_cam) return set_err(c, MCPT_E_INVALID, "no camera set");
        if ((uint64_t)W * H != n || W < 2 || H < 2) return set_err(c, MCPT_E_INVALID, "film_w * film_h must equal n (>= 2 x 2)");
    }
    if (n >= (1u << 26)) return set_err(c, MCPT_E_INVALID, "too many paths for one stage call");
    if (mat && in->hit_tri)  // k_material rebuilds the hit record from the triangle: it must exist
        for (uint32_t i = 0; i < n; i++)
            if (in->hit_tri[i] < 0 || in->hit_tri[i] >= c->scene.ntri)
                return set_err(c, MCPT_E_INVALID, "MATERIAL: every path needs a hit (0 <= hit_tri < ntri)");
    if (stage == MCPT_STAGE_LOGIC && in->hit_tri && c->em.dev_table())  // the emission lookup reads the hit's record
        for (uint32_t i = 0; i < n; i++)
            if (in->hit_tri[i] >= c->scene.ntri)
                return set_err(c, MCPT_E_INVALID, "LOGIC with emission: hit_tri must be < ntri");
    if (!in->hit_tri || !in->flags || (!gen && (!in->ray_d || !in->beta)) || (!mat && !in->samples) ||
        (mat && !in->ray_o) || (stage == MCPT_STAGE_LOGIC && (!in->nee0 || !in->nee1 || !in->vis || !in->Ld)))
        return set_err(c, MCPT_E_INVALID, "missing path-state input");
    HIPCHK(c, hipSetDevice(c->device));
    TmpScope tmp(c);
    auto& L = tmp.L;
    // shard capacity: LOGIC blocks of 256 paths push into shard block mod 64; MATERIAL records are
    // dealt to shards i mod 64
    const uint32_t nblocks = (uint32_t)shade_blocks_per_tile((int)n, 1);
    const uint32_t per_shard = mat ? (n + kShards - 1) / kShards : ((nblocks + kShards - 1) / kShards) * kBlock;
    const uint32_t ext_cap = std::max<uint32_t>(kBlock, (per_shard + kBlock - 1) / kBlock * kBlock), any_cap = 2 * ext_cap;
    const size_t qn = (size_t)kShards * ext_cap;
    DevPaths p{};
    uint32_t *ext_q, *any_q;
    uint4* mrec;
    float4* mbeta;
    CounterBlock* cnt;
    int2* tl;
    int rc;
    if ((rc = dalloc(c, L, &p.ray_o, n)) || (rc = dalloc(c, L, &p.ray_d, n)) || (rc = dalloc(c, L, &p.beta, n)) ||
        (rc = dalloc(c, L, &p.nee0, n)) || (rc = dalloc(c, L, &p.nee1, n)) || (rc = dalloc(c, L, &p.Ld, n)) ||
        (rc = dalloc(c, L, &p.hit_tri, n)) || (rc = dalloc(c, L, &p.flags, n)) || (rc = dalloc(c, L, &p.samples, n)) ||
        (rc = dalloc(c, L, &p.vis, 2 * (size_t)n)) ||
        (rc = dalloc(c, L, &p.sray_o, 2 * qn)) || (rc = dalloc(c, L, &p.sray_d, 2 * qn)) ||
        (rc = dalloc(c, L, &ext_q, qn)) || (rc = dalloc(c, L, &any_q, 2 * qn)) || (rc = dalloc(c, L, &mrec, qn)) ||
        (rc = dalloc(c, L, &mbeta, qn)) || (rc = dalloc(c, L, &cnt, 1)) || (rc = dalloc(c, L, &tl, 1)))
        return rc;
    auto f4v = [n](const float* a, int k, float w) {  // host k-float SoA -> float4 (w pad)
        std::vector<float4> v(n, make_float4(0.f, 0.f, 0.f, w));
        if (a)
            for (uint32_t i = 0; i < n; i++)
                v[i] = make_float4(a[k * i], a[k * i + 1], a[k * i + 2], k == 4 ? a[4 * i + 3] : w);
        return v;
    };
    auto up = [&](void* d, const void* h, size_t bytes) -> hipError_t {
        return hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, c->stream);
    };
    std::vector<float4> ro = f4v(in->ray_o, 3, 0.f), rd = f4v(in->ray_d, 3, 0.f), be = f4v(in->beta, 4, 0.f),
                        n0 = f4v(in->nee0, 4, 0.f), n1 = f4v(in->nee1, 4, 0.f), ld = f4v(in->Ld, 3, 0.f);
    std::vector<uint32_t> fl(in->flags, in->flags + n), sm(n, 0u);
    if (in->samples) sm.assign(in->samples, in->samples + n);
    if (gen) std::fill(fl.begin(), fl.end(), (uint32_t)F_DEAD);
    if (!mat) {
        // The device's flags word carries a dead path's next sample index too, and k_shade derives
        // the film's sample count from it (one path slot here: sample index = count).  In: a dead
        // path's index is its samples; a live path's must equal them (the oracle's and the
        // reference's states always agree: samples changes only when a path ends).  Out: dead
        // paths' flags as the interface has them (F_DEAD alone).
        for (uint32_t i = 0; i < n; i++) {
            if (fl[i] & F_DEAD) fl[i] = (uint32_t)F_DEAD | (sm[i] << F_SIDX_SHIFT);
            else if ((fl[i] >> F_SIDX_SHIFT) != sm[i])
                return set_err(c, MCPT_E_INVALID, "LOGIC: a live path's sample index (flags) must equal its samples");
            if (sm[i] >= kMaxSpp) return set_err(c, MCPT_E_INVALID, "samples must be < 2^19");
        }
    }
    std::vector<uint8_t> vis(2 * (size_t)n, 0);
    if (in->vis) vis.assign(in->vis, in->vis + 2 * (size_t)n);
    CounterBlock* hc = c->cnt.host;  // pinned staging (the context's counters stay on the device)
    memset(hc, 0, sizeof(CounterBlock));
    std::vector<uint4> rec;
    std::vector<float4> rbeta;
    if (mat) {  // records {pid, len, sample index, hit_tri} + throughput, path i in shard i mod 64
        rec.assign(qn, make_uint4(0, 0, 0, 0));
        rbeta.assign(qn, make_float4(0.f, 0.f, 0.f, 0.f));
        for (uint32_t i = 0; i < n; i++) {
            const uint32_t sh = i % kShards, k = i / kShards;
            rec[(size_t)sh * ext_cap + k] = make_uint4(i, i, (fl[i] >> F_SIDX_SHIFT) | (((fl[i] >> F_LEN_SHIFT) & 0xffu) << kRecLenShift),
                                                       (uint32_t)in->hit_tri[i]);
            rbeta[(size_t)sh * ext_cap + k] = make_float4(be[i].x, be[i].y, be[i].z, 0.f);
            hc->shard[sh][C_MAT]++;
        }
    }
    const int2 tile0 = make_int2(0, 0);
    hipError_t e = hipSuccess;
    if (e == hipSuccess) e = up(p.ray_o, ro.data(), n * sizeof(float4));
    if (e == hipSuccess) e = up(p.ray_d, rd.data(), n * sizeof(float4));
    if (e == hipSuccess) e = up(p.beta, be.data(), n * sizeof(float4));
    if (e == hipSuccess) e = up(p.nee0, n0.data(), n * sizeof(float4));
    if (e == hipSuccess) e = up(p.nee1, n1.data(), n * sizeof(float4));
    if (e == hipSuccess) e = up(p.Ld, ld.data(), n * sizeof(float4));
    if (e == hipSuccess) e = up(p.hit_tri, in->hit_tri, n * sizeof(int32_t));
    if (e == hipSuccess) e = up(p.flags, fl.data(), n * sizeof(uint32_t));
    if (e == hipSuccess) e = up(p.samples, sm.data(), n * sizeof(uint32_t));
    if (e == hipSuccess) e = up(p.vis, vis.data(), 2 * (size_t)n);
    if (e == hipSuccess) e = up(cnt, hc, sizeof(CounterBlock));
    if (e == hipSuccess) e = up(tl, &tile0, sizeof(int2));
    if (e == hipSuccess && mat) e = up(mrec, rec.data(), qn * sizeof(uint4));
    if (e == hipSuccess && mat) e = up(mbeta, rbeta.data(), qn * sizeof(float4));
    if (e != hipSuccess) return set_err(c, MCPT_E_HIP, std::string("stage upload: ") + hipGetErrorString(e));
    ShadeArgs sa{};
    sa.scene = c->scene.dev;
    sa.scene.occ = nullptr;  // stage runs: outputs of the stage alone (no occluder cache)
    sa.cam = c->cam;
    sa.p = p;
    sa.tiles = tl;
    sa.ntiles = 1;
    sa.tile_w = (int)W;
    sa.tile_h = (int)H;
    sa.W = (int)W;
    sa.H = (int)H;
    sa.spp = c->cfg.spp;
    sa.max_depth = c->cfg.max_depth;
    sa.rr_depth = c->cfg.rr_depth;
    sa.seed = c->cfg.seed;
    sa.slots = 1;
    sa.slots_rcp = 1.0f;
    sa.npx = n;  // path i is pixel i of the W x H stage film
    if ((rc = cam_table(c, W, H, &sa.cam_px, &sa.cam_dir))) return rc;
    sa.ext_q = ext_q;
    sa.any_q = any_q;
    sa.mat_rec = mrec;
    sa.mat_beta = mbeta;
    sa.ext_cap = ext_cap;
    sa.any_cap = any_cap;
    sa.cnt = cnt;
    if (stage == MCPT_STAGE_LOGIC) sa.emis = c->em.dev_table();  // the context's emission
    if (mat) sa.tex = c->tx.view();  // ... and its base-colour textures (section 19)
    HIPCHK(c, hipEventRecord(ev(c, 0), c->stream));
    launch_shade_stage(mat, sa, (int)nblocks, c->geom, (c->cfg.flags & MCPT_FLAG_FIXED) != 0, c->tx.level(), c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(ev(c, 1), c->stream));
    HIPCHK(c, hipMemcpyAsync(hc, cnt, sizeof(CounterBlock), hipMemcpyDeviceToHost, c->stream));
    std::vector<float4> o_ro(n), o_rd(n), o_be(n), o_n0(n), o_n1(n), o_ld(n);
    std::vector<uint32_t> o_fl(n), o_sm(n), o_eq(qn);
    std::vector<int32_t> o_ht(n);
    std::vector<uint8_t> o_vis(2 * (size_t)n);
    std::vector<uint4> o_rec(qn);
    std::vector<float4> o_rb(qn), o_so(2 * qn), o_sd(2 * qn);
    auto dn = [&](void* h, const void* d, size_t bytes) -> hipError_t {
        return hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, c->stream);
    };
    if (e == hipSuccess) e = dn(o_ro.data(), p.ray_o, n * sizeof(float4));
    if (e == hipSuccess) e = dn(o_rd.data(), p.ray_d, n * sizeof(float4));
    if (e == hipSuccess) e = dn(o_be.data(), p.beta, n * sizeof(float4));
    if (e == hipSuccess) e = dn(o_n0.data(), p.nee0, n * sizeof(float4));
    if (e == hipSuccess) e = dn(o_n1.data(), p.nee1, n * sizeof(float4));
    if (e == hipSuccess) e = dn(o_ld.data(), p.Ld, n * sizeof(float4));
    if (e == hipSuccess) e = dn(o_fl.data(), p.flags, n * sizeof(uint32_t));
    if (e == hipSuccess) e = dn(o_sm.data(), p.samples, n * sizeof(uint32_t));
    if (e == hipSuccess) e = dn(o_ht.data(), p.hit_tri, n * sizeof(int32_t));
    if (e == hipSuccess) e = dn(o_vis.data(), p.vis, 2 * (size_t)n);
    if (e == hipSuccess) e = dn(o_eq.data(), ext_q, qn * sizeof(uint32_t));
    if (e == hipSuccess) e = dn(o_rec.data(), mrec, qn * sizeof(uint4));
    if (e == hipSuccess) e = dn(o_rb.data(), mbeta, qn * sizeof(float4));
    if (e == hipSuccess) e = dn(o_so.data(), p.sray_o, 2 * qn * sizeof(float4));
    if (e == hipSuccess) e = dn(o_sd.data(), p.sray_d, 2 * qn * sizeof(float4));
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return set_err(c, MCPT_E_HIP, std::string("stage run: ") + hipGetErrorString(e));
    HIPCHK(c, hipEventElapsedTime(&c->last_stage_ms, c->events[0], c->events[1]));
    const float qnan = __builtin_nanf("");
    std::vector<uint8_t> queued(n, 0);
    std::vector<float> lo(3 * (size_t)n, qnan), ldr(3 * (size_t)n, qnan), bo(3 * (size_t)n, qnan), bd(3 * (size_t)n, qnan);
    for (int sh = 0; sh < kShards; sh++) {
        for (uint32_t k = 0; k < hc->shard[sh][C_EXT]; k++) queued[o_eq[(size_t)sh * ext_cap + k]] |= 1;
        if (!mat)
            for (uint32_t k = 0; k < hc->shard[sh][C_MAT]; k++) {  // continuing paths: their updated throughput
                const size_t q = (size_t)sh * ext_cap + k;
                const uint32_t pid = o_rec[q].x;
                queued[pid] |= 2;
                o_be[pid] = make_float4(o_rb[q].x, o_rb[q].y, o_rb[q].z, o_be[pid].w);
            }
        for (uint32_t k = 0; k < hc->shard[sh][C_ANY]; k++) {
            const size_t q = (size_t)sh * any_cap + k;
            uint32_t r;  // the ray's result index (2 pid + BRDF ray) rides in its origin's .w
            memcpy(&r, &o_so[q].w, sizeof(r));
            const uint32_t pid = r >> 1;
            float* so = (r & 1) ? bo.data() : lo.data();
            float* sd = (r & 1) ? bd.data() : ldr.data();
            queued[pid] |= (r & 1) ? 8 : 4;
            so[3 * pid] = o_so[q].x; so[3 * pid + 1] = o_so[q].y; so[3 * pid + 2] = o_so[q].z;
            sd[3 * pid] = o_sd[q].x; sd[3 * pid + 1] = o_sd[q].y; sd[3 * pid + 2] = o_sd[q].z;
        }
    }
    auto put3 = [n](float* dst, const std::vector<float4>& v) {
        if (dst)
            for (uint32_t i = 0; i < n; i++) { dst[3 * i] = v[i].x; dst[3 * i + 1] = v[i].y; dst[3 * i + 2] = v[i].z; }
    };
    auto put4 = [n](float* dst, const std::vector<float4>& v) {
        if (dst) memcpy(dst, v.data(), n * sizeof(float4));
    };
    if (!mat)
        for (uint32_t& f : o_fl)
            if (f & F_DEAD) f = F_DEAD;  // the interface's dead flags (the index lives in samples)
    if (out->flags) memcpy(out->flags, o_fl.data(), n * sizeof(uint32_t));
    if (out->samples) memcpy(out->samples, o_sm.data(), n * sizeof(uint32_t));
    if (out->hit_tri) memcpy(out->hit_tri, o_ht.data(), n * sizeof(int32_t));
    put3(out->ray_o, o_ro);
    put3(out->ray_d, o_rd);
    put4(out->beta, o_be);
    put4(out->nee0, o_n0);
    put4(out->nee1, o_n1);
    if (out->vis) memcpy(out->vis, o_vis.data(), 2 * (size_t)n);
    put3(out->Ld, o_ld);
    if (out->light_o) memcpy(out->light_o, lo.data(), 3 * (size_t)n * sizeof(float));
    if (out->light_d) memcpy(out->light_d, ldr.data(), 3 * (size_t)n * sizeof(float));
    if (out->bvis_o) memcpy(out->bvis_o, bo.data(), 3 * (size_t)n * sizeof(float));
    if (out->bvis_d) memcpy(out->bvis_d, bd.data(), 3 * (size_t)n * sizeof(float));
    if (out->queued) memcpy(out->queued, queued.data(), n);
    return MCPT_OK;
}

extern "C" {

int mcpt_stage_run(mcpt_ctx* c, int stage, const mcpt_soa_view* in, mcpt_soa_view* out, uint32_t n) {
    if (!c || !in || !out) return set_err(c, MCPT_E_INVALID, "null argument");
    if (!c->scene.ok) return set_err(c, MCPT_E_INVALID, "no scene uploaded");
    if (stage < MCPT_STAGE_LOGIC || stage > MCPT_STAGE_SHADOW) return set_err(c, MCPT_E_INVALID, "unknown stage");
    if (n == 0) return MCPT_OK;
    if (stage == MCPT_STAGE_LOGIC || stage == MCPT_STAGE_GENERATE || stage == MCPT_STAGE_MATERIAL)
        return stage_run_paths(c, stage, in->paths, out->paths, n);
    if (!in->ray_o || !in->ray_d) return set_err(c, MCPT_E_INVALID, "null rays");
    if (stage == MCPT_STAGE_EXTEND && (!out->hit_pos_t || !out->hit_nrm_mat)) return set_err(c, MCPT_E_INVALID, "null outputs");
    if (stage == MCPT_STAGE_SHADOW && !out->visible) return set_err(c, MCPT_E_INVALID, "null outputs");
    HIPCHK(c, hipSetDevice(c->device));
    TmpScope tmp(c);
    std::vector<float4> ro(n), rd(n);
    for (uint32_t i = 0; i < n; i++) {
        ro[i] = make_float4(in->ray_o[3 * i], in->ray_o[3 * i + 1], in->ray_o[3 * i + 2], 0.f);
        rd[i] = make_float4(in->ray_d[3 * i], in->ray_d[3 * i + 1], in->ray_d[3 * i + 2], 0.f);
    }
    float4 *dro, *drd, *hp = nullptr, *hn = nullptr;
    int32_t* ht = nullptr;
    uint8_t* vis = nullptr;
    int rc;
    if ((rc = dupload(c, tmp.L, &dro, ro.data(), n)) || (rc = dupload(c, tmp.L, &drd, rd.data(), n)))
        return rc;
    TraceArgs ta{};
    ta.scene = c->scene.dev;
    ta.scene.occ = nullptr;  // stage runs: outputs of the stage alone (no occluder cache)
    ta.nshards = 1;
    TraceSet& ts = ta.set[stage == MCPT_STAGE_SHADOW ? 1 : 0];
    ts.ro = dro;
    ts.rd = drd;
    ts.count = n;
    ts.shard_cap = n;
    if (stage == MCPT_STAGE_EXTEND) {
        if ((rc = dalloc(c, tmp.L, &hp, n)) || (rc = dalloc(c, tmp.L, &hn, n)) || (rc = dalloc(c, tmp.L, &ht, n)))
            return rc;
        ta.hit_tri = ht;
    } else {
        if ((rc = dalloc(c, tmp.L, &vis, n))) return rc;
        ta.vis = vis;
    }
    uint32_t* steps = nullptr;
    if (out->steps) {
        if ((rc = dalloc(c, tmp.L, &steps, n))) return rc;
        ts.ray_steps = steps;
    }
    ta.grab = &c->cnt.dev->grab[0][0];
    HIPCHK(c, hipEventRecord(ev(c, 0), c->stream));
    ta.tiny_stack = c->tiny_stack ? 1 : 0;
    launch_trace(ta, c->geom, c->stream);
    HIPCHK(c, hipEventRecord(ev(c, 1), c->stream));
    uint32_t grab0 = 0;  // drain check: the one shard is partition 0's
    HIPCHK(c, hipMemcpyAsync(&c->cnt.host->grab[0][0], &c->cnt.dev->grab[0][0], sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemsetAsync(c->cnt.dev->grab, 0, sizeof(c->cnt.dev->grab), c->stream));  // hand-out counters back to 0
    if (stage == MCPT_STAGE_EXTEND) {
        HitRecordArgs ha{c->scene.dev, dro, drd, ht, hp, hn, ht, n};  // ht: positions in, scene indices out
        launch_hit_record(ha, c->stream);
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipEventElapsedTime(&c->last_stage_ms, c->events[0], c->events[1]));
    grab0 = c->cnt.host->grab[0][0];
    if (grab0 < n) return set_err(c, MCPT_E_HIP, "k_trace left rays untraced");
    if (steps) HIPCHK(c, hipMemcpy(out->steps, steps, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (stage == MCPT_STAGE_EXTEND) {
        std::vector<float4> a(n), b(n);
        HIPCHK(c, hipMemcpy(a.data(), hp, n * sizeof(float4), hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(b.data(), hn, n * sizeof(float4), hipMemcpyDeviceToHost));
        std::vector<int32_t> t(n);
        HIPCHK(c, hipMemcpy(t.data(), ht, n * sizeof(int32_t), hipMemcpyDeviceToHost));
        for (uint32_t i = 0; i < n; i++) {
            out->hit_pos_t[4 * i + 0] = a[i].x; out->hit_pos_t[4 * i + 1] = a[i].y;
            out->hit_pos_t[4 * i + 2] = a[i].z; out->hit_pos_t[4 * i + 3] = a[i].w;
            int m;
            memcpy(&m, &b[i].w, 4);
            out->hit_nrm_mat[4 * i + 0] = b[i].x; out->hit_nrm_mat[4 * i + 1] = b[i].y;
            out->hit_nrm_mat[4 * i + 2] = b[i].z; out->hit_nrm_mat[4 * i + 3] = (float)m;
            if (out->hit_tri) out->hit_tri[i] = t[i];
        }
    } else {
        HIPCHK(c, hipMemcpy(out->visible, vis, n, hipMemcpyDeviceToHost));
    }
    return MCPT_OK;
}

int mcpt_debug_queue_rays(mcpt_ctx* c, int which, float* ro, float* rd, uint32_t* n_inout) {
    if (!c || !c->film.allocated || !n_inout || (which != 0 && which != 1)) return set_err(c, MCPT_E_INVALID, "bad argument");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    CounterBlock cb;
    HIPCHK(c, hipMemcpy(&cb, c->cnt.dev, sizeof(cb), hipMemcpyDeviceToHost));
    // k_accumulate reset the live counters; the queues still hold the last iteration's entries
    uint32_t n = which == 0 ? cb.last_ext : 0;
    if (which == 1) return set_err(c, MCPT_E_INVALID, "any-hit queue length is not retained");
    if (!ro || !rd) { *n_inout = n; return MCPT_OK; }
    n = std::min(n, *n_inout);
    std::vector<uint32_t> all((size_t)kShards * c->queues.ext_cap), q;
    HIPCHK(c, hipMemcpy(all.data(), c->queues.ext, all.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (int sh = 0; sh < kShards; sh++)
        for (uint32_t k = 0; k < cb.last_ext_shard[sh] && q.size() < n; k++) q.push_back(all[(size_t)sh * c->queues.ext_cap + k]);
    n = (uint32_t)q.size();
    const size_t np = c->film.L.paths;
    std::vector<float4> o(np), d(np);
    HIPCHK(c, hipMemcpy(o.data(), c->film.ray_o, np * sizeof(float4), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(d.data(), c->film.ray_d, np * sizeof(float4), hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < n; i++) {
        float4 a = o[q[i]], b = d[q[i]];
        ro[3 * i] = a.x; ro[3 * i + 1] = a.y; ro[3 * i + 2] = a.z;
        rd[3 * i] = b.x; rd[3 * i + 1] = b.y; rd[3 * i + 2] = b.z;
    }
    *n_inout = n;
    return MCPT_OK;
}
float mcpt_debug_last_stage_ms(const mcpt_ctx* c) { return c ? c->last_stage_ms : -1.f; }
int mcpt_debug_tiny_lds_stack(mcpt_ctx* c, int32_t on) {
    if (!c) return MCPT_E_INVALID;
    c->tiny_stack = on != 0;
    return MCPT_OK;
}

int mcpt_debug_quot(mcpt_ctx* c, const float* a, const float* b, uint32_t n, float* out) {
    if (!c || (n && (!a || !b || !out))) return set_err(c, MCPT_E_INVALID, "null argument");
    HIPCHK(c, hipSetDevice(c->device));
    float* d = nullptr;
    if (n == 0) return MCPT_OK;
    if (hipMalloc(&d, (size_t)3 * n * sizeof(float)) != hipSuccess) return set_err(c, MCPT_E_NOMEM, "quot buffers");
    int rc = MCPT_OK;
    if (hipMemcpyAsync(d, a, n * sizeof(float), hipMemcpyHostToDevice, c->stream) != hipSuccess ||
        hipMemcpyAsync(d + n, b, n * sizeof(float), hipMemcpyHostToDevice, c->stream) != hipSuccess)
        rc = set_err(c, MCPT_E_HIP, "copy");
    if (!rc) {
        launch_quot(d, d + n, d + 2 * (size_t)n, n, c->stream);
        if (hipGetLastError() != hipSuccess ||
            hipMemcpyAsync(out, d + 2 * (size_t)n, n * sizeof(float), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
            hipStreamSynchronize(c->stream) != hipSuccess)
            rc = set_err(c, MCPT_E_HIP, "quot kernel");
    }
    (void)hipFree(d);
    return rc;
}

int mcpt_debug_hbm_copy(mcpt_ctx* c, uint64_t bytes, uint32_t iters, double* gbps) {
    if (!c || !gbps || bytes < 4096 || iters == 0) return set_err(c, MCPT_E_INVALID, "bad argument");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n = (size_t)(bytes / sizeof(float4));
    float4* d = nullptr;
    if (hipMalloc(&d, 2 * n * sizeof(float4)) != hipSuccess) return set_err(c, MCPT_E_NOMEM, "copy buffers");
    hipEvent_t e0 = nullptr, e1 = nullptr;
    int rc = MCPT_OK;
    if (hipMemsetAsync(d, 0, 2 * n * sizeof(float4), c->stream) != hipSuccess ||
        hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) {
        rc = set_err(c, MCPT_E_HIP, "copy setup");
    } else {
        launch_copy(d, d + n, n, c->stream);  // warm-up
        (void)hipEventRecord(e0, c->stream);
        for (uint32_t i = 0; i < iters; i++) launch_copy(i & 1 ? d + n : d, i & 1 ? d : d + n, n, c->stream);
        (void)hipEventRecord(e1, c->stream);
        float ms = 0.f;
        if (hipGetLastError() != hipSuccess || hipEventSynchronize(e1) != hipSuccess ||
            hipEventElapsedTime(&ms, e0, e1) != hipSuccess || ms <= 0.f)
            rc = set_err(c, MCPT_E_HIP, "copy kernel");
        else
            *gbps = 2.0 * (double)n * sizeof(float4) * iters / (ms * 1e-3) / 1e9;  // read + write bytes
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    (void)hipFree(d);
    return rc;
}

// k_trace's loop-phase counts (PH_*, counting build: mcpt_set_work_counters on) since the last film
// clear or reset, from the host copy of the counters the last call left: returns kPhaseWords
int mcpt_debug_trace_profile(mcpt_ctx* c, uint64_t* out12, int reset) {
    if (!c || !out12) return MCPT_E_INVALID;
    for (int i = 0; i < 12; i++) out12[i] = 0;
    if (!c->cnt.totals_ok) return 0;
    for (int i = 0; i < kPhaseWords; i++) out12[i] = c->cnt.totals.tot_phase[i] - c->cnt.phase_base[i];
    if (reset)
        for (int i = 0; i < kPhaseWords; i++) c->cnt.phase_base[i] = c->cnt.totals.tot_phase[i];
    return kPhaseWords;
}
// Not part of mcpt.h: entry / exit s_memrealtime (100 MHz) stamps of the last k_trace launch's first n
// waves (out: 4n words: entry, exit, partition, time the partition ran dry); returns n or 0.
// The round-2/3 diagnostics builds (per-section wave clocks of k_shade / k_material, k_trace loop
// profiles, wave lifetimes, per-ray step counts) are gone from the kernels (they are in git
// history); rocprofv3 counter passes (tools/gpu/run.sh pmc) replace them.  The ABI entry stays
// and reports that nothing was collected.
int mcpt_debug_wave_times(mcpt_ctx* c, uint64_t* out, int n) {
    if (!c || !out || n < 0) return MCPT_E_INVALID;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}
// Diagnostics builds (-DMCPT_DIAG_SHADE) only, not part of mcpt.h: k_shade's per-section wave entries
// and active lanes (SD_* pairs, kernels.hip) summed since the last reset; returns the word count or 0.
int mcpt_debug_shade_sections(mcpt_ctx* c, uint64_t* out, int n, int reset) {
    if (!c || !out || n < 0) return MCPT_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return shade_sections(reinterpret_cast<unsigned long long*>(out), n, reset);
}

}  // extern "C"
