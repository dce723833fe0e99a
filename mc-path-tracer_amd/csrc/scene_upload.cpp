// scene_upload.cpp -- the device half of a scene upload behind the mcpt_* C ABI (include/mcpt.h), and
// the geometry update that runs its geometry-dependent steps again.  Replaces the reference's
// Scene::transfer_data_to_device (Scene.cu:363-470).  The host half -- validation, the pair tree,
// the records -- is host/pair_tree.cpp; all the state is the context's SceneState.
#include "host/pair_tree.hpp"
#include "runtime_internal.hpp"

using mcpt_host::PairTree;

// The context's events as this file uses them.  A pair is reused once its elapsed time is read: the
// tree build, the HRDI table build and the complete keys share the first, the occluder records and
// the pre-fill probes the second; a geometry update's phases stand across those.
enum SceneEvent : size_t { EV_A0, EV_A1, EV_B0, EV_B1, EV_UPD_START, EV_UPD_REC, EV_UPD_TREE, EV_UPD_QUAD, EV_UPD_END };

// The upload-time environment knobs, read once per upload; an update takes them from the context.
static void read_upload_env(UploadKnobs& g) {
    auto is0 = [](const char* e) { return e && e[0] == '0' && e[1] == 0; };
    g = UploadKnobs{};
    g.cull_off = is0(getenv("MCPT_CULL"));  // 0: no culling at all (A/B, and a reference-order traversal)
    // MCPT_CULL_PLANE=0: the general bound for axis-plane triangles too (A/B; the host
    // builder's isolation of unbounded triangles reads the same variable)
    g.plane = !is0(getenv("MCPT_CULL_PLANE"));
    if (const char* we = getenv("MCPT_BVH_WIDTH"))
        if ((we[0] == '2' || we[0] == '4') && we[1] == 0) g.width = we[0] - '0';
    // MCPT_SIBLING_LAYOUT=0/1/2/3 forces a pair numbering (host/pair_tree.cpp; other values are ignored)
    if (const char* sl = getenv("MCPT_SIBLING_LAYOUT"))
        if (sl[0] >= '0' && sl[0] <= '3' && sl[1] == 0) g.layout = sl[0] - '0';
    if (const char* e = getenv("MCPT_OCC_G")) g.occ_g = atoi(e);
    if (const char* e = getenv("MCPT_OCC_B")) g.occ_b = atoi(e);
    g.occ_complete = !is0(getenv(kOccCompleteEnv));
    g.occ_prefill = !is0(getenv("MCPT_OCC_PREFILL"));
    if (const char* e = getenv("MCPT_ENV_GUIDES")) g.env_guides = e[0] != '0';  // 0: plain bisection (A/B, tests)
}

// The device build of the pair tree over the desc-order records li.d_tri / li.d_sh: the context's
// builder, its arrays into the scene's list, build_ms, pair_depth.
static int gpu_tree_build(mcpt_ctx* c, const LbvhInput& li, LbvhOutput& lb) {
    SceneState& sc = c->scene;
    HIPCHK(c, hipEventRecord(ev(c, EV_A0), c->stream));
    const int brc = c->gpu_bvh_builder == MCPT_GPU_BVH_LBVH ? build_lbvh(li, lb, c->stream) : build_ploc(li, lb, c->stream);
    for (void* q : {(void*)lb.nodes, (void*)lb.tri, (void*)lb.tri_sh, (void*)lb.order})
        if (q) sc.bufs.push_back(q);
    if (brc) return set_err(c, MCPT_E_HIP, "GPU BVH build failed (" + std::to_string(brc) + ")");
    HIPCHK(c, hipEventRecord(ev(c, EV_A1), c->stream));
    HIPCHK(c, hipEventSynchronize(ev(c, EV_A1)));
    HIPCHK(c, hipEventElapsedTime(&sc.build_ms, ev(c, EV_A0), ev(c, EV_A1)));
    if (lb.depth > kMaxStack) return set_err(c, MCPT_E_INVALID, "GPU BVH deeper than the 64-entry traversal stack");
    sc.pair_depth = lb.depth;
    sc.bvh_nodes = lb.nodes;
    sc.order = lb.order;
    return MCPT_OK;
}

// Culling margins of the pair tree dn (launch_cull_margins), the far coefficient P and the root's margin
static int pair_margins(mcpt_ctx* c, float4* dn, uint32_t npairs, int proot, const float4* dt, int32_t ntri,
                        float* cull_p, float* root_w) {
    int rc;
    float* tw = nullptr;
    uint32_t* pm = nullptr;
    TmpScope tmp(c);
    if ((rc = dalloc(c, tmp.L, &tw, (size_t)ntri)) || (rc = dalloc(c, tmp.L, &pm, 1))) return rc;
    HIPCHK(c, hipMemsetAsync(pm, 0, sizeof(uint32_t), c->stream));
    mcpt_dev::launch_cull_margins(dn, npairs, dt, (uint32_t)ntri, tw, pm, c->scene.pair_depth + 2, c->scene.knobs.plane, c->stream);
    HIPCHK(c, hipGetLastError());
    uint32_t pb = 0;
    HIPCHK(c, hipMemcpyAsync(&pb, pm, sizeof(pb), hipMemcpyDeviceToHost, c->stream));
    float4 rq = make_float4(0.f, 0.f, 0.f, 0.f);
    std::vector<float> leaf_w;
    if (proot >= 0 && npairs > 0) {
        HIPCHK(c, hipMemcpyAsync(&rq, dn + 4 * (size_t)proot + 3, sizeof(rq), hipMemcpyDeviceToHost, c->stream));
    } else if (proot < 0) {  // the whole tree is one leaf
        const uint32_t off = (uint32_t)proot & 0xffffffu, cnt = (((uint32_t)proot >> 24) & 7u) + 1u;
        leaf_w.resize(cnt);
        HIPCHK(c, hipMemcpyAsync(leaf_w.data(), tw + off, cnt * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    memcpy(cull_p, &pb, 4);
    *root_w = proot >= 0 ? std::fmax(rq.z, rq.w) : 0.f;
    for (float w : leaf_w) *root_w = std::fmax(*root_w, w);
    return MCPT_OK;
}

// Node width of a tree of tree_pairs pair nodes: 4-wide nodes (one 128-B line tests four boxes, half
// the levels) for trees of more than 32 MB of pair nodes, child pairs otherwise.  Per launch,
// interleaved on one box: config 5 (2 M tris, 128 MB) 16.7 -> 15.6 ms and config 3 (871K, 55 MB)
// 1.154 -> 1.148 ms with quads; config 4 (252K, 16 MB) 7.69 -> 7.79 ms and config 2 (4.8K) 0.783 ->
// 0.848 ms, so those keep pairs.  MCPT_BVH_WIDTH=2/4 forces a width.
static int node_width(const mcpt_ctx* c, size_t tree_pairs) {
    return c->scene.knobs.width ? c->scene.knobs.width : tree_pairs * 64 > ((size_t)32 << 20) ? 4 : 2;
}

// 4-wide traversal: collapse the pair tree on the device (host SAH or GPU-built, with the margins
// launch_cull_margins wrote) into 4-wide nodes; s.nodes, the slot source map for later refits.
static int quads_upload(mcpt_ctx* c, const float4* d_pairs, size_t npairs, int proot, DevScene& s, uint32_t& nnodes,
                        int& quad_root, int& quad_push) {
    SceneState& sc = c->scene;
    std::vector<float4> pairs(npairs * 4);
    if (npairs) HIPCHK(c, hipMemcpy(pairs.data(), d_pairs, pairs.size() * sizeof(float4), hipMemcpyDeviceToHost));
    std::vector<float4> quads;
    std::vector<uint32_t> src;
    int max_push = 0, rc;
    mcpt_host::pairs_to_quads(pairs, proot, quads, quad_root, max_push, src);
    if (max_push > kMaxStack) return set_err(c, MCPT_E_INVALID, "4-wide BVH needs more than 64 stack entries");
    quad_push = max_push;
    if ((rc = dupload(c, sc.bufs, &sc.quads, quads.data(), quads.size()))) return rc;
    if ((rc = dupload(c, sc.bufs, &sc.quad_src, src.data(), src.size()))) return rc;
    s.nodes = sc.quads;
    nnodes = sc.nquads = (uint32_t)(quads.size() / 8);
    return MCPT_OK;
}

// What every adopted pair tree gets, host- or device-built: it becomes the scene's tree, with its
// margins, P and the root's margin, the node width, the 4-wide collapse, the root ref and the depth.
// s.tri, s.ntri and the root box are set; sc.pair_depth and sc.cull_ok are the tree's.  nnodes: the
// nodes of the uploaded width (the leaf-box pass).  after_margins (or nullptr): recorded between the
// margins and the collapse.
static int tree_finish(mcpt_ctx* c, DevScene& s, float4* nodes, uint32_t npairs, int proot, uint32_t& nnodes,
                       hipEvent_t after_margins) {
    SceneState& sc = c->scene;
    int rc;
    sc.pair_nodes = npairs ? nodes : nullptr;
    sc.pair_count = npairs;
    sc.pair_root = proot;
    s.nodes = nodes;
    s.cull_p = 0.f;
    s.root_w = __builtin_huge_valf();
    if (s.ntri > 0 && (rc = pair_margins(c, nodes, npairs, proot, s.tri, (int32_t)s.ntri, &s.cull_p, &s.root_w))) return rc;
    if (after_margins) HIPCHK(c, hipEventRecord(after_margins, c->stream));
    nnodes = npairs;
    s.width = node_width(c, npairs);
    int quad_root = 0, quad_push = 0;
    if (s.width == 4 && s.ntri > 0 && (rc = quads_upload(c, nodes, npairs, proot, s, nnodes, quad_root, quad_push))) return rc;
    s.root_ref = s.width == 4 ? (proot < 0 ? proot : quad_root) : proot;
    s.depth = s.width == 4 ? quad_push : sc.pair_depth;
    s.cull_ok = sc.cull_ok ? 1 : 0;
    return MCPT_OK;
}

// The host-built tree of an upload (an empty one for a scene without triangles)
static int adopt_host_tree(mcpt_ctx* c, const mcpt_scene_desc& d, const PairTree& pt, DevScene& s, uint32_t& nnodes) {
    SceneState& sc = c->scene;
    int rc;
    float4* dn;
    if ((rc = dupload(c, sc.bufs, &dn, pt.pairs.data(), pt.pairs.size()))) return rc;
    sc.pair_depth = pt.depth;
    sc.node_layout = pt.layout;
    sc.cull_ok = pt.contained && !sc.knobs.cull_off;
    sc.nest_ok = pt.nested;
    for (int k = 0; k < 3; k++) {  // (no triangles: a root box that no ray can enter)
        s.root_mn[k] = d.ntri > 0 ? d.bmin[k] : 1.f;
        s.root_mx[k] = d.ntri > 0 ? d.bmax[k] : -1.f;
    }
    return tree_finish(c, s, dn, (uint32_t)(pt.pairs.size() / 4), pt.root_ref, nnodes, nullptr);
}

// A tree built on the device over the desc-order records sc.desc_tri / sc.desc_sh (li), by an upload
// and by MCPT_GEOM_REBUILD alike: the builder's permuted records become s.tri / s.tri_sh.  Its boxes
// contain their triangles and nest by construction.
static int adopt_device_tree(mcpt_ctx* c, const LbvhInput& li, DevScene& s, uint32_t& nnodes, hipEvent_t after_margins) {
    SceneState& sc = c->scene;
    int rc;
    LbvhOutput lb;
    if ((rc = gpu_tree_build(c, li, lb))) return rc;
    sc.pair_gpu_built = true;
    sc.ploc_rounds = c->gpu_bvh_builder == MCPT_GPU_BVH_PLOC ? lb.rounds : 0;
    sc.cull_ok = !sc.knobs.cull_off;
    sc.nest_ok = true;
    s.tri = lb.tri;
    s.tri_sh = lb.tri_sh;
    for (int k = 0; k < 3; k++) { s.root_mn[k] = lb.root_mn[k]; s.root_mx[k] = lb.root_mx[k]; }
    return tree_finish(c, s, lb.nodes, (uint32_t)lb.nnodes, lb.root_ref, nnodes, after_margins);
}

// The leaf-box record of every triangle (they serve the occluder cache and the primary-hit table alike:
// either switch alone keeps them; for the table alone they are best-effort) and the occluder table of
// G cells per axis and B bins per face coordinate, with its cell sizes from the root box and the
// complete keys' direction-bin table.  Arrays the context already holds are reused.
static int occ_arrays(mcpt_ctx* c, DevScene& s, uint32_t nnodes, float* ms) {
    SceneState& sc = c->scene;
    int rc;
    uint32_t* const occ_have = sc.dev.occ;  // the table of the scene this one replaces in place (an update)
    // 24^3 cells x 6 x 12^2 bins x 2 ways = 96 MB.  Config 2 with the table emptied at every film
    // clear: 62 % of the any-hit rays resolved (16^3 x 8^2: 60 %, 32^3 x 16^2: 64 %; frame rates
    // within 1 %: the bigger tables resolve more but warm up more slowly and miss L2 more)
    const int G = sc.knobs.occ_g, B = sc.knobs.occ_b;
    // the index G^3 * 6 * B^2 must fit 32 bits
    // (off unless every box nests in its parent's: occ_test relies on it, see SceneState::nest_ok)
    const bool occ_want = G > 0 && G <= 64 && B > 0 && B <= 64 && (uint64_t)G * G * G * 6 * B * B <= 0xffffffffull;
    float4* lbx = sc.occ_rec;
    if (!lbx && s.ntri > 0 && sc.nest_ok && (occ_want || c->prim.on)) {
        void* q = nullptr;
        if (hipMalloc(&q, kOccRecF4 * (size_t)s.ntri * sizeof(float4)) == hipSuccess) {
            sc.bufs.push_back(q);
            lbx = (float4*)q;
        } else {
            (void)hipGetLastError();
            if (occ_want) return set_err(c, MCPT_E_NOMEM, "hipMalloc: occluder records");
        }
    }
    sc.occ_rec = lbx;
    if (lbx && !(s.ntri > 0 && sc.nest_ok)) lbx = nullptr;
    if (lbx) {
        // NaN boxes (all-ones bytes) for a record no leaf holds: occ_test's slab then fails
        HIPCHK(c, hipEventRecord(ev(c, EV_B0), c->stream));
        HIPCHK(c, hipMemsetAsync(lbx, 0xff, kOccRecF4 * (size_t)s.ntri * sizeof(float4), c->stream));
        launch_occ_records(s, nnodes, lbx, c->stream);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipEventRecord(ev(c, EV_B1), c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (ms) HIPCHK(c, hipEventElapsedTime(&ms[0], ev(c, EV_B0), ev(c, EV_B1)));
        s.occ_rec = lbx;
    }
    if (!(occ_want && lbx)) return MCPT_OK;
    uint32_t* occ = occ_have;
    const size_t ne = occ_entries(G, B);
    if (!occ && (rc = dalloc(c, sc.bufs, &occ, ne + kOccGateWords))) return rc;
    HIPCHK(c, hipMemsetAsync(occ, 0xff, ne * sizeof(uint32_t), c->stream));
    HIPCHK(c, hipMemsetAsync(occ + ne, 0, kOccGateWords * sizeof(uint32_t), c->stream));  // the lookup gate: on
    HIPCHK(c, hipStreamSynchronize(c->stream));
    s.occ = occ;
    s.occ_gate = occ + ne;
    sc.occ_entries_n = ne;
    s.occ_g = G;
    s.occ_b = B;
    for (int k = 0; k < 3; k++) {
        const float ext = s.root_mx[k] - s.root_mn[k];
        s.occ_inv[k] = ext > 0.f && ext < 3.4e38f ? (float)G / ext : 0.f;
        s.occ_cell[k] = s.occ_inv[k] > 0.f ? ext / (float)G : 0.f;
    }
    // Complete keys (device/occ_beam.hpp): the direction-bin table of the keys' beams.  They
    // need the culling bound (a resolved ray's culling scale is positive) and a root box with
    // an extent on every axis, and at most 32 cells per axis (k_material's packed key coordinates).
    // MCPT_OCC_COMPLETE=0: none (A/B runs, tests).
    if (sc.knobs.occ_complete && s.cull_ok && G <= 32 && s.occ_cell[0] > 0.f && s.occ_cell[1] > 0.f && s.occ_cell[2] > 0.f) {
        if (!sc.occ_dir) {
            std::vector<float4> dirs((size_t)6 * B * B * mcpt::kOccDirF4);
            mcpt::occ_dir_table(B, dirs.data());
            if ((rc = dupload(c, sc.bufs, &sc.occ_dir, dirs.data(), dirs.size()))) return rc;
        }
        s.occ_dir = sc.occ_dir;
    }
    return MCPT_OK;
}

// The occluder table's scene-derived content: the pre-fill probes, the complete keys, the occ_init
// snapshot film clears restore and the gate words.  The scratch (three arrays of a key each for the
// probes, a counter for the complete keys) lives until the end, as the snapshot's copy may still run.
static int occ_fill(mcpt_ctx* c, DevScene& s, float* ms) {
    SceneState& sc = c->scene;
    int rc;
    // Occluder-table pre-fill: one any-hit probe ray per table key (origin cell centre, direction
    // bin centre; k_occ_probes) traced with occluder recording on, so every key whose probe is
    // occluded starts with a triangle -- derived from the scene alone, like the BVH.  Film
    // clears restore this table, so every frame starts from the same one and no frame depends
    // on another.  MCPT_OCC_PREFILL=0: frames start from an empty table.
    const bool prefill = sc.knobs.occ_prefill, complete = s.occ_dir != nullptr;
    const uint32_t nkeys = (uint32_t)(sc.occ_entries_n / kOccWays);
    if (!prefill && !complete) return MCPT_OK;
    if (!sc.occ_init && (rc = dalloc(c, sc.bufs, &sc.occ_init, sc.occ_entries_n))) return rc;
    TmpScope tmp(c);
    if (prefill) {
        float4 *pro, *prd;
        uint8_t* pvis;
        if ((rc = dalloc(c, tmp.L, &pro, nkeys)) || (rc = dalloc(c, tmp.L, &prd, nkeys)) || (rc = dalloc(c, tmp.L, &pvis, nkeys)))
            return rc;
        HIPCHK(c, hipEventRecord(ev(c, EV_B0), c->stream));
        launch_occ_probes(s, pro, prd, nkeys, c->stream);
        TraceArgs ta{};
        ta.scene = s;  // occ on, gate words 0: the finish records the occluder of every occluded probe
        ta.nshards = 1;
        TraceSet& ts = ta.set[1];
        ts.ro = pro;
        ts.rd = prd;
        ts.count = nkeys;
        ts.shard_cap = nkeys;
        ta.vis = pvis;
        ta.grab = &c->cnt.dev->grab[0][0];
        launch_trace(ta, c->geom, c->stream);
        HIPCHK(c, hipMemsetAsync(c->cnt.dev->grab, 0, sizeof(c->cnt.dev->grab), c->stream));  // hand-out counters back to 0
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipEventRecord(ev(c, EV_B1), c->stream));
        if (ms) {
            HIPCHK(c, hipEventSynchronize(ev(c, EV_B1)));
            HIPCHK(c, hipEventElapsedTime(&ms[1], ev(c, EV_B0), ev(c, EV_B1)));
        }
    }
    if (complete) {
        // Complete keys, over the pre-fill: the candidate lists of the keys that have at most
        // kOccWays candidates, from the child-pair tree (kept on the device for either node width:
        // the 4-wide nodes' boxes and margins are copies of its entries).  Like the pre-fill a
        // property of the scene alone; the snapshot below carries them into every frame.
        mcpt::OccTree tr{};
        tr.nodes = sc.pair_nodes;
        tr.tri = s.tri;
        tr.tri_f4 = kTriF4;
        tr.ntri = s.ntri;
        tr.root_ref = sc.pair_root;
        for (int k = 0; k < 3; k++) { tr.root_mn[k] = s.root_mn[k]; tr.root_mx[k] = s.root_mx[k]; }
        tr.root_w = s.root_w;
        tr.cull_p = s.cull_p;
        uint32_t* dn;
        if ((rc = dalloc(c, tmp.L, &dn, 1))) return rc;
        HIPCHK(c, hipMemsetAsync(dn, 0, sizeof(uint32_t), c->stream));
        HIPCHK(c, hipEventRecord(ev(c, EV_A0), c->stream));
        launch_occ_complete(s, tr, nkeys, dn, c->stream);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipEventRecord(ev(c, EV_A1), c->stream));
        uint32_t nd = 0;
        HIPCHK(c, hipMemcpyAsync(&nd, dn, sizeof(nd), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipEventSynchronize(ev(c, EV_A1)));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipEventElapsedTime(&sc.occ_done_ms, ev(c, EV_A0), ev(c, EV_A1)));
        sc.occ_done_keys = nd;
        if (ms) ms[2] = sc.occ_done_ms;
    }
    HIPCHK(c, hipMemcpyAsync(sc.occ_init, s.occ, sc.occ_entries_n * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
    const uint32_t warm[kOccGateWords] = {0u, 0u, 1u};  // the table holds occluders: lookups from the start
    HIPCHK(c, hipMemcpyAsync(s.occ_gate, warm, sizeof(warm), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MCPT_OK;
}

// Any-hit occluder cache (kernels.hip occ_hit1) and everything else that follows from the finished
// tree of s.  Run by an upload and by a geometry update alike (an upload starts without any array).
// MCPT_OCC_G=0 turns the cache off; MCPT_OCC_G / MCPT_OCC_B set the cells per axis / bins per face
// coordinate.  ms (or nullptr): device ms of the leaf-box records, the pre-fill probes and the
// complete keys.
static int occ_state(mcpt_ctx* c, DevScene& s, uint32_t nnodes, float* ms) {
    int rc;
    s.occ = nullptr;
    s.occ_gate = nullptr;
    s.occ_rec = nullptr;
    s.occ_dir = nullptr;
    for (int k = 0; k < 3; k++) s.occ_cell[k] = 0.f;
    c->scene.occ_done_keys = 0;
    c->scene.occ_done_ms = 0.f;
    if (ms) ms[0] = ms[1] = ms[2] = 0.f;
    if ((rc = occ_arrays(c, s, nnodes, ms))) return rc;
    return s.occ ? occ_fill(c, s, ms) : MCPT_OK;
}

// The records (pack_records' tri and sh), materials and lights of a desc
static int records_upload(mcpt_ctx* c, const mcpt_scene_desc& d, const std::vector<float4>& tri, const std::vector<float4>& sh,
                          DevScene& s) {
    SceneState& sc = c->scene;
    int rc;
    float4 *dt, *dsh;
    float *dm, *dd;
    if ((rc = dupload(c, sc.bufs, &dt, tri.data(), tri.size()))) return rc;
    if ((rc = dupload(c, sc.bufs, &dsh, sh.data(), sh.size()))) return rc;
    if ((rc = dupload(c, sc.bufs, &dm, d.mat_params, (size_t)d.nmat * 8))) return rc;
    if ((rc = dupload(c, sc.bufs, &dd, d.dir_params, (size_t)d.ndir * 7))) return rc;
    s.tri = dt; s.tri_sh = dsh; s.mats = dm; s.dirs = dd;
    s.ntri = (uint32_t)d.ntri;
    s.nlights = 1 + d.ndir;
    return MCPT_OK;
}

// Search guides for env_cell, on the device for either source of tables: valid on a sorted, NaN-free
// marginal CDF and conditional rows that are sorted and NaN-free or NaN throughout (upper_bound
// returns 0 on such a row for every value, and so does the guided search with its all-zero guide).
// Every HRDI map has one: row 0's sin(0) = 0 makes it 0 / (denom * 0)
// (light_initialization_kernels.cu:72).  Otherwise the plain bisection is used.
static int env_guides(mcpt_ctx* c, mcpt::EnvView& env) {
    SceneState& sc = c->scene;
    const int W = env.w, H = env.h;
    int rc;
    if (W > 65535 || H > 65535) return MCPT_OK;
    const size_t G1 = mcpt::kEnvGuide + 1;
    uint16_t *dgm, *dgc;
    uint32_t* dbad;
    if ((rc = dalloc(c, sc.bufs, &dgm, G1)) || (rc = dalloc(c, sc.bufs, &dgc, (size_t)H * G1)) || (rc = dalloc(c, sc.bufs, &dbad, 1)))
        return rc;
    HIPCHK(c, hipMemsetAsync(dbad, 0, sizeof(uint32_t), c->stream));
    mcpt_dev::launch_env_guides(env.marginal_y, env.conds_y, W, H, dgm, dgc, dbad, c->stream);
    HIPCHK(c, hipGetLastError());
    uint32_t bad = 1;
    HIPCHK(c, hipMemcpyAsync(&bad, dbad, sizeof(bad), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (bad == 0 && sc.knobs.env_guides) {
        env.guide_m = dgm;
        env.guide_c = dgc;
        sc.env_guides = true;
    }
    return MCPT_OK;
}

// The environment light: colour, or the HRDI texture with its sampling tables (given, or built on the
// device from the texture), the search guides and the light-sample tables
static int env_upload(mcpt_ctx* c, const mcpt_scene_desc& d, mcpt::EnvView& env) {
    SceneState& sc = c->scene;
    int rc;
    env.mode = d.env_mode;
    for (int k = 0; k < 3; k++) env.color[k] = d.env_color[k];
    env.ls = d.env_ls;
    env.w = d.env_w;
    env.h = d.env_h;
    if (d.env_mode != 1) return MCPT_OK;
    float4* tx;
    float *my, *cy, *pd;
    const int W = d.env_w, H = d.env_h;
    const size_t WH = (size_t)W * H;
    if ((rc = dupload(c, sc.bufs, &tx, reinterpret_cast<const float4*>(d.env_tex), WH))) return rc;
    sc.env_device_built = !d.env_marginal_y;
    if (!sc.env_device_built) {
        if ((rc = dupload(c, sc.bufs, &my, d.env_marginal_y, (size_t)H))) return rc;
        if ((rc = dupload(c, sc.bufs, &cy, d.env_conds_y, WH))) return rc;
        if ((rc = dupload(c, sc.bufs, &pd, d.env_pdf, WH))) return rc;
    } else {
        // build_environment_light (light_initialization_kernels.cu:134-161) on the device
        if ((rc = dalloc(c, sc.bufs, &my, (size_t)H)) || (rc = dalloc(c, sc.bufs, &cy, WH)) || (rc = dalloc(c, sc.bufs, &pd, WH)))
            return rc;
        float* scratch = nullptr;
        hipError_t e = hipMalloc(&scratch, mcpt_dev::env_build_scratch_floats(W, H) * sizeof(float));
        if (e != hipSuccess) return set_err(c, MCPT_E_NOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
        HIPCHK(c, hipEventRecord(ev(c, EV_A0), c->stream));
        mcpt_dev::launch_env_build(tx, W, H, scratch, my, cy, pd, c->stream);
        HIPCHK(c, hipEventRecord(ev(c, EV_A1), c->stream));
        e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        (void)hipFree(scratch);
        if (e != hipSuccess) return set_err(c, MCPT_E_HIP, std::string("env build: ") + hipGetErrorString(e));
        HIPCHK(c, hipEventElapsedTime(&sc.env_build_ms, ev(c, EV_A0), ev(c, EV_A1)));
    }
    env.tex = tx; env.marginal_y = my; env.conds_y = cy; env.pdf = pd;
    mcpt_dev::launch_env_pack(tx, pd, WH, c->stream);  // before the tables below read env_pdf
    HIPCHK(c, hipGetLastError());
    if ((rc = env_guides(c, env))) return rc;
    // light-sample tables, reference and quality mode (k_env_table)
    if ((size_t)(W + 1) * H < ((size_t)1 << 28)) {
        const size_t ne = (size_t)(W + 1) * H;
        float4 *lt0, *lt1;
        float2 *rc0, *rc1;  // row table (h entries) then column table (w + 1)
        const size_t nrc = (size_t)H + W + 1;
        if ((rc = dalloc(c, sc.bufs, &lt0, ne)) || (rc = dalloc(c, sc.bufs, &lt1, ne)) || (rc = dalloc(c, sc.bufs, &rc0, nrc)) ||
            (rc = dalloc(c, sc.bufs, &rc1, nrc)))
            return rc;
        launch_env_table(env, false, lt0, rc0, rc0 + H, c->stream);
        launch_env_table(env, true, lt1, rc1, rc1 + H, c->stream);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(c->stream));
        env.ltab[0] = lt0;
        env.ltab[1] = lt1;
        env.lrow[0] = rc0;
        env.lrow[1] = rc1;
        env.lcol[0] = rc0 + H;
        env.lcol[1] = rc1 + H;
    }
    return MCPT_OK;
}

// s becomes the context's scene.  The film sees an update as it sees a re-upload.
static void scene_commit(mcpt_ctx* c, const DevScene& s, bool notify_film) {
    c->scene.dev = s;
    c->scene_gen++;    // with the scene itself: the previous scene's primary-hit table and guides are stale
    c->tp.ok = false;  // ... and so is the temporal history (no motion vectors for moved geometry)
    if (notify_film) c->film_stale = true;
    c->scene.ok = true;
}

// Argument checks reject the call and leave the context as it was; from there on the context has no
// scene until the new one stands.
static int scene_upload(mcpt_ctx* c, const mcpt_scene_desc* d, bool gpu_bvh) {
    if (!c || !d) return set_err(c, MCPT_E_INVALID, "null argument");
    std::string err;
    if (!mcpt_host::validate_desc(*d, !gpu_bvh, err)) return set_err(c, MCPT_E_INVALID, err);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    SceneState& sc = c->scene;
    c->has_scene_before = c->has_scene_before || sc.ok;
    sc.reset();
    c->em.drop();  // the emission table belongs to the scene that goes
    c->es.drop_table();  // ... and the emitter table with it (the switch stays; section 17)
    c->es.drop_streams();
    c->tx.drop();  // ... and the texture set: its uvs are the old scene's triangles' (section 19)
    read_upload_env(sc.knobs);
    sc.gpu_upload = gpu_bvh;
    sc.ntri = d->ntri;
    sc.nmat = d->nmat;
    PairTree pt;  // gpu_bvh: the desc's BVH arrays are ignored
    if (!gpu_bvh && !mcpt_host::build_pair_tree(*d, sc.knobs.layout, pt, err)) return set_err(c, MCPT_E_INVALID, err);
    DevScene s{};
    uint32_t nnodes = 0;  // nodes of the uploaded width
    int rc;
    // The packed records live until the upload ends: freeing the two arrays (96 MB each at 2 M triangles)
    // right after their copy put about 1 ms into the device build that follows (build_ms 5.6 -> 6.7 ms).
    std::vector<float4> tri, sh;
    mcpt_host::pack_records(*d, tri, sh);
    if ((rc = records_upload(c, *d, tri, sh, s))) return rc;
    if (gpu_bvh && d->ntri > 0) {
        sc.desc_tri = const_cast<float4*>(s.tri);  // the builders' input: kept for mcpt_scene_update_geometry's rebuild
        sc.desc_sh = const_cast<float4*>(s.tri_sh);
        rc = adopt_device_tree(c, LbvhInput{d->ntri, d->v0, d->v1, d->v2, sc.desc_tri, sc.desc_sh}, s, nnodes, nullptr);
    } else {
        rc = adopt_host_tree(c, *d, pt, s, nnodes);
    }
    if (rc || (rc = env_upload(c, *d, s.env)) || (rc = occ_state(c, s, nnodes, nullptr))) return rc;
    scene_commit(c, s, c->has_scene_before);  // a re-upload notifies the film
    return MCPT_OK;
}

// ---- geometry update ----
// New vertex positions (and optionally normals) for the uploaded scene's triangles, in the order of
// the desc's arrays: the records are rewritten in place and the tree is refitted (topology kept) or,
// for a device-built scene, built again; then exactly the state that depends on geometry is derived
// again -- margins, P, the root box, the 4-wide nodes' boxes, the occluder state -- and nothing else:
// materials, lights, the environment and its tables, ids and the occluder grid's size stay.
static int geometry_check(mcpt_ctx* c, int32_t ntri, const void* v0, const void* v1, const void* v2, const void* n0,
                          const void* n1, const void* n2, int32_t mode) {
    if (!c) return set_err(c, MCPT_E_INVALID, "null context");
    if (!c->scene.ok) return set_err(c, MCPT_E_INVALID, "no scene uploaded");
    if (ntri != c->scene.ntri) return set_err(c, MCPT_E_INVALID, "ntri differs from the uploaded scene's (topology changes need an upload)");
    const int given = !!n0 + !!n1 + !!n2;
    if (given != 0 && given != 3) return set_err(c, MCPT_E_INVALID, "normals: all three arrays or none");
    if (mode != MCPT_GEOM_REFIT && mode != MCPT_GEOM_REBUILD) return set_err(c, MCPT_E_INVALID, "unknown geometry update mode");
    if (mode == MCPT_GEOM_REBUILD && !c->scene.gpu_upload)
        return set_err(c, MCPT_E_INVALID, "MCPT_GEOM_REBUILD needs a scene uploaded by mcpt_scene_upload_gpu_bvh");
    if (ntri > 0 && (!v0 || !v1 || !v2)) return set_err(c, MCPT_E_INVALID, "null vertex array");
    return MCPT_OK;
}

// MCPT_GEOM_REFIT: the records of s in place, the pair tree's boxes and margins bottom-up, the 4-wide
// nodes' copies of them
static int geometry_refit(mcpt_ctx* c, DevScene& s, uint32_t n, const float* v0, const float* v1, const float* v2,
                          const float* n0, const float* n1, const float* n2, uint32_t& nnodes) {
    SceneState& g = c->scene;
    float4* pairs = const_cast<float4*>(g.pair_nodes);
    launch_geom_records(GeomRecordsArgs{n, g.order, v0, v1, v2, n0, n1, n2, const_cast<float4*>(s.tri),
                                        const_cast<float4*>(s.tri_sh), g.box},
                        c->stream);
    // New normals also go into the desc-order records a later rebuild permutes from: a rebuild
    // without normals keeps the current ones, not the upload's.  (Positions need no such copy: a
    // rebuild always rewrites them.)
    if (n0 && g.desc_tri && g.desc_sh)
        launch_geom_records(GeomRecordsArgs{n, nullptr, v0, v1, v2, n0, n1, n2, g.desc_tri, g.desc_sh, nullptr}, c->stream);
    HIPCHK(c, hipEventRecord(ev(c, EV_UPD_REC), c->stream));
    HIPCHK(c, hipMemsetAsync(g.out, 0, 8 * sizeof(float), c->stream));
    launch_cull_tri(s.tri, n, g.tri_w, reinterpret_cast<uint32_t*>(g.out.get() + 7), g.knobs.plane, c->stream);
    launch_refit(pairs, g.pair_count, g.pair_root, g.pair_depth + 2, g.box, g.tri_w, n, g.out, c->stream);
    float out[8] = {};
    HIPCHK(c, hipMemcpyAsync(out, g.out, sizeof(out), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipEventRecord(ev(c, EV_UPD_TREE), c->stream));
    // the 4-wide nodes' boxes and margins are copies of the pair tree's: gather them again
    if (s.width == 4 && g.quads && g.nquads) launch_quad_regather(g.quads, g.nquads, g.quad_src, pairs, g.pair_count, c->stream);
    HIPCHK(c, hipEventRecord(ev(c, EV_UPD_QUAD), c->stream));
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int k = 0; k < 3; k++) { s.root_mn[k] = out[k]; s.root_mx[k] = out[3 + k]; }
    s.root_w = out[6];
    memcpy(&s.cull_p, &out[7], 4);
    // the refitted boxes contain their triangles and nest, whatever the uploaded ones did
    g.cull_ok = !g.knobs.cull_off;
    g.nest_ok = true;
    s.cull_ok = g.cull_ok ? 1 : 0;
    nnodes = s.width == 4 ? g.nquads : g.pair_count;
    return MCPT_OK;
}

// MCPT_GEOM_REBUILD: the desc-order records rewritten, the old tree freed, a new one built and adopted
static int geometry_rebuild(mcpt_ctx* c, DevScene& s, int32_t ntri, const float* v0, const float* v1, const float* v2,
                            const float* n0, const float* n1, const float* n2, uint32_t& nnodes) {
    SceneState& g = c->scene;
    launch_geom_records(GeomRecordsArgs{(uint32_t)ntri, nullptr, v0, v1, v2, n0, n1, n2, g.desc_tri, g.desc_sh, nullptr}, c->stream);
    HIPCHK(c, hipEventRecord(ev(c, EV_UPD_REC), c->stream));
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    // the old tree goes
    c->tx.dev_ok = false;  // (the uv stream belongs to the old record order: textures_reorder, after the commit)
    g.release(g.bvh_nodes), g.release(s.tri), g.release(s.tri_sh), g.release(g.order), g.release(g.quads), g.release(g.quad_src);
    g.nquads = 0;
    g.pair_nodes = nullptr;
    g.pair_count = 0;
    int rc = adopt_device_tree(c, LbvhInput{ntri, v0, v1, v2, g.desc_tri, g.desc_sh, true}, s, nnodes, ev(c, EV_UPD_TREE));
    if (rc) return rc;
    HIPCHK(c, hipEventRecord(ev(c, EV_UPD_QUAD), c->stream));
    return MCPT_OK;
}

// The arguments are checked, the arrays on the device and complete.
static int geometry_update_device(mcpt_ctx* c, int32_t ntri, const float* v0, const float* v1, const float* v2,
                                  const float* n0, const float* n1, const float* n2, int32_t mode) {
    if (ntri == 0) return MCPT_OK;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    SceneState& g = c->scene;
    const uint32_t n = (uint32_t)ntri;
    int rc;
    DevScene s = g.dev;
    float* ms = g.update_ms;
    for (int k = 0; k < 8; k++) ms[k] = 0.f;
    if (!g.out.ensure(8) || (mode == MCPT_GEOM_REFIT && (!g.box.ensure(2 * (size_t)n) || !g.tri_w.ensure(n))))
        return set_err(c, MCPT_E_NOMEM, "hipMalloc: geometry update");  // (nothing is rewritten yet)
    uint32_t nnodes = 0;
    // From here the scene is rewritten in place: until the update stands the context has no scene, so
    // an error on the way (MCPT_E_HIP, MCPT_E_NOMEM) cannot leave a half-updated one to be rendered.
    g.ok = false;
    HIPCHK(c, hipEventRecord(ev(c, EV_UPD_START), c->stream));
    if ((rc = mode == MCPT_GEOM_REFIT ? geometry_refit(c, s, n, v0, v1, v2, n0, n1, n2, nnodes)
                                      : geometry_rebuild(c, s, ntri, v0, v1, v2, n0, n1, n2, nnodes)))
        return rc;
    if ((rc = occ_state(c, s, nnodes, ms + 3))) return rc;
    HIPCHK(c, hipEventRecord(ev(c, EV_UPD_END), c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipEventElapsedTime(&ms[0], ev(c, EV_UPD_START), ev(c, EV_UPD_REC)));
    HIPCHK(c, hipEventElapsedTime(&ms[1], ev(c, EV_UPD_REC), ev(c, EV_UPD_TREE)));
    HIPCHK(c, hipEventElapsedTime(&ms[2], ev(c, EV_UPD_TREE), ev(c, EV_UPD_QUAD)));
    HIPCHK(c, hipEventElapsedTime(&ms[6], ev(c, EV_UPD_START), ev(c, EV_UPD_END)));
    scene_commit(c, s, true);
    // a rebuild re-sorted the records: the textures' uv stream follows (section 19; a refit keeps the order)
    if (mode == MCPT_GEOM_REBUILD && (rc = textures_reorder(c))) return rc;
    return emitter_table_refresh(c);  // areas and positions moved (emitter sampling, section 17)
}

// ---- base-colour textures ----
// The uv stream of t in the scene's record order: the desc-order uvs staged on the device, permuted by
// the upload's order array (a device-built tree stores its records in Morton order; nullptr: identity).
static int textures_uv_stream(mcpt_ctx* c, Textures& t) {
    const size_t n = (size_t)c->scene.ntri;
    t.dev_ok = false;
    if (!t.installed()) return MCPT_OK;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));  // no launch in flight reads the old stream
    // (section 21) the tangent stream, three float4 per record, behind the uv stream in the same allocation
    const bool tans = !t.tan[0].empty();
    const size_t tan_at = mcpt::tex_tan_offset((uint32_t)n);  // in float2
    if (!t.d_uv.ensure(tans ? tan_at + 6 * n : 3 * n) || !t.d_stage.ensure(3 * n) || (tans && !t.d_tstage.ensure(3 * n))) {
        (void)hipGetLastError();
        return set_err(c, MCPT_E_NOMEM, "hipMalloc: texture uv stream");
    }
    for (int k = 0; k < 3 && n; k++)
        HIPCHK(c, hipMemcpy(t.d_stage.get() + k * n, t.uv[k].data(), n * sizeof(float2), hipMemcpyHostToDevice));
    launch_tex_uv_records(t.d_stage.get(), t.d_stage.get() + n, t.d_stage.get() + 2 * n, c->scene.order, t.d_uv, (uint32_t)n,
                          c->stream);
    HIPCHK(c, hipGetLastError());
    if (tans) {
        for (int k = 0; k < 3 && n; k++)
            HIPCHK(c, hipMemcpy(t.d_tstage.get() + k * n, t.tan[k].data(), n * sizeof(float4), hipMemcpyHostToDevice));
        launch_tex_tangent_records(t.d_tstage.get(), t.d_tstage.get() + n, t.d_tstage.get() + 2 * n, c->scene.order,
                                   reinterpret_cast<float4*>(t.d_uv.get() + tan_at), (uint32_t)n, c->stream);
        HIPCHK(c, hipGetLastError());
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    t.dev_ok = true;
    return MCPT_OK;
}
int textures_reorder(mcpt_ctx* c) { return textures_uv_stream(c, c->tx); }

static int textures_install(mcpt_ctx* c, const mcpt_texture_set& set) {
    if (!c) return MCPT_E_INVALID;
    const int32_t ntri = set.ntri, ntex = set.ntex, nmat = set.nmat;
    const float *uv0 = set.uv0, *uv1 = set.uv1, *uv2 = set.uv2;
    const mcpt_texture* tex = set.textures;
    const int32_t *mat_tex = set.mat_tex, *mat_mr = set.mat_mr, *mat_nrm = set.mat_nrm;
    const float* tan[3] = {set.tan0, set.tan1, set.tan2};
    if (!c->scene.ok) return set_err(c, MCPT_E_INVALID, "no scene uploaded");
    auto changed = [c] {  // what a changed set means to the film, the history and the guides
        c->film_stale = true;
        c->tp.ok = false;
        c->guides.ok = false;
    };
    if (ntex == 0 || !tex) {  // removal
        HIPCHK(c, hipSetDevice(c->device));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        const bool was = c->tx.shaded();
        c->tx.drop();
        if (was) changed();
        return MCPT_OK;
    }
    if (ntri != c->scene.ntri) return set_err(c, MCPT_E_INVALID, "textures: ntri differs from the uploaded scene's");
    if (nmat != c->scene.nmat) return set_err(c, MCPT_E_INVALID, "textures: nmat differs from the uploaded scene's");
    if (ntex < 0 || !mat_tex || (ntri > 0 && (!uv0 || !uv1 || !uv2))) return set_err(c, MCPT_E_INVALID, "textures: null array");
    uint64_t total = 0;
    for (int32_t k = 0; k < ntex; k++) {
        if (tex[k].w < 1 || tex[k].w > 16384 || tex[k].h < 1 || tex[k].h > 16384)
            return set_err(c, MCPT_E_INVALID, "textures: width and height must be 1..16384");
        if (!tex[k].rgba8) return set_err(c, MCPT_E_INVALID, "textures: null texel pointer");
        total += (uint64_t)tex[k].w * (uint64_t)tex[k].h;
        if (total >= (1ull << 31)) return set_err(c, MCPT_E_INVALID, "textures: 2^31 texels or more in total");
    }
    for (int32_t m = 0; m < nmat; m++)
        if (mat_tex[m] < -1 || mat_tex[m] >= ntex) return set_err(c, MCPT_E_INVALID, "textures: material texture index out of range");
    for (int32_t m = 0; mat_mr && m < nmat; m++)
        if (mat_mr[m] < -1 || mat_mr[m] >= ntex)
            return set_err(c, MCPT_E_INVALID, "textures: material metallic-roughness texture index out of range");
    // the normal-map fields (section 21)
    const int ntan = (tan[0] != nullptr) + (tan[1] != nullptr) + (tan[2] != nullptr);
    if (ntan != 0 && ntan != 3) return set_err(c, MCPT_E_INVALID, "textures: one or two of the three tangent arrays");
    for (int32_t m = 0; mat_nrm && m < nmat; m++) {
        if (mat_nrm[m] < -1 || mat_nrm[m] >= ntex)
            return set_err(c, MCPT_E_INVALID, "textures: material normal texture index out of range");
        if (mat_nrm[m] >= 0 && ntan == 0) return set_err(c, MCPT_E_INVALID, "textures: a normal texture needs tangents");
    }
    for (int32_t m = 0; set.nrm_scale && m < nmat; m++)
        if (!std::isfinite(set.nrm_scale[m])) return set_err(c, MCPT_E_INVALID, "textures: non-finite normal scale");
    for (int k = 0; k < 3 && ntan; k++)
        for (size_t i = 0; i < 4 * (size_t)ntri; i++)
            if (!std::isfinite(tan[k][i])) return set_err(c, MCPT_E_INVALID, "textures: non-finite tangent component");
    // the per-texture flags (section 22; a flagged entry's index shares its word with kTexEntrySrgb)
    if (set.tex_flags && ntex >= mcpt::kTexEntrySrgb) return set_err(c, MCPT_E_INVALID, "textures: 2^30 textures or more with flags");
    for (int32_t k = 0; set.tex_flags && k < ntex; k++)
        if (set.tex_flags[k] & ~(uint32_t)MCPT_TEX_SRGB) return set_err(c, MCPT_E_INVALID, "textures: unknown texture flag");
    Textures now;
    if (set.tex_flags) now.flags.assign(set.tex_flags, set.tex_flags + ntex);
    now.nrm_fields = ntan != 0 || mat_nrm || set.nrm_scale;
    for (int k = 0; k < 3 && ntan; k++) now.tan[k].assign(tan[k], tan[k] + 4 * (size_t)ntri);
    if (mat_nrm) now.mat_nrm.assign(mat_nrm, mat_nrm + nmat);
    else now.mat_nrm.assign((size_t)nmat, -1);
    if (set.nrm_scale) now.nrm_scale.assign(set.nrm_scale, set.nrm_scale + nmat);
    else now.nrm_scale.assign((size_t)nmat, 1.f);
    const float* src[3] = {uv0, uv1, uv2};
    for (int k = 0; k < 3; k++) now.uv[k].assign(src[k], src[k] + 2 * (size_t)ntri);
    now.mat_tex.assign(mat_tex, mat_tex + nmat);
    if (mat_mr) now.mat_mr.assign(mat_mr, mat_mr + nmat);
    else now.mat_mr.assign((size_t)nmat, -1);
    now.atlas.resize((size_t)total);
    uint32_t at = 0;
    for (int32_t k = 0; k < ntex; k++) {
        const size_t px = (size_t)tex[k].w * (size_t)tex[k].h;
        now.tw.push_back(tex[k].w), now.th.push_back(tex[k].h), now.first.push_back(at);
        memcpy(now.atlas.data() + at, tex[k].rgba8, px * 4);
        at += (uint32_t)px;
    }
    // 2 nmat entries: the base-colour ones at nmat + m (TexView::mat points there), the metallic-roughness
    // ones in front of them and mirrored, at nmat - 1 - m (TexView::mat[-1 - m]; section 20)
    std::vector<int4> dm(2 * (size_t)nmat);
    auto entry = [&now](int32_t k) { return k < 0 ? make_int4(0, 0, 0, -1) : make_int4((int)now.first[k], now.tw[k], now.th[k], k); };
    // (section 22) a base-colour entry's fourth word carries its texture's sRGB flag for tex_base_srgb; every
    // other entry, and every entry of a set without a flagged base-colour texture, is the word it was
    auto srgb = [&now](int32_t k) { return k >= 0 && !now.flags.empty() && (now.flags[k] & MCPT_TEX_SRGB) != 0; };
    for (int32_t m = 0; m < nmat; m++) {
        dm[(size_t)nmat + m] = entry(now.mat_tex[m]);
        if (srgb(now.mat_tex[m])) dm[(size_t)nmat + m].w |= mcpt::kTexEntrySrgb, now.textured_srgb++;
        dm[(size_t)nmat - 1 - m] = entry(now.mat_mr[m]);
        now.textured += now.mat_tex[m] >= 0;
        now.textured_mr += now.mat_mr[m] >= 0;
        now.textured_nrm += now.mat_nrm[m] >= 0;
    }
    // (section 21) the normal entries {first texel, w, h, scale bits} in front of the atlas, mirrored: material
    // m's at int4 nmat - 1 - m of the allocation (TexView::atlas points behind them)
    std::vector<uint32_t> dn(4 * (size_t)nmat, 0u);
    for (int32_t m = 0; m < nmat; m++) {
        const int32_t k = now.mat_nrm[m];
        if (k < 0) continue;
        uint32_t* e = dn.data() + 4 * ((size_t)nmat - 1 - m);
        e[0] = now.first[k], e[1] = (uint32_t)now.tw[k], e[2] = (uint32_t)now.th[k];
        memcpy(e + 3, &now.nrm_scale[m], sizeof(float));
    }
    const Textures& was = c->tx;
    auto same_bytes = [](const auto& a, const auto& b) {
        return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(a[0])) == 0);
    };
    if (was.installed() && same_bytes(was.uv[0], now.uv[0]) && same_bytes(was.uv[1], now.uv[1]) && same_bytes(was.uv[2], now.uv[2]) &&
        same_bytes(was.tw, now.tw) && same_bytes(was.th, now.th) && same_bytes(was.mat_tex, now.mat_tex) &&
        same_bytes(was.mat_mr, now.mat_mr) && same_bytes(was.atlas, now.atlas) && same_bytes(was.mat_nrm, now.mat_nrm) &&
        same_bytes(was.nrm_scale, now.nrm_scale) && same_bytes(was.tan[0], now.tan[0]) && same_bytes(was.tan[1], now.tan[1]) &&
        same_bytes(was.tan[2], now.tan[2]) && was.nrm_fields == now.nrm_fields && same_bytes(was.flags, now.flags) &&
        (was.dev_ok || !was.shaded()))
        return MCPT_OK;  // an identical set does nothing
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));  // no launch in flight reads the old set
    if (!now.d_atlas.ensure(dn.size() + now.atlas.size()) || !now.d_mat.ensure(dm.size())) {
        (void)hipGetLastError();
        return set_err(c, MCPT_E_NOMEM, "hipMalloc: texture atlas");  // (the installed set stays)
    }
    if (!dn.empty()) HIPCHK(c, hipMemcpy(now.d_atlas, dn.data(), dn.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(now.d_atlas.get() + dn.size(), now.atlas.data(), now.atlas.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (!dm.empty()) HIPCHK(c, hipMemcpy(now.d_mat, dm.data(), dm.size() * sizeof(int4), hipMemcpyHostToDevice));
    if (int rc = textures_uv_stream(c, now)) return rc;
    // what the film depends on is what the lookups shade: a set without a textured material (in either
    // index array) shades as none
    // ... and a set that differs from the installed one only in normal-map fields no lookup reads (their
    // presence, the scale of a material without a normal map, the tangents while no material has one; section
    // 21) shades as it: the new set is installed and read back, the film, the history and the guides stay
    auto scale_in_use = [](const Textures& t, size_t m) { return t.mat_nrm[m] >= 0 ? t.nrm_scale[m] : 1.f; };
    bool same_shading = was.installed() && (was.dev_ok || !was.shaded()) && same_bytes(was.uv[0], now.uv[0]) &&
                        same_bytes(was.uv[1], now.uv[1]) && same_bytes(was.uv[2], now.uv[2]) && same_bytes(was.tw, now.tw) &&
                        same_bytes(was.th, now.th) && same_bytes(was.mat_tex, now.mat_tex) && same_bytes(was.mat_mr, now.mat_mr) &&
                        same_bytes(was.atlas, now.atlas) && same_bytes(was.mat_nrm, now.mat_nrm);
    for (size_t m = 0; same_shading && m < now.mat_nrm.size(); m++) {
        const float a = scale_in_use(was, m), b = scale_in_use(now, m);
        same_shading = memcmp(&a, &b, sizeof(float)) == 0;
    }
    if (same_shading && now.textured_nrm > 0)
        same_shading = same_bytes(was.tan[0], now.tan[0]) && same_bytes(was.tan[1], now.tan[1]) && same_bytes(was.tan[2], now.tan[2]);
    // ... nor do the texture flags (section 22) beyond the sRGB bit of a texture some base-colour slot uses
    auto srgb_in_use = [](const Textures& t, size_t m) {
        return t.mat_tex[m] >= 0 && !t.flags.empty() && (t.flags[(size_t)t.mat_tex[m]] & MCPT_TEX_SRGB) != 0;
    };
    for (size_t m = 0; same_shading && m < now.mat_tex.size(); m++) same_shading = srgb_in_use(was, m) == srgb_in_use(now, m);
    const bool differs = (was.shaded() || now.shaded()) && !same_shading;
    c->tx = std::move(now);
    if (differs) changed();
    return MCPT_OK;
}

extern "C" {

int mcpt_set_material_textures(mcpt_ctx* c, int32_t ntri, const float* uv0, const float* uv1, const float* uv2, int32_t ntex,
                               const mcpt_texture* textures, int32_t nmat, const int32_t* mat_tex) {
    return textures_install(c, mcpt_texture_set{ntri, uv0, uv1, uv2, nullptr, nullptr, nullptr, ntex, textures, nmat, mat_tex, nullptr,
                                                nullptr, nullptr, nullptr});
}
int mcpt_set_material_texture_maps(mcpt_ctx* c, int32_t ntri, const float* uv0, const float* uv1, const float* uv2, int32_t ntex,
                                   const mcpt_texture* textures, int32_t nmat, const int32_t* mat_tex, const int32_t* mat_mr) {
    return textures_install(c, mcpt_texture_set{ntri, uv0, uv1, uv2, nullptr, nullptr, nullptr, ntex, textures, nmat, mat_tex, mat_mr,
                                                nullptr, nullptr, nullptr});
}
int mcpt_set_material_texture_set(mcpt_ctx* c, const mcpt_texture_set* set) {
    if (!c) return MCPT_E_INVALID;
    if (!set) return set_err(c, MCPT_E_INVALID, "textures: null set");
    return textures_install(c, *set);
}
int mcpt_material_normal_read(mcpt_ctx* c, int32_t* nmat, int32_t* ntri_tan, int32_t* mat_nrm, float* nrm_scale, float* tan0,
                              float* tan1, float* tan2) {
    if (!c) return MCPT_E_INVALID;
    const Textures& t = c->tx;
    if (nmat) *nmat = t.nrm_fields ? (int32_t)t.mat_nrm.size() : 0;
    if (ntri_tan) *ntri_tan = (int32_t)(t.tan[0].size() / 4);
    if (!t.nrm_fields) return MCPT_OK;
    if (mat_nrm && !t.mat_nrm.empty()) memcpy(mat_nrm, t.mat_nrm.data(), t.mat_nrm.size() * sizeof(int32_t));
    if (nrm_scale && !t.nrm_scale.empty()) memcpy(nrm_scale, t.nrm_scale.data(), t.nrm_scale.size() * sizeof(float));
    float* dst[3] = {tan0, tan1, tan2};
    for (int k = 0; k < 3; k++)
        if (dst[k] && !t.tan[k].empty()) memcpy(dst[k], t.tan[k].data(), t.tan[k].size() * sizeof(float));
    return MCPT_OK;
}
int mcpt_debug_texture_normal_stats(const mcpt_ctx* c, int32_t* nrm_materials, int32_t* nrm_in_effect) {
    if (!c) return MCPT_E_INVALID;
    if (nrm_materials) *nrm_materials = c->tx.textured_nrm;
    if (nrm_in_effect) *nrm_in_effect = c->tx.view().uv && c->tx.textured_nrm > 0 ? 1 : 0;
    return MCPT_OK;
}
int mcpt_material_mr_read(mcpt_ctx* c, int32_t* nmat, int32_t* mat_mr) {
    if (!c) return MCPT_E_INVALID;
    if (nmat) *nmat = (int32_t)c->tx.mat_mr.size();
    if (mat_mr && !c->tx.mat_mr.empty()) memcpy(mat_mr, c->tx.mat_mr.data(), c->tx.mat_mr.size() * sizeof(int32_t));
    return MCPT_OK;
}
int mcpt_debug_texture_mr_stats(const mcpt_ctx* c, int32_t* mr_materials, int32_t* mr_in_effect) {
    if (!c) return MCPT_E_INVALID;
    if (mr_materials) *mr_materials = c->tx.textured_mr;
    if (mr_in_effect) *mr_in_effect = c->tx.view().uv && c->tx.textured_mr > 0 ? 1 : 0;
    return MCPT_OK;
}
int mcpt_material_textures_read(mcpt_ctx* c, int32_t* ntri, int32_t* ntex, int32_t* nmat, int32_t* mat_tex, int32_t tex,
                                int32_t* w, int32_t* h, uint8_t* rgba8, float* uv0, float* uv1, float* uv2) {
    if (!c) return MCPT_E_INVALID;
    const Textures& t = c->tx;
    if (ntri) *ntri = (int32_t)(t.uv[0].size() / 2);
    if (ntex) *ntex = (int32_t)t.tw.size();
    if (nmat) *nmat = (int32_t)t.mat_tex.size();
    if (!t.installed()) return MCPT_OK;
    if (tex >= (int32_t)t.tw.size()) return set_err(c, MCPT_E_INVALID, "textures: no such texture");
    if (mat_tex) memcpy(mat_tex, t.mat_tex.data(), t.mat_tex.size() * sizeof(int32_t));
    if (tex >= 0) {
        if (w) *w = t.tw[tex];
        if (h) *h = t.th[tex];
        if (rgba8) memcpy(rgba8, t.atlas.data() + t.first[tex], (size_t)t.tw[tex] * t.th[tex] * 4);
    }
    float* dst[3] = {uv0, uv1, uv2};
    for (int k = 0; k < 3; k++)
        if (dst[k] && !t.uv[k].empty()) memcpy(dst[k], t.uv[k].data(), t.uv[k].size() * sizeof(float));
    return MCPT_OK;
}
int mcpt_material_texture_flags_read(mcpt_ctx* c, int32_t* ntex, uint32_t* tex_flags) {
    if (!c) return MCPT_E_INVALID;
    if (ntex) *ntex = (int32_t)c->tx.flags.size();
    if (tex_flags && !c->tx.flags.empty()) memcpy(tex_flags, c->tx.flags.data(), c->tx.flags.size() * sizeof(uint32_t));
    return MCPT_OK;
}
int mcpt_debug_texture_srgb_stats(const mcpt_ctx* c, int32_t* srgb_materials, int32_t* srgb_in_effect) {
    if (!c) return MCPT_E_INVALID;
    if (srgb_materials) *srgb_materials = c->tx.textured_srgb;
    if (srgb_in_effect) *srgb_in_effect = c->tx.view().uv && c->tx.textured_srgb > 0 ? 1 : 0;
    return MCPT_OK;
}
int mcpt_texture_sample_run(mcpt_ctx* c, int32_t w, int32_t h, const uint8_t* rgba8, uint32_t n, const float* uv,
                            float* out_rgb) {
    return mcpt_texture_sample_run_ex(c, w, h, rgba8, 0u, n, uv, out_rgb);
}
int mcpt_texture_sample_run_ex(mcpt_ctx* c, int32_t w, int32_t h, const uint8_t* rgba8, uint32_t flags, uint32_t n,
                               const float* uv, float* out_rgb) {
    if (!c) return MCPT_E_INVALID;
    if (flags & ~(uint32_t)MCPT_TEX_SRGB) return set_err(c, MCPT_E_INVALID, "texture sample: unknown texture flag");
    if (w < 1 || w > 16384 || h < 1 || h > 16384 || !rgba8) return set_err(c, MCPT_E_INVALID, "texture sample: bad image");
    if (n == 0) return MCPT_OK;
    if (!uv || !out_rgb || n >= (1u << 28)) return set_err(c, MCPT_E_INVALID, "texture sample: bad uv / output array");
    HIPCHK(c, hipSetDevice(c->device));
    TmpScope tmp(c);
    uint32_t* d_tex = nullptr;
    float2* d_uv = nullptr;
    float* d_out = nullptr;
    int rc;
    if ((rc = dupload(c, tmp.L, &d_tex, reinterpret_cast<const uint32_t*>(rgba8), (size_t)w * h)) ||
        (rc = dupload(c, tmp.L, &d_uv, reinterpret_cast<const float2*>(uv), (size_t)n)) || (rc = dalloc(c, tmp.L, &d_out, 3 * (size_t)n)))
        return rc;
    if (flags & MCPT_TEX_SRGB) launch_tex_sample_srgb(d_tex, w, h, d_uv, d_out, n, c->stream);
    else launch_tex_sample(d_tex, w, h, d_uv, d_out, n, c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(out_rgb, d_out, 3 * (size_t)n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MCPT_OK;
}
int mcpt_debug_texture_stats(const mcpt_ctx* c, uint64_t* bytes, int32_t* textured_materials, int32_t* in_effect) {
    if (!c) return MCPT_E_INVALID;
    if (bytes) *bytes = (uint64_t)c->tx.bytes();
    if (textured_materials) *textured_materials = c->tx.textured;
    if (in_effect) *in_effect = c->tx.view().uv ? 1 : 0;
    return MCPT_OK;
}

int mcpt_scene_upload(mcpt_ctx* c, const mcpt_scene_desc* d) { return scene_upload(c, d, false); }
int mcpt_scene_upload_gpu_bvh(mcpt_ctx* c, const mcpt_scene_desc* d) { return scene_upload(c, d, true); }
int mcpt_set_gpu_bvh_builder(mcpt_ctx* c, int32_t builder) {
    if (!c || (builder != MCPT_GPU_BVH_LBVH && builder != MCPT_GPU_BVH_PLOC))
        return set_err(c, MCPT_E_INVALID, "unknown GPU BVH builder");
    c->gpu_bvh_builder = builder;
    return MCPT_OK;
}

int mcpt_scene_update_geometry(mcpt_ctx* c, int32_t ntri, const float* v0, const float* v1, const float* v2,
                               const float* n0, const float* n1, const float* n2, int32_t mode) {
    int rc = geometry_check(c, ntri, v0, v1, v2, n0, n1, n2, mode);
    if (rc || ntri == 0) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const size_t m = 3 * (size_t)ntri;
    const float* src[6] = {v0, v1, v2, n0, n1, n2};
    const int arrays = n0 ? 6 : 3;
    if (!c->scene.stage.ensure(arrays * m)) return set_err(c, MCPT_E_NOMEM, "hipMalloc: geometry staging");
    float* st = c->scene.stage;
    for (int k = 0; k < arrays; k++) HIPCHK(c, hipMemcpy(st + k * m, src[k], m * sizeof(float), hipMemcpyHostToDevice));
    return geometry_update_device(c, ntri, st, st + m, st + 2 * m, n0 ? st + 3 * m : nullptr, n0 ? st + 4 * m : nullptr,
                                  n0 ? st + 5 * m : nullptr, mode);
}
int mcpt_scene_update_geometry_device(mcpt_ctx* c, int32_t ntri, const void* d_v0, const void* d_v1, const void* d_v2,
                                      const void* d_n0, const void* d_n1, const void* d_n2, int32_t mode) {
    int rc = geometry_check(c, ntri, d_v0, d_v1, d_v2, d_n0, d_n1, d_n2, mode);
    if (rc) return rc;
    return geometry_update_device(c, ntri, (const float*)d_v0, (const float*)d_v1, (const float*)d_v2, (const float*)d_n0,
                                  (const float*)d_n1, (const float*)d_n2, mode);
}

// ---- debug readers of the scene state ----
int mcpt_debug_geometry_update_ms(const mcpt_ctx* c, float* out8) {
    if (!c || !out8) return MCPT_E_INVALID;
    for (int k = 0; k < 8; k++) out8[k] = c->scene.update_ms[k];
    return MCPT_OK;
}
float mcpt_debug_last_build_ms(const mcpt_ctx* c) { return c ? c->scene.build_ms : -1.f; }
float mcpt_debug_last_env_build_ms(const mcpt_ctx* c) { return c ? c->scene.env_build_ms : -1.f; }

int mcpt_debug_env_tables(mcpt_ctx* c, float* marginal_y, float* conds_y, float* pdf, int32_t* flags) {
    if (!c) return set_err(c, MCPT_E_INVALID, "null context");
    const mcpt::EnvView& e = c->scene.dev.env;
    if (!c->scene.ok || e.mode != 1 || !e.tex) return set_err(c, MCPT_E_INVALID, "no HRDI scene uploaded");
    const size_t WH = (size_t)e.w * e.h;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (marginal_y) HIPCHK(c, hipMemcpy(marginal_y, e.marginal_y, (size_t)e.h * sizeof(float), hipMemcpyDeviceToHost));
    if (conds_y) HIPCHK(c, hipMemcpy(conds_y, e.conds_y, WH * sizeof(float), hipMemcpyDeviceToHost));
    if (pdf) HIPCHK(c, hipMemcpy(pdf, e.pdf, WH * sizeof(float), hipMemcpyDeviceToHost));
    if (flags) *flags = (c->scene.env_device_built ? 1 : 0) | (c->scene.env_guides ? 2 : 0);
    return MCPT_OK;
}
int mcpt_debug_node_layout(const mcpt_ctx* c) { return c ? c->scene.node_layout : MCPT_E_INVALID; }
int mcpt_debug_bvh_read(mcpt_ctx* c, float* nodes, float* tris, mcpt_bvh_info* info) {
    if (!c) return set_err(c, MCPT_E_INVALID, "null context");
    const SceneState& sc = c->scene;
    if (!sc.ok) return set_err(c, MCPT_E_INVALID, "no scene uploaded");
    const DevScene& s = sc.dev;
    if (info) {
        info->npairs = (int32_t)sc.pair_count;
        info->root_ref = sc.pair_root;
        info->depth = sc.pair_depth;
        info->width = s.width;
        info->layout = sc.node_layout;
        info->ntri = (int32_t)s.ntri;
        info->tri_f4 = kTriF4;
        info->gpu_built = sc.pair_gpu_built ? 1 : 0;
        info->rounds = sc.ploc_rounds;
        for (int k = 0; k < 3; k++) { info->root_mn[k] = s.root_mn[k]; info->root_mx[k] = s.root_mx[k]; }
        info->cull_p = s.cull_p;
    }
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (nodes && sc.pair_count)
        HIPCHK(c, hipMemcpy(nodes, sc.pair_nodes, (size_t)sc.pair_count * 4 * sizeof(float4), hipMemcpyDeviceToHost));
    if (tris && s.ntri)
        HIPCHK(c, hipMemcpy(tris, s.tri, (size_t)s.ntri * kTriF4 * sizeof(float4), hipMemcpyDeviceToHost));
    return MCPT_OK;
}

}  // extern "C"
