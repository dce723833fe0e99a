// k_material_body.inc -- the body of k_material and of its TexMr overload (kernels.hip), included into each:
// one text, so that k_material's instantiations stay the code they were while k_material<TexMr, ...> adds the
// metallic-roughness level (DESIGN.md section 20).  The including kernel defines
//   FIXED, SAMP, MIS   its template arguments
//   TEX                the texture level: 0 none, 1 base colour, 2 base colour and metallic-roughness,
//                      3 those and the normal map (DESIGN.md section 21), 4 level 3 with the base-colour
//                      lookup decoding sRGB-flagged textures (DESIGN.md section 22)
//   tex_stash          levels 2 to 4: the block's 5 x kBlock LDS floats (material()); else nullptr
    const ShadeArgs& a = kernarg_fresh<ShadeArgs>();
    if (a.cnt->idle) return;  // the tile set is complete
    const uint32_t shard = blockIdx.x % kShards, w_in = blockIdx.x / kShards, bps = gridDim.x / kShards;
    uint32_t* sc_ctr = a.cnt->shard[shard];
    const uint32_t n = sc_ctr[C_MAT];
    const int lane = threadIdx.x & 63;
    uint32_t n_ext = 0, n_any = 0, n_vis = 0, n_occ = 0, occ_try = 0, n_skip = 0, n_inpl = 0, n_dvis = 0, n_docc = 0;
    uint32_t n_emit = 0;  // SAMP: emitter rays made
    (void)n_emit;
    const bool occ_on = a.scene.occ && a.scene.occ_gate[0] == 0 && a.scene.occ_gate[2] != 0;  // see DevScene::occ_gate
    // Any-hit rays are staged here (light ray o/d, BRDF visibility ray o/d) and stored after
    // the block push at their queue positions: the block's rays of one kind land contiguously,
    // so k_trace reads them densely and without the queue-entry hop (the pid-indexed layout
    // wrote and read 32-B pieces of partly used lines).
    __shared__ float4 s_any[SAMP ? 6 : 4][kBlock];
    for (uint32_t base = w_in * kBlock; base < n; base += bps * kBlock) {  // block-uniform trip count
        const ShadeArgs& a = kernarg_fresh<ShadeArgs>();  // this trip's loads (see kernarg_fresh)
        const uint32_t i = base + threadIdx.x;
        MatOut mo{};
        bool want_e = false;  // SAMP: the emitter ray (DESIGN.md section 17)
        uint32_t mpid = 0;
        bool occ_l = false, occ_b = false, try_l = false, try_b = false;  // resolved by / tested against the occluder cache
        bool done_l = false, done_b = false, clr_l = false, clr_b = false;  // ... from a complete entry / as unoccluded
        if (i < n) {
            const uint4 q = ld_s(a.mat_rec + shard * a.ext_cap + i);  // {pid, pixel, sample index | len << 24, hit_tri}
            const float4 b4 = ld_s(a.mat_beta + shard * a.ext_cap + i);
            mpid = q.x;
            mo = material<FIXED, SAMP, MIS, TEX>(a, mpid, q.y, q.z & (kRecNoCont - 1u), q.z >> kRecLenShift, xyz(b4), (int32_t)q.w,
                                            &s_any[0][0], occ_on, (q.z & kRecNoCont) != 0u, want_e, tex_stash);
            // the occluder cache (see occ_hit1), before the BRDF sample's light terms: a ray it
            // resolves gets its wf_shadow result here and is not queued
            MCPT_MARK("m_occ");
            if (occ_on) {
                try_l = mo.want_l;
                try_b = mo.want_b;
                const V3 ol = xyz(s_any[0][threadIdx.x]), dl = xyz(s_any[1][threadIdx.x]);
                const V3 ob = xyz(s_any[2][threadIdx.x]), db = xyz(s_any[3][threadIdx.x]);
                if (mo.want_l) {
                    const int r = occ_hit1(a.scene, ol, dl, mo.el, done_l);
                    occ_l = r == kOccHit;
                    clr_l = r == kOccMaybe;
                }
                if (mo.want_b) {
                    const int r = occ_hit1(a.scene, ob, db, mo.eb, done_b);
                    occ_b = r == kOccHit;
                    clr_b = r == kOccMaybe;
                }
                if (clr_l || clr_b) {
                    bool m_l, m_b;
                    occ_member2(a.scene, ol, dl, mo.kl, ob, db, mo.kb, m_l, m_b);
                    clr_l = clr_l && m_l;
                    clr_b = clr_b && m_b;
                }
                // unoccluded by a complete entry: wf_shadow's result for a ray that finds nothing
                if (clr_l) {
                    a.p.vis[2 * mpid] = 1;
                    mo.want_l = false;
                    mo.trivial_any++;
                }
                if (clr_b) {
                    a.p.vis[2 * mpid + 1] = 1;
                    mo.want_b = false;
                    mo.trivial_any++;
                }
                if (occ_l) {
                    a.p.vis[2 * mpid] = 0;
                    mo.want_l = false;
                    mo.trivial_any++;
                }
                if (occ_b) {
                    a.p.vis[2 * mpid + 1] = 0;
                    mo.want_b = false;
                    mo.need_cb = false;
                    mo.trivial_any++;
                }
            }
            MCPT_MARK("m_bterms");
            material_brdf_terms<FIXED, TEX>(a, mpid, mo, tex_stash);
        }
        MCPT_MARK("m_push");
        uint32_t slot[SAMP ? 4 : 3], total[SAMP ? 4 : 3];
        if constexpr (SAMP) {
            bool want[4] = {mo.want_ext, mo.want_l, mo.want_b, want_e};
            uint32_t* ctr[4] = {sc_ctr + C_EXT, sc_ctr + C_ANY, sc_ctr + C_ANY, sc_ctr + C_ANY};
            block_push<4>(want, ctr, slot, total);
        } else {
            bool want[3] = {mo.want_ext, mo.want_l, mo.want_b};
            uint32_t* ctr[3] = {sc_ctr + C_EXT, sc_ctr + C_ANY, sc_ctr + C_ANY};
            block_push<3>(want, ctr, slot, total);
        }
        if (mo.want_ext) st_q(a.ext_q + shard * a.ext_cap + slot[0], mpid);
        // (the any-hit rays carry their result index in o.w: no queue entries)
        if (mo.want_l) {
            const uint32_t k = shard * a.any_cap + slot[1];
            if constexpr (MCPT_NT & 8) {
                st_s(a.p.sray_o + k, s_any[0][threadIdx.x]);
                st_s(a.p.sray_d + k, s_any[1][threadIdx.x]);
            } else {
                a.p.sray_o[k] = s_any[0][threadIdx.x];
                a.p.sray_d[k] = s_any[1][threadIdx.x];
            }
        }
        if (mo.want_b) {
            const uint32_t k = shard * a.any_cap + slot[2];
            if constexpr (MCPT_NT & 8) {
                st_s(a.p.sray_o + k, s_any[2][threadIdx.x]);
                st_s(a.p.sray_d + k, s_any[3][threadIdx.x]);
            } else {
                a.p.sray_o[k] = s_any[2][threadIdx.x];
                a.p.sray_d[k] = s_any[3][threadIdx.x];
            }
        }
        if constexpr (SAMP) {
            if (want_e) {  // (any_cap is 3 x ext_cap while sampling is active: set_tiles_internal)
                const uint32_t k = shard * a.any_cap + slot[3];
                if constexpr (MCPT_NT & 8) {
                    st_s(a.p.sray_o + k, s_any[4][threadIdx.x]);
                    st_s(a.p.sray_d + k, s_any[5][threadIdx.x]);
                } else {
                    a.p.sray_o[k] = s_any[4][threadIdx.x];
                    a.p.sray_d[k] = s_any[5][threadIdx.x];
                }
            }
            n_emit += (uint32_t)__popcll(__ballot(want_e));
        }
        MCPT_MARK("m_count");
        // per-wave ray counts from lane masks (wave-uniform scalars: no registers held across the
        // next trip's material())
        n_occ += (uint32_t)(__popcll(__ballot(occ_l)) + __popcll(__ballot(occ_b)));
        occ_try += (uint32_t)(__popcll(__ballot(try_l)) + __popcll(__ballot(try_b)));
        n_dvis += (uint32_t)(__popcll(__ballot(clr_l)) + __popcll(__ballot(clr_b)));
        n_docc += (uint32_t)(__popcll(__ballot(occ_l && done_l)) + __popcll(__ballot(occ_b && done_b)));
        // queued + resolved-in-place rays + those the next logic pass would discard (counted, not made)
        n_ext += (uint32_t)__popcll(__ballot(mo.want_ext || mo.trivial_ext || mo.skip_ext));
        n_skip += (uint32_t)__popcll(__ballot(mo.skip_ext));
        n_inpl += (uint32_t)__popcll(__ballot(mo.doomed_inplace));
        n_any += (uint32_t)(__popcll(__ballot(mo.want_l)) + __popcll(__ballot(mo.want_b)) +
                            __popcll(__ballot(mo.trivial_any >= 1u)) + __popcll(__ballot(mo.trivial_any >= 2u)));
        n_vis += (uint32_t)__popcll(__ballot(mo.vis_ray));
    }
    if (lane == 0) {
        if (n_ext) atomicAdd(sc_ctr + C_EXT_RAYS, n_ext);
        if (n_any) atomicAdd(sc_ctr + C_ANY_RAYS, n_any);
        if (n_vis) atomicAdd(sc_ctr + C_VIS, n_vis);
        if (n_occ) atomicAdd(sc_ctr + C_OCC, n_occ);
        if (occ_try) atomicAdd(sc_ctr + C_OCC_TRY, occ_try);
        if (n_dvis) atomicAdd(sc_ctr + C_OCC_DONE_VIS, n_dvis);
        if (n_docc) atomicAdd(sc_ctr + C_OCC_DONE_OCC, n_docc);
        if (n_skip) atomicAdd(sc_ctr + C_SKIP_EXT, n_skip);
        if (n_inpl) atomicAdd(sc_ctr + C_SKIP_INPLACE, n_inpl);
        if constexpr (SAMP)
            if (n_emit) atomicAdd(a.cnt->tot_emit + shard, (unsigned long long)n_emit);
    }
