// postprocess.cpp -- film post-processing behind the mcpt_* C ABI (include/mcpt.h): the preview
// denoiser's guide buffers and a-trous filter (DESIGN.md sections 10 and 12), adaptive sampling
// (section 11), temporal accumulation (section 13) and the spatial variance estimate (section 14).
// The context, the film and the render loop are runtime.cpp's; runtime_internal.hpp holds what the
// two share.
#include <cfloat>

#include "runtime_internal.hpp"

// ---------------------------------------------------------------------------
// Helpers of every stage below
// ---------------------------------------------------------------------------
// A device-time span on the context's stream: span_begin, the launches, span_end (launch error, end
// event, synchronise, the time between events 0 and 1 -> *ms)
static int span_begin(mcpt_ctx* c) {
    HIPCHK(c, hipEventRecord(ev(c, 0), c->stream));
    return MCPT_OK;
}
static int span_end(mcpt_ctx* c, float* ms) {
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(ev(c, 1), c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipEventElapsedTime(ms, c->events[0], c->events[1]));
    return MCPT_OK;
}
// MCPT_OK when the last iteration since the film clear left no live path (the counters' host copy),
// else MCPT_E_INVALID with `busy` as its text
static int require_idle(mcpt_ctx* c, const char* busy) {
    if (!c->cnt.totals_ok)
        if (int rc = c->cnt.refresh(c)) return rc;
    return c->cnt.totals.last_live != 0 ? set_err(c, MCPT_E_INVALID, busy) : MCPT_OK;
}
// The caller's parameters, or the defaults where it passed none
template <class P>
static P params_or(const P* pp, int (*defaults)(P*)) {
    P p;
    if (pp) p = *pp;
    else (void)defaults(&p);
    return p;
}
static bool finite_nonneg(float v) { return v >= 0.f && v <= FLT_MAX; }  // false for NaN
// DevBuf::ensure with dalloc's error
template <class T>
static int ensure_or_nomem(mcpt_ctx* c, DevBuf<T>& b, size_t count) {
    if (b.ensure(count)) return MCPT_OK;
    return set_err(c, MCPT_E_NOMEM, std::string("hipMalloc: ") + hipGetErrorString(hipGetLastError()));
}
// Read-back of the first component of n float2
static int read_x(mcpt_ctx* c, const float2* d, size_t n, float* x) {
    std::vector<float2> o(n);
    HIPCHK(c, hipMemcpy(o.data(), d, n * sizeof(float2), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; i++) x[i] = o[i].x;
    return MCPT_OK;
}

// ---------------------------------------------------------------------------
// Preview denoiser: first-hit guide buffers and the a-trous filter
// (device/denoise.hpp, denoise.hip) between the film and the display.
// ---------------------------------------------------------------------------
static bool guides_valid(const mcpt_ctx* c) {
    const Guides& g = c->guides;
    return g.ok && g.alb && g.nz && g.key.same(c->view(), ViewKey::SCENE | ViewKey::SEED | ViewKey::CAM);
}
// The filter's planes of the film: allocates those that are missing, the float2 planes only with_vl,
// and forgets the last result.  false: an allocation failed and every plane was freed.
static bool denoise_planes_ensure(mcpt_ctx* c, bool with_vl) {
    Denoise& d = c->dn;
    d.result = -1;
    d.guided = false;
    const size_t P = c->film.pixels();
    const bool ok = d.col[0].ensure(P) && d.col[1].ensure(P) && d.gd.ensure(P) && d.al.ensure(P) &&
                    (!with_vl || (d.vl[0].ensure(P) && d.vl[1].ensure(P)));
    if (!ok) {
        (void)hipGetLastError();
        d = Denoise{};
    }
    return ok;
}
// One filter request, from either parameter struct: the plain parameters, and with `guided` the
// variance-guided form's two; `who` heads its error texts
struct DenoiseRequest {
    mcpt_denoise_params p;
    bool guided;
    float sigma_lum, lum_eps;
    const char* who;
};
static DenoiseRequest denoise_request(const mcpt_denoise_params& p) { return {p, false, 0.f, 0.f, "denoise"}; }
static DenoiseRequest denoise_request(const mcpt_denoise_guided_params& q) {
    return {{q.passes, q.sigma_color, q.sigma_normal, q.sigma_albedo, q.sigma_depth}, true, q.sigma_lum, q.lum_eps,
            "guided denoise"};
}
static int denoise_check_params(mcpt_ctx* c, const DenoiseRequest& r) {
    if (r.p.passes < 1 || r.p.passes > 8) return set_err(c, MCPT_E_INVALID, std::string(r.who) + ": passes must be 1..8");
    if (!r.guided) return MCPT_OK;
    if (!finite_nonneg(r.sigma_lum) || !(r.sigma_lum > 0.f)) return set_err(c, MCPT_E_INVALID, "guided denoise: sigma_lum must be > 0");
    if (!finite_nonneg(r.lum_eps)) return set_err(c, MCPT_E_INVALID, "guided denoise: lum_eps must be >= 0");
    return MCPT_OK;
}
// The passes over planes of a W x H image, after the caller's span_begin and prepare launch: col
// ping-pongs, and vl with it where the request is guided (vl is not looked at otherwise); *result =
// the plane that holds the last pass
static int denoise_passes(mcpt_ctx* c, const DenoiseRequest& r, uint32_t W, uint32_t H, float4* const col[2],
                          float2* const vl[2], const float4* gd, const float4* al, int* result) {
    const mcpt_denoise_params& p = r.p;
    int lds_max = 2;  // MCPT_DENOISE_LDS_MAX: the widest stride that takes the LDS kernel (A/B; same bits)
    if (const char* e = getenv(kDenoiseLdsEnv))
        if (e[0] >= '0' && e[0] <= '2' && e[1] == 0) lds_max = e[0] - '0';
    float* ms = c->ms.dn;
    for (int i = 0; i < 8; i++) ms[1 + i] = 0.f;
    int src = 0;
    for (int i = 0; i < p.passes; i++) {
        DenoiseGuidedArgs a{};
        float sc = p.sigma_color;
        for (int k = 0; k < i; k++) sc = sc * 0.5f;  // sigma_color 2^-i
        a.k.kc = mcpt::dn_k(sc);
        a.k.kn = mcpt::dn_k(p.sigma_normal);
        a.k.ka = mcpt::dn_k(p.sigma_albedo);
        a.k.kz = mcpt::dn_k(p.sigma_depth);
        a.k.stride = 1 << i;
        a.W = (int)W;
        a.H = (int)H;
        a.col = col[src];
        a.gd = gd;
        a.al = al;
        a.out = col[src ^ 1];
        if (r.guided) a.v = {r.sigma_lum, r.lum_eps, vl[src], vl[src ^ 1]};
        HIPCHK(c, hipEventRecord(ev(c, 1 + (size_t)i), c->stream));
        launch_denoise_pass(a, lds_max, c->stream);
        src ^= 1;
    }
    HIPCHK(c, hipEventRecord(ev(c, 1 + (size_t)p.passes), c->stream));
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i <= p.passes; i++) HIPCHK(c, hipEventElapsedTime(&ms[i], c->events[i], c->events[i + 1]));
    *result = src;
    return MCPT_OK;
}
// The context's planes through the passes, after the caller's span_begin and prepare launch into
// them; the result is remembered
static int denoise_film_planes(mcpt_ctx* c, const DenoiseRequest& r) {
    Denoise& d = c->dn;
    float4* const col[2] = {d.col[0], d.col[1]};
    float2* const vl[2] = {d.vl[0], d.vl[1]};
    int res = 0;
    if (int rc = denoise_passes(c, r, c->W, c->H, col, vl, d.gd, d.al, &res)) return rc;
    d.result = res;
    d.guided = r.guided;
    return MCPT_OK;
}

// mcpt_denoise_run / mcpt_denoise_guided_run (whose null checks come first): upload, planes, passes,
// read-back.  variance and out_variance are the guided form's; out_variance may be nullptr.
static int denoise_run(mcpt_ctx* c, const DenoiseRequest& r, uint32_t w, uint32_t h, const float* rgb, const uint32_t* samples,
                       const float* variance, const float* albedo, const float* normal, const float* depth, float* out_rgb,
                       float* out_variance) {
    if (w == 0 || h == 0 || (uint64_t)w * h >= (1ull << 28))
        return set_err(c, MCPT_E_INVALID, std::string(r.who) + ": bad image size");
    int rc = denoise_check_params(c, r);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n = (size_t)w * h;
    TmpScope tmp(c);
    auto& L = tmp.L;
    float *d_rgb, *d_al, *d_n, *d_z, *d_v = nullptr;
    uint32_t* d_s = nullptr;
    float4 *col[2], *gd, *al;
    float2* vl[2] = {nullptr, nullptr};
    if ((rc = dupload(c, L, &d_rgb, rgb, 3 * n)) || (rc = dupload(c, L, &d_al, albedo, 3 * n)) ||
        (rc = dupload(c, L, &d_n, normal, 3 * n)) || (rc = dupload(c, L, &d_z, depth, n)) ||
        (samples && (rc = dupload(c, L, &d_s, samples, n))) || (rc = dalloc(c, L, &col[0], n)) ||
        (rc = dalloc(c, L, &col[1], n)) || (rc = dalloc(c, L, &gd, n)) || (rc = dalloc(c, L, &al, n)) ||
        (r.guided && ((rc = dupload(c, L, &d_v, variance, n)) || (rc = dalloc(c, L, &vl[0], n)) || (rc = dalloc(c, L, &vl[1], n)))))
        return rc;
    DenoiseGuidedPrepArgs pa{};
    pa.samples = d_s;
    pa.rgb = d_rgb;
    pa.normal = d_n;
    pa.albedo = d_al;
    pa.depth = d_z;
    pa.col = col[0];
    pa.gd = gd;
    pa.al = al;
    pa.n = (uint32_t)n;
    pa.variance = d_v;
    pa.vl = vl[0];
    if ((rc = span_begin(c))) return rc;
    launch_denoise_prep(pa, c->stream);
    int res = 0;
    if ((rc = denoise_passes(c, r, w, h, col, vl, gd, al, &res))) return rc;
    if ((rc = read_plane(c, col[res], n, out_rgb, nullptr))) return rc;
    return out_variance ? read_x(c, vl[res], n, out_variance) : MCPT_OK;
}

// ---- spatial variance estimate: what the film stages below share ----
static int variance_check_params(mcpt_ctx* c, const mcpt_variance_params& p) {
    if (p.radius < 1 || p.radius > 3) return set_err(c, MCPT_E_INVALID, "variance: radius must be 1..3");
    if (!mcpt::dn_finite(p.sigma_normal)) return set_err(c, MCPT_E_INVALID, "variance: sigma_normal must be a finite number");
    if (!mcpt::dn_finite(p.sigma_albedo)) return set_err(c, MCPT_E_INVALID, "variance: sigma_albedo must be a finite number");
    if (!mcpt::dn_finite(p.sigma_depth)) return set_err(c, MCPT_E_INVALID, "variance: sigma_depth must be a finite number");
    if (!(p.min_neff >= 1.f && p.min_neff <= FLT_MAX)) return set_err(c, MCPT_E_INVALID, "variance: min_neff must be a finite number >= 1");
    return MCPT_OK;
}
// k_variance_spatial over planes of a W x H image, in place on vl, between events 10 and 11 (past the
// filter's 0 .. 9); variance_time, after the stream is synchronised: its device time -> ms.var
constexpr size_t kVarianceEv = 10;
static int variance_launch(mcpt_ctx* c, const mcpt_variance_params& p, uint32_t W, uint32_t H, const float4* col,
                           const float4* gd, const float4* al, float2* vl) {
    VarianceArgs a{};
    a.k = mcpt::VariancePass{mcpt::dn_k(p.sigma_normal), mcpt::dn_k(p.sigma_albedo), mcpt::dn_k(p.sigma_depth), p.min_neff, p.radius};
    a.W = (int)W;
    a.H = (int)H;
    a.col = col;
    a.gd = gd;
    a.al = al;
    a.vl = vl;
    HIPCHK(c, hipEventRecord(ev(c, kVarianceEv), c->stream));
    launch_variance_spatial(a, c->stream);
    HIPCHK(c, hipEventRecord(ev(c, kVarianceEv + 1), c->stream));
    return MCPT_OK;
}
static int variance_time(mcpt_ctx* c) {
    HIPCHK(c, hipEventElapsedTime(&c->ms.var, c->events[kVarianceEv], c->events[kVarianceEv + 1]));
    return MCPT_OK;
}
// The film's planes into the context's (after denoise_planes_ensure(c, guided)).  Guided: variance =
// se^2 of the last mcpt_film_error with >= 2 path slots, unknown everywhere with one; then, with the
// fill on, the estimate where it is unknown.  Launches only; variance_time is the caller's.
static int film_planes(mcpt_ctx* c, bool guided, const float4* Ld, const uint32_t* samples) {
    DenoiseGuidedPrepArgs pa{};
    pa.Ld = Ld;
    pa.samples = samples;
    pa.g_alb = c->guides.alb;
    pa.g_nz = c->guides.nz;
    pa.col = c->dn.col[0];
    pa.gd = c->dn.gd;
    pa.al = c->dn.al;
    pa.n = (uint32_t)c->film.pixels();
    if (guided) {
        pa.err = c->slots >= 2 ? c->ad.err4.get() : nullptr;
        pa.vl = c->dn.vl[0];
    }
    launch_denoise_prep(pa, c->stream);
    if (!guided || !c->vf.on) return MCPT_OK;
    return variance_launch(c, c->vf.p, c->W, c->H, c->dn.col[0], c->dn.gd, c->dn.al, c->dn.vl[0]);
}

// mcpt_film_denoise / mcpt_film_denoise_guided: the film and the context's guides through the
// context's planes.  Guided: the variance is se^2 of a fresh mcpt_film_error estimate, on that
// call's own path (its checks: >= 2 path slots, no paths in flight); with the variance fill on, one
// path slot skips that call (no paths in flight all the same) and every variance is the estimate.
static int film_denoise(mcpt_ctx* c, const DenoiseRequest& r) {
    if (!c || !c->film.allocated) return set_err(c, MCPT_E_INVALID, "film not allocated");
    int rc = denoise_check_params(c, r);
    if (rc) return rc;
    if (!guides_valid(c))
        return set_err(c, MCPT_E_INVALID, "denoise: guide buffers missing or stale (camera, scene or film changed): call mcpt_guides_render first");
    if (r.guided && c->vf.on && c->slots < 2) {
        HIPCHK(c, hipSetDevice(c->device));
        if ((rc = require_idle(c, "guided denoise: paths are in flight"))) return rc;
    } else if (r.guided && (rc = mcpt_film_error(c))) {
        return rc;
    }
    HIPCHK(c, hipSetDevice(c->device));
    if (!denoise_planes_ensure(c, r.guided)) return set_err(c, MCPT_E_NOMEM, std::string(r.who) + ": plane allocation failed");
    const float4* Ld;
    const uint32_t* samples;
    if ((rc = film_view(c, &Ld, &samples)) || (rc = span_begin(c)) || (rc = film_planes(c, r.guided, Ld, samples)) ||
        (rc = denoise_film_planes(c, r)))
        return rc;
    return (r.guided && c->vf.on) ? variance_time(c) : MCPT_OK;
}

extern "C" {

int mcpt_denoise_default_params(mcpt_denoise_params* p) {
    if (!p) return MCPT_E_INVALID;
    // the best row of profiles/denoise_defaults.txt (4 spp against 1024 spp; configs 1, 2, cube)
    p->passes = 5;
    p->sigma_color = 2.0f;
    p->sigma_normal = 0.3f;
    p->sigma_albedo = 0.3f;
    p->sigma_depth = 0.1f;
    return MCPT_OK;
}

int mcpt_guides_render(mcpt_ctx* c, uint32_t nsamples) {
    int rc = check_ready(c);
    if (rc) return rc;
    if (nsamples < 1 || nsamples >= kMaxSpp - 256) return set_err(c, MCPT_E_INVALID, "guides: nsamples must be 1 .. 2^19 - 257");
    HIPCHK(c, hipSetDevice(c->device));
    Guides& g = c->guides;
    g.ok = false;
    const size_t P = c->film.pixels();
    if (!g.alb || !g.nz) {
        c->dn = Denoise{};  // (the filter's planes go too: they are re-made on demand)
        g = Guides{};
        if (!g.alb.ensure(P) || !g.nz.ensure(P)) {
            (void)hipGetLastError();
            g = Guides{};
            return set_err(c, MCPT_E_NOMEM, "guides: buffer allocation failed");
        }
    }
    // Chunk: np pixels x ns samples of rays; per ray 2 float4 (ray), 2 float4 (hit record), 1 index
    constexpr size_t kRayBytes = 4 * sizeof(float4) + sizeof(int32_t);
    size_t budget = (size_t)64 << 20;
    if (const char* e = getenv(kGuideChunkEnv)) {
        const long long v = atoll(e);
        if (v > 0) budget = (size_t)v;
    }
    const size_t R = std::min<size_t>(std::max<size_t>(budget / kRayBytes, 1), (size_t)1 << 24);
    const uint32_t n_eff = c->cam.lens_radius > 0.f ? nsamples : 1u;  // a pinhole's samples share one ray
    const uint32_t np_max = (uint32_t)std::min<size_t>(P, R);
    const uint32_t ns_max = (uint32_t)std::min<size_t>(n_eff, std::max<size_t>(R / np_max, 1));
    const size_t nr = (size_t)np_max * ns_max;
    TmpScope tmp(c);
    float4 *ro, *rd, *hp, *hn;
    int32_t* ht;
    if ((rc = dalloc(c, tmp.L, &ro, nr)) || (rc = dalloc(c, tmp.L, &rd, nr)) || (rc = dalloc(c, tmp.L, &hp, nr)) ||
        (rc = dalloc(c, tmp.L, &hn, nr)) || (rc = dalloc(c, tmp.L, &ht, nr))) {
        (void)hipGetLastError();
        return rc;
    }
    GuideArgs ga{};
    ga.cam = c->cam;
    if ((rc = cam_table(c, c->W, c->H, &ga.cam_px, &ga.cam_dir))) return rc;
    ga.W = (int)c->W;
    ga.H = (int)c->H;
    ga.seed = c->cfg.seed;
    ga.ro = ro;
    ga.rd = rd;
    ga.hit_p = hp;
    ga.hit_n = hn;
    ga.mats = c->scene.dev.mats;
    ga.g_alb = g.alb;
    ga.g_nz = g.nz;
    const mcpt::TexView tex = c->tx.view();
    if ((rc = span_begin(c))) return rc;
    HIPCHK(c, hipMemsetAsync(g.alb, 0, P * sizeof(float4), c->stream));
    HIPCHK(c, hipMemsetAsync(g.nz, 0, P * sizeof(float4), c->stream));
    bool drained = true;
    for (size_t p0 = 0; p0 < P; p0 += np_max) {
        ga.p0 = (uint32_t)p0;
        ga.np = (uint32_t)std::min<size_t>(np_max, P - p0);
        for (uint32_t s0 = 0; s0 < n_eff; s0 += ns_max) {
            ga.s0 = s0;
            ga.ns = std::min<uint32_t>(ns_max, n_eff - s0);
            const uint32_t n = ga.np * ga.ns;
            launch_guide_rays(ga, c->stream);
            // closest hits as mcpt_stage_run(EXTEND) traces them: no occluder cache, unfiltered rays
            TraceArgs ta{};
            ta.scene = c->scene.dev;
            ta.scene.occ = nullptr;
            ta.nshards = 1;
            TraceSet& ts = ta.set[0];
            ts.ro = ro;
            ts.rd = rd;
            ts.count = n;
            ts.shard_cap = n;
            ta.hit_tri = ht;
            ta.grab = &c->cnt.dev->grab[0][0];
            ta.tiny_stack = c->tiny_stack ? 1 : 0;
            launch_trace(ta, c->geom, c->stream);
            HIPCHK(c, hipMemcpyAsync(&c->cnt.host->grab[0][0], &c->cnt.dev->grab[0][0], sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipMemsetAsync(c->cnt.dev->grab, 0, sizeof(c->cnt.dev->grab), c->stream));  // hand-out counters back to 0
            if (tex.uv) {  // textures in effect (section 19): the albedo is the shaded base colour at the hit
                // (a normal-mapped set, section 21: and the normal guide is the mapped normal)
                // (an sRGB-flagged base colour, section 22: and the albedo is the decoded colour)
                if (c->tx.level() == 4) launch_guide_accum_srgb(GuideTexArgs{ga, c->scene.dev, tex, ht}, c->stream);
                else if (c->tx.level() == 3) launch_guide_accum_nrm(GuideTexArgs{ga, c->scene.dev, tex, ht}, c->stream);
                else launch_guide_accum_tex(GuideTexArgs{ga, c->scene.dev, tex, ht}, c->stream);
            } else {
                HitRecordArgs ha{c->scene.dev, ro, rd, ht, hp, hn, ht, n};
                launch_hit_record(ha, c->stream);
                launch_guide_accum(ga, c->stream);
            }
            HIPCHK(c, hipGetLastError());
            HIPCHK(c, hipStreamSynchronize(c->stream));  // the next chunk reuses the buffers (and the staging word)
            if (c->cnt.host->grab[0][0] < n) drained = false;
        }
    }
    if ((rc = span_end(c, &c->ms.guides))) return rc;
    if (!drained) return set_err(c, MCPT_E_HIP, "guides: k_trace left rays untraced");
    g.key = c->view();
    g.ok = true;
    return MCPT_OK;
}

int mcpt_guides_read(mcpt_ctx* c, float* albedo, float* normal, float* depth, uint32_t* count) {
    if (!c || !c->film.allocated) return set_err(c, MCPT_E_INVALID, "film not allocated");
    if (!guides_valid(c)) return set_err(c, MCPT_E_INVALID, "no valid guide buffers: call mcpt_guides_render first");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::vector<float> cnt(count ? c->film.pixels() : 0);  // the sample counts are kept as floats
    int rc;
    if ((rc = read_plane(c, c->guides.alb, c->film.pixels(), albedo, count ? cnt.data() : nullptr)) ||
        (rc = read_plane(c, c->guides.nz, c->film.pixels(), normal, depth)))
        return rc;
    for (size_t i = 0; i < cnt.size(); i++) count[i] = (uint32_t)cnt[i];
    return MCPT_OK;
}

int mcpt_denoise_run(mcpt_ctx* c, uint32_t w, uint32_t h, const float* rgb, const uint32_t* samples, const float* albedo,
                     const float* normal, const float* depth, const mcpt_denoise_params* pp, float* out_rgb) {
    if (!c || !rgb || !albedo || !normal || !depth || !out_rgb || !pp) return set_err(c, MCPT_E_INVALID, "denoise: null argument");
    return denoise_run(c, denoise_request(*pp), w, h, rgb, samples, nullptr, albedo, normal, depth, out_rgb, nullptr);
}

int mcpt_film_denoise(mcpt_ctx* c, const mcpt_denoise_params* pp) {
    return film_denoise(c, denoise_request(params_or(pp, mcpt_denoise_default_params)));
}

static int denoised_check(mcpt_ctx* c) {
    if (!c || !c->film.allocated) return set_err(c, MCPT_E_INVALID, "film not allocated");
    if (c->dn.result < 0) return set_err(c, MCPT_E_INVALID, "no denoised frame: call mcpt_film_denoise first");
    return MCPT_OK;
}

int mcpt_denoised_read(mcpt_ctx* c, float* rgb) {
    int rc = denoised_check(c);
    if (rc) return rc;
    if (!rgb) return set_err(c, MCPT_E_INVALID, "null argument");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return read_plane(c, c->dn.col[c->dn.result], c->film.pixels(), rgb, nullptr);
}

int mcpt_denoised_read_device(mcpt_ctx* c, void* d_rgb) {
    int rc = denoised_check(c);
    if (rc) return rc;
    if (!d_rgb) return set_err(c, MCPT_E_INVALID, "null argument");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(d_rgb, c->dn.col[c->dn.result], c->film.pixels() * sizeof(float4), hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MCPT_OK;
}

int mcpt_denoised_tonemap_rgba8(mcpt_ctx* c, float exposure, uint8_t* out) {
    int rc = denoised_check(c);
    if (rc) return rc;
    if (!out) return set_err(c, MCPT_E_INVALID, "null argument");
    HIPCHK(c, hipSetDevice(c->device));
    // k_tonemap over the denoised means with a sample count of 1 per pixel
    return tonemap_rgba8(c, c->dn.col[c->dn.result], nullptr, exposure, out);
}

// ---- variance-guided form ----

int mcpt_denoise_guided_default_params(mcpt_denoise_guided_params* p) {
    if (!p) return MCPT_E_INVALID;
    // sigma_lum / lum_eps: the best row of profiles/denoise_guided_defaults.txt (4 and 16 spp and an
    // adaptive frame against 1024 spp; configs 1, 2, cube).  The rest: mcpt_denoise_default_params
    p->passes = 5;
    p->sigma_lum = 8.0f;
    p->lum_eps = 0.f;
    p->sigma_color = 2.0f;
    p->sigma_normal = 0.3f;
    p->sigma_albedo = 0.3f;
    p->sigma_depth = 0.1f;
    return MCPT_OK;
}

int mcpt_denoise_guided_run(mcpt_ctx* c, uint32_t w, uint32_t h, const float* rgb, const uint32_t* samples, const float* variance,
                            const float* albedo, const float* normal, const float* depth, const mcpt_denoise_guided_params* pp,
                            float* out_rgb, float* out_variance) {
    if (!c || !rgb || !variance || !albedo || !normal || !depth || !out_rgb || !pp)
        return set_err(c, MCPT_E_INVALID, "guided denoise: null argument");
    return denoise_run(c, denoise_request(*pp), w, h, rgb, samples, variance, albedo, normal, depth, out_rgb, out_variance);
}

int mcpt_film_denoise_guided(mcpt_ctx* c, const mcpt_denoise_guided_params* pp) {
    return film_denoise(c, denoise_request(params_or(pp, mcpt_denoise_guided_default_params)));
}

int mcpt_denoised_variance_read(mcpt_ctx* c, float* var) {
    int rc = denoised_check(c);
    if (rc) return rc;
    if (!c->dn.guided) return set_err(c, MCPT_E_INVALID, "no denoised variance: the last denoise was not mcpt_film_denoise_guided");
    if (!var) return set_err(c, MCPT_E_INVALID, "null argument");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return read_x(c, c->dn.vl[c->dn.result], c->film.pixels(), var);
}

int mcpt_debug_denoise_ms(const mcpt_ctx* c, float* out10) {
    if (!c || !out10) return MCPT_E_INVALID;
    out10[0] = c->ms.guides;
    for (int i = 0; i < 9; i++) out10[1 + i] = c->ms.dn[i];
    return MCPT_OK;
}

// ---- adaptive sampling ----

// What a finished frame leaves behind that would keep raised sample counts from being picked up: the
// k_shade block done flags and the counter block's idle word (run_iterations resets the latter per
// call too).  The film, the flags words' next sample indices and the ray counters stay.
static int frame_done_reset(mcpt_ctx* c) {
    if (c->film.blk_done) HIPCHK(c, hipMemsetAsync(c->film.blk_done, 0, c->film.L.blk_done_n, c->stream));
    HIPCHK(c, hipMemsetAsync(&c->cnt.dev->idle, 0, sizeof(uint32_t), c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MCPT_OK;
}
// The film tiles' ownership for the current tile set and layout (OwnMap), uploaded
static int own_map_build(mcpt_ctx* c, OwnMap* m) {
    const uint32_t ntx = c->film.L.nx, nty = c->film.L.ny;
    std::vector<int32_t> own((size_t)ntx * nty, -1);
    for (size_t i = 0; i < c->tiles.host.size(); i++) own[(size_t)c->tiles.host[i].y * ntx + (size_t)c->tiles.host[i].x] = (int32_t)i;
    for (const int2& t : c->film.unpacked) own[(size_t)t.y * ntx + (size_t)t.x] = -1;  // another context's pixels
    if (int rc = ensure_or_nomem(c, c->ad.own_map, own.size())) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(c->ad.own_map, own.data(), own.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    *m = OwnMap{c->ad.own_map, c->compact ? 1 : 0, (int)c->tile_w, (int)c->tile_h, (int)c->W, (int)c->H};
    return MCPT_OK;
}
// k_film_error between span_begin and span_end; its device time -> ms.err
static int film_error_launch(mcpt_ctx* c, const FilmErrorArgs& a) {
    if (int rc = span_begin(c)) return rc;
    launch_film_error(a, c->stream);
    return span_end(c, &c->ms.err);
}

int mcpt_set_sample_budget(mcpt_ctx* c, const uint32_t* budget) {
    if (!c || !c->film.allocated) return set_err(c, MCPT_E_INVALID, "film not allocated");
    HIPCHK(c, hipSetDevice(c->device));
    int rc = require_idle(c, "sample budget: paths are in flight (finish the render or clear the film)");
    if (rc) return rc;
    uint32_t mx = 0;
    if (budget) {
        for (size_t i = 0; i < c->film.pixels(); i++) mx = std::max(mx, budget[i]);
        if (mx > kMaxSpp - 256) return set_err(c, MCPT_E_INVALID, "sample budget: an entry exceeds 2^19 - 256");
        if ((rc = ensure_or_nomem(c, c->ad.budget, c->film.pixels()))) return rc;
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipMemcpy(c->ad.budget, budget, c->film.pixels() * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    c->ad.budget_on = budget != nullptr;
    c->ad.budget_max = mx;
    return frame_done_reset(c);
}

int mcpt_sample_budget_read(mcpt_ctx* c, uint32_t* out) {
    if (!c || !out) return set_err(c, MCPT_E_INVALID, "null argument");
    if (!c->ad.budget_on) return set_err(c, MCPT_E_INVALID, "no sample budget installed");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(out, c->ad.budget, c->film.pixels() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return MCPT_OK;
}

int mcpt_set_spp(mcpt_ctx* c, int32_t spp) {
    if (!c) return MCPT_E_INVALID;
    if (spp < 0 || (uint32_t)spp > kMaxSpp - 256) return set_err(c, MCPT_E_INVALID, "spp must be 0..2^19-256");
    if (c->film.allocated) {
        HIPCHK(c, hipSetDevice(c->device));
        if (int rc = require_idle(c, "set_spp: paths are in flight (finish the render or clear the film)")) return rc;
    }
    c->cfg.spp = spp;
    return c->film.allocated ? frame_done_reset(c) : MCPT_OK;
}

int mcpt_film_error(mcpt_ctx* c) {
    if (!c || !c->film.allocated) return set_err(c, MCPT_E_INVALID, "film not allocated");
    if (c->slots < 2) return set_err(c, MCPT_E_INVALID, "film error: needs at least 2 path slots (mcpt_set_path_slots)");
    HIPCHK(c, hipSetDevice(c->device));
    int rc = require_idle(c, "film error: paths are in flight");
    if (rc) return rc;
    if ((rc = ensure_or_nomem(c, c->ad.err4, c->film.pixels()))) return rc;
    FilmErrorArgs a{};
    if ((rc = own_map_build(c, &a.m))) return rc;
    a.Ld = c->film.Ld;
    a.samples = c->film.samples;
    a.stride = c->film.L.npx;
    a.slots = (int)c->slots;
    a.out = c->ad.err4;
    c->ad.err_ok = false;
    if ((rc = film_error_launch(c, a))) return rc;
    c->ad.err_ok = true;
    return MCPT_OK;
}

int mcpt_film_error_read(mcpt_ctx* c, float* out4) {
    if (!c || !out4) return set_err(c, MCPT_E_INVALID, "null argument");
    if (!c->ad.err_ok) return set_err(c, MCPT_E_INVALID, "no film error estimate (call mcpt_film_error first)");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(out4, c->ad.err4, c->film.pixels() * sizeof(float4), hipMemcpyDeviceToHost));
    return MCPT_OK;
}

int mcpt_error_run(mcpt_ctx* c, uint32_t w, uint32_t h, uint32_t slots, const float* Ld_slots, const uint32_t* samples_slots,
                   float* out4) {
    if (!c || !Ld_slots || !samples_slots || !out4) return set_err(c, MCPT_E_INVALID, "error run: null argument");
    if (w == 0 || h == 0 || slots == 0 || slots > 256 || (uint64_t)w * h * slots >= (1ull << 28))
        return set_err(c, MCPT_E_INVALID, "error run: bad image size or slot count");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n = (size_t)w * h;
    std::vector<float4> L4(n * slots);
    for (size_t i = 0; i < n * slots; i++) L4[i] = make_float4(Ld_slots[3 * i], Ld_slots[3 * i + 1], Ld_slots[3 * i + 2], 0.f);
    TmpScope tmp(c);
    float4 *d_L, *d_out;
    uint32_t* d_s;
    int rc;
    if ((rc = dupload(c, tmp.L, &d_L, L4.data(), n * slots)) || (rc = dupload(c, tmp.L, &d_s, samples_slots, n * slots)) ||
        (rc = dalloc(c, tmp.L, &d_out, n)))
        return rc;
    FilmErrorArgs a{};
    a.m = OwnMap{nullptr, 0, (int)w, (int)h, (int)w, (int)h};
    a.Ld = d_L;
    a.samples = d_s;
    a.stride = n;
    a.slots = (int)slots;
    a.out = d_out;
    if ((rc = film_error_launch(c, a))) return rc;
    HIPCHK(c, hipMemcpy(out4, d_out, n * sizeof(float4), hipMemcpyDeviceToHost));
    return MCPT_OK;
}

int mcpt_debug_film_read_slot(mcpt_ctx* c, uint32_t slot, float* Ld, uint32_t* samples) {
    if (!c || !c->film.allocated) return set_err(c, MCPT_E_INVALID, "film not allocated");
    if (slot >= c->slots) return set_err(c, MCPT_E_INVALID, "slot out of range");
    HIPCHK(c, hipSetDevice(c->device));
    SlotImageArgs a{};
    int rc = own_map_build(c, &a.m);
    if (rc) return rc;
    TmpScope tmp(c);
    if ((rc = dalloc(c, tmp.L, &a.out_Ld, c->film.pixels())) || (rc = dalloc(c, tmp.L, &a.out_samples, c->film.pixels()))) return rc;
    a.Ld = c->film.Ld + (size_t)slot * c->film.L.npx;
    a.samples = c->film.samples + (size_t)slot * c->film.L.npx;
    launch_slot_image(a, c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (Ld && (rc = read_plane(c, a.out_Ld, c->film.pixels(), Ld, nullptr))) return rc;
    if (samples) HIPCHK(c, hipMemcpy(samples, a.out_samples, c->film.pixels() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return MCPT_OK;
}

int mcpt_sample_budget_default_params(mcpt_sample_budget_params* p) {
    if (!p) return MCPT_E_INVALID;
    // target_rel_err: see DESIGN.md section 11 for the rows it was chosen from
    p->target_rel_err = 0.05f;
    p->lum_floor = 0.01f;
    p->min_spp = 32;
    p->max_spp = 256;
    return MCPT_OK;
}

int mcpt_budget_from_error(mcpt_ctx* c, const mcpt_sample_budget_params* pp, uint64_t* out3) {
    if (!c || !c->film.allocated) return set_err(c, MCPT_E_INVALID, "film not allocated");
    const mcpt_sample_budget_params p = params_or(pp, mcpt_sample_budget_default_params);
    if (!finite_nonneg(p.target_rel_err) || !(p.target_rel_err > 0.f) || !finite_nonneg(p.lum_floor) || p.min_spp > p.max_spp ||
        p.max_spp > kMaxSpp - 256)
        return set_err(c, MCPT_E_INVALID, "budget: bad parameters (target_rel_err > 0, lum_floor >= 0, min_spp <= max_spp <= 2^19-256)");
    Adaptive& ad = c->ad;
    if (!ad.err_ok) return set_err(c, MCPT_E_INVALID, "budget: no film error estimate (call mcpt_film_error first)");
    HIPCHK(c, hipSetDevice(c->device));
    int rc = require_idle(c, "budget: paths are in flight");
    if (rc) return rc;
    if ((rc = ensure_or_nomem(c, ad.budget, c->film.pixels())) || (rc = ensure_or_nomem(c, ad.bud_cnt, 4))) return rc;
    BudgetArgs a{};
    if ((rc = own_map_build(c, &a.m))) return rc;
    a.err = ad.err4;
    a.p = mcpt::BudgetParams{p.target_rel_err, p.lum_floor, p.min_spp, p.max_spp};
    a.budget = ad.budget;
    a.cnt = ad.bud_cnt;
    HIPCHK(c, hipMemsetAsync(ad.bud_cnt, 0, 4 * sizeof(unsigned long long), c->stream));
    if ((rc = span_begin(c))) return rc;
    launch_budget(a, c->stream);
    if ((rc = span_end(c, &c->ms.budget))) return rc;
    unsigned long long cnt[4] = {};
    HIPCHK(c, hipMemcpy(cnt, ad.bud_cnt, sizeof(cnt), hipMemcpyDeviceToHost));
    // (an entry past a pixel's n > max_spp is that n: still a count the film holds, below 2^19)
    ad.budget_on = true;
    ad.budget_max = (uint32_t)cnt[1];
    if (out3) { out3[0] = cnt[0]; out3[1] = cnt[1]; out3[2] = cnt[2]; }
    return frame_done_reset(c);
}

int64_t mcpt_debug_adaptive_bytes(const mcpt_ctx* c) { return c ? (int64_t)c->ad.bytes() : (int64_t)MCPT_E_INVALID; }

int mcpt_debug_adaptive_ms(const mcpt_ctx* c, float* out2) {
    if (!c || !out2) return MCPT_E_INVALID;
    out2[0] = c->ms.err;
    out2[1] = c->ms.budget;
    return MCPT_OK;
}

// ---- temporal accumulation ----

int mcpt_set_seed(mcpt_ctx* c, uint64_t seed) {
    if (!c) return MCPT_E_INVALID;
    if (c->film.allocated) {
        HIPCHK(c, hipSetDevice(c->device));
        if (int rc = require_idle(c, "set_seed: paths are in flight (finish the render or clear the film)")) return rc;
    }
    c->cfg.seed = seed;  // (guides_valid compares it: the guides are stale from here on)
    return c->film.allocated ? mcpt_film_clear(c) : MCPT_OK;
}

int mcpt_camera_view_proj(const mcpt_camera* cam, float* out16) {
    if (!cam || !out16) return MCPT_E_INVALID;
    mcpt::tp_view_proj(cam->inv_view_proj, out16);
    return MCPT_OK;
}

int mcpt_temporal_default_params(mcpt_temporal_params* p) {
    if (!p) return MCPT_E_INVALID;
    // the best row of profiles/temporal_defaults.txt (8 frames of 2 spp against 1024 spp; configs 1, 2, cube).
    // With 2-spp frames max_history 8 bounds alpha at 0.2 from below, SVGF's value; the rows that reach
    // that bound through alpha_min tie with it exactly.
    p->pos_tol = 0.1f;
    p->nrm_tol = 1.0f;
    p->max_history = 8.f;
    p->alpha_min = 0.f;
    return MCPT_OK;
}

static int temporal_check_params(mcpt_ctx* c, const mcpt_temporal_params& p) {
    if (!finite_nonneg(p.pos_tol)) return set_err(c, MCPT_E_INVALID, "temporal: pos_tol must be a finite number >= 0");
    if (!finite_nonneg(p.nrm_tol)) return set_err(c, MCPT_E_INVALID, "temporal: nrm_tol must be a finite number >= 0");
    if (!finite_nonneg(p.max_history)) return set_err(c, MCPT_E_INVALID, "temporal: max_history must be a finite number >= 0");
    if (!finite_nonneg(p.alpha_min) || p.alpha_min > 1.f) return set_err(c, MCPT_E_INVALID, "temporal: alpha_min must be in [0, 1]");
    return MCPT_OK;
}
static mcpt::TemporalParams temporal_params(const mcpt_temporal_params& p) {
    return mcpt::TemporalParams{p.pos_tol, p.nrm_tol, p.max_history, p.alpha_min};
}
// k_temporal between span_begin and span_end; its device time -> ms.tp
static int temporal_launch(mcpt_ctx* c, const TemporalArgs& a) {
    if (int rc = span_begin(c)) return rc;
    launch_temporal(a, c->stream);
    return span_end(c, &c->ms.tp);
}

int mcpt_film_temporal(mcpt_ctx* c, const mcpt_temporal_params* pp) {
    if (!c || !c->film.allocated) return set_err(c, MCPT_E_INVALID, "film not allocated");
    const mcpt_temporal_params p = params_or(pp, mcpt_temporal_default_params);
    int rc = temporal_check_params(c, p);
    if (rc) return rc;
    if (!guides_valid(c))
        return set_err(c, MCPT_E_INVALID, "temporal: guide buffers missing or stale (camera, scene, seed or film changed): call mcpt_guides_render first");
    HIPCHK(c, hipSetDevice(c->device));
    if ((rc = require_idle(c, "temporal: paths are in flight"))) return rc;
    if (c->slots >= 2 && (rc = mcpt_film_error(c))) return rc;
    Temporal& t = c->tp;
    bool ok = t.col.ensure(c->film.pixels()) && t.vl.ensure(c->film.pixels());
    for (auto& set : t.h)
        for (auto& plane : set) ok = ok && plane.ensure(c->film.pixels());
    if (!ok) {
        (void)hipGetLastError();
        t = Temporal{};
        return set_err(c, MCPT_E_NOMEM, "temporal: plane allocation failed");
    }
    // the variance fill forms v_c in the filter's planes (which forgets the last denoised frame)
    const bool fill = c->vf.on;
    if (fill && !denoise_planes_ensure(c, true)) return set_err(c, MCPT_E_NOMEM, "temporal: plane allocation failed");
    const int prev = t.set, next = prev ^ 1;
    if (!t.ok)  // no history: N = 0 everywhere, and every tap is rejected
        for (int k = 0; k < 3; k++) HIPCHK(c, hipMemsetAsync(t.h[prev][k], 0, c->film.pixels() * sizeof(float4), c->stream));
    TemporalArgs a{};
    a.W = (int)c->W;
    a.H = (int)c->H;
    a.k = temporal_params(p);
    mcpt::tp_view_proj(t.ok ? t.key.cam.ivp : c->cam.ivp, a.vp_prev);
    if ((rc = film_view(c, &a.Ld, &a.samples))) return rc;
    a.err = c->slots >= 2 ? c->ad.err4.get() : nullptr;
    a.g_alb = c->guides.alb;
    a.g_nz = c->guides.nz;
    if ((rc = cam_table(c, c->W, c->H, &a.cam_px, &a.cam_dir))) return rc;
    a.cam = c->cam;
    a.hcol = t.h[prev][0];
    a.hpos = t.h[prev][1];
    a.hnrm = t.h[prev][2];
    a.col = t.col;
    a.vl = t.vl;
    a.out_hcol = t.h[next][0];
    a.out_hpos = t.h[next][1];
    a.out_hnrm = t.h[next][2];
    t.ok = false;
    if (fill) {
        if ((rc = film_planes(c, true, a.Ld, a.samples))) return rc;
        a.vfill = c->dn.vl[0];
    }
    if ((rc = temporal_launch(c, a))) return rc;
    t.set = next;
    t.key = c->view();
    t.ok = true;
    return fill ? variance_time(c) : MCPT_OK;
}

int mcpt_temporal_reset(mcpt_ctx* c) {
    if (!c) return MCPT_E_INVALID;
    c->tp.ok = false;
    return MCPT_OK;
}

int mcpt_temporal_read(mcpt_ctx* c, float* rgb, float* nsamples, float* variance, float* position) {
    if (!c || !c->film.allocated) return set_err(c, MCPT_E_INVALID, "film not allocated");
    if (!c->tp.ok) return set_err(c, MCPT_E_INVALID, "no accumulated frame: call mcpt_film_temporal first");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const auto& h = c->tp.h[c->tp.set];
    if (int rc = read_plane(c, h[0], c->film.pixels(), rgb, nsamples)) return rc;
    return read_plane(c, h[1], c->film.pixels(), position, variance);
}

int mcpt_temporal_denoise(mcpt_ctx* c, const mcpt_denoise_guided_params* pp) {
    if (!c || !c->film.allocated) return set_err(c, MCPT_E_INVALID, "film not allocated");
    const DenoiseRequest r = denoise_request(params_or(pp, mcpt_denoise_guided_default_params));
    int rc = denoise_check_params(c, r);
    if (rc) return rc;
    if (!c->tp.ok) return set_err(c, MCPT_E_INVALID, "temporal denoise: no accumulated frame: call mcpt_film_temporal first");
    if (!guides_valid(c) || !c->tp.key.same(c->view(), ViewKey::CAM))
        return set_err(c, MCPT_E_INVALID, "temporal denoise: the camera, scene or seed changed since the frame was accumulated: call mcpt_guides_render and mcpt_film_temporal first");
    HIPCHK(c, hipSetDevice(c->device));
    if (!denoise_planes_ensure(c, true)) return set_err(c, MCPT_E_NOMEM, "temporal denoise: plane allocation failed");
    const TemporalPrepArgs pa{c->tp.col, c->tp.vl, c->guides.alb, c->guides.nz, c->dn.col[0], c->dn.gd, c->dn.al, c->dn.vl[0], (uint32_t)c->film.pixels()};
    if ((rc = span_begin(c))) return rc;
    launch_temporal_prep(pa, c->stream);
    return denoise_film_planes(c, r);
}

int mcpt_temporal_run(mcpt_ctx* c, uint32_t w, uint32_t h, const float* rgb, const uint32_t* samples, const float* variance,
                      const float* position, const float* normal, const float* depth, const float* hcol, const float* hpos,
                      const float* hnrm, const float* vp_prev16, const mcpt_temporal_params* pp, float* out_col, float* out_vl,
                      float* out_hcol, float* out_hpos, float* out_hnrm) {
    if (!c || !rgb || !samples || !variance || !position || !normal || !depth || !hcol || !hpos || !hnrm || !vp_prev16 || !pp ||
        !out_col || !out_vl || !out_hcol || !out_hpos || !out_hnrm)
        return set_err(c, MCPT_E_INVALID, "temporal: null argument");
    if (w == 0 || h == 0 || (uint64_t)w * h >= (1ull << 28)) return set_err(c, MCPT_E_INVALID, "temporal: bad image size");
    int rc = temporal_check_params(c, *pp);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n = (size_t)w * h;
    TmpScope tmp(c);
    auto& L = tmp.L;
    float *d_rgb, *d_v, *d_x, *d_n, *d_z, *d_hc, *d_hp, *d_hn;
    uint32_t* d_s;
    float4 *o_col, *o_hc, *o_hp, *o_hn;
    float2* o_vl;
    if ((rc = dupload(c, L, &d_rgb, rgb, 3 * n)) || (rc = dupload(c, L, &d_s, samples, n)) || (rc = dupload(c, L, &d_v, variance, n)) ||
        (rc = dupload(c, L, &d_x, position, 3 * n)) || (rc = dupload(c, L, &d_n, normal, 3 * n)) ||
        (rc = dupload(c, L, &d_z, depth, n)) || (rc = dupload(c, L, &d_hc, hcol, 4 * n)) || (rc = dupload(c, L, &d_hp, hpos, 4 * n)) ||
        (rc = dupload(c, L, &d_hn, hnrm, 4 * n)) || (rc = dalloc(c, L, &o_col, n)) || (rc = dalloc(c, L, &o_vl, n)) ||
        (rc = dalloc(c, L, &o_hc, n)) || (rc = dalloc(c, L, &o_hp, n)) || (rc = dalloc(c, L, &o_hn, n)))
        return rc;
    TemporalArgs a{};
    a.W = (int)w;
    a.H = (int)h;
    a.k = temporal_params(*pp);
    memcpy(a.vp_prev, vp_prev16, sizeof(a.vp_prev));
    a.samples = d_s;
    a.rgb = d_rgb;
    a.variance = d_v;
    a.position = d_x;
    a.normal = d_n;
    a.depth = d_z;
    a.hcol = (const float4*)d_hc;
    a.hpos = (const float4*)d_hp;
    a.hnrm = (const float4*)d_hn;
    a.col = o_col;
    a.vl = o_vl;
    a.out_hcol = o_hc;
    a.out_hpos = o_hp;
    a.out_hnrm = o_hn;
    if ((rc = temporal_launch(c, a))) return rc;
    HIPCHK(c, hipMemcpy(out_col, o_col, n * sizeof(float4), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(out_vl, o_vl, n * sizeof(float2), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(out_hcol, o_hc, n * sizeof(float4), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(out_hpos, o_hp, n * sizeof(float4), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(out_hnrm, o_hn, n * sizeof(float4), hipMemcpyDeviceToHost));
    return MCPT_OK;
}

int64_t mcpt_debug_temporal_bytes(const mcpt_ctx* c) { return c ? (int64_t)c->tp.bytes() : (int64_t)MCPT_E_INVALID; }

int mcpt_debug_temporal_ms(const mcpt_ctx* c, float* out1) {
    if (!c || !out1) return MCPT_E_INVALID;
    out1[0] = c->ms.tp;
    return MCPT_OK;
}

// ---- spatial variance estimate ----

int mcpt_variance_default_params(mcpt_variance_params* p) {
    if (!p) return MCPT_E_INVALID;
    // radius / min_neff: the best row of profiles/variance_defaults.txt (one-slot frames of 2 .. 16 spp
    // against 1024 spp; configs 1, 2, cube).  The guide sigmas: mcpt_denoise_default_params
    p->radius = 1;
    p->sigma_normal = 0.3f;
    p->sigma_albedo = 0.3f;
    p->sigma_depth = 0.1f;
    p->min_neff = 4.f;
    return MCPT_OK;
}

int mcpt_variance_run(mcpt_ctx* c, uint32_t w, uint32_t h, const float* rgb, const uint32_t* samples, const float* variance,
                      const float* albedo, const float* normal, const float* depth, const mcpt_variance_params* pp,
                      float* out_variance) {
    if (!c || !rgb || !albedo || !normal || !depth || !pp || !out_variance) return set_err(c, MCPT_E_INVALID, "variance: null argument");
    if (w == 0 || h == 0 || (uint64_t)w * h >= (1ull << 28)) return set_err(c, MCPT_E_INVALID, "variance: bad image size");
    int rc = variance_check_params(c, *pp);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n = (size_t)w * h;
    TmpScope tmp(c);
    auto& L = tmp.L;
    DenoiseGuidedPrepArgs pa{};
    float *d_rgb, *d_al, *d_n, *d_z, *d_v = nullptr;
    uint32_t* d_s = nullptr;
    if ((rc = dupload(c, L, &d_rgb, rgb, 3 * n)) || (rc = dupload(c, L, &d_al, albedo, 3 * n)) ||
        (rc = dupload(c, L, &d_n, normal, 3 * n)) || (rc = dupload(c, L, &d_z, depth, n)) ||
        (samples && (rc = dupload(c, L, &d_s, samples, n))) || (variance && (rc = dupload(c, L, &d_v, variance, n))) ||
        (rc = dalloc(c, L, &pa.col, n)) || (rc = dalloc(c, L, &pa.gd, n)) || (rc = dalloc(c, L, &pa.al, n)) ||
        (rc = dalloc(c, L, &pa.vl, n)))
        return rc;
    pa.samples = d_s;
    pa.rgb = d_rgb;
    pa.normal = d_n;
    pa.albedo = d_al;
    pa.depth = d_z;
    pa.variance = d_v;
    pa.n = (uint32_t)n;
    launch_denoise_prep(pa, c->stream);
    if ((rc = variance_launch(c, *pp, w, h, pa.col, pa.gd, pa.al, pa.vl))) return rc;
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if ((rc = variance_time(c))) return rc;
    return read_x(c, pa.vl, n, out_variance);
}

int mcpt_set_variance_fill(mcpt_ctx* c, const mcpt_variance_params* p) {
    if (!c) return MCPT_E_INVALID;
    if (p)
        if (int rc = variance_check_params(c, *p)) return rc;
    c->vf.on = p != nullptr;
    if (p) c->vf.p = *p;
    return MCPT_OK;
}

int mcpt_debug_variance_ms(const mcpt_ctx* c, float* out1) {
    if (!c || !out1) return MCPT_E_INVALID;
    out1[0] = c->ms.var;
    return MCPT_OK;
}

}  // extern "C"
