// mcpt_render.cpp -- the reference's render loop written against the C ABI only
// (what a maintainer's PathTracer::render_image + RenderingContext "Save" become,
// INTEGRATION.md): build a BASELINE config scene with the host builder, upload it,
// run the wavefront iterations until every pixel has its samples, write PNG + PFM.
//
//   mcpt_render <config 1-5> [spp] [out_prefix] [--gpu-bvh] [--reference-bvh] [--fixed] [--tiles-per-call] [--slots S] [--denoise [guide_samples]] [--denoise-guided [guide_samples]] [--adaptive <target> <min> <max> [rounds]] [--temporal <frames> <yaw_step_deg>] [--variance-fill] [--animate <frames> <amplitude>] [--emissive <mat> <r> <g> <b>]... [--env-color <r> <g> <b>] [--sample-emitters] [--emitter-mis] [--checker <mat> <n>]... [--checker-mr <mat> <n>]... [--bumps <mat> <n> <scale>]... [--glb <file>]
//
// --denoise renders the first-hit guide buffers (default 4 guide samples per pixel), filters the film
// with the default parameters and writes <out_prefix>_denoised.png beside the raw image.
// --denoise-guided does the same with the variance-guided filter and writes
// <out_prefix>_denoised_guided.png; its variance comes from the path slots, so it needs --slots >= 2
// (4 if --slots is not given).  It combines with --denoise and with --adaptive.
// --adaptive renders every pixel to <min> samples, then [rounds] (default 2) times estimates the
// film's error from the path slots, builds per-pixel budgets that aim at the relative standard error
// <target> within [<min>, <max>] and renders on; it needs --slots >= 2 (8 if
// --slots is not given) and replaces [spp].  It combines with --denoise.
// --temporal renders <frames> frames at [spp] while the camera yaws by <yaw_step_deg> per frame, gives
// every frame its own seed, accumulates each into the temporal history and filters it (DESIGN.md section
// 13); it writes the last frame's <out_prefix>_temporal.png beside that frame's single-frame
// <out_prefix>_denoised.png.  It uses 2 path slots if --slots is not given (the variance).
// --variance-fill turns the spatial variance estimate on (at its defaults): the
// variances the path slots do not give are estimated from the frame, so --denoise-guided and --temporal
// work with --slots 1, which is what they then use if --slots is not given.
// --animate renders <frames> frames at [spp] of the config's mesh under a deterministic sinusoidal warp
// (a wave along y of <amplitude> times the scene's extent that travels with the frame number): before
// every frame the moved vertices go to mcpt_scene_update_geometry, which refits the tree on the device
// (DESIGN.md section 15), and the frame is rendered; the last frame is the one written.  It combines with
// --temporal (the longer of the two frame counts; an update drops the temporal history, there being no
// motion vectors for moved geometry) and with --denoise / --denoise-guided (the last frame); not with
// --tiles-per-call or --adaptive (rejected).
// --emissive makes material <mat> of the config's scene emit the radiance <r> <g> <b> (DESIGN.md section
// 16; repeatable; the ids are the scene's materials in the order its meshes were added: in config 2 the
// back wall, floor, ceiling, left and right wall are 0..4 and the spheres 5..9).  --env-color replaces the
// config's environment map with a constant colour: `mcpt_render 2 64 --emissive 2 8 8 8 --env-color 0 0 0`
// is a Cornell box lit by its ceiling alone.  Emitters are not sampled as lights, so small ones are noisy,
// unless --sample-emitters turns emitter sampling on: every vertex then draws a
// point on an emissive triangle and traces a shadow ray to it (`mcpt_render 2 64 --emissive 7 40 40 40
// --env-color 0 0 0 --sample-emitters` is the box lit by one small sphere).  --emitter-mis implies
// --sample-emitters and weights the emitter sample against collected emission (multiple importance
// sampling): the choice for emitters that touch other surfaces, as that sphere does.
// --checker puts an <n> x <n> two-colour procedural checker (16 x 16 texels per square, so the bilinear
// filter softens only the squares' edges) on material <mat> as its base-colour texture (DESIGN.md section
// 19; repeatable), over the uvs the mesh came with: `mcpt_render 1 64 --checker 0 8` is config 1's mesh
// (Cube.glb, each face a quarter of the uv square wide) with 2 x 2 squares per face.
// --bumps puts an <n> x <n> grid of procedural dimples (16 x 16 texels each) on material <mat> as its
// tangent-space normal map with the given scale (repeatable), with the built scene's
// tangents: `mcpt_render 2 64 --bumps 0 8 1.0` is config 2 with a dimpled wall.
// --checker-mr puts the same checker on material <mat> as its metallic-roughness texture (DESIGN.md section
// 20; repeatable) and sets the material's metallic factor to 1: the squares alternate G = B = 255 (rough
// metal: the material's own roughness) with G = 26, B = 255 (roughness a tenth of it: near-mirror metal).
// --glb <file> renders a glb as authored in place of the config's meshes, under the config's
// camera and environment: its PBR factors, its embedded PNG base-colour (sRGB), metallic-roughness and normal
// textures and its tangents; the meshes are scaled and centred into the unit sphere at the origin, and the report
// of what could not be honoured goes to stderr.
// --tiles-per-call uses the reference orchestration (one 256x256 tile per call,
// wavefront_kernels.cu:377-442 + Film::update_tile_position) instead of batch mode.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "mcpt.h"

struct Cfg { int w, h, spp, depth; float pos[3], pitch; const char* env; };

// --animate: the desc's vertices under a wave along y, amp x the scene's largest extent high, whose
// phase advances one turn over `frames` frames; a function of the position, so shared vertices stay shared
static void warp(const mcpt_scene_desc& d, float amp, uint32_t frame, uint32_t frames, std::vector<float> out[3]) {
    float ext = 0.f;
    for (int k = 0; k < 3 && d.nnodes > 0; k++) ext = fmaxf(ext, d.bmax[k] - d.bmin[k]);
    if (!(ext > 0.f)) ext = 1.f;
    const float ph = 6.2831853f * (float)frame / (float)frames, kx = 9.f / ext;
    const float* in[3] = {d.v0, d.v1, d.v2};
    for (int a = 0; a < 3; a++) {
        out[a].assign(in[a], in[a] + 3 * (size_t)d.ntri);
        for (size_t t = 0; t < (size_t)d.ntri; t++)
            out[a][3 * t + 1] += amp * ext * sinf(ph + kx * (out[a][3 * t] + out[a][3 * t + 2]));
    }
}

int main(int argc, char** argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: %s <config 1-5> [spp] [out_prefix] [--gpu-bvh] [--reference-bvh] [--fixed] [--tiles-per-call] [--slots S] [--denoise [guide_samples]] [--denoise-guided [guide_samples]] [--adaptive <target> <min> <max> [rounds]] [--temporal <frames> <yaw_step_deg>] [--variance-fill] [--animate <frames> <amplitude>] [--emissive <mat> <r> <g> <b>]... [--env-color <r> <g> <b>] [--sample-emitters] [--emitter-mis] [--checker <mat> <n>]... [--checker-mr <mat> <n>]... [--bumps <mat> <n> <scale>]... [--glb <file>]\n", argv[0]);
        return 2;
    }
    const Cfg cfgs[6] = {{0, 0, 0, 0, {0, 0, 0}, 0, ""},
                         {256, 256, 16, 3, {0.f, 0.f, 4.f}, 0.f, "HDR_029_Sky_Cloudy_Env.hdr"},
                         {1920, 1080, 256, 5, {0.f, 0.f, 3.5f}, 0.f, "night_free_Env.hdr"},
                         {1920, 1080, 256, 5, {0.f, 1.5f, 4.5f}, -10.f, "night_free_Env.hdr"},
                         {3840, 2160, 1024, 8, {0.f, 0.f, 2.5f}, 0.f, "HDR_029_Sky_Cloudy_Env.hdr"},
                         {4096, 4096, 4096, 12, {0.f, 1.2f, 3.f}, -5.f, "night_free_Env.hdr"}};
    const int id = atoi(argv[1]);
    if (id < 1 || id > 5) { fprintf(stderr, "config must be 1..5\n"); return 2; }
    Cfg c = cfgs[id];
    if (argc > 2 && argv[2][0] != '-') c.spp = atoi(argv[2]);
    std::string out = (argc > 3 && argv[3][0] != '-') ? argv[3] : "mcpt_render";
    bool gpu_bvh = false, ref_bvh = false, fixed = false, per_tile = false;
    uint32_t slots = 1, guide_samples = 0, guided_samples = 0;  // guide_samples / guided_samples > 0: denoise [guided]
    bool adaptive = false, slots_given = false, variance_fill = false, sample_emitters = false, emitter_mis = false;
    mcpt_sample_budget_params ap;
    mcpt_sample_budget_default_params(&ap);
    uint32_t rounds = 2;
    uint32_t t_frames = 0;  // > 0: --temporal
    float t_yaw = 0.f;
    uint32_t a_frames = 0;  // > 0: --animate
    float a_amp = 0.f;
    std::vector<float> emissive;  // --emissive: {mat, r, g, b} per use
    std::vector<int> checker;     // --checker: {mat, n} per use
    std::vector<int> checker_mr;  // --checker-mr: {mat, n} per use
    std::vector<float> bumps;     // --bumps: {mat, n, scale} per use
    std::string glb;              // --glb: the file rendered in place of the config's meshes
    float env_rgb[3] = {0.f, 0.f, 0.f};
    bool env_given = false;
    for (int i = 2; i < argc; i++) {
        if (!strcmp(argv[i], "--animate")) {
            if (i + 2 >= argc || atoi(argv[i + 1]) < 1) { fprintf(stderr, "--animate needs <frames> <amplitude>\n"); return 2; }
            a_frames = (uint32_t)atoi(argv[++i]);
            a_amp = (float)atof(argv[++i]);
            continue;
        }
        if (!strcmp(argv[i], "--emissive")) {
            if (i + 4 >= argc) { fprintf(stderr, "--emissive needs <mat> <r> <g> <b>\n"); return 2; }
            for (int k = 0; k < 4; k++) emissive.push_back((float)atof(argv[++i]));
            continue;
        }
        if (!strcmp(argv[i], "--checker")) {
            if (i + 2 >= argc || atoi(argv[i + 1]) < 0 || atoi(argv[i + 2]) < 1 || atoi(argv[i + 2]) > 1024) {
                fprintf(stderr, "--checker needs <mat> <n> (n in 1..1024)\n");
                return 2;
            }
            checker.push_back(atoi(argv[++i]));
            checker.push_back(atoi(argv[++i]));
            continue;
        }
        if (!strcmp(argv[i], "--bumps")) {
            if (i + 3 >= argc || atoi(argv[i + 1]) < 0 || atoi(argv[i + 2]) < 1 || atoi(argv[i + 2]) > 1024) {
                fprintf(stderr, "--bumps needs <mat> <n> <scale> (n in 1..1024)\n");
                return 2;
            }
            bumps.push_back((float)atoi(argv[++i]));
            bumps.push_back((float)atoi(argv[++i]));
            bumps.push_back((float)atof(argv[++i]));
            continue;
        }
        if (!strcmp(argv[i], "--checker-mr")) {
            if (i + 2 >= argc || atoi(argv[i + 1]) < 0 || atoi(argv[i + 2]) < 1 || atoi(argv[i + 2]) > 1024) {
                fprintf(stderr, "--checker-mr needs <mat> <n> (n in 1..1024)\n");
                return 2;
            }
            checker_mr.push_back(atoi(argv[++i]));
            checker_mr.push_back(atoi(argv[++i]));
            continue;
        }
        if (!strcmp(argv[i], "--glb")) {
            if (i + 1 >= argc) { fprintf(stderr, "--glb needs <file>\n"); return 2; }
            glb = argv[++i];
            continue;
        }
        if (!strcmp(argv[i], "--env-color")) {
            if (i + 3 >= argc) { fprintf(stderr, "--env-color needs <r> <g> <b>\n"); return 2; }
            for (int k = 0; k < 3; k++) env_rgb[k] = (float)atof(argv[++i]);
            env_given = true;
            continue;
        }
        if (!strcmp(argv[i], "--temporal")) {
            if (i + 2 >= argc || atoi(argv[i + 1]) < 1) { fprintf(stderr, "--temporal needs <frames> <yaw_step_deg>\n"); return 2; }
            t_frames = (uint32_t)atoi(argv[++i]);
            t_yaw = (float)atof(argv[++i]);
        }
        if (!strcmp(argv[i], "--gpu-bvh")) gpu_bvh = true;
        if (!strcmp(argv[i], "--reference-bvh")) ref_bvh = true;
        if (!strcmp(argv[i], "--fixed")) fixed = true;
        if (!strcmp(argv[i], "--variance-fill")) variance_fill = true;
        if (!strcmp(argv[i], "--sample-emitters")) sample_emitters = true;
        if (!strcmp(argv[i], "--emitter-mis")) sample_emitters = emitter_mis = true;
        if (!strcmp(argv[i], "--tiles-per-call")) per_tile = true;
        if (!strcmp(argv[i], "--slots") && i + 1 < argc) { slots = (uint32_t)atoi(argv[++i]); slots_given = true; }
        if (!strcmp(argv[i], "--adaptive")) {
            if (i + 3 >= argc) { fprintf(stderr, "--adaptive needs <target> <min> <max>\n"); return 2; }
            adaptive = true;
            ap.target_rel_err = (float)atof(argv[++i]);
            ap.min_spp = (uint32_t)atoi(argv[++i]);
            ap.max_spp = (uint32_t)atoi(argv[++i]);
            if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') rounds = (uint32_t)atoi(argv[++i]);
        }
        if (!strcmp(argv[i], "--denoise")) {
            guide_samples = 4;
            if (i + 1 < argc && argv[i + 1][0] >= '1' && argv[i + 1][0] <= '9') guide_samples = (uint32_t)atoi(argv[++i]);
        }
        if (!strcmp(argv[i], "--denoise-guided")) {
            guided_samples = 4;
            if (i + 1 < argc && argv[i + 1][0] >= '1' && argv[i + 1][0] <= '9') guided_samples = (uint32_t)atoi(argv[++i]);
        }
    }
    // the variance is the spread of the path slots' means, or with --variance-fill the frame's own estimate
    if (guided_samples && !slots_given && !variance_fill) slots = 4;
    if (t_frames && !slots_given && !variance_fill) slots = 2;
    if (adaptive && !slots_given) slots = 8;  // the estimate is the spread of the path slots' means
    if (adaptive) c.spp = (int)ap.min_spp;    // the first pass
    if (a_frames && (per_tile || adaptive)) { fprintf(stderr, "--animate does not combine with --tiles-per-call or --adaptive\n"); return 2; }
    const char* assets = getenv("MCPT_ASSETS") ? getenv("MCPT_ASSETS") : "assets";

    // Scene::load + BVHAccel + EnvironmentLight (host builder)
    mcpt_scene* s = mcpt_scene_new();
    // host BVH: binned 3-axis SAH (default) or BVHAccel's builder; films are identical either way
    mcpt_bvh_params bp = {MCPT_BVH_SAH3, 8, 128, 0.5f, 1.0f};
    int src = !s;
    if (!src && glb.empty()) {
        src = mcpt_scene_make_proxy(s, id, assets);
    } else if (!src) {
        // --glb: the file's meshes in place of the config's, as authored, under the config's environment map; scaled
        // uniformly and centred into the unit sphere at the origin through the loader's transform (the bounds come
        // from a first load without flags), so the config's camera frames them
        mcpt_scene* probe = mcpt_scene_new();
        mcpt_scene_desc pd;
        src = !probe || mcpt_scene_load_glb(probe, glb.c_str(), nullptr) || mcpt_scene_build(probe, 8) || mcpt_scene_get_desc(probe, &pd);
        float xf[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
        if (!src && pd.nnodes > 0) {
            float r2 = 0.f, ctr[3];
            for (int k = 0; k < 3; k++) {
                ctr[k] = 0.5f * (pd.bmin[k] + pd.bmax[k]);
                r2 += 0.25f * (pd.bmax[k] - pd.bmin[k]) * (pd.bmax[k] - pd.bmin[k]);
            }
            const float sc = r2 > 0.f ? 1.f / sqrtf(r2) : 1.f;
            xf[0] = xf[5] = xf[10] = sc;
            for (int k = 0; k < 3; k++) xf[12 + k] = -ctr[k] * sc;
        }
        if (probe) mcpt_scene_free(probe);
        if (!src) src = mcpt_scene_load_glb_ex(s, glb.c_str(), xf, MCPT_GLB_AS_AUTHORED);
        if (!src) {
            int32_t cnt[4];
            std::vector<char> lines(1 << 16);
            mcpt_scene_glb_report(s, cnt, lines.data(), (int32_t)lines.size());
            fprintf(stderr, "glb: %d images decoded, %d skipped; %d texture slots attached, %d skipped\n%s", cnt[0], cnt[1], cnt[2], cnt[3], lines.data());
            src = mcpt_scene_set_env_hdr(s, (std::string(assets) + "/" + c.env).c_str(), 1);
        }
    }
    if (!src && env_given) src = mcpt_scene_set_env_color(s, env_rgb, 1.f);
    for (size_t k = 0; !src && k < emissive.size(); k += 4) src = mcpt_scene_set_material_emission(s, (int32_t)emissive[k], &emissive[k + 1]);
    for (size_t k = 0; !src && k < checker.size(); k += 2) {  // dark / light squares, opaque
        const int sq = 16, n = checker[k + 1] * sq;  // texels per square, per side
        std::vector<uint8_t> px((size_t)n * n * 4, 255);
        for (int y = 0; y < n; y++)
            for (int x = 0; x < n; x++)
                for (int ch = 0; ch < 3; ch++) px[4 * ((size_t)y * n + x) + ch] = ((x / sq + y / sq) & 1) ? 255 : 40;
        src = mcpt_scene_set_material_texture(s, checker[k], n, n, px.data());
    }
    for (size_t k = 0; !src && k < checker_mr.size(); k += 2) {  // rough / near-mirror squares, metallic throughout
        const int sq = 16, n = checker_mr[k + 1] * sq;
        std::vector<uint8_t> px((size_t)n * n * 4, 255);
        for (int y = 0; y < n; y++)
            for (int x = 0; x < n; x++) px[4 * ((size_t)y * n + x) + 1] = ((x / sq + y / sq) & 1) ? 255 : 26;
        src = mcpt_scene_set_material_mr_texture(s, checker_mr[k], n, n, px.data());
    }
    for (size_t k = 0; !src && k < bumps.size(); k += 3) {  // n x n dimples: the normal of the height field -(1 - r^2)^2
        const int sq = 16, nb = (int)bumps[k + 1], n = nb * sq;
        std::vector<uint8_t> px((size_t)n * n * 4, 255);
        for (int y = 0; y < n; y++)
            for (int x = 0; x < n; x++) {
                const float fx = ((x % sq) + 0.5f) / sq * 2.f - 1.f, fy = ((y % sq) + 0.5f) / sq * 2.f - 1.f;
                const float r2 = fx * fx + fy * fy, g = r2 < 1.f ? 4.f * (1.f - r2) : 0.f;  // dh/dr / r of the dimple
                float nx = -g * fx * 0.5f, ny = -g * fy * 0.5f, nz = 1.f;
                const float l = sqrtf(nx * nx + ny * ny + nz * nz);
                nx /= l, ny /= l, nz /= l;
                uint8_t* q = &px[4 * ((size_t)y * n + x)];
                q[0] = (uint8_t)lrintf((nx * 0.5f + 0.5f) * 255.f);
                q[1] = (uint8_t)lrintf((ny * 0.5f + 0.5f) * 255.f);
                q[2] = (uint8_t)lrintf((nz * 0.5f + 0.5f) * 255.f);
            }
        src = mcpt_scene_set_material_normal_texture(s, (int32_t)bumps[k], n, n, px.data(), bumps[k + 2]);
    }
    if (src || (ref_bvh ? mcpt_scene_build(s, 8) : mcpt_scene_build_ex(s, &bp))) {
        fprintf(stderr, "scene: %s\n", mcpt_last_error(nullptr));
        return 1;
    }
    mcpt_scene_desc d;
    mcpt_scene_get_desc(s, &d);
    // --checker-mr: the textured materials' metallic factor is 1 (the builder's materials have 0, which
    // would scale the texture's B channel away); the desc then points at this copy of the parameters
    std::vector<float> mat_params(d.mat_params, d.mat_params + 8 * (size_t)d.nmat);
    for (size_t k = 0; k < checker_mr.size(); k += 2) mat_params[8 * (size_t)checker_mr[k] + 7] = 1.f;
    if (!checker_mr.empty()) d.mat_params = mat_params.data();
    const float* em_rgb = nullptr;  // the scene's emission table travels beside the desc
    int32_t em_nmat = 0;
    mcpt_scene_get_emission(s, &em_rgb, &em_nmat);

    // PathTracer::PathTracer
    mcpt_config cfg{0x5EED2026ull, c.spp, c.depth, 3, 256, 256, fixed ? MCPT_FLAG_FIXED : 0};
    mcpt_ctx* ctx = nullptr;
    if (mcpt_create(0, &cfg, &ctx) != MCPT_OK) {
        fprintf(stderr, "mcpt_create: %s\n", mcpt_last_error(nullptr));
        return 1;
    }
    int rc = gpu_bvh ? mcpt_scene_upload_gpu_bvh(ctx, &d) : mcpt_scene_upload(ctx, &d);
    if (!rc && em_rgb) rc = mcpt_set_material_emission(ctx, em_nmat, em_rgb);
    {  // ... and so do its textures and uvs
        const mcpt_texture* tex = nullptr;
        const int32_t *mat_tex = nullptr, *mat_mr = nullptr;
        const float *uv0 = nullptr, *uv1 = nullptr, *uv2 = nullptr;
        int32_t ntex = 0, nmat = 0, ntri = 0, nmr = 0;
        if (!rc) rc = mcpt_scene_get_textures(s, &tex, &ntex, &mat_tex, &nmat);
        if (!rc) rc = mcpt_scene_get_material_mr(s, &mat_mr, &nmr);
        if (!rc && tex && !(rc = mcpt_scene_get_uv(s, &uv0, &uv1, &uv2, &ntri))) {
            // the scene's normal maps (--bumps or a glb's) with its tangents, and its texture
            // flags (a glb's sRGB base colours; section 22), through the descriptor call; else the older call
            const uint32_t* flags = nullptr;
            const int32_t* mat_nrm = nullptr;
            const float *nrm_scale = nullptr, *t0 = nullptr, *t1 = nullptr, *t2 = nullptr;
            int32_t nf = 0, nn = 0, nt = 0;
            bool flagged = false, mapped = false;
            rc = mcpt_scene_get_texture_flags(s, &flags, &nf);
            if (!rc) rc = mcpt_scene_get_material_normal(s, &mat_nrm, &nrm_scale, &nn);
            for (int32_t k = 0; !rc && k < nf; k++) flagged = flagged || flags[k] != 0;
            for (int32_t k = 0; !rc && k < nn; k++) mapped = mapped || mat_nrm[k] >= 0;
            if (!rc && mapped) rc = mcpt_scene_get_tangents(s, &t0, &t1, &t2, &nt);
            if (!rc && !mapped && !flagged) {
                rc = mcpt_set_material_texture_maps(ctx, ntri, uv0, uv1, uv2, ntex, tex, nmat, mat_tex, mat_mr);
            } else if (!rc) {
                const mcpt_texture_set set{ntri, uv0, uv1, uv2, t0, t1, t2, ntex, tex, nmat, mat_tex, mat_mr, mapped ? mat_nrm : nullptr,
                                           mapped ? nrm_scale : nullptr, flagged ? flags : nullptr};
                rc = mcpt_set_material_texture_set(ctx, &set);
            }
        }
    }
    if (!rc && sample_emitters) rc = mcpt_set_emitter_sampling(ctx, 1);
    if (!rc && emitter_mis) rc = mcpt_set_emitter_mis(ctx, 1);
    // Camera::update
    mcpt_camera_params cp{{c.pos[0], c.pos[1], c.pos[2]}, -90.f, c.pitch, 0.785398163f, (float)c.w / (float)c.h,
                          0.01f, 1e4f, 1e-4f, 35.f};
    mcpt_camera cam;
    if (!rc) rc = mcpt_camera_make(&cp, &cam);
    if (!rc) rc = mcpt_camera_set(ctx, &cam);
    if (!rc) rc = mcpt_set_path_slots(ctx, slots);  // paths in flight per pixel (default 1)
    if (!rc) rc = mcpt_film_resize(ctx, c.w, c.h, 256, 256);
    mcpt_variance_params vp;
    if (!rc && variance_fill && !(rc = mcpt_variance_default_params(&vp))) rc = mcpt_set_variance_fill(ctx, &vp);
    if (rc) { fprintf(stderr, "setup: %s\n", mcpt_last_error(ctx)); return 1; }

    mcpt_stage_stats st{};
    if (per_tile) {  // reference orchestration: one iteration of one tile per call, tiles round-robin
        const uint32_t tx_n = (c.w + 255) / 256, ty_n = (c.h + 255) / 256;
        uint64_t rays = 0;
        double ms = 0;
        for (uint32_t round = 0; round < 1000000u && !rc; round++) {
            uint64_t round_rays = 0;
            for (uint32_t t = 0; t < tx_n * ty_n && !rc; t++) {  // Film::update_tile_position
                mcpt_stage_stats one{};
                rc = mcpt_wavefront_step(ctx, t % tx_n, t / tx_n, &one);
                round_rays += one.extend_rays + one.shadow_rays + one.vis_rays;
                ms += one.ms_total;
            }
            rays += round_rays;
            if (round_rays == 0) break;  // every pixel has its samples
        }
        st.extend_rays = rays;
        st.ms_total = (float)ms;
    } else if (a_frames && !t_frames) {  // animated geometry: move the mesh, refit, render
        std::vector<float> w[3];
        float ums[8] = {0};
        for (uint32_t f = 0; f < a_frames && !rc; f++) {
            mcpt_stage_stats one{};
            warp(d, a_amp, f, a_frames, w);
            if ((rc = mcpt_scene_update_geometry(ctx, d.ntri, w[0].data(), w[1].data(), w[2].data(), nullptr, nullptr, nullptr,
                                                 MCPT_GEOM_REFIT)) ||
                (rc = mcpt_render(ctx, &one)))
                break;
            st.extend_rays += one.extend_rays;
            st.shadow_rays += one.shadow_rays;
            st.vis_rays += one.vis_rays;
            st.ms_total += one.ms_total;
        }
        if (!rc) rc = mcpt_debug_geometry_update_ms(ctx, ums);
        if (!rc) printf("animate: %u frames, amplitude %.3f of the extent, last update %.3f ms on the device\n", a_frames, a_amp, ums[6]);
    } else if (t_frames) {  // a preview loop: camera, seed, render, guides, accumulate, filter
        std::vector<float> w[3];
        const uint32_t nframes = a_frames > t_frames ? a_frames : t_frames;
        for (uint32_t f = 0; f < nframes && !rc; f++) {
            cp.yaw_deg = -90.f + (float)f * t_yaw;
            mcpt_stage_stats one{};
            if (a_frames) {
                warp(d, a_amp, f, nframes, w);
                if ((rc = mcpt_scene_update_geometry(ctx, d.ntri, w[0].data(), w[1].data(), w[2].data(), nullptr, nullptr,
                                                     nullptr, MCPT_GEOM_REFIT)))
                    break;
            }
            // (a seed per frame that differs in every bit field: seeds one apart repeat each other's samples)
            if ((rc = mcpt_camera_make(&cp, &cam)) || (rc = mcpt_camera_set(ctx, &cam)) ||
                (rc = mcpt_set_seed(ctx, 0x9E3779B97F4A7C15ull * (uint64_t)(f + 1))) || (rc = mcpt_render(ctx, &one)) ||
                (rc = mcpt_guides_render(ctx, 4)) || (rc = mcpt_film_temporal(ctx, nullptr)) ||
                (rc = mcpt_temporal_denoise(ctx, nullptr)))
                break;
            st.extend_rays += one.extend_rays;
            st.shadow_rays += one.shadow_rays;
            st.vis_rays += one.vis_rays;
            st.ms_total += one.ms_total;
        }
        float tms = 0.f;
        if (!rc) rc = mcpt_debug_temporal_ms(ctx, &tms);
        if (!rc) rc = mcpt_denoised_write_png(ctx, 1.f, (out + "_temporal.png").c_str());
        if (!rc) rc = mcpt_film_denoise(ctx, nullptr);  // the last frame alone, for comparison
        if (!rc) rc = mcpt_denoised_write_png(ctx, 1.f, (out + "_denoised.png").c_str());
        if (!rc) printf("temporal: %u frames, %.2f degrees per frame, last accumulation %.3f ms\n", t_frames, t_yaw, tms);
    } else {
        rc = mcpt_render(ctx, &st);  // batch: every tile per iteration until all pixels have spp
        // adaptive: estimate -> budget -> render on, `rounds` times
        for (uint32_t r = 0; adaptive && r < rounds && !rc; r++) {
            uint64_t b3[3] = {0, 0, 0};
            mcpt_stage_stats more{};
            if ((rc = mcpt_film_error(ctx)) || (rc = mcpt_budget_from_error(ctx, &ap, b3)) || (rc = mcpt_render(ctx, &more))) break;
            printf("adaptive round %u: %llu samples budgeted, largest budget %llu, %llu pixels left at their count\n", r + 1,
                   (unsigned long long)b3[0], (unsigned long long)b3[1], (unsigned long long)b3[2]);
            st.extend_rays += more.extend_rays;
            st.shadow_rays += more.shadow_rays;
            st.vis_rays += more.vis_rays;
            st.ms_total += more.ms_total;
        }
    }
    if (rc) { fprintf(stderr, "render: %s\n", mcpt_last_error(ctx)); return 1; }
    const uint64_t rays = per_tile ? st.extend_rays : st.extend_rays + st.shadow_rays + st.vis_rays;
    printf("config %d %dx%d %d spp depth %d%s%s: %llu rays, %.1f ms device time, %.0f Mray/s\n", id, c.w, c.h,
           c.spp, c.depth, gpu_bvh ? " gpu-bvh" : "", fixed ? " fixed" : "", (unsigned long long)rays,
           st.ms_total, rays / (st.ms_total * 1e-3) / 1e6);
    if ((rc = mcpt_film_write_png(ctx, 1.f, (out + ".png").c_str())) ||
        (rc = mcpt_film_write_pfm(ctx, (out + ".pfm").c_str()))) {
        fprintf(stderr, "write: %s\n", mcpt_last_error(ctx));
        return 1;
    }
    if (guide_samples) {  // film -> guides -> filter -> display
        if ((rc = mcpt_guides_render(ctx, guide_samples)) || (rc = mcpt_film_denoise(ctx, nullptr)) ||
            (rc = mcpt_denoised_write_png(ctx, 1.f, (out + "_denoised.png").c_str()))) {
            fprintf(stderr, "denoise: %s\n", mcpt_last_error(ctx));
            return 1;
        }
    }
    if (guided_samples) {  // film + its error estimate -> guides -> guided filter -> display
        if (((guided_samples != guide_samples) && (rc = mcpt_guides_render(ctx, guided_samples))) ||
            (rc = mcpt_film_denoise_guided(ctx, nullptr)) ||
            (rc = mcpt_denoised_write_png(ctx, 1.f, (out + "_denoised_guided.png").c_str()))) {
            fprintf(stderr, "denoise-guided: %s\n", mcpt_last_error(ctx));
            return 1;
        }
    }
    mcpt_destroy(ctx);
    mcpt_scene_free(s);
    return 0;
}
