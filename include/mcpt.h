/*
 * mcpt.h -- C ABI of the MI355X-native wavefront path-tracing backend.
 *
 * Drop-in for the reference's CUDA path (JakeKurtz/MC-Path-Tracer):
 *   wavefront_pathtrace(...)   CUDA-RayTracer/wavefront_kernels.cuh:24-31 (body :377-442)
 *   clear_dfilm(dFilm*)        CUDA-RayTracer/wavefront_kernels.cuh:18   (body :55-76)
 *   draw_to_surface            CUDA-RayTracer/wavefront_kernels.cu:6-40
 *   PathTracer::render_image   CUDA-RayTracer/PathTracer.cpp:112-130
 *   Scene::load / set_environment_light / add_light   CUDA-RayTracer/Scene.h:40-58
 *   Camera::update (matrices)  CUDA-RayTracer/Camera.cu:194-224, PerspectiveCamera.cpp:49
 *
 * Conventions: every call returns 0 on success or a negative MCPT_E* code and
 * stores a message retrievable with mcpt_last_error(); nothing calls exit()
 * (the reference's checkCudaErrors exits with 99, CudaHelpers.cpp:3-11).
 * Host buffers passed in are copied; device memory is owned by the context.
 * Plain pointers and sizes only.
 */
#ifndef MCPT_H
#define MCPT_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MCPT_ABI_VERSION 1

enum {
    MCPT_OK = 0,
    MCPT_E_INVALID = -1,   /* bad argument / state */
    MCPT_E_HIP = -2,       /* HIP runtime error */
    MCPT_E_IO = -3,        /* file could not be read / parsed */
    MCPT_E_NOMEM = -4,
    MCPT_E_NODEVICE = -5   /* no gfx950 device: the product never falls back to the CPU */
};

/* Integrator configuration.  Reference mode reproduces the hard-coded values of
 * wavefront_kernels.cu: max_depth 5 (:142), rr_depth 3 (:189), spp <= 250 (:124). */
typedef struct mcpt_config {
    uint64_t seed;       /* keyed RNG seed; default 0x5EED2026 */
    int32_t spp;         /* samples per pixel (<= 2^19 - 256): gates processing and new samples */
    int32_t max_depth;   /* 'path_length > max_depth' terminates */
    int32_t rr_depth;    /* Russian roulette when 'path_length > rr_depth' */
    int32_t tile_w;      /* film tile (Film.cu:17: 256x256) */
    int32_t tile_h;
    int32_t flags;       /* MCPT_FLAG_* (0 = reference mode) */
} mcpt_config;

/* Quality mode: fixes the reference quirks of Appendix A.4-A.7, A.9 and
 * A.11 -- background added once, Russian-roulette survivors reweighted by 1/(1-q) with q from
 * the updated throughput, light-selection pdf 1/N, MIS weight 1 for delta lights, textbook
 * Gram-Schmidt, env sampling and pdf on matched (clamped) cells.  An alternative integrator:
 * never compared against the reference, only against the oracle's fixed mode. */
#define MCPT_FLAG_FIXED 1
/* The film observes the camera and the scene as in the reference (Film::update -> clear(),
 * Film.cu:278-281): mcpt_camera_set with a different camera, or a scene re-upload, marks the
 * film stale and the next mcpt_iterate / mcpt_wavefront_step / mcpt_render clears it first.
 * This flag turns that off (the caller clears explicitly with mcpt_film_clear). */
#define MCPT_FLAG_NO_AUTO_CLEAR 2

/* Scene as flat, BVH-ordered arrays (the device data model of Scene.h:24-33,
 * BVH.h:63-72, Triangle.h:11-23, dMaterial.cuh:11-33, EnvironmentLight.h:17-40). */
typedef struct mcpt_scene_desc {
    int32_t ntri;
    const float *v0, *v1, *v2;    /* 3*ntri world-space positions */
    const float *n0, *n1, *n2;    /* 3*ntri vertex normals */
    const int32_t *mat;           /* ntri material ids */
    int32_t nnodes;               /* LinearBVHNode array, depth-first */
    const float *bmin, *bmax;     /* 3*nnodes */
    const int32_t *offset;        /* primitivesOffset (leaf) / secondChildOffset (interior) */
    const int32_t *nprims;        /* 0 => interior */
    const int32_t *axis;
    int32_t nmat;
    const float *mat_params;      /* nmat*8: base rgb, fresnel rgb, roughness, metallic */
    int32_t ndir;                 /* directional lights (light ids 1..ndir; env is light 0) */
    const float *dir_params;      /* ndir*7: dir xyz, color rgb, ls */
    int32_t env_mode;             /* 0 = Color, 1 = HRDI */
    float env_color[3];
    float env_ls;
    int32_t env_w, env_h;
    const float *env_tex;         /* env_h*env_w*4 RGBA32F, row 0 = top */
    const float *env_marginal_y;  /* env_h */
    const float *env_conds_y;     /* env_h*env_w */
    const float *env_pdf;         /* env_h*env_w */
    const int32_t *tri_id;        /* optional ntri original triangle ids (NULL = array position): the
                                     exact-t tie-break key and the id the trace API reports, so
                                     neither depends on the order a BVH builder stored triangles in */
} mcpt_scene_desc;

/* dCamera (Camera.h:34-46): column-major m[c][r] = m[c*4+r]. */
typedef struct mcpt_camera {
    float inv_view_proj[16];
    float inv_view[16];
    float lens_radius;
    float focal;
} mcpt_camera;

/* PerspectiveCamera parameters (Camera.h:98-117, PerspectiveCamera.cpp:30-49). */
typedef struct mcpt_camera_params {
    float position[3];
    float yaw_deg, pitch_deg;     /* Camera.cu:210-224 */
    float fovy_rad, aspect, znear, zfar;
    float lens_radius, focal;     /* defaults 1e-4, 35 (Camera.h:115-116) */
} mcpt_camera_params;

typedef struct mcpt_stage_stats {
    uint64_t extend_rays;   /* closest-hit rays traced */
    uint64_t shadow_rays;   /* light-sample shadow rays */
    uint64_t vis_rays;      /* BRDF-sample visibility rays (wavefront_kernels.cu:334-336) */
    uint64_t iterations;    /* wavefront iterations executed */
    uint64_t live_paths;    /* paths still in flight after the call */
    float ms_total;         /* device time of logic+generate+material+extend+shadow */
    float ms_shade;         /* k_shade: logic + generate + material (fused) */
    float ms_extend;        /* k_trace: extension AND any-hit rays (one fused persistent launch) */
    float ms_shadow;        /* 0: the any-hit rays are traced inside the k_trace launch */
    uint64_t ext_nodes;     /* closest-hit: child-pair nodes fetched (2 boxes each); this and the next five
                               are counted only under mcpt_set_work_counters(ctx, 1) */
    uint64_t ext_tests;     /* closest-hit: ray/triangle tests */
    uint64_t ext_hits;      /* closest-hit: rays that found a surface */
    uint64_t any_nodes, any_tests, any_hits;   /* any-hit (shadow + visibility) */
} mcpt_stage_stats;

enum { MCPT_STAGE_LOGIC = 0, MCPT_STAGE_GENERATE = 1, MCPT_STAGE_MATERIAL = 2,
       MCPT_STAGE_EXTEND = 3, MCPT_STAGE_SHADOW = 4 };

/* Path state at the shading stages' boundary, for mcpt_stage_run(LOGIC | GENERATE | MATERIAL)
 * (host SoA, n paths; SURVEY.md 8(b) per-stage parity harness).  Field meaning against the
 * reference's Paths (Wavefront.cuh:8-26):
 *   flags     bit 0 dead; bits 1..8 len (path_length); bits 9..12 the MIS conditions of the
 *             previous vertex (9 light term w > 0 && pdf > 0, 10 BRDF term, 11 f_sample == 0 or
 *             pdf_sample == 0, 12 a BRDF visibility ray was drawn: non-delta light); bits 13..31
 *             the sample index the path renders (keys its RNG draws)
 *   samples   dFilm.samples of the pixel (completed samples)
 *   hit_tri   the closest hit of `ray` (index into the uploaded scene's triangle arrays, -1 none)
 *   ray_o/_d  Paths.ray (3n each)
 *   beta      Paths.beta in xyz, (f_sample / pdf_sample).x in w (4n)
 *   nee0/1    the light-sample / BRDF-sample MIS terms f * Li * w / pdf (wavefront_kernels.cu:
 *             168-179) in xyz, (f_sample / pdf_sample).y / .z in w (4n)
 *   vis       light-sample / BRDF-sample visibility (Paths.visible; the BRDF one is the
 *             reference's inline visibility ray, :334-336) (2n)
 *   Ld        dFilm.Ld of the pixel (3n)
 *   light_o/_d, bvis_o/_d   MATERIAL out: the light-sample shadow ray (ray_light, :212-213) and the
 *             BRDF visibility ray (:334) it queued for the trace stage; NaN where none was
 *             queued (a delta light, or a ray resolved in place because it cannot hit the scene:
 *             its vis byte is then set to 1) (3n each)
 *   queued    out: bit 0 extension ray queued, bit 1 path continues into MATERIAL (LOGIC),
 *             bit 2 light ray queued, bit 3 BRDF visibility ray queued (n)
 * LOGIC (k_shade): wf_logic + wf_generate of a film of film_w x film_h pixels, path i = pixel
 * (i % film_w, i / film_w), one path per pixel, the context's camera and config.  In: flags,
 * samples, hit_tri, ray_d, beta, nee0, nee1, vis, Ld; a live path's sample index (flags bits
 * 13..31) must equal its samples, as in every state the reference or the oracle produces
 * (MCPT_E_INVALID otherwise: the device derives the count from the index).  Out: flags, samples,
 * Ld, ray_o/_d of new paths, beta (the updated throughput of continuing paths), hit_tri, queued.
 * GENERATE: LOGIC with every path dead (wf_generate for sample index `samples`).
 * MATERIAL (k_material): the light choice (:207-213) and wf_mat_mix (:295-375) of continuing path
 * i at pixel i.  In: flags (len, sample index), hit_tri, ray_o/_d, beta.  Out: flags, ray_o/_d
 * (the next extension ray), beta, nee0, nee1, hit_tri, vis, light/bvis rays, queued. */
typedef struct mcpt_path_view {
    uint32_t film_w, film_h;
    uint32_t *flags, *samples;
    int32_t *hit_tri;
    float *ray_o, *ray_d, *beta, *nee0, *nee1;
    uint8_t *vis;
    float *Ld;
    float *light_o, *light_d, *bvis_o, *bvis_d;
    uint8_t *queued;
} mcpt_path_view;

/* Caller SoA buffers for mcpt_stage_run (host memory). */
typedef struct mcpt_soa_view {
    const float *ray_o;     /* EXTEND / SHADOW in: 3*n */
    const float *ray_d;     /* EXTEND / SHADOW in: 3*n */
    float *hit_pos_t;       /* EXTEND out: 4*n pos.xyz, t */
    float *hit_nrm_mat;     /* EXTEND out: 4*n normal.xyz, (float)material (-1 miss) */
    int32_t *hit_tri;       /* EXTEND out: n triangle index or -1 */
    uint8_t *visible;       /* SHADOW out: n */
    uint32_t *steps;        /* optional out, unused since round 4 (was: per-ray node fetches + tests in diagnostics builds; left zero) */
    mcpt_path_view *paths;  /* LOGIC / GENERATE / MATERIAL: in->paths inputs, out->paths outputs */
} mcpt_soa_view;

typedef struct mcpt_ctx mcpt_ctx;     /* device context: one per GPU, not thread-safe */
typedef struct mcpt_scene mcpt_scene; /* host scene builder (Scene.cu) */

/* ---- device context (replaces wavefront_pathtrace / clear_dfilm) ---- */
int mcpt_create(int device, const mcpt_config *cfg, mcpt_ctx **out);
void mcpt_destroy(mcpt_ctx *ctx);
const char *mcpt_last_error(const mcpt_ctx *ctx);   /* ctx may be NULL: last global error */
int mcpt_scene_upload(mcpt_ctx *ctx, const mcpt_scene_desc *desc);
/* Same scene with the BVH built on the GPU instead of taken from desc (its
 * BVH arrays are ignored and may be empty); one triangle per leaf.  Hits and films are
 * identical to mcpt_scene_upload's: the traversal's result does not depend on the tree.
 * Builders (mcpt_set_gpu_bvh_builder):
 *   MCPT_GPU_BVH_PLOC (default): parallel locally-ordered clustering over Morton-sorted
 *     triangles -- surface-area agglomeration, quality close to a full SAH build;
 *   MCPT_GPU_BVH_LBVH: Karras' linear BVH (Morton-code splits; fastest build, slower trees). */
#define MCPT_GPU_BVH_LBVH 0
#define MCPT_GPU_BVH_PLOC 1
int mcpt_scene_upload_gpu_bvh(mcpt_ctx *ctx, const mcpt_scene_desc *desc);
int mcpt_set_gpu_bvh_builder(mcpt_ctx *ctx, int32_t builder);
/* Geometry update: new vertex positions, and optionally normals, for the
 * triangles of the scene that is already uploaded -- animated geometry without a re-upload.  The arrays
 * are in the order of the uploaded desc's triangle arrays.  The triangle records are rewritten on the
 * device and the tree is refitted in place or rebuilt; then exactly the state that depends on geometry
 * is derived again (culling margins, root box, the 4-wide nodes' boxes, the occluder cache's records,
 * cells, pre-fill and complete keys).  Triangle and material ids, materials, lights, the environment
 * with all its tables and the occluder grid's size stay, and so do the upload-time environment knobs
 * (MCPT_CULL, MCPT_CULL_PLANE, MCPT_BVH_WIDTH, MCPT_SIBLING_LAYOUT, MCPT_OCC_*) as the upload read them.
 * Hits and films after an update equal, bit for bit, those of a fresh upload of the moved mesh.
 * The film sees an update as it sees a re-upload: it goes stale (the next iteration clears it unless
 * MCPT_FLAG_NO_AUTO_CLEAR), the guides go stale, the temporal history is dropped and the primary-hit
 * table is rebuilt on next use.
 * MCPT_E_INVALID, with the scene left exactly as it was: no scene; ntri different from the uploaded
 * count; only some of the three normal arrays; an unknown mode; MCPT_GEOM_REBUILD on a scene uploaded
 * with a host tree.  A scene without triangles accepts ntri == 0 and does nothing.  Synchronous.
 * Any other error (MCPT_E_HIP, MCPT_E_NOMEM) does not leave the scene as it was: the records and nodes
 * are rewritten in place before the occluder state is derived, and a rebuild frees the old tree before
 * it builds the new one.  After such an error the context has no scene: upload it again.
 * Normals left NULL keep the current ones: those of the last update that gave normals, else the upload's.
 * The update keeps device scratch between calls (per triangle 32 B of vertex boxes and 4 B of margins,
 * and for the host entry 36 B of staged vertices, 72 B with normals); a scene upload frees it. */
#define MCPT_GEOM_REFIT   0   /* keep the tree's topology, recompute boxes and margins */
/* Device-built scenes only: run the GPU builder (mcpt_set_gpu_bvh_builder) again.  A scene of 4-wide
 * nodes (more than 32 MB of pair nodes, or MCPT_BVH_WIDTH=4) is collapsed again on the host as at upload,
 * which dominates such a rebuild (2 M triangles: 173 of 210 ms); a refit only regathers boxes on the device. */
#define MCPT_GEOM_REBUILD 1
int mcpt_scene_update_geometry(mcpt_ctx *ctx, int32_t ntri,
                               const float *v0, const float *v1, const float *v2,   /* 3*ntri each, host */
                               const float *n0, const float *n1, const float *n2,   /* all three, or all NULL: keep */
                               int32_t mode);
/* The same with device pointers on ctx's GPU (vertices skinned by a torch op, say); the caller has
 * finished writing them. */
int mcpt_scene_update_geometry_device(mcpt_ctx *ctx, int32_t ntri, const void *d_v0, const void *d_v1,
                                      const void *d_v2, const void *d_n0, const void *d_n1, const void *d_n2,
                                      int32_t mode);
/* Device ms of the last update: [0] records, [1] refit or rebuild incl. margins, [2] 4-wide regather
 * (a rebuild: the collapse), [3] occluder records, [4] pre-fill probes, [5] complete keys, [6] total; [7] 0 */
int mcpt_debug_geometry_update_ms(const mcpt_ctx *ctx, float *out8);
int mcpt_camera_set(mcpt_ctx *ctx, const mcpt_camera *cam);
int mcpt_film_resize(mcpt_ctx *ctx, uint32_t w, uint32_t h, uint32_t tile_w, uint32_t tile_h);
int mcpt_film_clear(mcpt_ctx *ctx);                                          /* == clear_dfilm */
/* Paths in flight per pixel (default 1, the reference's one path per pixel,
 * wavefront_kernels.cu:108,114).  With S > 1, path slot k of a pixel renders its samples
 * k, k + S, k + 2S, ... into its own accumulator and the film readers sum the slots in
 * slot order: the same per-sample contributions, summed in another order (films agree to
 * float rounding, samples exactly).  More rays per iteration amortise each launch's ramp
 * and drain.  Re-allocates the path state, so a change CLEARS the film.  A rejected count
 * (W*H*slots >= 2^31, or out of memory) leaves the previous slot count in place. */
int mcpt_set_path_slots(mcpt_ctx *ctx, uint32_t slots);
/* Work partitions of the persistent traversal kernel (0 = device default: two per XCD, 16 on
 * MI355X; at most 64).  Each partition's rays are handed out by one counter; waves start on a
 * partition of their die and, once it is drained, join the others, so all settings trace every
 * ray and give identical results -- a tuning knob only (MCPT_TRACE_PARTS sets the default). */
int mcpt_set_trace_partitions(mcpt_ctx *ctx, uint32_t nparts);
/* Traversal work counters (mcpt_stage_stats ext_nodes / ext_tests / ext_hits / any_*): on = 1 runs
 * k_trace's counting build, off (0, the default) leaves them 0.  The counting build holds six more
 * per-lane registers, which the 64-VGPR 8-wave traversal cannot afford without spilling. */
int mcpt_set_work_counters(mcpt_ctx *ctx, int32_t on);
/* Continuation rays the next logic pass is certain to discard: on = 1 (the
 * default) does not make them.  A path that Russian roulette will end at its next vertex -- the
 * decision reads only the throughput stored now and a keyed draw -- gets no continuation sample and
 * no extension ray; a path whose next vertex lies beyond max_depth ends at once, without its
 * material evaluation and its three rays.  Films, sample counts and every ray count are the same
 * with 0 and 1 (the rays are counted as the reference traces them and appear as resolved in place);
 * mcpt_stage_run always runs the stages without it.  May be changed between calls, mid-frame too. */
int mcpt_set_skip_discarded(mcpt_ctx *ctx, int32_t on);
int mcpt_set_tiles(mcpt_ctx *ctx, const uint32_t *tile_xy, uint32_t ntiles); /* batch tile set; NULL = all */
/* Path-state layout (default 0, full: one path per pixel of the whole W x H film per slot, path id =
 * pixel id as in the reference, wavefront_kernels.cu:108,114; Film.cu:254-275 sizes the pool at
 * W x H).  on = 1, compact: the path state covers only the tile set, slots x (tiles x tile pixels)
 * paths -- a rank of a multi-GPU split that owns 1/N of the tiles holds 1/N of the state and clears
 * 1/N of it.  Results do not change (every sample is keyed by its pixel).  In the compact layout
 * mcpt_set_tiles re-allocates the path state and CLEARS the film (a tile listed twice is rejected),
 * mcpt_set_path_slots keeps the tile set, mcpt_film_resize resets it to every tile, and
 * mcpt_wavefront_step accepts only tiles of the set.  The film readers still return the W x H frame:
 * the tile set's pixels, pixels scattered in by mcpt_film_unpack_tiles / mcpt_gather, zero elsewhere.
 * A change re-allocates and clears the film. */
int mcpt_set_compact_paths(mcpt_ctx *ctx, int32_t on);
int mcpt_wavefront_step(mcpt_ctx *ctx, uint32_t tile_x, uint32_t tile_y, mcpt_stage_stats *st); /* one iteration, one tile */
int mcpt_iterate(mcpt_ctx *ctx, uint32_t iterations, mcpt_stage_stats *st);  /* batch iterations over the tile set */
int mcpt_render(mcpt_ctx *ctx, mcpt_stage_stats *st);                       /* iterate until every pixel has spp */
int mcpt_stage_run(mcpt_ctx *ctx, int stage, const mcpt_soa_view *in, mcpt_soa_view *out, uint32_t n);
int mcpt_film_read(mcpt_ctx *ctx, float *Ld_rgb, uint32_t *samples);         /* host copies, 3*W*H / W*H */
int mcpt_film_read_device(mcpt_ctx *ctx, void *d_Ld_rgb, void *d_samples);  /* device-to-device */
int mcpt_film_pack_tiles(mcpt_ctx *ctx, void *d_out, uint32_t *npix);       /* tile-set pixels -> packed 16 B/px (rgb f32, samples u32) */
/* The inverse on the gathering rank: scatter another rank's packed tile pixels (device memory on
 * ctx's GPU, 16 B/px in the order mcpt_film_pack_tiles wrote them for tiles tile_xy[0..ntiles))
 * into ctx's film accumulators.  The tiles must not be ctx's own (their other path slots would
 * be added in), and until the next film clear they cannot become ctx's own either: mcpt_set_tiles
 * rejects a set holding one (MCPT_E_INVALID; the compact layout's set_tiles clears the film
 * anyway).  Synchronous. */
int mcpt_film_unpack_tiles(mcpt_ctx *ctx, const void *d_in, const uint32_t *tile_xy, uint32_t ntiles);
int mcpt_film_tonemap_rgba8(mcpt_ctx *ctx, float exposure, uint8_t *out);   /* == draw_to_surface */
int mcpt_film_size(const mcpt_ctx *ctx, uint32_t *w, uint32_t *h);
/* Frame-end gather of a multi-GPU render in one process: the tile-set pixels of
 * every context (one per GPU, same film and tile size, tile sets disjoint from the root's) are
 * copied device-to-device over xGMI into ctxs[root]'s film, whose readers then return the whole
 * frame.  Processes with one GPU each send their mcpt_film_pack_tiles buffer to the root over
 * RCCL, which scatters it with mcpt_film_unpack_tiles (mcpt/parallel.py).  Synchronous. */
int mcpt_gather(mcpt_ctx *const *ctxs, int32_t n, int32_t root);
/* Film output (replaces stbi_write_png of the display buffer, RenderingContext.cpp:114-118):
 * PNG = tonemapped 8-bit RGB, row 0 = top; PFM = float RGB radiance Ld/samples (0 where no sample). */
int mcpt_film_write_png(mcpt_ctx *ctx, float exposure, const char *path);
int mcpt_film_write_pfm(mcpt_ctx *ctx, const char *path);
int mcpt_image_write_png(const char *path, uint32_t w, uint32_t h, const uint8_t *rgba8);
int mcpt_image_write_pfm(const char *path, uint32_t w, uint32_t h, const float *rgb);
/* PNG reader for texture images (host/png_read.cpp; an inflate and a PNG decoder of the project's own, no
 * library, no device call).  mcpt_image_read_png_memory decodes the n bytes of a PNG payload into w x h RGBA8
 * texels, row 0 of the file first (glTF's and section 19's orientation): what mcpt_texture and the scene's
 * texture setters take.  With rgba8 == NULL it validates the signature and IHDR only and returns the size;
 * otherwise cap is the buffer's size in bytes, and a cap below 4 w h is MCPT_E_INVALID (as is a NULL data, w
 * or h).  mcpt_image_read_png is the same over a file.
 * Accepted: colour type 0 at bit depth 1/2/4/8/16, 2 at 8/16, 3 at 1/2/4/8 with PLTE and optional tRNS, 4 at
 * 8/16, 6 at 8/16; non-interlaced; all five filter types; one or more consecutive IDAT chunks; ancillary chunks
 * are skipped; w and h in 1..16384.  A 16-bit sample becomes its high byte; a grey sample of depth d < 8 becomes
 * v * (255 / (2^d - 1)); grey replicates to rgb; alpha is 255 where the file has none (tRNS counts for palette
 * images only).
 * Refused with MCPT_E_IO, nothing written to rgba8, w or h: a bad signature, a bad chunk CRC, chunk order
 * violations, an unknown critical chunk, Adam7 interlace, a palette index beyond PLTE, a zlib header that is
 * not deflate with a 32K window, a preset dictionary, a bad Adler-32, a deflate stream that is malformed
 * (reserved block type, LEN / NLEN mismatch, over-subscribed or incomplete code lengths other than the
 * one-code distance case, a distance beyond the bytes produced) or that yields fewer or more than
 * h * (1 + rowbytes) bytes.  MCPT_E_NOMEM, nothing written either: the decoder's buffers cannot be allocated.
 * mcpt_image_read_png_error: the reason of the calling thread's last MCPT_E_IO or MCPT_E_NOMEM from either
 * call (a static string buffer; "" before any). */
int mcpt_image_read_png_memory(const uint8_t *data, size_t n, int32_t *w, int32_t *h, uint8_t *rgba8, size_t cap);
int mcpt_image_read_png(const char *path, int32_t *w, int32_t *h, uint8_t *rgba8, size_t cap);
const char *mcpt_image_read_png_error(void);
/* ---- preview denoiser: first-hit guide buffers + an edge-avoiding a-trous
 * wavelet filter (Dammertz et al. 2010) between the film and the display.  A context that never
 * calls these allocates and launches nothing for them.
 *
 * Guides: per pixel the sums over guide samples of the first hit's albedo (the material's base
 * rgb), normal and distance t; a miss adds albedo (1,1,1), normal 0 and depth 0.  Guide sample s of
 * a pixel is traced along the camera ray of film sample s (same seed, pixel and sample key), over
 * exactly the pixels the renderer renders (x < W-1 && y < H-1) of the whole film, whatever the tile
 * set or path layout; other pixels keep count 0 and zeros.  With lens_radius == 0 every sample's ray
 * is the same, so one is traced and the count is 1.  1 <= nsamples < 2^19 - 256; needs a scene, a
 * camera and a film.  The path state, the queues, the ray counters and the occluder cache are not
 * touched.  The rays are traced in chunks whose temporary buffers stay under 64 MiB
 * (MCPT_GUIDE_CHUNK_BYTES overrides the budget; the result does not depend on it).  The guides are
 * stale after mcpt_camera_set with a different camera, a scene upload or mcpt_film_resize; a film
 * clear leaves them valid. */
int mcpt_guides_render(mcpt_ctx *ctx, uint32_t nsamples);
/* Guide sums (3*W*H, 3*W*H, W*H floats) and sample counts (W*H); any pointer may be NULL.
 * MCPT_E_INVALID without valid guides. */
int mcpt_guides_read(mcpt_ctx *ctx, float *albedo_rgb, float *normal_xyz, float *depth, uint32_t *count);
/* Filter parameters.  Pass i (0 <= i < passes) visits the 25 taps q = p + 2^i (dx, dy), dx, dy in
 * -2..2, row by row, skips taps outside the film or invalid (no samples, or a colour that is not
 * finite) and weights the rest by h[dy] h[dx] exp(-x), h = {1/16, 1/4, 3/8, 1/4, 1/16},
 *   x = |C(p)-C(q)|^2 / sc_i^2 + |N(p)-N(q)|^2 / sn^2 + |A(p)-A(q)|^2 / sa^2 + (Z(p)-Z(q))^2 / (sz^2 max(Z(p)^2, 1e-12))
 * with sc_i = sigma_color 2^-i; the centre tap has x = 0, and a tap whose x is not a finite number
 * >= 0 has weight 0.  C is the mean radiance, N / A / Z the mean guides.  An invalid pixel outputs 0. */
typedef struct mcpt_denoise_params {
    int32_t passes;        /* 1..8; pass i taps at stride 2^i */
    float sigma_color;     /* pass 0; halves every pass.  A sigma <= 0 disables its term */
    float sigma_normal, sigma_albedo, sigma_depth;
} mcpt_denoise_params;
int mcpt_denoise_default_params(mcpt_denoise_params *p);
/* The filter over host images of means (w*h pixels: rgb / albedo / normal 3 floats each, depth 1,
 * samples 1 or NULL = every pixel has samples) into out_rgb (3*w*h): the kernels mcpt_film_denoise
 * runs, for parity tests and for frames gathered elsewhere.  Needs neither a scene nor a film. */
int mcpt_denoise_run(mcpt_ctx *ctx, uint32_t w, uint32_t h, const float *rgb, const uint32_t *samples,
                     const float *albedo, const float *normal, const float *depth, const mcpt_denoise_params *p,
                     float *out_rgb);
/* Filter the film as its readers see it (every path slot summed, the compact layout scattered, a
 * root's gathered frame) with the context's guides; p == NULL: the defaults.  MCPT_E_INVALID when the
 * guides are missing or stale (call mcpt_guides_render first).  The film itself is not changed. */
int mcpt_film_denoise(mcpt_ctx *ctx, const mcpt_denoise_params *p);
/* The last mcpt_film_denoise result: rgb (3*W*H floats); device-to-device as W*H float4 (rgb, 1 for a
 * valid pixel / 0); Reinhard-tonemapped like mcpt_film_tonemap_rgba8 (with samples = 1); as PNG.
 * MCPT_E_INVALID until a denoise has run since the last mcpt_film_resize. */
int mcpt_denoised_read(mcpt_ctx *ctx, float *rgb);
int mcpt_denoised_read_device(mcpt_ctx *ctx, void *d_rgb);
int mcpt_denoised_tonemap_rgba8(mcpt_ctx *ctx, float exposure, uint8_t *out);
int mcpt_denoised_write_png(mcpt_ctx *ctx, float exposure, const char *path);
/* Device times (ms) of the last mcpt_guides_render (out10[0]) and of the last mcpt_film_denoise /
 * mcpt_denoise_run: the plane set-up (out10[1]) and each pass (out10[2 + i]; 0 beyond the passes run). */
int mcpt_debug_denoise_ms(const mcpt_ctx *ctx, float *out10);
/* ---- variance-guided denoising: the a-trous filter above steered by a
 * per-pixel variance of the mean luminance, as SVGF's spatial filter is (Schied et al. 2017, 4.4).
 * A second path beside the plain one: a context that never calls these allocates and launches
 * nothing for them, and mcpt_film_denoise / mcpt_denoise_run compute what they always did.
 *
 * Each pixel carries a variance v (-1: unknown) and its luminance l.  In pass i a pixel p with a
 * variance replaces the plain filter's colour term by
 *   |l(p) - l(q)| / (sigma_lum sqrt(vt(p)) + lum_eps)
 * with vt the 3 x 3 Gaussian ({1/4, 1/8, 1/16}, stride 1) of the known variances around p, and its
 * variance becomes sum w^2 v(q) / (sum w)^2 (v(p) for a tap without one).  A pixel without a variance
 * takes the plain term with sigma_color 2^-i and stays without one.  With lum_eps = 0 the result is
 * equivariant under radiance scaling by powers of two, and a pixel of zero variance is left alone. */
typedef struct mcpt_denoise_guided_params {
    int32_t passes;        /* 1..8 */
    float sigma_lum;       /* > 0 */
    float lum_eps;         /* >= 0 */
    float sigma_color;     /* the plain term of pixels without a variance */
    float sigma_normal, sigma_albedo, sigma_depth;
} mcpt_denoise_guided_params;
int mcpt_denoise_guided_default_params(mcpt_denoise_guided_params *p);
/* The counterpart of mcpt_denoise_run: host images as there plus variance (w*h floats; a value that is
 * not in [0, FLT_MAX] is "unknown"); out_variance (w*h floats, -1 where unknown) may be NULL. */
int mcpt_denoise_guided_run(mcpt_ctx *ctx, uint32_t w, uint32_t h, const float *rgb, const uint32_t *samples,
                            const float *variance, const float *albedo, const float *normal, const float *depth,
                            const mcpt_denoise_guided_params *p, float *out_rgb, float *out_variance);
/* Filter the film as mcpt_film_denoise does, with v = se^2 of a fresh mcpt_film_error estimate (which
 * it runs itself and leaves readable through mcpt_film_error_read): needs valid guides, >= 2 path
 * slots and no paths in flight.  Pixels without an estimate (fewer than 2 slots with samples; pixels
 * scattered in from another context) take the plain term, unless mcpt_set_variance_fill is on (below),
 * which also lifts the slot requirement.  The result replaces the last denoised frame: the
 * mcpt_denoised_* readers serve it. */
int mcpt_film_denoise_guided(mcpt_ctx *ctx, const mcpt_denoise_guided_params *p);
/* The filtered variances (W*H floats, -1 where unknown) of the last denoise; MCPT_E_INVALID unless
 * that was mcpt_film_denoise_guided. */
int mcpt_denoised_variance_read(mcpt_ctx *ctx, float *var);
/* ---- adaptive sampling: per-pixel sample budgets, "continue rendering", and
 * an error estimate of the film.  A context that never calls these allocates and launches nothing
 * for them, and renders with the kernels it always did.
 *
 * Composition property: every sample is keyed by (pixel, sample index) and pixels never share an
 * accumulator, so with budget map m, pixel p of the film equals pixel p of a uniform render at
 * spp = m[p] with the same path-slot count, bit for bit (Ld and samples), and a frame continued from
 * n to n' samples equals a direct n' render.
 *
 * Known bias: a budget computed from the samples a pixel already has stops the pixel when those
 * samples happen to agree, so the expected pixel value is no longer the plain mean's (Kirk and Arvo,
 * "Unbiased sampling techniques for image synthesis", SIGGRAPH 1991).  Not corrected here: min_spp
 * bounds it, and a two-pass scheme (budgets from one render, the image from a fresh one) avoids it.
 *
 * mcpt_set_sample_budget installs budget[y * W + x] (W*H entries, copied) in place of the uniform spp:
 * pixel p is sampled until it has budget[p] samples, 0 = never; NULL removes the map.  A budget below
 * a pixel's completed count stops the pixel and removes nothing.  mcpt_set_spp changes the uniform
 * count of a live context (bounds as in mcpt_config).  Neither clears the film; both make the next
 * mcpt_iterate / mcpt_render pick raised counts up.  Rejected with MCPT_E_INVALID, the previous map
 * and spp staying in place: an entry above 2^19 - 256, and any call while paths are in flight (the
 * last iteration since the film clear left live paths).  The map is keyed by film pixel: film
 * clears, mcpt_set_path_slots, mcpt_set_tiles and mcpt_set_compact_paths keep it, mcpt_film_resize
 * drops it.  mcpt_render sizes its batches by the largest budget.  mcpt_stage_run never uses it. */
int mcpt_set_sample_budget(mcpt_ctx *ctx, const uint32_t *budget);
int mcpt_sample_budget_read(mcpt_ctx *ctx, uint32_t *out);   /* W*H; MCPT_E_INVALID when no map is installed */
int mcpt_set_spp(mcpt_ctx *ctx, int32_t spp);
/* Error estimate from the path slots (>= 2 slots, no path in flight): slot k of a pixel holds the
 * samples k, k + S, ... in its own accumulator (Ld_k, n_k), so the slot means are estimates from
 * disjoint samples.  Over the slots with n_k > 0, in ascending order, K of them:
 *   y_k = lum(Ld_k) / n_k,  ybar = (sum y_k) / K,  s2 = sum (y_k - ybar)^2 / (K - 1),  se = sqrt(s2 / K)
 * in fp32, lum = 0.299 r + 0.587 g + 0.114 b.  Per pixel {se, ybar, (float)K, (float)n}, n = sum n_k;
 * K < 2: se = -1 (no estimate).  Pixels that are not the context's own (outside its tile set, or
 * scattered in by mcpt_film_unpack_tiles / mcpt_gather) get K = 0.  Non-finite radiance propagates.
 * mcpt_film_error_read copies the last result (4*W*H floats). */
int mcpt_film_error(mcpt_ctx *ctx);
int mcpt_film_error_read(mcpt_ctx *ctx, float *out4);
/* The same kernel over host images, slot-major: Ld_slots 3*w*h floats per slot, samples_slots w*h per
 * slot, out4 4*w*h.  Needs neither a scene nor a film (the counterpart of mcpt_denoise_run). */
int mcpt_error_run(mcpt_ctx *ctx, uint32_t w, uint32_t h, uint32_t slots, const float *Ld_slots,
                   const uint32_t *samples_slots, float *out4);
/* One path slot's accumulators as W x H images (3*W*H / W*H; either may be NULL), zero where the pixel
 * is not the context's own: summed in slot order they are mcpt_film_read's film. */
int mcpt_debug_film_read_slot(mcpt_ctx *ctx, uint32_t slot, float *Ld_rgb, uint32_t *samples);
/* Budgets from the last mcpt_film_error result, built on the device and installed like
 * mcpt_set_sample_budget's.  Per pixel, in fp32, with tau = target_rel_err and lo = max(n, min_spp):
 *   r = se / (ybar + lum_floor),  q = r / tau,  want = n * (q * q)
 *   budget = max(ceil(want), lo), or max(max_spp, lo) unless want < max_spp (the large value is never
 *   converted); lo where r <= tau or there is no estimate (se < 0); n where r is not finite (a NaN
 *   pixel cannot converge and is not fed); 0 for the never-rendered last row and column and for
 *   pixels that are not the context's own.
 * out3 (may be NULL): the sum of the budgets, the largest, and the context's pixels left at their
 * current count.  p == NULL: the defaults.  target_rel_err > 0, min_spp <= max_spp <= 2^19 - 256. */
typedef struct mcpt_sample_budget_params {
    float target_rel_err;   /* tau: the standard error aimed at, relative to mean luminance + lum_floor */
    float lum_floor;        /* default 0.01: keeps dark pixels from demanding every sample */
    uint32_t min_spp, max_spp;
} mcpt_sample_budget_params;
int mcpt_sample_budget_default_params(mcpt_sample_budget_params *p);
int mcpt_budget_from_error(mcpt_ctx *ctx, const mcpt_sample_budget_params *p, uint64_t *out3);
/* Device bytes the context holds for adaptive sampling (0 until one of the calls above needs some),
 * and the device times (ms) of the last error kernel (out2[0]) and budget kernel (out2[1]). */
int64_t mcpt_debug_adaptive_bytes(const mcpt_ctx *ctx);
int mcpt_debug_adaptive_ms(const mcpt_ctx *ctx, float *out2);
/* ---- temporal accumulation: the previous accumulated frame reprojected into
 * the current one, SVGF's temporal half (Schied et al. 2017, 4.1 - 4.2), between the film and the
 * a-trous passes.  Opt-in: a context that never calls these allocates and launches nothing for them.
 *
 * mcpt_set_seed sets the seed of a live context and clears the film: a sample is keyed by (seed, pixel,
 * sample index), so frames after a clear repeat their noise unless the seed changes, and temporal reuse
 * needs frames that do not.  MCPT_E_INVALID while paths are in flight.  The guide buffers become stale
 * (lens guide rays are keyed by the seed); the temporal history stays.  The seed is XORed onto
 * (pixel << 32 | sample index) before it is hashed, so seeds that differ in their low bits alone hand a
 * pixel the same samples in another order (k and k ^ 1 at 2 spp): give successive frames seeds that
 * differ in every bit field, e.g. (frame + 1) * 0x9E3779B97F4A7C15. */
int mcpt_set_seed(mcpt_ctx *ctx, uint64_t seed);
/* Host only: proj * view = inverse(cam->inv_view_proj), column-major, by cofactors in double rounded
 * once.  The matrix mcpt_film_temporal stores as VP_prev, and the one mcpt_temporal_run takes. */
int mcpt_camera_view_proj(const mcpt_camera *cam, float *out16);
/* Per pixel: X = world position of the first hit (pinhole ray origin + depth * direction; with a lens
 * the centre-of-lens ray), projected with VP_prev to the previous frame's pixel grid; a bilinear tap of
 * the previous accumulated colour whose corners must lie inside the film, hold a history, and agree in
 * position (|X_q - X| <= pos_tol * depth) and normal (|n_q - n| <= nrm_tol); then with s the pixel's
 * sample count and N_h the tap's:
 *   N_c = min(N_h, max_history),  alpha = max(s / (N_c + s), alpha_min),
 *   c' = h + alpha (c - h),  N' = N_c + s,  v' = (1 - alpha)^2 v_h + alpha^2 v_c
 * v' is known only where both variances are.  Without an accepted corner (a disocclusion, the first
 * call, a pixel whose depth is not a finite number > 0): c' = c, N' = s, v' = v_c. */
typedef struct mcpt_temporal_params {
    float pos_tol;       /* >= 0, relative to the pixel's depth */
    float nrm_tol;       /* >= 0 */
    float max_history;   /* >= 0, in samples */
    float alpha_min;     /* 0..1 */
} mcpt_temporal_params;
int mcpt_temporal_default_params(mcpt_temporal_params *p);
/* Accumulate the film into the history (p == NULL: the defaults): needs valid guides and no paths in
 * flight; with >= 2 path slots v_c = se^2 of a fresh mcpt_film_error estimate, with 1 slot every
 * variance is unknown (mcpt_set_variance_fill, below, estimates the unknown ones).  Uses the camera and planes the previous call stored, then stores this call's.
 * The first call, and any call after a reset, accumulates nothing.  mcpt_temporal_reset drops the
 * history, and so do a scene upload and mcpt_film_resize; film clears, mcpt_set_seed, camera changes
 * and mcpt_set_path_slots keep it. */
int mcpt_film_temporal(mcpt_ctx *ctx, const mcpt_temporal_params *p);
int mcpt_temporal_reset(mcpt_ctx *ctx);
/* The last accumulated frame: rgb 3*W*H, nsamples W*H (N'), variance W*H (-1 unknown), position 3*W*H
 * (zero where the pixel was not reprojectable); any may be NULL.  MCPT_E_INVALID before the first
 * accumulation. */
int mcpt_temporal_read(mcpt_ctx *ctx, float *rgb, float *nsamples, float *variance, float *position);
/* The guided a-trous passes over the last accumulated frame (p == NULL: the guided defaults), under the
 * camera it was accumulated at; the mcpt_denoised_* readers and mcpt_denoised_variance_read serve the
 * result. */
int mcpt_temporal_denoise(mcpt_ctx *ctx, const mcpt_denoise_guided_params *p);
/* The same kernel over host images (the counterpart of mcpt_denoise_guided_run; needs neither a scene
 * nor a film).  Current frame: rgb / position / normal 3*w*h, samples / variance / depth w*h.  History:
 * hcol {r, g, b, N}, hpos {X, v}, hnrm {n, depth}, 4*w*h each, as a previous call returned them (all
 * zero: none).  Out: col {r, g, b, valid} 4*w*h, vl {variance, luminance} 2*w*h, and the new history. */
int mcpt_temporal_run(mcpt_ctx *ctx, uint32_t w, uint32_t h, const float *rgb, const uint32_t *samples,
                      const float *variance, const float *position, const float *normal, const float *depth,
                      const float *hcol, const float *hpos, const float *hnrm, const float *vp_prev16,
                      const mcpt_temporal_params *p, float *out_col, float *out_vl, float *out_hcol, float *out_hpos,
                      float *out_hnrm);
/* Device bytes held for the temporal stage (0 until the first mcpt_film_temporal) and the device time
 * (ms) of the last k_temporal launch. */
int64_t mcpt_debug_temporal_bytes(const mcpt_ctx *ctx);
int mcpt_debug_temporal_ms(const mcpt_ctx *ctx, float *out1);
/* ---- spatial variance estimate: a variance of the mean luminance for pixels
 * the path slots give none -- every pixel of a one-slot render, pixels scattered in from another
 * context, host frames -- from the frame itself, as SVGF's spatial fallback does (Schied et al. 2017,
 * 4.2).  Opt-in: a context that never calls these launches nothing for them and every entry point above
 * computes what it always did, the one-slot refusal of mcpt_film_denoise_guided and the one-slot
 * "variance unknown" of mcpt_film_temporal included.
 *
 * Of a valid pixel p without a known variance, over the valid taps q of the (2 radius + 1)^2 window:
 *   e = 1 at p, else the filter's edge-stopping factor without its colour term (sigma_normal,
 *   sigma_albedo, sigma_depth);  d = l(q) - l(p)
 *   m = sum e d / sum e;  var = max(sum e d^2 / sum e - m^2, 0);  neff = (sum e)^2 / sum e^2
 *   v = var neff / (neff - 1), known if neff >= min_neff and v is a finite number >= 0, else -1
 * A known variance is kept; an invalid pixel stays at -1.  A constant window gives exactly 0, and
 * radiance scaled by 2^k scales v by 4^k exactly.  The estimate is the variance among the neighbours'
 * means: it assumes the window's pixels hold about the centre's sample count. */
typedef struct mcpt_variance_params {
    int32_t radius;                                  /* 1..3 */
    float sigma_normal, sigma_albedo, sigma_depth;   /* <= 0 disables the term */
    float min_neff;                                  /* >= 1 */
} mcpt_variance_params;
int mcpt_variance_default_params(mcpt_variance_params *p);
/* The estimate over host images as mcpt_denoise_guided_run takes them (needs neither a scene nor a
 * film): variance (w*h floats, a value outside [0, FLT_MAX] is "unknown") may be NULL (none known);
 * out_variance: w*h floats, the known inputs unchanged, the estimate elsewhere, -1 where unknown. */
int mcpt_variance_run(mcpt_ctx *ctx, uint32_t w, uint32_t h, const float *rgb, const uint32_t *samples,
                      const float *variance, const float *albedo, const float *normal, const float *depth,
                      const mcpt_variance_params *p, float *out_variance);
/* p != NULL: mcpt_film_denoise_guided and mcpt_film_temporal fill the variances they do not know with
 * the estimate over the current film frame (exactly mcpt_variance_run's values for the film's means, the
 * guides' means and v = se^2 where the slots give one); p == NULL (the default): off.
 *   mcpt_film_denoise_guided: with >= 2 path slots pixels of fewer than 2 slots with samples and
 *     scattered-in pixels are filled; with 1 slot it is no longer refused, runs no mcpt_film_error
 *     (but still needs no paths in flight), and every variance is the estimate.
 *   mcpt_film_temporal: v_c is se^2 where the slots give one, else the estimate.  It forms them in
 *     the filter's planes, so the last denoised frame is forgotten (mcpt_denoised_* return
 *     MCPT_E_INVALID until the next denoise).
 * mcpt_denoise_guided_run and mcpt_temporal_run are unchanged: compose them with mcpt_variance_run.
 * The setting survives film clears, resizes, seed and slot changes.  MCPT_E_INVALID (radius outside
 * 1..3, a sigma that is not finite, min_neff below 1 or not finite) leaves the previous setting. */
int mcpt_set_variance_fill(mcpt_ctx *ctx, const mcpt_variance_params *p);
/* Device time (ms) of the last k_variance_spatial launch.  (Where it runs inside a film denoise, the
 * plane set-up time of mcpt_debug_denoise_ms includes it.) */
int mcpt_debug_variance_ms(const mcpt_ctx *ctx, float *out1);
/* ---- emissive materials: a per-material table of emitted radiance.  A path
 * collects the emission of the surface it hit exactly when the logic stage lets it continue into the
 * material stage from that hit (a hit, len <= max_depth, a non-zero sample, the roulette survived):
 *   film += Le[material of the hit] * beta, beta the throughput the logic stage stores for the path
 * after the vertex's MIS terms and the roulette.  len 1 is the primary hit (beta = 1): the term the
 * reference leaves at zero (wavefront_kernels.cu:132).  Two-sided (emissive_L has no normal test).
 * Emitters are not sampled as lights: paths, random draws and ray counts are those of the same
 * scene without emission, and only the film differs.  Opt-in: a context without a table, or with an
 * all-zero one, launches the kernels it launched before.
 *
 * mcpt_set_material_emission installs rgb (3 * nmat floats of radiance, copied); NULL removes the
 * table.  MCPT_E_INVALID, the installed table staying: no scene, nmat different from the uploaded
 * scene's, an entry that is negative or not finite.  Values that differ bitwise from the installed
 * ones mark the film stale as mcpt_camera_set with a different camera does (cleared by the next
 * iteration unless MCPT_FLAG_NO_AUTO_CLEAR) and drop the temporal history; the guide buffers stay
 * valid.  Identical values do nothing.  mcpt_scene_update_geometry* keeps the table (it is keyed by
 * material id, not by triangle); a scene upload drops it.  mcpt_stage_run(MCPT_STAGE_LOGIC) applies it.
 * mcpt_material_emission_read copies the table (rgb may be NULL) and its size; it returns the number
 * of materials with a non-zero entry, 0 with *nmat = 0 when no table is installed, or an error code. */
int mcpt_set_material_emission(mcpt_ctx *ctx, int32_t nmat, const float *rgb);
int mcpt_material_emission_read(mcpt_ctx *ctx, float *rgb, int32_t *nmat);
/* ---- emitter sampling: emissive triangles sampled as lights.  Off by default.
 * Active = switched on and a non-empty emitter table (some triangle of non-zero area has an emissive
 * material); otherwise the context launches the kernels and renders the films it did before.  While
 * active, every material evaluation draws one emitter sample (a triangle by its share of area x
 * luminance(Le), a uniform point on it) and traces a shadow ray that ends just short of that point;
 * the logic stage adds the sample's term where it adds the light sample's, and collects emission
 * (section 16) at the primary hit only.  No MIS between the two: a clean split.  Paths, the other
 * random draws and the five counts of mcpt_debug_ray_counts are those of the same scene without
 * sampling.  mcpt_stage_run always runs with sampling off.
 *
 * mcpt_set_emitter_sampling: on != 0 builds the emitter table of the uploaded scene (none: when one is
 * uploaded and its emission installed) and rebuilds it when mcpt_set_material_emission changes the
 * emission or mcpt_scene_update_geometry* moves the triangles; a scene upload drops it.  Turning the
 * switch on or off, and a rebuild that changes the table bitwise, mark the film stale and drop the
 * temporal history as mcpt_set_material_emission does; the same value again does nothing.  Turning it
 * on without an emissive triangle is no error: sampling is then inactive.
 * mcpt_emitter_table_read: the table's entries in ascending scene triangle id; cdf, pick and tri_id
 * (each *n entries; any may be NULL) and *n (0: no table).  pick[k] = cdf[k] - cdf[k-1] in fp32.
 * mcpt_debug_emitter_stats: out4 = entries, total weight (sum of area x luminance), emitter rays made
 * since the last film clear, the last table build's milliseconds; returns 1 while sampling is active,
 * 0 while it is not, or an error code. */
int mcpt_set_emitter_sampling(mcpt_ctx *ctx, int32_t on);
int mcpt_emitter_table_read(mcpt_ctx *ctx, float *cdf, float *pick, uint32_t *tri_id, int32_t *n);
int mcpt_debug_emitter_stats(const mcpt_ctx *ctx, double *out4);
/* ---- emitter MIS: multiple importance sampling between the emitter sample and
 * collected emission.  A switch beside emitter sampling, off by default, in effect only while emitter
 * sampling is active and the switch is on; otherwise the context launches the kernels and renders the
 * films it did before.  While in effect the emitter sample's term carries the power-heuristic weight of
 * its area pdf (as a solid angle) against the BRDF's pdf of its direction, and a path collects emission
 * at every vertex again (section 16's condition), at len >= 2 weighted by the power heuristic of the
 * pdf its direction had as the previous vertex's continuation sample against the pdf the emitter sample
 * has for the point hit; the primary hit collects with weight 1.  Paths, rays, random draws and every ray
 * count, emitter rays included, are those of emitter sampling without MIS; only the film differs.  The
 * two pdfs are taken from ray origins 0.009 apart along the normal (the light rays' and the extension
 * rays' offsets), so the weights sum to one only up to that offset.
 *
 * mcpt_set_emitter_mis: turning the switch on or off while emitter sampling is active marks the film
 * stale and drops the temporal history as mcpt_set_emitter_sampling does; the same value again, and any
 * change while sampling is not active, does nothing beyond storing the switch.  It survives scene
 * uploads, as the sampling switch does.  mcpt_stage_run is unaffected.
 * mcpt_debug_emitter_mis: 1 while MIS is in effect, 0 while it is not, or an error code. */
int mcpt_set_emitter_mis(mcpt_ctx *ctx, int32_t on);
int mcpt_debug_emitter_mis(const mcpt_ctx *ctx);
/* ---- base-colour textures: per-hit albedo from a texture lookup in the material
 * stage.  For a hit with Moller-Trumbore u, v and w = (1 - u) - v on a triangle with corner uvs uv0, uv1,
 * uv2:
 *   tc   = (u * uv1 + v * uv2) + w * uv0         fp32 per component, this order (Triangle.cu:79)
 *   T    = the bilinear lookup of the material's texture at tc: normalised coordinates, wrap addressing,
 *          8-bit fractional weights, texel = byte / 255 correctly rounded, rgb only (dTexture.cu:107-117)
 *   base = base_factor * T                        one fp32 multiply per channel (the glTF rule)
 * and the BRDF's f and pdf of every part of the material stage, the emitter sample's and MIS's BRDF pdf
 * use this base.  Fresnel stays per material, and so do roughness and metallic unless a
 * metallic-roughness texture is installed (section 20, below).  Row 0 of a texture is v in
 * [0, 1 / h): glTF's orientation, no flip.  Texels are used as stored (the reference has no sRGB decode)
 * unless the texture is flagged MCPT_TEX_SRGB (section 22, below), and alpha is ignored.  Texels arrive
 * decoded: mcpt_image_read_png* reads a PNG file or payload into them; other codecs are out of scope.
 * Paths, random draws, ray counts, emission and every table do not depend on the textures; while a set is
 * in effect the albedo guide (mcpt_guides_render) accumulates the same base at the first hit.  Opt-in: a
 * context without a set, or with one whose every material index is -1, launches the kernels it launched
 * before.
 *
 * mcpt_set_material_textures installs a set (everything copied): uv0 / uv1 / uv2, 2 * ntri floats each,
 * the corners' uvs in the uploaded desc's triangle order; textures[k] = {w, h, rgba8} with w * h RGBA8
 * texels, row-major; mat_tex[m] = the texture of material m, or -1.  ntex == 0 or textures == NULL
 * removes the set.  MCPT_E_INVALID, the installed set staying: no scene, ntri or nmat different from the
 * uploaded scene's, a NULL array, an index outside [-1, ntex), w or h outside 1..16384, a NULL texel
 * pointer, 2^31 texels or more in total.  A set that differs bitwise from the installed one marks the film
 * stale and drops the temporal history as mcpt_set_material_emission does, and makes the guide buffers
 * stale (their albedo changes); an identical set does nothing.  mcpt_scene_update_geometry* keeps the set
 * (a rebuild re-orders the device's uv stream); a scene upload drops it.
 * mcpt_stage_run(MCPT_STAGE_MATERIAL) applies it.
 * mcpt_material_textures_read: the set's sizes (*ntri, *ntex, *nmat; all 0: none installed), mat_tex,
 * texture `tex`'s size and texels (ignored when tex < 0; MCPT_E_INVALID when tex >= *ntex) and the uvs in
 * desc order; every output may be NULL.
 * mcpt_texture_sample_run: the lookup alone, out_rgb[3 i ..] = T(uv[2 i], uv[2 i + 1]) for n host uv
 * pairs over a caller image; it needs neither a scene nor a film.
 * mcpt_debug_texture_stats: device bytes the set holds, materials with a texture, and 1 / 0 for whether
 * the textured kernels are in effect (any may be NULL). */
typedef struct mcpt_texture {
    int32_t w, h;
    const uint8_t *rgba8;
} mcpt_texture;
int mcpt_set_material_textures(mcpt_ctx *ctx, int32_t ntri, const float *uv0, const float *uv1, const float *uv2,
                               int32_t ntex, const mcpt_texture *textures, int32_t nmat, const int32_t *mat_tex);
int mcpt_material_textures_read(mcpt_ctx *ctx, int32_t *ntri, int32_t *ntex, int32_t *nmat, int32_t *mat_tex,
                                int32_t tex, int32_t *w, int32_t *h, uint8_t *rgba8, float *uv0, float *uv1,
                                float *uv2);
int mcpt_texture_sample_run(mcpt_ctx *ctx, int32_t w, int32_t h, const uint8_t *rgba8, uint32_t n, const float *uv,
                            float *out_rgb);
int mcpt_debug_texture_stats(const mcpt_ctx *ctx, uint64_t *bytes, int32_t *textured_materials, int32_t *in_effect);
/* ---- metallic-roughness textures: per-hit roughness and metallic from a second
 * lookup at the same texture coordinate tc, in a texture of the same list:
 *   T     = the section-19 lookup of the material's metallic-roughness texture at tc, unchanged, over rgb
 *   rough = max(rough_factor * T.g, 0.00001)       one fp32 multiply, then the clamp every roughness gets
 *   metal = metal_factor * T.b                     one fp32 multiply
 * (the glTF rule: factor times texel; rough_factor is the material's stored roughness, before the clamp).
 * R and A are ignored; texels are used as stored.  A material whose MR index is -1 keeps its factors.  The
 * two textures of a material are independent: either, both or none, of any two sizes.  Every part of the
 * material stage reads the textured values: the continuation, light and BRDF samples, the emitter sample's
 * f and the MIS weight's BRDF pdf.  Unlike the base colour, roughness and metallic decide whether a
 * continuation sample is valid (f == 0 or pdf == 0 ends the path), so ray counts depend on the set at every
 * depth.  The albedo guide stays base colour only.
 *
 * mcpt_set_material_texture_maps is mcpt_set_material_textures with a second index array: mat_mr[m] = the
 * metallic-roughness texture of material m in the same list, or -1; mat_mr == NULL means all -1, and
 * mcpt_set_material_textures is this call with NULL.  Every rule of that call holds, for both arrays: an
 * index outside [-1, ntex) in either is refused, a bitwise-identical set (mat_mr included) does nothing, a
 * differing one marks the film stale, drops the temporal history and makes the guides stale unless neither
 * set textures a material in either array.  A set with an MR-textured material launches k_material's
 * metallic-roughness instantiations; a set with base-colour textures only, or none, launches what it
 * launched before.
 * mcpt_material_mr_read: *nmat (0: no set installed) and the nmat MR indices (either may be NULL).
 * mcpt_debug_texture_mr_stats: materials with an MR texture, and 1 / 0 for whether the metallic-roughness
 * kernels are in effect (either may be NULL).  mcpt_debug_texture_stats' in_effect is 1 whenever either
 * kind of textured kernel is. */
int mcpt_set_material_texture_maps(mcpt_ctx *ctx, int32_t ntri, const float *uv0, const float *uv1, const float *uv2,
                                   int32_t ntex, const mcpt_texture *textures, int32_t nmat, const int32_t *mat_tex,
                                   const int32_t *mat_mr);
int mcpt_material_mr_read(mcpt_ctx *ctx, int32_t *nmat, int32_t *mat_mr);
int mcpt_debug_texture_mr_stats(const mcpt_ctx *ctx, int32_t *mr_materials, int32_t *mr_in_effect);
/* ---- normal-map textures: per-hit shading normals from a tangent-space lookup at
 * the same texture coordinate tc, in a texture of the same list.  For a hit on a triangle with vertex
 * normals N_i and vertex tangents (T_i, s_i), i = 0, 1, 2, all fp32 in this order:
 *   t   = the section-19 lookup of the material's normal texture at tc, unchanged, over rgb
 *   c.x = (2 t.x - 1) * scale    c.y = (2 t.y - 1) * scale    c.z = 2 t.z - 1         (glTF: z is "up")
 *   B_i = cross(N_i, T_i) * s_i                                                          glTF's bitangent
 *   m_i = (T_i * c.x + B_i * c.y) + N_i * c.z                                            per vertex
 *   nrm = normalize(normalize((m_1 * u + m_2 * v) + m_0 * w))           the hit record's two lines, on m_i
 * The perturbation is applied to the three vertex normals before the hit record interpolates them;
 * interpolation is linear, so this is the usual perturbation of the interpolated frame.  glTF's inner
 * normalize(c) is left out (a positive scalar the hit record's normalisation removes).  A material whose
 * normal index is -1 keeps N_i.  Texels are used as stored; alpha is ignored.  nrm stands for the hit's
 * normal everywhere the material stage reads it: the sampling frames, every f and pdf, the emitter sample
 * and its MIS pdf, and the offsets of the ray origins.  There is no separate geometric normal: a strong
 * perturbation can let light leak through a surface (DESIGN.md names a geometric-normal guard as a
 * follow-up).  Ray counts depend on the set at every depth.  The first-hit normal guide accumulates nrm; the
 * albedo guide is unchanged.
 *
 * mcpt_texture_set describes a whole set; NULL means absent.  ntri .. mat_mr are the arguments of
 * mcpt_set_material_texture_maps.  tan0 / tan1 / tan2: 4 ntri floats each, {T.x, T.y, T.z, s} of corner 0 /
 * 1 / 2 per triangle, in the uploaded desc's triangle order (mcpt_tangents_from_uv makes them; all three or
 * none).  mat_nrm[m]: the normal texture of material m in the same list, or -1 (NULL: all -1).  nrm_scale:
 * one float per material (NULL: all 1).
 * mcpt_set_material_texture_set installs it.  mcpt_set_material_textures and mcpt_set_material_texture_maps
 * are this call with the new fields NULL, and behave as before.  Every rule of those calls holds for the new
 * arrays: everything is copied and checked before anything changes, MCPT_E_INVALID leaves the installed
 * set, a bitwise-identical set (the new fields and their absence included) does nothing, a differing one
 * marks the film stale, drops the temporal history and makes the guides stale (unless it differs only in
 * normal-map fields that no lookup reads: their presence, the scale of a material without a normal map, the
 * tangents while no material has one; such a set is installed and read back, nothing else), a geometry update keeps the
 * set (a rebuild permutes the tangent stream with the uv stream), an upload drops it.  Refused beyond the
 * older calls' refusals: a mat_nrm index outside [-1, ntex), a non-negative mat_nrm entry without tangents,
 * a non-finite nrm_scale or tangent component, one or two of the three tangent arrays.
 * A set with a normal-mapped material launches k_material's normal-map instantiations (base colour, MR and
 * normal per material); every other set launches what it launched before.
 * mcpt_material_normal_read: *nmat (0: no set installed, or one installed without any of the new fields)
 * and *ntri_tan (the triangles the installed tangents cover: 0 without tangents), then whichever of mat_nrm
 * (nmat), nrm_scale (nmat), tan0 / tan1 / tan2 (4 ntri_tan floats each) is not NULL.
 * mcpt_debug_texture_normal_stats: materials with a normal map, and 1 / 0 for whether the normal-map kernels
 * are in effect (either may be NULL).  mcpt_debug_texture_stats' in_effect is 1 whenever any textured level
 * is launched. */
typedef struct mcpt_texture_set {
    int32_t ntri;
    const float *uv0, *uv1, *uv2;
    const float *tan0, *tan1, *tan2;
    int32_t ntex;
    const mcpt_texture *textures;
    int32_t nmat;
    const int32_t *mat_tex, *mat_mr, *mat_nrm;
    const float *nrm_scale;
    const uint32_t *tex_flags; /* section 22: ntex words of MCPT_TEX_*, NULL: all 0 */
} mcpt_texture_set;
int mcpt_set_material_texture_set(mcpt_ctx *ctx, const mcpt_texture_set *set);
int mcpt_material_normal_read(mcpt_ctx *ctx, int32_t *nmat, int32_t *ntri_tan, int32_t *mat_nrm, float *nrm_scale, float *tan0,
                              float *tan1, float *tan2);
int mcpt_debug_texture_normal_stats(const mcpt_ctx *ctx, int32_t *nrm_materials, int32_t *nrm_in_effect);
/* ---- sRGB base colour: glTF base-colour images are sRGB-encoded.  A texture whose
 * flag word has MCPT_TEX_SRGB is decoded when, and only when, it is read as a base colour:
 *   texel = L[c]                                  in place of c / 255, per channel, before the bilinear filter
 * with L a table of 256 floats: x = c / 255 in double, L[c] = x / 12.92 for x <= 0.04045 (bytes 0..10), else
 * ((x + 0.055) / 1.055)^2.4 (bytes 11..255), rounded to float; the rest of the section-19 lookup is unchanged.
 * Metallic-roughness and normal lookups never decode, whatever the texture's flag; alpha is ignored.
 *
 * mcpt_texture_set::tex_flags: ntex words, NULL meaning all 0; bit 0 is MCPT_TEX_SRGB.  The two older install
 * calls pass NULL.  Every rule of mcpt_set_material_texture_set holds for the field: an unknown bit is
 * MCPT_E_INVALID and the installed set stays; a bitwise-identical set (the field and its absence included) does
 * nothing; a differing one marks the film stale, drops the temporal history and makes the guides stale, unless
 * it differs only in flags no base-colour lookup reads (the field's presence, the flag of a texture no
 * base-colour slot uses): such a set is installed and read back, nothing else.
 * A set with a material whose base-colour texture is flagged launches k_material's sRGB instantiations (base
 * colour with the decode, MR and normal per material) and the albedo guide accumulates the decoded colour; every
 * other set launches what it launched before.
 * mcpt_material_texture_flags_read: *ntex (0: no set installed, or one installed without tex_flags) and the
 * flag words (either may be NULL).
 * mcpt_debug_texture_srgb_stats: materials whose base-colour texture is flagged, and 1 / 0 for whether the
 * sRGB kernels are in effect (either may be NULL).
 * mcpt_texture_sample_run_ex: mcpt_texture_sample_run with a flag word for the image: with MCPT_TEX_SRGB the
 * lookup decodes every texel through the table (the base-colour lookup of a flagged texture); an unknown bit is
 * MCPT_E_INVALID.  mcpt_texture_sample_run is this call with 0. */
#define MCPT_TEX_SRGB 1u
int mcpt_material_texture_flags_read(mcpt_ctx *ctx, int32_t *ntex, uint32_t *tex_flags);
int mcpt_debug_texture_srgb_stats(const mcpt_ctx *ctx, int32_t *srgb_materials, int32_t *srgb_in_effect);
int mcpt_texture_sample_run_ex(mcpt_ctx *ctx, int32_t w, int32_t h, const uint8_t *rgba8, uint32_t flags,
                               uint32_t n, const float *uv, float *out_rgb);
/* Vertex tangents from texture coordinates (host/tangents.cpp; no device call).  Per triangle, in double on
 * the float inputs and in this order:
 *   e1 = v1 - v0, e2 = v2 - v0;  (du1, dv1) = uv1 - uv0, (du2, dv2) = uv2 - uv0
 *   det = du1 * dv2 - du2 * dv1;  r = 1 / det
 *   Tt = (e1 * dv2 - e2 * dv1) * r        Bt = (e2 * du1 - e1 * du2) * r
 * and per corner i with normal N_i (dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z):
 *   q = Tt - N_i * dot(N_i, Tt);  l = sqrt(dot(q, q));  T_i = q / l
 *   s_i = -1 if dot(cross(N_i, T_i), Bt) < 0, else +1
 * rounded to float into tan_i[4 t ..] = {T_i, s_i}.  Where det is 0 or not finite, or l is 0 or not finite:
 * T_i = normalize(cross(N_i, e_k)), e_k the coordinate axis of N_i's smallest component in magnitude (the
 * first such on a tie), or (1, 0, 0) where that cross has no finite non-zero length; s_i = +1.
 * Arrays: 3 ntri floats (v, n), 2 ntri (uv), 4 ntri (tan).  MCPT_E_INVALID on a NULL array or ntri < 0. */
int mcpt_tangents_from_uv(int32_t ntri, const float *v0, const float *v1, const float *v2, const float *n0, const float *n1,
                          const float *n2, const float *uv0, const float *uv1, const float *uv2, float *tan0, float *tan1,
                          float *tan2);
int mcpt_sync(mcpt_ctx *ctx);
int mcpt_device_name(mcpt_ctx *ctx, char *buf, int32_t len);
/* diagnostics: rays of the current extension (which=0) or any-hit (which=1) queue, and the
 * device time of the last mcpt_stage_run kernel. */
int mcpt_debug_queue_rays(mcpt_ctx *ctx, int which, float *ray_o, float *ray_d, uint32_t *n_inout);
float mcpt_debug_last_stage_ms(const mcpt_ctx *ctx);
/* Tests: on = 1 runs the traversal with a 2-entry LDS stack per lane (deeper entries in scratch)
 * instead of the 8 / 10 entries the tree depth selects, so that the scratch path is exercised on
 * every tree.  Same results, slower. */
int mcpt_debug_tiny_lds_stack(mcpt_ctx *ctx, int32_t on);
float mcpt_debug_last_build_ms(const mcpt_ctx *ctx);  /* device time of the last GPU BVH build */
/* HRDI tables: an upload whose desc has env_tex but no env_marginal_y / env_conds_y / env_pdf builds
 * them on the device (build_environment_light, light_initialization_kernels.cu:3-161; bit-identical to
 * the host build).  Device time of the last such build, and a copy of the uploaded scene's device
 * tables (any output may be NULL; *flags bit 0 = built on the device, bit 1 = env_cell search guides on). */
float mcpt_debug_last_env_build_ms(const mcpt_ctx *ctx);
int mcpt_debug_env_tables(mcpt_ctx *ctx, float *marginal_y, float *conds_y, float *pdf, int32_t *flags);
/* pair-node numbering of the last uploaded tree: 0 depth-first, 1 depth-first by sibling pairs,
 * 2 breadth-first, 3 line pairs (a node and its larger-area child per 128-B line, pad nodes where a
 * node has no interior child; opt-in) (default 2 for trees of <= 2 MiB of nodes, else 0;
 * MCPT_SIBLING_LAYOUT=0/1/2/3 at upload forces one; inputs that are not a tree -- a shared child --
 * always get 0). */
int mcpt_debug_node_layout(const mcpt_ctx *ctx);
/* Tests: the child-pair tree of the last upload, read back from the device.
 *   nodes: 16 floats per pair node, 4 x float4: per axis (min child 0, min child 1, max child 0,
 *     max child 1), then (ref 0, ref 1, margin 0, margin 1) -- refs as int32 bits: >= 0 a pair
 *     node, < 0 a leaf (bits 0..23 first triangle record, bits 24..26 count - 1), -1 no child (pad
 *     nodes of layout 3) -- with the culling margins as the upload left them.  A 4-wide upload
 *     (MCPT_BVH_WIDTH=4) collapses this array; it is reported unchanged.
 *   tris: 4 * tri_f4 floats per triangle record in storage order ((v0.xyz, e1.x) (e1.yz, e2.xy)
 *     (e2.z, id, -, -)): scene order for a host tree, Morton order for a device-built one.
 * Either may be NULL (sizes only: read info first).  An empty scene reports npairs = ntri = 0 and
 * root_ref 0; a tree that is one leaf reports npairs = 0 and a negative root_ref. */
typedef struct mcpt_bvh_info {
    int32_t npairs;      /* pair nodes in `nodes` (pads of layout 3 included) */
    int32_t root_ref;    /* ref of the root: a pair node or, for a single-leaf tree, a leaf */
    int32_t depth;       /* the largest number of pair nodes on a root-to-leaf path as the upload took
                          * it (the margin passes and the traversal stack are sized by it) */
    int32_t width;       /* node width the traversal uses (2 or 4) */
    int32_t layout;      /* mcpt_debug_node_layout (host numbering; 0 for a device-built tree) */
    int32_t ntri;        /* triangle records */
    int32_t tri_f4;      /* float4 per triangle record */
    int32_t gpu_built;   /* 1: built by mcpt_scene_upload_gpu_bvh */
    int32_t rounds;      /* clustering rounds of a PLOC build, else 0 */
    float root_mn[3], root_mx[3]; /* the root box */
    float cull_p;        /* the far coefficient P of the culling bound */
} mcpt_bvh_info;
int mcpt_debug_bvh_read(mcpt_ctx *ctx, float *nodes, float *tris, mcpt_bvh_info *info);
/* any-hit occluder cache: any-hit rays resolved by it since the film was
 * last cleared (counted in shadow_rays / vis_rays as traced rays; they skip the traversal), and
 * whether the uploaded scene has the cache (MCPT_OCC_G=0 at upload turns it off). */
int mcpt_debug_occ_stats(const mcpt_ctx *ctx, uint64_t *resolved, int32_t *enabled);
/* Complete keys of the occluder table (MCPT_OCC_COMPLETE=0 at upload turns them
 * off), 4 values: keys of the uploaded scene whose entry lists every triangle a ray of the key can be
 * accepted on; since the last film clear, any-hit rays such entries resolved as unoccluded (counted as
 * any-hit rays, neither as traversed nor in mcpt_debug_occ_stats' count) and as occluded (part of that
 * count); and the milliseconds the upload spent building the lists. */
int mcpt_debug_occ_complete_stats(const mcpt_ctx *ctx, double *out4);
/* Ray counts since the last film clear (5 values): extension rays, of them traversed by k_trace
 * (the rest: NaN / zero directions and root-box misses resolved where the ray was made), any-hit
 * (shadow + BRDF visibility) rays, of them traversed, and of them resolved by the occluder cache. */
int mcpt_debug_ray_counts(const mcpt_ctx *ctx, uint64_t *out);
/* Primary-hit candidate table (MCPT_PRIMARY_HITS=0 at context creation turns it
 * off), 4 values: pixels with a candidate list and pixels without one (overflow or no bound) in the
 * current table, primary rays resolved from the table since the last film clear (they count as
 * extension rays, not as traversed ones), and the last table build's milliseconds.  Returns the
 * number of table builds of the context so far (a film clear alone never rebuilds), < 0 on error. */
int mcpt_debug_primary_stats(const mcpt_ctx *ctx, double *out4);
/* mcpt_set_skip_discarded, 4 values since the last film clear: [0] extension rays counted but not
 * made (whether or not they would have entered the scene's box), [1] any-hit rays likewise, [2]
 * material evaluations not run (paths ended one vertex short of max_depth + 1: each is one of [0]
 * and one or two of [1]; [0] - [2] are the roulette's), and, counted only while the switch is off,
 * [3] the extension rays of such paths that were resolved in place, i.e. that the switch would not
 * have saved the traversal. */
int mcpt_debug_discard_stats(const mcpt_ctx *ctx, uint64_t *out4);
/* The traversal's loop-phase counts, recorded by the counting build (mcpt_set_work_counters on)
 * since the last film clear or reset (reset = 1 starts a new count after reading): out12[0] loop
 * trips, [1] refills, [2] lanes refilled, [3] node-phase wave iterations, [4] triangle phases,
 * [5] lanes testing a triangle in them, [6] / [7] / [8] lanes with node work / a parked leaf / no
 * ray at a trip's start, [9] trips in which a lane finished its ray, [10] node-phase iterations in
 * which a lane popped its stack; [11] 0.  With the node steps of mcpt_stage_stats they split the
 * lane utilisation by phase, and with the kernel's ISA sections its VALU (tools/trace_attrib.py).
 * Returns the number of words filled (11), 0 when none were recorded. */
int mcpt_debug_trace_profile(mcpt_ctx *ctx, uint64_t *out12, int reset);
/* k_shade's per-section wave entries and active lanes, summed over the
 * launches since the last reset, in a build with -DMCPT_DIAG_SHADE: out[2k] entries and out[2k+1]
 * lanes of section k (waves, valid paths, logic, MIS terms, generate, continuing, background), up to
 * n words.  Returns the words available (14); the product build fills zeros and returns 0. */
int mcpt_debug_shade_sections(mcpt_ctx *ctx, uint64_t *out, int n, int reset);
/* diagnostics: the kernels' shared-denominator division (mcpt::quot3, mcpt_core.hpp) on the
 * device for n host pairs: out[i] = a[i] / b[i] as the kernels compute it (must equal IEEE fp32). */
int mcpt_debug_quot(mcpt_ctx *ctx, const float *a, const float *b, uint32_t n, float *out);
/* Measured HBM ceiling for the roofline: a hand-written dwordx4 copy of `bytes`
 * between two device buffers, `iters` launches timed with HIP events; *gbps = (read + write) bytes / s. */
int mcpt_debug_hbm_copy(mcpt_ctx *ctx, uint64_t bytes, uint32_t iters, double *gbps);

/* ---- host scene builder (Scene.cu:24-470, EnvironmentLight.cu:329-452, BVH.cu) ---- */
mcpt_scene *mcpt_scene_new(void);
void mcpt_scene_free(mcpt_scene *s);
int mcpt_scene_load_glb(mcpt_scene *s, const char *path, const float *xform16);  /* xform may be NULL */
int mcpt_scene_add_mesh(mcpt_scene *s, int32_t ntri, const float *v0, const float *v1, const float *v2,
                        const float *n0, const float *n1, const float *n2, const float *base_rgb);
/* Emitted radiance per material (mcpt_set_material_emission takes the array as it is).  mat: a material
 * id as in mcpt_scene_get_desc's mat array, one material per added mesh (glb primitive) in add order;
 * a glb material's is emissiveFactor x KHR_materials_emissive_strength.emissiveStrength (defaults 0, 1).
 * MCPT_E_INVALID: mat out of range, an entry that is negative or not finite.  get: the 3 * nmat floats,
 * owned by the scene (valid until the next mesh is added); *rgb = NULL when every entry is zero.  The
 * scene desc does not carry the table. */
int mcpt_scene_set_material_emission(mcpt_scene *s, int32_t mat, const float *rgb);
int mcpt_scene_get_emission(const mcpt_scene *s, const float **rgb, int32_t *nmat);
/* Base-colour textures (mcpt_set_material_textures takes what the getters return).  The glb reader keeps
 * every primitive's TEXCOORD_0 (a float VEC2 accessor; absent: zeros) through mcpt_scene_transform and the
 * BVH's reordering.  mcpt_scene_load_glb reads nothing else of a material but its base-colour factor;
 * mcpt_scene_load_glb_ex (below) imports the factors, the embedded PNG textures and the tangents as authored.
 * Otherwise texels arrive decoded, through mcpt_scene_set_material_texture (mcpt_image_read_png* decodes a PNG).
 * mcpt_scene_set_mesh_uv: the corners' uvs of material mat's triangles (one material per added mesh), 2
 * floats per triangle in each array, in the order the mesh's triangles were added.
 * mcpt_scene_set_material_texture: attaches a copy of the w x h RGBA8 image (row 0 = v in [0, 1 / h), used
 * as stored -- mcpt_scene_set_material_texture_ex flags sRGB texels -- alpha ignored) to material mat,
 * replacing its previous one (an entry that other slots use too stays theirs: the image is then appended);
 * rgba8 == NULL detaches.
 * MCPT_E_INVALID: mat out of range, w or h outside 1..16384, a NULL uv array.
 * mcpt_scene_get_textures: the textures, *ntex of them (*textures = NULL, *ntex = 0 when no material has
 * one) and the nmat texture indices (-1: none).  mcpt_scene_get_uv: the built scene's uvs, 2 * ntri floats
 * each, in the desc's triangle order.  The pointers are owned by the scene (valid until it changes).  The
 * scene desc does not carry any of this. */
int mcpt_scene_set_mesh_uv(mcpt_scene *s, int32_t mat, const float *uv0, const float *uv1, const float *uv2);
int mcpt_scene_set_material_texture(mcpt_scene *s, int32_t mat, int32_t w, int32_t h, const uint8_t *rgba8);
int mcpt_scene_get_textures(const mcpt_scene *s, const mcpt_texture **textures, int32_t *ntex,
                            const int32_t **mat_tex, int32_t *nmat);
int mcpt_scene_get_uv(const mcpt_scene *s, const float **uv0, const float **uv1, const float **uv2, int32_t *ntri);
/* Metallic-roughness textures (mcpt_set_material_texture_maps takes what the getters
 * return).  mcpt_scene_set_material_mr_texture: attaches a copy of the w x h RGBA8 image to material mat as
 * its metallic-roughness texture (G: roughness, B: metallic; R and A ignored), replacing its previous one;
 * rgba8 == NULL detaches.  The refusals are mcpt_scene_set_material_texture's.  The image joins the list
 * mcpt_scene_get_textures returns, which then hands out that list when a material has a texture of either
 * kind; a scene without MR textures returns what it returned before.
 * mcpt_scene_get_material_mr: the nmat MR indices into that list (-1: none), owned by the scene. */
int mcpt_scene_set_material_mr_texture(mcpt_scene *s, int32_t mat, int32_t w, int32_t h, const uint8_t *rgba8);
int mcpt_scene_get_material_mr(const mcpt_scene *s, const int32_t **mat_mr, int32_t *nmat);
/* Normal maps (mcpt_set_material_texture_set takes what the getters return).
 * mcpt_scene_set_material_normal_texture: attaches a copy of the w x h RGBA8 image to material mat as its
 * tangent-space normal map with the given scale (finite, or refused), replacing its previous one; rgba8 ==
 * NULL detaches.  The other refusals are mcpt_scene_set_material_texture's.  The image joins the one list
 * mcpt_scene_get_textures returns, which hands that list out when a material has a texture of any kind.
 * mcpt_scene_get_material_normal: the nmat normal indices into that list (-1: none) and the nmat scales (1
 * where none was set), owned by the scene.
 * mcpt_scene_get_tangents: the built scene's vertex tangents, mcpt_tangents_from_uv over its vertices,
 * normals and uvs, 4 ntri floats per corner in the desc's triangle order, owned by the scene (valid until
 * the scene changes or is built again). */
int mcpt_scene_set_material_normal_texture(mcpt_scene *s, int32_t mat, int32_t w, int32_t h, const uint8_t *rgba8, float scale);
int mcpt_scene_get_material_normal(const mcpt_scene *s, const int32_t **mat_nrm, const float **nrm_scale, int32_t *nmat);
int mcpt_scene_get_tangents(const mcpt_scene *s, const float **tan0, const float **tan1, const float **tan2, int32_t *ntri);
/* sRGB base colour (mcpt_texture_set::tex_flags takes what the getter returns).
 * mcpt_scene_set_material_texture_ex: mcpt_scene_set_material_texture with the image's MCPT_TEX_* flags
 * (MCPT_TEX_SRGB: the texels are sRGB-encoded and decoded when read as a base colour); an unknown bit is
 * MCPT_E_INVALID.  mcpt_scene_set_material_texture is this call with 0; the MR and normal setters attach
 * unflagged images.
 * mcpt_scene_get_texture_flags: one flag word per texture of the list mcpt_scene_get_textures returns, owned
 * by the scene (valid until it changes). */
int mcpt_scene_set_material_texture_ex(mcpt_scene *s, int32_t mat, int32_t w, int32_t h, const uint8_t *rgba8,
                                       uint32_t flags);
int mcpt_scene_get_texture_flags(const mcpt_scene *s, const uint32_t **tex_flags, int32_t *ntex);
/* glb material import.  mcpt_scene_load_glb_ex is mcpt_scene_load_glb with flags; with 0
 * it is that call, array for array.  An unknown bit is MCPT_E_INVALID.
 *   MCPT_GLB_PBR_FACTORS  roughnessFactor and metallicFactor as authored (glTF's defaults 1 and 1) in place of
 *                         the forced roughness 1 and metallic 0.
 *   MCPT_GLB_TEXTURES     every material's pbrMetallicRoughness.baseColorTexture, .metallicRoughnessTexture and
 *                         normalTexture (with its scale): textures[i].source -> images[j] -> bufferView -> the
 *                         PNG reader, attached as the texture setters attach them; one glTF image becomes one
 *                         entry of the scene's texture list, however many slots use it.  A primitive's TANGENT
 *                         (a float VEC4 accessor) is kept: T' = normalize(M3 T), M3 the node matrix's upper
 *                         3 x 3, s' = s sign(det M3); mcpt_scene_get_tangents returns the authored tangents for
 *                         the triangles that have them and mcpt_tangents_from_uv's for the rest.
 *   MCPT_GLB_SRGB         the images a base-colour slot uses carry MCPT_TEX_SRGB.
 * A slot or image that cannot be honoured does not fail the load: the slot stays empty, the factor still
 * applies, and the report gets a line.  The cases: an image that is not image/png, an image given by uri,
 * texCoord != 0, KHR_texture_transform, a sampler whose wrapS / wrapT is not REPEAT (10497) or absent, an image
 * the PNG reader refuses, an index out of range; and a TANGENT accessor with a zero or non-finite tangent or a
 * handedness other than +-1, whose primitive takes the uv-derived tangents (a line, no count).  Sampler filters
 * are ignored (the lookup is bilinear).
 * mcpt_scene_glb_report: of the last load, counts4 = {images decoded, images skipped, slots attached, slots
 * skipped} and in buf (len bytes, NUL-terminated, truncated) one newline-terminated line per skipped image or
 * slot, naming the material, the slot and the reason; either may be NULL. */
#define MCPT_GLB_PBR_FACTORS 1u
#define MCPT_GLB_TEXTURES 2u
#define MCPT_GLB_SRGB 4u
#define MCPT_GLB_AS_AUTHORED 7u
int mcpt_scene_load_glb_ex(mcpt_scene *s, const char *path, const float *xform16, uint32_t flags);
int mcpt_scene_glb_report(const mcpt_scene *s, int32_t *counts4, char *buf, int32_t len);
int mcpt_scene_set_env_hdr(mcpt_scene *s, const char *path, int32_t mode);
/* flags MCPT_ENV_DEVICE_TABLES: keep the texture only; mcpt_scene_upload then builds the tables on
 * the device (for large maps: the host build is several serial passes over every texel). */
#define MCPT_ENV_DEVICE_TABLES 1
int mcpt_scene_set_env_hdr_ex(mcpt_scene *s, const char *path, int32_t mode, uint32_t flags);
int mcpt_scene_set_env_color(mcpt_scene *s, const float *rgb, float ls);
int mcpt_scene_add_dir_light(mcpt_scene *s, const float *dir, const float *rgb, float ls);
int mcpt_scene_transform(mcpt_scene *s, const float *xform16);   /* bake a transform into all meshes */
int mcpt_scene_make_proxy(mcpt_scene *s, int32_t config_id, const char *asset_dir); /* SURVEY.md 8d proxies */
int mcpt_scene_build(mcpt_scene *s, int32_t max_prims_in_node);  /* SAH BVH (BVH.cu:84-333) + env tables */
/* BVH builder choice.  Topology is not a parity contract (hits are tree-independent: conservative
 * culling + (t, scene index) ties), so any builder gives identical films.
 *   MCPT_BVH_REFERENCE: BVHAccel's SAH (BVH.cu:84-333) -- 12 buckets on the largest centroid axis,
 *     cost .125 + (n0 A0 + n1 A1) / A; what mcpt_scene_build runs.
 *   MCPT_BVH_SAH3: binned SAH over all three axes (buckets per axis), cost
 *     trav_cost + isect_cost (n0 A0 + n1 A1) / A against a leaf cost isect_cost n. */
#define MCPT_BVH_REFERENCE 0
#define MCPT_BVH_SAH3 1
typedef struct mcpt_bvh_params {
    int32_t builder;      /* MCPT_BVH_* */
    int32_t max_prims;    /* 1..8 triangles per leaf */
    int32_t buckets;      /* SAH3: bins per axis (2..256) */
    float trav_cost;      /* SAH3: cost of a node visit, relative to ... */
    float isect_cost;     /* ... a triangle test */
} mcpt_bvh_params;
int mcpt_scene_build_ex(mcpt_scene *s, const mcpt_bvh_params *p); /* BVH + env tables */
int mcpt_scene_get_desc(const mcpt_scene *s, mcpt_scene_desc *out); /* pointers owned by s */
int mcpt_scene_bvh_depth(const mcpt_scene *s);
int mcpt_camera_make(const mcpt_camera_params *p, mcpt_camera *out);

#ifdef __cplusplus
}
#endif
#endif
