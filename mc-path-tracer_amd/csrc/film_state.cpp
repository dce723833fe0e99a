// film_state.cpp -- the state the wavefront iteration runs on, behind the mcpt_* C ABI (include/mcpt.h):
// the tile set and its ray queues, the film and path streams for a film size, path-slot count and
// layout (allocation, resize, slots, compact, clear), and the film's readers (film view, read, pack /
// unpack / gather, tonemap).  Replaces the reference's Film device state (Film.cu:121-276).  The
// owners are runtime_internal.hpp's RayQueues, TileSet, FilmState and Counters, the sizing rules
// host/film_layout.hpp's; the context and the render loop are runtime.cpp's.
#include "runtime_internal.hpp"

int set_tiles_internal(mcpt_ctx* c, const std::vector<int2>& t) {
    const FilmLayout L = c->layout(t.size());
    if (!c->queues.fits(L)) HIPCHK(c, hipStreamSynchronize(c->stream));  // no launch in flight reads the old queues
    if (!c->queues.ensure(L)) return set_err(c, MCPT_E_NOMEM, "queue allocation failed");
    TileSet& ts = c->tiles;
    if (t.size() > ts.dev.size() && !ts.dev.ensure(t.size()))
        return set_err(c, MCPT_E_HIP, std::string("tile set allocation failed: ") + hipGetErrorString(hipGetLastError()));
    if (!t.empty()) HIPCHK(c, hipMemcpyAsync(ts.dev, t.data(), t.size() * sizeof(int2), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    ts.host = t;
    return MCPT_OK;
}

extern "C" {

int mcpt_film_clear(mcpt_ctx* c) {
    if (!c || !c->film.allocated) return set_err(c, MCPT_E_INVALID, "film not allocated");
    HIPCHK(c, hipSetDevice(c->device));
    FilmState& f = c->film;
    ClearArgs a{f.flags, f.samples, f.Ld, (uint32_t)f.L.paths, (uint32_t)f.L.npx};
    launch_clear(a, c->stream);
    HIPCHK(c, hipGetLastError());
    if (f.L.compact) {  // the W x H film also holds pixels unpacked from other contexts (mcpt_film_unpack_tiles)
        HIPCHK(c, hipMemsetAsync(f.sum_Ld, 0, f.L.npix * sizeof(float4), c->stream));
        HIPCHK(c, hipMemsetAsync(f.sum_samples, 0, f.L.npix * sizeof(uint32_t), c->stream));
    }
    if (f.blk_done) HIPCHK(c, hipMemsetAsync(f.blk_done, 0, f.L.blk_done_n, c->stream));
    // The occluder cache starts every film from the same table -- the upload's pre-fill, or empty --
    // with its lookup gate on, so a frame's work never depends on the frames before it.  (It only
    // ever chooses which triangle an any-hit ray tests first; the 96 MB copy takes ~0.04 ms.)
    if (c->scene.dev.occ) {
        if (c->scene.occ_init) {  // the upload's pre-filled table (scene-derived), the same for every frame
            HIPCHK(c, hipMemcpyAsync(c->scene.dev.occ, c->scene.occ_init, c->scene.occ_entries_n * sizeof(uint32_t),
                                     hipMemcpyDeviceToDevice, c->stream));
            static const uint32_t warm[kOccGateWords] = {0u, 0u, 1u};
            HIPCHK(c, hipMemcpyAsync(c->scene.dev.occ_gate, warm, sizeof(warm), hipMemcpyHostToDevice, c->stream));
        } else {
            HIPCHK(c, hipMemsetAsync(c->scene.dev.occ, 0xff, c->scene.occ_entries_n * sizeof(uint32_t), c->stream));
            HIPCHK(c, hipMemsetAsync(c->scene.dev.occ_gate, 0, kOccGateWords * sizeof(uint32_t), c->stream));
        }
    }
    c->film_stale = false;
    f.unpacked.clear();
    HIPCHK(c, hipMemsetAsync(c->cnt.dev, 0, sizeof(CounterBlock), c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    memset(&c->cnt.totals, 0, sizeof(c->cnt.totals));  // the counters are now zero on the device too
    memset(c->cnt.phase_base, 0, sizeof(c->cnt.phase_base));
    c->cnt.totals_ok = true;
    return MCPT_OK;
}

// Film state for the current film size, path slots, layout and tile set (FilmState).  Frees the
// previous film state first; the caller clears the film.
static int alloc_film_state(mcpt_ctx* c) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    FilmState& f = c->film;
    f.release();
    const FilmLayout L = c->layout(c->tiles.host.size());
    if (const char* e = path_count_error(L.npx, L.slots)) return set_err(c, MCPT_E_INVALID, e);
    if (!f.alloc(L)) return set_err(c, MCPT_E_NOMEM, std::string("hipMalloc: ") + hipGetErrorString(hipGetLastError()));
    HIPCHK(c, hipMemset(f.hit_tri, 0xff, L.paths * sizeof(int32_t)));
    HIPCHK(c, hipMemset(f.vis, 0, 2 * L.paths));
    f.allocated = true;
    return MCPT_OK;
}

// (mcpt_set_path_slots re-sizes the full layout's film through this: the sample budget stays)
static int film_resize(mcpt_ctx* c, uint32_t w, uint32_t h, uint32_t tw, uint32_t th) {
    if (!c) return set_err(c, MCPT_E_INVALID, "bad film size");
    if (const char* e = film_size_error(w, h, tw, th)) return set_err(c, MCPT_E_INVALID, e);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->film.release();
    c->guides = Guides{};  // guide sums and filter planes: they belong to the film size
    c->dn = Denoise{};
    c->W = w; c->H = h; c->tile_w = tw; c->tile_h = th;
    c->queues.release();  // re-sized for the new tile set below
    int rc = set_tiles_internal(c, TileSet::all(c->layout(0)));
    if (rc) return rc;
    if ((rc = alloc_film_state(c))) return rc;
    return mcpt_film_clear(c);
}
int mcpt_film_resize(mcpt_ctx* c, uint32_t w, uint32_t h, uint32_t tw, uint32_t th) {
    if (!c || w == 0 || h == 0 || tw == 0 || th == 0) return set_err(c, MCPT_E_INVALID, "bad film size");
    if (c->ad.bytes() || c->tp.bytes()) {  // the sample budget, the estimate and the temporal history belong to the film size
        HIPCHK(c, hipSetDevice(c->device));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->ad = Adaptive{};
        c->tp = Temporal{};
    }
    return film_resize(c, w, h, tw, th);
}

// What the queues and the film state of one film size are allocated for
struct FilmSettings {
    std::vector<int2> tiles;
    uint32_t slots;
    bool compact;
};
// New settings under an allocated film: the queues, then the film state, then a film clear.  When an
// allocation fails (e.g. out of memory) the previous settings come back with their (cleared) film and
// the first error is the call's.
static int apply_settings(mcpt_ctx* c, const FilmSettings& want) {
    const FilmSettings old{c->tiles.host, c->slots, c->compact};
    auto attempt = [c](const FilmSettings& s) {
        c->slots = s.slots;
        c->compact = s.compact;
        int rc = set_tiles_internal(c, s.tiles);
        return rc ? rc : alloc_film_state(c);
    };
    if (int rc = attempt(want)) {
        const std::string err = c->err;
        if (attempt(old) == MCPT_OK) (void)mcpt_film_clear(c);
        return set_err(c, rc, err);
    }
    return mcpt_film_clear(c);
}

// A new tile set.  In the compact layout the path state follows the tile set: it is re-allocated and
// the film cleared (a tile listed twice would share its paths: rejected).
static int set_tiles_checked(mcpt_ctx* c, const std::vector<int2>& t) {
    if (!c->compact) {
        for (const int2& x : t)
            if (tile_index(c->film.unpacked, x) >= 0)
                return set_err(c, MCPT_E_INVALID, "a tile of the set holds pixels unpacked from another context: clear the film first");
        return set_tiles_internal(c, t);
    }
    for (size_t i = 0; i < t.size(); i++)
        for (size_t j = 0; j < i; j++)
            if (t[i].x == t[j].x && t[i].y == t[j].y)
                return set_err(c, MCPT_E_INVALID, "compact paths: a tile is listed twice");
    return apply_settings(c, {t, c->slots, c->compact});
}

int mcpt_set_tiles(mcpt_ctx* c, const uint32_t* xy, uint32_t n) {
    if (!c || !c->film.allocated) return set_err(c, MCPT_E_INVALID, "film not allocated");
    HIPCHK(c, hipSetDevice(c->device));
    if (!xy) return set_tiles_checked(c, TileSet::all(c->film.L));
    std::vector<int2> t;
    if (TileSet::parse(xy, n, c->film.L, t) < n) return set_err(c, MCPT_E_INVALID, "tile out of range");
    return set_tiles_checked(c, t);
}

int mcpt_set_compact_paths(mcpt_ctx* c, int32_t on) {
    if (!c) return MCPT_E_INVALID;
    const bool v = on != 0;
    if (v == c->compact) return MCPT_OK;
    if (!c->film.allocated) {  // takes effect with the film's allocation
        c->compact = v;
        return MCPT_OK;
    }
    HIPCHK(c, hipSetDevice(c->device));
    return apply_settings(c, {c->tiles.host, c->slots, v});
}

int mcpt_set_path_slots(mcpt_ctx* c, uint32_t slots) {
    if (!c || slots < 1 || slots > 256) return set_err(c, MCPT_E_INVALID, "path slots must be 1..256");
    if (slots == c->slots) return MCPT_OK;
    if (!c->film.allocated) {
        c->slots = slots;
        return MCPT_OK;
    }
    // check the new size before touching anything: a rejected count leaves the film as it was
    if (const char* e = path_count_error(c->film.L.npx, slots)) return set_err(c, MCPT_E_INVALID, e);
    if (c->compact) {  // the path state of the current tile set (its queues too: their capacity follows the slots)
        HIPCHK(c, hipSetDevice(c->device));
        return apply_settings(c, {c->tiles.host, slots, c->compact});
    }
    // full layout: through film_resize, which also drops the guide sums and filter planes and resets the
    // tile set, and keeps the sample budget and the temporal history
    const uint32_t old = c->slots;
    c->slots = slots;
    int rc = film_resize(c, c->W, c->H, c->tile_w, c->tile_h);  // clears the film
    if (rc != MCPT_OK) {  // e.g. out of memory: back to the old slot count and its (cleared) film
        const std::string err = c->err;
        c->slots = old;
        (void)film_resize(c, c->W, c->H, c->tile_w, c->tile_h);
        return set_err(c, rc, err);
    }
    return MCPT_OK;
}

// The film (dFilm.Ld / samples): the path state's accumulators with one slot per pixel,
// else their per-pixel sum in slot order (k_resolve) -- enqueued on the context stream.
extern "C++" int film_view(mcpt_ctx* c, const float4** Ld, const uint32_t** samples) {
    const FilmState& f = c->film;
    if (!f.L.sum_planes) {
        *Ld = f.Ld;
        *samples = f.samples;
        return MCPT_OK;
    }
    ResolveArgs a{f.Ld, f.samples, f.sum_Ld, f.sum_samples, (uint32_t)f.L.npx, (int)f.L.slots,
                  f.L.compact ? c->tiles.dev.get() : nullptr, (int)c->tile_w, (int)c->tile_h, (int)c->W, (int)c->H};
    launch_resolve(a, c->stream);
    HIPCHK(c, hipGetLastError());
    *Ld = f.sum_Ld;
    *samples = f.sum_samples;
    return MCPT_OK;
}

// Where another context's tile pixels are scattered (mcpt_film_unpack_tiles, mcpt_gather): the
// pixel-indexed accumulators the film view reads beside the context's own tiles
static void unpack_target(mcpt_ctx* c, float4** Ld, uint32_t** samples) {
    const FilmState& f = c->film;
    *Ld = f.L.compact ? f.sum_Ld : f.Ld;
    *samples = f.L.compact ? f.sum_samples : f.samples;
}
static void note_unpacked(mcpt_ctx* c, const std::vector<int2>& t) {
    for (const int2& x : t)
        if (tile_index(c->film.unpacked, x) < 0) c->film.unpacked.push_back(x);
}

int mcpt_film_read(mcpt_ctx* c, float* Ld, uint32_t* samples) {
    if (!c || !c->film.allocated) return set_err(c, MCPT_E_INVALID, "film not allocated");
    HIPCHK(c, hipSetDevice(c->device));
    const float4* fL;
    const uint32_t* fs;
    int rc = film_view(c, &fL, &fs);
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const size_t P = c->film.pixels();
    if (Ld && (rc = read_plane(c, fL, P, Ld, nullptr))) return rc;
    if (samples) HIPCHK(c, hipMemcpy(samples, fs, P * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return MCPT_OK;
}

int mcpt_film_read_device(mcpt_ctx* c, void* dLd, void* dsamples) {
    if (!c || !c->film.allocated) return set_err(c, MCPT_E_INVALID, "film not allocated");
    HIPCHK(c, hipSetDevice(c->device));
    const float4* fL;
    const uint32_t* fs;
    int rc = film_view(c, &fL, &fs);
    if (rc) return rc;
    const size_t P = c->film.pixels();
    if (dLd) HIPCHK(c, hipMemcpyAsync(dLd, fL, P * sizeof(float4), hipMemcpyDeviceToDevice, c->stream));
    if (dsamples) HIPCHK(c, hipMemcpyAsync(dsamples, fs, P * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MCPT_OK;
}

int mcpt_film_pack_tiles(mcpt_ctx* c, void* d_out, uint32_t* npix) {
    if (!c || !c->film.allocated) return set_err(c, MCPT_E_INVALID, "film not allocated");
    const TileSet& ts = c->tiles;
    uint32_t n = (uint32_t)(ts.host.size() * c->tile_w * c->tile_h);
    if (npix) *npix = n;
    if (!d_out) return MCPT_OK;
    HIPCHK(c, hipSetDevice(c->device));
    const float4* fL;
    const uint32_t* fs;
    int rc = film_view(c, &fL, &fs);
    if (rc) return rc;
    PackArgs a{fL, fs, ts.dev, (int)ts.host.size(), (int)c->tile_w, (int)c->tile_h, (int)c->W, (int)c->H, (float4*)d_out};
    if (n) launch_pack(a, c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MCPT_OK;
}

int mcpt_film_unpack_tiles(mcpt_ctx* c, const void* d_in, const uint32_t* xy, uint32_t n) {
    if (!c || !c->film.allocated) return set_err(c, MCPT_E_INVALID, "film not allocated");
    if (n == 0) return MCPT_OK;
    if (!d_in || !xy) return set_err(c, MCPT_E_INVALID, "null argument");
    std::vector<int2> t;
    const uint32_t parsed = TileSet::parse(xy, n, c->film.L, t);  // (the first bad tile decides, in the caller's order)
    for (const int2& x : t)
        if (c->tiles.index_of(x) >= 0)  // the context's own pixels would mix with its other slots
            return set_err(c, MCPT_E_INVALID, "unpack into one of the context's own tiles");
    if (parsed < n) return set_err(c, MCPT_E_INVALID, "tile out of range");
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf<int2> dt;
    if (!dt.ensure(n)) return set_err(c, MCPT_E_HIP, std::string("unpack: ") + hipGetErrorString(hipGetLastError()));
    hipError_t e = hipMemcpyAsync(dt, t.data(), n * sizeof(int2), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        // scattered into slot 0 of the path state (its other slots of a pixel the context never
        // renders stay zero, so the film view's slot sum returns these values); compact layout: into
        // the W x H film, where the film view's resolve writes only the context's own tiles
        float4* tL;
        uint32_t* ts;
        unpack_target(c, &tL, &ts);
        UnpackArgs ua{(const float4*)d_in, dt, (int)n, (int)c->tile_w, (int)c->tile_h, (int)c->W, (int)c->H, tL, ts};
        launch_unpack(ua, c->stream);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    dt.reset();
    if (e != hipSuccess) return set_err(c, MCPT_E_HIP, std::string("unpack: ") + hipGetErrorString(e));
    note_unpacked(c, t);
    return MCPT_OK;
}

// Frame-end gather of a multi-GPU render inside one process (SURVEY.md 8(b) mcpt_gather, 8(e)):
// every context's tile-set pixels, resolved over its path slots and packed 16 B/px, are copied
// device-to-device onto the root's device (hipMemcpyPeerAsync: SDMA over xGMI between MI355X
// dies of a node) and scattered into the root's film accumulators, so the root's film readers
// return the whole frame.  Tile sets must not overlap the root's own tiles (the interleaved
// partition of mcpt/parallel.py); the multi-process form sends the same packed buffers to the
// root over RCCL and scatters them with mcpt_film_unpack_tiles (mcpt/parallel.py).
int mcpt_gather(mcpt_ctx* const* ctxs, int32_t n, int32_t root) {
    if (!ctxs || n < 1 || root < 0 || root >= n || !ctxs[root]) return set_err(nullptr, MCPT_E_INVALID, "bad gather arguments");
    mcpt_ctx* R = ctxs[root];
    for (int32_t i = 0; i < n; i++) {
        mcpt_ctx* c = ctxs[i];
        if (!c || !c->film.allocated) return set_err(R, MCPT_E_INVALID, "gather: a context has no film");
        if (c->W != R->W || c->H != R->H || c->tile_w != R->tile_w || c->tile_h != R->tile_h)
            return set_err(R, MCPT_E_INVALID, "gather: film or tile sizes differ between contexts");
        for (int32_t j = 0; j < i; j++)
            if (ctxs[j] == c) return set_err(R, MCPT_E_INVALID, "gather: a context is listed twice");
        if (c != R)
            for (const int2& x : c->tiles.host)
                if (R->tiles.index_of(x) >= 0) return set_err(R, MCPT_E_INVALID, "gather: a tile set overlaps the root's own tiles");
    }
    for (int32_t i = 0; i < n; i++) {
        mcpt_ctx* c = ctxs[i];
        const std::vector<int2>& tiles = c->tiles.host;
        if (c == R || tiles.empty()) continue;
        const size_t npix = tiles.size() * (size_t)c->tile_w * c->tile_h;
        // pack on the source device (its film view resolves the path slots)
        HIPCHK(R, hipSetDevice(c->device));
        const float4* fL;
        const uint32_t* fs;
        int rc = film_view(c, &fL, &fs);
        if (rc) return set_err(R, rc, c->err);
        DevBuf<float4> src;  // on the source device; dst and dt on the root's: each freed with its device current
        if (!src.ensure(npix)) return set_err(R, MCPT_E_NOMEM, "gather: pack buffer");
        PackArgs pa{fL, fs, c->tiles.dev, (int)tiles.size(), (int)c->tile_w, (int)c->tile_h, (int)c->W, (int)c->H, src};
        launch_pack(pa, c->stream);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        // copy to the root's device and scatter into its accumulators (slot 0; the other slots
        // of pixels the root does not render are zero, so its slot sum returns these values)
        DevBuf<float4> dst;
        DevBuf<int2> dt;
        if (e == hipSuccess) e = hipSetDevice(R->device);
        if (e == hipSuccess && c->device != R->device) {
            // direct xGMI access where the pair supports it; hipMemcpyPeerAsync also works
            // without it (staged), so a refusal here is not an error
            int can = 0;
            if (hipDeviceCanAccessPeer(&can, R->device, c->device) == hipSuccess && can)
                (void)hipDeviceEnablePeerAccess(c->device, 0);
            (void)hipGetLastError();
        }
        if (e == hipSuccess && !(dst.ensure(npix) && dt.ensure(tiles.size()))) e = hipErrorOutOfMemory;
        if (e == hipSuccess)
            e = hipMemcpyPeerAsync(dst, R->device, src, c->device, npix * sizeof(float4), R->stream);
        if (e == hipSuccess)
            e = hipMemcpyAsync(dt, tiles.data(), tiles.size() * sizeof(int2), hipMemcpyHostToDevice, R->stream);
        if (e == hipSuccess) {
            float4* tL;
            uint32_t* ts;
            unpack_target(R, &tL, &ts);
            UnpackArgs ua{dst, dt, (int)tiles.size(), (int)R->tile_w, (int)R->tile_h, (int)R->W, (int)R->H, tL, ts};
            launch_unpack(ua, R->stream);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipStreamSynchronize(R->stream);
        dst.reset();
        dt.reset();
        (void)hipSetDevice(c->device);
        src.reset();
        if (e != hipSuccess) return set_err(R, MCPT_E_HIP, std::string("gather: ") + hipGetErrorString(e));
        note_unpacked(R, tiles);
    }
    (void)hipSetDevice(R->device);
    return MCPT_OK;
}

int mcpt_film_size(const mcpt_ctx* c, uint32_t* w, uint32_t* h) {
    if (!c || !w || !h) return MCPT_E_INVALID;
    if (!c->film.allocated) return set_err(const_cast<mcpt_ctx*>(c), MCPT_E_INVALID, "film not allocated");
    *w = c->W;
    *h = c->H;
    return MCPT_OK;
}

int mcpt_film_tonemap_rgba8(mcpt_ctx* c, float exposure, uint8_t* out) {
    if (!c || !c->film.allocated || !out) return set_err(c, MCPT_E_INVALID, "bad argument");
    HIPCHK(c, hipSetDevice(c->device));
    const float4* fL;
    const uint32_t* fs;
    int rc = film_view(c, &fL, &fs);
    if (rc) return rc;
    return tonemap_rgba8(c, fL, fs, exposure, out);
}

}  // extern "C"

int tonemap_rgba8(mcpt_ctx* c, const float4* col, const uint32_t* samples, float exposure, uint8_t* out) {
    const size_t P = c->film.pixels();
    DevBuf<uchar4> d;
    DevBuf<uint32_t> ones;
    if (!d.ensure(P) || (!samples && !ones.ensure(P))) {
        (void)hipGetLastError();
        return set_err(c, MCPT_E_NOMEM, "tonemap buffers");
    }
    hipError_t e = samples ? hipSuccess : hipMemsetD32Async((hipDeviceptr_t)ones.get(), 1, P, c->stream);
    if (e == hipSuccess) {
        TonemapArgs a{col, samples ? samples : ones.get(), d, exposure, (uint32_t)P};
        launch_tonemap(a, c->stream);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = hipMemcpy(out, d, P * sizeof(uchar4), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return set_err(c, MCPT_E_HIP, std::string("tonemap: ") + hipGetErrorString(e));
    return MCPT_OK;
}

int read_plane(mcpt_ctx* c, const float4* d, size_t n, float* xyz, float* w) {
    std::vector<float4> o(n);
    HIPCHK(c, hipMemcpy(o.data(), d, n * sizeof(float4), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; i++) {
        if (xyz) { xyz[3 * i] = o[i].x; xyz[3 * i + 1] = o[i].y; xyz[3 * i + 2] = o[i].z; }
        if (w) w[i] = o[i].w;
    }
    return MCPT_OK;
}
