// capi_host.cpp -- extern "C" entry points of the host scene builder (mcpt_scene_*).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>

#include "host_internal.hpp"
#include "mcpt.h"

struct mcpt_scene {
    mcpt_host::Scene s;
};

namespace mcpt_host {
thread_local std::string g_last_error;
void set_global_error(const std::string& e) { g_last_error = e; }
const char* global_error() { return g_last_error.c_str(); }
}  // namespace mcpt_host

static int fail(mcpt_scene* s, int rc, const std::string& msg) {
    if (s) s->s.err = msg;
    mcpt_host::set_global_error(msg);
    return rc;
}

extern "C" {

mcpt_scene* mcpt_scene_new(void) { return new (std::nothrow) mcpt_scene(); }
void mcpt_scene_free(mcpt_scene* s) { delete s; }

int mcpt_scene_load_glb(mcpt_scene* s, const char* path, const float* xform16) { return mcpt_scene_load_glb_ex(s, path, xform16, 0u); }
int mcpt_scene_load_glb_ex(mcpt_scene* s, const char* path, const float* xform16, uint32_t flags) {
    if (!s || !path) return fail(s, MCPT_E_INVALID, "null argument");
    if (flags & ~(uint32_t)MCPT_GLB_AS_AUTHORED) return fail(s, MCPT_E_INVALID, "unknown glb flag");
    std::string err;
    int rc;
    try {
        rc = s->s.load_glb(path, xform16, flags, err);
    } catch (const std::bad_alloc&) {
        return fail(s, MCPT_E_NOMEM, "glb: out of memory");
    }
    return rc ? fail(s, rc, err) : MCPT_OK;
}
int mcpt_scene_glb_report(const mcpt_scene* s, int32_t* counts4, char* buf, int32_t len) {
    if (!s) return MCPT_E_INVALID;
    for (int k = 0; counts4 && k < 4; k++) counts4[k] = s->s.glb_counts[k];
    if (buf && len > 0) {
        const size_t n = std::min((size_t)len - 1, s->s.glb_lines.size());
        memcpy(buf, s->s.glb_lines.data(), n);
        buf[n] = 0;
    }
    return MCPT_OK;
}

int mcpt_scene_add_mesh(mcpt_scene* s, int32_t ntri, const float* v0, const float* v1, const float* v2,
                        const float* n0, const float* n1, const float* n2, const float* base_rgb) {
    if (!s || ntri < 0 || (ntri > 0 && (!v0 || !v1 || !v2 || !n0 || !n1 || !n2)))
        return fail(s, MCPT_E_INVALID, "bad mesh arguments");
    std::vector<mcpt::V3> pos, nrm;
    std::vector<uint32_t> idx;
    const float* P[3] = {v0, v1, v2};
    const float* N[3] = {n0, n1, n2};
    for (int32_t t = 0; t < ntri; t++)
        for (int k = 0; k < 3; k++) {
            pos.push_back(mcpt::ld3(P[k], t));
            nrm.push_back(mcpt::ld3(N[k], t));
            idx.push_back((uint32_t)idx.size());
        }
    mcpt::V3 bc = base_rgb ? mcpt::v3(base_rgb[0], base_rgb[1], base_rgb[2]) : mcpt::v3(1.f, 1.f, 1.f);
    s->s.add_mesh(pos, nrm, idx, bc);
    return MCPT_OK;
}

int mcpt_scene_set_env_hdr(mcpt_scene* s, const char* path, int32_t mode) {
    if (!s || !path || (mode != 0 && mode != 1)) return fail(s, MCPT_E_INVALID, "bad env arguments");
    std::string err;
    int rc = s->s.set_env_hdr(path, mode, err);
    return rc ? fail(s, rc, err) : MCPT_OK;
}

int mcpt_scene_set_env_hdr_ex(mcpt_scene* s, const char* path, int32_t mode, uint32_t flags) {
    if (!s || !path || (mode != 0 && mode != 1) || (flags & ~(uint32_t)MCPT_ENV_DEVICE_TABLES))
        return fail(s, MCPT_E_INVALID, "bad env arguments");
    std::string err;
    int rc = s->s.set_env_hdr(path, mode, err, !(flags & MCPT_ENV_DEVICE_TABLES));
    return rc ? fail(s, rc, err) : MCPT_OK;
}

int mcpt_scene_set_env_color(mcpt_scene* s, const float* rgb, float ls) {
    if (!s || !rgb) return fail(s, MCPT_E_INVALID, "null argument");
    for (int i = 0; i < 3; i++) s->s.env_color[i] = rgb[i];
    s->s.env_ls = ls;
    s->s.env_mode = 0;
    return MCPT_OK;
}

int mcpt_scene_add_dir_light(mcpt_scene* s, const float* dir, const float* rgb, float ls) {
    if (!s || !dir || !rgb) return fail(s, MCPT_E_INVALID, "null argument");
    // device copy is NOT normalised (DirectionalLight.cu:82-88)
    float p[7] = {dir[0], dir[1], dir[2], rgb[0], rgb[1], rgb[2], ls};
    s->s.dir_lights.insert(s->s.dir_lights.end(), p, p + 7);
    return MCPT_OK;
}

int mcpt_scene_transform(mcpt_scene* s, const float* xform16) {
    if (!s || !xform16) return fail(s, MCPT_E_INVALID, "null argument");
    s->s.transform(xform16);
    return MCPT_OK;
}

int mcpt_scene_make_proxy(mcpt_scene* s, int32_t config_id, const char* asset_dir) {
    if (!s || !asset_dir) return fail(s, MCPT_E_INVALID, "null argument");
    std::string err;
    int rc = mcpt_host::make_proxy(s->s, config_id, asset_dir, err);
    return rc ? fail(s, rc, err) : MCPT_OK;
}

int mcpt_scene_build(mcpt_scene* s, int32_t max_prims_in_node) {
    if (!s) return fail(s, MCPT_E_INVALID, "null scene");
    std::string err;
    int rc = s->s.build(max_prims_in_node, err);
    return rc ? fail(s, rc, err) : MCPT_OK;
}

int mcpt_scene_build_ex(mcpt_scene* s, const mcpt_bvh_params* p) {
    if (!s || !p) return fail(s, MCPT_E_INVALID, "null argument");
    std::string err;
    int rc = s->s.build(*p, err);
    return rc ? fail(s, rc, err) : MCPT_OK;
}

int mcpt_scene_get_desc(const mcpt_scene* s, mcpt_scene_desc* out) {
    if (!s || !out) return MCPT_E_INVALID;
    if (!s->s.built) return fail(const_cast<mcpt_scene*>(s), MCPT_E_INVALID, "scene not built");
    s->s.desc(out);
    return MCPT_OK;
}

int mcpt_scene_set_material_emission(mcpt_scene* s, int32_t mat, const float* rgb) {
    if (!s || !rgb) return fail(s, MCPT_E_INVALID, "null argument");
    if (mat < 0 || (size_t)mat >= s->s.emission.size() / 3) return fail(s, MCPT_E_INVALID, "material id out of range");
    for (int k = 0; k < 3; k++)
        if (!(rgb[k] >= 0.f) || !std::isfinite(rgb[k])) return fail(s, MCPT_E_INVALID, "emission must be finite and >= 0");
    for (int k = 0; k < 3; k++) s->s.emission[3 * (size_t)mat + k] = rgb[k];
    return MCPT_OK;
}

int mcpt_scene_get_emission(const mcpt_scene* s, const float** rgb, int32_t* nmat) {
    if (!s || !rgb || !nmat) return MCPT_E_INVALID;
    *nmat = (int32_t)(s->s.emission.size() / 3);
    *rgb = s->s.has_emission() ? s->s.emission.data() : nullptr;
    return MCPT_OK;
}

// ---- base-colour textures ----
int mcpt_scene_set_mesh_uv(mcpt_scene* s, int32_t mat, const float* uv0, const float* uv1, const float* uv2) {
    if (!s || !uv0 || !uv1 || !uv2) return fail(s, MCPT_E_INVALID, "null argument");
    if (mat < 0 || (size_t)mat >= s->s.mat_tex.size()) return fail(s, MCPT_E_INVALID, "material id out of range");
    const float* src[3] = {uv0, uv1, uv2};
    size_t i = 0;  // the mesh's triangles in add order
    for (mcpt_host::Tri& t : s->s.tris)
        if (t.mat == mat) {
            for (int k = 0; k < 3; k++) { t.uv[k][0] = src[k][2 * i]; t.uv[k][1] = src[k][2 * i + 1]; }
            i++;
        }
    if (s->s.built) s->s.gather_uv();
    return MCPT_OK;
}

// Attaches the image to material mat through the index array idx (mat_tex: base colour; mat_mr:
// metallic-roughness, section 20; mat_nrm: normal map, section 21): all kinds share the texture list.
static int scene_attach_texture(mcpt_scene* s, std::vector<int32_t> mcpt_host::Scene::*idx, int32_t mat, int32_t w, int32_t h,
                                const uint8_t* rgba8, uint32_t flags = 0) {
    if (!s) return fail(s, MCPT_E_INVALID, "null scene");
    if (mat < 0 || (size_t)mat >= s->s.mat_tex.size()) return fail(s, MCPT_E_INVALID, "material id out of range");
    if (!rgba8) {  // detach (the texture itself stays in the list: the other indices keep their meaning)
        (s->s.*idx)[mat] = -1;
        return MCPT_OK;
    }
    if (w < 1 || w > 16384 || h < 1 || h > 16384) return fail(s, MCPT_E_INVALID, "texture width and height must be 1..16384");
    mcpt_host::Texture t;
    t.w = w;
    t.h = h;
    t.rgba8.assign(rgba8, rgba8 + (size_t)w * h * 4);
    t.flags = flags;
    int32_t& k = (s->s.*idx)[mat];
    // an entry may serve several slots (a glb image is one entry however many slots use it; section 22): it is
    // replaced in place only when this slot alone refers to it, so the other slots keep their image
    int users = 0;
    for (const std::vector<int32_t>* a : {&s->s.mat_tex, &s->s.mat_mr, &s->s.mat_nrm})
        for (int32_t v : *a) users += k >= 0 && v == k;
    if (k >= 0 && users == 1) {
        s->s.textures[k] = std::move(t);  // the material's own texture is replaced
    } else {
        k = (int32_t)s->s.textures.size();
        s->s.textures.push_back(std::move(t));
    }
    return MCPT_OK;
}

int mcpt_scene_set_material_texture(mcpt_scene* s, int32_t mat, int32_t w, int32_t h, const uint8_t* rgba8) {
    return scene_attach_texture(s, &mcpt_host::Scene::mat_tex, mat, w, h, rgba8);
}
// sRGB base colour: the texture carries MCPT_TEX_* flags into the set
int mcpt_scene_set_material_texture_ex(mcpt_scene* s, int32_t mat, int32_t w, int32_t h, const uint8_t* rgba8, uint32_t flags) {
    if (s && (flags & ~(uint32_t)MCPT_TEX_SRGB)) return fail(s, MCPT_E_INVALID, "unknown texture flag");
    return scene_attach_texture(s, &mcpt_host::Scene::mat_tex, mat, w, h, rgba8, flags);
}
int mcpt_scene_get_texture_flags(const mcpt_scene* s, const uint32_t** tex_flags, int32_t* ntex) {
    if (!s || !tex_flags || !ntex) return MCPT_E_INVALID;
    const mcpt_host::Scene& sc = s->s;
    sc.tex_flag_views.clear();
    for (const mcpt_host::Texture& t : sc.textures) sc.tex_flag_views.push_back(t.flags);
    *ntex = (int32_t)sc.tex_flag_views.size();
    *tex_flags = sc.tex_flag_views.data();
    return MCPT_OK;
}
int mcpt_scene_set_material_mr_texture(mcpt_scene* s, int32_t mat, int32_t w, int32_t h, const uint8_t* rgba8) {
    return scene_attach_texture(s, &mcpt_host::Scene::mat_mr, mat, w, h, rgba8);
}
// Normal maps: a third index array into the same list, and a scale per material
int mcpt_scene_set_material_normal_texture(mcpt_scene* s, int32_t mat, int32_t w, int32_t h, const uint8_t* rgba8, float scale) {
    if (s && rgba8 && !std::isfinite(scale)) return fail(s, MCPT_E_INVALID, "normal scale must be finite");
    const int rc = scene_attach_texture(s, &mcpt_host::Scene::mat_nrm, mat, w, h, rgba8);
    if (rc == MCPT_OK) s->s.nrm_scale[mat] = rgba8 ? scale : 1.f;
    return rc;
}
int mcpt_scene_get_material_normal(const mcpt_scene* s, const int32_t** mat_nrm, const float** nrm_scale, int32_t* nmat) {
    if (!s || !mat_nrm || !nrm_scale || !nmat) return MCPT_E_INVALID;
    *nmat = (int32_t)s->s.mat_nrm.size();
    *mat_nrm = s->s.mat_nrm.data();
    *nrm_scale = s->s.nrm_scale.data();
    return MCPT_OK;
}
int mcpt_scene_get_tangents(const mcpt_scene* s, const float** tan0, const float** tan1, const float** tan2, int32_t* ntri) {
    if (!s || !tan0 || !tan1 || !tan2 || !ntri) return MCPT_E_INVALID;
    const mcpt_host::Scene& sc = s->s;
    if (!sc.built) return fail(const_cast<mcpt_scene*>(s), MCPT_E_INVALID, "scene not built");
    const int32_t n = (int32_t)sc.f_id.size();
    for (auto& t : sc.f_tan) t.assign(4 * (size_t)n, 0.f);
    const int rc = mcpt_tangents_from_uv(n, sc.f_v0.data(), sc.f_v1.data(), sc.f_v2.data(), sc.f_n0.data(), sc.f_n1.data(),
                                         sc.f_n2.data(), sc.f_uv0.data(), sc.f_uv1.data(), sc.f_uv2.data(), sc.f_tan[0].data(),
                                         sc.f_tan[1].data(), sc.f_tan[2].data());
    if (rc) return fail(const_cast<mcpt_scene*>(s), rc, "tangents: bad arrays");
    // (section 22) a triangle that came with a glb's TANGENT keeps the authored ones
    for (int32_t i = 0; i < n; i++) {
        const mcpt_host::Tri& t = sc.tris[(size_t)sc.f_id[(size_t)i]];
        if (!t.has_tan) continue;
        for (int k = 0; k < 3; k++) memcpy(&sc.f_tan[k][4 * (size_t)i], t.tan[k], 4 * sizeof(float));
    }
    *ntri = n;
    *tan0 = sc.f_tan[0].data();
    *tan1 = sc.f_tan[1].data();
    *tan2 = sc.f_tan[2].data();
    return MCPT_OK;
}
int mcpt_scene_get_material_mr(const mcpt_scene* s, const int32_t** mat_mr, int32_t* nmat) {
    if (!s || !mat_mr || !nmat) return MCPT_E_INVALID;
    *nmat = (int32_t)s->s.mat_mr.size();
    *mat_mr = s->s.mat_mr.data();
    return MCPT_OK;
}

int mcpt_scene_get_textures(const mcpt_scene* s, const mcpt_texture** textures, int32_t* ntex, const int32_t** mat_tex,
                            int32_t* nmat) {
    if (!s || !textures || !ntex || !mat_tex || !nmat) return MCPT_E_INVALID;
    const mcpt_host::Scene& sc = s->s;
    bool any = false;
    for (int32_t k : sc.mat_tex) any = any || k >= 0;
    for (int32_t k : sc.mat_mr) any = any || k >= 0;  // (section 20: the list holds MR images too)
    for (int32_t k : sc.mat_nrm) any = any || k >= 0;  // (section 21: and normal maps)
    sc.tex_views.clear();
    for (const mcpt_host::Texture& t : sc.textures) sc.tex_views.push_back(mcpt_texture{t.w, t.h, t.rgba8.data()});
    *nmat = (int32_t)sc.mat_tex.size();
    *mat_tex = sc.mat_tex.data();
    *ntex = any ? (int32_t)sc.tex_views.size() : 0;
    *textures = any ? sc.tex_views.data() : nullptr;
    return MCPT_OK;
}

int mcpt_scene_get_uv(const mcpt_scene* s, const float** uv0, const float** uv1, const float** uv2, int32_t* ntri) {
    if (!s || !uv0 || !uv1 || !uv2 || !ntri) return MCPT_E_INVALID;
    if (!s->s.built) return fail(const_cast<mcpt_scene*>(s), MCPT_E_INVALID, "scene not built");
    *ntri = (int32_t)s->s.f_id.size();
    *uv0 = s->s.f_uv0.data();
    *uv1 = s->s.f_uv1.data();
    *uv2 = s->s.f_uv2.data();
    return MCPT_OK;
}

int mcpt_scene_bvh_depth(const mcpt_scene* s) { return s ? s->s.bvh_depth : MCPT_E_INVALID; }

int mcpt_camera_make(const mcpt_camera_params* p, mcpt_camera* out) {
    if (!p || !out) return MCPT_E_INVALID;
    mcpt_host::make_camera(*p, *out);
    return MCPT_OK;
}

}  // extern "C"
