// host_internal.hpp -- host-side scene model (Scene.h / Mesh.h / EnvironmentLight.h
// of the reference, reduced to what the path-tracing backend consumes).
#pragma once
#include <functional>
#include <string>
#include <vector>

#include "../device/mcpt_core.hpp"
#include "mcpt.h"

namespace mcpt_host {

struct Tri {
    mcpt::V3 p[3];
    mcpt::V3 n[3];
    int mat;
    float uv[3][2] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};  // TEXCOORD_0 of the corners (absent: zeros)
    // a glb's TANGENT of the corners {T.xyz, s}, transformed with the node (MCPT_GLB_TEXTURES; section 22)
    float tan[3][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    bool has_tan = false;
};

// A base-colour texture attached to a material: decoded RGBA8 texels, row 0 first
struct Texture {
    int w = 0, h = 0;
    std::vector<uint8_t> rgba8;
    uint32_t flags = 0;  // MCPT_TEX_* 
};

struct Scene {
    // meshes (Scene::render_objects, Mesh.cu:35-60), world space
    std::vector<Tri> tris;
    std::vector<float> materials;   // 8 floats per material (dMaterial.cuh:11-33)
    std::vector<float> emission;    // 3 floats per material: emitted radiance (dMaterial.cuh:14-24, emissive_L)
    std::vector<float> dir_lights;  // 7 floats per light (DirectionalLight.h)
    // base-colour textures (dMaterial.cu:14-26 base_color_texture): the attached textures and, per
    // material, its texture's index or -1; tex_views: what mcpt_scene_get_textures hands out
    std::vector<Texture> textures;
    std::vector<int32_t> mat_tex;
    std::vector<int32_t> mat_mr;  // metallic-roughness textures: indices into the same list
    // normal maps: indices into the same list, a scale per material, and what
    // mcpt_scene_get_tangents hands out (mcpt_tangents_from_uv over the built arrays)
    std::vector<int32_t> mat_nrm;
    std::vector<float> nrm_scale;
    mutable std::vector<float> f_tan[3];
    mutable std::vector<mcpt_texture> tex_views;
    mutable std::vector<uint32_t> tex_flag_views;  // what mcpt_scene_get_texture_flags hands out
    // environment light (EnvironmentLight.h:17-40); default Color 0.8 (Scene.cu:21)
    int env_mode = 0;
    float env_color[3] = {0.8f, 0.8f, 0.8f};
    float env_ls = 1.f;
    int env_w = 0, env_h = 0;
    float env_pdf_denom = 0.f;
    std::vector<float> env_tex, env_marginal_y, env_marginal_p, env_conds_y, env_pdf;
    // built, BVH-ordered arrays (mcpt_scene_desc)
    bool built = false;
    int bvh_depth = 0;
    std::vector<float> f_v0, f_v1, f_v2, f_n0, f_n1, f_n2;
    std::vector<int32_t> f_mat;
    std::vector<int32_t> f_id;  // original triangle index of each BVH-ordered slot
    std::vector<float> f_uv0, f_uv1, f_uv2;  // the corners' uvs, 2 floats per BVH-ordered slot (not in the desc)
    std::vector<float> node_bmin, node_bmax;
    std::vector<int32_t> node_offset, node_nprims, node_axis;
    std::string err;
    // what the last load_glb could not honour (mcpt_scene_glb_report): images decoded / skipped, slots attached /
    // skipped, and one line per skipped image or slot
    int32_t glb_counts[4] = {0, 0, 0, 0};
    std::string glb_lines;

    void add_mesh(const std::vector<mcpt::V3>& pos, const std::vector<mcpt::V3>& nrm,
                  const std::vector<uint32_t>& idx, mcpt::V3 base, mcpt::V3 emit = mcpt::v3(0.f, 0.f, 0.f),
                  const std::vector<float>* uv = nullptr,    // uv: 2 floats per vertex, or none (zeros)
                  const std::vector<float>* tan = nullptr);  // tan: 4 floats per vertex {T.xyz, s}, or none
    bool has_emission() const;  // some material emits
    void gather_uv();           // f_uv0..2 from tris by f_id (build, and a uv change on a built scene)
    void transform(const float* xf16);
    int load_glb(const char* path, const float* xf16, uint32_t flags, std::string& err);
    int set_env_hdr(const char* path, int mode, std::string& err, bool host_tables = true);
    int build(int max_prims, std::string& err);
    int build(const mcpt_bvh_params& p, std::string& err);
    void desc(mcpt_scene_desc* d) const;
};

int load_hdr(const char* path, int& W, int& H, std::vector<float>& rgba, std::string& err);
void build_env_tables(int W, int H, const std::vector<float>& tex, std::vector<float>& marginal_y,
                      std::vector<float>& marginal_p, std::vector<float>& conds_y, std::vector<float>& pdf,
                      float& denom);
void make_camera(const mcpt_camera_params& p, mcpt_camera& out);
int make_proxy(Scene& s, int config_id, const std::string& asset_dir, std::string& err);

}  // namespace mcpt_host
