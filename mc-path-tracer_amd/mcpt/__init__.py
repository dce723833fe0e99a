"""mcpt -- Python view of the MI355X wavefront path-tracing backend (ctypes over include/mcpt.h).

The product is the C ABI in ``libmcpt.so`` (HIP kernels for gfx950 + host C++).  This module
is the thin Python mirror of the reference's host objects, used by tests/ and bench.py:

* :class:`Scene`      -- ``Scene::load`` / ``set_environment_light`` / ``add_light``
                         (CUDA-RayTracer/Scene.h:40-58) plus the BVH build (BVH.cu).
* :class:`PathTracer` -- ``PathTracer::render_image`` (PathTracer.cpp:112-130) and the
                         ``wavefront_pathtrace`` / ``clear_dfilm`` entry points
                         (wavefront_kernels.cuh:18-31), on one device.
* :func:`make_camera` -- ``Camera::update`` matrices (Camera.cu:194-224).

There is no CPU fallback: constructing a :class:`PathTracer` without a gfx950 device raises.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
PKG_DIR = os.path.dirname(_HERE)
REPO_DIR = os.path.dirname(PKG_DIR)
LIB_PATH = os.environ.get("MCPT_LIB") or os.path.join(PKG_DIR, "libmcpt.so")
ASSET_DIR = os.path.join(REPO_DIR, "assets")

MCPT_OK = 0
STAGE_LOGIC, STAGE_GENERATE, STAGE_MATERIAL, STAGE_EXTEND, STAGE_SHADOW = range(5)

_f = C.POINTER(C.c_float)
_i = C.POINTER(C.c_int32)
_u = C.POINTER(C.c_uint32)


class Config(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("spp", C.c_int32), ("max_depth", C.c_int32), ("rr_depth", C.c_int32),
                ("tile_w", C.c_int32), ("tile_h", C.c_int32), ("flags", C.c_int32)]


class SceneDesc(C.Structure):
    _fields_ = [("ntri", C.c_int32), ("v0", _f), ("v1", _f), ("v2", _f), ("n0", _f), ("n1", _f), ("n2", _f),
                ("mat", _i), ("nnodes", C.c_int32), ("bmin", _f), ("bmax", _f), ("offset", _i), ("nprims", _i),
                ("axis", _i), ("nmat", C.c_int32), ("mat_params", _f), ("ndir", C.c_int32), ("dir_params", _f),
                ("env_mode", C.c_int32), ("env_color", C.c_float * 3), ("env_ls", C.c_float),
                ("env_w", C.c_int32), ("env_h", C.c_int32), ("env_tex", _f), ("env_marginal_y", _f),
                ("env_conds_y", _f), ("env_pdf", _f), ("tri_id", _i)]


class Camera(C.Structure):
    _fields_ = [("inv_view_proj", C.c_float * 16), ("inv_view", C.c_float * 16), ("lens_radius", C.c_float),
                ("focal", C.c_float)]


class CameraParams(C.Structure):
    _fields_ = [("position", C.c_float * 3), ("yaw_deg", C.c_float), ("pitch_deg", C.c_float),
                ("fovy_rad", C.c_float), ("aspect", C.c_float), ("znear", C.c_float), ("zfar", C.c_float),
                ("lens_radius", C.c_float), ("focal", C.c_float)]


class StageStats(C.Structure):
    _fields_ = [("extend_rays", C.c_uint64), ("shadow_rays", C.c_uint64), ("vis_rays", C.c_uint64),
                ("iterations", C.c_uint64), ("live_paths", C.c_uint64), ("ms_total", C.c_float),
                ("ms_shade", C.c_float), ("ms_extend", C.c_float), ("ms_shadow", C.c_float),
                ("ext_nodes", C.c_uint64), ("ext_tests", C.c_uint64), ("ext_hits", C.c_uint64),
                ("any_nodes", C.c_uint64), ("any_tests", C.c_uint64), ("any_hits", C.c_uint64)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}

    @property
    def rays(self) -> int:
        return int(self.extend_rays + self.shadow_rays + self.vis_rays)


class DenoiseParams(C.Structure):  # mcpt_denoise_params
    _fields_ = [("passes", C.c_int32), ("sigma_color", C.c_float), ("sigma_normal", C.c_float),
                ("sigma_albedo", C.c_float), ("sigma_depth", C.c_float)]


class DenoiseGuidedParams(C.Structure):  # mcpt_denoise_guided_params
    _fields_ = [("passes", C.c_int32), ("sigma_lum", C.c_float), ("lum_eps", C.c_float), ("sigma_color", C.c_float),
                ("sigma_normal", C.c_float), ("sigma_albedo", C.c_float), ("sigma_depth", C.c_float)]


class SampleBudgetParams(C.Structure):  # mcpt_sample_budget_params
    _fields_ = [("target_rel_err", C.c_float), ("lum_floor", C.c_float), ("min_spp", C.c_uint32), ("max_spp", C.c_uint32)]


class TemporalParams(C.Structure):  # mcpt_temporal_params
    _fields_ = [("pos_tol", C.c_float), ("nrm_tol", C.c_float), ("max_history", C.c_float), ("alpha_min", C.c_float)]


class VarianceParams(C.Structure):  # mcpt_variance_params
    _fields_ = [("radius", C.c_int32), ("sigma_normal", C.c_float), ("sigma_albedo", C.c_float),
                ("sigma_depth", C.c_float), ("min_neff", C.c_float)]


class BvhInfo(C.Structure):  # mcpt_bvh_info
    _fields_ = [("npairs", C.c_int32), ("root_ref", C.c_int32), ("depth", C.c_int32), ("width", C.c_int32),
                ("layout", C.c_int32), ("ntri", C.c_int32), ("tri_f4", C.c_int32), ("gpu_built", C.c_int32),
                ("rounds", C.c_int32), ("root_mn", C.c_float * 3), ("root_mx", C.c_float * 3), ("cull_p", C.c_float)]


class Texture(C.Structure):  # mcpt_texture: a decoded RGBA8 image
    _fields_ = [("w", C.c_int32), ("h", C.c_int32), ("rgba8", C.POINTER(C.c_uint8))]


class TextureSet(C.Structure):  # mcpt_texture_set: a whole texture set, NULL = absent
    _fields_ = [("ntri", C.c_int32), ("uv0", _f), ("uv1", _f), ("uv2", _f), ("tan0", _f), ("tan1", _f), ("tan2", _f),
                ("ntex", C.c_int32), ("textures", C.POINTER(Texture)), ("nmat", C.c_int32), ("mat_tex", _i), ("mat_mr", _i),
                ("mat_nrm", _i), ("nrm_scale", _f), ("tex_flags", _u)]  # tex_flags: section 22


# mcpt_scene_load_glb_ex flags
MCPT_GLB_PBR_FACTORS, MCPT_GLB_TEXTURES, MCPT_GLB_SRGB, MCPT_GLB_AS_AUTHORED = 1, 2, 4, 7
MCPT_TEX_SRGB = 1  # mcpt_texture_set.tex_flags bit 0: sRGB-encoded texels, decoded when read as a base colour


class PathView(C.Structure):  # mcpt_path_view: path state at the shading stages' boundary
    _fields_ = [("film_w", C.c_uint32), ("film_h", C.c_uint32), ("flags", _u), ("samples", _u), ("hit_tri", _i),
                ("ray_o", _f), ("ray_d", _f), ("beta", _f), ("nee0", _f), ("nee1", _f),
                ("vis", C.POINTER(C.c_uint8)), ("Ld", _f), ("light_o", _f), ("light_d", _f), ("bvis_o", _f),
                ("bvis_d", _f), ("queued", C.POINTER(C.c_uint8))]


class SoaView(C.Structure):
    _fields_ = [("ray_o", _f), ("ray_d", _f), ("hit_pos_t", _f), ("hit_nrm_mat", _f), ("hit_tri", _i),
                ("visible", C.POINTER(C.c_uint8)), ("steps", _u), ("paths", C.POINTER(PathView))]


# mcpt_path_view fields as numpy: (dtype, values per path)
PATH_FIELDS = {"flags": (np.uint32, 1), "samples": (np.uint32, 1), "hit_tri": (np.int32, 1), "ray_o": (np.float32, 3),
               "ray_d": (np.float32, 3), "beta": (np.float32, 4), "nee0": (np.float32, 4), "nee1": (np.float32, 4),
               "vis": (np.uint8, 2), "Ld": (np.float32, 3), "light_o": (np.float32, 3), "light_d": (np.float32, 3),
               "bvis_o": (np.float32, 3), "bvis_d": (np.float32, 3), "queued": (np.uint8, 1)}
STAGE_BY_NAME = {"logic": STAGE_LOGIC, "generate": STAGE_GENERATE, "material": STAGE_MATERIAL}


def path_view(arrs: dict, n, film=(0, 0)):
    """PathView over numpy arrays (missing fields stay NULL); the arrays are kept on the view."""
    v = PathView()
    v.film_w, v.film_h = film
    keep = {}
    for k, (dt, m) in PATH_FIELDS.items():
        if k in arrs and arrs[k] is not None:
            a = np.ascontiguousarray(arrs[k], dt).reshape(n * m)
            keep[k] = a
            setattr(v, k, a.ctypes.data_as(C.POINTER(np.ctypeslib.as_ctypes_type(dt))))
    v._keep = keep
    return v


# Every symbol declared in include/mcpt.h with its ctypes signature.
ABI = {
    "mcpt_create": (C.c_int, [C.c_int, C.POINTER(Config), C.POINTER(C.c_void_p)]),
    "mcpt_destroy": (None, [C.c_void_p]),
    "mcpt_last_error": (C.c_char_p, [C.c_void_p]),
    "mcpt_scene_upload": (C.c_int, [C.c_void_p, C.POINTER(SceneDesc)]),
    "mcpt_camera_set": (C.c_int, [C.c_void_p, C.POINTER(Camera)]),
    "mcpt_film_resize": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]),
    "mcpt_film_clear": (C.c_int, [C.c_void_p]),
    "mcpt_set_tiles": (C.c_int, [C.c_void_p, _u, C.c_uint32]),
    "mcpt_set_compact_paths": (C.c_int, [C.c_void_p, C.c_int32]),
    "mcpt_debug_tiny_lds_stack": (C.c_int, [C.c_void_p, C.c_int32]),
    "mcpt_set_path_slots": (C.c_int, [C.c_void_p, C.c_uint32]),
    "mcpt_set_trace_partitions": (C.c_int, [C.c_void_p, C.c_uint32]),
    "mcpt_gather": (C.c_int, [C.POINTER(C.c_void_p), C.c_int32, C.c_int32]),
    "mcpt_wavefront_step": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(StageStats)]),
    "mcpt_iterate": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(StageStats)]),
    "mcpt_render": (C.c_int, [C.c_void_p, C.POINTER(StageStats)]),
    "mcpt_stage_run": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(SoaView), C.POINTER(SoaView), C.c_uint32]),
    "mcpt_film_read": (C.c_int, [C.c_void_p, _f, _u]),
    "mcpt_film_read_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "mcpt_film_pack_tiles": (C.c_int, [C.c_void_p, C.c_void_p, _u]),
    "mcpt_film_unpack_tiles": (C.c_int, [C.c_void_p, C.c_void_p, _u, C.c_uint32]),
    "mcpt_film_tonemap_rgba8": (C.c_int, [C.c_void_p, C.c_float, C.POINTER(C.c_uint8)]),
    "mcpt_guides_render": (C.c_int, [C.c_void_p, C.c_uint32]),
    "mcpt_guides_read": (C.c_int, [C.c_void_p, _f, _f, _f, _u]),
    "mcpt_denoise_default_params": (C.c_int, [C.POINTER(DenoiseParams)]),
    "mcpt_denoise_run": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, _f, _u, _f, _f, _f, C.POINTER(DenoiseParams), _f]),
    "mcpt_film_denoise": (C.c_int, [C.c_void_p, C.POINTER(DenoiseParams)]),
    "mcpt_denoised_read": (C.c_int, [C.c_void_p, _f]),
    "mcpt_denoised_read_device": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mcpt_denoised_tonemap_rgba8": (C.c_int, [C.c_void_p, C.c_float, C.POINTER(C.c_uint8)]),
    "mcpt_denoised_write_png": (C.c_int, [C.c_void_p, C.c_float, C.c_char_p]),
    "mcpt_debug_denoise_ms": (C.c_int, [C.c_void_p, _f]),
    "mcpt_denoise_guided_default_params": (C.c_int, [C.POINTER(DenoiseGuidedParams)]),
    "mcpt_denoise_guided_run": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, _f, _u, _f, _f, _f, _f,
                                          C.POINTER(DenoiseGuidedParams), _f, _f]),
    "mcpt_film_denoise_guided": (C.c_int, [C.c_void_p, C.POINTER(DenoiseGuidedParams)]),
    "mcpt_denoised_variance_read": (C.c_int, [C.c_void_p, _f]),
    "mcpt_set_sample_budget": (C.c_int, [C.c_void_p, _u]),
    "mcpt_sample_budget_read": (C.c_int, [C.c_void_p, _u]),
    "mcpt_set_spp": (C.c_int, [C.c_void_p, C.c_int32]),
    "mcpt_film_error": (C.c_int, [C.c_void_p]),
    "mcpt_film_error_read": (C.c_int, [C.c_void_p, _f]),
    "mcpt_error_run": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, _f, _u, _f]),
    "mcpt_debug_film_read_slot": (C.c_int, [C.c_void_p, C.c_uint32, _f, _u]),
    "mcpt_sample_budget_default_params": (C.c_int, [C.POINTER(SampleBudgetParams)]),
    "mcpt_budget_from_error": (C.c_int, [C.c_void_p, C.POINTER(SampleBudgetParams), C.POINTER(C.c_uint64)]),
    "mcpt_debug_adaptive_bytes": (C.c_int64, [C.c_void_p]),
    "mcpt_debug_adaptive_ms": (C.c_int, [C.c_void_p, _f]),
    "mcpt_set_seed": (C.c_int, [C.c_void_p, C.c_uint64]),
    "mcpt_camera_view_proj": (C.c_int, [C.POINTER(Camera), _f]),
    "mcpt_temporal_default_params": (C.c_int, [C.POINTER(TemporalParams)]),
    "mcpt_film_temporal": (C.c_int, [C.c_void_p, C.POINTER(TemporalParams)]),
    "mcpt_temporal_reset": (C.c_int, [C.c_void_p]),
    "mcpt_temporal_read": (C.c_int, [C.c_void_p, _f, _f, _f, _f]),
    "mcpt_temporal_denoise": (C.c_int, [C.c_void_p, C.POINTER(DenoiseGuidedParams)]),
    "mcpt_temporal_run": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, _f, _u, _f, _f, _f, _f, _f, _f, _f, _f,
                                    C.POINTER(TemporalParams), _f, _f, _f, _f, _f]),
    "mcpt_debug_temporal_bytes": (C.c_int64, [C.c_void_p]),
    "mcpt_debug_temporal_ms": (C.c_int, [C.c_void_p, _f]),
    "mcpt_variance_default_params": (C.c_int, [C.POINTER(VarianceParams)]),
    "mcpt_variance_run": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, _f, _u, _f, _f, _f, _f, C.POINTER(VarianceParams), _f]),
    "mcpt_set_variance_fill": (C.c_int, [C.c_void_p, C.POINTER(VarianceParams)]),
    "mcpt_debug_variance_ms": (C.c_int, [C.c_void_p, _f]),
    "mcpt_set_material_emission": (C.c_int, [C.c_void_p, C.c_int32, _f]),
    "mcpt_material_emission_read": (C.c_int, [C.c_void_p, _f, _i]),
    "mcpt_set_emitter_sampling": (C.c_int, [C.c_void_p, C.c_int32]),
    "mcpt_emitter_table_read": (C.c_int, [C.c_void_p, _f, _f, _u, _i]),
    "mcpt_debug_emitter_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "mcpt_set_emitter_mis": (C.c_int, [C.c_void_p, C.c_int32]),
    "mcpt_debug_emitter_mis": (C.c_int, [C.c_void_p]),
    "mcpt_scene_set_material_emission": (C.c_int, [C.c_void_p, C.c_int32, _f]),
    "mcpt_scene_get_emission": (C.c_int, [C.c_void_p, C.POINTER(_f), _i]),
    "mcpt_set_material_textures": (C.c_int, [C.c_void_p, C.c_int32, _f, _f, _f, C.c_int32, C.POINTER(Texture), C.c_int32, _i]),
    "mcpt_material_textures_read": (C.c_int, [C.c_void_p, _i, _i, _i, _i, C.c_int32, _i, _i, C.POINTER(C.c_uint8), _f, _f, _f]),
    "mcpt_texture_sample_run": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_uint8), C.c_uint32, _f, _f]),
    "mcpt_debug_texture_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), _i, _i]),
    "mcpt_scene_set_mesh_uv": (C.c_int, [C.c_void_p, C.c_int32, _f, _f, _f]),
    "mcpt_scene_set_material_texture": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_uint8)]),
    "mcpt_scene_get_textures": (C.c_int, [C.c_void_p, C.POINTER(C.POINTER(Texture)), _i, C.POINTER(_i), _i]),
    "mcpt_scene_get_uv": (C.c_int, [C.c_void_p, C.POINTER(_f), C.POINTER(_f), C.POINTER(_f), _i]),
    "mcpt_set_material_texture_maps": (C.c_int, [C.c_void_p, C.c_int32, _f, _f, _f, C.c_int32, C.POINTER(Texture), C.c_int32, _i, _i]),
    "mcpt_material_mr_read": (C.c_int, [C.c_void_p, _i, _i]),
    "mcpt_debug_texture_mr_stats": (C.c_int, [C.c_void_p, _i, _i]),
    "mcpt_scene_set_material_mr_texture": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_uint8)]),
    "mcpt_scene_get_material_mr": (C.c_int, [C.c_void_p, C.POINTER(_i), _i]),
    "mcpt_set_material_texture_set": (C.c_int, [C.c_void_p, C.POINTER(TextureSet)]),
    "mcpt_material_normal_read": (C.c_int, [C.c_void_p, _i, _i, _i, _f, _f, _f, _f]),
    "mcpt_debug_texture_normal_stats": (C.c_int, [C.c_void_p, _i, _i]),
    "mcpt_tangents_from_uv": (C.c_int, [C.c_int32] + [_f] * 12),
    "mcpt_material_texture_flags_read": (C.c_int, [C.c_void_p, _i, _u]),
    "mcpt_debug_texture_srgb_stats": (C.c_int, [C.c_void_p, _i, _i]),
    "mcpt_texture_sample_run_ex": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_uint8), C.c_uint32, C.c_uint32, _f, _f]),
    "mcpt_scene_set_material_texture_ex": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_uint8), C.c_uint32]),
    "mcpt_scene_get_texture_flags": (C.c_int, [C.c_void_p, C.POINTER(_u), _i]),
    "mcpt_scene_load_glb_ex": (C.c_int, [C.c_void_p, C.c_char_p, _f, C.c_uint32]),
    "mcpt_scene_glb_report": (C.c_int, [C.c_void_p, _i, C.c_char_p, C.c_int32]),
    "mcpt_scene_set_material_normal_texture": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_uint8), C.c_float]),
    "mcpt_scene_get_material_normal": (C.c_int, [C.c_void_p, C.POINTER(_i), C.POINTER(_f), _i]),
    "mcpt_scene_get_tangents": (C.c_int, [C.c_void_p, C.POINTER(_f), C.POINTER(_f), C.POINTER(_f), _i]),
    "mcpt_sync": (C.c_int, [C.c_void_p]),
    "mcpt_device_name": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int32]),
    "mcpt_debug_queue_rays": (C.c_int, [C.c_void_p, C.c_int, _f, _f, _u]),
    "mcpt_debug_last_stage_ms": (C.c_float, [C.c_void_p]),
    "mcpt_debug_last_build_ms": (C.c_float, [C.c_void_p]),
    "mcpt_debug_last_env_build_ms": (C.c_float, [C.c_void_p]),
    "mcpt_debug_env_tables": (C.c_int, [C.c_void_p, _f, _f, _f, _i]),
    "mcpt_debug_node_layout": (C.c_int, [C.c_void_p]),
    "mcpt_debug_bvh_read": (C.c_int, [C.c_void_p, _f, _f, C.POINTER(BvhInfo)]),
    "mcpt_debug_occ_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_int32)]),
    "mcpt_debug_occ_complete_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "mcpt_debug_ray_counts": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "mcpt_debug_primary_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "mcpt_set_work_counters": (C.c_int, [C.c_void_p, C.c_int32]),
    "mcpt_set_skip_discarded": (C.c_int, [C.c_void_p, C.c_int32]),
    "mcpt_debug_discard_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "mcpt_scene_upload_gpu_bvh": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mcpt_set_gpu_bvh_builder": (C.c_int, [C.c_void_p, C.c_int32]),
    "mcpt_scene_update_geometry": (C.c_int, [C.c_void_p, C.c_int32, _f, _f, _f, _f, _f, _f, C.c_int32]),
    "mcpt_scene_update_geometry_device": (C.c_int, [C.c_void_p, C.c_int32] + [C.c_void_p] * 6 + [C.c_int32]),
    "mcpt_debug_geometry_update_ms": (C.c_int, [C.c_void_p, _f]),
    "mcpt_film_size": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "mcpt_film_write_png": (C.c_int, [C.c_void_p, C.c_float, C.c_char_p]),
    "mcpt_film_write_pfm": (C.c_int, [C.c_void_p, C.c_char_p]),
    "mcpt_image_write_png": (C.c_int, [C.c_char_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint8)]),
    "mcpt_image_read_png_memory": (C.c_int, [C.c_char_p, C.c_size_t, _i, _i, C.POINTER(C.c_uint8), C.c_size_t]),
    "mcpt_image_read_png": (C.c_int, [C.c_char_p, _i, _i, C.POINTER(C.c_uint8), C.c_size_t]),
    "mcpt_image_read_png_error": (C.c_char_p, []),
    "mcpt_image_write_pfm": (C.c_int, [C.c_char_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_float)]),
    "mcpt_debug_trace_profile": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.c_int]),
    "mcpt_debug_shade_sections": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.c_int, C.c_int]),
    "mcpt_scene_build_ex": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mcpt_debug_quot": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "mcpt_debug_hbm_copy": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.POINTER(C.c_double)]),
    "mcpt_scene_new": (C.c_void_p, []),
    "mcpt_scene_free": (None, [C.c_void_p]),
    "mcpt_scene_load_glb": (C.c_int, [C.c_void_p, C.c_char_p, _f]),
    "mcpt_scene_add_mesh": (C.c_int, [C.c_void_p, C.c_int32, _f, _f, _f, _f, _f, _f, _f]),
    "mcpt_scene_set_env_hdr": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int32]),
    "mcpt_scene_set_env_hdr_ex": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int32, C.c_uint32]),
    "mcpt_scene_set_env_color": (C.c_int, [C.c_void_p, _f, C.c_float]),
    "mcpt_scene_add_dir_light": (C.c_int, [C.c_void_p, _f, _f, C.c_float]),
    "mcpt_scene_transform": (C.c_int, [C.c_void_p, _f]),
    "mcpt_scene_make_proxy": (C.c_int, [C.c_void_p, C.c_int32, C.c_char_p]),
    "mcpt_scene_build": (C.c_int, [C.c_void_p, C.c_int32]),
    "mcpt_scene_get_desc": (C.c_int, [C.c_void_p, C.POINTER(SceneDesc)]),
    "mcpt_scene_bvh_depth": (C.c_int, [C.c_void_p]),
    "mcpt_camera_make": (C.c_int, [C.POINTER(CameraParams), C.POINTER(Camera)]),
}

_lib = None


def lib() -> C.CDLL:
    """Load libmcpt.so (in-tree build).  Raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} missing: run __graft_entry__.build() (make) first")
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in ABI.items():
            fn = getattr(l, name, None)
            if fn is None and os.environ.get("MCPT_LIB"):
                continue  # an older experimental variant library (tools/gpu/ab_libs.sh)
            if fn is None:
                raise RuntimeError(f"{LIB_PATH} does not export {name}: rebuild it")
            fn.restype = res
            fn.argtypes = args
        _lib = l
    return _lib


class McptError(RuntimeError):
    pass


def _check(rc: int, ctx=None):
    if rc != MCPT_OK:
        msg = lib().mcpt_last_error(ctx)
        raise McptError(f"mcpt error {rc}: {msg.decode() if msg else ''}")


def fptr(a: np.ndarray):
    return a.ctypes.data_as(_f)


class BvhParams(C.Structure):  # mcpt_bvh_params
    _fields_ = [("builder", C.c_int32), ("max_prims", C.c_int32), ("buckets", C.c_int32),
                ("trav_cost", C.c_float), ("isect_cost", C.c_float)]


BVH_REFERENCE, BVH_SAH3 = 0, 1
FLAG_FIXED = 1  # MCPT_FLAG_FIXED: quality-mode integrator
FLAG_NO_AUTO_CLEAR = 2  # MCPT_FLAG_NO_AUTO_CLEAR: camera / scene changes do not clear the film
ENV_DEVICE_TABLES = 1  # MCPT_ENV_DEVICE_TABLES: HRDI tables built on the device at upload
GEOM_MODES = {"refit": 0, "rebuild": 1}  # MCPT_GEOM_REFIT / MCPT_GEOM_REBUILD


def default_config(spp=16, max_depth=5, rr_depth=3, seed=0x5EED2026, tile=256, fixed=False,
                   auto_clear=True) -> Config:
    flags = (FLAG_FIXED if fixed else 0) | (0 if auto_clear else FLAG_NO_AUTO_CLEAR)
    return Config(seed, spp, max_depth, rr_depth, tile, tile, flags)


def make_camera(position, yaw_deg=-90.0, pitch_deg=0.0, fovy_deg=45.0, aspect=1.0, znear=0.01, zfar=1e4,
                lens_radius=1e-4, focal=35.0) -> Camera:
    """PerspectiveCamera + Camera::update (Camera.cu:194-224) -> dCamera matrices."""
    p = CameraParams((C.c_float * 3)(*position), yaw_deg, pitch_deg, np.float32(np.radians(np.float32(fovy_deg))),
                     aspect, znear, zfar, lens_radius, focal)
    cam = Camera()
    _check(lib().mcpt_camera_make(C.byref(p), C.byref(cam)))
    return cam


def _arr(ptr, n, dtype):
    if n == 0 or not ptr:
        return np.zeros(0, dtype)
    ct = {np.float32: C.c_float, np.int32: C.c_int32, np.uint32: C.c_uint32}[dtype]
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ct)), shape=(n,)).copy()


def tangents_from_uv(v0, v1, v2, n0, n1, n2, uv0, uv1, uv2):
    """Vertex tangents for normal maps (mcpt_tangents_from_uv): (tan0, tan1, tan2),
    (ntri, 4) float32 each, {T.x, T.y, T.z, s} per corner, from (ntri, 3) vertices and normals and (ntri, 2)
    uvs.  Double arithmetic in a stated order (include/mcpt.h), with a stated fallback where a triangle's uvs
    are degenerate."""
    a = [np.ascontiguousarray(x, np.float32).reshape(-1, 3) for x in (v0, v1, v2, n0, n1, n2)]
    u = [np.ascontiguousarray(x, np.float32).reshape(-1, 2) for x in (uv0, uv1, uv2)]
    n = len(a[0])
    if any(len(x) != n for x in a + u):
        raise ValueError("every array must have one row per triangle")
    out = [np.zeros((n, 4), np.float32) for _ in range(3)]
    _check(lib().mcpt_tangents_from_uv(n, *[fptr(x) for x in a + u + out]))
    return tuple(out)


def _rgba8(img) -> np.ndarray:
    """An (h, w, 4) contiguous uint8 image from an (h, w, 4) or (h, w, 3) one (alpha 255)."""
    a = np.asarray(img)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] not in (3, 4) or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("a texture is an (h, w, 4) or (h, w, 3) uint8 image")
    if a.shape[2] == 3:
        a = np.concatenate([a, np.full(a.shape[:2] + (1,), 255, np.uint8)], axis=2)
    return np.ascontiguousarray(a)


class Scene:
    """Host scene builder (Scene.cu) -- owns flat BVH-ordered arrays after build()."""

    def __init__(self):
        self.h = lib().mcpt_scene_new()
        if not self.h:
            raise McptError("mcpt_scene_new failed")

    def __del__(self):
        if getattr(self, "h", None):
            try:
                lib().mcpt_scene_free(self.h)
            except Exception:  # interpreter shutdown
                pass
            self.h = None

    def _ck(self, rc):
        _check(rc)
        return self

    def load_glb(self, path, xform=None, flags=0):
        """Add a glb's meshes (mcpt_scene_load_glb_ex).  flags: MCPT_GLB_PBR_FACTORS, MCPT_GLB_TEXTURES,
        MCPT_GLB_SRGB or MCPT_GLB_AS_AUTHORED (all three); 0 keeps TEXCOORD_0 and the
        base-colour factor alone, as before.  glb_report() says what could not be honoured."""
        xf = None if xform is None else fptr(np.ascontiguousarray(xform, np.float32).reshape(16))
        if not flags:
            return self._ck(lib().mcpt_scene_load_glb(self.h, str(path).encode(), xf))
        return self._ck(lib().mcpt_scene_load_glb_ex(self.h, str(path).encode(), xf, int(flags)))

    def glb_report(self):
        """Of the last load_glb: {"images_decoded", "images_skipped", "slots_attached", "slots_skipped": int,
        "lines": [str]}, one line per image or material slot that could not be honoured (mcpt_scene_glb_report)."""
        c = (C.c_int32 * 4)()
        buf = C.create_string_buffer(1 << 16)
        _check(lib().mcpt_scene_glb_report(self.h, c, buf, len(buf)))
        return {"images_decoded": c[0], "images_skipped": c[1], "slots_attached": c[2], "slots_skipped": c[3],
                "lines": [l for l in buf.value.decode().split("\n") if l]}

    def add_mesh(self, v0, v1, v2, n0, n1, n2, base_rgb=(1.0, 1.0, 1.0)):
        arrs = [np.ascontiguousarray(a, np.float32).reshape(-1, 3) for a in (v0, v1, v2, n0, n1, n2)]
        bc = np.asarray(base_rgb, np.float32)
        return self._ck(lib().mcpt_scene_add_mesh(self.h, len(arrs[0]), *[fptr(a) for a in arrs], fptr(bc)))

    def set_emission(self, mat, rgb):
        """Emitted radiance of material ``mat`` (one material per added mesh, in add order: the ids of
        arrays()["mat"]).  PathTracer.upload_scene installs the scene's table after the upload."""
        e = np.ascontiguousarray(rgb, np.float32).reshape(3)
        return self._ck(lib().mcpt_scene_set_material_emission(self.h, int(mat), fptr(e)))

    def emission(self):
        """The per-material emission as an (nmat, 3) array, or None when no material emits."""
        p, n = _f(), C.c_int32(0)
        if not hasattr(lib(), "mcpt_scene_get_emission") and os.environ.get("MCPT_LIB"):
            return None  # (an older variant library: no emission)
        _check(lib().mcpt_scene_get_emission(self.h, C.byref(p), C.byref(n)))
        return _arr(p, 3 * n.value, np.float32).reshape(n.value, 3) if p else None

    def set_uv(self, mat, uv0, uv1, uv2):
        """Corner uvs of material ``mat``'s triangles, (n, 2) each, in the order the mesh's triangles were
        added (mcpt_scene_set_mesh_uv).  The library reads 2 floats per triangle of
        the mesh from each array."""
        u = [np.ascontiguousarray(a, np.float32).reshape(-1, 2) for a in (uv0, uv1, uv2)]
        if not (len(u[0]) == len(u[1]) == len(u[2])):
            raise ValueError("uv0, uv1 and uv2 must have one row per triangle of the mesh")
        d = SceneDesc()
        if lib().mcpt_scene_get_desc(self.h, C.byref(d)) == MCPT_OK and 0 <= int(mat) < d.nmat:  # built: the size is known
            if len(u[0]) != int((_arr(d.mat, d.ntri, np.int32) == int(mat)).sum()):
                raise ValueError("uv0, uv1 and uv2 must have one row per triangle of the mesh")
        return self._ck(lib().mcpt_scene_set_mesh_uv(self.h, int(mat), *[fptr(a) for a in u]))

    def set_texture(self, mat, img_u8, srgb=False):
        """Attach a base-colour texture to material ``mat``: an (h, w, 4) or (h, w, 3) uint8 image, row 0
        = v in [0, 1/h), alpha ignored.  Used as stored unless ``srgb``: then the texels are sRGB-encoded
        (every glTF base-colour image is) and the lookup decodes them before filtering.
        None detaches.  PathTracer.upload_scene installs the scene's textures after the upload."""
        if img_u8 is None:
            return self._ck(lib().mcpt_scene_set_material_texture(self.h, int(mat), 0, 0, None))
        img = _rgba8(img_u8)
        if srgb:
            return self._ck(lib().mcpt_scene_set_material_texture_ex(self.h, int(mat), img.shape[1], img.shape[0],
                                                                     img.ctypes.data_as(C.POINTER(C.c_uint8)), MCPT_TEX_SRGB))
        return self._ck(lib().mcpt_scene_set_material_texture(self.h, int(mat), img.shape[1], img.shape[0],
                                                              img.ctypes.data_as(C.POINTER(C.c_uint8))))

    def set_mr_texture(self, mat, img_u8):
        """Attach a metallic-roughness texture to material ``mat``: an image as
        set_texture takes it, whose G channel scales the material's roughness and whose B channel its
        metallic (R and alpha ignored; used as stored).  None detaches.  Independent of the material's
        base-colour texture; PathTracer.upload_scene installs it with the rest."""
        if img_u8 is None:
            return self._ck(lib().mcpt_scene_set_material_mr_texture(self.h, int(mat), 0, 0, None))
        img = _rgba8(img_u8)
        return self._ck(lib().mcpt_scene_set_material_mr_texture(self.h, int(mat), img.shape[1], img.shape[0],
                                                                 img.ctypes.data_as(C.POINTER(C.c_uint8))))

    def set_normal_texture(self, mat, img_u8, scale=1.0):
        """Attach a tangent-space normal map to material ``mat``: an image as
        set_texture takes it (R, G: the tangent and bitangent components times ``scale``, B: "up"; alpha
        ignored; used as stored).  None detaches.  Independent of the material's other textures;
        PathTracer.upload_scene installs it with the rest, with the built scene's tangents()."""
        L = lib().mcpt_scene_set_material_normal_texture
        if img_u8 is None:
            return self._ck(L(self.h, int(mat), 0, 0, None, 1.0))
        img = _rgba8(img_u8)
        return self._ck(L(self.h, int(mat), img.shape[1], img.shape[0], img.ctypes.data_as(C.POINTER(C.c_uint8)), float(scale)))

    def tangents(self):
        """The built scene's vertex tangents (tan0, tan1, tan2), (ntri, 4) each, in the desc's triangle
        order: tangents_from_uv over its vertices, normals and uvs."""
        p, n = [_f(), _f(), _f()], C.c_int32(0)
        self._ck(lib().mcpt_scene_get_tangents(self.h, C.byref(p[0]), C.byref(p[1]), C.byref(p[2]), C.byref(n)))
        return tuple(_arr(q, 4 * n.value, np.float32).reshape(n.value, 4) for q in p)

    def textures(self):
        """None when no material has a texture of any kind, else {"textures": [(h, w, 4) uint8, ...],
        "mat_tex": int32 (nmat,), "mat_mr": int32 (nmat,)} (copies): per material the index of its
        base-colour and of its metallic-roughness texture in the one list, or -1; and, only when a material
        has a normal map, "mat_nrm": int32 (nmat,) and "nrm_scale": float32 (nmat,); and, only when a texture
        carries a flag (set_texture(..., srgb=True); section 22), "tex_flags": uint32 per texture."""
        t, mt, nt, nm = C.POINTER(Texture)(), _i(), C.c_int32(0), C.c_int32(0)
        _check(lib().mcpt_scene_get_textures(self.h, C.byref(t), C.byref(nt), C.byref(mt), C.byref(nm)))
        if not t or nt.value == 0:
            return None
        imgs = [np.ctypeslib.as_array(t[k].rgba8, shape=(t[k].h, t[k].w, 4)).copy() for k in range(nt.value)]
        out = {"textures": imgs, "mat_tex": _arr(mt, nm.value, np.int32), "mat_mr": np.full(nm.value, -1, np.int32)}
        if hasattr(lib(), "mcpt_scene_get_material_mr"):  # (an older variant library has none)
            mr, nr = _i(), C.c_int32(0)
            _check(lib().mcpt_scene_get_material_mr(self.h, C.byref(mr), C.byref(nr)))
            out["mat_mr"] = _arr(mr, nr.value, np.int32)
        if hasattr(lib(), "mcpt_scene_get_material_normal"):  # (an older variant library has none)
            mn, sc, nn = _i(), _f(), C.c_int32(0)
            _check(lib().mcpt_scene_get_material_normal(self.h, C.byref(mn), C.byref(sc), C.byref(nn)))
            mn = _arr(mn, nn.value, np.int32)
            if (mn >= 0).any():
                out["mat_nrm"], out["nrm_scale"] = mn, _arr(sc, nn.value, np.float32)
        fl, nf = _u(), C.c_int32(0)
        _check(lib().mcpt_scene_get_texture_flags(self.h, C.byref(fl), C.byref(nf)))
        fl = _arr(fl, nf.value, np.uint32)
        if fl.any():
            out["tex_flags"] = fl
        return out

    def uv(self):
        """The built scene's corner uvs (uv0, uv1, uv2), (ntri, 2) each, in the desc's triangle order."""
        p, n = [_f(), _f(), _f()], C.c_int32(0)
        _check(lib().mcpt_scene_get_uv(self.h, C.byref(p[0]), C.byref(p[1]), C.byref(p[2]), C.byref(n)))
        return tuple(_arr(q, 2 * n.value, np.float32).reshape(n.value, 2) for q in p)

    def set_env_hdr(self, path, mode=1, device_tables=False):
        """EnvironmentLight from an .hdr.  device_tables=True keeps the texture only; the
        light tables are then built on the device at upload (MCPT_ENV_DEVICE_TABLES)."""
        if device_tables:
            return self._ck(lib().mcpt_scene_set_env_hdr_ex(self.h, str(path).encode(), mode, ENV_DEVICE_TABLES))
        return self._ck(lib().mcpt_scene_set_env_hdr(self.h, str(path).encode(), mode))

    def set_env_color(self, rgb, ls=1.0):
        return self._ck(lib().mcpt_scene_set_env_color(self.h, fptr(np.asarray(rgb, np.float32)), ls))

    def add_dir_light(self, direction, rgb, ls=1.0):
        return self._ck(lib().mcpt_scene_add_dir_light(self.h, fptr(np.asarray(direction, np.float32)),
                                                       fptr(np.asarray(rgb, np.float32)), ls))

    def transform(self, xform):
        return self._ck(lib().mcpt_scene_transform(self.h, fptr(np.ascontiguousarray(xform, np.float32).reshape(16))))

    def make_proxy(self, config_id, asset_dir=ASSET_DIR):
        return self._ck(lib().mcpt_scene_make_proxy(self.h, config_id, str(asset_dir).encode()))

    def build(self, max_prims=8, builder="reference", buckets=32, trav_cost=1.0, isect_cost=1.0):
        """BVH + env tables.  builder "reference" = BVHAccel's SAH (mcpt_scene_build); "sah3" =
        binned SAH over all three axes (mcpt_scene_build_ex).  Films do not depend on the tree."""
        if builder == "reference":
            return self._ck(lib().mcpt_scene_build(self.h, max_prims))
        if builder != "sah3":
            raise ValueError(f"unknown builder {builder!r}")
        p = BvhParams(BVH_SAH3, max_prims, buckets, trav_cost, isect_cost)
        return self._ck(lib().mcpt_scene_build_ex(self.h, C.byref(p)))

    def desc(self) -> SceneDesc:
        d = SceneDesc()
        _check(lib().mcpt_scene_get_desc(self.h, C.byref(d)))
        d._owner = self  # keep arrays alive
        return d

    @property
    def bvh_depth(self) -> int:
        return lib().mcpt_scene_bvh_depth(self.h)

    def arrays(self) -> dict:
        """Copies of the built arrays as numpy (for oracles, tests and fixtures)."""
        d = self.desc()
        T, N = d.ntri, d.nnodes
        out = {k: _arr(getattr(d, k), 3 * T, np.float32).reshape(T, 3) for k in ("v0", "v1", "v2", "n0", "n1", "n2")}
        out["mat"] = _arr(d.mat, T, np.int32)
        out["bmin"] = _arr(d.bmin, 3 * N, np.float32).reshape(N, 3)
        out["bmax"] = _arr(d.bmax, 3 * N, np.float32).reshape(N, 3)
        for k in ("offset", "nprims", "axis"):
            out[k] = _arr(getattr(d, k), N, np.int32)
        out["mat_params"] = _arr(d.mat_params, 8 * d.nmat, np.float32).reshape(d.nmat, 8)
        out["dir_params"] = _arr(d.dir_params, 7 * d.ndir, np.float32).reshape(d.ndir, 7)
        out["env_mode"] = d.env_mode
        out["env_color"] = np.array(list(d.env_color), np.float32)
        out["env_ls"] = np.float32(d.env_ls)
        W, H = d.env_w, d.env_h
        out["env_tex"] = _arr(d.env_tex, 4 * W * H, np.float32).reshape(H, W, 4)
        out["env_marginal_y"] = _arr(d.env_marginal_y, H, np.float32)
        # tables are absent (size 0) when left to the device build (set_env_hdr(device_tables=True))
        out["env_conds_y"] = _arr(d.env_conds_y, W * H, np.float32).reshape(H, W) if d.env_conds_y else np.zeros(0, np.float32)
        out["env_pdf"] = _arr(d.env_pdf, W * H, np.float32).reshape(H, W) if d.env_pdf else np.zeros(0, np.float32)
        out["tri_id"] = _arr(d.tri_id, T, np.int32) if d.tri_id else np.arange(T, dtype=np.int32)
        if hasattr(lib(), "mcpt_scene_get_uv"):  # (an older variant library has none)
            out["uv0"], out["uv1"], out["uv2"] = self.uv()  # not part of the desc
        return out


def desc_from_arrays(a: dict) -> SceneDesc:
    """SceneDesc pointing at numpy arrays in ``a`` (kept alive on the returned object)."""
    keep = {}

    def f(k):
        arr = np.ascontiguousarray(a[k], np.float32)
        keep[k] = arr
        return arr.ctypes.data_as(_f) if arr.size else None

    def i(k):
        arr = np.ascontiguousarray(a[k], np.int32)
        keep[k] = arr
        return arr.ctypes.data_as(_i) if arr.size else None

    d = SceneDesc()
    d.ntri = len(a["mat"])
    d.v0, d.v1, d.v2, d.n0, d.n1, d.n2 = (f(k) for k in ("v0", "v1", "v2", "n0", "n1", "n2"))
    d.mat = i("mat")
    d.nnodes = len(a["nprims"])
    d.bmin, d.bmax = f("bmin"), f("bmax")
    d.offset, d.nprims, d.axis = i("offset"), i("nprims"), i("axis")
    d.nmat = len(a["mat_params"])
    d.mat_params = f("mat_params")
    d.ndir = len(a["dir_params"])
    d.dir_params = f("dir_params")
    d.env_mode = int(a["env_mode"])
    for k in range(3):
        d.env_color[k] = float(a["env_color"][k])
    d.env_ls = float(a["env_ls"])
    tex = np.asarray(a["env_tex"])
    d.env_h, d.env_w = (tex.shape[0], tex.shape[1]) if tex.size else (0, 0)
    d.env_tex, d.env_marginal_y, d.env_conds_y, d.env_pdf = (f(k) for k in ("env_tex", "env_marginal_y", "env_conds_y", "env_pdf"))
    d.tri_id = i("tri_id") if "tri_id" in a and len(a["tri_id"]) else None
    d._keep = keep
    return d


class PathTracer:
    """Device context (one GPU): the reference's PathTracer + Film device state."""

    def __init__(self, device=0, config: Config | None = None):
        self.cfg = config or default_config()
        h = C.c_void_p()
        _check(lib().mcpt_create(device, C.byref(self.cfg), C.byref(h)))
        self.h = h
        self.device = device
        self.W = self.H = 0

    def close(self):
        if getattr(self, "h", None):
            try:
                lib().mcpt_destroy(self.h)
            except Exception:  # interpreter shutdown
                pass
            self.h = None

    __del__ = close

    def _ck(self, rc):
        _check(rc, self.h)

    @property
    def device_name(self) -> str:
        buf = C.create_string_buffer(256)
        self._ck(lib().mcpt_device_name(self.h, buf, 256))
        return buf.value.decode()

    def upload_scene(self, scene, gpu_bvh=False):
        """mcpt_scene_upload (host BVH from the scene), or with gpu_bvh=True / "ploc" / "lbvh"
        mcpt_scene_upload_gpu_bvh (BVH built on the device, PLOC by default; same hits)."""
        d = scene.desc() if isinstance(scene, Scene) else scene
        if gpu_bvh:
            if gpu_bvh not in (True, "ploc", "lbvh"):
                raise ValueError(f"unknown GPU BVH builder {gpu_bvh!r}")
            # True is the documented default (PLOC), set explicitly: the builder is context state,
            # so an earlier "lbvh" upload must not carry over
            self._ck(lib().mcpt_set_gpu_bvh_builder(self.h, 0 if gpu_bvh == "lbvh" else 1))
            self._ck(lib().mcpt_scene_upload_gpu_bvh(self.h, C.byref(d)))
        else:
            self._ck(lib().mcpt_scene_upload(self.h, C.byref(d)))
        # the desc carries no emission: a Scene's table is installed after the upload (which dropped
        # the previous scene's), so every rank of mcpt.parallel renders under the same one
        e = scene.emission() if isinstance(scene, Scene) else None
        if e is not None:
            self.set_emission(e)
        # ... and no textures: a Scene's are installed likewise
        if isinstance(scene, Scene) and hasattr(lib(), "mcpt_scene_get_textures"):
            t = scene.textures()
            if t is not None:
                kw = {}
                if "mat_nrm" in t:  # (section 21) normal maps come with the built scene's tangents
                    kw = dict(tangents=scene.tangents(), mat_nrm=t["mat_nrm"], nrm_scale=t["nrm_scale"])
                if "tex_flags" in t:  # (section 22) a flagged texture: its sRGB flag comes along
                    kw["tex_flags"] = t["tex_flags"]
                self.set_textures(*scene.uv(), t["textures"], t["mat_tex"], mat_mr=t["mat_mr"] if (t["mat_mr"] >= 0).any() else None, **kw)

    def set_textures(self, uv0=None, uv1=None, uv2=None, textures=None, mat_tex=None, mat_mr=None, tangents=None, mat_nrm=None,
                     nrm_scale=None, tex_flags=None):
        """Base-colour textures (mcpt_set_material_textures): the corner uvs, (ntri, 2)
        each in the uploaded desc's triangle order, a list of (h, w, 4) / (h, w, 3) uint8 images, and per
        material a texture index or -1.  No arguments (or no textures) remove the set.  A change clears the
        film at the next render and makes the guide buffers stale.
        mat_mr (mcpt_set_material_texture_maps; section 20): per material the index of its
        metallic-roughness texture in the same list, or -1; None: no material has one (the older call).
        tangents, mat_nrm, nrm_scale (mcpt_set_material_texture_set; section 21): (tan0, tan1, tan2), (ntri, 4)
        each as tangents_from_uv returns them; per material the index of its normal map in the same list,
        or -1; one scale per material.  Each may be None (absent); all None: the older calls.
        tex_flags (section 22): one word per texture, bit 0 MCPT_TEX_SRGB (the texels are sRGB-encoded and
        decoded when read as a base colour); None: absent, every texture used as stored."""
        if not textures:
            self._ck(lib().mcpt_set_material_textures(self.h, 0, None, None, None, 0, None, 0, None))
            return
        u = [np.ascontiguousarray(a, np.float32).reshape(-1, 2) for a in (uv0, uv1, uv2)]
        if not (len(u[0]) == len(u[1]) == len(u[2])):
            raise ValueError("uv0, uv1 and uv2 must have one row per triangle")
        imgs = [_rgba8(t) for t in textures]
        arr = (Texture * len(imgs))()
        for k, im in enumerate(imgs):
            arr[k].w, arr[k].h = im.shape[1], im.shape[0]
            arr[k].rgba8 = im.ctypes.data_as(C.POINTER(C.c_uint8))
        mt = np.ascontiguousarray(mat_tex, np.int32).reshape(-1)
        if tangents is not None or mat_nrm is not None or nrm_scale is not None or tex_flags is not None:
            ts = TextureSet()
            ts.ntri, ts.uv0, ts.uv1, ts.uv2 = len(u[0]), fptr(u[0]), fptr(u[1]), fptr(u[2])
            ts.ntex, ts.textures, ts.nmat, ts.mat_tex = len(imgs), arr, len(mt), mt.ctypes.data_as(_i)
            keep = []  # (the arrays the struct points into, alive across the call)
            if tangents is not None:
                tn = [np.ascontiguousarray(t, np.float32).reshape(-1, 4) for t in tangents]
                if len(tn) != 3 or any(len(t) != len(u[0]) for t in tn):
                    raise ValueError("tangents are three arrays with one row {T.xyz, s} per triangle")
                ts.tan0, ts.tan1, ts.tan2 = (fptr(t) for t in tn)
                keep += tn
            if tex_flags is not None:
                fl = np.ascontiguousarray(tex_flags, np.uint32).reshape(-1)
                if len(fl) != len(imgs):
                    raise ValueError("tex_flags must have one word per texture")
                ts.tex_flags = fl.ctypes.data_as(_u)
                keep.append(fl)
            for name, val, dt, ct in (("mat_mr", mat_mr, np.int32, _i), ("mat_nrm", mat_nrm, np.int32, _i),
                                      ("nrm_scale", nrm_scale, np.float32, _f)):
                if val is not None:
                    v = np.ascontiguousarray(val, dt).reshape(-1)
                    if len(v) != len(mt):
                        raise ValueError(f"mat_tex and {name} must have one entry per material")
                    setattr(ts, name, v.ctypes.data_as(ct))
                    keep.append(v)
            self._ck(lib().mcpt_set_material_texture_set(self.h, C.byref(ts)))
            return
        if mat_mr is None:
            self._ck(lib().mcpt_set_material_textures(self.h, len(u[0]), fptr(u[0]), fptr(u[1]), fptr(u[2]), len(imgs), arr,
                                                      len(mt), mt.ctypes.data_as(_i)))
            return
        mr = np.ascontiguousarray(mat_mr, np.int32).reshape(-1)
        if len(mr) != len(mt):
            raise ValueError("mat_tex and mat_mr must have one entry per material")
        self._ck(lib().mcpt_set_material_texture_maps(self.h, len(u[0]), fptr(u[0]), fptr(u[1]), fptr(u[2]), len(imgs), arr,
                                                      len(mt), mt.ctypes.data_as(_i), mr.ctypes.data_as(_i)))

    def textures(self):
        """The installed set as {"uv0", "uv1", "uv2": (ntri, 2), "textures": [(h, w, 4) uint8], "mat_tex":
        int32 (nmat,), "mat_mr": int32 (nmat,)}, or None when none is installed; "mat_nrm", "nrm_scale" and
        "tangents" only while the set carries normal-map fields, "tex_flags" only while it carries flags."""
        nt, nx, nm = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        L = lib().mcpt_material_textures_read
        self._ck(L(self.h, C.byref(nt), C.byref(nx), C.byref(nm), None, -1, None, None, None, None, None, None))
        if nx.value == 0 and nm.value == 0:
            return None
        u = [np.zeros((nt.value, 2), np.float32) for _ in range(3)]
        mt = np.zeros(nm.value, np.int32)
        self._ck(L(self.h, None, None, None, mt.ctypes.data_as(_i), -1, None, None, None, fptr(u[0]), fptr(u[1]), fptr(u[2])))
        imgs = []
        for k in range(nx.value):
            w, h = C.c_int32(0), C.c_int32(0)
            self._ck(L(self.h, None, None, None, None, k, C.byref(w), C.byref(h), None, None, None, None))
            im = np.zeros((h.value, w.value, 4), np.uint8)
            self._ck(L(self.h, None, None, None, None, k, None, None, im.ctypes.data_as(C.POINTER(C.c_uint8)), None, None, None))
            imgs.append(im)
        mr = np.full(nm.value, -1, np.int32)
        if hasattr(lib(), "mcpt_material_mr_read"):  # (an older variant library has none)
            self._ck(lib().mcpt_material_mr_read(self.h, None, mr.ctypes.data_as(_i)))
        out = {"uv0": u[0], "uv1": u[1], "uv2": u[2], "textures": imgs, "mat_tex": mt, "mat_mr": mr}
        if hasattr(lib(), "mcpt_material_normal_read"):  # (an older variant library has none)
            n, ntan = C.c_int32(0), C.c_int32(0)
            L = lib().mcpt_material_normal_read
            self._ck(L(self.h, C.byref(n), C.byref(ntan), None, None, None, None, None))
            if n.value:  # the set carries normal-map fields (section 21): the keys exist only then
                mn, sc = np.zeros(n.value, np.int32), np.zeros(n.value, np.float32)
                tn = [np.zeros((ntan.value, 4), np.float32) for _ in range(3)]
                self._ck(L(self.h, None, None, mn.ctypes.data_as(_i), fptr(sc), fptr(tn[0]), fptr(tn[1]), fptr(tn[2])))
                out.update(mat_nrm=mn, nrm_scale=sc, tangents=tuple(tn) if ntan.value else None)
        n = C.c_int32(0)
        self._ck(lib().mcpt_material_texture_flags_read(self.h, C.byref(n), None))
        if n.value:  # the set carries texture flags (section 22): the key exists only then
            fl = np.zeros(n.value, np.uint32)
            self._ck(lib().mcpt_material_texture_flags_read(self.h, None, fl.ctypes.data_as(_u)))
            out["tex_flags"] = fl
        return out

    def texture_sample(self, img, uv, srgb=False):
        """The texture lookup alone on the device (mcpt_texture_sample_run): (n, 3) float32 for (n, 2) uvs
        over an (h, w, 4) / (h, w, 3) uint8 image.  Needs neither a scene nor a film.  srgb: the base-colour
        lookup of a texture flagged MCPT_TEX_SRGB (mcpt_texture_sample_run_ex)."""
        im = _rgba8(img)
        c = np.ascontiguousarray(uv, np.float32).reshape(-1, 2)
        out = np.zeros((len(c), 3), np.float32)
        if srgb:
            self._ck(lib().mcpt_texture_sample_run_ex(self.h, im.shape[1], im.shape[0], im.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                      MCPT_TEX_SRGB, len(c), fptr(c), fptr(out)))
            return out
        self._ck(lib().mcpt_texture_sample_run(self.h, im.shape[1], im.shape[0], im.ctypes.data_as(C.POINTER(C.c_uint8)),
                                               len(c), fptr(c), fptr(out)))
        return out

    def texture_stats(self):
        """dict: device bytes the installed set holds, materials with a base-colour texture, and whether
        textured kernels (of either kind) are in effect (mcpt_debug_texture_stats).  While a set is installed
        also "mr_materials", the materials with a metallic-roughness texture, and "mr_in_effect", whether the
        metallic-roughness kernels are (mcpt_debug_texture_mr_stats); a context without a set returns the
        three keys it always returned (read the other two with .get).  While a set with normal-map fields
        (tangents, mat_nrm or nrm_scale) is installed also "nrm_materials", the materials
        with a normal map, and "nrm_in_effect", whether the normal-map kernels are
        (mcpt_debug_texture_normal_stats); no other set, and no context without one, has these two keys.
        While a set with texture flags (section 22) is installed also "srgb_materials", the materials whose
        base-colour texture is flagged sRGB, and "srgb_in_effect", whether the sRGB kernels are
        (mcpt_debug_texture_srgb_stats); again no other set has these two keys."""
        b, m, on = C.c_uint64(0), C.c_int32(0), C.c_int32(0)
        self._ck(lib().mcpt_debug_texture_stats(self.h, C.byref(b), C.byref(m), C.byref(on)))
        out = {"bytes": int(b.value), "textured_materials": int(m.value), "in_effect": bool(on.value)}
        if hasattr(lib(), "mcpt_debug_texture_mr_stats"):  # (an older variant library has none)
            n = C.c_int32(0)
            self._ck(lib().mcpt_material_mr_read(self.h, C.byref(n), None))
            if n.value:
                self._ck(lib().mcpt_debug_texture_mr_stats(self.h, C.byref(m), C.byref(on)))
                out["mr_materials"], out["mr_in_effect"] = int(m.value), bool(on.value)
        if hasattr(lib(), "mcpt_debug_texture_normal_stats"):  # (an older variant library has none)
            n = C.c_int32(0)
            self._ck(lib().mcpt_material_normal_read(self.h, C.byref(n), None, None, None, None, None, None))
            if n.value:  # only while a set with normal-map fields is installed
                self._ck(lib().mcpt_debug_texture_normal_stats(self.h, C.byref(m), C.byref(on)))
                out["nrm_materials"], out["nrm_in_effect"] = int(m.value), bool(on.value)
        n = C.c_int32(0)
        self._ck(lib().mcpt_material_texture_flags_read(self.h, C.byref(n), None))
        if n.value:  # only while a set with texture flags is installed
            self._ck(lib().mcpt_debug_texture_srgb_stats(self.h, C.byref(m), C.byref(on)))
            out["srgb_materials"], out["srgb_in_effect"] = int(m.value), bool(on.value)
        return out

    def set_emission(self, rgb=None):
        """Per-material emitted radiance, (nmat, 3) for the uploaded scene's materials, or None to
        remove the table (mcpt_set_material_emission).  A change clears the film at the next render."""
        if rgb is None:
            self._ck(lib().mcpt_set_material_emission(self.h, 0, None))
            return
        e = np.ascontiguousarray(rgb, np.float32)
        if e.ndim != 2 or e.shape[1] != 3:
            raise ValueError("emission must be an (nmat, 3) array")
        self._ck(lib().mcpt_set_material_emission(self.h, e.shape[0], fptr(e)))

    def set_emitter_sampling(self, on=True):
        """Sample emissive triangles as lights (mcpt_set_emitter_sampling).  Off by
        default; inactive while no triangle emits.  Toggling clears the film at the next render."""
        self._ck(lib().mcpt_set_emitter_sampling(self.h, 1 if on else 0))

    def set_emitter_mis(self, on=True):
        """Multiple importance sampling between the emitter sample and collected emission
        (mcpt_set_emitter_mis).  Off by default; in effect only while emitter
        sampling is active, and toggling it then clears the film at the next render."""
        self._ck(lib().mcpt_set_emitter_mis(self.h, 1 if on else 0))

    def emitter_table(self):
        """The emitter table as (cdf, pick, tri_id) arrays in ascending scene triangle id, empty when
        sampling is off or nothing emits."""
        n = C.c_int32(0)
        self._ck(lib().mcpt_emitter_table_read(self.h, None, None, None, C.byref(n)))
        cdf, pick = np.zeros(n.value, np.float32), np.zeros(n.value, np.float32)
        tid = np.zeros(n.value, np.uint32)
        if n.value:
            self._ck(lib().mcpt_emitter_table_read(self.h, fptr(cdf), fptr(pick), tid.ctypes.data_as(_u), C.byref(n)))
        return cdf, pick, tid

    def emitter_stats(self):
        """dict: entries, total weight, emitter rays made since the last film clear, the last table
        build's ms, whether sampling is active (mcpt_debug_emitter_stats) and whether MIS is in effect
        (mcpt_debug_emitter_mis)."""
        out = (C.c_double * 4)()
        rc = lib().mcpt_debug_emitter_stats(self.h, out)
        if rc < 0:
            self._ck(rc)
        mis = lib().mcpt_debug_emitter_mis(self.h)
        if mis < 0:
            self._ck(mis)
        return {"entries": int(out[0]), "total_weight": out[1], "emitter_rays": int(out[2]), "build_ms": out[3],
                "active": rc == 1, "mis": mis == 1}

    def emission(self):
        """The installed table as an (nmat, 3) array, or None when none is installed."""
        n = C.c_int32(0)
        rc = lib().mcpt_material_emission_read(self.h, None, C.byref(n))
        if rc < 0:
            self._ck(rc)
        if n.value == 0:
            return None
        e = np.zeros((n.value, 3), np.float32)
        rc = lib().mcpt_material_emission_read(self.h, fptr(e), C.byref(n))
        if rc < 0:
            self._ck(rc)
        return e

    def update_geometry(self, v0, v1, v2, n0=None, n1=None, n2=None, mode="refit"):
        """New vertex positions (and normals: all three or none) for the uploaded scene's triangles, in
        the order of the uploaded desc's arrays (mcpt_scene_update_geometry).  mode "refit" keeps the
        tree's topology; "rebuild" (device-built scenes) runs the GPU builder again.  numpy arrays go
        through the host entry; torch tensors on the context's device go to the _device entry as they
        are (float32, contiguous).  The film goes stale, as after a re-upload."""
        if mode not in GEOM_MODES:
            raise ValueError(f"unknown geometry update mode {mode!r}")
        arrs = [v0, v1, v2, n0, n1, n2]
        if all(hasattr(a, "data_ptr") for a in arrs if a is not None) and v0 is not None:
            import torch

            keep = []
            for a in arrs:
                if a is not None:
                    if not a.is_cuda or a.dtype != torch.float32:
                        raise ValueError("device arrays must be float32 tensors on the GPU")
                    if a.device.index != self.device:
                        raise ValueError(f"device arrays must be on the context's GPU {self.device}, not {a.device}")
                    a = a.contiguous()
                keep.append(a)
            n = keep[0].numel() // 3
            if any(a is not None and a.numel() != 3 * n for a in keep):
                raise ValueError("vertex arrays differ in size")
            torch.cuda.synchronize(keep[0].device)  # the tensors are complete before the context's stream reads them
            ptrs = [C.c_void_p(a.data_ptr()) if a is not None and a.numel() else None for a in keep]
            self._ck(lib().mcpt_scene_update_geometry_device(self.h, n, *ptrs, GEOM_MODES[mode]))
            return
        keep = [None if a is None else np.ascontiguousarray(a, np.float32).reshape(-1, 3) for a in arrs]
        n = len(keep[0])
        if any(a is not None and len(a) != n for a in keep):
            raise ValueError("vertex arrays differ in size")
        self._ck(lib().mcpt_scene_update_geometry(self.h, n, *[None if a is None else fptr(a) for a in keep],
                                                  GEOM_MODES[mode]))

    def geometry_update_ms(self) -> dict:
        """Device times of the last update_geometry() in ms (mcpt_debug_geometry_update_ms)."""
        v = (C.c_float * 8)()
        self._ck(lib().mcpt_debug_geometry_update_ms(self.h, v))
        return dict(zip(("records", "tree", "quads", "occ_records", "prefill", "complete_keys", "total"), [float(x) for x in v[:7]]))

    def ray_counts(self) -> dict:
        """Ray counts since the last film clear (mcpt_debug_ray_counts)."""
        v = (C.c_uint64 * 5)()
        if hasattr(lib(), "mcpt_debug_ray_counts") or not os.environ.get("MCPT_LIB"):
            self._ck(lib().mcpt_debug_ray_counts(self.h, v))  # (an older variant library: zeros)
        return dict(zip(("extension", "extension_traversed", "any_hit", "any_hit_traversed", "any_hit_occluder_cache"),
                        [int(x) for x in v]))

    def primary_stats(self) -> dict:
        """Primary-hit candidate table (mcpt_debug_primary_stats): pixels with a list, overflow pixels,
        rays resolved since the last film clear, the last build's ms, and the builds so far."""
        v = (C.c_double * 4)()
        n = lib().mcpt_debug_primary_stats(self.h, v)
        if n < 0:
            raise McptError(f"mcpt_debug_primary_stats failed ({n})")
        return dict(lists=int(v[0]), overflow=int(v[1]), resolved=int(v[2]), build_ms=float(v[3]), builds=int(n))

    def set_skip_discarded(self, on=True):
        """Continuation rays the next logic pass is certain to discard are not made
        (mcpt_set_skip_discarded; on by default, the same results either way)."""
        if hasattr(lib(), "mcpt_set_skip_discarded") or not os.environ.get("MCPT_LIB"):
            self._ck(lib().mcpt_set_skip_discarded(self.h, int(bool(on))))  # (an older variant library: never skips)

    def discard_stats(self) -> dict:
        """mcpt_debug_discard_stats since the last film clear: extension rays and any-hit rays counted
        but not made, material evaluations not run, and (switch off only) the extension rays of
        discarded paths that were resolved in place."""
        v = (C.c_uint64 * 4)()
        if hasattr(lib(), "mcpt_debug_discard_stats") or not os.environ.get("MCPT_LIB"):
            self._ck(lib().mcpt_debug_discard_stats(self.h, v))  # (an older variant library: zeros)
        return dict(zip(("extension_untraced", "any_hit_untraced", "evaluations_not_run", "doomed_in_place"),
                        [int(x) for x in v]))

    def occ_stats(self):
        """(any-hit rays the occluder cache resolved since the last film clear, cache enabled)."""
        r, e = C.c_uint64(0), C.c_int32(0)
        self._ck(lib().mcpt_debug_occ_stats(self.h, C.byref(r), C.byref(e)))
        return int(r.value), bool(e.value)

    def occ_complete_stats(self) -> dict:
        """Complete keys of the occluder table (mcpt_debug_occ_complete_stats): keys of the uploaded scene
        with a complete candidate list, any-hit rays they resolved as unoccluded / as occluded since the
        last film clear, and the upload's build time of the lists in ms."""
        v = (C.c_double * 4)()
        if hasattr(lib(), "mcpt_debug_occ_complete_stats") or not os.environ.get("MCPT_LIB"):
            self._ck(lib().mcpt_debug_occ_complete_stats(self.h, v))  # (an older variant library: zeros)
        return dict(keys=int(v[0]), unoccluded=int(v[1]), occluded=int(v[2]), build_ms=float(v[3]))

    @property
    def last_build_ms(self) -> float:
        return lib().mcpt_debug_last_build_ms(self.h)

    def bvh_read(self):
        """The last upload's child-pair tree (mcpt_debug_bvh_read): (nodes (npairs, 4, 4) float32 with the
        culling margins in, triangle records (ntri, tri_f4, 4) float32 in storage order, info dict)."""
        bi = BvhInfo()
        self._ck(lib().mcpt_debug_bvh_read(self.h, None, None, C.byref(bi)))
        nodes = np.zeros((bi.npairs, 4, 4), np.float32)
        tris = np.zeros((bi.ntri, bi.tri_f4, 4), np.float32)
        self._ck(lib().mcpt_debug_bvh_read(self.h, fptr(nodes) if nodes.size else None,
                                           fptr(tris) if tris.size else None, C.byref(bi)))
        info = {k: getattr(bi, k) for k, _ in BvhInfo._fields_}
        for k in ("root_mn", "root_mx"):
            info[k] = np.array(list(info[k]), np.float32)
        info["cull_p"] = np.float32(info["cull_p"])
        return nodes, tris, info

    @property
    def last_env_build_ms(self) -> float:
        """Device time of the last HRDI table build at upload (tables not in the desc)."""
        return lib().mcpt_debug_last_env_build_ms(self.h)

    def env_tables(self, W, H) -> dict:
        """The uploaded scene's device HRDI tables (W x H map) and whether they were built on the
        device / the env_cell search guides are on."""
        my = np.zeros(H, np.float32)
        cy = np.zeros((H, W), np.float32)
        pdf = np.zeros((H, W), np.float32)
        fl = C.c_int32(0)
        self._ck(lib().mcpt_debug_env_tables(self.h, fptr(my), fptr(cy), fptr(pdf), C.byref(fl)))
        return {"marginal_y": my, "conds_y": cy, "pdf": pdf, "device_built": bool(fl.value & 1),
                "guides": bool(fl.value & 2)}

    def set_camera(self, cam: Camera):
        self._ck(lib().mcpt_camera_set(self.h, C.byref(cam)))

    def resize(self, W, H, tile_w=256, tile_h=256):
        self._ck(lib().mcpt_film_resize(self.h, W, H, tile_w, tile_h))
        self.W, self.H, self.tile_w, self.tile_h = W, H, tile_w, tile_h

    def clear(self):
        self._ck(lib().mcpt_film_clear(self.h))

    def set_path_slots(self, slots):
        """Paths in flight per pixel (mcpt_set_path_slots); re-allocates and clears the film."""
        self._ck(lib().mcpt_set_path_slots(self.h, slots))

    def set_work_counters(self, on=True):
        """Traversal work counters in StageStats (mcpt_set_work_counters; off by default: the
        counting k_trace build is slower)."""
        if hasattr(lib(), "mcpt_set_work_counters") or not os.environ.get("MCPT_LIB"):
            self._ck(lib().mcpt_set_work_counters(self.h, int(bool(on))))  # (an older variant library counts always)

    def set_trace_partitions(self, nparts=0):
        """k_trace work partitions (mcpt_set_trace_partitions); 0 = the device default, two per XCD."""
        self._ck(lib().mcpt_set_trace_partitions(self.h, nparts))

    def set_compact_paths(self, on=True):
        """Path state over the tile set only (mcpt_set_compact_paths); re-allocates and clears the film.
        In this layout set_tiles re-allocates and clears too."""
        self._ck(lib().mcpt_set_compact_paths(self.h, int(bool(on))))

    def set_tiny_lds_stack(self, on=True):
        """Tests: the traversal's 2-entry LDS stack instantiation (mcpt_debug_tiny_lds_stack)."""
        self._ck(lib().mcpt_debug_tiny_lds_stack(self.h, int(bool(on))))

    def set_tiles(self, tiles=None):
        if tiles is None:
            self._ck(lib().mcpt_set_tiles(self.h, None, 0))
        else:
            t = np.ascontiguousarray(tiles, np.uint32).reshape(-1, 2)
            self._ck(lib().mcpt_set_tiles(self.h, t.ctypes.data_as(_u), len(t)))

    def step(self, tile_x, tile_y) -> StageStats:
        st = StageStats()
        self._ck(lib().mcpt_wavefront_step(self.h, tile_x, tile_y, C.byref(st)))
        return st

    def iterate(self, n) -> StageStats:
        st = StageStats()
        self._ck(lib().mcpt_iterate(self.h, n, C.byref(st)))
        return st

    def render(self) -> StageStats:
        st = StageStats()
        self._ck(lib().mcpt_render(self.h, C.byref(st)))
        return st

    def film(self):
        P = self.W * self.H
        Ld = np.zeros(3 * P, np.float32)
        s = np.zeros(P, np.uint32)
        self._ck(lib().mcpt_film_read(self.h, fptr(Ld), s.ctypes.data_as(_u)))
        return Ld.reshape(self.H, self.W, 3), s.reshape(self.H, self.W)

    def tonemap(self, exposure=1.0, denoised=False):
        """Reinhard-tonemapped RGBA8 of the film, or with denoised=True of the last denoise()."""
        out = np.zeros(self.W * self.H * 4, np.uint8)
        fn = lib().mcpt_denoised_tonemap_rgba8 if denoised else lib().mcpt_film_tonemap_rgba8
        self._ck(fn(self.h, exposure, out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out.reshape(self.H, self.W, 4)

    def render_guides(self, n=1):
        """First-hit guide buffers of the film under the current camera (mcpt_guides_render): n guide
        samples per pixel along the camera rays of film samples 0..n-1."""
        self._ck(lib().mcpt_guides_render(self.h, n))

    def guides(self) -> dict:
        """Guide sums and counts (mcpt_guides_read): albedo / normal (H, W, 3), depth / count (H, W)."""
        P = self.W * self.H
        a, n = np.zeros(3 * P, np.float32), np.zeros(3 * P, np.float32)
        z, cnt = np.zeros(P, np.float32), np.zeros(P, np.uint32)
        self._ck(lib().mcpt_guides_read(self.h, fptr(a), fptr(n), fptr(z), cnt.ctypes.data_as(_u)))
        return {"albedo": a.reshape(self.H, self.W, 3), "normal": n.reshape(self.H, self.W, 3),
                "depth": z.reshape(self.H, self.W), "count": cnt.reshape(self.H, self.W)}

    def denoise(self, **params):
        """A-trous filter of the film with the context's guides (mcpt_film_denoise); keyword
        arguments override the default parameters (passes, sigma_color, sigma_normal, ...)."""
        p = denoise_params(**params) if params else None
        self._ck(lib().mcpt_film_denoise(self.h, C.byref(p) if p is not None else None))

    def denoised(self):
        """The last denoise() result as (H, W, 3) float32 (mcpt_denoised_read)."""
        out = np.zeros(3 * self.W * self.H, np.float32)
        self._ck(lib().mcpt_denoised_read(self.h, fptr(out)))
        return out.reshape(self.H, self.W, 3)

    def denoise_guided(self, **params):
        """Variance-guided a-trous filter of the film (mcpt_film_denoise_guided): the variance is the
        squared standard error of a fresh film error estimate (>= 2 path slots; with
        set_variance_fill() the spatial estimate fills in, and one slot is enough).  The result is read
        like denoise()'s; keyword arguments override the defaults (passes, sigma_lum, lum_eps, ...)."""
        p = denoise_guided_params(**params) if params else None
        self._ck(lib().mcpt_film_denoise_guided(self.h, C.byref(p) if p is not None else None))

    def denoised_variance(self):
        """The filtered variances of the last denoise_guided() as (H, W) float32, -1 where unknown
        (mcpt_denoised_variance_read)."""
        out = np.zeros(self.W * self.H, np.float32)
        self._ck(lib().mcpt_denoised_variance_read(self.h, fptr(out)))
        return out.reshape(self.H, self.W)

    def write_denoised_png(self, path, exposure=1.0):
        """Tonemapped denoised frame as 8-bit RGB PNG (mcpt_denoised_write_png)."""
        self._ck(lib().mcpt_denoised_write_png(self.h, exposure, os.fsencode(path)))

    def denoise_ms(self) -> dict:
        """Device times of the last guide pass and the last filter run (mcpt_debug_denoise_ms)."""
        v = (C.c_float * 10)()
        self._ck(lib().mcpt_debug_denoise_ms(self.h, v))
        return {"guides": float(v[0]), "prepare": float(v[1]), "passes": [float(x) for x in v[2:]]}

    # ---- temporal accumulation ----
    def set_seed(self, seed):
        """Seed of the live context (mcpt_set_seed): clears the film and makes the guides stale; the
        temporal history stays."""
        self._ck(lib().mcpt_set_seed(self.h, int(seed)))
        self.cfg.seed = int(seed)

    def temporal_accumulate(self, **params):
        """Reproject the previous accumulated frame into the film's and blend the two
        (mcpt_film_temporal); keyword arguments override the defaults (pos_tol, nrm_tol, max_history,
        alpha_min).  Needs render_guides() under the current camera."""
        p = temporal_params(**params) if params else None
        self._ck(lib().mcpt_film_temporal(self.h, C.byref(p) if p is not None else None))

    def temporal(self) -> dict:
        """The last accumulated frame (mcpt_temporal_read): rgb / position (H, W, 3), nsamples /
        variance (H, W; variance -1 where unknown)."""
        P = self.W * self.H
        rgb, pos = np.zeros(3 * P, np.float32), np.zeros(3 * P, np.float32)
        ns, var = np.zeros(P, np.float32), np.zeros(P, np.float32)
        self._ck(lib().mcpt_temporal_read(self.h, fptr(rgb), fptr(ns), fptr(var), fptr(pos)))
        return {"rgb": rgb.reshape(self.H, self.W, 3), "nsamples": ns.reshape(self.H, self.W),
                "variance": var.reshape(self.H, self.W), "position": pos.reshape(self.H, self.W, 3)}

    def temporal_denoise(self, **params):
        """The guided a-trous passes over the last accumulated frame (mcpt_temporal_denoise); read the
        result like denoise_guided()'s.  Keyword arguments override the guided defaults."""
        p = denoise_guided_params(**params) if params else None
        self._ck(lib().mcpt_temporal_denoise(self.h, C.byref(p) if p is not None else None))

    def temporal_reset(self):
        """Drop the temporal history (mcpt_temporal_reset): the next temporal_accumulate() starts over."""
        self._ck(lib().mcpt_temporal_reset(self.h))

    def temporal_bytes(self) -> int:
        """Device bytes held for the temporal stage (mcpt_debug_temporal_bytes): 0 until it is used."""
        return int(lib().mcpt_debug_temporal_bytes(self.h))

    def temporal_ms(self) -> float:
        """Device time of the last k_temporal launch (mcpt_debug_temporal_ms)."""
        v = (C.c_float * 1)()
        self._ck(lib().mcpt_debug_temporal_ms(self.h, v))
        return float(v[0])

    # ---- spatial variance estimate ----
    def set_variance_fill(self, *off, **params):
        """mcpt_set_variance_fill: set_variance_fill(**params) makes denoise_guided() and
        temporal_accumulate() fill the variances the path slots do not give with the spatial estimate
        (keyword arguments override the defaults: radius, sigma_normal, sigma_albedo, sigma_depth,
        min_neff), which makes both usable with one path slot; set_variance_fill(None) turns it off."""
        if off:
            if len(off) != 1 or off[0] is not None or params:
                raise TypeError("set_variance_fill takes keyword parameters, or None alone")
            self._ck(lib().mcpt_set_variance_fill(self.h, None))
            return
        p = variance_params(**params)
        self._ck(lib().mcpt_set_variance_fill(self.h, C.byref(p)))

    def variance_ms(self) -> float:
        """Device time of the last k_variance_spatial launch (mcpt_debug_variance_ms)."""
        v = (C.c_float * 1)()
        self._ck(lib().mcpt_debug_variance_ms(self.h, v))
        return float(v[0])

    # ---- adaptive sampling ----
    def set_sample_budget(self, budget=None):
        """Per-pixel sample budget ((H, W) uint32; mcpt_set_sample_budget) in place of the uniform spp;
        None removes it.  The film is not cleared: the next render() picks raised budgets up."""
        if budget is None:
            self._ck(lib().mcpt_set_sample_budget(self.h, None))
            return
        b = np.ascontiguousarray(budget, np.uint32)
        if b.shape != (self.H, self.W):
            raise ValueError(f"budget must be ({self.H}, {self.W}), got {b.shape}")
        self._ck(lib().mcpt_set_sample_budget(self.h, b.ctypes.data_as(_u)))

    def sample_budget(self):
        """The installed budget map as (H, W) uint32 (mcpt_sample_budget_read; raises when there is none)."""
        out = np.zeros((self.H, self.W), np.uint32)
        self._ck(lib().mcpt_sample_budget_read(self.h, out.ctypes.data_as(_u)))
        return out

    def set_spp(self, spp):
        """Uniform sample count of the live context (mcpt_set_spp); the film is kept, so a following
        render() continues the frame."""
        self._ck(lib().mcpt_set_spp(self.h, int(spp)))
        self.cfg.spp = int(spp)

    def film_error(self):
        """Error estimate from the path slots (mcpt_film_error + mcpt_film_error_read): (H, W, 4)
        float32 {standard error of the mean luminance (-1: none), mean luminance, slots with samples,
        samples}."""
        self._ck(lib().mcpt_film_error(self.h))
        out = np.zeros((self.H, self.W, 4), np.float32)
        self._ck(lib().mcpt_film_error_read(self.h, fptr(out)))
        return out

    def film_slot(self, slot):
        """One path slot's accumulators as images (mcpt_debug_film_read_slot): (H, W, 3) Ld, (H, W) samples."""
        Ld = np.zeros((self.H, self.W, 3), np.float32)
        s = np.zeros((self.H, self.W), np.uint32)
        self._ck(lib().mcpt_debug_film_read_slot(self.h, slot, fptr(Ld), s.ctypes.data_as(_u)))
        return Ld, s

    def budget_from_error(self, **params) -> dict:
        """Budgets from the last film_error(), installed (mcpt_budget_from_error); keyword arguments
        override the default parameters (target_rel_err, lum_floor, min_spp, max_spp)."""
        p = sample_budget_params(**params)
        v = (C.c_uint64 * 3)()
        self._ck(lib().mcpt_budget_from_error(self.h, C.byref(p), v))
        return dict(total=int(v[0]), max=int(v[1]), unchanged=int(v[2]))

    def render_adaptive(self, target=None, min_spp=None, max_spp=None, rounds=2):
        """Render to min_spp, then `rounds` times: estimate the film's error, build budgets that aim at
        a relative standard error `target` within [min_spp, max_spp], and render on.  Needs >= 2 path
        slots.  Returns the render() statistics of every pass and the budget summaries."""
        kw = {k: v for k, v in (("target_rel_err", target), ("min_spp", min_spp), ("max_spp", max_spp)) if v is not None}
        p = sample_budget_params(**kw)
        self.set_sample_budget(None)
        self.set_spp(p.min_spp)
        stats, budgets = [self.render()], []
        for _ in range(rounds):
            self._ck(lib().mcpt_film_error(self.h))
            budgets.append(self.budget_from_error(**kw))
            stats.append(self.render())
        return stats, budgets

    @property
    def adaptive_bytes(self) -> int:
        """Device bytes held for adaptive sampling (mcpt_debug_adaptive_bytes)."""
        return int(lib().mcpt_debug_adaptive_bytes(self.h))

    def adaptive_ms(self) -> dict:
        """Device times of the last error and budget kernels (mcpt_debug_adaptive_ms)."""
        v = (C.c_float * 2)()
        self._ck(lib().mcpt_debug_adaptive_ms(self.h, v))
        return {"error": float(v[0]), "budget": float(v[1])}

    def trace_closest(self, ro, rd, steps=False):
        ro = np.ascontiguousarray(ro, np.float32).reshape(-1, 3)
        rd = np.ascontiguousarray(rd, np.float32).reshape(-1, 3)
        n = len(ro)
        pos_t = np.zeros((n, 4), np.float32)
        nrm = np.zeros((n, 4), np.float32)
        tri = np.zeros(n, np.int32)
        st = np.zeros(n, np.uint32) if steps else None
        vin = SoaView(fptr(ro), fptr(rd), None, None, None, None, None)
        vout = SoaView(None, None, fptr(pos_t), fptr(nrm), tri.ctypes.data_as(_i), None,
                       st.ctypes.data_as(_u) if steps else None)
        self._ck(lib().mcpt_stage_run(self.h, STAGE_EXTEND, C.byref(vin), C.byref(vout), n))
        return (pos_t, nrm, tri, st) if steps else (pos_t, nrm, tri)

    def trace_any(self, ro, rd, steps=False):
        ro = np.ascontiguousarray(ro, np.float32).reshape(-1, 3)
        rd = np.ascontiguousarray(rd, np.float32).reshape(-1, 3)
        n = len(ro)
        vis = np.zeros(n, np.uint8)
        st = np.zeros(n, np.uint32) if steps else None
        vin = SoaView(fptr(ro), fptr(rd), None, None, None, None, None)
        vout = SoaView(None, None, None, None, None, vis.ctypes.data_as(C.POINTER(C.c_uint8)),
                       st.ctypes.data_as(_u) if steps else None)
        self._ck(lib().mcpt_stage_run(self.h, STAGE_SHADOW, C.byref(vin), C.byref(vout), n))
        return (vis, st) if steps else vis

    def stage(self, name, state: dict, film=None) -> dict:
        """mcpt_stage_run of one shading stage ("logic", "generate", "material") over caller path
        state (numpy arrays keyed as mcpt_path_view's fields, n paths); returns every output
        field.  film=(W, H) for logic / generate: path i is pixel (i % W, i // W)."""
        n = len(state["flags"])
        film = film or (0, 0)
        vin = SoaView()
        pin = path_view(state, n, film)
        vin.paths = C.pointer(pin)
        outs = {k: np.zeros((n, m) if m > 1 else n, dt) for k, (dt, m) in PATH_FIELDS.items()}
        vout = SoaView()
        pout = path_view(outs, n, film)
        vout.paths = C.pointer(pout)
        self._ck(lib().mcpt_stage_run(self.h, STAGE_BY_NAME[name], C.byref(vin), C.byref(vout), n))
        return {k: pout._keep[k].reshape(outs[k].shape) for k in outs}

    @property
    def last_stage_ms(self) -> float:
        return lib().mcpt_debug_last_stage_ms(self.h)

    def write_png(self, path, exposure=1.0):
        """Tonemapped film as 8-bit RGB PNG (mcpt_film_write_png)."""
        self._ck(lib().mcpt_film_write_png(self.h, exposure, os.fsencode(path)))

    def write_pfm(self, path):
        """Averaged radiance Ld/samples as float RGB PFM (mcpt_film_write_pfm)."""
        self._ck(lib().mcpt_film_write_pfm(self.h, os.fsencode(path)))

    def trace_profile(self, reset=True):
        """k_trace loop-phase counts of the counting build (mcpt_debug_trace_profile; work counters on)
        since the last film clear or reset, as a dict of wave-summed counts (None: none recorded)."""
        v = (C.c_uint64 * 12)()
        n = lib().mcpt_debug_trace_profile(self.h, v, int(reset))
        names = ("trips", "refills", "refill_lanes", "node_iters", "tri_phases", "tri_lanes", "trip_node_lanes",
                 "trip_leaf_lanes", "trip_idle_lanes", "finish_trips", "pop_iters")
        return {k: int(x) for k, x in zip(names, v)} if n > 0 else None

    def hbm_copy_gbps(self, nbytes=1 << 30, iters=20) -> float:
        """Measured HBM copy ceiling (read + write GB/s) of a hand-written dwordx4 copy kernel."""
        g = C.c_double(0.0)
        self._ck(lib().mcpt_debug_hbm_copy(self.h, nbytes, iters, C.byref(g)))
        return g.value

    def debug_quot(self, a, b):
        """a / b as the kernels divide (shared fp64 reciprocal, mcpt_core.hpp quot3)."""
        a = np.ascontiguousarray(a, np.float32)
        b = np.ascontiguousarray(b, np.float32)
        out = np.empty_like(a)
        self._ck(lib().mcpt_debug_quot(self.h, a.ctypes.data, b.ctypes.data, a.size, out.ctypes.data))
        return out

    def queue_rays(self):
        """Rays of the current extension queue (diagnostics)."""
        n = C.c_uint32(0)
        self._ck(lib().mcpt_debug_queue_rays(self.h, 0, None, None, C.byref(n)))
        ro = np.zeros((n.value, 3), np.float32)
        rd = np.zeros((n.value, 3), np.float32)
        self._ck(lib().mcpt_debug_queue_rays(self.h, 0, fptr(ro), fptr(rd), C.byref(n)))
        return ro[: n.value], rd[: n.value]


def denoise_params(**kw) -> DenoiseParams:
    """mcpt_denoise_default_params with keyword overrides."""
    p = DenoiseParams()
    _check(lib().mcpt_denoise_default_params(C.byref(p)))
    for k, v in kw.items():
        if k not in dict(DenoiseParams._fields_):
            raise TypeError(f"unknown denoise parameter {k!r}")
        setattr(p, k, v)
    return p


def denoise_guided_params(**kw) -> DenoiseGuidedParams:
    """mcpt_denoise_guided_default_params with keyword overrides."""
    p = DenoiseGuidedParams()
    _check(lib().mcpt_denoise_guided_default_params(C.byref(p)))
    for k, v in kw.items():
        if k not in dict(DenoiseGuidedParams._fields_):
            raise TypeError(f"unknown guided denoise parameter {k!r}")
        setattr(p, k, v)
    return p


def temporal_params(**kw) -> TemporalParams:
    """mcpt_temporal_default_params with keyword overrides."""
    p = TemporalParams()
    _check(lib().mcpt_temporal_default_params(C.byref(p)))
    for k, v in kw.items():
        if k not in dict(TemporalParams._fields_):
            raise TypeError(f"unknown temporal parameter {k!r}")
        setattr(p, k, v)
    return p


def camera_view_proj(cam: Camera):
    """proj * view of a Camera as 16 float32, column-major (mcpt_camera_view_proj): the inverse of its
    inv_view_proj, the matrix the temporal stage projects into the previous frame with."""
    out = np.zeros(16, np.float32)
    _check(lib().mcpt_camera_view_proj(C.byref(cam), fptr(out)))
    return out


def temporal_run(pt, rgb, samples, variance, position, normal, depth, hcol, hpos, hnrm, vp_prev, **params):
    """mcpt_temporal_run on PathTracer pt: the temporal stage over host images of the current frame
    ((H, W, 3) rgb / position / normal, (H, W) samples / variance / depth), the three (H, W, 4) history
    planes of the previous call and VP_prev; returns (col (H, W, 4), vl (H, W, 2), hcol, hpos, hnrm)."""
    rgb = np.ascontiguousarray(rgb, np.float32)
    H, W = rgb.shape[:2]
    sm = np.ascontiguousarray(samples, np.uint32).reshape(H, W)
    var = np.ascontiguousarray(variance, np.float32).reshape(H, W)
    pos = np.ascontiguousarray(position, np.float32).reshape(H, W, 3)
    nm = np.ascontiguousarray(normal, np.float32).reshape(H, W, 3)
    z = np.ascontiguousarray(depth, np.float32).reshape(H, W)
    hist = [np.ascontiguousarray(a, np.float32).reshape(H, W, 4) for a in (hcol, hpos, hnrm)]
    vp = np.ascontiguousarray(vp_prev, np.float32).reshape(16)
    out = [np.zeros((H, W, k), np.float32) for k in (4, 2, 4, 4, 4)]
    p = temporal_params(**params)
    _check(lib().mcpt_temporal_run(pt.h, W, H, fptr(rgb), sm.ctypes.data_as(_u), fptr(var), fptr(pos), fptr(nm), fptr(z),
                                   *(fptr(a) for a in hist), fptr(vp), C.byref(p), *(fptr(a) for a in out)), pt.h)
    return tuple(out)


def sample_budget_params(**kw) -> SampleBudgetParams:
    """mcpt_sample_budget_default_params with keyword overrides."""
    p = SampleBudgetParams()
    _check(lib().mcpt_sample_budget_default_params(C.byref(p)))
    for k, v in kw.items():
        if k not in dict(SampleBudgetParams._fields_):
            raise TypeError(f"unknown sample budget parameter {k!r}")
        setattr(p, k, v)
    return p


def error_run(pt, Ld_slots, samples_slots):
    """mcpt_error_run on PathTracer pt: the error estimate over host slot images ((S, H, W, 3) radiance
    sums and (S, H, W) sample counts); returns (H, W, 4) float32."""
    L = np.ascontiguousarray(Ld_slots, np.float32)
    S, H, W = L.shape[:3]
    n = np.ascontiguousarray(samples_slots, np.uint32).reshape(S, H, W)
    out = np.zeros((H, W, 4), np.float32)
    _check(lib().mcpt_error_run(pt.h, W, H, S, fptr(L), n.ctypes.data_as(_u), fptr(out)), pt.h)
    return out


def denoise_run(pt, rgb, albedo, normal, depth, samples=None, **params):
    """mcpt_denoise_run on PathTracer pt: the filter over host images of means ((H, W, 3) rgb, albedo
    and normal, (H, W) depth and optional sample counts); returns the filtered (H, W, 3) image."""
    rgb = np.ascontiguousarray(rgb, np.float32)
    H, W = rgb.shape[:2]
    al = np.ascontiguousarray(albedo, np.float32).reshape(H, W, 3)
    nm = np.ascontiguousarray(normal, np.float32).reshape(H, W, 3)
    z = np.ascontiguousarray(depth, np.float32).reshape(H, W)
    sm = None if samples is None else np.ascontiguousarray(samples, np.uint32).reshape(H, W)
    out = np.zeros((H, W, 3), np.float32)
    p = denoise_params(**params)
    _check(lib().mcpt_denoise_run(pt.h, W, H, fptr(rgb), None if sm is None else sm.ctypes.data_as(_u), fptr(al),
                                  fptr(nm), fptr(z), C.byref(p), fptr(out)), pt.h)
    return out


def denoise_guided_run(pt, rgb, variance, albedo, normal, depth, samples=None, **params):
    """mcpt_denoise_guided_run on PathTracer pt: denoise_run's images plus an (H, W) variance of the
    mean luminance (a value outside [0, FLT_MAX]: unknown); returns the filtered (H, W, 3) image and
    the filtered (H, W) variances (-1 where unknown)."""
    rgb = np.ascontiguousarray(rgb, np.float32)
    H, W = rgb.shape[:2]
    var = np.ascontiguousarray(variance, np.float32).reshape(H, W)
    al = np.ascontiguousarray(albedo, np.float32).reshape(H, W, 3)
    nm = np.ascontiguousarray(normal, np.float32).reshape(H, W, 3)
    z = np.ascontiguousarray(depth, np.float32).reshape(H, W)
    sm = None if samples is None else np.ascontiguousarray(samples, np.uint32).reshape(H, W)
    out = np.zeros((H, W, 3), np.float32)
    out_v = np.zeros((H, W), np.float32)
    p = denoise_guided_params(**params)
    _check(lib().mcpt_denoise_guided_run(pt.h, W, H, fptr(rgb), None if sm is None else sm.ctypes.data_as(_u), fptr(var),
                                         fptr(al), fptr(nm), fptr(z), C.byref(p), fptr(out), fptr(out_v)), pt.h)
    return out, out_v


def variance_params(**kw) -> VarianceParams:
    """mcpt_variance_default_params with keyword overrides."""
    p = VarianceParams()
    _check(lib().mcpt_variance_default_params(C.byref(p)))
    for k, v in kw.items():
        if k not in dict(VarianceParams._fields_):
            raise TypeError(f"unknown variance parameter {k!r}")
        setattr(p, k, v)
    return p


def variance_run(pt, rgb, albedo, normal, depth, samples=None, variance=None, **params):
    """mcpt_variance_run on PathTracer pt: the spatial variance estimate over denoise_guided_run's host
    images; variance (H, W) holds what is already known (None: nothing).  Returns (H, W) float32: the
    known inputs unchanged, the estimate elsewhere, -1 where unknown."""
    rgb = np.ascontiguousarray(rgb, np.float32)
    H, W = rgb.shape[:2]
    al = np.ascontiguousarray(albedo, np.float32).reshape(H, W, 3)
    nm = np.ascontiguousarray(normal, np.float32).reshape(H, W, 3)
    z = np.ascontiguousarray(depth, np.float32).reshape(H, W)
    sm = None if samples is None else np.ascontiguousarray(samples, np.uint32).reshape(H, W)
    var = None if variance is None else np.ascontiguousarray(variance, np.float32).reshape(H, W)
    out = np.zeros((H, W), np.float32)
    p = variance_params(**params)
    _check(lib().mcpt_variance_run(pt.h, W, H, fptr(rgb), None if sm is None else sm.ctypes.data_as(_u),
                                   None if var is None else fptr(var), fptr(al), fptr(nm), fptr(z), C.byref(p), fptr(out)),
           pt.h)
    return out


def gather(tracers, root=0):
    """mcpt_gather: copy every PathTracer's tile-set pixels into tracers[root]'s film (one process,
    one context per GPU, device-to-device over xGMI)."""
    arr = (C.c_void_p * len(tracers))(*[t.h for t in tracers])
    _check(lib().mcpt_gather(arr, len(tracers), root), tracers[root].h)


@dataclass(frozen=True)
class RenderConfig:
    """BASELINE.json configs."""
    cid: int
    width: int
    height: int
    spp: int
    max_depth: int
    position: tuple
    yaw: float = -90.0
    pitch: float = 0.0
    fovy: float = 45.0


CONFIGS = {
    1: RenderConfig(1, 256, 256, 16, 3, (0.0, 0.0, 4.0)),
    2: RenderConfig(2, 1920, 1080, 256, 5, (0.0, 0.0, 3.5)),
    3: RenderConfig(3, 1920, 1080, 256, 5, (0.0, 1.5, 4.5), pitch=-10.0),
    4: RenderConfig(4, 3840, 2160, 1024, 8, (0.0, 0.0, 2.5)),
    5: RenderConfig(5, 4096, 4096, 4096, 12, (0.0, 1.2, 3.0), pitch=-5.0),
}


def write_png(path, rgba8):
    """Write an (H, W, 4) uint8 buffer as RGB PNG (mcpt_image_write_png; host-only, no GPU)."""
    a = np.ascontiguousarray(rgba8, np.uint8)
    h, w = a.shape[:2]
    rc = lib().mcpt_image_write_png(os.fsencode(path), w, h, a.ctypes.data_as(C.POINTER(C.c_uint8)))
    if rc != 0:
        raise McptError(f"mcpt_image_write_png failed ({rc})")


def read_png(path_or_bytes):
    """Decode a PNG file (a path) or payload (bytes) into an (h, w, 4) uint8 array, row 0 of the file first
    (mcpt_image_read_png / _memory: the project's own inflate and PNG decoder; host-only, no GPU).  What
    Scene.set_texture and PathTracer.set_textures take.  McptError with the decoder's reason for a file it
    refuses (DESIGN.md section 22 lists what it accepts)."""
    w, h = C.c_int32(0), C.c_int32(0)
    mem = isinstance(path_or_bytes, (bytes, bytearray, memoryview))
    if mem:
        data = bytes(path_or_bytes)
        call = lambda buf, cap: lib().mcpt_image_read_png_memory(data, len(data), C.byref(w), C.byref(h), buf, cap)
    else:
        name = os.fsencode(path_or_bytes)
        call = lambda buf, cap: lib().mcpt_image_read_png(name, C.byref(w), C.byref(h), buf, cap)
    rc = call(None, 0)
    if rc == 0:
        out = np.zeros((h.value, w.value, 4), np.uint8)
        rc = call(out.ctypes.data_as(C.POINTER(C.c_uint8)), out.size)
    if rc != 0:
        raise McptError(f"read_png failed ({rc}): {lib().mcpt_image_read_png_error().decode()}")
    return out


def write_pfm(path, rgb):
    """Write an (H, W, 3) float buffer as PFM (mcpt_image_write_pfm; host-only, no GPU)."""
    a = np.ascontiguousarray(rgb, np.float32)
    h, w = a.shape[:2]
    rc = lib().mcpt_image_write_pfm(os.fsencode(path), w, h, a.ctypes.data_as(C.POINTER(C.c_float)))
    if rc != 0:
        raise McptError(f"mcpt_image_write_pfm failed ({rc})")


# The build's default BVH: binned SAH over all three axes (mcpt_scene_build_ex).  On config 2 it
# traces ~14% faster than BVHAccel's single-axis 12-bucket SAH; films are identical for any tree.
DEFAULT_BVH = dict(builder="sah3", buckets=128, trav_cost=0.5, isect_cost=1.0, max_prims=8)
# A/B knobs for the builder's cost model (films do not depend on the tree)
for _k, _env, _t in (("trav_cost", "MCPT_BVH_TRAV_COST", float), ("max_prims", "MCPT_BVH_MAX_PRIMS", int),
                     ("builder", "MCPT_BVH_BUILDER", str), ("buckets", "MCPT_BVH_BUCKETS", int),
                     ("isect_cost", "MCPT_BVH_ISECT_COST", float)):
    if os.environ.get(_env):
        DEFAULT_BVH[_k] = _t(os.environ[_env])


def build_config_scene(cid: int, asset_dir=ASSET_DIR, **build_kw) -> Scene:
    """BASELINE config cid's proxy scene, built with DEFAULT_BVH (or ``builder="reference"``, ...)."""
    s = Scene()
    s.make_proxy(cid, asset_dir)
    if (DEFAULT_BVH | build_kw).get("builder") == "reference":
        s.build(max_prims=(DEFAULT_BVH | build_kw).get("max_prims", 8))
    else:
        s.build(**(DEFAULT_BVH | build_kw))
    return s


def config_camera(rc: RenderConfig, width=None, height=None) -> Camera:
    w, h = width or rc.width, height or rc.height
    return make_camera(rc.position, rc.yaw, rc.pitch, rc.fovy, aspect=np.float32(w) / np.float32(h))
