"""fovrt — Python mirror of the reference's renderer classes over the libfovrt C ABI.

The reference drives its hot path from C++ (FR/main.cpp:152-462) through the classes
``PathTracer``, ``JumpFlooding``, ``SibsonInterpolation``, ``PullPushInterpolation``, ``ATrous`` and
``Camera``.  This module exposes the same names, method names and argument order on top of
``include/fovrt.h`` (ctypes, no torch types), so tests and the benchmark read like the reference's
frame loop.  GL texture handles become fr_buffer_id integers; ``get_texture`` returns the buffer id
and ``read`` copies a buffer to a numpy array.

Nothing here computes pixels: every stage runs in the HIP kernels of libfovrt.so.  Importing this
module does not touch the GPU; creating a ``PathTracer`` does, and fails loudly (FovrtError) if the
library or a device is missing.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass

import numpy as np

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_PKG_DIR), "libfovrt.so")
REPO_ROOT = os.path.dirname(os.path.dirname(_PKG_DIR))
DEFAULT_ASSET_DIR = os.path.join(REPO_ROOT, "assets")

ABI_VERSION = 2  # FOVRT_ABI_VERSION of include/fovrt.h this mirror is written against
GROUP_MAX_VIEW_RANKS = 16
# fr_status
FR_OK, FR_E_INVALID, FR_E_HIP, FR_E_NOMEM, FR_E_IO, FR_E_STATE, FR_E_UNSUPPORTED = 0, -1, -2, -3, -4, -5, -6
# scenes / masks
SCENE_BOX, SCENE_BUNNY, SCENE_VOKSELIA = 0, 1, 2
# fr_update_positions: what follows the new positions, and where they come from
FR_BVH_REBUILD, FR_BVH_REFIT = 0, 1
FR_VISIBLE_ALL = 0xFFFFFFFF  # fr_set_model_visibility: every model visible
FR_MEM_HOST, FR_MEM_DEVICE = 0, 1
# fr_update_geometry: what becomes of the shading normals
FR_NORMALS_KEEP, FR_NORMALS_GIVEN, FR_NORMALS_RECOMPUTE = 0, 1, 2
# fr_trace_rays: what a query answers
FR_RAYS_CLOSEST, FR_RAYS_TRANSMITTANCE, FR_RAYS_SURFACE = 0, 1, 2
RAY_KINDS = {"closest": FR_RAYS_CLOSEST, "transmittance": FR_RAYS_TRANSMITTANCE, "surface": FR_RAYS_SURFACE}
MASK_SALIENCY, MASK_LOGPOLAR, MASK_UNIFORM2X2, MASK_ALL, MASK_LOGPOLAR_SIGNED = 0, 1, 2, 3, 4
MASK_ECCENTRIC, MASK_CALLER = 5, 6  # fr_set_foveation / fr_set_sampling_mask
# fr_set_pipeline_mode
PIPELINE_THROUGHPUT, PIPELINE_LATENCY = 0, 1
# fr_present_enable: the byte order of a presented texel; TOP_DOWN is or-ed in (row 0 of the output = the top row)
FR_PRESENT_RGBA8, FR_PRESENT_BGRA8, FR_PRESENT_TOP_DOWN = 0, 1, 0x100
FR_PRESENT_PENDING = 1  # fr_present_acquire without waiting: the frame is not there yet
SCENES = {"box": SCENE_BOX, "bunny": SCENE_BUNNY, "vokselia": SCENE_VOKSELIA}
MASKS = {"saliency": MASK_SALIENCY, "logpolar": MASK_LOGPOLAR, "uniform": MASK_UNIFORM2X2, "all": MASK_ALL,
         "logpolar10": MASK_LOGPOLAR_SIGNED}
# the steered modes: entered with PathTracer.set_mask_mode (a context is created in one of MASKS)
STEERED_MASKS = {"eccentric": MASK_ECCENTRIC, "caller": MASK_CALLER}


class TextureName:
    """PathTracer::TextureName (FR/PathTracer.h:13-31) plus the reconstruction outputs."""
    POSITION, NORMAL, DEPTH, DIFFUSE, WEIGHT, THREAD, HISTORY, SHADING, EXTRA = range(9)
    JFA_COORD, JFA_COLOR, SIBSON, PULLPUSH, ATROUS, DEPTH_CACHE, HISTORY_CACHE, MASK = range(9, 17)
    LOGPOLAR, LOGPOLAR_INVERSE, GCLASS = 17, 18, 19


class FovrtError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"fovrt error {code}: {msg}")
        self.code = code


class fr_config(C.Structure):
    _fields_ = [("abi_version", C.c_int), ("width", C.c_int), ("height", C.c_int), ("scene", C.c_int),
                ("mask_mode", C.c_int),
                ("spp", C.c_int), ("diffuse_max_depth", C.c_int), ("refraction_max_depth", C.c_int),
                ("light_power", C.c_float), ("optimize", C.c_int), ("atrous_iterations", C.c_int),
                ("write_extra", C.c_int), ("device", C.c_int), ("texture_mode", C.c_int), ("detail", C.c_int),
                ("mesh_mode", C.c_int), ("bvh_builder", C.c_int), ("sibson_mode", C.c_int),
                ("asset_dir", C.c_char_p)]


class fr_camera(C.Structure):
    _fields_ = [("eye", C.c_float * 3), ("prev_eye", C.c_float * 3), ("inv_vp", C.c_float * 16),
                ("prev_vp", C.c_float * 16), ("up", C.c_float * 3), ("target", C.c_float * 3),
                ("gaze", C.c_float * 2)]


class fr_camera_pose(C.Structure):
    _fields_ = [("pos", C.c_float * 3), ("rot", C.c_float * 4), ("fovy_deg", C.c_float),
                ("znear", C.c_float), ("zfar", C.c_float), ("aspect", C.c_float)]


class fr_buffer_view(C.Structure):
    _fields_ = [("device_ptr", C.c_void_p), ("width", C.c_int), ("height", C.c_int),
                ("pitch_bytes", C.c_size_t), ("bytes", C.c_size_t), ("format", C.c_int)]


class fr_stats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("gbuffer_primary", "primary", "shadow", "diffuse_bounce", "mirror",
                                          "refraction", "reflection", "truncated", "overflow", "segments")] + \
                [("diag", C.c_uint64 * 6)]


class fr_frame_timing(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("geometry_ms", "sampling_ms", "optimize_ms", "shading_ms", "jfa_ms",
                                         "sibson_ms", "pullpush_ms", "atrous_ms", "total_ms")] + \
               [("ray_count", C.c_uint32), ("shade_paths_ms", C.c_float)]


class fr_stage_times(C.Structure):
    _fields_ = [("frames", C.c_uint32), ("shading_ms", C.c_double), ("shade_paths_ms", C.c_double)]


class fr_group_config(C.Structure):
    _fields_ = [("views", C.c_int), ("tile", C.c_int), ("split_recon", C.c_int), ("moving_camera", C.c_int),
                ("composite", C.c_int), ("recon_cost", C.c_float * 2), ("weights", C.c_float * GROUP_MAX_VIEW_RANKS),
                ("sample_sum", C.c_int), ("front_local", C.c_int),
                ("jfa_ranks", C.c_int)]


class fr_foveation(C.Structure):
    _fields_ = [("radius_px", C.c_float), ("floor_ranks", C.c_int), ("ray_budget", C.c_uint32),
                ("tolerance", C.c_float)]


class fr_present_warp(C.Structure):
    _fields_ = [("h", C.c_float * 9), ("out_width", C.c_int), ("out_height", C.c_int)]


class fr_present_blend(C.Structure):
    _fields_ = [("inner_buffer", C.c_int), ("outer_buffer", C.c_int), ("gaze", C.c_float * 2),
                ("inner_radius_px", C.c_float), ("outer_radius_px", C.c_float)]


class fr_present_reproject(C.Structure):
    _fields_ = [("vp", C.c_float * 16), ("fallback", fr_present_warp)]


class fr_ray(C.Structure):
    _fields_ = [("origin", C.c_float * 3), ("tmin", C.c_float), ("dir", C.c_float * 3), ("tmax", C.c_float)]


class fr_ray_hit(C.Structure):
    _fields_ = [("t", C.c_float), ("beta", C.c_float), ("gamma", C.c_float), ("prim", C.c_int32)]


class fr_ray_surface(C.Structure):
    _fields_ = [("t", C.c_float), ("beta", C.c_float), ("gamma", C.c_float), ("prim", C.c_int32),
                ("point", C.c_float * 3), ("model", C.c_int32), ("ng", C.c_float * 3), ("u", C.c_float),
                ("ns", C.c_float * 3), ("v", C.c_float), ("kd", C.c_float * 3), ("surface", C.c_int32)]


# fr_ray / fr_ray_hit / fr_ray_surface as numpy record types (PathTracer.trace_rays)
RAY_DTYPE = np.dtype([("origin", np.float32, 3), ("tmin", np.float32), ("dir", np.float32, 3), ("tmax", np.float32)])
RAY_HIT_DTYPE = np.dtype([("t", np.float32), ("beta", np.float32), ("gamma", np.float32), ("prim", np.int32)])
RAY_SURFACE_DTYPE = np.dtype([("t", np.float32), ("beta", np.float32), ("gamma", np.float32), ("prim", np.int32),
                              ("point", np.float32, 3), ("model", np.int32), ("ng", np.float32, 3), ("u", np.float32),
                              ("ns", np.float32, 3), ("v", np.float32), ("kd", np.float32, 3), ("surface", np.int32)])
_RAY_RESULT = {FR_RAYS_CLOSEST: RAY_HIT_DTYPE, FR_RAYS_TRANSMITTANCE: np.dtype(np.float32),
               FR_RAYS_SURFACE: RAY_SURFACE_DTYPE}


class fr_scene_arrays(C.Structure):
    _fields_ = [("num_tris", C.c_int), ("pos", C.POINTER(C.c_float)), ("nrm", C.POINTER(C.c_float)),
                ("uv", C.POINTER(C.c_float)), ("flags", C.POINTER(C.c_int32)), ("num_materials", C.c_int),
                ("materials", C.POINTER(C.c_int32)), ("num_textures", C.c_int), ("tex_dims", C.POINTER(C.c_int32)),
                ("tex_data", C.POINTER(C.POINTER(C.c_float))), ("envmap", C.c_int), ("light", C.c_float * 15),
                ("bbox", C.c_float * 6), ("bvh_nodes", C.c_int), ("bvh_depth", C.c_int),
                ("bvh_max_stack", C.c_int)]


# exported symbols and their signatures (kept in sync with include/fovrt.h)
_SIGS = {
    "fr_config_default": [C.POINTER(fr_config)],
    "fr_version": [],
    "fr_abi_version": [],
    "fr_create": [C.POINTER(fr_config), C.POINTER(C.c_void_p)],
    "fr_destroy": [C.c_void_p],
    "fr_last_error": [C.c_void_p],
    "fr_camera_look_at": [C.POINTER(fr_camera_pose), C.POINTER(C.c_float), C.POINTER(C.c_float)],
    "fr_camera_matrices": [C.POINTER(fr_camera_pose), C.POINTER(C.c_float), C.POINTER(C.c_float)],
    "fr_camera_uniforms": [C.POINTER(fr_camera_pose), C.POINTER(fr_camera_pose), C.c_int, C.c_int,
                           C.POINTER(fr_camera)],
    "fr_preset_camera": [C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float)],
    "fr_set_camera": [C.c_void_p, C.POINTER(fr_camera)],
    "fr_set_light_power": [C.c_void_p, C.c_float],
    "fr_set_diffuse_max_depth": [C.c_void_p, C.c_int],
    "fr_reset_accumulation": [C.c_void_p],
    "fr_accum_frame": [C.c_void_p, C.POINTER(C.c_uint32)],
    "fr_geometry_launch": [C.c_void_p, C.POINTER(C.c_float)],
    "fr_sampling_launch": [C.c_void_p, C.POINTER(C.c_float)],
    "fr_optimize_launch": [C.c_void_p, C.POINTER(C.c_float)],
    "fr_shading_launch": [C.c_void_p, C.POINTER(C.c_float)],
    "fr_ray_count": [C.c_void_p, C.POINTER(C.c_uint32)],
    "fr_gaze_target": [C.c_void_p, C.POINTER(C.c_float)],
    "fr_jfa_render": [C.c_void_p, C.c_int, C.POINTER(C.c_uint64)],
    "fr_sibson_render": [C.c_void_p, C.POINTER(C.c_uint64)],
    "fr_pullpush_render": [C.c_void_p, C.c_int, C.POINTER(C.c_uint64)],
    "fr_atrous_render": [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint64)],
    "fr_logpolar_render": [C.c_void_p, C.c_int, C.POINTER(C.c_uint64)],
    "fr_set_gaze": [C.c_void_p, C.c_double, C.c_double, C.c_int],
    "fr_reset_gaze": [C.c_void_p],
    "fr_composite_views": [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t],
    "fr_frame": [C.c_void_p, C.POINTER(fr_frame_timing)],
    "fr_set_recon_chains": [C.c_void_p, C.c_int],
    "fr_set_pipeline_mode": [C.c_void_p, C.c_int],
    "fr_set_sample_sum": [C.c_void_p, C.c_int],
    "fr_set_front_local": [C.c_void_p, C.c_int],
    "fr_shard_unpack_active_enqueue": [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32],
    "fr_trace_frame": [C.c_void_p, C.POINTER(fr_frame_timing)],
    "fr_reconstruct_frame": [C.c_void_p, C.POINTER(fr_frame_timing)],
    "fr_set_shard": [C.c_void_p, C.c_int, C.c_int, C.c_int],
    "fr_set_shard_ex": [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int],
    "fr_set_shard_plan": [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint8), C.c_size_t],
    "fr_shard_plan": [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.c_size_t],
    "fr_shard_counts": [C.c_void_p, C.POINTER(C.c_uint32), C.c_int],
    "fr_shard_pack_active": [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.POINTER(C.c_uint32)],
    "fr_shard_unpack_active": [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32],
    "fr_shard_texels": [C.c_void_p, C.POINTER(C.c_size_t)],
    "fr_shard_pack": [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t],
    "fr_shard_unpack": [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t],
    "fr_synchronize": [C.c_void_p],
    "fr_get_buffer": [C.c_void_p, C.c_int, C.POINTER(fr_buffer_view)],
    "fr_read_buffer": [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t],
    "fr_write_buffer": [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t],
    "fr_copy_buffer": [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t],
    "fr_snapshot_bytes": [C.c_void_p, C.POINTER(C.c_size_t)],
    "fr_snapshot": [C.c_void_p, C.c_void_p, C.c_size_t],
    "fr_restore": [C.c_void_p, C.c_void_p, C.c_size_t],
    "fr_rebuild_bvh": [C.c_void_p, C.POINTER(C.c_float)],
    "fr_set_positions": [C.c_void_p, C.POINTER(C.c_float), C.c_size_t],
    "fr_refit_bvh": [C.c_void_p, C.POINTER(C.c_float)],
    "fr_update_positions": [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int],
    "fr_bvh_sah_cost": [C.c_void_p, C.POINTER(C.c_float)],
    "fr_update_geometry": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int],
    "fr_update_geometry_enqueue": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p],
    "fr_geometry_consumed": [C.c_void_p, C.c_void_p],
    "fr_ray_query_reserve": [C.c_void_p, C.c_size_t],
    "fr_trace_rays": [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p],
    "fr_trace_rays_enqueue": [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p],
    "fr_rays_consumed": [C.c_void_p, C.c_void_p],
    "fr_ray_query_reserve_kind": [C.c_void_p, C.c_size_t, C.c_int, C.c_int],
    "fr_trace_rays_masked": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p],
    "fr_trace_rays_masked_enqueue": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p],
    "fr_set_geometry_overlap": [C.c_void_p, C.c_int],
    "fr_geometry_update_status": [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)],
    "fr_rebuild_bvh_enqueue": [C.c_void_p],
    "fr_bvh_rebuild_status": [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)],
    "fr_rebuild_bvh_enqueue_if": [C.c_void_p, C.c_float],
    "fr_set_rebuild_policy": [C.c_void_p, C.c_float, C.c_int],
    "fr_bvh_rebuild_policy_status": [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_float),
                                     C.POINTER(C.c_float)],
    "fr_model_count": [C.c_void_p, C.POINTER(C.c_int)],
    "fr_model_info": [C.c_void_p, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int), C.POINTER(C.c_int)],
    "fr_scene_model_count": [C.c_void_p, C.POINTER(C.c_int)],
    "fr_scene_model_info": [C.c_void_p, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int), C.POINTER(C.c_int)],
    "fr_model_pose_enable": [C.c_void_p, C.c_int],
    "fr_set_model_transforms": [C.c_void_p, C.POINTER(C.c_float), C.c_size_t, C.c_int],
    "fr_set_model_transforms_enqueue": [C.c_void_p, C.POINTER(C.c_float), C.c_size_t],
    "fr_model_transforms": [C.c_void_p, C.POINTER(C.c_float), C.c_size_t],
    "fr_model_visibility_enable": [C.c_void_p, C.c_int],
    "fr_set_model_visibility": [C.c_void_p, C.c_uint32, C.c_int],
    "fr_set_model_visibility_enqueue": [C.c_void_p, C.c_uint32],
    "fr_model_visibility": [C.c_void_p, C.POINTER(C.c_uint32)],
    "fr_foveation_default": [C.c_int, C.c_int, C.POINTER(fr_foveation)],
    "fr_set_foveation": [C.c_void_p, C.POINTER(fr_foveation)],
    "fr_get_foveation": [C.c_void_p, C.POINTER(fr_foveation)],
    "fr_foveation_mask": [C.c_int, C.c_int, C.POINTER(C.c_float), C.c_float, C.c_int, C.c_void_p,
                          C.POINTER(C.c_uint32)],
    "fr_foveation_status": [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64),
                            C.POINTER(C.c_uint64)],
    "fr_set_mask_mode": [C.c_void_p, C.c_int],
    "fr_get_mask_mode": [C.c_void_p, C.POINTER(C.c_int)],
    "fr_sampling_mask_enable": [C.c_void_p, C.c_int],
    "fr_set_sampling_mask": [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int],
    "fr_set_sampling_mask_enqueue": [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p],
    "fr_sampling_mask_consumed": [C.c_void_p, C.c_void_p],
    "fr_present_pack": [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p],
    "fr_present_enable": [C.c_void_p, C.c_int, C.c_int],
    "fr_present_enqueue": [C.c_void_p, C.c_int, C.POINTER(C.c_uint64)],
    "fr_present_acquire": [C.c_void_p, C.c_uint64, C.c_int, C.POINTER(C.c_void_p)],
    "fr_present_release": [C.c_void_p, C.c_uint64],
    "fr_present_times": [C.c_void_p, C.c_uint64, C.POINTER(C.c_float), C.POINTER(C.c_float)],
    "fr_present_enqueue_device": [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t],
    "fr_present_done": [C.c_void_p, C.c_void_p],
    "fr_present_warp_pack": [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(fr_present_warp), C.c_void_p],
    "fr_present_warp_from_poses": [C.POINTER(fr_camera_pose), C.POINTER(fr_camera_pose), C.c_int, C.c_int, C.c_int,
                                   C.c_int, C.c_float, C.POINTER(fr_present_warp)],
    "fr_present_enqueue_warped": [C.c_void_p, C.c_int, C.POINTER(fr_present_warp), C.POINTER(C.c_uint64)],
    "fr_present_enqueue_warped_device": [C.c_void_p, C.c_int, C.POINTER(fr_present_warp), C.c_void_p, C.c_size_t],
    "fr_present_blend_default": [C.c_void_p, C.POINTER(fr_present_blend)],
    "fr_present_blend_pack": [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(fr_present_blend),
                              C.POINTER(fr_present_warp), C.c_void_p],
    "fr_present_enqueue_blended": [C.c_void_p, C.POINTER(fr_present_blend), C.POINTER(fr_present_warp),
                                   C.POINTER(C.c_uint64)],
    "fr_present_reproject_from_poses": [C.POINTER(fr_camera_pose), C.POINTER(fr_camera_pose), C.c_int, C.c_int, C.c_int,
                                        C.c_int, C.c_float, C.POINTER(fr_present_reproject)],
    "fr_present_reproject_pack": [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(fr_present_reproject),
                                  C.c_void_p],
    "fr_present_reproject_enable": [C.c_void_p, C.c_int],
    "fr_present_enqueue_reprojected": [C.c_void_p, C.c_int, C.POINTER(fr_present_reproject), C.POINTER(C.c_uint64)],
    "fr_present_enqueue_reprojected_device": [C.c_void_p, C.c_int, C.POINTER(fr_present_reproject), C.c_void_p,
                                              C.c_size_t],
    "fr_present_enqueue_blended_device": [C.c_void_p, C.POINTER(fr_present_blend), C.POINTER(fr_present_warp),
                                          C.c_void_p, C.c_size_t],
    "fr_set_normals": [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int],
    "fr_recompute_normals": [C.c_void_p, C.POINTER(C.c_float)],
    "fr_normal_groups": [C.c_void_p, C.POINTER(C.c_int32), C.c_size_t, C.POINTER(C.c_int)],
    "fr_set_motion_reprojection": [C.c_void_p, C.c_int],
    "fr_scene_normal_groups": [C.c_void_p, C.POINTER(C.c_int32), C.c_size_t, C.POINTER(C.c_int)],
    "fr_get_stats": [C.c_void_p, C.POINTER(fr_stats)],
    "fr_reset_stats": [C.c_void_p],
    "fr_jfa_reuse_count": [C.c_void_p, C.POINTER(C.c_uint32)],
    "fr_kernel_timing": [C.c_void_p, C.c_int],
    "fr_kernel_times": [C.c_void_p, C.POINTER(fr_stage_times)],
    "fr_frame_clock": [C.c_void_p, C.c_int],
    "fr_frame_clock_read": [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_int),
                            C.POINTER(C.c_int)],
    "fr_scene_export": [C.c_void_p, C.POINTER(fr_scene_arrays)],
    "fr_scene_create": [C.POINTER(fr_config), C.POINTER(C.c_void_p)],
    "fr_scene_get_arrays": [C.c_void_p, C.POINTER(fr_scene_arrays)],
    "fr_scene_destroy": [C.c_void_p],
    "fr_group_config_default": [C.POINTER(fr_group_config)],
    "fr_rccl_unique_id": [C.c_void_p],
    "fr_rccl_comm_init": [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)],
    "fr_rccl_comm_destroy": [C.c_void_p],
    "fr_group_create": [C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.POINTER(fr_group_config), C.POINTER(C.c_void_p)],
    "fr_group_frame": [C.c_void_p, C.POINTER(fr_frame_timing)],
    "fr_group_composite": [C.c_void_p, C.c_void_p, C.c_size_t],
    "fr_group_rank_info": [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                           C.POINTER(C.c_int)],
    "fr_group_tile_owners": [C.c_void_p, C.c_void_p, C.c_size_t],
    "fr_group_output_ranks": [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)],
    "fr_group_plan": [C.c_int, C.c_int, C.c_int, C.POINTER(fr_group_config), C.c_void_p, C.c_size_t],
    "fr_group_synchronize": [C.c_void_p],
    "fr_group_destroy": [C.c_void_p],
    "fr_group_last_error": [],
}

_lib = None


def load_library(path: str | None = None):
    """Loads libfovrt.so (raises FovrtError if it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    path = path or os.environ.get("FOVRT_LIB") or LIB_PATH  # FOVRT_LIB: a diagnostic build of the same ABI
    if not os.path.exists(path):
        raise FovrtError(FR_E_STATE, f"{path} not built: run __graft_entry__.build() or make -C "
                                     f"foveated-rendering-using-ray-tracing_amd")
    lib = C.CDLL(path)
    older = path != LIB_PATH and os.environ.get("FOVRT_LIB_OLDER") == "1"  # A/B against an older build
    for name, args in _SIGS.items():
        if older and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = C.c_char_p if name in ("fr_version", "fr_last_error", "fr_group_last_error") else C.c_int
    if lib.fr_abi_version() != ABI_VERSION:
        raise FovrtError(FR_E_STATE, f"{path}: ABI version {lib.fr_abi_version()}, this mirror expects {ABI_VERSION}")
    _lib = lib
    return lib


def _f(arr, n):
    return (C.c_float * n)(*[float(v) for v in arr])


# ------------------------------------------------------------------------------------------
# Camera (FR/Camera.cpp): pose state on the host, matrices from the C ABI's glm restatement.
# ------------------------------------------------------------------------------------------
class Camera:
    PM_Perspective = 0

    def __init__(self):
        self.pos = np.zeros(3, np.float32)
        self.rot = np.array([1, 0, 0, 0], np.float32)  # glm::quat (w, x, y, z); FR/Camera.cpp:12 is (0,0,0,1) xyzw
        self.fovy, self.znear, self.zfar = 45.0, 0.01, 100.0
        self.aspect = 1.0
        self.screen = (1, 1)
        self.target = np.zeros(3, np.float32)
        self.prev = None  # previous pose (setPrevState); None -> same as current

    def setPosition(self, p):
        self.pos = np.asarray(p, np.float32).copy()

    def setRotation(self, q):
        self.rot = np.asarray(q, np.float32).copy()

    def setTarget(self, t):
        self.target = np.asarray(t, np.float32).copy()

    def setProjectMode(self, mode, fovy, n, f):
        self.fovy, self.znear, self.zfar = float(fovy), float(n), float(f)

    def setScreen(self, screen):
        self.screen = (int(screen[0]), int(screen[1]))

    def setViewport(self, vp):
        self.aspect = np.float32(vp[2]) / np.float32(vp[3])

    def lookAt(self, target, up=(0.0, 1.0, 0.0)):
        lib = load_library()
        pose = self._pose()
        lib.fr_camera_look_at(C.byref(pose), _f(target, 3), _f(up, 3))
        self.rot = np.array(pose.rot[:], np.float32)
        self.target = np.asarray(target, np.float32).copy()

    def _pose(self, which=None):
        p = fr_camera_pose()
        src = which or (self.pos, self.rot, self.fovy, self.znear, self.zfar, self.aspect)
        p.pos[:] = [float(v) for v in src[0]]
        p.rot[:] = [float(v) for v in src[1]]
        p.fovy_deg, p.znear, p.zfar, p.aspect = float(src[2]), float(src[3]), float(src[4]), float(src[5])
        return p

    def getVMat(self):
        return self._matrices()[0]

    def getPMat(self):
        return self._matrices()[1]

    def _matrices(self):
        lib = load_library()
        v, p = (C.c_float * 16)(), (C.c_float * 16)()
        lib.fr_camera_matrices(C.byref(self._pose()), v, p)
        return np.array(v[:], np.float32).reshape(4, 4), np.array(p[:], np.float32).reshape(4, 4)

    def setPrevState(self):
        self.prev = (self.pos.copy(), self.rot.copy(), self.fovy, self.znear, self.zfar, self.aspect)

    def uniforms(self, width, height) -> fr_camera:
        lib = load_library()
        cam = fr_camera()
        cur = self._pose()
        prev = self._pose(self.prev) if self.prev is not None else cur
        rc = lib.fr_camera_uniforms(C.byref(cur), C.byref(prev), int(width), int(height), C.byref(cam))
        if rc:
            raise FovrtError(rc, "fr_camera_uniforms")
        return cam

    @staticmethod
    def preset(scene, width, height):
        """The reference's camera set-up (FR/main.cpp:179-209) for a scene preset."""
        lib = load_library()
        eye, tgt = (C.c_float * 3)(), (C.c_float * 3)()
        lib.fr_preset_camera(int(scene), eye, tgt)
        cam = Camera()
        cam.setRotation((1, 0, 0, 0))
        cam.setPosition(eye[:])
        cam.lookAt(tgt[:])
        cam.setProjectMode(Camera.PM_Perspective, 45, 0.1, 500.1)
        cam.setScreen((width, height))
        cam.setViewport((0, 0, width, height))
        return cam


@dataclass
class Config:
    width: int = 1024
    height: int = 1024
    scene: int = SCENE_BUNNY
    mask_mode: int = MASK_SALIENCY
    spp: int = 1
    diffuse_max_depth: int = 1
    refraction_max_depth: int = 16
    light_power: float = 810.0
    optimize: int = 1
    atrous_iterations: int = 1
    write_extra: int = 1
    device: int = 0
    texture_mode: int = 0
    detail: int = 0
    mesh_mode: int = 0  # 0: .obj meshes where present, else procedural; 1: procedural; 2: .obj required
    bvh_builder: int = 0  # 0: host binned SAH; 1: GPU LBVH (k_bvh.hip); 2: GPU binned SAH, the host's tree (k_bvh_sah.hip)
    sibson_mode: int = 0  # 0: run form (prefix sums, ~1e-6 of the per-tap sum); 1: per tap, bit-exact
    asset_dir: str = DEFAULT_ASSET_DIR

    def to_c(self) -> fr_config:
        c = fr_config()
        for f in fr_config._fields_:
            name = f[0]
            if name == "asset_dir":
                c.asset_dir = self.asset_dir.encode()
            elif name == "abi_version":
                c.abi_version = ABI_VERSION
            else:
                setattr(c, name, getattr(self, name))
        return c


# ------------------------------------------------------------------------------------------
# PathTracer (FR/PathTracer.h:73-94)
# ------------------------------------------------------------------------------------------
class PathTracer:
    def __init__(self, config: Config | None = None):
        self.config = config or Config()
        self._ctx = None
        self._ticket_shapes = {}  # (rows, columns) of the present tickets whose image is not the screen's

    # bool initialize(int w, int h)
    def initialize(self, width=None, height=None):
        if self._ctx is not None:
            return False  # FR/PathTracer.cpp:43-45
        lib = load_library()
        if width is not None:
            self.config.width, self.config.height = int(width), int(height)
        self._cfg = self.config.to_c()  # keep asset_dir bytes alive
        ctx = C.c_void_p()
        rc = lib.fr_create(C.byref(self._cfg), C.byref(ctx))
        if rc:
            raise FovrtError(rc, lib.fr_last_error(None).decode())
        self._ctx = ctx
        return True

    def __del__(self):
        self.destroy()

    def destroy(self):
        # a group over this context goes first (fr_group_destroy reads its contexts; under garbage
        # collection of a cycle the tracers' finalisers can run before the group's)
        # (a copy: Group.destroy removes the group from this list, and a tracer may be a rank of several groups)
        for grp in list(getattr(self, "_groups", ())):
            grp.destroy()  # (strong references: weak ones are cleared before a cycle's finalisers run)
        self._groups = []
        if getattr(self, "_ctx", None) is not None and _lib is not None:
            _lib.fr_destroy(self._ctx)
            self._ctx = None

    def _check(self, rc):
        if rc:
            raise FovrtError(rc, _lib.fr_last_error(self._ctx).decode())

    def last_error(self) -> str:
        """fr_last_error: the message of this context's last failure (or of the last rejected enqueued update)."""
        return _lib.fr_last_error(self._ctx).decode()

    @property
    def width(self):
        return self.config.width

    @property
    def height(self):
        return self.config.height

    def init_camera(self, camera: Camera):
        self.update_optix_variables(camera)

    def update_optix_variables(self, camera: Camera):
        cam = camera.uniforms(self.width, self.height)
        self._check(_lib.fr_set_camera(self._ctx, C.byref(cam)))

    def set_camera_uniforms(self, cam: fr_camera):
        self._check(_lib.fr_set_camera(self._ctx, C.byref(cam)))

    def _launch(self, fn):
        ms = C.c_float()
        self._check(fn(self._ctx, C.byref(ms)))
        return ms.value

    def geometry_launch(self):
        return self._launch(_lib.fr_geometry_launch)

    def sampling_launch(self):
        return self._launch(_lib.fr_sampling_launch)

    def optimize_launch(self):
        return self._launch(_lib.fr_optimize_launch)

    def shading_launch(self):
        return self._launch(_lib.fr_shading_launch)

    @property
    def m_accumFrame(self):
        v = C.c_uint32()
        self._check(_lib.fr_accum_frame(self._ctx, C.byref(v)))
        return v.value

    def reset_accumulation(self):
        self._check(_lib.fr_reset_accumulation(self._ctx))

    def set_light_power(self, p):
        self._check(_lib.fr_set_light_power(self._ctx, float(p)))

    def set_diffuse_max_depth(self, d):
        self._check(_lib.fr_set_diffuse_max_depth(self._ctx, int(d)))

    def ray_count(self):
        v = C.c_uint32()
        self._check(_lib.fr_ray_count(self._ctx, C.byref(v)))
        return v.value

    def gaze_target(self):
        v = (C.c_float * 3)()
        self._check(_lib.fr_gaze_target(self._ctx, v))
        return np.array(v[:], np.float32)

    def get_texture(self, name):
        return int(name)

    def view(self, buf) -> fr_buffer_view:
        v = fr_buffer_view()
        self._check(_lib.fr_get_buffer(self._ctx, int(buf), C.byref(v)))
        return v

    def read(self, buf) -> np.ndarray:
        v = self.view(buf)
        if v.format == 0:
            out = np.empty((v.height, v.width, 4), np.float32)
        elif v.format == 1:
            out = np.empty((v.width,), np.uint32)
        else:
            out = np.empty((v.height, v.width), np.uint8)
        self._check(_lib.fr_read_buffer(self._ctx, int(buf), out.ctypes.data, out.nbytes))
        return out

    def write(self, buf, arr: np.ndarray):
        arr = np.ascontiguousarray(arr)
        self._check(_lib.fr_write_buffer(self._ctx, int(buf), arr.ctypes.data, arr.nbytes))

    def stats(self) -> dict:
        s = fr_stats()
        self._check(_lib.fr_get_stats(self._ctx, C.byref(s)))
        return {n: (list(getattr(s, n)) if n == "diag" else getattr(s, n)) for n, _ in fr_stats._fields_}

    def reset_stats(self):
        self._check(_lib.fr_reset_stats(self._ctx))

    def jfa_reuse_count(self) -> int:
        """fr_jfa_reuse_count: JumpFlooding launches whose passes were skipped (the seed set had not changed)."""
        v = C.c_uint32()
        self._check(_lib.fr_jfa_reuse_count(self._ctx, C.byref(v)))
        return v.value

    def kernel_timing(self, enable: bool):
        """Starts (or stops) the live HIP-event timing of entry 3 inside pipelined frames."""
        self._check(_lib.fr_kernel_timing(self._ctx, 1 if enable else 0))

    def kernel_times(self) -> dict:
        """{frames, shading_ms, shade_paths_ms}: stages timed since kernel_timing(True), summed ms."""
        t = fr_stage_times()
        self._check(_lib.fr_kernel_times(self._ctx, C.byref(t)))
        return {"frames": t.frames, "shading_ms": t.shading_ms, "shade_paths_ms": t.shade_paths_ms}

    def frame_clock(self, enable: bool):
        """fr_frame_clock: starts (or stops and clears) the per-frame latency / interval events of fr_frame."""
        self._check(_lib.fr_frame_clock(self._ctx, 1 if enable else 0))

    def frame_clock_read(self, cap=100000):
        """(latency_ms, interval_ms) numpy arrays of every frame since frame_clock(True)."""
        lat = (C.c_float * cap)()
        itv = (C.c_float * cap)()
        nl, ni = C.c_int(0), C.c_int(0)
        self._check(_lib.fr_frame_clock_read(self._ctx, lat, itv, cap, C.byref(nl), C.byref(ni)))
        return (np.frombuffer(lat, np.float32, nl.value).copy(), np.frombuffer(itv, np.float32, ni.value).copy())

    def _frame(self, fn, timing):
        t = fr_frame_timing() if timing else None
        self._check(fn(self._ctx, C.byref(t) if timing else None))
        if not timing:
            return None
        return {n: getattr(t, n) for n, _ in fr_frame_timing._fields_}

    def frame(self, timing=True):
        """One iteration of the FR/main.cpp:253-358 loop body on the device."""
        return self._frame(_lib.fr_frame, timing)

    def set_pipeline_mode(self, mode):
        """fr_set_pipeline_mode: PIPELINE_THROUGHPUT (0, frames enqueued back to back) or PIPELINE_LATENCY (1,
        one trace half in flight: fr_frame waits for the previous frame's path trace before it starts)."""
        self._check(_lib.fr_set_pipeline_mode(self._ctx, int(mode)))

    def set_sample_sum(self, mode):
        """fr_set_sample_sum: 0 fp32, 1 by frame size (default), 2 fixed point with the tail handoff."""
        self._check(_lib.fr_set_sample_sum(self._ctx, int(mode)))

    def shard_unpack_active_enqueue(self, device_ptr, capacity, count):
        """fr_shard_unpack_active without synchronisation (enqueued on the context stream)."""
        self._check(_lib.fr_shard_unpack_active_enqueue(self._ctx, C.c_void_p(device_ptr), int(capacity) * 20,
                                                        int(capacity), int(count)))

    def set_front_local(self, on=True):
        """fr_set_front_local: front stages on this rank's tiles plus halo only (a still camera's tracer)."""
        self._check(_lib.fr_set_front_local(self._ctx, int(bool(on))))

    def set_recon_chains(self, chains):
        """Reconstruction chains this context runs: bit 0 JFA -> Sibson, bit 1 pull-push -> A-Trous."""
        self._check(_lib.fr_set_recon_chains(self._ctx, int(chains)))

    def trace_frame(self, timing=True):
        """The trace half of a frame (update -> entries 0..3)."""
        return self._frame(_lib.fr_trace_frame, timing)

    def reconstruct_frame(self, timing=True):
        """The reconstruction half of a frame (JFA -> Sibson -> pull-push -> A-Trous)."""
        return self._frame(_lib.fr_reconstruct_frame, timing)

    def snapshot(self) -> bytes:
        """fr_snapshot: the temporal state (history / depth pairs, pull-push atlases, frame counter, camera)."""
        n = C.c_size_t()
        self._check(_lib.fr_snapshot_bytes(self._ctx, C.byref(n)))
        buf = (C.c_uint8 * n.value)()
        self._check(_lib.fr_snapshot(self._ctx, buf, n.value))
        return bytes(buf)

    def restore(self, snap: bytes):
        """fr_restore: load a snapshot of a context with the same size, spp and scene."""
        buf = (C.c_uint8 * len(snap)).from_buffer_copy(snap)
        self._check(_lib.fr_restore(self._ctx, buf, len(snap)))

    def copy_buffer(self, buffer_id, device_ptr, nbytes):
        """Device-to-device copy of a buffer into memory the caller owns (e.g. a torch tensor)."""
        self._check(_lib.fr_copy_buffer(self._ctx, int(buffer_id), C.c_void_p(device_ptr), int(nbytes)))

    def composite_views(self, views_ptr, nviews, out_ptr, out_bytes):
        """Side-by-side composite of nviews W x H device images into (nviews W) x H (device pointers)."""
        self._check(_lib.fr_composite_views(self._ctx, C.c_void_p(views_ptr), int(nviews), C.c_void_p(out_ptr),
                                            int(out_bytes)))

    def rebuild_bvh(self) -> float:
        """Re-indexes the current triangles with the GPU builder; returns its wall time in ms."""
        return self._launch(_lib.fr_rebuild_bvh)

    def refit_bvh(self) -> float:
        """Keeps the tree's topology and recomputes its boxes and leaf triangles from the current positions;
        returns its wall time in ms."""
        return self._launch(_lib.fr_refit_bvh)

    @staticmethod
    def _update_kind(update) -> int:
        """"rebuild" / "refit" (or an fr_update_positions `how` value, passed through)."""
        if isinstance(update, str):
            try:
                return {"rebuild": FR_BVH_REBUILD, "refit": FR_BVH_REFIT}[update]
            except KeyError:
                raise ValueError(f"update must be 'rebuild' or 'refit', not {update!r}") from None
        return int(update)

    @staticmethod
    def _normals_kind(normals) -> int:
        """"keep" / "recompute" (or an fr_update_geometry `normals` value, passed through)."""
        if isinstance(normals, str):
            try:
                return {"keep": FR_NORMALS_KEEP, "recompute": FR_NORMALS_RECOMPUTE}[normals]
            except KeyError:
                raise ValueError(f"normals must be 'keep', 'recompute' or the normals, not {normals!r}") from None
        return int(normals)

    def set_positions(self, xyz: np.ndarray, update="rebuild", normals="keep"):
        """New world-space vertex positions (ntris x 3 x 3 float32, scene triangle order), then a GPU
        rebuild of the BVH (update="rebuild") or a refit of the tree in use (update="refit"). The shading
        normals stay (normals="keep"), are recomputed from the new positions over the scene's smooth vertices
        (normals="recompute", fr_update_geometry's rule) or are taken from an array shaped like xyz."""
        a = np.ascontiguousarray(xyz, dtype=np.float32)
        n = a.size // 9
        if isinstance(normals, str) and normals == "keep":
            if update == "rebuild":
                self._check(_lib.fr_set_positions(self._ctx, a.ctypes.data_as(C.POINTER(C.c_float)), n))
            else:
                self._check(_lib.fr_update_positions(self._ctx, C.c_void_p(a.ctypes.data), n, FR_MEM_HOST,
                                                     self._update_kind(update)))
        elif isinstance(normals, (str, int)):
            self._check(_lib.fr_update_geometry(self._ctx, C.c_void_p(a.ctypes.data), None, n, FR_MEM_HOST,
                                                self._update_kind(update), self._normals_kind(normals)))
        else:
            nr = np.ascontiguousarray(normals, dtype=np.float32)
            if nr.size != a.size:
                raise ValueError(f"normals hold {nr.size} floats, positions {a.size}")
            self._check(_lib.fr_update_geometry(self._ctx, C.c_void_p(a.ctypes.data), C.c_void_p(nr.ctypes.data), n,
                                                FR_MEM_HOST, self._update_kind(update), FR_NORMALS_GIVEN))

    def set_positions_device(self, device_ptr, ntris, update="rebuild", normals="keep"):
        """As set_positions from device memory (e.g. tensor.data_ptr() of ntris x 9 float32 on this
        context's device): checked on the device, never copied to the host unless scene_arrays() asks.
        normals: "keep", "recompute", or a device pointer to ntris x 9 float32 normals."""
        if isinstance(normals, str):
            kind, nrm = self._normals_kind(normals), None
        else:
            kind, nrm = FR_NORMALS_GIVEN, C.c_void_p(int(normals))
        if kind == FR_NORMALS_KEEP:
            self._check(_lib.fr_update_positions(self._ctx, C.c_void_p(device_ptr), int(ntris), FR_MEM_DEVICE,
                                                 self._update_kind(update)))
        else:
            self._check(_lib.fr_update_geometry(self._ctx, C.c_void_p(device_ptr), nrm, int(ntris), FR_MEM_DEVICE,
                                                self._update_kind(update), kind))

    @staticmethod
    def _device_ptr(x):
        """A device pointer (int), or an object with data_ptr() (a torch tensor); None stays None."""
        if x is None:
            return None
        return C.c_void_p(int(x.data_ptr() if hasattr(x, "data_ptr") else x))

    def update_geometry_enqueue(self, xyz, ntris=None, normals="keep", ready_event=None):
        """fr_update_geometry_enqueue: set_positions_device(update="refit") in stream order, without waiting for
        the GPU. xyz: a device pointer or an object with data_ptr() (ntris x 9 float32 on this context's device;
        ntris defaults to its numel() // 9). normals: "keep", "recompute", or the normals as xyz (a pointer or a
        tensor). ready_event: a torch event (its cuda_event) or a raw hipEvent_t recorded after the arrays were
        produced. A bad array is rejected on the device: geometry_update_status(). Keep the arrays untouched until
        geometry_consumed() has ordered your stream behind the update's reads."""
        if ntris is None:
            ntris = xyz.numel() // 9
        if isinstance(normals, (str, int)):
            kind, nrm = self._normals_kind(normals), None
        else:
            kind, nrm = FR_NORMALS_GIVEN, self._device_ptr(normals)
        ev = getattr(ready_event, "cuda_event", ready_event)
        self._check(_lib.fr_update_geometry_enqueue(self._ctx, self._device_ptr(xyz), nrm, int(ntris), kind,
                                                    C.c_void_p(int(ev)) if ev else None))

    def geometry_consumed(self, stream=None):
        """fr_geometry_consumed: `stream` (a torch stream, a raw hipStream_t, or None for the null stream) waits on
        the device for the last enqueued update's reads of the caller's arrays. Does not block the host."""
        s = getattr(stream, "cuda_stream", stream)
        self._check(_lib.fr_geometry_consumed(self._ctx, C.c_void_p(int(s)) if s else None))

    @staticmethod
    def _ray_kind(kind):
        if kind not in RAY_KINDS and kind not in RAY_KINDS.values():
            raise ValueError(f"kind must be one of {sorted(RAY_KINDS)}")
        return RAY_KINDS.get(kind, kind)

    def ray_query_reserve(self, n):
        """fr_ray_query_reserve: the staging area host batches of trace_rays go through, for n rays and results
        (48 B per ray on the device; grows only). Waits for the context's pending work."""
        self._check(_lib.fr_ray_query_reserve(self._ctx, int(n)))

    def ray_query_reserve_kind(self, n, kind="closest", masked=False):
        """fr_ray_query_reserve_kind: the same staging area sized for n rays of one kind: 32 B per ray, the kind's
        result (16, 4 or 80 B) and 4 B when masked (grows only). Waits for the context's pending work."""
        self._check(_lib.fr_ray_query_reserve_kind(self._ctx, int(n), self._ray_kind(kind), int(bool(masked))))

    def trace_rays(self, rays, kind="closest", out=None, n=None, masks=None):
        """fr_trace_rays: a batch of rays against the scene as it is now, waiting for the answers.
        rays: a numpy array of n x 8 float32, rows (origin, tmin, dir, tmax), or RAY_DTYPE records; the answers come
        back as numpy: RAY_HIT_DTYPE records (t, beta, gamma, prim; a miss is (inf, 0, 0, -1)) for "closest", n
        float32 for "transmittance", RAY_SURFACE_DTYPE records (the hit, then point, model, ng, u, ns, v, kd and the
        material word; include/fovrt.h) for "surface". The staging area is reserved on demand. Or rays: a device
        pointer or an object with data_ptr() (n x 8 float32 on this context's device; n defaults to its
        numel() // 8), with `out` the same kind of array for the answers (n x 16 B, n floats, or n x 80 B); returns
        `out`. masks (fr_trace_rays_masked): one uint32 per ray, bit k set: model k of models() takes part in that
        ray; memory of the same kind as rays."""
        k = self._ray_kind(kind)
        plain = masks is None and k != FR_RAYS_SURFACE
        if isinstance(rays, np.ndarray):
            a = np.ascontiguousarray(rays.view(np.float32) if rays.dtype == RAY_DTYPE else rays, dtype=np.float32)
            a = a.reshape(-1, 8)
            cnt = a.shape[0]
            res = np.empty(cnt, _RAY_RESULT[k])
            if plain:
                self.ray_query_reserve(cnt)  # (allocates only when the request grows)
                self._check(_lib.fr_trace_rays(self._ctx, C.c_void_p(a.ctypes.data), cnt, FR_MEM_HOST, k,
                                               C.c_void_p(res.ctypes.data)))
                return res
            m = None
            if masks is not None:
                m = np.ascontiguousarray(masks, dtype=np.uint32).reshape(-1)
                if m.shape[0] != cnt:
                    raise ValueError("masks needs one uint32 per ray")
            self.ray_query_reserve_kind(cnt, k, m is not None)
            self._check(_lib.fr_trace_rays_masked(self._ctx, C.c_void_p(a.ctypes.data),
                                                  C.c_void_p(m.ctypes.data) if m is not None else None, cnt,
                                                  FR_MEM_HOST, k, C.c_void_p(res.ctypes.data)))
            return res
        if out is None:
            raise ValueError("device rays need out, a device array for the answers")
        if n is None:
            n = rays.numel() // 8
        if plain:
            self._check(_lib.fr_trace_rays(self._ctx, self._device_ptr(rays), int(n), FR_MEM_DEVICE, k,
                                           self._device_ptr(out)))
        else:
            self._check(_lib.fr_trace_rays_masked(self._ctx, self._device_ptr(rays),
                                                  self._device_ptr(masks) if masks is not None else None, int(n),
                                                  FR_MEM_DEVICE, k, self._device_ptr(out)))
        return out

    def trace_rays_enqueue(self, rays, out, n=None, kind="closest", ready_event=None, masks=None):
        """fr_trace_rays_enqueue: trace_rays over device arrays in stream order, without waiting for the GPU. The
        query sees the scene as of this call's place among the enqueued updates, poses and rebuilds. rays, out, masks:
        device pointers or objects with data_ptr(); ready_event as in update_geometry_enqueue. Keep the arrays
        untouched until rays_consumed() has ordered your stream behind the query. kind "surface" and masks go through
        fr_trace_rays_masked_enqueue."""
        if n is None:
            n = rays.numel() // 8
        ev = getattr(ready_event, "cuda_event", ready_event)
        k = self._ray_kind(kind)
        if masks is None and k != FR_RAYS_SURFACE:
            self._check(_lib.fr_trace_rays_enqueue(self._ctx, self._device_ptr(rays), int(n), k,
                                                   self._device_ptr(out), C.c_void_p(int(ev)) if ev else None))
        else:
            self._check(_lib.fr_trace_rays_masked_enqueue(self._ctx, self._device_ptr(rays),
                                                          self._device_ptr(masks) if masks is not None else None,
                                                          int(n), k, self._device_ptr(out),
                                                          C.c_void_p(int(ev)) if ev else None))

    def rays_consumed(self, stream=None):
        """fr_rays_consumed: `stream` (a torch stream, a raw hipStream_t, or None for the null stream) waits on the
        device for the last enqueued query: work submitted to it afterwards may read the answers and overwrite the
        rays. Does not block the host."""
        s = getattr(stream, "cuda_stream", stream)
        self._check(_lib.fr_rays_consumed(self._ctx, C.c_void_p(int(s)) if s else None))

    def model_of(self, prims):
        """The model index (the order of models()) of each triangle index; -1 for a miss (a negative index)."""
        p = np.asarray(prims["prim"] if getattr(prims, "dtype", None) == RAY_HIT_DTYPE else prims).astype(np.int64)
        first = np.array([m[1] for m in self.models()], np.int64)
        return np.where(p < 0, -1, np.searchsorted(first, p, side="right") - 1).astype(np.int32)

    def set_geometry_overlap(self, on=True):
        """fr_set_geometry_overlap: enqueued updates and enqueued poses refit into a second tree and write second
        normals on the front stages' stream, beside the previous frame's path trace (off by default; the first on
        allocates 64 B per triangle). Waits for the context's pending work."""
        self._check(_lib.fr_set_geometry_overlap(self._ctx, int(bool(on))))

    def geometry_update_status(self):
        """(applied, rejected): enqueued updates by their verdict on the device since the context was created.
        Waits for the context's pending work; after a new rejection last_error() names the array."""
        a, r = C.c_uint64(), C.c_uint64()
        self._check(_lib.fr_geometry_update_status(self._ctx, C.byref(a), C.byref(r)))
        return a.value, r.value

    def rebuild_bvh_enqueue(self):
        """fr_rebuild_bvh_enqueue: rebuild_bvh() in stream order, without waiting for the GPU, with the context's
        builder over the current positions; compose it with update_geometry_enqueue or an enqueued pose. A build
        that fails on the device keeps the tree in use: bvh_rebuild_status()."""
        self._check(_lib.fr_rebuild_bvh_enqueue(self._ctx))

    def bvh_rebuild_status(self):
        """(built, failed): enqueued rebuilds by their verdict on the device since the context was created.
        Waits for the context's pending work; after a new failure last_error() names the cause."""
        b, f = C.c_uint64(), C.c_uint64()
        self._check(_lib.fr_bvh_rebuild_status(self._ctx, C.byref(b), C.byref(f)))
        return b.value, f.value

    def rebuild_bvh_enqueue_if(self, ratio):
        """fr_rebuild_bvh_enqueue_if: rebuild_bvh_enqueue() when the device finds the SAH cost of the tree in use
        above `ratio` times its baseline (the cost of that tree when it was built, or when the first conditional
        call saw it). Nothing waits; a skipped build leaves tree and frames as they were."""
        self._check(_lib.fr_rebuild_bvh_enqueue_if(self._ctx, float(ratio)))

    def set_rebuild_policy(self, ratio, period):
        """fr_set_rebuild_policy: after every `period`-th update_geometry_enqueue or enqueued pose the context
        makes rebuild_bvh_enqueue_if(ratio) itself. period 0 turns the policy off (the default)."""
        self._check(_lib.fr_set_rebuild_policy(self._ctx, float(ratio), int(period)))

    def bvh_rebuild_policy_status(self):
        """(evaluated, skipped, last_cost, base_cost): the conditional rebuilds since the context was created, how
        many of them the device declined, the SAH cost it evaluated last and the baseline it compares with.
        Waits for the context's pending work."""
        e, s, l, b = C.c_uint64(), C.c_uint64(), C.c_float(), C.c_float()
        self._check(_lib.fr_bvh_rebuild_policy_status(self._ctx, C.byref(e), C.byref(s), C.byref(l), C.byref(b)))
        return e.value, s.value, l.value, b.value

    def models(self):
        """[(name, first_tri, ntris)]: the scene's models, contiguous triangle ranges in scene order."""
        return _models(_lib.fr_model_count, _lib.fr_model_info, self._ctx, self._check)

    def enable_model_pose(self, on=True):
        """fr_model_pose_enable: captures the current device positions and normals as the rest geometry that
        set_model_transforms poses (four device arrays of 36 B per triangle at the first call); calling it again
        captures again. on=False: the pose calls fail (FR_E_STATE) until the next enable."""
        self._check(_lib.fr_model_pose_enable(self._ctx, int(bool(on))))

    def set_model_transforms(self, m, update="refit", enqueue=False):
        """One row-major 3 x 4 matrix per model (float32, shape (nmodels, 3, 4) or (nmodels, 12)), v' = A v + t
        over the rest geometry: positions and normals are posed on the device and taken as by set_positions_device
        with given normals (fr_set_model_transforms), or with enqueue=True in stream order without waiting for the
        GPU, always a refit (fr_set_model_transforms_enqueue; geometry_update_status() counts it)."""
        a = np.ascontiguousarray(m, dtype=np.float32)
        if a.ndim < 2 or a.size != a.shape[0] * 12:
            raise ValueError(f"m has shape {a.shape}, not (nmodels, 3, 4) or (nmodels, 12)")
        p = a.ctypes.data_as(C.POINTER(C.c_float))
        if enqueue:
            if self._update_kind(update) != FR_BVH_REFIT:
                raise ValueError("an enqueued pose always refits")
            self._check(_lib.fr_set_model_transforms_enqueue(self._ctx, p, a.shape[0]))
        else:
            self._check(_lib.fr_set_model_transforms(self._ctx, p, a.shape[0], self._update_kind(update)))

    def model_transforms(self) -> np.ndarray:
        """The pose last submitted, shape (nmodels, 3, 4) (identities after enable_model_pose)."""
        n = C.c_int()
        self._check(_lib.fr_model_count(self._ctx, C.byref(n)))
        m = np.empty((n.value, 3, 4), np.float32)
        self._check(_lib.fr_model_transforms(self._ctx, m.ctypes.data_as(C.POINTER(C.c_float)), n.value))
        return m

    def enable_model_visibility(self, on=True):
        """fr_model_visibility_enable: makes the device array the collapsed positions live in (36 B per triangle, at
        the first call). on=False: set_model_visibility fails (FR_E_STATE) until the next enable; refused while a
        model is hidden."""
        self._check(_lib.fr_model_visibility_enable(self._ctx, int(bool(on))))

    def _visible_mask(self, visible) -> int:
        if isinstance(visible, (int, np.integer)):
            return int(visible) & 0xFFFFFFFF
        if isinstance(visible, str):
            visible = [visible]
        names = [m[0] for m in self.models()]
        mask = 0
        for name in visible:
            if name not in names:
                raise ValueError(f"no model named {name!r} (models: {names})")
            mask |= 1 << names.index(name)
        return mask

    def set_model_visibility(self, visible, update="refit", enqueue=False):
        """The models frames and ray queries see: `visible` is a mask (bit k: model k of models()) or an iterable of
        model names; every other model is hidden, by a refit or a rebuild over the positions with its triangles
        collapsed to points (fr_set_model_visibility), or with enqueue=True in stream order without waiting for the
        GPU, always a refit (fr_set_model_visibility_enqueue). Exported arrays and the scene box do not change."""
        mask = self._visible_mask(visible)
        if enqueue:
            if self._update_kind(update) != FR_BVH_REFIT:
                raise ValueError("an enqueued visibility change always refits")
            self._check(_lib.fr_set_model_visibility_enqueue(self._ctx, mask))
        else:
            self._check(_lib.fr_set_model_visibility(self._ctx, mask, self._update_kind(update)))

    def model_visibility(self) -> int:
        """The mask last submitted, valid bits only (every model before the first call)."""
        v = C.c_uint32()
        self._check(_lib.fr_model_visibility(self._ctx, C.byref(v)))
        return v.value

    # ---- foveation control ----
    def set_mask_mode(self, mode):
        """fr_set_mask_mode: the sampling mask from the next sampling launch on (a MASK_* value, or a name of MASKS or
        STEERED_MASKS). Host state; waits for nothing."""
        self._check(_lib.fr_set_mask_mode(self._ctx, int({**MASKS, **STEERED_MASKS}.get(mode, mode))))

    def mask_mode(self) -> int:
        v = C.c_int()
        self._check(_lib.fr_get_mask_mode(self._ctx, C.byref(v)))
        return v.value

    def foveation(self) -> dict:
        """fr_get_foveation: the eccentricity mask's parameters in place."""
        f = fr_foveation()
        self._check(_lib.fr_get_foveation(self._ctx, C.byref(f)))
        return {"radius_px": f.radius_px, "floor_ranks": f.floor_ranks, "ray_budget": f.ray_budget,
                "tolerance": f.tolerance}

    def set_foveation(self, radius_px=None, floor_ranks=None, ray_budget=None, tolerance=None):
        """fr_set_foveation: the parameters of MASK_ECCENTRIC; an argument left None keeps its value. ray_budget > 0:
        the device steers the radius toward that many traced pixels (foveation_status())."""
        f = fr_foveation()
        self._check(_lib.fr_get_foveation(self._ctx, C.byref(f)))
        if radius_px is not None:
            f.radius_px = float(radius_px)
        if floor_ranks is not None:
            f.floor_ranks = int(floor_ranks)
        if ray_budget is not None:
            f.ray_budget = int(ray_budget)
        if tolerance is not None:
            f.tolerance = float(tolerance)
        self._check(_lib.fr_set_foveation(self._ctx, C.byref(f)))

    def foveation_status(self) -> dict:
        """fr_foveation_status (waits for pending work): the r2 the last mode-5 sampling launch used, the count the
        budget's controller read last, and its adjusted / held launches since set_foveation."""
        r2, n, a, h = C.c_float(), C.c_uint32(), C.c_uint64(), C.c_uint64()
        self._check(_lib.fr_foveation_status(self._ctx, C.byref(r2), C.byref(n), C.byref(a), C.byref(h)))
        return {"r2": r2.value, "last_count": n.value, "adjusted": a.value, "held": h.value}

    def enable_sampling_mask(self, on=True):
        """fr_sampling_mask_enable: makes the context's copy of a caller's mask (W * H bytes, at the first call)."""
        self._check(_lib.fr_sampling_mask_enable(self._ctx, int(bool(on))))

    def set_sampling_mask(self, mask, enqueue=False, ready_event=None):
        """The mask MASK_CALLER samples with: H x W bytes, a pixel sampled when its byte is not 0. A numpy array is
        copied from the host; a device pointer or an object with data_ptr() (16-byte aligned, W * H bytes) is read on
        the device, and with enqueue=True in stream order without waiting for the GPU (ready_event as in
        update_geometry_enqueue; keep the array untouched until sampling_mask_consumed())."""
        nbytes = self.width * self.height
        if isinstance(mask, np.ndarray):
            if enqueue:
                raise ValueError("an enqueued mask lives in device memory")
            a = np.ascontiguousarray(mask, dtype=np.uint8)
            self._check(_lib.fr_set_sampling_mask(self._ctx, C.c_void_p(a.ctypes.data), a.size, FR_MEM_HOST))
        elif enqueue:
            ev = getattr(ready_event, "cuda_event", ready_event)
            self._check(_lib.fr_set_sampling_mask_enqueue(self._ctx, self._device_ptr(mask), nbytes,
                                                          C.c_void_p(int(ev)) if ev else None))
        else:
            self._check(_lib.fr_set_sampling_mask(self._ctx, self._device_ptr(mask), nbytes, FR_MEM_DEVICE))

    def sampling_mask_consumed(self, stream=None):
        """fr_sampling_mask_consumed: `stream` waits on the device for the last enqueued mask's reads."""
        s = getattr(stream, "cuda_stream", stream)
        self._check(_lib.fr_sampling_mask_consumed(self._ctx, C.c_void_p(int(s)) if s else None))

    # Present: 8-bit frames in stream order (fr_present_enable and the calls beside it in include/fovrt.h)
    def present_enable(self, slots, format=FR_PRESENT_RGBA8):
        """fr_present_enable: a ring of `slots` (1..8) pinned host images of H x W x 4 bytes in `format`
        (FR_PRESENT_RGBA8 or FR_PRESENT_BGRA8, FR_PRESENT_TOP_DOWN or-ed in); slots=0 turns presenting off."""
        self._check(_lib.fr_present_enable(self._ctx, int(slots), int(format)))

    def _present_ticket(self, enqueue, *args, shape=None) -> int:
        """enqueue(ctx, *args, &ticket), checked; `shape`: what present_acquire gives the ticket's image (rows, columns)
        when that is not the screen's. Returns the ticket."""
        t = C.c_uint64()
        self._check(enqueue(self._ctx, *args, C.byref(t)))
        if shape is not None:
            self._ticket_shapes[t.value] = shape
        return t.value

    def present(self, buffer) -> int:
        """fr_present_enqueue: the buffer (SHADING, SIBSON, PULLPUSH or ATROUS) as it stands at this place of the
        stream order, on its way to the host without waiting for the GPU; returns the ticket. FovrtError with
        FR_E_STATE when every slot is held."""
        return self._present_ticket(_lib.fr_present_enqueue, int(buffer))

    def present_acquire(self, ticket, wait=True):
        """fr_present_acquire: the frame of `ticket` as an (H, W, 4) uint8 view over the slot's pinned image, valid
        until present_release(ticket); None while the frame is pending (wait=False only)."""
        p = C.c_void_p()
        rc = _lib.fr_present_acquire(self._ctx, int(ticket), int(bool(wait)), C.byref(p))
        if rc == FR_PRESENT_PENDING:
            return None
        self._check(rc)
        h, w = self._ticket_shapes.get(int(ticket), (self.height, self.width))
        buf = (C.c_uint8 * (w * h * 4)).from_address(p.value)
        a = np.frombuffer(buf, np.uint8).reshape(h, w, 4)
        a.flags.writeable = False
        return a

    def present_release(self, ticket):
        """fr_present_release: the slot of `ticket` is free again (acquired or not); its view is no longer valid."""
        self._check(_lib.fr_present_release(self._ctx, int(ticket)))
        self._ticket_shapes.pop(int(ticket), None)

    def present_warped(self, buffer, warp) -> int:
        """fr_present_enqueue_warped: as present(), through the homography `warp` (a PresentWarp): late reprojection,
        crop or scale. present_acquire gives the ticket's image in the warp's output shape."""
        return self._present_ticket(_lib.fr_present_enqueue_warped, int(buffer), C.byref(warp.c_struct()),
                                    shape=warp.shape(self.width, self.height))

    def present_warped_to(self, buffer, warp, tensor):
        """fr_present_enqueue_warped_device: as present_to(), through `warp`; the tensor holds the output's
        height * width * 4 bytes."""
        nbytes = tensor.numel() * tensor.element_size()
        self._check(_lib.fr_present_enqueue_warped_device(self._ctx, int(buffer), C.byref(warp.c_struct()),
                                                          self._device_ptr(tensor), nbytes))

    def present_blend_default(self) -> "PresentBlend":
        """fr_present_blend_default: SIBSON inside, ATROUS outside, around the gaze the next launch uses, from the
        foveation radius to twice that. Host state only."""
        b = fr_present_blend()
        self._check(_lib.fr_present_blend_default(self._ctx, C.byref(b)))
        return PresentBlend.from_c(b)

    def present_blended(self, blend, warp=None) -> int:
        """fr_present_enqueue_blended: as present(), of the virtual image that is blend.inner_buffer around the gaze,
        blend.outer_buffer in the periphery and their smoothstep mix between the radii (a PresentBlend); through
        `warp` (a PresentWarp) when one is given. Returns the ticket."""
        return self._present_ticket(_lib.fr_present_enqueue_blended, C.byref(blend.c_struct()),
                                    None if warp is None else C.byref(warp.c_struct()),
                                    shape=None if warp is None else warp.shape(self.width, self.height))

    def present_blended_to(self, blend, tensor, warp=None):
        """fr_present_enqueue_blended_device: as present_to() / present_warped_to(), of the blended image."""
        nbytes = tensor.numel() * tensor.element_size()
        self._check(_lib.fr_present_enqueue_blended_device(self._ctx, C.byref(blend.c_struct()),
                                                           None if warp is None else C.byref(warp.c_struct()),
                                                           self._device_ptr(tensor), nbytes))

    def present_reproject_enable(self, on=True):
        """fr_present_reproject_enable: the key image of the reprojected present (W * H * 8 bytes, made by the first
        call, which waits for the context's pending work); after present_enable. on=False turns the calls off."""
        self._check(_lib.fr_present_reproject_enable(self._ctx, int(bool(on))))

    def present_reprojected(self, buffer, rp) -> int:
        """fr_present_enqueue_reprojected: as present_warped(), with every texel moved to where the display camera of
        `rp` (a PresentReproject) sees its POSITION; rp.fallback fills where nothing lands. Returns the ticket."""
        return self._present_ticket(_lib.fr_present_enqueue_reprojected, int(buffer), C.byref(rp.c_struct()),
                                    shape=rp.fallback.shape(self.width, self.height))

    def present_reprojected_to(self, buffer, rp, tensor):
        """fr_present_enqueue_reprojected_device: as present_warped_to(), reprojected by `rp`."""
        nbytes = tensor.numel() * tensor.element_size()
        self._check(_lib.fr_present_enqueue_reprojected_device(self._ctx, int(buffer), C.byref(rp.c_struct()),
                                                               self._device_ptr(tensor), nbytes))

    def present_times(self, ticket) -> dict:
        """fr_present_times: the pack kernel's and the host copy's time of an acquired ticket, in ms."""
        a, b = C.c_float(), C.c_float()
        self._check(_lib.fr_present_times(self._ctx, int(ticket), C.byref(a), C.byref(b)))
        return {"pack_ms": a.value, "copy_ms": b.value}

    def present_to(self, buffer, tensor):
        """fr_present_enqueue_device: the same pack straight into device memory, H * W * 4 bytes, 16-byte aligned
        (a torch uint8 tensor or anything with data_ptr() and numel() * element_size()); read it on a stream that
        present_done() has ordered behind the pack."""
        nbytes = tensor.numel() * tensor.element_size()
        self._check(_lib.fr_present_enqueue_device(self._ctx, int(buffer), self._device_ptr(tensor), nbytes))

    def present_done(self, stream=None):
        """fr_present_done: `stream` (a torch stream, a raw hipStream_t, or None for the null stream) waits on the
        device for the last present_to(). Does not block the host."""
        s = getattr(stream, "cuda_stream", stream)
        self._check(_lib.fr_present_done(self._ctx, C.c_void_p(int(s)) if s else None))

    def set_normals(self, nrm: np.ndarray):
        """New shading normals (ntris x 3 x 3 float32, scene triangle order) for the triangles that have
        normals; positions, tree, texture coordinates and flags stay."""
        a = np.ascontiguousarray(nrm, dtype=np.float32)
        self._check(_lib.fr_set_normals(self._ctx, C.c_void_p(a.ctypes.data), a.size // 9, FR_MEM_HOST))

    def set_normals_device(self, device_ptr, ntris):
        """As set_normals from device memory (ntris x 9 float32 on this context's device)."""
        self._check(_lib.fr_set_normals(self._ctx, C.c_void_p(device_ptr), int(ntris), FR_MEM_DEVICE))

    def recompute_normals(self) -> float:
        """Recomputes the shading normals from the current positions (fr_update_geometry's rule); returns
        the wall time in ms."""
        return self._launch(_lib.fr_recompute_normals)

    def normal_groups(self):
        """(corner_vertex, nverts): the smooth vertex of every corner 3 t + k (int32, -1 for triangles without
        normals) and the number of vertices; fixed for the life of the context."""
        a = fr_scene_arrays()
        self._check(_lib.fr_scene_export(self._ctx, C.byref(a)))
        cv, nv = np.empty(3 * a.num_tris, np.int32), C.c_int()
        self._check(_lib.fr_normal_groups(self._ctx, cv.ctypes.data_as(C.POINTER(C.c_int32)), cv.size, C.byref(nv)))
        return cv, nv.value

    def set_motion_reprojection(self, on=True):
        """fr_set_motion_reprojection: the first G-buffer after a position update reprojects each hit point from
        where its triangle was when the previous G-buffer traced it, and that frame's sampling tests the history
        depth against that point (off by default; one more device position array at the first on)."""
        self._check(_lib.fr_set_motion_reprojection(self._ctx, int(bool(on))))

    def bvh_sah_cost(self) -> float:
        """SAH cost of the tree in use (fr_bvh_sah_cost): compare a refitted tree with itself when built."""
        v = C.c_float()
        self._check(_lib.fr_bvh_sah_cost(self._ctx, C.byref(v)))
        return v.value

    def set_gaze(self, xpos, ypos, fullscreen=False):
        """cursorPosCallback (FR/gui.cpp:48-66): the cursor in window coordinates (y down);
        g_gaze = (LONG(xpos), LONG(ypos * adjust_scale)), adjust_scale 1 in full screen, 1.25 in a window."""
        self._check(_lib.fr_set_gaze(self._ctx, float(xpos), float(ypos), 1 if fullscreen else 0))

    def reset_gaze(self):
        """framebufferSizeCallback (FR/gui.cpp:32-35): g_gaze = (W / 2, H / 2)."""
        self._check(_lib.fr_reset_gaze(self._ctx))

    # tile sharding of one view across ranks (include/fovrt.h, fr_set_shard)
    def set_shard(self, rank, count, tile=128, first_tracer=0):
        """fr_set_shard_ex: tiles dealt round robin over ranks first_tracer .. count-1."""
        self._check(_lib.fr_set_shard_ex(self._ctx, int(rank), int(count), int(tile), int(first_tracer)))

    def set_shard_plan(self, rank, count, tile, owner):
        """fr_set_shard_plan: owner[t] (uint8, one per tile in raster order) traces tile t."""
        o = np.ascontiguousarray(owner, dtype=np.uint8)
        self._check(_lib.fr_set_shard_plan(self._ctx, int(rank), int(count), int(tile),
                                           o.ctypes.data_as(C.POINTER(C.c_uint8)), o.size))

    def shard_counts(self, n) -> np.ndarray:
        """Active pixels of every view rank in the last front stages, from this rank's own full mask."""
        out = np.zeros(int(n), np.uint32)
        self._check(_lib.fr_shard_counts(self._ctx, out.ctypes.data_as(C.POINTER(C.c_uint32)), int(n)))
        return out

    def shard_texels(self) -> int:
        n = C.c_size_t()
        self._check(_lib.fr_shard_texels(self._ctx, C.byref(n)))
        return n.value

    def shard_pack(self, buffer_id, device_ptr, nbytes):
        """Packs this rank's tiles of an RGBA32F buffer into the device slab at device_ptr."""
        self._check(_lib.fr_shard_pack(self._ctx, int(buffer_id), C.c_void_p(device_ptr), int(nbytes)))

    def shard_unpack(self, buffer_id, src_rank, device_ptr, nbytes):
        """Writes rank src_rank's tiles from the device slab at device_ptr into the buffer."""
        self._check(_lib.fr_shard_unpack(self._ctx, int(buffer_id), int(src_rank), C.c_void_p(device_ptr),
                                         int(nbytes)))

    def shard_pack_active(self, device_ptr, capacity, slab_bytes=None) -> int:
        """Packs the pixels this rank's last trace half shaded (capacity x 20 B slab); returns their count."""
        n = C.c_uint32()
        nb = int(capacity) * 20 if slab_bytes is None else int(slab_bytes)
        self._check(_lib.fr_shard_pack_active(self._ctx, C.c_void_p(device_ptr), nb, int(capacity), C.byref(n)))
        return n.value

    def shard_unpack_active(self, device_ptr, capacity, count, slab_bytes=None):
        """Adds this rank's reprojected history to another rank's packed pixels (their radiance) and scatters
        the sums into HISTORY_CACHE and SHADING."""
        nb = int(capacity) * 20 if slab_bytes is None else int(slab_bytes)
        self._check(_lib.fr_shard_unpack_active(self._ctx, C.c_void_p(device_ptr), nb, int(capacity), int(count)))

    def synchronize(self):
        self._check(_lib.fr_synchronize(self._ctx))

    def scene_arrays(self) -> dict:
        a = fr_scene_arrays()
        self._check(_lib.fr_scene_export(self._ctx, C.byref(a)))
        return _arrays_to_dict(a)


def _models(count_fn, info_fn, handle, check):
    n = C.c_int()
    check(count_fn(handle, C.byref(n)))
    out = []
    for i in range(n.value):
        name, first, nt = C.c_char_p(), C.c_int(), C.c_int()
        check(info_fn(handle, i, C.byref(name), C.byref(first), C.byref(nt)))
        out.append((name.value.decode(), first.value, nt.value))
    return out


def _arrays_to_dict(a: fr_scene_arrays) -> dict:
        n = a.num_tris
        tex = []
        for i in range(a.num_textures):
            w, h = a.tex_dims[2 * i], a.tex_dims[2 * i + 1]
            tex.append(np.ctypeslib.as_array(a.tex_data[i], shape=(h, w, 4)).copy())
        return {
            "pos": np.ctypeslib.as_array(a.pos, shape=(n, 9)).copy(),
            "nrm": np.ctypeslib.as_array(a.nrm, shape=(n, 9)).copy(),
            "uv": np.ctypeslib.as_array(a.uv, shape=(n, 6)).copy(),
            "flags": np.ctypeslib.as_array(a.flags, shape=(n,)).copy(),
            "materials": np.ctypeslib.as_array(a.materials, shape=(a.num_materials, 2)).copy(),
            "textures": tex,
            "envmap": a.envmap,
            "light": np.array(a.light[:], np.float32),
            "bbox": np.array(a.bbox[:], np.float32),
            "bvh_nodes": a.bvh_nodes,
            "bvh_depth": a.bvh_depth,
            "bvh_max_stack": a.bvh_max_stack,
        }


class Scene:
    """Host-only preset scene (fr_scene_create): no device required."""

    def __init__(self, config: Config):
        lib = load_library()
        self._cfg = config.to_c()
        h = C.c_void_p()
        rc = lib.fr_scene_create(C.byref(self._cfg), C.byref(h))
        if rc:
            raise FovrtError(rc, lib.fr_last_error(None).decode())
        self._h = h

    def arrays(self) -> dict:
        a = fr_scene_arrays()
        rc = _lib.fr_scene_get_arrays(self._h, C.byref(a))
        if rc:
            raise FovrtError(rc, "fr_scene_get_arrays")
        return _arrays_to_dict(a)

    def models(self):
        """[(name, first_tri, ntris)] as PathTracer.models, on the host."""
        def check(rc):
            if rc:
                raise FovrtError(rc, "fr_scene_model_info")
        return _models(_lib.fr_scene_model_count, _lib.fr_scene_model_info, self._h, check)

    def normal_groups(self):
        """(corner_vertex, nverts) as PathTracer.normal_groups, on the host."""
        a = fr_scene_arrays()
        rc = _lib.fr_scene_get_arrays(self._h, C.byref(a))
        if rc:
            raise FovrtError(rc, "fr_scene_get_arrays")
        cv, nv = np.empty(3 * a.num_tris, np.int32), C.c_int()
        rc = _lib.fr_scene_normal_groups(self._h, cv.ctypes.data_as(C.POINTER(C.c_int32)), cv.size, C.byref(nv))
        if rc:
            raise FovrtError(rc, "fr_scene_normal_groups")
        return cv, nv.value

    def __del__(self):
        if getattr(self, "_h", None) is not None and _lib is not None:
            _lib.fr_scene_destroy(self._h)
            self._h = None


class _Pass:
    def __init__(self, tracer: PathTracer):
        self.tracer = tracer

    def resetShader(self):  # GLSL reload (FR/JumpFlooding.cpp:51-58): nothing to reload here
        pass


class JumpFlooding(_Pass):
    """JumpFlooding::render(rt, query, elapsed, done) (FR/JumpFlooding.cpp:60-140)."""
    coordTex = TextureName.JFA_COORD
    colorTex = TextureName.JFA_COLOR

    def render(self, rt=TextureName.SHADING):
        ns = C.c_uint64()
        self.tracer._check(_lib.fr_jfa_render(self.tracer._ctx, int(rt), C.byref(ns)))
        return ns.value


class LogPolarTransform(_Pass):
    """LogPolarTransform::render(pt, query, elapsed, done) (FR/Log_Polar_Transform.cpp:40-106)."""
    logPolarTex = TextureName.LOGPOLAR
    ilogPolarTex = TextureName.LOGPOLAR_INVERSE

    def render(self, pt=TextureName.PULLPUSH):
        ns = C.c_uint64()
        self.tracer._check(_lib.fr_logpolar_render(self.tracer._ctx, int(pt), C.byref(ns)))
        return ns.value


class SibsonInterpolation(_Pass):
    """SibsonInterpolation::render(coord, color, ...) (FR/SibsonInterpolation.cpp:28-53)."""
    outputTex = TextureName.SIBSON

    def render(self, coord=TextureName.JFA_COORD, color=TextureName.JFA_COLOR):
        if coord != TextureName.JFA_COORD or color != TextureName.JFA_COLOR:
            raise FovrtError(FR_E_UNSUPPORTED, "Sibson reads the JumpFlooding outputs")
        ns = C.c_uint64()
        self.tracer._check(_lib.fr_sibson_render(self.tracer._ctx, C.byref(ns)))
        return ns.value


class PullPushInterpolation(_Pass):
    """PullPushInterpolation::render(sparse, ...) (FR/PullPushInterpolation.cpp:48-238)."""
    outputTex = TextureName.PULLPUSH

    def render(self, sparse=TextureName.SHADING):
        ns = C.c_uint64()
        self.tracer._check(_lib.fr_pullpush_render(self.tracer._ctx, int(sparse), C.byref(ns)))
        return ns.value


class ATrous(_Pass):
    """ATrous::render(count, pos, nrm, col, rt, frame, ...) (FR/ATrous.cpp:47-132)."""
    colorTex = TextureName.ATROUS

    def render(self, count=1, positionTex=TextureName.POSITION, normalTex=TextureName.NORMAL,
               colorTex=TextureName.PULLPUSH, rtTex=None, frame=0):
        ns = C.c_uint64()
        self.tracer._check(_lib.fr_atrous_render(self.tracer._ctx, int(count), int(positionTex), int(normalTex),
                                                 int(colorTex), C.byref(ns)))
        return ns.value


def version():
    return load_library().fr_version().decode()


def foveation_default(width, height) -> dict:
    """fr_foveation_default (host only): the parameters a context of this size starts from."""
    lib = load_library()
    f = fr_foveation()
    rc = lib.fr_foveation_default(int(width), int(height), C.byref(f))
    if rc:
        raise FovrtError(rc, "fr_foveation_default: bad size")
    return {"radius_px": f.radius_px, "floor_ranks": f.floor_ranks, "ray_budget": f.ray_budget,
            "tolerance": f.tolerance}


def foveation_mask(width, height, gaze, r2, floor_ranks=1, count_only=False):
    """fr_foveation_mask (host only): the MASK_ECCENTRIC mask of a screen as (H x W uint8, count), through the
    function the kernel runs; count_only=True returns the count alone."""
    lib = load_library()
    m = None if count_only else np.zeros((int(height), int(width)), np.uint8)
    n = C.c_uint32()
    g = None if gaze is None else (C.c_float * 2)(float(gaze[0]), float(gaze[1]))
    rc = lib.fr_foveation_mask(int(width), int(height), g, C.c_float(r2), int(floor_ranks),
                               None if m is None else C.c_void_p(m.ctypes.data), C.byref(n))
    if rc:
        raise FovrtError(rc, "fr_foveation_mask: bad argument")
    return n.value if count_only else (m, n.value)


def present_pack(rgba, format=FR_PRESENT_RGBA8) -> np.ndarray:
    """fr_present_pack (host only): an (H, W, 4) float32 image as (H, W, 4) uint8 by the present rule, through the
    function the kernel runs."""
    lib = load_library()
    a = np.ascontiguousarray(rgba, dtype=np.float32)
    if a.ndim != 3 or a.shape[2] != 4:
        raise ValueError("present_pack: an (H, W, 4) float32 image")
    out = np.empty(a.shape, np.uint8)
    rc = lib.fr_present_pack(C.c_void_p(a.ctypes.data), a.shape[1], a.shape[0], int(format), C.c_void_p(out.ctypes.data))
    if rc:
        raise FovrtError(rc, "fr_present_pack: bad size or format")
    return out


class PresentWarp:
    """fr_present_warp: a homography h (9 float32, row-major) from output texel centres to source texel coordinates,
    and the output size (0, 0: the source's). include/fovrt.h, "Present", has the rule."""

    def __init__(self, h, out_width=0, out_height=0):
        self.h = np.asarray(h, np.float32).reshape(9).copy()
        self.out_width, self.out_height = int(out_width), int(out_height)

    def c_struct(self) -> fr_present_warp:
        w = fr_present_warp()
        C.memmove(w.h, self.h.ctypes.data, 36)  # the bits as they are: a float() round trip would change no value
        w.out_width, w.out_height = self.out_width, self.out_height
        return w

    def shape(self, width, height):
        """(rows, columns) of the output over a width x height source."""
        if self.out_width == 0 and self.out_height == 0:
            return int(height), int(width)
        return self.out_height, self.out_width

    @staticmethod
    def identity():
        return PresentWarp([1, 0, 0, 0, 1, 0, 0, 0, 1])

    @staticmethod
    def crop(x0, y0, out_width, out_height):
        """The out_width x out_height texels whose lower left texel is (x0, y0) (rows bottom-up)."""
        return PresentWarp([1, 0, x0, 0, 1, y0, 0, 0, 1], out_width, out_height)

    @staticmethod
    def scale(width, height, out_width, out_height):
        """The whole width x height image as out_width x out_height texels."""
        return PresentWarp([np.float32(width) / np.float32(out_width), 0, 0,
                            0, np.float32(height) / np.float32(out_height), 0, 0, 0, 1], out_width, out_height)

    @staticmethod
    def from_poses(rendered, display, width, height, out_width=None, out_height=None, ndc_depth=1.0):
        return present_warp_from_poses(rendered, display, width, height, out_width, out_height, ndc_depth)


def present_warp_from_poses(rendered, display, width, height, out_width=None, out_height=None, ndc_depth=1.0) -> PresentWarp:
    """fr_present_warp_from_poses (host only): the late reprojection from the camera a frame was rendered for to the
    one it is displayed for (each a Camera or an fr_camera_pose), through the points at `ndc_depth` of the display
    camera; with equal eye positions (a rotation) the depth does not matter."""
    lib = load_library()
    r, d = (p._pose() if isinstance(p, Camera) else p for p in (rendered, display))
    w = fr_present_warp()
    rc = lib.fr_present_warp_from_poses(C.byref(r), C.byref(d), int(width), int(height),
                                        int(width if out_width is None else out_width),
                                        int(height if out_height is None else out_height), C.c_float(ndc_depth), C.byref(w))
    if rc:
        raise FovrtError(rc, "fr_present_warp_from_poses: bad size or depth, a singular matrix, or the output's corner "
                             "is not in front of the rendered camera")
    return PresentWarp(np.array(w.h[:], np.float32), w.out_width, w.out_height)


def present_warp_pack(rgba, warp, format=FR_PRESENT_RGBA8) -> np.ndarray:
    """fr_present_warp_pack (host only): an (H, W, 4) float32 image through `warp` as (oh, ow, 4) uint8 by the warped
    present rule, through the function the kernel runs."""
    lib = load_library()
    a = np.ascontiguousarray(rgba, dtype=np.float32)
    if a.ndim != 3 or a.shape[2] != 4:
        raise ValueError("present_warp_pack: an (H, W, 4) float32 image")
    out = np.empty(warp.shape(a.shape[1], a.shape[0]) + (4,), np.uint8)
    rc = lib.fr_present_warp_pack(C.c_void_p(a.ctypes.data), a.shape[1], a.shape[0], int(format), C.byref(warp.c_struct()),
                                  C.c_void_p(out.ctypes.data))
    if rc:
        raise FovrtError(rc, "fr_present_warp_pack: bad size, format or warp")
    return out


class PresentBlend:
    """fr_present_blend: two presentable buffers, a gaze point (texels, row 0 at the bottom) and the two radii between
    which the image goes from `inner_buffer` to `outer_buffer` by a smoothstep of the squared distance. The gaze and
    the radii are kept as float32. include/fovrt.h, "Present", has the rule."""

    def __init__(self, gaze, inner_radius_px, outer_radius_px, inner_buffer=TextureName.SIBSON,
                 outer_buffer=TextureName.ATROUS):
        self.inner_buffer, self.outer_buffer = int(inner_buffer), int(outer_buffer)
        self.gaze = np.asarray(gaze, np.float32).reshape(2).copy()
        self.inner_radius_px, self.outer_radius_px = np.float32(inner_radius_px), np.float32(outer_radius_px)

    def c_struct(self) -> fr_present_blend:
        b = fr_present_blend()
        b.inner_buffer, b.outer_buffer = self.inner_buffer, self.outer_buffer
        b.gaze[0], b.gaze[1] = float(self.gaze[0]), float(self.gaze[1])
        b.inner_radius_px, b.outer_radius_px = float(self.inner_radius_px), float(self.outer_radius_px)
        return b

    @staticmethod
    def from_c(b) -> "PresentBlend":
        return PresentBlend((b.gaze[0], b.gaze[1]), b.inner_radius_px, b.outer_radius_px, b.inner_buffer, b.outer_buffer)


def present_blend_pack(inner, outer, blend, warp=None, format=FR_PRESENT_RGBA8) -> np.ndarray:
    """fr_present_blend_pack (host only): two (H, W, 4) float32 images blended by `blend` (a PresentBlend; its buffer
    ids are not used) as (H, W, 4) uint8, or through `warp` as (oh, ow, 4), through the functions the kernels run."""
    lib = load_library()
    a, b = (np.ascontiguousarray(x, dtype=np.float32) for x in (inner, outer))
    if a.ndim != 3 or a.shape[2] != 4 or b.shape != a.shape:
        raise ValueError("present_blend_pack: two (H, W, 4) float32 images of one size")
    shape = (a.shape[0], a.shape[1]) if warp is None else warp.shape(a.shape[1], a.shape[0])
    out = np.empty(shape + (4,), np.uint8)
    rc = lib.fr_present_blend_pack(C.c_void_p(a.ctypes.data), C.c_void_p(b.ctypes.data), a.shape[1], a.shape[0], int(format),
                                   C.byref(blend.c_struct()), None if warp is None else C.byref(warp.c_struct()),
                                   C.c_void_p(out.ctypes.data))
    if rc:
        raise FovrtError(rc, "fr_present_blend_pack: bad size, format, blend or warp")
    return out


class PresentReproject:
    """fr_present_reproject: vp (16 float32, row-major: a world point to the display camera's clip space) and the
    fallback homography (a PresentWarp, whose output size is the output's). include/fovrt.h, "Present", has the rule."""

    def __init__(self, vp, fallback=None):
        self.vp = np.asarray(vp, np.float32).reshape(16).copy()
        self.fallback = PresentWarp.identity() if fallback is None else fallback

    def c_struct(self) -> fr_present_reproject:
        r = fr_present_reproject()
        C.memmove(r.vp, self.vp.ctypes.data, 64)  # the bits as they are
        r.fallback = self.fallback.c_struct()
        return r

    @staticmethod
    def from_poses(rendered, display, width, height, out_width=None, out_height=None, ndc_depth=1.0):
        return present_reproject_from_poses(rendered, display, width, height, out_width, out_height, ndc_depth)


def present_reproject_from_poses(rendered, display, width, height, out_width=None, out_height=None,
                                 ndc_depth=1.0) -> PresentReproject:
    """fr_present_reproject_from_poses (host only): `rendered` is the camera the frame was traced with, `display` the
    one it is shown for (each a Camera or an fr_camera_pose): the display camera's proj * view, and the homography of
    present_warp_from_poses for the same arguments as the fallback."""
    lib = load_library()
    r, d = (p._pose() if isinstance(p, Camera) else p for p in (rendered, display))
    rp = fr_present_reproject()
    rc = lib.fr_present_reproject_from_poses(C.byref(r), C.byref(d), int(width), int(height),
                                             int(width if out_width is None else out_width),
                                             int(height if out_height is None else out_height), C.c_float(ndc_depth),
                                             C.byref(rp))
    if rc:
        raise FovrtError(rc, "fr_present_reproject_from_poses: bad size or depth, a singular matrix, or the output's "
                             "corner is not in front of the rendered camera")
    return PresentReproject(np.array(rp.vp[:], np.float32),
                            PresentWarp(np.array(rp.fallback.h[:], np.float32), rp.fallback.out_width, rp.fallback.out_height))


def present_reproject_pack(rgba, position, rp, format=FR_PRESENT_RGBA8) -> np.ndarray:
    """fr_present_reproject_pack (host only): an (H, W, 4) float32 image and its (H, W, 4) float32 POSITION through
    `rp` (a PresentReproject) as (oh, ow, 4) uint8 by the reprojected present rule, through the functions the kernels
    run."""
    lib = load_library()
    a, p = (np.ascontiguousarray(x, dtype=np.float32) for x in (rgba, position))
    if a.ndim != 3 or a.shape[2] != 4 or p.shape != a.shape:
        raise ValueError("present_reproject_pack: two (H, W, 4) float32 images of one size")
    out = np.empty(rp.fallback.shape(a.shape[1], a.shape[0]) + (4,), np.uint8)
    rc = lib.fr_present_reproject_pack(C.c_void_p(a.ctypes.data), C.c_void_p(p.ctypes.data), a.shape[1], a.shape[0],
                                       int(format), C.byref(rp.c_struct()), C.c_void_p(out.ctypes.data))
    if rc:
        raise FovrtError(rc, "fr_present_reproject_pack: bad size, format or reprojection")
    return out


def shard_plan(width, height, tile, count, weights=None) -> np.ndarray:
    """fr_shard_plan (host only): tile owners dealt by smooth weighted round robin in raster order."""
    lib = load_library()
    nt = ((width + tile - 1) // tile) * ((height + tile - 1) // tile)
    owner = np.zeros(nt, np.uint8)
    w = None if weights is None else (C.c_float * count)(*[float(x) for x in weights])
    rc = lib.fr_shard_plan(int(width), int(height), int(tile), int(count), w,
                           owner.ctypes.data_as(C.POINTER(C.c_uint8)), nt)
    if rc:
        raise FovrtError(rc, lib.fr_last_error(None).decode())
    return owner


def group_plan(width, height, ranks_per_view, tile=128, split_recon=True, recon_cost=None, weights=None,
               jfa_ranks=0) -> np.ndarray:
    """fr_group_plan (host only): the tile plan fr_group_create deals for one view (view rank per tile)."""
    lib = load_library()
    cfg = fr_group_config()
    lib.fr_group_config_default(C.byref(cfg))
    cfg.tile, cfg.split_recon, cfg.jfa_ranks = int(tile), int(bool(split_recon)), int(jfa_ranks)
    if recon_cost is not None:
        cfg.recon_cost[0], cfg.recon_cost[1] = float(recon_cost[0]), float(recon_cost[1])
    if weights is not None:
        for i, w in enumerate(weights):
            cfg.weights[i] = float(w)
    nt = ((width + tile - 1) // tile) * ((height + tile - 1) // tile)
    owner = np.zeros(nt, np.uint8)
    rc = lib.fr_group_plan(int(width), int(height), int(ranks_per_view), C.byref(cfg), owner.ctypes.data, nt)
    if rc:
        raise FovrtError(rc, lib.fr_group_last_error().decode())
    return owner


def rccl_unique_id() -> bytes:
    """fr_rccl_unique_id: the 128-byte RCCL id rank 0 creates and every rank passes to Group.rccl."""
    lib = load_library()
    buf = (C.c_uint8 * 128)()
    rc = lib.fr_rccl_unique_id(buf)
    if rc:
        raise FovrtError(rc, lib.fr_group_last_error().decode())
    return bytes(buf)


class Group:
    """fr_group_*: R ranks (one PathTracer each) rendering `views` views, tile-sharded, with the sparse
    gather to the reconstruction ranks and the optional composite on rank 0 (include/fovrt.h).

    Group(tracers) puts every rank in this process (device-to-device copies); Group.rccl(tracer, id,
    nranks, rank) makes this process's tracer one rank of an RCCL communicator."""

    def __init__(self, tracers, views=1, tile=128, split_recon=True, moving_camera=False, composite=False,
                 recon_cost=None, weights=None, sample_sum=None, front_local=None, jfa_ranks=None,
                 _comm=None):
        lib = load_library()
        cfg = fr_group_config()
        lib.fr_group_config_default(C.byref(cfg))
        cfg.views, cfg.tile = int(views), int(tile)
        cfg.split_recon, cfg.moving_camera, cfg.composite = int(bool(split_recon)), int(bool(moving_camera)), int(bool(composite))
        if recon_cost is not None:
            cfg.recon_cost[0], cfg.recon_cost[1] = float(recon_cost[0]), float(recon_cost[1])
        if weights is not None:
            for i, w in enumerate(weights):
                cfg.weights[i] = float(w)
        if sample_sum is not None:
            cfg.sample_sum = int(sample_sum)
        if front_local is not None:
            cfg.front_local = int(bool(front_local))
        if jfa_ranks is not None:
            cfg.jfa_ranks = int(jfa_ranks)
        self.tracers = list(tracers)
        arr = (C.c_void_p * len(self.tracers))(*[t._ctx.value for t in self.tracers])
        h = C.c_void_p()
        rc = lib.fr_group_create(arr, len(self.tracers), _comm, C.byref(cfg), C.byref(h))
        if rc:
            raise FovrtError(rc, lib.fr_group_last_error().decode())
        self._h = h
        self._comm = _comm
        self._owns_comm = False
        self.config = cfg
        for t in self.tracers:
            if not hasattr(t, "_groups"):
                t._groups = []
            t._groups.append(self)

    @classmethod
    def rccl(cls, tracer, unique_id: bytes, nranks, rank, **kw):
        lib = load_library()
        buf = (C.c_uint8 * 128).from_buffer_copy(unique_id)
        comm = C.c_void_p()
        rc = lib.fr_rccl_comm_init(buf, int(nranks), int(rank), int(tracer.config.device), C.byref(comm))
        if rc:
            raise FovrtError(rc, lib.fr_group_last_error().decode())
        try:
            g = cls([tracer], _comm=comm, **kw)
        except Exception:
            lib.fr_rccl_comm_destroy(comm)
            raise
        g._owns_comm = True
        return g

    def _check(self, rc):
        if rc:
            raise FovrtError(rc, _lib.fr_group_last_error().decode())

    def frame(self, timing=False):
        """One frame of every local rank; timing=True returns one stage-time dict per local rank."""
        if not timing:
            self._check(_lib.fr_group_frame(self._h, None))
            return None
        t = (fr_frame_timing * len(self.tracers))()
        self._check(_lib.fr_group_frame(self._h, t))
        return [{n: getattr(x, n) for n, _ in fr_frame_timing._fields_} for x in t]

    def composite(self, device_ptr, nbytes):
        self._check(_lib.fr_group_composite(self._h, C.c_void_p(device_ptr), int(nbytes)))

    def rank_info(self, i):
        v, vr, ch, tl = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        self._check(_lib.fr_group_rank_info(self._h, int(i), C.byref(v), C.byref(vr), C.byref(ch), C.byref(tl)))
        return {"view": v.value, "view_rank": vr.value, "chains": ch.value, "tiles": tl.value}

    def output_ranks(self, view=0):
        """fr_group_output_ranks: (rank holding the last frame's JFA / Sibson, rank holding its A-Trous)."""
        a, b = C.c_int(), C.c_int()
        self._check(_lib.fr_group_output_ranks(self._h, int(view), C.byref(a), C.byref(b)))
        return a.value, b.value

    def tile_owners(self, width, height):
        """fr_group_tile_owners: the view rank tracing each screen tile, as a (tiles_y, tiles_x) array."""
        T = int(self.config.tile)
        tx, ty = (width + T - 1) // T, (height + T - 1) // T
        out = np.zeros(tx * ty, np.uint8)
        self._check(_lib.fr_group_tile_owners(self._h, out.ctypes.data, out.size))
        return out.reshape(ty, tx)

    def synchronize(self):
        self._check(_lib.fr_group_synchronize(self._h))

    def destroy(self):
        if getattr(self, "_h", None) is not None and _lib is not None:
            _lib.fr_group_destroy(self._h)
            self._h = None
            if self._owns_comm and self._comm is not None:
                _lib.fr_rccl_comm_destroy(self._comm)
                self._comm = None
        # break the tracer <-> group reference cycle: after an explicit destroy both sides are freed by
        # reference counting again (their GPU memory no longer waits for the cycle collector)
        for t in getattr(self, "tracers", ()):
            gs = getattr(t, "_groups", None)
            if gs is not None and self in gs:
                gs.remove(self)
        self.tracers = []

    def __del__(self):
        self.destroy()
