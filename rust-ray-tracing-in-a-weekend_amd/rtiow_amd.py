"""rtiow_amd — Python host binding over the C ABI (include/rt/rt_abi.h).

This mirrors the reference's host surface (themeshpotato/rust-ray-tracing-in-a-weekend):
``World`` + ``register_material`` (main.rs:40-50), the Hittable / Material / Texture
constructors (hittable.rs:77-207, material.rs:6-12, texture.rs:4-22), the scene
builders (main.rs:52-289), ``Camera::new`` (camera.rs:18-56) and the render loop
(main.rs:497-551, ray_color main.rs:19-38), which here runs as the HIP megakernel in
``lib/librtiow_amd.so``.

There is no CPU fallback: if the shared library is missing or no GPU is visible,
``Renderer`` raises. (The CPU oracle under oracle/ is test infrastructure only.)
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional, Sequence

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RT_LIB_PATH", os.path.join(HERE, "lib", "librtiow_amd.so"))
REPO = os.path.dirname(HERE)
EARTH_JPG = os.path.join(REPO, "assets", "earthmap.jpg")

RT_OK = 0
ERRORS = {-1: "RT_ERR_INVALID", -2: "RT_ERR_HIP", -3: "RT_ERR_UNSUPPORTED", -4: "RT_ERR_OOM",
          -5: "RT_ERR_NO_DEVICE", -6: "RT_ERR_NO_SCENE", -7: "RT_ERR_COMM", -8: "RT_ERR_PEER"}
RT_COMM_ID_BYTES = 128

SCENES = {"random": 0, "two_spheres": 1, "two_perlin": 2, "earth": 3, "simple_light": 4,
          "cornell": 5, "cornell_smoke": 6, "final": 7}
SCENES_NEEDING_IMAGE = (3, 7)

RT_OUT_F32, RT_OUT_F64 = 0, 1
RT_SCHED_CHUNKS = 0
RT_SCHED_POOL = 1
RT_SCHED_ITEMS = 2
RT_SCHED_AUTO = 3
RT_PREC_F64 = 0
RT_PREC_F32 = 1
RT_ACCEL_SAH = 0
RT_ACCEL_LINEAR = 1     # hit_hittables linear scan (hittable.rs:31-41)
RT_ACCEL_MEDIAN = 2     # the reference BvhNode hierarchy (hittable.rs:77-130)
# context options (rt_ctx_set_option)
RT_OPT_TRACE_BUF_BYTES = 1
RT_OPT_BATCH_OVERLAP = 2
RT_OPT_BLOCK_SAMPLES = 3
RT_OPT_BLOCK_CHUNKS = 4
RT_OPT_EXTRA_FEATURES = 5
RT_OPT_HOIST = 6
RT_OPT_POOL_RING = 9
RT_OPT_COMM_DIRECT = 10
RT_OPT_AUTO_DEAL_ORDER = 11   # 1 (default): whole frames dealt in self-measured cost order; 0 off; 2 measure only
RT_OPT_PRIMARY_CANDIDATES = 12    # 1 (default): new samples take their first hit from their pixel's candidate list; 0 off
RT_OPT_PRIMARY_CANDIDATES_K = 13  # candidates per pixel before it is flagged "walk" (1..7, default 7; tests force 1)
RT_OPT_SKIP_SKY_TILES = 14        # 1 (default): 8x8 tiles whose pixels' candidate lists are all empty are not traced; 0 off
RT_OPT_DEFER_ROOTS = 15           # 1 (default): the primary-candidate kernel computes a cast's winning sphere's exact root only; 0 off
# SAH builder options (rt_world_set_build_option)
RT_BUILD_C_ISECT = 1
RT_BUILD_MAX_LEAF = 2
RT_BUILD_FORCE_LEAF = 3
RT_BUILD_ROOT_LEAF = 4
RT_BUILD_SPLIT_BOX_PAIRS = 5
RT_BUILD_SPLIT_BLAS_PAIRS = 6
RT_BUILD_TIME0 = 7              # the ray times the node boxes are built for (default 0 and 1): set them to
RT_BUILD_TIME1 = 8              # the camera's shutter when that is not within [0, 1]

# every symbol include/rt/rt_abi.h declares
EXPORTED = [
    "rt_abi_version", "rt_last_error", "rt_device_count", "rt_ctx_create", "rt_ctx_destroy",
    "rt_world_create", "rt_world_destroy", "rt_world_texture_solid", "rt_world_texture_checker",
    "rt_world_texture_noise", "rt_world_texture_image", "rt_world_material_lambertian",
    "rt_world_material_metal", "rt_world_material_dielectric", "rt_world_material_diffuse_light",
    "rt_world_material_isotropic", "rt_world_sphere", "rt_world_moving_sphere", "rt_world_rect",
    "rt_world_box", "rt_world_translate", "rt_world_rotate_y", "rt_world_constant_medium",
    "rt_world_bvh", "rt_world_push", "rt_world_build_scene", "rt_world_info_get", "rt_camera_new",
    "rt_scene_preset_get", "rt_scene_camera", "rt_world_flatten", "rt_ctx_upload_soa",
    "rt_ctx_upload_world", "rt_render", "rt_rows_in_shard", "rt_rows_in_band_shard", "rt_tiles_in_shard", "rt_last_stats", "rt_last_counters", "rt_write_ppm",
    "rt_write_ppm_f64", "rt_write_color",
    "rt_ctx_set_variant", "rt_device_eval", "rt_accum_create", "rt_accum_destroy", "rt_accum_add",
    "rt_accum_get", "rt_accum_set", "rt_accum_resolve", "rt_render_progressive", "rt_ctx_set_schedule", "rt_ctx_set_precision",
    "rt_scene_validate", "rt_build_info", "rt_ctx_set_option", "rt_ctx_get_option", "rt_world_set_build_option",
    "rt_last_tile_costs", "rt_ctx_set_tile_order", "rt_last_deal_order",
    "rt_comm_unique_id", "rt_comm_init_rank", "rt_comm_init_all", "rt_comm_destroy", "rt_comm_rank",
    "rt_comm_tile_order", "rt_comm_tile_order_all", "rt_render_gather", "rt_render_gather_all",
    "rt_comm_last_stats", "rt_tiles_assemble", "rt_tiles_assemble_host", "rt_cost_tile_order",
    "rt_render_adaptive", "rt_adaptive_last_stats", "rt_adaptive_tile_errors_host",
    "rt_denoise", "rt_denoise_host", "rt_denoise_last_stats",
    "rt_render_features", "rt_features_last_stats", "rt_denoise_guided", "rt_denoise_guided_host",
    "rt_denoise_atrous", "rt_denoise_atrous_host", "rt_atrous_last_stats",
    "rt_denoise_pyramid", "rt_denoise_pyramid_host", "rt_pyramid_last_stats",
    "rt_render_adaptive_halves", "rt_denoise_cross", "rt_denoise_cross_host", "rt_cross_last_stats",
    "rt_adaptive_state_create", "rt_adaptive_state_destroy", "rt_adaptive_state_advance",
    "rt_adaptive_state_resolve", "rt_adaptive_state_get", "rt_adaptive_state_set",
    "rt_adaptive_state_last_stats", "rt_adaptive_next_group_host",
    "rt_primary_candidates_host", "rt_primary_sky_tiles_host",
    "rt_trace_rays", "rt_query_last_stats", "rt_camera_rays",
]

# int (*rt_progress_fn)(void* user, int64_t samples_done, int64_t samples_total)
PROGRESS_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64)


class RTError(RuntimeError):
    pass


class Camera(ctypes.Structure):
    """rt_camera == the reference's Camera struct (camera.rs:4-15)."""
    _fields_ = [("origin", ctypes.c_double * 3), ("lower_left_corner", ctypes.c_double * 3),
                ("horizontal", ctypes.c_double * 3), ("vertical", ctypes.c_double * 3),
                ("u", ctypes.c_double * 3), ("v", ctypes.c_double * 3), ("w", ctypes.c_double * 3),
                ("lens_radius", ctypes.c_double), ("time0", ctypes.c_double), ("time1", ctypes.c_double)]


class ScenePreset(ctypes.Structure):
    _fields_ = [("look_from", ctypes.c_double * 3), ("look_at", ctypes.c_double * 3),
                ("background", ctypes.c_double * 3), ("vfov", ctypes.c_double),
                ("aperture", ctypes.c_double), ("focus_dist", ctypes.c_double),
                ("time0", ctypes.c_double), ("time1", ctypes.c_double),
                ("default_width", ctypes.c_int32), ("default_spp", ctypes.c_int32),
                ("default_aspect", ctypes.c_double)]


class WorldInfo(ctypes.Structure):
    _fields_ = [("n_hittables", ctypes.c_int32), ("n_materials", ctypes.c_int32),
                ("n_leaf_prims", ctypes.c_int32), ("n_media", ctypes.c_int32), ("checksum", ctypes.c_double)]


class SceneSoA(ctypes.Structure):
    _fields_ = [("n_prims", ctypes.c_int32), ("n_prim_refs", ctypes.c_int32), ("n_nodes", ctypes.c_int32),
                ("n_instances", ctypes.c_int32), ("n_materials", ctypes.c_int32), ("n_textures", ctypes.c_int32),
                ("n_perlin", ctypes.c_int32), ("n_media", ctypes.c_int32), ("tlas_root", ctypes.c_int32),
                ("accel", ctypes.c_int32), ("image_bytes", ctypes.c_int64), ("pad_extent", ctypes.c_double),
                ("tlas_depth", ctypes.c_int32), ("blas_depth", ctypes.c_int32),
                ("n_tlas_nodes", ctypes.c_int32), ("pad0", ctypes.c_int32),
                ("prims", ctypes.c_void_p), ("prim_refs", ctypes.c_void_p), ("nodes", ctypes.c_void_p),
                ("instances", ctypes.c_void_p), ("materials", ctypes.c_void_p), ("textures", ctypes.c_void_p),
                ("perlin_ranvec", ctypes.c_void_p), ("perlin_perm", ctypes.c_void_p),
                ("image_data", ctypes.c_void_p), ("time_lo", ctypes.c_double), ("time_hi", ctypes.c_double)]


class RenderParams(ctypes.Structure):
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("spp", ctypes.c_int32),
                ("max_depth", ctypes.c_int32), ("spp_chunk", ctypes.c_int32), ("row_begin", ctypes.c_int32),
                ("row_stride", ctypes.c_int32), ("out_format", ctypes.c_int32),
                ("out_on_device", ctypes.c_int32), ("count_work", ctypes.c_int32),
                ("background", ctypes.c_double * 3), ("render_seed", ctypes.c_uint64),
                ("stream", ctypes.c_void_p), ("row_block", ctypes.c_int32), ("tile_shard", ctypes.c_int32)]


class Stats(ctypes.Structure):
    _fields_ = [("kernel_ms", ctypes.c_double), ("reduce_ms", ctypes.c_double), ("samples", ctypes.c_uint64),
                ("casts", ctypes.c_uint64), ("node_visits", ctypes.c_uint64), ("prim_tests", ctypes.c_uint64),
                ("n_items", ctypes.c_uint64), ("n_chunks", ctypes.c_int32), ("spp_chunk", ctypes.c_int32),
                ("scene_bytes", ctypes.c_int64), ("node_bytes", ctypes.c_int32), ("prim_bytes", ctypes.c_int32),
                ("material_bytes", ctypes.c_int32), ("variant_features", ctypes.c_int32),
                ("slab32", ctypes.c_int32), ("lds_stack", ctypes.c_int32), ("lds_nodes", ctypes.c_int32),
                ("cycles_camera", ctypes.c_uint64),
                ("cycles_trace", ctypes.c_uint64), ("cycles_shade", ctypes.c_uint64),
                ("wave_steps", ctypes.c_uint64), ("wave_node_steps", ctypes.c_uint64),
                ("cycles_nodes", ctypes.c_uint64), ("cycles_leaves", ctypes.c_uint64),
                ("schedule", ctypes.c_int32), ("n_batches", ctypes.c_int32),
                ("wave_leaf_steps", ctypes.c_uint64), ("camera_lanes", ctypes.c_uint64),
                ("camera_steps", ctypes.c_uint64), ("shade_lanes", ctypes.c_uint64),
                ("shade_steps", ctypes.c_uint64), ("precision", ctypes.c_int32), ("waves_per_simd", ctypes.c_int32),
                ("trace_buf_bytes", ctypes.c_int64), ("overlapped", ctypes.c_int32), ("reserved0", ctypes.c_int32),
                ("ring_bytes", ctypes.c_int64),
                ("primary_table_bytes", ctypes.c_int64), ("primary_build_ms", ctypes.c_double),
                ("primary_walk_share", ctypes.c_double), ("sky_tiles", ctypes.c_int64),
                ("defer_roots", ctypes.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class PrimaryCandidatesInfo(ctypes.Structure):
    _fields_ = [("pixels", ctypes.c_int64), ("flagged", ctypes.c_int64), ("candidates", ctypes.c_int64),
                ("max_candidates", ctypes.c_int32), ("slots", ctypes.c_int32)]


class CommStats(ctypes.Structure):
    """rt_comm_stats: the last rt_render_gather / rt_comm_tile_order of one rank."""
    _fields_ = [("render_ms", ctypes.c_double), ("gather_ms", ctypes.c_double), ("assemble_ms", ctypes.c_double),
                ("kernel_ms", ctypes.c_double), ("slab_bytes", ctypes.c_int64), ("tiles", ctypes.c_int32),
                ("tile_order", ctypes.c_int32), ("cost_pass_ms", ctypes.c_double), ("peer_failed", ctypes.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class AdaptiveParams(ctypes.Structure):
    """rt_adaptive_params."""
    _fields_ = [("min_spp", ctypes.c_int32), ("step_spp", ctypes.c_int32), ("threshold", ctypes.c_double)]


class AdaptiveOut(ctypes.Structure):
    """rt_adaptive_out: mean is required, the others may be null."""
    _fields_ = [("mean", ctypes.c_void_p), ("tile_spp", ctypes.c_void_p), ("tile_error", ctypes.c_void_p),
                ("stderr_map", ctypes.c_void_p)]


class AdaptiveHalves(ctypes.Structure):
    """rt_adaptive_halves: both required."""
    _fields_ = [("mean_a", ctypes.c_void_p), ("mean_b", ctypes.c_void_p)]


class AdaptiveStats(ctypes.Structure):
    """rt_adaptive_stats: the last rt_render_adaptive of a context."""
    _fields_ = [("passes", ctypes.c_int32), ("min_spp", ctypes.c_int32), ("step_spp", ctypes.c_int32),
                ("spp_chunk", ctypes.c_int32), ("tiles", ctypes.c_int32), ("max_pass_batches", ctypes.c_int32),
                ("samples_traced", ctypes.c_uint64), ("samples_uniform", ctypes.c_uint64),
                ("trace_ms", ctypes.c_double), ("moments_ms", ctypes.c_double), ("classify_ms", ctypes.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class AdaptiveAdvanceParams(ctypes.Structure):
    """rt_adaptive_advance_params."""
    _fields_ = [("threshold", ctypes.c_double), ("spp_cap", ctypes.c_int32), ("max_launches", ctypes.c_int32),
                ("error_on_device", ctypes.c_int32), ("reserved0", ctypes.c_int32),
                ("tile_error_in", ctypes.c_void_p), ("stream", ctypes.c_void_p)]


class AdaptiveStateHeader(ctypes.Structure):
    """rt_adaptive_state_header: what a checkpoint must match, and the host side of the state."""
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("spp_chunk", ctypes.c_int32),
                ("min_spp", ctypes.c_int32), ("step_spp", ctypes.c_int32), ("with_halves", ctypes.c_int32),
                ("ragged_cap", ctypes.c_int32), ("reserved0", ctypes.c_int32),
                ("groups_total", ctypes.c_uint64), ("samples_total", ctypes.c_uint64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class AdaptiveStateData(ctypes.Structure):
    """rt_adaptive_state_data: a checkpoint's arrays (host pointers)."""
    _fields_ = [("sums", ctypes.c_void_p), ("q", ctypes.c_void_p), ("tile_spp", ctypes.c_void_p),
                ("tile_error", ctypes.c_void_p), ("sum_a", ctypes.c_void_p), ("sum_b", ctypes.c_void_p)]


class AdaptiveStateStats(ctypes.Structure):
    """rt_adaptive_state_stats: the last advance of a state, and its totals."""
    _fields_ = [("groups", ctypes.c_int32), ("active_left", ctypes.c_int32), ("min_count", ctypes.c_int32),
                ("max_count", ctypes.c_int32), ("spp_chunk", ctypes.c_int32), ("min_spp", ctypes.c_int32),
                ("step_spp", ctypes.c_int32), ("tiles", ctypes.c_int32), ("samples_traced", ctypes.c_uint64),
                ("groups_total", ctypes.c_uint64), ("samples_total", ctypes.c_uint64),
                ("trace_ms", ctypes.c_double), ("moments_ms", ctypes.c_double), ("classify_ms", ctypes.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class AdaptiveGroup(ctypes.Structure):
    """rt_adaptive_group: what rt_adaptive_next_group_host decides."""
    _fields_ = [("n_group", ctypes.c_int64), ("n_active", ctypes.c_int64), ("n_star", ctypes.c_int32),
                ("n_next", ctypes.c_int32)]


class DenoiseParams(ctypes.Structure):
    """rt_denoise_params."""
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("format", ctypes.c_int32),
                ("on_device", ctypes.c_int32), ("radius", ctypes.c_int32), ("patch", ctypes.c_int32),
                ("k", ctypes.c_double), ("stream", ctypes.c_void_p)]


class DenoiseStats(ctypes.Structure):
    """rt_denoise_stats: the last rt_denoise of a context."""
    _fields_ = [("kernel_ms", ctypes.c_double), ("radius", ctypes.c_int32), ("patch", ctypes.c_int32),
                ("lds_bytes", ctypes.c_int32), ("reserved0", ctypes.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class FeaturesOut(ctypes.Structure):
    """rt_features_out: any may be null, not all."""
    _fields_ = [("albedo", ctypes.c_void_p), ("normal", ctypes.c_void_p), ("depth", ctypes.c_void_p)]


class FeaturesStats(ctypes.Structure):
    """rt_features_stats: the last rt_render_features of a context."""
    _fields_ = [("kernel_ms", ctypes.c_double), ("reduce_ms", ctypes.c_double), ("samples", ctypes.c_uint64),
                ("variant_features", ctypes.c_int32), ("spp_chunk", ctypes.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


# rt_ray and rt_hit as numpy record dtypes (80 bytes each, the C structs' offsets)
RAY = np.dtype([("o", "<f8", (3,)), ("d", "<f8", (3,)), ("time", "<f8"), ("t_min", "<f8"), ("t_max", "<f8"),
                ("key_pixel", "<u4"), ("key_sample", "<u4")])
HIT = np.dtype([("t", "<f8"), ("p", "<f8", (3,)), ("n", "<f8", (3,)), ("prim", "<i4"), ("inner", "<i4"), ("mat", "<i4"),
                ("flags", "<i4"), ("key_pixel", "<u4"), ("key_sample", "<u4")])
RT_HIT_FRONT, RT_HIT_MEDIUM, RT_HIT_INVALID = 1, 2, 4
RT_QUERY_CLOSEST, RT_QUERY_ANY = 0, 1


class QueryParams(ctypes.Structure):
    """rt_query_params."""
    _fields_ = [("n", ctypes.c_int64), ("mode", ctypes.c_int32), ("on_device", ctypes.c_int32), ("seed", ctypes.c_uint64),
                ("bounce", ctypes.c_uint32), ("origin_bound", ctypes.c_double), ("stream", ctypes.c_void_p)]


class QueryOut(ctypes.Structure):
    """rt_query_out: CLOSEST hits and / or albedo, ANY occluded."""
    _fields_ = [("hits", ctypes.c_void_p), ("albedo", ctypes.c_void_p), ("occluded", ctypes.c_void_p)]


class QueryStats(ctypes.Structure):
    """rt_query_stats: the last rt_trace_rays of a context."""
    _fields_ = [("kernel_ms", ctypes.c_double), ("rays", ctypes.c_int64), ("invalid", ctypes.c_int64),
                ("variant_features", ctypes.c_int32), ("slab32", ctypes.c_int32), ("mode", ctypes.c_int32),
                ("batches", ctypes.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class DenoiseGuides(ctypes.Structure):
    """rt_denoise_guides: the guide frames (any may be null) and their sigmas."""
    _fields_ = [("albedo", ctypes.c_void_p), ("normal", ctypes.c_void_p), ("depth", ctypes.c_void_p),
                ("sigma_albedo", ctypes.c_double), ("sigma_normal", ctypes.c_double), ("sigma_depth", ctypes.c_double)]


# rt_denoise_guided's default sigmas (albedo, normal, depth): the lowest RMSE of the sweep over
# {0.05, 0.1, 0.2, 0.4}^3 on C2 at threshold 0.02 with (10, 3, 0.45), guides at 16 spp; the
# loosest corner of that grid (profiles/guided_sweep_c2.json)
GUIDE_SIGMAS = (0.4, 0.4, 0.4)


class AtrousParams(ctypes.Structure):
    """rt_atrous_params."""
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("format", ctypes.c_int32),
                ("on_device", ctypes.c_int32), ("levels", ctypes.c_int32), ("demodulate", ctypes.c_int32),
                ("sigma_l", ctypes.c_double), ("stream", ctypes.c_void_p)]


class AtrousStats(ctypes.Structure):
    """rt_atrous_stats: the last rt_denoise_atrous of a context."""
    _fields_ = [("kernel_ms", ctypes.c_double), ("levels", ctypes.c_int32), ("scratch_bytes", ctypes.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


# rt_denoise_atrous's defaults (levels, sigma_l), with demodulate off: the lowest RMSE of the sweep
# over {3, 4, 5} x {1, 2, 4, 8} x {off, on} on C2 at threshold 0.02, guides at 16 spp with
# GUIDE_SIGMAS (profiles/atrous_sweep_c2.json)
ATROUS_LEVELS = 3
ATROUS_SIGMA_L = 2.0


class CrossParams(ctypes.Structure):
    """rt_cross_params."""
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("format", ctypes.c_int32),
                ("on_device", ctypes.c_int32), ("radius", ctypes.c_int32), ("patch", ctypes.c_int32),
                ("k", ctypes.c_double), ("variance_scale", ctypes.c_double), ("stream", ctypes.c_void_p)]


class CrossStats(ctypes.Structure):
    """rt_cross_stats: the last rt_denoise_cross of a context."""
    _fields_ = [("kernel_ms", ctypes.c_double), ("radius", ctypes.c_int32), ("patch", ctypes.c_int32),
                ("lds_bytes", ctypes.c_int32), ("reserved0", ctypes.c_int32), ("scratch_bytes", ctypes.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class PyramidParams(ctypes.Structure):
    """rt_pyramid_params."""
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("format", ctypes.c_int32),
                ("on_device", ctypes.c_int32), ("radius", ctypes.c_int32), ("patch", ctypes.c_int32),
                ("k", ctypes.c_double), ("levels", ctypes.c_int32), ("reserved0", ctypes.c_int32),
                ("stream", ctypes.c_void_p)]


class PyramidStats(ctypes.Structure):
    """rt_pyramid_stats: the last rt_denoise_pyramid of a context."""
    _fields_ = [("kernel_ms", ctypes.c_double), ("levels", ctypes.c_int32), ("radius", ctypes.c_int32),
                ("patch", ctypes.c_int32), ("reserved0", ctypes.c_int32), ("scratch_bytes", ctypes.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


# rt_denoise_pyramid's defaults: the small window over three levels
PYRAMID_LEVELS = 3
PYRAMID_WINDOW = (5, 2, 1.0)   # (radius, patch, k)


# rt_denoise_cross's default variance_scale: the two halves of an evenly split mean each have twice
# its variance (rt_abi.h), and of {1, 2, 4} it gives the lowest RMSE on C2 at threshold 0.02 with
# rt_denoise's default window (10, 3, 0.45), which the cross filter keeps (DESIGN.md 5.12,
# profiles/cross_scale*_c2_10_3.log)
CROSS_VARIANCE_SCALE = 2.0

_lib = None


def load_library(path: str = LIB_PATH) -> ctypes.CDLL:
    """Loads lib/librtiow_amd.so (built by __graft_entry__.build()); raises if absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise RTError(f"HIP library not built: {path} (run __graft_entry__.build())")
    lib = ctypes.CDLL(path)
    P, I, D, U64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_uint64
    PI = ctypes.POINTER(ctypes.c_int)
    PD = ctypes.POINTER(ctypes.c_double)
    sigs = {
        "rt_abi_version": ([], I), "rt_last_error": ([], ctypes.c_char_p), "rt_build_info": ([], ctypes.c_char_p),
        "rt_ctx_set_option": ([P, I, ctypes.c_int64], I),
        "rt_ctx_get_option": ([P, I, ctypes.POINTER(ctypes.c_int64)], I),
        "rt_world_set_build_option": ([P, I, D], I),
        "rt_device_count": ([PI], I), "rt_ctx_create": ([I, ctypes.POINTER(P)], I),
        "rt_ctx_destroy": ([P], None), "rt_world_create": ([U64, ctypes.POINTER(P)], I),
        "rt_world_destroy": ([P], None), "rt_world_texture_solid": ([P, D, D, D, PI], I),
        "rt_world_texture_checker": ([P, PD, PD, PI], I), "rt_world_texture_noise": ([P, D, PI], I),
        "rt_world_texture_image": ([P, P, I, I, PI], I),
        "rt_world_material_lambertian": ([P, I, PI], I), "rt_world_material_metal": ([P, PD, D, PI], I),
        "rt_world_material_dielectric": ([P, D, PI], I), "rt_world_material_diffuse_light": ([P, I, PI], I),
        "rt_world_material_isotropic": ([P, I, PI], I), "rt_world_sphere": ([P, I, PD, D, PI], I),
        "rt_world_moving_sphere": ([P, I, PD, PD, D, D, D, PI], I),
        "rt_world_rect": ([P, I, I, D, D, D, D, D, PI], I), "rt_world_box": ([P, PD, PD, I, PI], I),
        "rt_world_translate": ([P, I, PD, PI], I), "rt_world_rotate_y": ([P, I, D, PI], I),
        "rt_world_constant_medium": ([P, I, D, I, PI], I), "rt_world_bvh": ([P, PI, I, D, D, PI], I),
        "rt_world_push": ([P, I], I), "rt_world_build_scene": ([P, I, P, I, I], I),
        "rt_world_info_get": ([P, ctypes.POINTER(WorldInfo)], I),
        "rt_camera_new": ([PD, PD, PD, D, D, D, D, D, D, ctypes.POINTER(Camera)], I),
        "rt_scene_preset_get": ([I, ctypes.POINTER(ScenePreset)], I),
        "rt_scene_camera": ([I, I, I, ctypes.POINTER(Camera), PD], I),
        "rt_world_flatten": ([P, I, ctypes.POINTER(ctypes.POINTER(SceneSoA))], I),
        "rt_ctx_upload_soa": ([P, ctypes.POINTER(SceneSoA)], I),
        "rt_scene_validate": ([ctypes.POINTER(SceneSoA), ctypes.POINTER(ctypes.c_int32),
                               ctypes.POINTER(ctypes.c_int32)], I), "rt_ctx_upload_world": ([P, P, I], I),
        "rt_render": ([P, ctypes.POINTER(Camera), ctypes.POINTER(RenderParams), P], I),
        "rt_rows_in_shard": ([I, I, I], I), "rt_rows_in_band_shard": ([I, I, I, I], I),
        "rt_tiles_in_shard": ([I, I, I, I], I), "rt_last_stats": ([P, ctypes.POINTER(Stats)], I),
        "rt_last_counters": ([P, P, I], I),
        "rt_last_tile_costs": ([P, P, ctypes.c_int64], I), "rt_ctx_set_tile_order": ([P, P, ctypes.c_int64], I),
        "rt_last_deal_order": ([P, P, ctypes.c_int64], I),
        "rt_write_ppm": ([P, I, I, ctypes.c_char_p], I),
        "rt_write_ppm_f64": ([P, I, I, I, ctypes.c_char_p], I),
        "rt_write_color": ([P, I, ctypes.c_int64, P], I),
        "rt_device_eval": ([P, I, P, P, P, P, I], I), "rt_ctx_set_variant": ([P, I, I, I], I),
        "rt_accum_create": ([P, ctypes.POINTER(RenderParams), ctypes.POINTER(P)], I),
        "rt_ctx_set_schedule": ([P, I], I),
        "rt_ctx_set_precision": ([P, I], I),
        "rt_accum_destroy": ([P], None),
        "rt_accum_add": ([P, P, ctypes.POINTER(Camera), ctypes.POINTER(RenderParams), I], I),
        "rt_accum_get": ([P, P, ctypes.POINTER(ctypes.c_int64)], I),
        "rt_accum_set": ([P, P, ctypes.c_int64], I),
        "rt_accum_resolve": ([P, P, D, I, I, P], I),
        "rt_render_progressive": ([P, ctypes.POINTER(Camera), ctypes.POINTER(RenderParams), I, PROGRESS_FN, P,
                                   P], I),
        "rt_comm_unique_id": ([P], I), "rt_comm_init_rank": ([P, I, I, P, ctypes.POINTER(P)], I),
        "rt_comm_init_all": ([P, I, P], I), "rt_comm_destroy": ([P], None), "rt_comm_rank": ([P, PI, PI], I),
        "rt_comm_tile_order": ([P, ctypes.POINTER(Camera), ctypes.POINTER(RenderParams), I], I),
        "rt_comm_tile_order_all": ([P, I, ctypes.POINTER(Camera), ctypes.POINTER(RenderParams), I], I),
        "rt_render_gather": ([P, ctypes.POINTER(Camera), ctypes.POINTER(RenderParams), P], I),
        "rt_render_gather_all": ([P, I, ctypes.POINTER(Camera), ctypes.POINTER(RenderParams), P], I),
        "rt_comm_last_stats": ([P, ctypes.POINTER(CommStats)], I),
        "rt_tiles_assemble": ([P, P, ctypes.c_int64, I, ctypes.POINTER(RenderParams), P], I),
        "rt_tiles_assemble_host": ([P, ctypes.c_int64, I, I, I, I, P, P], I),
        "rt_cost_tile_order": ([P, ctypes.c_int64, P], I),
        "rt_primary_candidates_host": ([ctypes.POINTER(SceneSoA), ctypes.POINTER(Camera), I, I, I, P,
                                        ctypes.POINTER(PrimaryCandidatesInfo)], I),
        "rt_primary_sky_tiles_host": ([ctypes.POINTER(SceneSoA), ctypes.POINTER(Camera), I, I, I, P,
                                       ctypes.POINTER(ctypes.c_int64)], I),
        "rt_render_adaptive": ([P, ctypes.POINTER(Camera), ctypes.POINTER(RenderParams),
                                ctypes.POINTER(AdaptiveParams), ctypes.POINTER(AdaptiveOut)], I),
        "rt_render_adaptive_halves": ([P, ctypes.POINTER(Camera), ctypes.POINTER(RenderParams),
                                       ctypes.POINTER(AdaptiveParams), ctypes.POINTER(AdaptiveOut),
                                       ctypes.POINTER(AdaptiveHalves)], I),
        "rt_adaptive_last_stats": ([P, ctypes.POINTER(AdaptiveStats)], I),
        "rt_adaptive_tile_errors_host": ([P, P, P, I, I, P, P], I),
        "rt_denoise": ([P, ctypes.POINTER(DenoiseParams), P, P, P], I),
        "rt_denoise_host": ([ctypes.POINTER(DenoiseParams), P, P, P], I),
        "rt_denoise_last_stats": ([P, ctypes.POINTER(DenoiseStats)], I),
        "rt_render_features": ([P, ctypes.POINTER(Camera), ctypes.POINTER(RenderParams),
                                ctypes.POINTER(FeaturesOut)], I),
        "rt_features_last_stats": ([P, ctypes.POINTER(FeaturesStats)], I),
        "rt_trace_rays": ([P, ctypes.POINTER(QueryParams), P, ctypes.POINTER(QueryOut)], I),
        "rt_query_last_stats": ([P, ctypes.POINTER(QueryStats)], I),
        "rt_camera_rays": ([ctypes.POINTER(Camera), I, I, U64, I, I, P], I),
        "rt_denoise_guided": ([P, ctypes.POINTER(DenoiseParams), P, P, ctypes.POINTER(DenoiseGuides), P], I),
        "rt_denoise_guided_host": ([ctypes.POINTER(DenoiseParams), P, P, ctypes.POINTER(DenoiseGuides), P], I),
        "rt_denoise_atrous": ([P, ctypes.POINTER(AtrousParams), P, P, ctypes.POINTER(DenoiseGuides), P, P], I),
        "rt_denoise_atrous_host": ([ctypes.POINTER(AtrousParams), P, P, ctypes.POINTER(DenoiseGuides), P, P], I),
        "rt_atrous_last_stats": ([P, ctypes.POINTER(AtrousStats)], I),
        "rt_denoise_pyramid": ([P, ctypes.POINTER(PyramidParams), P, P, ctypes.POINTER(DenoiseGuides), P], I),
        "rt_denoise_pyramid_host": ([ctypes.POINTER(PyramidParams), P, P, ctypes.POINTER(DenoiseGuides), P], I),
        "rt_pyramid_last_stats": ([P, ctypes.POINTER(PyramidStats)], I),
        "rt_denoise_cross": ([P, ctypes.POINTER(CrossParams), P, P, P, ctypes.POINTER(DenoiseGuides), P, P], I),
        "rt_denoise_cross_host": ([ctypes.POINTER(CrossParams), P, P, P, ctypes.POINTER(DenoiseGuides), P, P], I),
        "rt_cross_last_stats": ([P, ctypes.POINTER(CrossStats)], I),
        "rt_adaptive_state_create": ([P, ctypes.POINTER(Camera), ctypes.POINTER(RenderParams),
                                      ctypes.POINTER(AdaptiveParams), I, ctypes.POINTER(P)], I),
        "rt_adaptive_state_destroy": ([P], None),
        "rt_adaptive_state_advance": ([P, ctypes.POINTER(AdaptiveAdvanceParams), ctypes.POINTER(ctypes.c_int32)], I),
        "rt_adaptive_state_resolve": ([P, I, I, ctypes.POINTER(AdaptiveOut), ctypes.POINTER(AdaptiveHalves)], I),
        "rt_adaptive_state_get": ([P, ctypes.POINTER(AdaptiveStateHeader), ctypes.POINTER(AdaptiveStateData)], I),
        "rt_adaptive_state_set": ([P, ctypes.POINTER(AdaptiveStateHeader), ctypes.POINTER(AdaptiveStateData)], I),
        "rt_adaptive_state_last_stats": ([P, ctypes.POINTER(AdaptiveStateStats)], I),
        "rt_adaptive_next_group_host": ([P, P, P, ctypes.c_int64, D, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, P,
                                         ctypes.POINTER(AdaptiveGroup)], I),
    }
    for name, (args, res) in sigs.items():
        fn = getattr(lib, name, None)
        if fn is None:   # an older build (A/B runs); build() and tests/test_abi.py check every export
            continue
        fn.argtypes = args
        fn.restype = res
    _lib = lib
    return lib


def build_info() -> str:
    """rt_build_info: the source hash the loaded library was compiled from."""
    return load_library().rt_build_info().decode()


def _check(rc: int, what: str) -> None:
    if rc != RT_OK:
        msg = _lib.rt_last_error().decode() if _lib is not None else ""
        raise RTError(f"{what} failed: {ERRORS.get(rc, rc)} {msg}")


def _stats(owner, fn_name: str, Struct):
    """Struct as the last-stats export fn_name fills it for owner's handle."""
    s = Struct()
    _check(getattr(owner.lib, fn_name)(owner.h, ctypes.byref(s)), fn_name)
    return s


def _d3(v: Sequence[float]):
    return (ctypes.c_double * 3)(*[float(x) for x in v])


def load_earth_texture(path: str = EARTH_JPG) -> np.ndarray:
    """RGB8 texels of textures/earthmap.jpg (texture.rs:12-22; decoded with PIL instead of stb_image)."""
    from PIL import Image
    return np.ascontiguousarray(np.asarray(Image.open(path).convert("RGB"), dtype=np.uint8))


class World:
    """The reference's World (main.rs:40-50) with its Hittable / Material / Texture constructors."""

    def __init__(self, scene_seed: int = 1):
        self.lib = load_library()
        h = ctypes.c_void_p()
        _check(self.lib.rt_world_create(ctypes.c_uint64(scene_seed), ctypes.byref(h)), "rt_world_create")
        self.h = h
        self._keep = []

    def close(self):
        if self.h:
            self.lib.rt_world_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _id(self, fn, *args) -> int:
        out = ctypes.c_int()
        _check(fn(self.h, *args, ctypes.byref(out)), fn.__name__)
        return out.value

    # textures (texture.rs:4-22)
    def solid(self, r, g, b): return self._id(self.lib.rt_world_texture_solid, r, g, b)
    def checker(self, even, odd): return self._id(self.lib.rt_world_texture_checker, _d3(even), _d3(odd))
    def noise(self, scale): return self._id(self.lib.rt_world_texture_noise, scale)

    def image(self, rgb: np.ndarray):
        rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
        return self._id(self.lib.rt_world_texture_image, rgb.ctypes.data, rgb.shape[1], rgb.shape[0])

    # materials (material.rs:6-12) -> 1-based handles
    def lambertian(self, tex): return self._id(self.lib.rt_world_material_lambertian, tex)
    def metal(self, albedo, fuzz): return self._id(self.lib.rt_world_material_metal, _d3(albedo), fuzz)
    def dielectric(self, ir): return self._id(self.lib.rt_world_material_dielectric, ir)
    def diffuse_light(self, tex): return self._id(self.lib.rt_world_material_diffuse_light, tex)
    def isotropic(self, tex): return self._id(self.lib.rt_world_material_isotropic, tex)

    # hittables (hittable.rs:30-41)
    def sphere(self, mat, center, radius): return self._id(self.lib.rt_world_sphere, mat, _d3(center), radius)

    def moving_sphere(self, mat, c0, c1, t0, t1, radius):
        return self._id(self.lib.rt_world_moving_sphere, mat, _d3(c0), _d3(c1), t0, t1, radius)

    def xy_rect(self, mat, x0, x1, y0, y1, k): return self._id(self.lib.rt_world_rect, 0, mat, x0, x1, y0, y1, k)
    def xz_rect(self, mat, x0, x1, z0, z1, k): return self._id(self.lib.rt_world_rect, 1, mat, x0, x1, z0, z1, k)
    def yz_rect(self, mat, y0, y1, z0, z1, k): return self._id(self.lib.rt_world_rect, 2, mat, y0, y1, z0, z1, k)
    def box(self, mn, mx, mat): return self._id(self.lib.rt_world_box, _d3(mn), _d3(mx), mat)
    def translate(self, child, offset): return self._id(self.lib.rt_world_translate, child, _d3(offset))
    def rotate_y(self, child, angle): return self._id(self.lib.rt_world_rotate_y, child, angle)

    def constant_medium(self, boundary, density, phase):
        return self._id(self.lib.rt_world_constant_medium, boundary, density, phase)

    def bvh(self, ids, t0=0.0, t1=1.0):
        arr = (ctypes.c_int * len(ids))(*ids)
        return self._id(self.lib.rt_world_bvh, arr, len(ids), t0, t1)

    def push(self, hid):
        _check(self.lib.rt_world_push(self.h, hid), "rt_world_push")

    def set_build_option(self, key: int, value: float):
        """rt_world_set_build_option: an SAH builder option of this world's flatten (RT_BUILD_*)."""
        _check(self.lib.rt_world_set_build_option(self.h, key, float(value)), "rt_world_set_build_option")
        return self

    def build_scene(self, scene_id: int, image: Optional[np.ndarray] = None):
        """The reference's scene builders (main.rs:52-289)."""
        if scene_id in SCENES_NEEDING_IMAGE and image is None:
            image = load_earth_texture()
        if image is not None:
            image = np.ascontiguousarray(image, dtype=np.uint8)
            self._keep.append(image)
            ptr, w, h = image.ctypes.data, image.shape[1], image.shape[0]
        else:
            ptr, w, h = None, 0, 0
        _check(self.lib.rt_world_build_scene(self.h, scene_id, ptr, w, h), "rt_world_build_scene")
        return self

    def info(self) -> WorldInfo:
        out = WorldInfo()
        _check(self.lib.rt_world_info_get(self.h, ctypes.byref(out)), "rt_world_info_get")
        return out

    def flatten(self, accel: int = RT_ACCEL_SAH) -> SceneSoA:
        p = ctypes.POINTER(SceneSoA)()
        _check(self.lib.rt_world_flatten(self.h, accel, ctypes.byref(p)), "rt_world_flatten")
        return p.contents


def validate_soa(soa: SceneSoA):
    """rt_scene_validate: (tlas_depth, blas_depth) the kernel's walks need; raises RTError on a
    malformed table (out-of-range index, cycle, too deep)."""
    lib = load_library()
    t, b = ctypes.c_int32(), ctypes.c_int32()
    _check(lib.rt_scene_validate(ctypes.byref(soa), ctypes.byref(t), ctypes.byref(b)), "rt_scene_validate")
    return t.value, b.value


def primary_candidates_host(soa: SceneSoA, cam: Camera, width: int, height: int, k_max: int = 7):
    """rt_primary_candidates_host: (records (height, width, 8) uint16 — [..., 0] the candidate count or
    0xffff for a pixel flagged "walk", then leaf slots — and the table's PrimaryCandidatesInfo)."""
    rec = np.zeros((height, width, 8), dtype=np.uint16)
    info = PrimaryCandidatesInfo()
    _check(load_library().rt_primary_candidates_host(ctypes.byref(soa), ctypes.byref(cam), width, height, k_max,
                                                     rec.ctypes.data, ctypes.byref(info)), "rt_primary_candidates_host")
    return rec, info


def primary_sky_tiles_host(soa: SceneSoA, cam: Camera, width: int, height: int, k_max: int = 7):
    """rt_primary_sky_tiles_host: (flags (ceil(height / 8), ceil(width / 8)) uint8 — 1 where every pixel of
    the 8x8 raster tile within the frame has an empty candidate list — and how many are 1)."""
    flags = np.zeros(((height + 7) // 8, (width + 7) // 8), dtype=np.uint8)
    n = ctypes.c_int64()
    _check(load_library().rt_primary_sky_tiles_host(ctypes.byref(soa), ctypes.byref(cam), width, height, k_max,
                                                    flags.ctypes.data, ctypes.byref(n)), "rt_primary_sky_tiles_host")
    return flags, n.value


def camera_rays(cam: Camera, width: int, height: int, seed: int, sample: int, tiled: bool = False) -> np.ndarray:
    """rt_camera_rays: the width * height RAY records rt_render shoots for `sample` of every pixel under
    render seed `seed` (t_min 0.001, t_max inf, key (pixel, sample)); row-major from the bottom row, or
    (tiled) 8x8 tiles in tile-grid order."""
    rays = np.zeros(width * height, dtype=RAY)
    lib = load_library()
    _check(lib.rt_camera_rays(ctypes.byref(cam), width, height, seed, sample, int(bool(tiled)), rays.ctypes.data),
           "rt_camera_rays")
    return rays


def camera_new(look_from, look_at, vup, vfov, aspect_ratio, aperture, focus_dist, time0, time1) -> Camera:
    lib = load_library()
    cam = Camera()
    _check(lib.rt_camera_new(_d3(look_from), _d3(look_at), _d3(vup), vfov, aspect_ratio, aperture, focus_dist,
                             time0, time1, ctypes.byref(cam)), "rt_camera_new")
    return cam


def scene_preset(scene_id: int) -> ScenePreset:
    lib = load_library()
    out = ScenePreset()
    _check(lib.rt_scene_preset_get(scene_id, ctypes.byref(out)), "rt_scene_preset_get")
    return out


def scene_camera(scene_id: int, width: int, height: int):
    """(Camera, background) of a preset scene at width x height (aspect = width/height)."""
    lib = load_library()
    cam = Camera()
    bg = (ctypes.c_double * 3)()
    _check(lib.rt_scene_camera(scene_id, width, height, ctypes.byref(cam), bg), "rt_scene_camera")
    return cam, tuple(bg)


def rows_in_shard(height: int, row_begin: int, row_stride: int, row_block: int = 1) -> int:
    if row_block > 1:
        return load_library().rt_rows_in_band_shard(height, row_begin, row_stride, row_block)
    return load_library().rt_rows_in_shard(height, row_begin, row_stride)


def shard_shape(params) -> tuple:
    """(rows, width) of a render's output: its rows of the image, or a tile shard's slab."""
    if params.tile_shard:
        n = tiles_in_shard(params.width, params.height, params.row_begin, params.row_stride)
        return (8 if n else 0), 8 * n
    return rows_in_shard(params.height, params.row_begin, params.row_stride, params.row_block), params.width


def shard_rows(height: int, rank: int, world: int, row_block: int = 1):
    """Image rows of rank `rank` in the N-way partition, in the shard's order: single rows
    y = rank + k*world, or bands of row_block rows interleaved the same way."""
    if row_block <= 1:
        return list(range(rank, height, world))
    return [y for band in range(rank, (height + row_block - 1) // row_block, world)
            for y in range(band * row_block, min(height, (band + 1) * row_block))]


def tiles_in_shard(width: int, height: int, tile_begin: int, tile_stride: int) -> int:
    """8x8 tiles of a tile shard (rt_render_params.tile_shard = 1)."""
    return load_library().rt_tiles_in_shard(width, height, tile_begin, tile_stride)


def _perm(a, axes):
    return a.permute(*axes) if hasattr(a, "permute") else a.transpose(axes)


def cost_tile_order(costs) -> np.ndarray:
    """rt_ctx_set_tile_order's order from per-tile costs (rt_last_tile_costs): the raster tiles
    by cost, most expensive first (ties in raster order). Dealt round-robin, every shard gets
    every N-th tile of the sorted list, so the shards' costs differ by at most about one
    tile's, and each shard renders its expensive tiles first. Integer costs go through the
    library's rt_cost_tile_order (what rt_comm_tile_order sets); others are sorted here."""
    c = np.asarray(costs)
    if c.dtype.kind in "ui" and (c.size == 0 or c.min() >= 0):
        c = np.ascontiguousarray(c, dtype=np.uint64)
        out = np.empty(c.size, dtype=np.uint32)
        _check(load_library().rt_cost_tile_order(c.ctypes.data, c.size, out.ctypes.data), "rt_cost_tile_order")
        return out
    return np.argsort(-np.asarray(c, dtype=np.float64), kind="stable").astype(np.uint32)


def assemble_tiles_host(slabs: np.ndarray, width: int, height: int, world: int, order=None) -> np.ndarray:
    """rt_tiles_assemble_host: slabs is world x slab_elems (f32 or f64; rank r's tile slab, padded
    to the largest shard's, at row r) -> the height x width x 3 frame."""
    a = np.ascontiguousarray(slabs)
    if a.dtype not in (np.float32, np.float64) or a.ndim < 2 or a.shape[0] != world:
        raise RTError("slabs: world x slab_elems of f32 / f64")
    a = a.reshape(world, -1)
    o = None if order is None else np.ascontiguousarray(order, dtype=np.uint32)
    out = np.zeros((height, width, 3), dtype=a.dtype)
    _check(load_library().rt_tiles_assemble_host(a.ctypes.data, a.shape[1], world, width, height, a.dtype.itemsize,
                                                 None if o is None else o.ctypes.data, out.ctypes.data),
           "rt_tiles_assemble_host")
    return out


def scattered_tile_order(n_tiles: int, stride: int) -> np.ndarray:
    """Every stride-th raster tile first (0, s, 2s, ...), then 1, 1 + s, ...: one GPU's frame
    spread over the image as an s-way round-robin shard is (scripts/tile_locality.py)."""
    return np.concatenate([np.arange(k, n_tiles, stride) for k in range(stride)]).astype(np.uint32)


def grouped_tile_order(n_tiles: int, world: int, group: int) -> np.ndarray:
    """A tile order that deals runs of `group` consecutive raster tiles round-robin over `world`
    tile shards (run j to shard j mod world), instead of single tiles: each shard's waves then work
    on neighbouring tiles. Shard r holds positions r, r + world, ... (rt_tiles_in_shard tiles);
    a run that does not fit its shard's remaining count continues on the next shard with room."""
    cap = [len(range(r, n_tiles, world)) for r in range(world)]
    lists = [[] for _ in range(world)]
    for j, t0 in enumerate(range(0, n_tiles, group)):
        k = j % world
        for t in range(t0, min(t0 + group, n_tiles)):
            while cap[k] == 0:
                k = (k + 1) % world
            lists[k].append(t)
            cap[k] -= 1
    order = np.empty(n_tiles, dtype=np.uint32)
    for r in range(world):
        order[r::world] = lists[r]
    return order


def assemble_tiles(slabs, width: int, height: int, world: int, out=None, order=None):
    """Inverse of the tile partition: slabs[r] is rank r's 8 x (8 * n_r) x 3 tile slab (the
    tiles at positions t = r + m*world side by side: raster tiles, or order[t] with a tile order
    set on the renderers, rt_ctx_set_tile_order; wider padding is ignored). Works on numpy
    arrays and torch tensors alike; returns the height x width x 3 frame."""
    tx, ty = (width + 7) // 8, (height + 7) // 8
    like = slabs[0]
    if hasattr(like, "new_empty"):
        tiles = like.new_empty((ty * tx, 8, 8, like.shape[-1]))
        if order is not None:
            import torch as _torch
            order = _torch.as_tensor(np.ascontiguousarray(order, dtype=np.int64), device=like.device)
    else:
        import numpy as _np
        tiles = _np.empty((ty * tx, 8, 8, like.shape[-1]), dtype=like.dtype)
        if order is not None:
            order = _np.asarray(order, dtype=_np.int64)
    if order is not None and len(order) != tx * ty:
        raise ValueError(f"tile order of {len(order)} tiles for a frame of {tx * ty}")
    for r in range(world):
        n = len(range(r, ty * tx, world))
        if n:
            dst = slice(r, None, world) if order is None else order[r::world]
            tiles[dst] = _perm(slabs[r][:, :8 * n].reshape(8, n, 8, like.shape[-1]), (1, 0, 2, 3))
    frame = _perm(tiles.reshape(ty, tx, 8, 8, like.shape[-1]), (0, 2, 1, 3, 4)).reshape(ty * 8, tx * 8, like.shape[-1])
    if out is None:
        return frame[:height, :width]
    out[...] = frame[:height, :width]
    return out


def assemble_rows(slabs, height: int, world: int, out=None, row_block: int = 1):
    """Inverse of the row partition: slabs[r] holds rank r's rows (padded to the largest
    shard). Works on numpy arrays and torch tensors alike."""
    if out is None:
        import numpy as _np
        out = _np.empty((height,) + tuple(slabs[0].shape[1:]), dtype=slabs[0].dtype)
    for r in range(world):
        if row_block <= 1:
            n = len(range(r, height, world))
            out[r::world] = slabs[r][:n]
            continue
        k = 0
        for band in range(r, (height + row_block - 1) // row_block, world):
            y0, y1 = band * row_block, min(height, (band + 1) * row_block)
            out[y0:y1] = slabs[r][k:k + (y1 - y0)]
            k += y1 - y0
    return out


def adaptive_tile_errors_host(sums, q, tile_spp, width: int, height: int):
    """rt_adaptive_tile_errors_host: the adaptive criterion (rt_abi.h) on the host, no device needed.
    sums: height x width x 3 RGB sums, q: height x width sums of squared sample luminances,
    tile_spp: samples per pixel of each raster 8x8 tile (all >= 2). Returns (tile_error per raster
    tile, stderr_map height x width)."""
    lib = load_library()
    tiles = ((width + 7) // 8) * ((height + 7) // 8)
    s = np.ascontiguousarray(sums, dtype=np.float64)
    qq = np.ascontiguousarray(q, dtype=np.float64)
    n = np.ascontiguousarray(np.asarray(tile_spp).reshape(-1), dtype=np.uint32)
    if s.size != width * height * 3 or qq.size != width * height or n.size != tiles:
        raise RTError(f"adaptive_tile_errors_host: {s.shape}, {qq.shape}, {n.shape} do not fit {width} x {height}")
    err = np.empty(tiles, dtype=np.float64)
    se = np.empty((height, width), dtype=np.float64)
    _check(lib.rt_adaptive_tile_errors_host(s.ctypes.data, qq.ctypes.data, n.ctypes.data, width, height,
                                            err.ctypes.data, se.ctypes.data), "rt_adaptive_tile_errors_host")
    return err, se


def adaptive_next_group_host(tile_spp, threshold: float, spp_cap: int, min_r: int, step_r: int, tile_error=None,
                             selected=None):
    """rt_adaptive_next_group_host: the selection rule of an rt_adaptive_state (rt_abi.h) on the host,
    no device needed. Give tile_error (the threshold decides) or selected (a mask, nonzero =
    selected). Returns (group: raster indices ascending, n_star, n_next, n_active)."""
    lib = load_library()
    n = np.ascontiguousarray(tile_spp, dtype=np.uint32).reshape(-1)
    err = None if tile_error is None else np.ascontiguousarray(tile_error, dtype=np.float64).reshape(-1)
    sel = None if selected is None else np.ascontiguousarray(np.asarray(selected) != 0, dtype=np.uint8).reshape(-1)
    for a in (err, sel):
        if a is not None and a.size != n.size:
            raise RTError(f"adaptive_next_group_host: {a.size} values for {n.size} tiles")
    group = np.empty(max(n.size, 1), dtype=np.uint32)
    g = AdaptiveGroup()
    _check(lib.rt_adaptive_next_group_host(n.ctypes.data, None if err is None else err.ctypes.data,
                                           None if sel is None else sel.ctypes.data, n.size, float(threshold),
                                           int(spp_cap), int(min_r), int(step_r), group.ctypes.data, ctypes.byref(g)),
           "rt_adaptive_next_group_host")
    return group[:g.n_group].copy(), g.n_star, g.n_next, g.n_active


def _denoise_args(mean, se, radius, patch, k):
    """(params, mean, se) of a host-pointer denoise call: mean height x width x 3 f32 or f64 (its
    dtype is the format), se height x width."""
    m = np.asarray(mean)
    if m.ndim != 3 or m.shape[2] != 3:
        raise RTError(f"denoise: mean is {m.shape}, not height x width x 3")
    m = np.ascontiguousarray(m, dtype=np.float32 if m.dtype == np.float32 else np.float64)
    s = np.ascontiguousarray(se, dtype=np.float64)
    if s.shape != m.shape[:2]:
        raise RTError(f"denoise: the error map is {s.shape}, the frame {m.shape[:2]}")
    fmt = RT_OUT_F64 if m.dtype == np.float64 else RT_OUT_F32
    return DenoiseParams(m.shape[1], m.shape[0], fmt, 0, int(radius), int(patch), float(k), None), m, s


def denoise_host(mean, se, radius: int = 10, patch: int = 3, k: float = 0.45) -> np.ndarray:
    """rt_denoise_host: the variance-guided NL-means filter (rt_abi.h) on the host, no device needed.
    mean: height x width x 3 f32 or f64, se: height x width (render_adaptive's stderr_map).
    Returns the filtered frame in mean's format."""
    lib = load_library()
    p, m, s = _denoise_args(mean, se, radius, patch, k)
    out = np.empty_like(m)
    _check(lib.rt_denoise_host(ctypes.byref(p), m.ctypes.data, s.ctypes.data, out.ctypes.data), "rt_denoise_host")
    return out


def _guides(albedo_ptr, normal_ptr, depth_ptr, sigmas):
    """rt_denoise_guides from the three frames' addresses (0 or None leaves one out) and
    sigmas = (albedo, normal, depth)."""
    sa, sn, sz = (float(v) for v in sigmas)
    return DenoiseGuides(albedo_ptr or None, normal_ptr or None, depth_ptr or None, sa, sn, sz)


def _guide_args(shape, albedo, normal, depth, sigmas):
    """(rt_denoise_guides, the arrays it points into) of a host-pointer guided call: albedo and normal
    height x width x 3, depth height x width, f64; None leaves a guide out."""
    H, W = shape
    keep = []

    def arr(a, want, name):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype=np.float64)
        if a.shape != want:
            raise RTError(f"denoise_guided: the {name} guide is {a.shape}, not {want}")
        keep.append(a)
        return a.ctypes.data

    g = _guides(arr(albedo, (H, W, 3), "albedo"), arr(normal, (H, W, 3), "normal"), arr(depth, (H, W), "depth"),
                sigmas)
    return g, keep


def denoise_guided_host(mean, se, albedo=None, normal=None, depth=None, sigmas=GUIDE_SIGMAS, radius: int = 10,
                        patch: int = 3, k: float = 0.45) -> np.ndarray:
    """rt_denoise_guided_host: the feature-guided NL-means filter (rt_abi.h) on the host, no device
    needed. mean and se as denoise_host; albedo, normal (height x width x 3) and depth (height x
    width) as render_features returns them, None to leave one out; sigmas = (albedo, normal, depth)."""
    lib = load_library()
    p, m, s = _denoise_args(mean, se, radius, patch, k)
    g, keep = _guide_args(m.shape[:2], albedo, normal, depth, sigmas)
    out = np.empty_like(m)
    _check(lib.rt_denoise_guided_host(ctypes.byref(p), m.ctypes.data, s.ctypes.data, ctypes.byref(g), out.ctypes.data),
           "rt_denoise_guided_host")
    del keep
    return out


def _atrous_args(mean, se, levels, sigma_l, demodulate):
    """(params, mean, se) of a host-pointer a-trous call: mean and se as _denoise_args takes them."""
    d, m, s = _denoise_args(mean, se, 1, 0, 1.0)
    return AtrousParams(d.width, d.height, d.format, 0, int(levels), int(demodulate), float(sigma_l), None), m, s


def denoise_atrous_host(mean, se, albedo=None, normal=None, depth=None, sigmas=GUIDE_SIGMAS,
                        levels: int = ATROUS_LEVELS, sigma_l: float = ATROUS_SIGMA_L, demodulate: bool = False,
                        want_stderr: bool = True):
    """rt_denoise_atrous_host: the variance-guided a-trous wavelet filter (rt_abi.h) on the host, no
    device needed. mean, se and the guides as denoise_guided_host takes them; demodulate filters
    colour / albedo (needs albedo). Returns (the filtered frame in mean's format, the standard error
    left in it, height x width f64, or None without want_stderr)."""
    lib = load_library()
    p, m, s = _atrous_args(mean, se, levels, sigma_l, demodulate)
    g, keep = _guide_args(m.shape[:2], albedo, normal, depth, sigmas)
    out = np.empty_like(m)
    se_out = np.empty_like(s) if want_stderr else None
    _check(lib.rt_denoise_atrous_host(ctypes.byref(p), m.ctypes.data, s.ctypes.data, ctypes.byref(g), out.ctypes.data,
                                      se_out.ctypes.data if want_stderr else None), "rt_denoise_atrous_host")
    del keep
    return out, se_out


def _pyramid_args(mean, se, radius, patch, k, levels):
    """(params, mean, se) of a host-pointer pyramid call: mean and se as _denoise_args takes them."""
    d, m, s = _denoise_args(mean, se, radius, patch, k)
    return PyramidParams(d.width, d.height, d.format, 0, d.radius, d.patch, d.k, int(levels), 0, None), m, s


def denoise_pyramid_host(mean, se, albedo=None, normal=None, depth=None, sigmas=GUIDE_SIGMAS,
                         radius: int = PYRAMID_WINDOW[0], patch: int = PYRAMID_WINDOW[1], k: float = PYRAMID_WINDOW[2],
                         levels: int = PYRAMID_LEVELS) -> np.ndarray:
    """rt_denoise_pyramid_host: the multi-scale NL-means filter (rt_abi.h) on the host, no device
    needed. mean, se and the guides as denoise_guided_host takes them. Returns the filtered frame in
    mean's format."""
    lib = load_library()
    p, m, s = _pyramid_args(mean, se, radius, patch, k, levels)
    g, keep = _guide_args(m.shape[:2], albedo, normal, depth, sigmas)
    out = np.empty_like(m)
    _check(lib.rt_denoise_pyramid_host(ctypes.byref(p), m.ctypes.data, s.ctypes.data, ctypes.byref(g), out.ctypes.data),
           "rt_denoise_pyramid_host")
    del keep
    return out


def _cross_args(mean_a, mean_b, se, radius, patch, k, variance_scale):
    """(params, mean_a, mean_b, se) of a host-pointer cross call: the half means as _denoise_args
    takes a mean, both of one format and shape."""
    d, a, s = _denoise_args(mean_a, se, radius, patch, k)
    b = np.asarray(mean_b)
    b = np.ascontiguousarray(b, dtype=np.float32 if b.dtype == np.float32 else np.float64)
    if b.shape != a.shape or b.dtype != a.dtype:
        raise RTError(f"denoise_cross: mean_b is {b.shape} {b.dtype}, mean_a {a.shape} {a.dtype}")
    p = CrossParams(d.width, d.height, d.format, 0, int(radius), int(patch), float(k), float(variance_scale), None)
    return p, a, b, s


def denoise_cross_host(mean_a, mean_b, se, albedo=None, normal=None, depth=None, sigmas=GUIDE_SIGMAS,
                       radius: int = 10, patch: int = 3, k: float = 0.45,
                       variance_scale: float = CROSS_VARIANCE_SCALE, want_stderr: bool = True):
    """rt_denoise_cross_host: the cross-filtered NL-means over two half frames (rt_abi.h) on the host,
    no device needed. mean_a, mean_b: height x width x 3, both f32 or both f64; se: the whole mean's
    standard error, height x width; the guides as denoise_guided_host takes them. Returns (the
    filtered frame in the means' format, the standard error the halves' disagreement leaves in it,
    height x width f64, or None without want_stderr)."""
    lib = load_library()
    p, a, b, s = _cross_args(mean_a, mean_b, se, radius, patch, k, variance_scale)
    g, keep = _guide_args(a.shape[:2], albedo, normal, depth, sigmas)
    out = np.empty_like(a)
    se_out = np.empty_like(s) if want_stderr else None
    _check(lib.rt_denoise_cross_host(ctypes.byref(p), a.ctypes.data, b.ctypes.data, s.ctypes.data, ctypes.byref(g),
                                     out.ctypes.data, se_out.ctypes.data if want_stderr else None),
           "rt_denoise_cross_host")
    del keep
    return out, se_out


def write_ppm(rgb: np.ndarray, path: str, samples_per_pixel: int = 1) -> None:
    """P3 writer of the reference (write_color, math.rs:119-132; main.rs:472, 591-596):
    height x width x 3, row 0 = bottom. An f64 array takes rt_write_ppm_f64 — the reference's
    bytes exactly: pass rt_render's RT_OUT_F64 mean with samples_per_pixel=1, or per-pixel sums
    (Accumulator.get) with their spp. An f32 array (the f32 frame) takes rt_write_ppm, whose
    f32-rounded mean can move a channel at a rounding boundary by one."""
    lib = load_library()
    if np.asarray(rgb).dtype == np.float64:
        a = np.ascontiguousarray(rgb, dtype=np.float64)
        _check(lib.rt_write_ppm_f64(a.ctypes.data, samples_per_pixel, a.shape[1], a.shape[0], str(path).encode()),
               "rt_write_ppm_f64")
        return
    if samples_per_pixel != 1:
        raise RTError("an f32 frame is a mean: samples_per_pixel must be 1")
    a = np.ascontiguousarray(rgb, dtype=np.float32)
    _check(lib.rt_write_ppm(a.ctypes.data, a.shape[1], a.shape[0], str(path).encode()), "rt_write_ppm")


def write_color(rgb: np.ndarray, samples_per_pixel: int = 1) -> np.ndarray:
    """The reference's write_color channel values (int32, same shape) of f64 sums / means."""
    lib = load_library()
    a = np.ascontiguousarray(rgb, dtype=np.float64)
    out = np.empty(a.shape, dtype=np.int32)
    _check(lib.rt_write_color(a.ctypes.data, samples_per_pixel, a.size // 3, out.ctypes.data), "rt_write_color")
    return out


class Renderer:
    """One device context: upload a world, render row shards through the megakernel."""

    def __init__(self, device: int = 0):
        self.lib = load_library()
        n = ctypes.c_int()
        _check(self.lib.rt_device_count(ctypes.byref(n)), "rt_device_count")
        if n.value <= 0:
            raise RTError("no HIP device visible")
        h = ctypes.c_void_p()
        _check(self.lib.rt_ctx_create(device, ctypes.byref(h)), "rt_ctx_create")
        self.h = h

    def close(self):
        if self.h:
            self.lib.rt_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def upload(self, world: World, accel: int = RT_ACCEL_SAH):
        _check(self.lib.rt_ctx_upload_world(self.h, world.h, accel), "rt_ctx_upload_world")

    @staticmethod
    def params(width, height, spp, max_depth=50, background=(0.0, 0.0, 0.0), render_seed=1, row_begin=0,
               row_stride=1, spp_chunk=0, out_format=RT_OUT_F32, out_on_device=0, count_work=0, stream=None,
               row_block=1, tile_shard=0):
        p = RenderParams()
        p.row_block = row_block
        p.tile_shard = tile_shard
        p.width, p.height, p.spp, p.max_depth = width, height, spp, max_depth
        p.spp_chunk, p.row_begin, p.row_stride = spp_chunk, row_begin, row_stride
        p.out_format, p.out_on_device, p.count_work = out_format, out_on_device, count_work
        p.background = _d3(background)
        p.render_seed = render_seed
        p.stream = stream
        return p

    def render(self, camera: Camera, params: RenderParams, out=None) -> np.ndarray:
        """Host-output render: returns rows_local x width x 3 mean radiance (row k = k-th selected
        row), or for a tile shard its 8 x (8 * tiles_local) x 3 slab."""
        n_rows, width = shard_shape(params)
        dt = np.float64 if params.out_format == RT_OUT_F64 else np.float32
        if out is None:
            out = np.empty((n_rows, width, 3), dtype=dt)
        if out.dtype != dt or out.size < n_rows * width * 3 or not out.flags.c_contiguous:
            raise RTError(f"output buffer too small or of the wrong type for {n_rows} x {width} x 3 {dt}")
        params.out_on_device = 0
        _check(self.lib.rt_render(self.h, ctypes.byref(camera), ctypes.byref(params), out.ctypes.data), "rt_render")
        return out

    def render_device(self, camera: Camera, params: RenderParams, dev_ptr: int, stream: Optional[int] = None):
        """Enqueues a render into a device buffer (e.g. a torch tensor's data_ptr()) on `stream`."""
        params.out_on_device = 1
        params.stream = stream
        _check(self.lib.rt_render(self.h, ctypes.byref(camera), ctypes.byref(params), ctypes.c_void_p(dev_ptr)),
               "rt_render")

    def render_progressive(self, camera: Camera, params: RenderParams, batch_spp: int, progress=None) -> np.ndarray:
        """rt_render in sample batches; progress(samples_done, samples_total) -> truthy stops early."""
        n_rows, width = shard_shape(params)
        dt = np.float64 if params.out_format == RT_OUT_F64 else np.float32
        out = np.empty((n_rows, width, 3), dtype=dt)
        params.out_on_device = 0
        cb = PROGRESS_FN(lambda _u, done, total: int(bool(progress(done, total)))) if progress else PROGRESS_FN()
        _check(self.lib.rt_render_progressive(self.h, ctypes.byref(camera), ctypes.byref(params), batch_spp, cb,
                                              None, out.ctypes.data), "rt_render_progressive")
        return out

    def render_adaptive(self, camera: Camera, params: RenderParams, min_spp: int, step_spp: int, threshold: float):
        """rt_render_adaptive: the frame in passes, 8x8 tiles stopping once their noise estimate
        E_t <= threshold (or at params.spp). Returns (mean height x width x 3, tile_spp and
        tile_error per raster tile as (tiles_y, tiles_x) arrays, stderr_map height x width)."""
        W, H = params.width, params.height
        ty, tx = (H + 7) // 8, (W + 7) // 8
        dt = np.float64 if params.out_format == RT_OUT_F64 else np.float32
        mean = np.empty((H, W, 3), dtype=dt)
        tile_spp = np.zeros((ty, tx), dtype=np.uint32)
        tile_error = np.zeros((ty, tx), dtype=np.float64)
        se = np.empty((H, W), dtype=np.float64)
        params.out_on_device = 0
        ap = AdaptiveParams(int(min_spp), int(step_spp), float(threshold))
        out = AdaptiveOut(mean.ctypes.data, tile_spp.ctypes.data, tile_error.ctypes.data, se.ctypes.data)
        _check(self.lib.rt_render_adaptive(self.h, ctypes.byref(camera), ctypes.byref(params), ctypes.byref(ap),
                                           ctypes.byref(out)), "rt_render_adaptive")
        return mean, tile_spp, tile_error, se

    def render_adaptive_device(self, camera: Camera, params: RenderParams, min_spp: int, step_spp: int,
                               threshold: float, mean_ptr: int, stderr_ptr: int = 0, tile_spp_ptr: int = 0,
                               tile_error_ptr: int = 0, stream: Optional[int] = None):
        """rt_render_adaptive into device buffers (e.g. torch tensors' data_ptr()): mean height x
        width x 3 of params.out_format, the optional others as rt_adaptive_out. The call itself is
        synchronous."""
        params.out_on_device = 1
        params.stream = stream
        ap = AdaptiveParams(int(min_spp), int(step_spp), float(threshold))
        out = AdaptiveOut(mean_ptr, tile_spp_ptr or None, tile_error_ptr or None, stderr_ptr or None)
        _check(self.lib.rt_render_adaptive(self.h, ctypes.byref(camera), ctypes.byref(params), ctypes.byref(ap),
                                           ctypes.byref(out)), "rt_render_adaptive")

    def render_adaptive_halves(self, camera: Camera, params: RenderParams, min_spp: int, step_spp: int,
                               threshold: float):
        """rt_render_adaptive_halves: render_adaptive's (mean, tile_spp, tile_error, stderr_map), bit
        for bit, and after them the means of every pixel's even and of its odd samples (mean_a,
        mean_b: height x width x 3 of the frame's format), rt_denoise_cross's input."""
        W, H = params.width, params.height
        ty, tx = (H + 7) // 8, (W + 7) // 8
        dt = np.float64 if params.out_format == RT_OUT_F64 else np.float32
        mean, mean_a, mean_b = (np.empty((H, W, 3), dtype=dt) for _ in range(3))
        tile_spp = np.zeros((ty, tx), dtype=np.uint32)
        tile_error = np.zeros((ty, tx), dtype=np.float64)
        se = np.empty((H, W), dtype=np.float64)
        params.out_on_device = 0
        ap = AdaptiveParams(int(min_spp), int(step_spp), float(threshold))
        out = AdaptiveOut(mean.ctypes.data, tile_spp.ctypes.data, tile_error.ctypes.data, se.ctypes.data)
        hv = AdaptiveHalves(mean_a.ctypes.data, mean_b.ctypes.data)
        _check(self.lib.rt_render_adaptive_halves(self.h, ctypes.byref(camera), ctypes.byref(params), ctypes.byref(ap),
                                                  ctypes.byref(out), ctypes.byref(hv)), "rt_render_adaptive_halves")
        return mean, tile_spp, tile_error, se, mean_a, mean_b

    def render_adaptive_halves_device(self, camera: Camera, params: RenderParams, min_spp: int, step_spp: int,
                                      threshold: float, mean_ptr: int, mean_a_ptr: int, mean_b_ptr: int,
                                      stderr_ptr: int = 0, tile_spp_ptr: int = 0, tile_error_ptr: int = 0,
                                      stream: Optional[int] = None):
        """rt_render_adaptive_halves into device buffers: as render_adaptive_device, with the two half
        means (height x width x 3 of params.out_format each). The call itself is synchronous."""
        params.out_on_device = 1
        params.stream = stream
        ap = AdaptiveParams(int(min_spp), int(step_spp), float(threshold))
        out = AdaptiveOut(mean_ptr, tile_spp_ptr or None, tile_error_ptr or None, stderr_ptr or None)
        hv = AdaptiveHalves(mean_a_ptr or None, mean_b_ptr or None)
        _check(self.lib.rt_render_adaptive_halves(self.h, ctypes.byref(camera), ctypes.byref(params), ctypes.byref(ap),
                                                  ctypes.byref(out), ctypes.byref(hv)), "rt_render_adaptive_halves")

    def denoise(self, mean, se, radius: int = 10, patch: int = 3, k: float = 0.45) -> np.ndarray:
        """rt_denoise on host arrays (synchronous): mean height x width x 3 f32 or f64, se height x
        width, as render_adaptive returns them. Returns the filtered frame in mean's format."""
        p, m, s = _denoise_args(mean, se, radius, patch, k)
        out = np.empty_like(m)
        _check(self.lib.rt_denoise(self.h, ctypes.byref(p), m.ctypes.data, s.ctypes.data, out.ctypes.data),
               "rt_denoise")
        return out

    def denoise_device(self, mean_ptr: int, stderr_ptr: int, out_ptr: int, width: int, height: int,
                       out_format: int = RT_OUT_F32, radius: int = 10, patch: int = 3, k: float = 0.45,
                       stream: Optional[int] = None):
        """Enqueues rt_denoise over device buffers (mean and out height x width x 3 of out_format,
        the error map height x width f64) on `stream`."""
        p = DenoiseParams(int(width), int(height), int(out_format), 1, int(radius), int(patch), float(k), stream)
        _check(self.lib.rt_denoise(self.h, ctypes.byref(p), ctypes.c_void_p(mean_ptr), ctypes.c_void_p(stderr_ptr),
                                   ctypes.c_void_p(out_ptr)), "rt_denoise")

    def denoise_guided(self, mean, se, albedo=None, normal=None, depth=None, sigmas=GUIDE_SIGMAS, radius: int = 10,
                       patch: int = 3, k: float = 0.45) -> np.ndarray:
        """rt_denoise_guided on host arrays (synchronous): denoise with the feature buffers of
        render_features in its weights; None leaves a guide out; sigmas = (albedo, normal, depth)."""
        p, m, s = _denoise_args(mean, se, radius, patch, k)
        g, keep = _guide_args(m.shape[:2], albedo, normal, depth, sigmas)
        out = np.empty_like(m)
        _check(self.lib.rt_denoise_guided(self.h, ctypes.byref(p), m.ctypes.data, s.ctypes.data, ctypes.byref(g),
                                          out.ctypes.data), "rt_denoise_guided")
        del keep
        return out

    def denoise_guided_device(self, mean_ptr: int, stderr_ptr: int, out_ptr: int, width: int, height: int,
                              albedo_ptr: int = 0, normal_ptr: int = 0, depth_ptr: int = 0, sigmas=GUIDE_SIGMAS,
                              out_format: int = RT_OUT_F32, radius: int = 10, patch: int = 3, k: float = 0.45,
                              stream: Optional[int] = None):
        """Enqueues rt_denoise_guided over device buffers on `stream`: as denoise_device, with the
        guide frames (f64; 0 leaves one out) render_features_device wrote."""
        p = DenoiseParams(int(width), int(height), int(out_format), 1, int(radius), int(patch), float(k), stream)
        g = _guides(albedo_ptr, normal_ptr, depth_ptr, sigmas)
        _check(self.lib.rt_denoise_guided(self.h, ctypes.byref(p), ctypes.c_void_p(mean_ptr),
                                          ctypes.c_void_p(stderr_ptr), ctypes.byref(g), ctypes.c_void_p(out_ptr)),
               "rt_denoise_guided")

    def denoise_atrous(self, mean, se, albedo=None, normal=None, depth=None, sigmas=GUIDE_SIGMAS,
                       levels: int = ATROUS_LEVELS, sigma_l: float = ATROUS_SIGMA_L, demodulate: bool = False,
                       want_stderr: bool = True):
        """rt_denoise_atrous on host arrays (synchronous): the a-trous wavelet filter with the feature
        buffers of render_features as edge stops (None leaves one out); demodulate filters colour /
        albedo. Returns (the filtered frame, the standard error left in it or None)."""
        p, m, s = _atrous_args(mean, se, levels, sigma_l, demodulate)
        g, keep = _guide_args(m.shape[:2], albedo, normal, depth, sigmas)
        out = np.empty_like(m)
        se_out = np.empty_like(s) if want_stderr else None
        _check(self.lib.rt_denoise_atrous(self.h, ctypes.byref(p), m.ctypes.data, s.ctypes.data, ctypes.byref(g),
                                          out.ctypes.data, se_out.ctypes.data if want_stderr else None),
               "rt_denoise_atrous")
        del keep
        return out, se_out

    def denoise_atrous_device(self, mean_ptr: int, stderr_ptr: int, out_ptr: int, width: int, height: int,
                              albedo_ptr: int = 0, normal_ptr: int = 0, depth_ptr: int = 0, sigmas=GUIDE_SIGMAS,
                              out_format: int = RT_OUT_F32, levels: int = ATROUS_LEVELS,
                              sigma_l: float = ATROUS_SIGMA_L, demodulate: bool = False, stderr_out_ptr: int = 0,
                              stream: Optional[int] = None):
        """Enqueues rt_denoise_atrous over device buffers on `stream`: as denoise_guided_device;
        stderr_out_ptr (height x width f64; 0 leaves it out) receives the standard error left."""
        p = AtrousParams(int(width), int(height), int(out_format), 1, int(levels), int(demodulate), float(sigma_l),
                         stream)
        g = _guides(albedo_ptr, normal_ptr, depth_ptr, sigmas)
        _check(self.lib.rt_denoise_atrous(self.h, ctypes.byref(p), ctypes.c_void_p(mean_ptr),
                                          ctypes.c_void_p(stderr_ptr), ctypes.byref(g), ctypes.c_void_p(out_ptr),
                                          ctypes.c_void_p(stderr_out_ptr or None)), "rt_denoise_atrous")

    def atrous_stats(self) -> AtrousStats:
        return _stats(self, "rt_atrous_last_stats", AtrousStats)

    def denoise_pyramid(self, mean, se, albedo=None, normal=None, depth=None, sigmas=GUIDE_SIGMAS,
                        radius: int = PYRAMID_WINDOW[0], patch: int = PYRAMID_WINDOW[1], k: float = PYRAMID_WINDOW[2],
                        levels: int = PYRAMID_LEVELS) -> np.ndarray:
        """rt_denoise_pyramid on host arrays (synchronous): denoise_guided run at `levels` scales of the
        frame; arguments and result as the module's denoise_pyramid_host."""
        p, m, s = _pyramid_args(mean, se, radius, patch, k, levels)
        g, keep = _guide_args(m.shape[:2], albedo, normal, depth, sigmas)
        out = np.empty_like(m)
        _check(self.lib.rt_denoise_pyramid(self.h, ctypes.byref(p), m.ctypes.data, s.ctypes.data, ctypes.byref(g),
                                           out.ctypes.data), "rt_denoise_pyramid")
        del keep
        return out

    def denoise_pyramid_device(self, mean_ptr: int, stderr_ptr: int, out_ptr: int, width: int, height: int,
                               albedo_ptr: int = 0, normal_ptr: int = 0, depth_ptr: int = 0, sigmas=GUIDE_SIGMAS,
                               out_format: int = RT_OUT_F32, radius: int = PYRAMID_WINDOW[0],
                               patch: int = PYRAMID_WINDOW[1], k: float = PYRAMID_WINDOW[2],
                               levels: int = PYRAMID_LEVELS, stream: Optional[int] = None):
        """Enqueues rt_denoise_pyramid over device buffers on `stream`: as denoise_guided_device."""
        p = PyramidParams(int(width), int(height), int(out_format), 1, int(radius), int(patch), float(k), int(levels),
                          0, stream)
        g = _guides(albedo_ptr, normal_ptr, depth_ptr, sigmas)
        _check(self.lib.rt_denoise_pyramid(self.h, ctypes.byref(p), ctypes.c_void_p(mean_ptr),
                                           ctypes.c_void_p(stderr_ptr), ctypes.byref(g), ctypes.c_void_p(out_ptr)),
               "rt_denoise_pyramid")

    def pyramid_stats(self) -> PyramidStats:
        return _stats(self, "rt_pyramid_last_stats", PyramidStats)

    def denoise_cross(self, mean_a, mean_b, se, albedo=None, normal=None, depth=None, sigmas=GUIDE_SIGMAS,
                      radius: int = 10, patch: int = 3, k: float = 0.45,
                      variance_scale: float = CROSS_VARIANCE_SCALE, want_stderr: bool = True):
        """rt_denoise_cross on host arrays (synchronous): NL-means over two half frames, each filtered
        with the other's weights; arguments and result as the module's denoise_cross_host."""
        p, a, b, s = _cross_args(mean_a, mean_b, se, radius, patch, k, variance_scale)
        g, keep = _guide_args(a.shape[:2], albedo, normal, depth, sigmas)
        out = np.empty_like(a)
        se_out = np.empty_like(s) if want_stderr else None
        _check(self.lib.rt_denoise_cross(self.h, ctypes.byref(p), a.ctypes.data, b.ctypes.data, s.ctypes.data,
                                         ctypes.byref(g), out.ctypes.data, se_out.ctypes.data if want_stderr else None),
               "rt_denoise_cross")
        del keep
        return out, se_out

    def denoise_cross_device(self, mean_a_ptr: int, mean_b_ptr: int, stderr_ptr: int, out_ptr: int, width: int,
                             height: int, albedo_ptr: int = 0, normal_ptr: int = 0, depth_ptr: int = 0,
                             sigmas=GUIDE_SIGMAS, out_format: int = RT_OUT_F32, radius: int = 10, patch: int = 3,
                             k: float = 0.45, variance_scale: float = CROSS_VARIANCE_SCALE, stderr_out_ptr: int = 0,
                             stream: Optional[int] = None):
        """Enqueues rt_denoise_cross over device buffers on `stream`: as denoise_guided_device, with
        the two half means; stderr_out_ptr (height x width f64; 0 leaves it out) receives the error
        map."""
        p = CrossParams(int(width), int(height), int(out_format), 1, int(radius), int(patch), float(k),
                        float(variance_scale), stream)
        g = _guides(albedo_ptr, normal_ptr, depth_ptr, sigmas)
        _check(self.lib.rt_denoise_cross(self.h, ctypes.byref(p), ctypes.c_void_p(mean_a_ptr),
                                         ctypes.c_void_p(mean_b_ptr), ctypes.c_void_p(stderr_ptr), ctypes.byref(g),
                                         ctypes.c_void_p(out_ptr), ctypes.c_void_p(stderr_out_ptr or None)),
               "rt_denoise_cross")

    def cross_stats(self) -> CrossStats:
        return _stats(self, "rt_cross_last_stats", CrossStats)

    def render_features(self, camera: Camera, params: RenderParams, albedo: bool = True, normal: bool = True,
                        depth: bool = True):
        """rt_render_features: the first hit's (albedo height x width x 3, normal height x width x 3,
        depth height x width), f64 means over params.spp samples of rt_render's primary rays; a
        buffer switched off comes back as None."""
        W, H = params.width, params.height
        a = np.empty((H, W, 3), dtype=np.float64) if albedo else None
        n = np.empty((H, W, 3), dtype=np.float64) if normal else None
        d = np.empty((H, W), dtype=np.float64) if depth else None
        params.out_on_device = 0
        out = FeaturesOut(*(x.ctypes.data if x is not None else None for x in (a, n, d)))
        _check(self.lib.rt_render_features(self.h, ctypes.byref(camera), ctypes.byref(params), ctypes.byref(out)),
               "rt_render_features")
        return a, n, d

    def render_features_device(self, camera: Camera, params: RenderParams, albedo_ptr: int = 0, normal_ptr: int = 0,
                               depth_ptr: int = 0, stream: Optional[int] = None):
        """Enqueues rt_render_features into device buffers (f64; 0 leaves one out) on `stream`."""
        params.out_on_device = 1
        params.stream = stream
        out = FeaturesOut(albedo_ptr or None, normal_ptr or None, depth_ptr or None)
        _check(self.lib.rt_render_features(self.h, ctypes.byref(camera), ctypes.byref(params), ctypes.byref(out)),
               "rt_render_features")

    def features_stats(self) -> FeaturesStats:
        return _stats(self, "rt_features_last_stats", FeaturesStats)

    def trace_rays(self, rays, mode: int = RT_QUERY_CLOSEST, seed: int = 1, bounce: int = 0, albedo: bool = False):
        """rt_trace_rays on host arrays. rays: RAY records. CLOSEST: the HIT records, or (albedo) the
        pair (HIT records, albedo n x 3); ANY: the occluded bytes as a bool array."""
        rays = np.ascontiguousarray(rays, dtype=RAY)
        n = rays.shape[0]
        p = QueryParams(n=n, mode=mode, on_device=0, seed=seed, bounce=bounce)
        if mode == RT_QUERY_ANY:
            occ = np.zeros(n, dtype=np.uint8)
            out = QueryOut(None, None, occ.ctypes.data)
        else:
            hits = np.zeros(n, dtype=HIT)
            alb = np.zeros((n, 3), dtype=np.float64) if albedo else None
            out = QueryOut(hits.ctypes.data, alb.ctypes.data if albedo else None, None)
        _check(self.lib.rt_trace_rays(self.h, ctypes.byref(p), rays.ctypes.data, ctypes.byref(out)), "rt_trace_rays")
        if mode == RT_QUERY_ANY:
            return occ.astype(bool)
        return (hits, alb) if albedo else hits

    def trace_rays_device(self, rays_ptr: int, n: int, mode: int = RT_QUERY_CLOSEST, hits_ptr: int = 0, albedo_ptr: int = 0,
                          occluded_ptr: int = 0, seed: int = 1, bounce: int = 0, origin_bound: float = 0.0,
                          stream: Optional[int] = None):
        """Enqueues rt_trace_rays on device arrays (RAY / HIT records 16-byte aligned; 0 leaves an
        output out) on `stream`. origin_bound: the caller's bound on |origin| components (0: unknown)."""
        p = QueryParams(n=n, mode=mode, on_device=1, seed=seed, bounce=bounce, origin_bound=origin_bound, stream=stream)
        out = QueryOut(hits_ptr or None, albedo_ptr or None, occluded_ptr or None)
        _check(self.lib.rt_trace_rays(self.h, ctypes.byref(p), rays_ptr, ctypes.byref(out)), "rt_trace_rays")

    def query_stats(self) -> QueryStats:
        return _stats(self, "rt_query_last_stats", QueryStats)

    def denoise_stats(self) -> DenoiseStats:
        return _stats(self, "rt_denoise_last_stats", DenoiseStats)

    def adaptive_stats(self) -> AdaptiveStats:
        return _stats(self, "rt_adaptive_last_stats", AdaptiveStats)

    def adaptive_state(self, camera: Camera, params: RenderParams, min_spp: int, step_spp: int,
                       halves: bool = False) -> "AdaptiveState":
        """rt_adaptive_state_create: render_adaptive's accumulators kept between calls (rt_abi.h)."""
        return AdaptiveState(self, camera, params, min_spp, step_spp, halves)

    def accumulator(self, params: RenderParams) -> "Accumulator":
        return Accumulator(self, params)

    def set_schedule(self, schedule: int):
        _check(self.lib.rt_ctx_set_schedule(self.h, schedule), "rt_ctx_set_schedule")

    def set_precision(self, precision: int):
        """RT_PREC_F64 (default: path-identical to the oracle, last-ulp summation differences) or
        RT_PREC_F32 (fast mode, statistical parity)."""
        _check(self.lib.rt_ctx_set_precision(self.h, precision), "rt_ctx_set_precision")

    def set_option(self, key: int, value: int):
        """rt_ctx_set_option (RT_OPT_*): buffer bound, batch overlap, block sizes, extra features, ..."""
        _check(self.lib.rt_ctx_set_option(self.h, key, int(value)), "rt_ctx_set_option")

    def get_option(self, key: int) -> int:
        v = ctypes.c_int64()
        _check(self.lib.rt_ctx_get_option(self.h, key, ctypes.byref(v)), "rt_ctx_get_option")
        return v.value

    def set_variant(self, slab32: int = 1, lds_stack: int = 1, lds_nodes: int = 1):
        _check(self.lib.rt_ctx_set_variant(self.h, slab32, lds_stack, lds_nodes), "rt_ctx_set_variant")

    def counters(self, n: int = 32) -> np.ndarray:
        """The last count_work render's raw counters (rt_last_counters: phase wave-cycles etc.)."""
        out = np.zeros(n, dtype=np.uint64)
        rc = self.lib.rt_last_counters(self.h, out.ctypes.data, n)
        if rc < 0:
            _check(rc, "rt_last_counters")
        return out[:rc]

    def tile_costs(self) -> np.ndarray:
        """Lane-cycles per raster 8x8 tile of the last count_work render on a pool schedule
        (rt_last_tile_costs); empty if it counted none."""
        n = self.lib.rt_last_tile_costs(self.h, None, 0)
        if n < 0:
            _check(n, "rt_last_tile_costs")
        out = np.zeros(n, dtype=np.uint64)
        if n:
            _check(min(0, self.lib.rt_last_tile_costs(self.h, out.ctypes.data, n)), "rt_last_tile_costs")
        return out

    def deal_order(self) -> np.ndarray:
        """The cost order the last render's work blocks were dealt in (rt_last_deal_order,
        RT_OPT_AUTO_DEAL_ORDER): position -> raster tile; empty if it was dealt in raster order."""
        n = self.lib.rt_last_deal_order(self.h, None, 0)
        if n < 0:
            _check(n, "rt_last_deal_order")
        out = np.zeros(n, dtype=np.uint32)
        if n:
            _check(min(0, self.lib.rt_last_deal_order(self.h, out.ctypes.data, n)), "rt_last_deal_order")
        return out

    def set_tile_order(self, order=None):
        """rt_ctx_set_tile_order: tile shards take the frame's tiles in this order (a permutation
        of its raster tiles, e.g. cost_tile_order(tile_costs())); None: raster order."""
        if order is None:
            _check(self.lib.rt_ctx_set_tile_order(self.h, None, 0), "rt_ctx_set_tile_order")
            return
        o = np.ascontiguousarray(np.asarray(order), dtype=np.uint32)
        _check(self.lib.rt_ctx_set_tile_order(self.h, o.ctypes.data, len(o)), "rt_ctx_set_tile_order")

    def stats(self) -> Stats:
        return _stats(self, "rt_last_stats", Stats)

    def assemble_device(self, slabs_ptr: int, slab_elems: int, world: int, params: RenderParams, frame_ptr: int,
                        stream: Optional[int] = None):
        """rt_tiles_assemble: gathered tile slabs (device) -> frame (device), in this context's tile order."""
        params.stream = stream
        _check(self.lib.rt_tiles_assemble(self.h, ctypes.c_void_p(slabs_ptr), slab_elems, world, ctypes.byref(params),
                                          ctypes.c_void_p(frame_ptr)), "rt_tiles_assemble")

    def device_eval(self, fn: int, x, y=None, z=None) -> np.ndarray:
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.ascontiguousarray(x if y is None else y, dtype=np.float64)
        z = np.ascontiguousarray(x if z is None else z, dtype=np.float64)
        out = np.empty_like(x)
        _check(self.lib.rt_device_eval(self.h, fn, x.ctypes.data, y.ctypes.data, z.ctypes.data, out.ctypes.data,
                                       x.size), "rt_device_eval")
        return out


class Comm:
    """One rank of a multi-GPU render (rt_comm_*): binds a Renderer (its device) to rank `rank` of
    `world`. One process per GPU: rank 0 makes the id (Comm.unique_id()) and sends it to the others
    (any channel), every rank then builds Comm(renderer, rank, world, uid). One process over several
    GPUs: Comm.init_all(renderers)."""

    def __init__(self, renderer: Renderer, rank: int, world: int, uid: bytes, _handle=None):
        self.r, self.lib = renderer, renderer.lib
        self.rank, self.world = rank, world
        if _handle is not None:
            self.h = _handle
            return
        if len(uid) != RT_COMM_ID_BYTES:
            raise RTError("unique id must be %d bytes" % RT_COMM_ID_BYTES)
        h = ctypes.c_void_p()
        buf = (ctypes.c_uint8 * RT_COMM_ID_BYTES).from_buffer_copy(uid)
        _check(self.lib.rt_comm_init_rank(renderer.h, rank, world, buf, ctypes.byref(h)), "rt_comm_init_rank")
        self.h = h

    @staticmethod
    def unique_id() -> bytes:
        buf = (ctypes.c_uint8 * RT_COMM_ID_BYTES)()
        _check(load_library().rt_comm_unique_id(buf), "rt_comm_unique_id")
        return bytes(buf)

    @staticmethod
    def init_all(renderers) -> list:
        n = len(renderers)
        ctxs = (ctypes.c_void_p * n)(*[r.h.value if isinstance(r.h, ctypes.c_void_p) else r.h for r in renderers])
        hs = (ctypes.c_void_p * n)()
        _check(load_library().rt_comm_init_all(ctxs, n, hs), "rt_comm_init_all")
        return [Comm(r, i, n, b"", _handle=ctypes.c_void_p(hs[i])) for i, r in enumerate(renderers)]

    def close(self):
        if self.h:
            self.lib.rt_comm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def tile_order(self, camera: Camera, params: RenderParams, cost_spp: int = 8):
        """Collective rt_comm_tile_order: every rank counts its raster shard, one all-reduce, the
        cost order set on every rank's context."""
        params.stream = params.stream if params.stream else None
        _check(self.lib.rt_comm_tile_order(self.h, ctypes.byref(camera), ctypes.byref(params), cost_spp),
               "rt_comm_tile_order")

    def render_gather(self, camera: Camera, params: RenderParams, out=None):
        """Collective rt_render_gather into host memory: rank 0 returns the height x width x 3 frame
        (or fills `out`), the other ranks None."""
        params.out_on_device = 0
        if self.rank != 0:
            _check(self.lib.rt_render_gather(self.h, ctypes.byref(camera), ctypes.byref(params), None),
                   "rt_render_gather")
            return None
        dt = np.float64 if params.out_format == RT_OUT_F64 else np.float32
        if out is None:
            out = np.empty((params.height, params.width, 3), dtype=dt)
        if out.dtype != dt or out.size != params.height * params.width * 3 or not out.flags.c_contiguous:
            raise RTError("frame buffer of the wrong shape or type")
        _check(self.lib.rt_render_gather(self.h, ctypes.byref(camera), ctypes.byref(params), out.ctypes.data),
               "rt_render_gather")
        return out

    def render_gather_device(self, camera: Camera, params: RenderParams, dev_ptr: Optional[int],
                             stream: Optional[int] = None):
        """Collective rt_render_gather, enqueued on `stream`: rank 0's frame into a device buffer."""
        params.out_on_device = 1
        params.stream = stream
        _check(self.lib.rt_render_gather(self.h, ctypes.byref(camera), ctypes.byref(params),
                                         ctypes.c_void_p(dev_ptr) if dev_ptr else None), "rt_render_gather")

    def stats(self) -> CommStats:
        return _stats(self, "rt_comm_last_stats", CommStats)


def _comm_array(comms):
    return (ctypes.c_void_p * len(comms))(*[c.h.value for c in comms])


def tile_order_all(comms, camera: Camera, params: RenderParams, cost_spp: int = 8):
    """rt_comm_tile_order_all over the ranks of one process (Comm.init_all)."""
    params.stream = None
    _check(load_library().rt_comm_tile_order_all(_comm_array(comms), len(comms), ctypes.byref(camera),
                                                 ctypes.byref(params), cost_spp), "rt_comm_tile_order_all")


def render_gather_all(comms, camera: Camera, params: RenderParams, out=None) -> np.ndarray:
    """rt_render_gather_all over the ranks of one process: the frame in host memory (or `out`)."""
    params.out_on_device = 0
    params.stream = None
    dt = np.float64 if params.out_format == RT_OUT_F64 else np.float32
    if out is None:
        out = np.empty((params.height, params.width, 3), dtype=dt)
    if out.dtype != dt or out.size != params.height * params.width * 3 or not out.flags.c_contiguous:
        raise RTError("frame buffer of the wrong shape or type")
    _check(load_library().rt_render_gather_all(_comm_array(comms), len(comms), ctypes.byref(camera),
                                               ctypes.byref(params), out.ctypes.data), "rt_render_gather_all")
    return out


def render_gather_all_device(comms, camera: Camera, params: RenderParams, dev_ptr: int):
    """rt_render_gather_all, enqueued on each context's stream: rank 0's frame into a device buffer."""
    params.out_on_device = 1
    params.stream = None
    _check(load_library().rt_render_gather_all(_comm_array(comms), len(comms), ctypes.byref(camera),
                                               ctypes.byref(params), ctypes.c_void_p(dev_ptr)), "rt_render_gather_all")


class Accumulator:
    """Progressive / resumable accumulation over one row shard (rt_accum_*)."""

    def __init__(self, renderer: Renderer, params: RenderParams):
        self.r, self.lib = renderer, renderer.lib
        self.rows, self.width = shard_shape(params)
        h = ctypes.c_void_p()
        _check(self.lib.rt_accum_create(renderer.h, ctypes.byref(params), ctypes.byref(h)), "rt_accum_create")
        self.h = h

    def close(self):
        if self.h:
            self.lib.rt_accum_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add(self, camera: Camera, params: RenderParams, sample_count: int):
        _check(self.lib.rt_accum_add(self.r.h, self.h, ctypes.byref(camera), ctypes.byref(params), sample_count),
               "rt_accum_add")

    @property
    def samples_done(self) -> int:
        n = ctypes.c_int64()
        _check(self.lib.rt_accum_get(self.h, None, ctypes.byref(n)), "rt_accum_get")
        return n.value

    def checkpoint(self):
        """(sums rows x width x 3 f64, samples done) — what rt_accum_set restores."""
        sums = np.empty((self.rows, self.width, 3), dtype=np.float64)
        n = ctypes.c_int64()
        _check(self.lib.rt_accum_get(self.h, sums.ctypes.data, ctypes.byref(n)), "rt_accum_get")
        return sums, n.value

    def restore(self, sums: np.ndarray, samples_done: int):
        sums = np.ascontiguousarray(sums, dtype=np.float64)
        assert sums.shape == (self.rows, self.width, 3)
        _check(self.lib.rt_accum_set(self.h, sums.ctypes.data, samples_done), "rt_accum_set")

    def resolve(self, divisor: float = 0.0, out_format: int = RT_OUT_F32) -> np.ndarray:
        dt = np.float64 if out_format == RT_OUT_F64 else np.float32
        out = np.empty((self.rows, self.width, 3), dtype=dt)
        _check(self.lib.rt_accum_resolve(self.r.h, self.h, divisor, out_format, 0, out.ctypes.data),
               "rt_accum_resolve")
        return out


class AdaptiveState:
    """A resumable, refinable adaptive frame (rt_adaptive_state_*, rt_abi.h): advance it to a
    threshold and a cap, resolve it between any two advances, checkpoint and restore it, or steer
    one round by a per-tile error map. Close it before its renderer."""

    def __init__(self, renderer: Renderer, camera: Camera, params: RenderParams, min_spp: int, step_spp: int,
                 halves: bool = False):
        self.r, self.lib = renderer, renderer.lib
        self.width, self.height, self.halves = params.width, params.height, bool(halves)
        self.tiles_y, self.tiles_x = (self.height + 7) // 8, (self.width + 7) // 8
        ap = AdaptiveParams(int(min_spp), int(step_spp), 0.0)
        h = ctypes.c_void_p()
        _check(self.lib.rt_adaptive_state_create(renderer.h, ctypes.byref(camera), ctypes.byref(params),
                                                 ctypes.byref(ap), int(self.halves), ctypes.byref(h)),
               "rt_adaptive_state_create")
        self.h = h

    def close(self):
        if self.h:
            if self.r.h:   # (a state outlived by its context is not touched: rt_abi.h's lifetime rule)
                self.lib.rt_adaptive_state_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def advance(self, threshold: float, spp_cap: int, max_launches: int = 0, tile_error=None,
                tile_error_ptr: int = 0, stream: Optional[int] = None) -> int:
        """rt_adaptive_state_advance. tile_error: a caller's error map on the host, one value per
        raster tile; tile_error_ptr: the same as a device pointer. Returns the active tiles left."""
        ap = AdaptiveAdvanceParams()
        ap.threshold, ap.spp_cap, ap.max_launches = float(threshold), int(spp_cap), int(max_launches)
        ap.stream = stream
        err = None
        if tile_error is not None:
            err = np.ascontiguousarray(tile_error, dtype=np.float64).reshape(-1)
            if err.size != self.tiles_x * self.tiles_y:
                raise RTError(f"advance: {err.size} errors for {self.tiles_x * self.tiles_y} tiles")
            ap.tile_error_in = err.ctypes.data
        elif tile_error_ptr:
            ap.tile_error_in, ap.error_on_device = tile_error_ptr, 1
        left = ctypes.c_int32()
        _check(self.lib.rt_adaptive_state_advance(self.h, ctypes.byref(ap), ctypes.byref(left)),
               "rt_adaptive_state_advance")
        return left.value

    def resolve(self, out_format: int = RT_OUT_F32):
        """rt_adaptive_state_resolve to the host: render_adaptive's (mean, tile_spp, tile_error,
        stderr_map), and with halves render_adaptive_halves' (..., mean_a, mean_b)."""
        W, H = self.width, self.height
        dt = np.float64 if out_format == RT_OUT_F64 else np.float32
        mean = np.empty((H, W, 3), dtype=dt)
        tile_spp = np.zeros((self.tiles_y, self.tiles_x), dtype=np.uint32)
        tile_error = np.zeros((self.tiles_y, self.tiles_x), dtype=np.float64)
        se = np.empty((H, W), dtype=np.float64)
        out = AdaptiveOut(mean.ctypes.data, tile_spp.ctypes.data, tile_error.ctypes.data, se.ctypes.data)
        if not self.halves:
            _check(self.lib.rt_adaptive_state_resolve(self.h, out_format, 0, ctypes.byref(out), None),
                   "rt_adaptive_state_resolve")
            return mean, tile_spp, tile_error, se
        mean_a, mean_b = np.empty((H, W, 3), dtype=dt), np.empty((H, W, 3), dtype=dt)
        hv = AdaptiveHalves(mean_a.ctypes.data, mean_b.ctypes.data)
        _check(self.lib.rt_adaptive_state_resolve(self.h, out_format, 0, ctypes.byref(out), ctypes.byref(hv)),
               "rt_adaptive_state_resolve")
        return mean, tile_spp, tile_error, se, mean_a, mean_b

    def resolve_device(self, out_format: int, mean_ptr: int, stderr_ptr: int = 0, tile_spp_ptr: int = 0,
                       tile_error_ptr: int = 0, mean_a_ptr: int = 0, mean_b_ptr: int = 0):
        """rt_adaptive_state_resolve into device buffers (e.g. torch tensors' data_ptr()); the half
        means when either of their pointers is given. The call itself is synchronous."""
        out = AdaptiveOut(mean_ptr, tile_spp_ptr or None, tile_error_ptr or None, stderr_ptr or None)
        hv = AdaptiveHalves(mean_a_ptr or None, mean_b_ptr or None) if (mean_a_ptr or mean_b_ptr) else None
        _check(self.lib.rt_adaptive_state_resolve(self.h, out_format, 1, ctypes.byref(out),
                                                  ctypes.byref(hv) if hv is not None else None),
               "rt_adaptive_state_resolve")

    def checkpoint(self):
        """(header, arrays): rt_adaptive_state_get's header and a dict of S, Q, tile_spp, tile_error
        (and S_a, S_b with halves) — what restore takes."""
        W, H = self.width, self.height
        arrays = dict(sums=np.empty((H, W, 3)), q=np.empty((H, W)),
                      tile_spp=np.empty((self.tiles_y, self.tiles_x), dtype=np.uint32),
                      tile_error=np.empty((self.tiles_y, self.tiles_x)))
        if self.halves:
            arrays.update(sum_a=np.empty((H, W, 3)), sum_b=np.empty((H, W, 3)))
        hdr = AdaptiveStateHeader()
        data = AdaptiveStateData(**{k: v.ctypes.data for k, v in arrays.items()})
        _check(self.lib.rt_adaptive_state_get(self.h, ctypes.byref(hdr), ctypes.byref(data)), "rt_adaptive_state_get")
        return hdr, arrays

    def restore(self, header: AdaptiveStateHeader, arrays: dict):
        W, H = self.width, self.height
        shapes = dict(sums=(H, W, 3), q=(H, W), tile_spp=(self.tiles_y, self.tiles_x),
                      tile_error=(self.tiles_y, self.tiles_x))
        if self.halves:
            shapes.update(sum_a=(H, W, 3), sum_b=(H, W, 3))
        keep = {}
        for k, shape in shapes.items():
            if k not in arrays:
                raise RTError(f"restore: no {k}")
            keep[k] = np.ascontiguousarray(arrays[k], dtype=np.uint32 if k == "tile_spp" else np.float64)
            if keep[k].shape != shape:
                raise RTError(f"restore: {k} is {keep[k].shape}, the state's is {shape}")
        data = AdaptiveStateData(**{k: v.ctypes.data for k, v in keep.items()})
        _check(self.lib.rt_adaptive_state_set(self.h, ctypes.byref(header), ctypes.byref(data)), "rt_adaptive_state_set")

    def stats(self) -> AdaptiveStateStats:
        return _stats(self, "rt_adaptive_state_last_stats", AdaptiveStateStats)


def render_scene(scene_id: int, width: int, height: int, spp: int, max_depth: int = 50, scene_seed: int = 1,
                 render_seed: int = 1, row_begin: int = 0, row_stride: int = 1, out_format: int = RT_OUT_F32,
                 spp_chunk: int = 0, device: int = 0, renderer: Optional[Renderer] = None,
                 image: Optional[np.ndarray] = None, accel: int = RT_ACCEL_SAH):
    """One-call path: build the preset scene, upload, render the row shard. Returns (image, stats)."""
    world = World(scene_seed).build_scene(scene_id, image)
    cam, bg = scene_camera(scene_id, width, height)
    r = renderer or Renderer(device)
    r.upload(world, accel)
    p = Renderer.params(width, height, spp, max_depth, bg, render_seed, row_begin, row_stride, spp_chunk,
                        out_format)
    img = r.render(cam, p)
    return img, r.stats()
