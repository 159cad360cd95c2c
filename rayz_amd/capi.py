"""ctypes view of include/rayz_hip.h — the C ABI of the MI355X render path.

The structures mirror the header field for field; `load()` opens the in-tree
`librayz_hip.so` built by `__graft_entry__.build()` and fails loudly when it is
missing: there is no CPU fallback anywhere in this package.
"""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "csrc", "librayz_hip.so")

ABI_VERSION = 5
MAX_DEVICES = 64
GATHER_RCCL, GATHER_PEER_COPY = 0, 1
GATHER_ALLOW_DUPLICATE_DEVICES = 0x100  # flag bit, peer-copy only (tests on a one-GPU box)
(DEBUG_QUEUE_GRAB, DEBUG_BVH_KEEP, DEBUG_BVH_PEEL, DEBUG_BVH_TOP, DEBUG_BVH_KERNEL, DEBUG_BVH2_KEEP,
 DEBUG_LDS_PAD, DEBUG_BVH_TOP_ORDER, DEBUG_BVH_NODES, DEBUG_BVH_SPLIT, DEBUG_BVHX, DEBUG_CHUNK_CAP,
 DEBUG_DENOISE_LDS_STRIDE) = range(13)
(KAT_REFRACT, KAT_REFLECTANCE, KAT_GET_RAY, KAT_BOX_HIT, KAT_SPHERE_HIT, KAT_SCATTER, KAT_CHECKER, KAT_BACKGROUND,
 KAT_TRIANGLE_HIT, KAT_SCAN_DISCS, KAT_BUCKET_DISCS, KAT_SCAN_DISCS_XY, KAT_BUCKET_DISCS_XY, KAT_SET_DISCS) = range(14)
SCAN_FORM_AUTO, SCAN_FORM_XZ, SCAN_FORM_XY, SCAN_FORM_ONE_RADIUS = 0, 1, 2, 3  # RayzScanForm: the basis of the flat list's reject test
PRIMARY_LISTS_AUTO, PRIMARY_LISTS_OFF, PRIMARY_LISTS_ON = 0, 1, 2  # RayzPrimaryLists: camera segments from per-pixel candidate lists
CELL_LISTS_AUTO, CELL_LISTS_OFF, CELL_LISTS_ON = 0, 1, 2  # RayzCellLists: listable segments from the slab's cells
KAT_IN_STRIDE, KAT_OUT_STRIDE = 48, 12

OK = 0
ERR_BAD_ARG = -1
ERR_HIP = -2
ERR_OOM = -3
ERR_NO_DEVICE = -4
ERR_STATE = -5

TEX_CHECKER, TEX_SOLID = 0, 1
MAT_DIFFUSE, MAT_METALLIC, MAT_DIELECTRIC = 0, 1, 2
DIFFUSE_UNIT_SPHERE, DIFFUSE_UNIT_SPHERE_SURFACE, DIFFUSE_HEMISPHERE = 0, 1, 2
PRECISION_F32, PRECISION_F64 = 0, 1
TRAVERSAL_LINEAR, TRAVERSAL_BVH, TRAVERSAL_AUTO = 0, 1, 2
QUERY_NEAREST, QUERY_ANY = 0, 1
CHAIN_MAX_DEPTH = 16
CHAIN_DEFAULTS = {"max_depth": 4, "max_fuzz": 0.25}  # provisional
DENOISE_ALBEDO = 1
DENOISE_DEFAULTS = {"levels": 5, "normal_power_log2": 6, "flags": DENOISE_ALBEDO, "sigma_color": 0.5, "sigma_plane": 0.25}
DENOISE_GUIDED_DEFAULTS = {"levels": 5, "normal_power_log2": 6, "flags": DENOISE_ALBEDO, "sigma_color": 2.0, "sigma_plane": 0.25,
                           "var_floor": 1e-4}
NOISE_DEFAULTS = {"rel_error": 0.05, "mean_floor": 0.02}
ADAPTIVE_DEFAULT_MIN_CHUNKS = 4
UPSCALE_FORM_AUTO, UPSCALE_FORM_DIRECT = 0, 1
# the denoiser's guide parameters; flags 0: demodulating by the low-resolution albedo measured far worse than not
UPSCALE_DEFAULTS = {"normal_power_log2": 6, "flags": 0, "form": UPSCALE_FORM_AUTO, "sigma_plane": 0.25}
TEMPORAL_DEFAULTS = {"alpha_min": 0.05, "n_max": 65536.0, "normal_cos_min": 0.9, "max_rel_dist": 0.05}  # provisional
TEMPORAL_MOMENTS_DEFAULTS = {"w2_max": 0.25, "min_taps": 4.0}  # provisional
TEMPORAL_RESAMPLE_BILINEAR, TEMPORAL_RESAMPLE_CUBIC = 0, 1  # RAYZ_TEMPORAL_RESAMPLE_* 
TEMPORAL_RESAMPLING = {"bilinear": TEMPORAL_RESAMPLE_BILINEAR, "cubic": TEMPORAL_RESAMPLE_CUBIC}
TEMPORAL_BACKGROUND_INPUT, TEMPORAL_BACKGROUND_ACCUMULATE = 0, 1  # RAYZ_TEMPORAL_BACKGROUND_* 
TEMPORAL_BACKGROUND = {"input": TEMPORAL_BACKGROUND_INPUT, "accumulate": TEMPORAL_BACKGROUND_ACCUMULATE}
TEMPORAL_CLIP_OFF, TEMPORAL_CLIP_VARIANCE = 0, 1  # RAYZ_TEMPORAL_CLIP_* 
TEMPORAL_CLIP = {"off": TEMPORAL_CLIP_OFF, "variance": TEMPORAL_CLIP_VARIANCE}
TEMPORAL_CLIP_DEFAULTS = {"gamma": 1.0, "min_taps": 4.0}  # RAYZ_TEMPORAL_CLIP_DEFAULT_*

D3 = C.c_double * 3


class Texture(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("even", C.c_uint32), ("odd", C.c_uint32), ("_pad", C.c_uint32),
                ("scale", C.c_double), ("color", D3)]


class Material(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("texture", C.c_uint32), ("method", C.c_uint32), ("_pad", C.c_uint32),
                ("param", C.c_double)]


class Sphere(C.Structure):
    _fields_ = [("center", D3), ("velocity", D3), ("radius", C.c_double), ("material", C.c_uint32),
                ("_pad", C.c_uint32)]


class Triangle(C.Structure):
    _fields_ = [("v0", D3), ("v1", D3), ("v2", D3), ("material", C.c_uint32), ("_pad", C.c_uint32)]


class SceneDesc(C.Structure):
    _fields_ = [("spheres", C.POINTER(Sphere)), ("materials", C.POINTER(Material)),
                ("textures", C.POINTER(Texture)), ("n_spheres", C.c_uint32), ("n_materials", C.c_uint32),
                ("n_textures", C.c_uint32), ("n_triangles", C.c_uint32), ("triangles", C.POINTER(Triangle))]


class CameraDesc(C.Structure):
    _fields_ = [("look_from", D3), ("px_du", D3), ("px_dv", D3), ("px_origin", D3), ("defocus_u", D3),
                ("defocus_v", D3), ("defocus", C.c_uint32), ("_pad", C.c_uint32)]


class RenderParams(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("samples_per_px", C.c_uint32),
                ("max_bounces", C.c_uint32), ("seed", C.c_uint64), ("tmin", C.c_double),
                ("precision", C.c_uint32), ("traversal", C.c_uint32), ("chunk_spp", C.c_uint32),
                ("tile_rows", C.c_uint32), ("shard_index", C.c_uint32), ("shard_count", C.c_uint32)]


class RenderStats(C.Structure):
    _fields_ = [("primary_rays", C.c_uint64), ("segments", C.c_uint64), ("sphere_tests", C.c_uint64),
                ("node_tests", C.c_uint64), ("kernel_ms", C.c_double)]


class QueryParams(C.Structure):
    _fields_ = [("n_rays", C.c_uint32), ("kind", C.c_uint32), ("precision", C.c_uint32), ("traversal", C.c_uint32),
                ("tmin", C.c_double)]


class QueryOutputs(C.Structure):
    _fields_ = [("index", C.c_void_p), ("t", C.c_void_p), ("point", C.c_void_p), ("normal", C.c_void_p),
                ("front_face", C.c_void_p), ("material", C.c_void_p), ("albedo", C.c_void_p), ("hit", C.c_void_p)]


class ChainParams(C.Structure):
    _fields_ = [("max_depth", C.c_uint32), ("_pad", C.c_uint32), ("max_fuzz", C.c_double)]


class ChainOutputs(C.Structure):
    _fields_ = [("key", C.c_void_p), ("depth", C.c_void_p), ("first_index", C.c_void_p)]


class SampledParams(C.Structure):
    _fields_ = [("samples", C.c_uint32), ("_pad", C.c_uint32)]


class SampledOutputs(C.Structure):
    _fields_ = [("albedo", C.c_void_p), ("normal", C.c_void_p), ("t", C.c_void_p), ("hits", C.c_void_p)]


class DenoiseParams(C.Structure):
    _fields_ = [("levels", C.c_uint32), ("normal_power_log2", C.c_uint32), ("flags", C.c_uint32), ("_pad", C.c_uint32),
                ("sigma_color", C.c_double), ("sigma_plane", C.c_double)]


class DenoiseGuidedParams(C.Structure):
    _fields_ = [("levels", C.c_uint32), ("normal_power_log2", C.c_uint32), ("flags", C.c_uint32), ("_pad", C.c_uint32),
                ("sigma_color", C.c_double), ("sigma_plane", C.c_double), ("var_floor", C.c_double)]


class UpscaleParams(C.Structure):
    _fields_ = [("factor", C.c_uint32), ("normal_power_log2", C.c_uint32), ("flags", C.c_uint32), ("form", C.c_uint32),
                ("sigma_plane", C.c_double)]


class NoiseParams(C.Structure):
    _fields_ = [("rel_error", C.c_double), ("mean_floor", C.c_double)]


class NoiseSummary(C.Structure):
    _fields_ = [("pixels", C.c_uint64), ("unconverged", C.c_uint64), ("max_rel2", C.c_double), ("mean_var", C.c_double),
                ("samples_done", C.c_uint32), ("chunks_done", C.c_uint32)]


class AdaptiveSummary(C.Structure):
    _fields_ = [("pixels", C.c_uint64), ("active", C.c_uint64), ("samples_traced", C.c_uint64), ("passes", C.c_uint32),
                ("chunks_done", C.c_uint32), ("samples_done", C.c_uint32), ("_pad", C.c_uint32)]


class TemporalParams(C.Structure):
    _fields_ = [("alpha_min", C.c_double), ("n_max", C.c_double), ("normal_cos_min", C.c_double), ("max_rel_dist", C.c_double)]


class TemporalMomentsParams(C.Structure):
    _fields_ = [("w2_max", C.c_double), ("min_taps", C.c_double)]


class TemporalClipParams(C.Structure):
    _fields_ = [("gamma", C.c_double), ("min_taps", C.c_double)]


assert C.sizeof(Texture) == 48 and C.sizeof(Material) == 24 and C.sizeof(Sphere) == 64 and C.sizeof(Triangle) == 80
assert C.sizeof(SceneDesc) == 48
assert C.sizeof(CameraDesc) == 152 and C.sizeof(RenderParams) == 56 and C.sizeof(RenderStats) == 40
assert C.sizeof(QueryParams) == 24 and C.sizeof(QueryOutputs) == 64 and C.sizeof(DenoiseParams) == 32
assert C.sizeof(NoiseParams) == 16 and C.sizeof(NoiseSummary) == 40 and C.sizeof(DenoiseGuidedParams) == 40
assert C.sizeof(UpscaleParams) == 24
assert C.sizeof(ChainParams) == 16 and C.sizeof(ChainOutputs) == 24
assert C.sizeof(SampledParams) == 8 and C.sizeof(SampledOutputs) == 32
assert C.sizeof(AdaptiveSummary) == 40 and C.sizeof(TemporalParams) == 32 and C.sizeof(TemporalMomentsParams) == 16
assert C.sizeof(TemporalClipParams) == 16

# every symbol include/rayz_hip.h declares: (name, restype, argtypes)
PROTOTYPES = [
    ("rayz_hip_init", C.c_int, [C.c_int]),
    ("rayz_hip_shutdown", None, []),
    ("rayz_hip_last_error", C.c_char_p, []),
    ("rayz_hip_abi_version", C.c_uint32, []),
    ("rayz_hip_debug_set", C.c_int, [C.c_uint32, C.c_longlong]),
    ("rayz_hip_shard_rows", C.c_uint32, [C.POINTER(RenderParams)]),
    ("rayz_hip_chunk_schedule", C.c_uint32, [C.POINTER(RenderParams), C.POINTER(C.c_uint32), C.c_uint32]),
    ("rayz_hip_scene_create", C.c_int, [C.POINTER(SceneDesc), C.POINTER(C.c_void_p)]),
    ("rayz_hip_scene_create_on", C.c_int, [C.c_int, C.POINTER(SceneDesc), C.POINTER(C.c_void_p)]),
    ("rayz_hip_scene_destroy", C.c_int, [C.c_void_p]),
    ("rayz_hip_scene_bvh", C.c_int,
     [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_double), C.POINTER(C.c_uint32),
      C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    ("rayz_hip_render_device", C.c_int,
     [C.c_void_p, C.POINTER(CameraDesc), C.POINTER(RenderParams), C.c_void_p, C.c_void_p]),
    ("rayz_hip_render_device_f64", C.c_int,
     [C.c_void_p, C.POINTER(CameraDesc), C.POINTER(RenderParams), C.c_void_p, C.c_void_p]),
    ("rayz_hip_scene_set_scan_form", C.c_int, [C.c_void_p, C.c_uint32]),
    ("rayz_hip_scene_get_scan_form", C.c_int, [C.c_void_p, C.POINTER(C.c_uint32)]),
    ("rayz_hip_scene_set_primary_lists", C.c_int, [C.c_void_p, C.c_uint32]),
    ("rayz_hip_scene_get_primary_lists", C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]),
    ("rayz_hip_scene_set_cell_lists", C.c_int, [C.c_void_p, C.c_uint32]),
    ("rayz_hip_scene_get_cell_lists", C.c_int, [C.c_void_p, C.POINTER(C.c_uint32)]),
    ("rayz_hip_scene_sync", C.c_int, [C.c_void_p, C.POINTER(RenderStats)]),
    ("rayz_hip_render", C.c_int,
     [C.POINTER(SceneDesc), C.POINTER(CameraDesc), C.POINTER(RenderParams), C.c_void_p,
      C.POINTER(RenderStats)]),
    ("rayz_hip_render_f64", C.c_int,
     [C.POINTER(SceneDesc), C.POINTER(CameraDesc), C.POINTER(RenderParams), C.c_void_p,
      C.POINTER(RenderStats)]),
    ("rayz_hip_tonemap_u8", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    ("rayz_hip_kat", C.c_int, [C.c_uint32, C.c_uint32, C.POINTER(C.c_double), C.c_uint32, C.POINTER(C.c_double)]),
    ("rayz_hip_progressive_create", C.c_int,
     [C.c_void_p, C.POINTER(CameraDesc), C.POINTER(RenderParams), C.POINTER(C.c_void_p)]),
    ("rayz_hip_progressive_step", C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    ("rayz_hip_progressive_step_f64", C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    ("rayz_hip_progressive_info", C.c_int,
     [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(RenderStats)]),
    ("rayz_hip_progressive_destroy", C.c_int, [C.c_void_p]),
    ("rayz_hip_progressive_track_noise", C.c_int, [C.c_void_p]),
    ("rayz_hip_progressive_noise", C.c_int,
     [C.c_void_p, C.POINTER(NoiseParams), C.c_void_p, C.c_void_p, C.POINTER(NoiseSummary), C.c_void_p]),
    ("rayz_hip_progressive_noise_rgb", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    ("rayz_hip_progressive_noise_state", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    ("rayz_hip_progressive_run_until", C.c_int,
     [C.c_void_p, C.POINTER(NoiseParams), C.c_double, C.c_uint32, C.c_void_p, C.POINTER(NoiseSummary), C.c_void_p]),
    ("rayz_hip_progressive_run_until_f64", C.c_int,
     [C.c_void_p, C.POINTER(NoiseParams), C.c_double, C.c_uint32, C.c_void_p, C.POINTER(NoiseSummary), C.c_void_p]),
    ("rayz_hip_noise_kat", C.c_int,
     [C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32, C.POINTER(NoiseParams),
      C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(NoiseSummary)]),
    ("rayz_hip_progressive_set_adaptive", C.c_int, [C.c_void_p, C.c_uint32]),
    ("rayz_hip_progressive_adaptive_step", C.c_int,
     [C.c_void_p, C.POINTER(NoiseParams), C.c_uint32, C.c_void_p, C.POINTER(AdaptiveSummary), C.c_void_p]),
    ("rayz_hip_progressive_adaptive_step_f64", C.c_int,
     [C.c_void_p, C.POINTER(NoiseParams), C.c_uint32, C.c_void_p, C.POINTER(AdaptiveSummary), C.c_void_p]),
    ("rayz_hip_progressive_run_adaptive", C.c_int,
     [C.c_void_p, C.POINTER(NoiseParams), C.c_uint32, C.c_void_p, C.POINTER(AdaptiveSummary), C.c_void_p]),
    ("rayz_hip_progressive_run_adaptive_f64", C.c_int,
     [C.c_void_p, C.POINTER(NoiseParams), C.c_uint32, C.c_void_p, C.POINTER(AdaptiveSummary), C.c_void_p]),
    ("rayz_hip_progressive_sample_counts", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    ("rayz_hip_progressive_frozen_at", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    ("rayz_hip_adaptive_kat", C.c_int,
     [C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32,
      C.c_uint32, C.POINTER(NoiseParams), C.POINTER(C.c_uint32), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
      C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    ("rayz_hip_scene_render_pixels", C.c_int,
     [C.c_void_p, C.POINTER(CameraDesc), C.POINTER(RenderParams), C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
      C.c_void_p]),
    ("rayz_hip_scene_render_pixels_f64", C.c_int,
     [C.c_void_p, C.POINTER(CameraDesc), C.POINTER(RenderParams), C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
      C.c_void_p]),
    ("rayz_hip_multi_create", C.c_int,
     [C.POINTER(C.c_int), C.c_int, C.POINTER(SceneDesc), C.c_uint32, C.POINTER(C.c_void_p)]),
    ("rayz_hip_multi_destroy", C.c_int, [C.c_void_p]),
    ("rayz_hip_multi_info", C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_uint32), C.POINTER(C.c_int)]),
    ("rayz_hip_multi_device_stats", C.c_int, [C.c_void_p, C.c_int, C.POINTER(RenderStats)]),
    ("rayz_hip_multi_timing", C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    ("rayz_hip_multi_render", C.c_int,
     [C.c_void_p, C.POINTER(CameraDesc), C.POINTER(RenderParams), C.c_void_p, C.POINTER(RenderStats)]),
    ("rayz_hip_multi_render_f64", C.c_int,
     [C.c_void_p, C.POINTER(CameraDesc), C.POINTER(RenderParams), C.c_void_p, C.POINTER(RenderStats)]),
    ("rayz_hip_multi_render_u8", C.c_int,
     [C.c_void_p, C.POINTER(CameraDesc), C.POINTER(RenderParams), C.c_void_p, C.POINTER(RenderStats)]),
    ("rayz_hip_render_multi", C.c_int,
     [C.POINTER(C.c_int), C.c_int, C.POINTER(SceneDesc), C.POINTER(CameraDesc), C.POINTER(RenderParams), C.c_void_p,
      C.POINTER(RenderStats)]),
    ("rayz_hip_render_multi_f64", C.c_int,
     [C.POINTER(C.c_int), C.c_int, C.POINTER(SceneDesc), C.POINTER(CameraDesc), C.POINTER(RenderParams), C.c_void_p,
      C.POINTER(RenderStats)]),
    ("rayz_hip_scene_query", C.c_int,
     [C.c_void_p, C.POINTER(QueryParams), C.c_void_p, C.POINTER(QueryOutputs), C.c_void_p]),
    ("rayz_hip_scene_query_camera", C.c_int,
     [C.c_void_p, C.POINTER(CameraDesc), C.POINTER(RenderParams), C.POINTER(QueryOutputs), C.c_void_p]),
    ("rayz_hip_query_sync", C.c_int, [C.c_void_p, C.POINTER(RenderStats)]),
    ("rayz_hip_scene_query_camera_chain", C.c_int,
     [C.c_void_p, C.POINTER(CameraDesc), C.POINTER(RenderParams), C.POINTER(ChainParams), C.POINTER(QueryOutputs),
      C.POINTER(ChainOutputs), C.c_void_p]),
    ("rayz_hip_scene_query_camera_sampled", C.c_int,
     [C.c_void_p, C.POINTER(CameraDesc), C.POINTER(RenderParams), C.POINTER(SampledParams), C.POINTER(SampledOutputs), C.c_void_p]),
    ("rayz_hip_denoiser_create", C.c_int, [C.c_int, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]),
    ("rayz_hip_denoiser_run", C.c_int,
     [C.c_void_p, C.POINTER(DenoiseParams), C.c_void_p, C.POINTER(QueryOutputs), C.c_void_p, C.c_void_p]),
    ("rayz_hip_denoiser_run_guided", C.c_int,
     [C.c_void_p, C.POINTER(DenoiseGuidedParams), C.c_void_p, C.c_void_p, C.POINTER(QueryOutputs), C.c_void_p, C.c_void_p, C.c_void_p]),
    ("rayz_hip_denoiser_run_guided_tap", C.c_int,
     [C.c_void_p, C.POINTER(DenoiseGuidedParams), C.c_void_p, C.c_void_p, C.POINTER(QueryOutputs), C.c_void_p, C.c_void_p, C.c_uint32,
      C.c_void_p, C.c_void_p]),
    ("rayz_hip_denoiser_set_keys", C.c_int, [C.c_void_p, C.c_void_p]),
    ("rayz_hip_denoiser_timing", C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_float), C.c_uint32]),
    ("rayz_hip_denoiser_destroy", C.c_int, [C.c_void_p]),
    ("rayz_hip_upscaler_create", C.c_int, [C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]),
    ("rayz_hip_upscaler_run", C.c_int,
     [C.c_void_p, C.POINTER(UpscaleParams), C.c_void_p, C.c_void_p, C.POINTER(QueryOutputs), C.POINTER(QueryOutputs), C.c_void_p, C.c_void_p,
      C.c_void_p, C.c_void_p]),
    ("rayz_hip_upscaler_run_phase", C.c_int,
     [C.c_void_p, C.POINTER(UpscaleParams), C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(QueryOutputs), C.POINTER(QueryOutputs),
      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("rayz_hip_upscaler_timing", C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    ("rayz_hip_upscaler_footprint_albedo", C.c_int,
     [C.c_void_p, C.POINTER(QueryOutputs), C.POINTER(QueryOutputs), C.c_void_p, C.c_void_p, C.c_void_p]),
    ("rayz_hip_upscaler_footprint_timing", C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    ("rayz_hip_upscaler_destroy", C.c_int, [C.c_void_p]),
    ("rayz_hip_temporal_create", C.c_int, [C.c_int, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]),
    ("rayz_hip_temporal_step", C.c_int,
     [C.c_void_p, C.POINTER(TemporalParams), C.POINTER(CameraDesc), C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(QueryOutputs), C.c_void_p,
      C.c_void_p, C.c_void_p, C.c_void_p]),
    ("rayz_hip_temporal_reset", C.c_int, [C.c_void_p]),
    ("rayz_hip_temporal_timing", C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    ("rayz_hip_temporal_destroy", C.c_int, [C.c_void_p]),
    ("rayz_hip_temporal_track_moments", C.c_int, [C.c_void_p]),
    ("rayz_hip_temporal_step_moments", C.c_int,
     [C.c_void_p, C.POINTER(TemporalParams), C.POINTER(TemporalMomentsParams), C.POINTER(CameraDesc), C.c_uint32, C.c_void_p,
      C.POINTER(QueryOutputs), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("rayz_hip_temporal_track_feedback", C.c_int, [C.c_void_p]),
    ("rayz_hip_temporal_feedback", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    ("rayz_hip_temporal_step_counts", C.c_int,
     [C.c_void_p, C.POINTER(TemporalParams), C.POINTER(CameraDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(QueryOutputs), C.c_void_p,
      C.c_void_p, C.c_void_p, C.c_void_p]),
    ("rayz_hip_temporal_step_moments_counts", C.c_int,
     [C.c_void_p, C.POINTER(TemporalParams), C.POINTER(TemporalMomentsParams), C.POINTER(CameraDesc), C.c_void_p, C.c_void_p,
      C.POINTER(QueryOutputs), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("rayz_hip_temporal_set_resampling", C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p]),
    ("rayz_hip_temporal_get_resampling", C.c_int, [C.c_void_p, C.POINTER(C.c_uint32)]),
    ("rayz_hip_temporal_set_background", C.c_int, [C.c_void_p, C.c_uint32]),
    ("rayz_hip_temporal_get_background", C.c_int, [C.c_void_p, C.POINTER(C.c_uint32)]),
    ("rayz_hip_temporal_set_clip", C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(TemporalClipParams), C.c_void_p]),
    ("rayz_hip_temporal_get_clip", C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(TemporalClipParams)]),
]


class RayzHipError(RuntimeError):
    pass


_lib = None


def load(path: str | None = None) -> C.CDLL:
    """Open librayz_hip.so and bind every prototype.  No fallback: a missing library is an error."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise RayzHipError(
            f"{p} not found: build the HIP extension first (python -c 'import __graft_entry__ as g; g.build()'). "
            "rayz_amd has no CPU fallback.")
    lib = C.CDLL(p)
    for name, res, args in PROTOTYPES:
        fn = getattr(lib, name)  # AttributeError if the library does not export it
        fn.restype = res
        fn.argtypes = args
    if lib.rayz_hip_abi_version() != ABI_VERSION:
        raise RayzHipError(f"ABI mismatch: library {lib.rayz_hip_abi_version()} != binding {ABI_VERSION}")
    if path is None:
        _lib = lib
    return lib


def check(lib: C.CDLL, rc: int, what: str) -> None:
    if rc != OK:
        msg = lib.rayz_hip_last_error()
        raise RayzHipError(f"{what} failed (status {rc}): {msg.decode() if msg else ''}")
