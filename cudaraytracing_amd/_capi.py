"""ctypes binding of lib/libcrt.so (include/crt.h).  No CPU fallback: if the
library is missing or a device call fails, the caller gets an exception."""
import ctypes as C
import os

import numpy as np

from . import build as _build

CRT_OK = 0
ERR_INVALID_ARG, ERR_NO_DEVICE, ERR_HIP, ERR_UNSUPPORTED = -1, -2, -3, -4   # include/crt.h: crt_status
TRAVERSAL_EXACT = 0      # the default: provably the reference's frame
TRAVERSAL_REFERENCE = 1
TRAVERSAL_FAST = 2       # + distance pruning (measured rate of lost rays, include/crt.h)
FLAG_STATS = 1
FLAG_TILED_OUTPUT = 2
FLAG_FORCE_EXACT = 4
FLAG_TRACE_ALL = 8
FLAG_BOUNDED_RADIANCE = 16
FLAG_VARIANCE = 32
FLAG_HALF_BUFFERS = 64   # implies FLAG_VARIANCE
FLAG_PIXEL_FILTER = 128  # keep the sums of the handle's pixel reconstruction filter (crt_set_pixel_filter, crt_filtered_frame)
PIXEL_FILTER_BOX, PIXEL_FILTER_TENT, PIXEL_FILTER_MITCHELL = 0, 1, 2
PIXEL_FILTER_KINDS = {"box": PIXEL_FILTER_BOX, "tent": PIXEL_FILTER_TENT, "mitchell": PIXEL_FILTER_MITCHELL}
GATHER_AUTO, GATHER_RCCL, GATHER_COPY = 0, 1, 2
INTERSECT_RAW_DIRECTIONS, INTERSECT_FORCE_EXACT, INTERSECT_VISIBILITY = 0x100, 0x200, 0x400
TILE = 8


class CrtError(RuntimeError):
    def __init__(self, status, where, detail):
        super().__init__("%s failed: %s (%d)%s" % (where, _strerror(status), status, (": " + detail) if detail else ""))
        self.status = status


class BvhNode(C.Structure):
    _fields_ = [("lc", C.c_int32), ("rc", C.c_int32), ("n", C.c_uint32), ("it", C.c_int32),
                ("aa", C.c_float * 3), ("bb", C.c_float * 3)]


class Triangle(C.Structure):
    _fields_ = [("v1", C.c_float * 3), ("v2", C.c_float * 3), ("v3", C.c_float * 3), ("normal", C.c_float * 3),
                ("area", C.c_float), ("area_of_obj", C.c_float), ("material", C.c_int32)]


class Material(C.Structure):
    _fields_ = [("kd", C.c_float * 3), ("ke", C.c_float * 3), ("ns", C.c_float), ("mode", C.c_int32),
                ("has_emit", C.c_int32)]


class Light(C.Structure):
    _fields_ = [("first_tri", C.c_uint32), ("count", C.c_uint32)]


class SceneDesc(C.Structure):
    _fields_ = [("nodes", C.POINTER(BvhNode)), ("n_nodes", C.c_uint32), ("root", C.c_int32),
                ("tris", C.POINTER(Triangle)), ("n_tris", C.c_uint32),
                ("materials", C.POINTER(Material)), ("n_materials", C.c_uint32),
                ("light_tris", C.POINTER(Triangle)), ("n_light_tris", C.c_uint32),
                ("lights", C.POINTER(Light)), ("n_lights", C.c_uint32)]


class Camera(C.Structure):
    _fields_ = [("eye", C.c_float * 3), ("inv_view", C.c_float * 9), ("fov_y", C.c_float)]


class Params(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("spp", C.c_uint32), ("p_rr", C.c_float),
                ("light_sample_n", C.c_int32), ("seed", C.c_uint64), ("rank", C.c_uint32), ("world", C.c_uint32),
                ("traversal", C.c_uint32), ("flags", C.c_uint32)]


class Stats(C.Structure):
    _fields_ = [("paths", C.c_uint64), ("rays", C.c_uint64), ("shadow_rays", C.c_uint64), ("probe_rays", C.c_uint64),
                ("inner_pops", C.c_uint64), ("leaf_pops", C.c_uint64), ("tri_tests", C.c_uint64), ("hits", C.c_uint64),
                ("stack_sum", C.c_uint64), ("stack_max", C.c_uint64), ("phase_cycles", C.c_uint64 * 24),
                ("kernel_ms", C.c_float), ("logic_ms", C.c_float), ("total_ms", C.c_float),
                ("kernel_launches", C.c_uint32), ("rays_untraced", C.c_uint64)]

    def as_dict(self):
        d = {n: getattr(self, n) for n, _ in self._fields_ if n != "phase_cycles"}
        d["phase_cycles"] = [int(x) for x in self.phase_cycles]
        return d


class MultiInfo(C.Structure):
    _fields_ = [("n_ranks", C.c_uint32), ("gather", C.c_uint32), ("rccl_ranks", C.c_uint32), ("rccl_version", C.c_int32),
                ("render_ms", C.c_float), ("gather_ms", C.c_float), ("frame_ms", C.c_float), ("max_kernel_ms", C.c_float),
                ("bytes_per_rank", C.c_uint64), ("rays", C.c_uint64), ("paths", C.c_uint64), ("rays_untraced", C.c_uint64),
                ("fallback_reason", C.c_char * 160)]

    def as_dict(self):
        d = {n: getattr(self, n) for n, _ in self._fields_}
        d["fallback_reason"] = d["fallback_reason"].decode("utf-8", "replace")
        return d


# crt_multi_buffers: the planes of a gathered multi-device frame in the order of their CRT_MULTI_* bits (plane k: bit 1 << k), each with
# its values per pixel and its element type
MULTI_BUFFERS = {"rgb": (3, np.uint8), "mean": (3, np.float32), "variance": (3, np.float32), "half_a": (3, np.float32), "half_b": (3, np.float32),
                 "albedo": (3, np.float32), "normal": (3, np.float32), "depth": (1, np.float32), "coverage": (1, np.float32), "tri": (1, np.int32),
                 "material": (1, np.int32), "emission": (3, np.float32), "diffuse_albedo": (3, np.float32)}
MULTI_BITS = {name: 1 << k for k, name in enumerate(MULTI_BUFFERS)}
MULTI_ALL = (1 << len(MULTI_BUFFERS)) - 1


class MultiBuffers(C.Structure):
    _fields_ = [(name, C.c_void_p) for name in MULTI_BUFFERS]


class InfoStruct(C.Structure):
    """An info struct of plain numbers: as_dict() is its fields by name."""

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class BvhBuildInfo(InfoStruct):
    _fields_ = [("n_triangles", C.c_uint32), ("n_nodes", C.c_uint32), ("levels", C.c_uint32), ("host_ranges", C.c_uint32),
                ("host_triangles", C.c_uint32), ("host_sorts", C.c_uint32), ("host_sort_elements", C.c_uint64), ("device_ms", C.c_float), ("total_ms", C.c_float), ("host_build_ms", C.c_float)]


class AccelInfo(InfoStruct):
    _fields_ = [("n_leaves", C.c_uint32), ("n_nodes2", C.c_uint32), ("n_nodes4", C.c_uint32), ("depth2", C.c_uint32), ("depth4", C.c_uint32),
                ("sah_on_device", C.c_uint32), ("index_splits", C.c_uint32), ("sah_ms", C.c_float), ("sah_device_ms", C.c_float), ("runtime_init_ms", C.c_float), ("layout_caps", C.c_uint32)]


class TreeScalars(InfoStruct):
    _fields_ = [("root_fast", C.c_int32), ("root_exact", C.c_int32), ("root3_fast", C.c_int32), ("root3_exact", C.c_int32), ("root4", C.c_int32),
                ("root4i", C.c_int32), ("n_mixed4i", C.c_uint32), ("empty4_off", C.c_uint32), ("empty4i_off", C.c_uint32), ("coord_max", C.c_float),
                ("stack_cap", C.c_uint32), ("node4i_f4", C.c_uint32)]


class RefitInfo(InfoStruct):
    _fields_ = [("n_tris", C.c_uint32), ("n_light_tris", C.c_uint32), ("leaves", C.c_uint32), ("boxes_written", C.c_uint32), ("launches", C.c_uint32),
                ("form", C.c_uint32), ("root_aa", C.c_float * 3), ("root_bb", C.c_float * 3), ("coord_max", C.c_float), ("prepare_ms", C.c_float),
                ("device_ms", C.c_float)]

    def as_dict(self):
        d = super().as_dict()
        d["root_aa"], d["root_bb"] = [float(x) for x in self.root_aa], [float(x) for x in self.root_bb]
        return d


class AovBuffers(C.Structure):
    _fields_ = [("albedo", C.c_void_p), ("normal", C.c_void_p), ("depth", C.c_void_p), ("coverage", C.c_void_p), ("tri", C.c_void_p),
                ("material", C.c_void_p)]


class AovInfo(InfoStruct):
    _fields_ = [("rays", C.c_uint64), ("chunks", C.c_uint32), ("total_ms", C.c_float)]


class AovShadingBuffers(C.Structure):
    _fields_ = [("emission", C.c_void_p), ("diffuse_albedo", C.c_void_p)]


class AovDirectBuffers(C.Structure):
    _fields_ = [("direct", C.c_void_p), ("unshadowed", C.c_void_p), ("direct_variance", C.c_void_p), ("visibility", C.c_void_p)]


class AovAoParams(C.Structure):
    _fields_ = [("ao_samples", C.c_uint32), ("max_distance", C.c_float)]


class AovAoBuffers(C.Structure):
    _fields_ = [("ao", C.c_void_p), ("openness", C.c_void_p), ("bent_normal", C.c_void_p)]


class ModulateParams(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("albedo_floor", C.c_float)]


class ModulateInfo(InfoStruct):
    _fields_ = [("total_ms", C.c_float)]


class AovSpecularParams(C.Structure):
    _fields_ = [("max_bounces", C.c_uint32)]


class AovSpecularBuffers(C.Structure):
    _fields_ = [("guide_albedo", C.c_void_p), ("last_normal", C.c_void_p), ("path_depth", C.c_void_p), ("bounces", C.c_void_p),
                ("last_tri", C.c_void_p)]


class DenoiseParams(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("iterations", C.c_uint32), ("sigma_color", C.c_float),
                ("sigma_normal", C.c_float), ("sigma_albedo", C.c_float), ("sigma_depth", C.c_float)]


class DenoiseInputs(C.Structure):
    _fields_ = [("color", C.c_void_p), ("albedo", C.c_void_p), ("normal", C.c_void_p), ("depth", C.c_void_p)]


class DenoiseVarInputs(C.Structure):
    _fields_ = [("color", C.c_void_p), ("variance", C.c_void_p), ("albedo", C.c_void_p), ("normal", C.c_void_p), ("depth", C.c_void_p)]


class NlmParams(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("radius", C.c_uint32), ("patch", C.c_uint32), ("k", C.c_float), ("alpha", C.c_float),
                ("sigma_normal", C.c_float), ("sigma_albedo", C.c_float), ("sigma_depth", C.c_float)]


REGRESS_NORMAL, REGRESS_ALBEDO, REGRESS_DEPTH, REGRESS_POSITION = 1, 2, 4, 8  # include/crt.h: CRT_REGRESS_*


class RegressParams(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("radius", C.c_uint32), ("patch", C.c_uint32), ("k", C.c_float), ("alpha", C.c_float),
                ("sigma_normal", C.c_float), ("sigma_albedo", C.c_float), ("sigma_depth", C.c_float), ("sigma_position", C.c_float), ("ridge", C.c_float),
                ("features", C.c_uint32)]


class RegressInputs(C.Structure):
    _fields_ = [("color", C.c_void_p), ("variance", C.c_void_p), ("weight_color", C.c_void_p), ("weight_variance", C.c_void_p), ("albedo", C.c_void_p),
                ("normal", C.c_void_p), ("depth", C.c_void_p)]


class RegressInfo(InfoStruct):
    _fields_ = [("total_ms", C.c_float), ("fallback_pixels", C.c_uint64)]


class DenoiseInfo(InfoStruct):
    _fields_ = [("total_ms", C.c_float), ("passes", C.c_uint32)]


class TemporalParams(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("cur", Camera), ("prev", Camera), ("depth_tolerance", C.c_float),
                ("normal_tolerance", C.c_float), ("alpha_min", C.c_float)]


class TemporalFrame(C.Structure):
    _fields_ = [("color", C.c_void_p), ("variance", C.c_void_p), ("depth", C.c_void_p), ("normal", C.c_void_p), ("id", C.c_void_p)]


class TemporalHistory(C.Structure):
    _fields_ = [("color", C.c_void_p), ("variance", C.c_void_p), ("history", C.c_void_p), ("depth", C.c_void_p), ("normal", C.c_void_p),
                ("id", C.c_void_p)]


class TemporalInfo(InfoStruct):
    _fields_ = [("total_ms", C.c_float), ("reprojected", C.c_uint64)]


class TemporalClamp(C.Structure):
    _fields_ = [("radius", C.c_uint32), ("gamma", C.c_float)]


class TemporalClampInfo(InfoStruct):
    _fields_ = [("total_ms", C.c_float), ("reprojected", C.c_uint64), ("clamped", C.c_uint64)]


class TemporalDual(C.Structure):
    _fields_ = [("radius", C.c_uint32), ("min_bounces", C.c_float)]


class TemporalSpecularPlanes(C.Structure):
    _fields_ = [("path_depth", C.c_void_p), ("bounces", C.c_void_p), ("last_normal", C.c_void_p)]


class TemporalDualInfo(InfoStruct):
    _fields_ = [("total_ms", C.c_float), ("reprojected", C.c_uint64), ("clamped", C.c_uint64), ("virtual_tried", C.c_uint64),
                ("virtual_taken", C.c_uint64)]


class TemporalMomentPlanes(C.Structure):
    _fields_ = [("m1", C.c_void_p), ("m2", C.c_void_p)]


class VarianceEstimateParams(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("min_history", C.c_uint32), ("radius", C.c_uint32),
                ("sigma_normal", C.c_float), ("sigma_depth", C.c_float), ("of_mean", C.c_uint32), ("history_cap", C.c_float)]


class VarianceEstimateInputs(C.Structure):
    _fields_ = [("m1", C.c_void_p), ("m2", C.c_void_p), ("history", C.c_void_p), ("normal", C.c_void_p), ("depth", C.c_void_p)]


class VarianceEstimateInfo(InfoStruct):
    _fields_ = [("total_ms", C.c_float), ("spatial", C.c_uint64)]


class UpsampleParams(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("low_width", C.c_uint32), ("low_height", C.c_uint32), ("radius", C.c_uint32),
                ("min_weight", C.c_float), ("sigma_normal", C.c_float), ("sigma_albedo", C.c_float), ("sigma_depth", C.c_float)]


class UpsampleLow(C.Structure):
    _fields_ = [("color", C.c_void_p), ("variance", C.c_void_p), ("albedo", C.c_void_p), ("normal", C.c_void_p), ("depth", C.c_void_p)]


class UpsampleGuides(C.Structure):
    _fields_ = [("albedo", C.c_void_p), ("normal", C.c_void_p), ("depth", C.c_void_p)]


class UpsampleInfo(InfoStruct):
    _fields_ = [("total_ms", C.c_float), ("fallback_pixels", C.c_uint64)]


class PyramidParams(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("low_width", C.c_uint32), ("low_height", C.c_uint32)]


class PyramidPlanes(C.Structure):
    """crt_pyramid_planes and crt_pyramid_out_planes: the same five pointers"""
    _fields_ = [("color", C.c_void_p), ("variance", C.c_void_p), ("albedo", C.c_void_p), ("normal", C.c_void_p), ("depth", C.c_void_p)]


class PyramidInfo(InfoStruct):
    _fields_ = [("total_ms", C.c_float)]


class PixelFilter(InfoStruct):
    _fields_ = [("kind", C.c_uint32), ("radius", C.c_float)]


SELECT_MAX_CANDIDATES = 4


class FilterSelectParams(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("n_candidates", C.c_uint32), ("error_radius", C.c_uint32), ("blend_radius", C.c_uint32)]


class FilterSelectInputs(C.Structure):
    _fields_ = [("half_a", C.c_void_p), ("half_b", C.c_void_p), ("half_variance", C.c_void_p), ("filtered_a", C.c_void_p * SELECT_MAX_CANDIDATES),
                ("filtered_b", C.c_void_p * SELECT_MAX_CANDIDATES)]


class FilterSelectInfo(C.Structure):
    _fields_ = [("total_ms", C.c_float), ("chosen", C.c_uint64 * SELECT_MAX_CANDIDATES)]

    def as_dict(self):
        return {"total_ms": float(self.total_ms), "chosen": [int(x) for x in self.chosen]}


class AdaptiveParams(C.Structure):
    _fields_ = [("min_samples", C.c_uint32), ("step_samples", C.c_uint32), ("threshold", C.c_float), ("mean_floor", C.c_float)]


ADAPTIVE_PASSES_REPORTED = 64


class AdaptiveInfo(C.Structure):
    _fields_ = [("passes", C.c_uint32), ("pass_pixels", C.c_uint32 * ADAPTIVE_PASSES_REPORTED), ("paths", C.c_uint64),
                ("paths_uniform", C.c_uint64), ("kernel_ms", C.c_float), ("total_ms", C.c_float)]

    def as_dict(self):
        d = {n: getattr(self, n) for n, _ in self._fields_ if n != "pass_pixels"}
        d["pass_pixels"] = [int(x) for x in self.pass_pixels[:max(0, min(self.passes - 1, ADAPTIVE_PASSES_REPORTED))]]
        return d


class MapInfo(InfoStruct):
    _fields_ = [("paths", C.c_uint64), ("paths_uniform", C.c_uint64), ("launches", C.c_uint32), ("max_samples", C.c_uint32),
                ("kernel_ms", C.c_float), ("total_ms", C.c_float)]


class PlanInfo(InfoStruct):
    _fields_ = [("samples", C.c_uint32), ("spp", C.c_uint32)]


class FrameErrorInfo(C.Structure):
    _fields_ = [("samples_done", C.c_uint32), ("spp", C.c_uint32), ("pixels", C.c_uint64), ("nan_pixels", C.c_uint64), ("above", C.c_uint64),
                ("hist", C.c_uint64 * 16), ("sum_variance", C.c_double), ("sum_mean", C.c_double)]

    def as_dict(self):
        d = {n: getattr(self, n) for n, _ in self._fields_ if n != "hist"}
        d["hist"] = [int(x) for x in self.hist]
        return d


class UntilParams(C.Structure):
    _fields_ = [("min_samples", C.c_uint32), ("step_samples", C.c_uint32), ("threshold", C.c_float), ("mean_floor", C.c_float), ("max_above", C.c_uint64)]


UNTIL_CHECKS_REPORTED = 64


class UntilInfo(C.Structure):
    _fields_ = [("passes", C.c_uint32), ("checks", C.c_uint32), ("samples_done", C.c_uint32), ("reserved_", C.c_uint32),
                ("above", C.c_uint64 * UNTIL_CHECKS_REPORTED), ("paths", C.c_uint64), ("kernel_ms", C.c_float), ("total_ms", C.c_float),
                ("last", FrameErrorInfo)]

    def as_dict(self):
        d = {n: getattr(self, n) for n in ("passes", "checks", "samples_done", "paths", "kernel_ms", "total_ms")}
        d["above"] = [int(x) for x in self.above[:min(self.checks, UNTIL_CHECKS_REPORTED)]]
        d["last"] = self.last.as_dict()
        return d


# the buffers of crt_aov_buffers: name -> (values per pixel, numpy type)
AOV_BUFFERS = {"albedo": (3, np.float32), "normal": (3, np.float32), "depth": (1, np.float32), "coverage": (1, np.float32),
               "tri": (1, np.int32), "material": (1, np.int32)}
# the buffers of crt_aov_specular_buffers
AOV_SPECULAR_BUFFERS = {"guide_albedo": (3, np.float32), "last_normal": (3, np.float32), "path_depth": (1, np.float32),
                        "bounces": (1, np.float32), "last_tri": (1, np.int32)}
# the buffers of crt_aov_shading_buffers
AOV_SHADING_BUFFERS = {"emission": (3, np.float32), "diffuse_albedo": (3, np.float32)}
# the buffers of crt_aov_direct_buffers
AOV_DIRECT_BUFFERS = {"direct": (3, np.float32), "unshadowed": (3, np.float32), "direct_variance": (3, np.float32), "visibility": (1, np.float32)}
# the buffers of crt_aov_ao_buffers
AOV_AO_BUFFERS = {"ao": (1, np.float32), "openness": (1, np.float32), "bent_normal": (3, np.float32)}


class Task(C.Structure):
    _fields_ = [("n_objs", C.c_uint32), ("obj_path", (C.c_char * 512) * 8), ("mtl_dir", (C.c_char * 512) * 8),
                ("lookat", C.c_float * 3), ("up", C.c_float * 3), ("eye_pos", C.c_float * 3), ("fov_y", C.c_float),
                ("width", C.c_uint32), ("height", C.c_uint32), ("bvh_thresh_n", C.c_uint32),
                ("light_sample_n", C.c_uint32), ("spp", C.c_uint32), ("p_rr", C.c_float)]


class ItemOrderInfo(C.Structure):
    _fields_ = [("lists_built", C.c_uint64), ("lists_reused", C.c_uint64), ("classes", C.c_uint32), ("window", C.c_uint32)]


NODE_DTYPE = np.dtype([("lc", "<i4"), ("rc", "<i4"), ("n", "<u4"), ("it", "<i4"), ("aa", "<f4", 3), ("bb", "<f4", 3)])
TRI_DTYPE = np.dtype([("v1", "<f4", 3), ("v2", "<f4", 3), ("v3", "<f4", 3), ("normal", "<f4", 3), ("area", "<f4"),
                      ("area_of_obj", "<f4"), ("material", "<i4")])
MAT_DTYPE = np.dtype([("kd", "<f4", 3), ("ke", "<f4", 3), ("ns", "<f4"), ("mode", "<i4"), ("has_emit", "<i4")])
LIGHT_DTYPE = np.dtype([("first_tri", "<u4"), ("count", "<u4")])

ABI_VERSION = 5  # include/crt.h: CRT_ABI_VERSION

# every symbol include/crt.h declares
EXPORTS = ["crt_strerror", "crt_last_error", "crt_abi_version", "crt_device_count", "crt_scene_create",
           "crt_scene_accel_info", "crt_scene_destroy", "crt_task_obj", "crt_shard_slots", "crt_render", "crt_render_device", "crt_render_range", "crt_render_range_device", "crt_last_launch_ms", "crt_radiance_storage", "crt_preview", "crt_preview_device", "crt_variance", "crt_variance_device", "crt_adaptive_defaults", "crt_render_adaptive", "crt_render_adaptive_device", "crt_render_aov", "crt_render_aov_device", "crt_denoise_defaults", "crt_denoise_scratch_bytes", "crt_denoise", "crt_denoise_device", "crt_denoise_var_defaults", "crt_denoise_var", "crt_denoise_var_device", "crt_denoise_nlm_defaults", "crt_denoise_nlm_scratch_bytes", "crt_denoise_nlm", "crt_denoise_nlm_device", "crt_temporal_defaults", "crt_temporal", "crt_temporal_device", "crt_temporal_clamp_defaults", "crt_temporal_clamped", "crt_temporal_clamped_device", "crt_temporal_moments", "crt_temporal_moments_device", "crt_temporal_dual_defaults", "crt_temporal_dual", "crt_temporal_dual_device", "crt_variance_estimate_defaults", "crt_variance_estimate", "crt_variance_estimate_device", "crt_multi_create", "crt_multi_destroy",
           "crt_multi_render", "crt_multi_frame_device", "crt_multi_render_buffers", "crt_multi_buffers_device", "crt_multi_untile_time", "crt_intersect",
           "crt_device_math", "crt_device_fn", "crt_device_philox", "crt_device_rcp_check", "crt_scene_export", "crt_host_scene_create", "crt_host_scene_destroy",
           "crt_host_scene_add_obj", "crt_host_scene_set_bvh", "crt_host_scene_set_bvh_device", "crt_host_scene_desc", "crt_host_scene_num_objects",
           "crt_host_scene_object", "crt_inverse_view", "crt_task_load", "crt_image_load", "crt_write_png", "crt_write_pfm",
           "crt_render_map", "crt_render_map_device", "crt_sample_plan", "crt_sample_plan_device", "crt_render_planned", "crt_render_planned_device",
           "crt_item_order", "crt_aov_specular_defaults", "crt_render_aov_specular", "crt_render_aov_specular_device",
           "crt_render_aov_shading", "crt_render_aov_shading_device", "crt_modulate_defaults", "crt_demodulate", "crt_demodulate_device", "crt_modulate",
           "crt_modulate_device", "crt_upsample_defaults", "crt_upsample", "crt_upsample_device", "crt_half_buffers", "crt_half_buffers_device",
           "crt_filter_select_defaults", "crt_filter_select_scratch_bytes", "crt_filter_select", "crt_filter_select_device",
           "crt_denoise_regress_defaults", "crt_denoise_regress_scratch_bytes", "crt_denoise_regress", "crt_denoise_regress_device",
           "crt_pyramid_size", "crt_pyramid_down", "crt_pyramid_down_device", "crt_pyramid_merge", "crt_pyramid_merge_device",
           "crt_pixel_filter_defaults", "crt_set_pixel_filter", "crt_filtered_frame", "crt_filtered_frame_device",
           "crt_render_aov_direct", "crt_render_aov_direct_device",
           "crt_aov_ao_defaults", "crt_render_aov_ao", "crt_render_aov_ao_device",
           "crt_frame_error_defaults", "crt_frame_error", "crt_frame_error_device", "crt_until_defaults", "crt_render_until", "crt_render_until_device",
           "crt_scene_refit", "crt_scene_refit_device", "crt_host_scene_transform_object"]

_lib = None


def lib_path():
    return _build.LIB


def lib():
    """Loads libcrt.so (building it first if the sources are newer).  Raises if it cannot."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("CRT_LIB_PATH") or _build.build_lib()  # (CRT_LIB_PATH: an A/B build of the library, tools/ab.sh)
    L = C.CDLL(path)
    L.crt_abi_version.restype = C.c_int
    if L.crt_abi_version() != ABI_VERSION:
        raise RuntimeError("%s speaks ABI version %d, these bindings version %d (include/crt.h: CRT_ABI_VERSION)" % (path, L.crt_abi_version(), ABI_VERSION))
    L.crt_strerror.restype = C.c_char_p
    L.crt_strerror.argtypes = [C.c_int]
    L.crt_last_error.restype = C.c_char_p
    L.crt_device_count.argtypes = [C.POINTER(C.c_int)]
    L.crt_scene_create.argtypes = [C.POINTER(SceneDesc), C.c_int, C.POINTER(C.c_void_p)]
    L.crt_scene_accel_info.argtypes = [C.c_void_p, C.POINTER(AccelInfo)]
    L.crt_scene_destroy.argtypes = [C.c_void_p]
    L.crt_shard_slots.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]
    L.crt_render.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(Params), C.c_void_p, C.c_void_p, C.POINTER(Stats)]
    L.crt_render_device.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(Params), C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.POINTER(Stats)]
    L.crt_render_range.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(Params), C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                   C.POINTER(Stats)]
    L.crt_render_range_device.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(Params), C.c_uint32, C.c_uint32, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.POINTER(Stats)]
    L.crt_last_launch_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_uint32)]
    L.crt_radiance_storage.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
    L.crt_preview.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)]
    L.crt_preview_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)]
    L.crt_variance.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)]
    L.crt_variance_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)]
    L.crt_adaptive_defaults.argtypes = [C.POINTER(AdaptiveParams)]
    L.crt_render_adaptive.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(Params), C.POINTER(AdaptiveParams), C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.POINTER(AdaptiveInfo)]
    L.crt_render_adaptive_device.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(Params), C.POINTER(AdaptiveParams), C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(AdaptiveInfo)]
    L.crt_render_aov.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(Params), C.POINTER(AovBuffers), C.POINTER(AovInfo)]
    L.crt_render_aov_device.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(Params), C.POINTER(AovBuffers), C.c_void_p,
                                        C.POINTER(AovInfo)]
    L.crt_aov_specular_defaults.argtypes = [C.POINTER(AovSpecularParams)]
    L.crt_render_aov_specular.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(Params), C.POINTER(AovSpecularParams),
                                          C.POINTER(AovSpecularBuffers), C.POINTER(AovInfo)]
    L.crt_render_aov_specular_device.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(Params), C.POINTER(AovSpecularParams),
                                                 C.POINTER(AovSpecularBuffers), C.c_void_p, C.POINTER(AovInfo)]
    L.crt_render_aov_shading.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(Params), C.POINTER(AovBuffers), C.POINTER(AovShadingBuffers),
                                         C.POINTER(AovInfo)]
    L.crt_render_aov_shading_device.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(Params), C.POINTER(AovBuffers), C.POINTER(AovShadingBuffers),
                                                C.c_void_p, C.POINTER(AovInfo)]
    L.crt_render_aov_direct.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(Params), C.POINTER(AovDirectBuffers), C.POINTER(AovInfo)]
    L.crt_render_aov_direct_device.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(Params), C.POINTER(AovDirectBuffers), C.c_void_p,
                                               C.POINTER(AovInfo)]
    L.crt_aov_ao_defaults.argtypes = [C.c_void_p, C.POINTER(AovAoParams)]
    L.crt_render_aov_ao.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(Params), C.POINTER(AovAoParams), C.POINTER(AovAoBuffers), C.POINTER(AovInfo)]
    L.crt_render_aov_ao_device.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(Params), C.POINTER(AovAoParams), C.POINTER(AovAoBuffers), C.c_void_p,
                                           C.POINTER(AovInfo)]
    L.crt_modulate_defaults.argtypes = [C.POINTER(ModulateParams)]
    L.crt_demodulate.argtypes = [C.c_int, C.POINTER(ModulateParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.POINTER(ModulateInfo)]
    L.crt_demodulate_device.argtypes = [C.c_int, C.POINTER(ModulateParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.POINTER(ModulateInfo)]
    L.crt_modulate.argtypes = [C.c_int, C.POINTER(ModulateParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(ModulateInfo)]
    L.crt_modulate_device.argtypes = [C.c_int, C.POINTER(ModulateParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.POINTER(ModulateInfo)]
    L.crt_denoise_defaults.argtypes = [C.POINTER(DenoiseParams)]
    L.crt_denoise_scratch_bytes.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]
    L.crt_denoise.argtypes = [C.c_int, C.POINTER(DenoiseParams), C.POINTER(DenoiseInputs), C.c_void_p, C.c_void_p, C.POINTER(DenoiseInfo)]
    L.crt_denoise_device.argtypes = [C.c_int, C.POINTER(DenoiseParams), C.POINTER(DenoiseInputs), C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                     C.c_void_p, C.POINTER(DenoiseInfo)]
    L.crt_denoise_var_defaults.argtypes = [C.POINTER(DenoiseParams)]
    L.crt_denoise_var.argtypes = [C.c_int, C.POINTER(DenoiseParams), C.POINTER(DenoiseVarInputs), C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.POINTER(DenoiseInfo)]
    L.crt_denoise_var_device.argtypes = [C.c_int, C.POINTER(DenoiseParams), C.POINTER(DenoiseVarInputs), C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(DenoiseInfo)]
    L.crt_denoise_nlm_defaults.argtypes = [C.POINTER(NlmParams)]
    L.crt_denoise_nlm_scratch_bytes.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]
    L.crt_denoise_nlm.argtypes = [C.c_int, C.POINTER(NlmParams), C.POINTER(DenoiseVarInputs), C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.POINTER(DenoiseInfo)]
    L.crt_denoise_nlm_device.argtypes = [C.c_int, C.POINTER(NlmParams), C.POINTER(DenoiseVarInputs), C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(DenoiseInfo)]
    L.crt_denoise_regress_defaults.argtypes = [C.POINTER(RegressParams)]
    L.crt_denoise_regress_scratch_bytes.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]
    L.crt_denoise_regress.argtypes = [C.c_int, C.POINTER(RegressParams), C.POINTER(RegressInputs), C.c_void_p, C.c_void_p, C.POINTER(RegressInfo)]
    L.crt_denoise_regress_device.argtypes = [C.c_int, C.POINTER(RegressParams), C.POINTER(RegressInputs), C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                             C.c_void_p, C.POINTER(RegressInfo)]
    L.crt_temporal_defaults.argtypes = [C.POINTER(TemporalParams)]
    L.crt_temporal.argtypes = [C.c_int, C.POINTER(TemporalParams), C.POINTER(TemporalFrame), C.POINTER(TemporalHistory), C.c_void_p, C.c_void_p,
                               C.c_void_p, C.c_void_p, C.POINTER(TemporalInfo)]
    L.crt_temporal_device.argtypes = [C.c_int, C.POINTER(TemporalParams), C.POINTER(TemporalFrame), C.POINTER(TemporalHistory), C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(TemporalInfo)]
    L.crt_temporal_clamp_defaults.argtypes = [C.POINTER(TemporalClamp)]
    L.crt_temporal_clamped.argtypes = [C.c_int, C.POINTER(TemporalParams), C.POINTER(TemporalClamp), C.POINTER(TemporalFrame), C.POINTER(TemporalHistory),
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(TemporalClampInfo)]
    L.crt_temporal_clamped_device.argtypes = [C.c_int, C.POINTER(TemporalParams), C.POINTER(TemporalClamp), C.POINTER(TemporalFrame),
                                              C.POINTER(TemporalHistory), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.POINTER(TemporalClampInfo)]
    L.crt_temporal_moments.argtypes = [C.c_int, C.POINTER(TemporalParams), C.POINTER(TemporalClamp), C.POINTER(TemporalFrame), C.POINTER(TemporalHistory),
                                       C.POINTER(TemporalMomentPlanes), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.POINTER(TemporalClampInfo)]
    L.crt_temporal_moments_device.argtypes = [C.c_int, C.POINTER(TemporalParams), C.POINTER(TemporalClamp), C.POINTER(TemporalFrame),
                                              C.POINTER(TemporalHistory), C.POINTER(TemporalMomentPlanes), C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(TemporalClampInfo)]
    L.crt_temporal_dual_defaults.argtypes = [C.POINTER(TemporalDual)]
    L.crt_temporal_dual.argtypes = [C.c_int, C.POINTER(TemporalParams), C.POINTER(TemporalClamp), C.POINTER(TemporalDual), C.POINTER(TemporalFrame),
                                    C.POINTER(TemporalSpecularPlanes), C.POINTER(TemporalHistory), C.POINTER(TemporalSpecularPlanes), C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(TemporalDualInfo)]
    L.crt_temporal_dual_device.argtypes = [C.c_int, C.POINTER(TemporalParams), C.POINTER(TemporalClamp), C.POINTER(TemporalDual), C.POINTER(TemporalFrame),
                                           C.POINTER(TemporalSpecularPlanes), C.POINTER(TemporalHistory), C.POINTER(TemporalSpecularPlanes), C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(TemporalDualInfo)]
    L.crt_variance_estimate_defaults.argtypes = [C.POINTER(VarianceEstimateParams)]
    L.crt_variance_estimate.argtypes = [C.c_int, C.POINTER(VarianceEstimateParams), C.POINTER(VarianceEstimateInputs), C.c_void_p,
                                        C.POINTER(VarianceEstimateInfo)]
    L.crt_variance_estimate_device.argtypes = [C.c_int, C.POINTER(VarianceEstimateParams), C.POINTER(VarianceEstimateInputs), C.c_void_p, C.c_void_p,
                                               C.POINTER(VarianceEstimateInfo)]
    L.crt_pyramid_size.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.crt_pyramid_down.argtypes = [C.c_int, C.POINTER(PyramidParams), C.POINTER(PyramidPlanes), C.POINTER(PyramidPlanes), C.POINTER(PyramidInfo)]
    L.crt_pyramid_down_device.argtypes = [C.c_int, C.POINTER(PyramidParams), C.POINTER(PyramidPlanes), C.POINTER(PyramidPlanes), C.c_void_p,
                                          C.POINTER(PyramidInfo)]
    L.crt_pyramid_merge.argtypes = [C.c_int, C.POINTER(PyramidParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(PyramidInfo)]
    L.crt_pyramid_merge_device.argtypes = [C.c_int, C.POINTER(PyramidParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.POINTER(PyramidInfo)]
    L.crt_upsample_defaults.argtypes = [C.POINTER(UpsampleParams)]
    L.crt_upsample.argtypes = [C.c_int, C.POINTER(UpsampleParams), C.POINTER(UpsampleLow), C.POINTER(UpsampleGuides), C.c_void_p, C.c_void_p, C.c_void_p,
                               C.POINTER(UpsampleInfo)]
    L.crt_upsample_device.argtypes = [C.c_int, C.POINTER(UpsampleParams), C.POINTER(UpsampleLow), C.POINTER(UpsampleGuides), C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.POINTER(UpsampleInfo)]
    L.crt_half_buffers.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)]
    L.crt_half_buffers_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)]
    L.crt_filter_select_defaults.argtypes = [C.POINTER(FilterSelectParams)]
    L.crt_filter_select_scratch_bytes.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]
    L.crt_filter_select.argtypes = [C.c_int, C.POINTER(FilterSelectParams), C.POINTER(FilterSelectInputs), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.POINTER(FilterSelectInfo)]
    L.crt_filter_select_device.argtypes = [C.c_int, C.POINTER(FilterSelectParams), C.POINTER(FilterSelectInputs), C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(FilterSelectInfo)]
    L.crt_multi_create.argtypes = [C.POINTER(SceneDesc), C.POINTER(C.c_int), C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]
    L.crt_multi_destroy.argtypes = [C.c_void_p]
    L.crt_multi_render.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(Params), C.c_void_p, C.c_void_p, C.POINTER(Stats),
                                   C.POINTER(MultiInfo)]
    L.crt_multi_frame_device.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int)]
    L.crt_multi_render_buffers.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(Params), C.c_uint32, C.POINTER(MultiBuffers), C.POINTER(Stats),
                                           C.POINTER(MultiInfo)]
    L.crt_multi_buffers_device.argtypes = [C.c_void_p, C.POINTER(MultiBuffers), C.POINTER(C.c_int)]
    L.crt_multi_untile_time.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_float)]
    L.crt_intersect.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    L.crt_device_math.argtypes = [C.c_int, C.c_char_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.crt_device_fn.argtypes = [C.c_int, C.c_char_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
    L.crt_device_philox.argtypes = [C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.crt_device_rcp_check.argtypes = [C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.crt_scene_export.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.crt_host_scene_create.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]
    L.crt_host_scene_destroy.argtypes = [C.c_void_p]
    L.crt_host_scene_add_obj.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p]
    L.crt_host_scene_set_bvh.argtypes = [C.c_void_p, C.c_uint32]
    L.crt_host_scene_set_bvh_device.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.POINTER(BvhBuildInfo)]
    L.crt_host_scene_desc.argtypes = [C.c_void_p, C.POINTER(SceneDesc)]
    L.crt_host_scene_num_objects.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
    L.crt_host_scene_object.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_float), C.POINTER(C.c_int32),
                                        C.POINTER(C.c_uint32)]
    L.crt_inverse_view.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.crt_task_load.argtypes = [C.c_char_p, C.POINTER(Task)]
    L.crt_task_obj.argtypes = [C.c_char_p, C.c_uint32, C.c_char_p, C.c_char_p, C.c_uint32]
    L.crt_image_load.argtypes = [C.c_char_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_void_p, C.c_uint64]
    L.crt_write_png.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.c_void_p]
    L.crt_write_pfm.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    L.crt_render_map.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(Params), C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.POINTER(MapInfo)]
    L.crt_render_map_device.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(Params), C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(MapInfo)]
    L.crt_sample_plan.argtypes = [C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.POINTER(PlanInfo)]
    L.crt_sample_plan_device.argtypes = [C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.POINTER(PlanInfo)]
    L.crt_render_planned.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(Params), C.POINTER(AdaptiveParams), C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.POINTER(MapInfo)]
    L.crt_render_planned_device.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(Params), C.POINTER(AdaptiveParams), C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(MapInfo)]
    if hasattr(L, "crt_set_pixel_filter"):  # (likewise: the entry points came without a new ABI version)
        L.crt_pixel_filter_defaults.argtypes = [C.POINTER(PixelFilter)]
        L.crt_set_pixel_filter.argtypes = [C.c_void_p, C.POINTER(PixelFilter)]
        L.crt_filtered_frame.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)]
        L.crt_filtered_frame_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)]
    if hasattr(L, "crt_item_order"):  # (a CRT_LIB_PATH library of this ABI version from before the entry point was appended has none)
        L.crt_item_order.argtypes = [C.c_void_p, C.POINTER(ItemOrderInfo)]
    if hasattr(L, "crt_frame_error"):  # (likewise)
        L.crt_frame_error_defaults.argtypes = [C.POINTER(C.c_float), C.POINTER(C.c_float)]
        L.crt_frame_error.argtypes = [C.c_void_p, C.c_float, C.c_float, C.POINTER(FrameErrorInfo)]
        L.crt_frame_error_device.argtypes = [C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_void_p]
        L.crt_until_defaults.argtypes = [C.POINTER(UntilParams)]
        L.crt_render_until.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(Params), C.POINTER(UntilParams), C.c_uint32, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.POINTER(UntilInfo)]
        L.crt_render_until_device.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(Params), C.POINTER(UntilParams), C.c_uint32, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.POINTER(UntilInfo)]
    if hasattr(L, "crt_scene_refit"):  # (likewise)
        L.crt_scene_refit.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(RefitInfo)]
        L.crt_scene_refit_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(RefitInfo)]
        L.crt_host_scene_transform_object.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_float)]
    _lib = L
    return L


def _strerror(status):
    try:
        return lib().crt_strerror(status).decode()
    except Exception:
        return "status"


def check(status, where):
    if status != CRT_OK:
        raise CrtError(status, where, lib().crt_last_error().decode())


def ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None
