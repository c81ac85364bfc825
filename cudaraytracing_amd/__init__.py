"""cudaraytracing_amd -- MI355X-native Monte-Carlo path tracer with the
config.json / Scene / Render surface of guomc9/CudaRayTracing.

The package is a thin ctypes layer over lib/libcrt.so (C ABI: include/crt.h),
which holds the C++ host side (OBJ/MTL loader, median-split BVH, flat scene
export) and the hand-written HIP kernels for gfx950.
"""
from .api import (MultiRender, Render, Scene, Task, adaptive_defaults, aov_specular_defaults, denoise, denoise_defaults, denoise_device, denoise_nlm, denoise_nlm_defaults, denoise_nlm_device, denoise_nlm_scratch_bytes, denoise_regress, denoise_regress_defaults, denoise_regress_device, denoise_regress_scratch_bytes, denoise_scratch_bytes, denoise_var, denoise_var_defaults, denoise_var_device, demodulate, demodulate_device, modulate, modulate_defaults, modulate_device, temporal, temporal_clamp_defaults, temporal_defaults, temporal_device, variance_estimate, variance_estimate_defaults, variance_estimate_device, upsample, upsample_defaults, upsample_device, filter_select, filter_select_defaults, filter_select_device, filter_select_scratch_bytes, device_count, device_fn, device_math, device_philox, device_rcp_check, fov_to_radians,
                  get_inverse_view_matrix, image_load, shard_slots, write_pfm)
from ._capi import (FLAG_BOUNDED_RADIANCE, FLAG_FORCE_EXACT, FLAG_STATS, FLAG_TILED_OUTPUT, FLAG_TRACE_ALL, FLAG_VARIANCE, FLAG_HALF_BUFFERS, TRAVERSAL_FAST, TRAVERSAL_REFERENCE, TRAVERSAL_EXACT, GATHER_AUTO, GATHER_RCCL,
                    GATHER_COPY, INTERSECT_RAW_DIRECTIONS, INTERSECT_FORCE_EXACT, INTERSECT_VISIBILITY, REGRESS_NORMAL, REGRESS_ALBEDO, REGRESS_DEPTH,
                    REGRESS_POSITION, CrtError)

__all__ = ["MultiRender", "REGRESS_NORMAL", "REGRESS_ALBEDO", "REGRESS_DEPTH", "REGRESS_POSITION","GATHER_AUTO", "GATHER_RCCL", "GATHER_COPY", "INTERSECT_RAW_DIRECTIONS", "INTERSECT_FORCE_EXACT", "INTERSECT_VISIBILITY", "Render", "Scene", "Task", "adaptive_defaults", "aov_specular_defaults", "denoise", "denoise_defaults", "denoise_device", "denoise_nlm", "denoise_nlm_defaults", "denoise_nlm_device", "denoise_nlm_scratch_bytes", "denoise_regress", "denoise_regress_defaults", "denoise_regress_device", "denoise_regress_scratch_bytes", "denoise_scratch_bytes", "denoise_var", "denoise_var_defaults", "denoise_var_device", "demodulate", "demodulate_device", "modulate", "modulate_defaults", "modulate_device", "temporal", "temporal_clamp_defaults", "temporal_defaults", "temporal_device", "variance_estimate", "variance_estimate_defaults", "variance_estimate_device", "upsample", "upsample_defaults", "upsample_device", "filter_select", "filter_select_defaults", "filter_select_device", "filter_select_scratch_bytes", "device_count", "device_fn", "device_math", "device_philox", "device_rcp_check", "fov_to_radians",
           "get_inverse_view_matrix", "image_load", "shard_slots", "write_pfm", "FLAG_STATS", "FLAG_TILED_OUTPUT", "FLAG_FORCE_EXACT", "FLAG_TRACE_ALL", "FLAG_BOUNDED_RADIANCE", "FLAG_VARIANCE", "FLAG_HALF_BUFFERS", "TRAVERSAL_FAST",
           "TRAVERSAL_REFERENCE", "TRAVERSAL_EXACT", "CrtError"]
