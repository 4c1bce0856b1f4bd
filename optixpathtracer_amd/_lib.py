"""ctypes binding of libptamd.so (include/pt_amd.h). Fails loudly when the library is absent."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PT_LIB") or os.path.join(HERE, "libptamd.so")  # PT_LIB: experiment builds (tools/variants.sh)

# every symbol include/pt_amd.h declares
EXPORTS = [
    "pt_create", "pt_destroy", "pt_last_error", "pt_set_options", "pt_get_options", "pt_set_probe", "pt_build_cdf",
    "pt_resize", "pt_set_camera", "pt_uvw_frame", "pt_set_partition", "pt_render", "pt_download", "pt_upload_accum",
    "pt_device_buffer", "pt_tonemap_sqrt", "pt_owned_pixels", "pt_pack", "pt_unpack", "pt_get_stats", "pt_trace", "pt_sync",
    "pt_eval_table", "pt_version", "pt_set_probe_image", "pt_get_probe_cdf", "pt_render_regions", "pt_denoise",
    "pt_create_multi", "pt_multi_destroy", "pt_multi_last_error", "pt_multi_size", "pt_multi_ctx", "pt_multi_set_options", "pt_multi_set_probe",
    "pt_multi_set_probe_image", "pt_multi_resize", "pt_multi_set_camera", "pt_multi_render", "pt_multi_render_regions", "pt_multi_gather",
    "pt_multi_get_stats", "pt_export_bvh", "pt_render_batch", "pt_multi_render_batch",
    "pt_pack_async", "pt_pack_wait", "pt_unpack_display", "pt_display_sync", "pt_display_buffer", "pt_download_display", "pt_multi_flush",
    "pt_render_device", "pt_stream", "pt_wait_event", "pt_get_stats_n", "pt_stats_size",
    "pt_load_obj", "pt_obj_free", "pt_obj_num_meshes", "pt_obj_get_mesh", "pt_obj_num_textures", "pt_obj_texture_path", "pt_obj_last_error",
    "pt_update_meshes", "pt_multi_update_meshes",
    "pt_update_meshes_device", "pt_transform_meshes", "pt_multi_transform_meshes", "pt_download_vertices",
    "pt_render_mask", "pt_adaptive_begin", "pt_render_adaptive", "pt_adaptive_end", "pt_download_adaptive",
    "pt_trace_device", "pt_query_wait", "pt_render_gbuffer", "pt_temporal_accumulate", "pt_filter_planes",
    "pt_vertex_count", "pt_copy_vertices_device", "pt_motion_planes", "pt_temporal_moments", "pt_modulate_planes",
    "pt_sample_plan", "pt_temporal_carry", "pt_copy_texcoords_device", "pt_surface_planes",
    "pt_texture_mips_layout", "pt_copy_texture_mips_device", "pt_surface_lod_planes", "pt_surface_aniso_planes",
    "pt_upsample_planes", "pt_edge_aa_planes", "pt_exposure_planes", "pt_tonemap_planes", "pt_bloom_layout", "pt_bloom_planes",
    "pt_motion_blur_layout", "pt_motion_blur_planes",
    "pt_dof_layout", "pt_dof_planes", "pt_lens_warp_planes", "pt_warp_matrix", "pt_ao_layout", "pt_ao_planes",
    "pt_reflect_layout", "pt_reflect_planes", "pt_shadow_layout", "pt_shadow_planes",
    "pt_set_views", "pt_get_views", "pt_set_view_cameras", "pt_set_view_cameras_device", "pt_multi_set_views", "pt_multi_set_view_cameras",
]

PT_UPDATE_REFIT, PT_UPDATE_REBUILD = 0, 1  # pt_update_mode
PT_FROM_REST, PT_FROM_CURRENT = 0, 1  # pt_transform_source


PT_ADAPT_MOMENTS, PT_ADAPT_ACTIVE = 0, 1  # pt_adaptive_array
PT_QUERY_CLOSEST, PT_QUERY_ANY, PT_QUERY_ASYNC = 0, 1, 2  # pt_query_flags
PT_MAX_VIEWS = 4096


class View(C.Structure):  # pt_view
    _fields_ = [("x", C.c_int32), ("y", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("eye", C.c_float * 3), ("U", C.c_float * 3), ("V", C.c_float * 3), ("W", C.c_float * 3)]


assert C.sizeof(View) == 64


class Hit(C.Structure):  # pt_hit
    _fields_ = [("t", C.c_float), ("u", C.c_float), ("v", C.c_float), ("prim", C.c_int32), ("mesh", C.c_int32), ("ng", C.c_float * 3)]


# pt_hit as a NumPy record: the same 32 bytes
HIT_DTYPE = np.dtype([("t", "<f4"), ("u", "<f4"), ("v", "<f4"), ("prim", "<i4"), ("mesh", "<i4"), ("ng", "<f4", (3,))])


class QueryStats(C.Structure):  # pt_query_stats
    _fields_ = [("rays", C.c_uint64), ("hits", C.c_uint64), ("invalid_rays", C.c_uint64), ("stage_ms", C.c_double), ("trace_ms", C.c_double),
                ("attrib_ms", C.c_double), ("state_bytes", C.c_uint64)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class GBufferDesc(C.Structure):  # pt_gbuffer_desc
    _fields_ = [("hit", C.c_void_p), ("depth", C.c_void_p), ("position", C.c_void_p), ("motion", C.c_void_p), ("ray", C.c_void_p),
                ("prev_cameras", C.c_void_p), ("num_prev_cameras", C.c_uint32), ("block_mask", C.c_void_p)]


class GBufferStats(C.Structure):  # pt_gbuffer_stats
    _fields_ = [("pixels", C.c_uint64), ("hits", C.c_uint64), ("kernel_ms", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


# the planes of pt_render_gbuffer: float32 words per pixel
GBUFFER_PLANES = {"hit": 8, "depth": 1, "position": 4, "motion": 2, "ray": 8}

PT_TEMPORAL_CLEAR_COLOR = 1  # pt_temporal_flags


class TemporalDesc(C.Structure):  # pt_temporal_desc
    _fields_ = [("color", C.c_void_p), ("motion", C.c_void_p), ("hit", C.c_void_p), ("position", C.c_void_p), ("prev_hit", C.c_void_p),
                ("prev_position", C.c_void_p), ("history_in", C.c_void_p), ("length_in", C.c_void_p), ("history_out", C.c_void_p),
                ("length_out", C.c_void_p), ("frame_rgba8", C.c_void_p), ("copy_out", C.c_void_p), ("block_mask", C.c_void_p),
                ("color_scale", C.c_float), ("normal_cos", C.c_float), ("plane_eps", C.c_float), ("min_weight", C.c_float),
                ("max_history", C.c_uint32), ("flags", C.c_uint32)]


class TemporalStats(C.Structure):  # pt_temporal_stats
    _fields_ = [("pixels", C.c_uint64), ("reprojected", C.c_uint64), ("kernel_ms", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


# the planes of pt_temporal_accumulate: 32-bit words per pixel (frame_rgba8 holds packed bytes, the others float32)
TEMPORAL_PLANES = {"color": 4, "motion": 2, "hit": 8, "position": 4, "prev_hit": 8, "prev_position": 4, "history_in": 4, "length_in": 1,
                   "history_out": 4, "length_out": 1, "frame_rgba8": 1, "copy_out": 4}
TEMPORAL_OUTPUTS = ("history_out", "length_out", "frame_rgba8", "copy_out")


class FilterDesc(C.Structure):  # pt_filter_desc
    _fields_ = [("color", C.c_void_p), ("hit", C.c_void_p), ("position", C.c_void_p), ("variance", C.c_void_p), ("length", C.c_void_p),
                ("out", C.c_void_p), ("scratch", C.c_void_p), ("frame_rgba8", C.c_void_p), ("block_mask", C.c_void_p),
                ("iterations", C.c_int32), ("sigma_lum", C.c_float), ("normal_cos", C.c_float), ("plane_eps", C.c_float),
                ("min_length", C.c_uint32), ("flags", C.c_uint32)]


class FilterStats(C.Structure):  # pt_filter_stats
    _fields_ = [("pixels", C.c_uint64), ("filtered", C.c_uint64), ("spatial", C.c_uint64), ("kernel_ms", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


# the planes of pt_filter_planes: 32-bit words per pixel (frame_rgba8 holds packed bytes, the others float32)
FILTER_PLANES = {"color": 4, "hit": 8, "position": 4, "variance": 1, "length": 1, "out": 4, "scratch": 4, "frame_rgba8": 1}
FILTER_OUTPUTS = ("out", "scratch", "frame_rgba8")


class MotionDesc(C.Structure):  # pt_motion_desc
    _fields_ = [("hit", C.c_void_p), ("prev_vertices", C.c_void_p), ("motion", C.c_void_p), ("prev_point", C.c_void_p), ("prev_surface", C.c_void_p),
                ("prev_cameras", C.c_void_p), ("num_prev_cameras", C.c_uint32), ("block_mask", C.c_void_p), ("flags", C.c_uint32)]


class MotionStats(C.Structure):  # pt_motion_stats
    _fields_ = [("pixels", C.c_uint64), ("hits", C.c_uint64), ("stale", C.c_uint64), ("kernel_ms", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


# the output planes of pt_motion_planes: float32 words per pixel
MOTION_PLANES = {"motion": 2, "prev_point": 4, "prev_surface": 8}


class SurfaceDesc(C.Structure):  # pt_surface_desc
    _fields_ = [("hit", C.c_void_p), ("prim_texcoords", C.c_void_p), ("albedo", C.c_void_p), ("texcoord", C.c_void_p), ("block_mask", C.c_void_p),
                ("flags", C.c_uint32)]


class SurfaceStats(C.Structure):  # pt_surface_stats
    _fields_ = [("pixels", C.c_uint64), ("hits", C.c_uint64), ("stale", C.c_uint64), ("textured", C.c_uint64), ("kernel_ms", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


# the output planes of pt_surface_planes: float32 words per pixel
SURFACE_PLANES = {"albedo": 4, "texcoord": 2}


class SurfaceLodDesc(C.Structure):  # pt_surface_lod_desc
    _fields_ = [("hit", C.c_void_p), ("prim_texcoords", C.c_void_p), ("mips", C.c_void_p), ("mips_bytes", C.c_size_t), ("albedo", C.c_void_p),
                ("texcoord", C.c_void_p), ("footprint", C.c_void_p), ("lod", C.c_void_p), ("block_mask", C.c_void_p),
                ("footprint_scale", C.c_float), ("flags", C.c_uint32)]


class SurfaceLodStats(C.Structure):  # pt_surface_lod_stats
    _fields_ = [("pixels", C.c_uint64), ("hits", C.c_uint64), ("stale", C.c_uint64), ("textured", C.c_uint64), ("minified", C.c_uint64),
                ("kernel_ms", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


# the output planes of pt_surface_lod_planes: float32 words per pixel
SURFACE_LOD_PLANES = {"albedo": 4, "texcoord": 2, "footprint": 4, "lod": 1}


class SurfaceAnisoDesc(C.Structure):  # pt_surface_aniso_desc
    _fields_ = [("hit", C.c_void_p), ("prim_texcoords", C.c_void_p), ("mips", C.c_void_p), ("mips_bytes", C.c_size_t), ("albedo", C.c_void_p),
                ("texcoord", C.c_void_p), ("footprint", C.c_void_p), ("lod", C.c_void_p), ("block_mask", C.c_void_p),
                ("footprint_scale", C.c_float), ("taps", C.c_void_p), ("max_aniso", C.c_uint32), ("flags", C.c_uint32)]


class SurfaceAnisoStats(C.Structure):  # pt_surface_aniso_stats
    _fields_ = [("pixels", C.c_uint64), ("hits", C.c_uint64), ("stale", C.c_uint64), ("textured", C.c_uint64), ("minified", C.c_uint64),
                ("anisotropic", C.c_uint64), ("taps", C.c_uint64), ("kernel_ms", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


# the output planes of pt_surface_aniso_planes: float32 words per pixel
SURFACE_ANISO_PLANES = {"albedo": 4, "texcoord": 2, "footprint": 4, "lod": 1, "taps": 1}


class UpsampleDesc(C.Structure):  # pt_upsample_desc
    _fields_ = [("lo_color", C.c_void_p), ("lo_hit", C.c_void_p), ("lo_position", C.c_void_p), ("hit", C.c_void_p), ("position", C.c_void_p),
                ("out", C.c_void_p), ("weight_out", C.c_void_p), ("block_mask", C.c_void_p), ("lo_width", C.c_uint32), ("lo_height", C.c_uint32),
                ("scale", C.c_uint32), ("normal_cos", C.c_float), ("plane_eps", C.c_float), ("flags", C.c_uint32)]


class UpsampleStats(C.Structure):  # pt_upsample_stats
    _fields_ = [("pixels", C.c_uint64), ("hits", C.c_uint64), ("full", C.c_uint64), ("rescued", C.c_uint64), ("orphans", C.c_uint64),
                ("kernel_ms", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


# the planes of pt_upsample_planes: float32 words per pixel (the lo_ planes at the low resolution, the others frame-sized)
UPSAMPLE_PLANES = {"lo_color": 4, "lo_hit": 8, "lo_position": 4, "hit": 8, "position": 4, "out": 4, "weight_out": 1}
UPSAMPLE_OUTPUTS = ("out", "weight_out")


class EdgeAaDesc(C.Structure):  # pt_edge_aa_desc
    _fields_ = [("color", C.c_void_p), ("hit", C.c_void_p), ("position", C.c_void_p), ("out", C.c_void_p), ("edge", C.c_void_p),
                ("frame_rgba8", C.c_void_p), ("block_mask", C.c_void_p), ("normal_cos", C.c_float), ("plane_eps", C.c_float), ("flags", C.c_uint32)]


class EdgeAaStats(C.Structure):  # pt_edge_aa_stats
    _fields_ = [("pixels", C.c_uint64), ("hits", C.c_uint64), ("stale", C.c_uint64), ("boundary", C.c_uint64), ("blended", C.c_uint64),
                ("kernel_ms", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


# the planes of pt_edge_aa_planes: 32-bit words per pixel
EDGE_AA_PLANES = {"color": 4, "hit": 8, "position": 4, "out": 4, "edge": 2, "frame_rgba8": 1}
EDGE_AA_OUTPUTS = ("out", "edge", "frame_rgba8")


PT_EXPOSURE_BINS = 256
PT_EXPOSURE_ACCUMULATE, PT_EXPOSURE_FROM_HISTOGRAM = 1, 2  # pt_exposure_flags
PT_TONEMAP_LINEAR, PT_TONEMAP_REINHARD, PT_TONEMAP_ACES = 0, 1, 2  # pt_tonemap_op
TONEMAP_OPS = {"linear": PT_TONEMAP_LINEAR, "reinhard": PT_TONEMAP_REINHARD, "aces": PT_TONEMAP_ACES}


class ExposureDesc(C.Structure):  # pt_exposure_desc
    _fields_ = [("color", C.c_void_p), ("hit", C.c_void_p), ("hist", C.c_void_p), ("state_in", C.c_void_p), ("state_out", C.c_void_p),
                ("block_mask", C.c_void_p), ("low_permille", C.c_uint32), ("high_permille", C.c_uint32), ("key_log2", C.c_float),
                ("ev_min", C.c_float), ("ev_max", C.c_float), ("rate_up", C.c_float), ("rate_down", C.c_float), ("flags", C.c_uint32)]


class ExposureStats(C.Structure):  # pt_exposure_stats
    _fields_ = [("pixels", C.c_uint64), ("skipped", C.c_uint64), ("nonfinite", C.c_uint64), ("under", C.c_uint64), ("over", C.c_uint64),
                ("kernel_ms", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class TonemapDesc(C.Structure):  # pt_tonemap_desc
    _fields_ = [("color", C.c_void_p), ("state", C.c_void_p), ("out", C.c_void_p), ("frame_rgba8", C.c_void_p), ("block_mask", C.c_void_p),
                ("exposure", C.c_float), ("white", C.c_float), ("op", C.c_uint32), ("flags", C.c_uint32)]


class TonemapStats(C.Structure):  # pt_tonemap_stats
    _fields_ = [("pixels", C.c_uint64), ("clipped", C.c_uint64), ("kernel_ms", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


# the frame-sized planes of pt_exposure_planes and pt_tonemap_planes: 32-bit words per pixel (hist and the state words are per view)
EXPOSURE_PLANES = {"color": 4, "hit": 8}
TONEMAP_PLANES = {"color": 4, "out": 4, "frame_rgba8": 1}
TONEMAP_OUTPUTS = ("out", "frame_rgba8")


PT_BLOOM_MAX_LEVELS = 8


class BloomDesc(C.Structure):  # pt_bloom_desc
    _fields_ = [("color", C.c_void_p), ("state", C.c_void_p), ("out", C.c_void_p), ("scratch", C.c_void_p), ("block_mask", C.c_void_p),
                ("exposure", C.c_float), ("threshold", C.c_float), ("knee", C.c_float), ("clamp", C.c_float), ("spread", C.c_float),
                ("intensity", C.c_float), ("levels", C.c_uint32), ("flags", C.c_uint32)]


class BloomStats(C.Structure):  # pt_bloom_stats
    _fields_ = [("pixels", C.c_uint64), ("sources", C.c_uint64), ("bright", C.c_uint64), ("nonfinite", C.c_uint64), ("kernel_ms", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


# the frame-sized planes of pt_bloom_planes: 32-bit words per pixel (the scratch pyramid is pt_bloom_layout's, the state words per view)
BLOOM_PLANES = {"color": 4, "out": 4}
BLOOM_OUTPUTS = ("out",)


PT_MOTION_BLUR_TILE = 16
PT_MOTION_BLUR_JITTER = 1  # pt_motion_blur_flags


class MotionBlurDesc(C.Structure):  # pt_motion_blur_desc
    _fields_ = [("color", C.c_void_p), ("motion", C.c_void_p), ("depth", C.c_void_p), ("out", C.c_void_p), ("scratch", C.c_void_p),
                ("block_mask", C.c_void_p), ("shutter", C.c_float), ("max_blur", C.c_float), ("depth_soft", C.c_float), ("taps", C.c_uint32),
                ("seed", C.c_uint32), ("flags", C.c_uint32)]


class MotionBlurStats(C.Structure):  # pt_motion_blur_stats
    _fields_ = [("pixels", C.c_uint64), ("sources", C.c_uint64), ("unknown", C.c_uint64), ("moving", C.c_uint64), ("taps", C.c_uint64),
                ("nonfinite", C.c_uint64), ("kernel_ms", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


# the frame-sized planes of pt_motion_blur_planes: 32-bit words per pixel (the scratch, T and N of every view, is pt_motion_blur_layout's)
MOTION_BLUR_PLANES = {"color": 4, "motion": 2, "depth": 1, "out": 4}
MOTION_BLUR_OUTPUTS = ("out",)


PT_DOF_TILE = 16
PT_DOF_JITTER = 1  # pt_dof_flags


class DofDesc(C.Structure):  # pt_dof_desc
    _fields_ = [("color", C.c_void_p), ("depth", C.c_void_p), ("out", C.c_void_p), ("scratch", C.c_void_p), ("block_mask", C.c_void_p),
                ("view_focus", C.c_void_p), ("focus", C.c_float), ("aperture", C.c_float), ("max_radius", C.c_float), ("taps", C.c_uint32),
                ("seed", C.c_uint32), ("flags", C.c_uint32)]


class DofStats(C.Structure):  # pt_dof_stats
    _fields_ = [("pixels", C.c_uint64), ("sources", C.c_uint64), ("gathered", C.c_uint64), ("taps", C.c_uint64), ("nonfinite", C.c_uint64),
                ("kernel_ms", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


# the frame-sized planes of pt_dof_planes: 32-bit words per pixel (the scratch, T and N of every view, is pt_dof_layout's)
DOF_PLANES = {"color": 4, "depth": 1, "out": 4}
DOF_OUTPUTS = ("out",)


PT_LENS_WARP_BICUBIC = 1  # pt_lens_warp_flags


class LensView(C.Structure):  # pt_lens_view
    _fields_ = [("center", C.c_float * 2), ("inv_radius", C.c_float * 2), ("k", (C.c_float * 3) * 3), ("warp", C.c_float * 9),
                ("reserved", C.c_float * 2)]


class LensWarpDesc(C.Structure):  # pt_lens_warp_desc
    _fields_ = [("color", C.c_void_p), ("out", C.c_void_p), ("frame_rgba8", C.c_void_p), ("block_mask", C.c_void_p), ("lenses", C.c_void_p),
                ("border", C.c_float * 3), ("flags", C.c_uint32)]


class LensWarpStats(C.Structure):  # pt_lens_warp_stats
    _fields_ = [("pixels", C.c_uint64), ("outside", C.c_uint64), ("nonfinite", C.c_uint64), ("kernel_ms", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


# the planes of pt_lens_warp_planes: 32-bit words per pixel (frame_rgba8 holds packed bytes, the others float32)
LENS_WARP_PLANES = {"color": 4, "out": 4, "frame_rgba8": 1}
LENS_WARP_OUTPUTS = ("out", "frame_rgba8")


PT_AO_MAX_RAYS = 32
PT_AO_DEFAULT_RAYS_IN_FLIGHT = 1 << 23
PT_AO_JITTER = 1  # pt_ao_flags


class AoDesc(C.Structure):  # pt_ao_desc
    _fields_ = [("hit", C.c_void_p), ("position", C.c_void_p), ("ao", C.c_void_p), ("out", C.c_void_p), ("bent", C.c_void_p),
                ("scratch", C.c_void_p), ("block_mask", C.c_void_p), ("rays", C.c_uint32), ("max_rays_in_flight", C.c_uint32),
                ("radius", C.c_float), ("bias", C.c_float), ("seed", C.c_uint32), ("flags", C.c_uint32)]


class AoStats(C.Structure):  # pt_ao_stats
    _fields_ = [("pixels", C.c_uint64), ("traced", C.c_uint64), ("skipped", C.c_uint64), ("nonfinite", C.c_uint64), ("rays", C.c_uint64),
                ("occluded", C.c_uint64), ("invalid", C.c_uint64), ("batches", C.c_uint64), ("kernel_ms", C.c_double), ("trace_ms", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


# the frame-sized planes of pt_ao_planes: 32-bit words per pixel (the scratch, one batch of rays, is pt_ao_layout's)
AO_PLANES = {"hit": 8, "position": 4, "ao": 1, "out": 4, "bent": 4}
AO_OUTPUTS = ("ao", "out", "bent")


PT_REFLECT_DEFAULT_RAYS_IN_FLIGHT = 1 << 23


class ReflectDesc(C.Structure):  # pt_reflect_desc
    _fields_ = [("hit", C.c_void_p), ("position", C.c_void_p), ("hit2", C.c_void_p), ("position2", C.c_void_p), ("ray", C.c_void_p),
                ("sky", C.c_void_p), ("scratch", C.c_void_p), ("block_mask", C.c_void_p), ("bias", C.c_float), ("max_distance", C.c_float),
                ("max_rays_in_flight", C.c_uint32), ("flags", C.c_uint32)]


class ReflectStats(C.Structure):  # pt_reflect_stats
    _fields_ = [("pixels", C.c_uint64), ("traced", C.c_uint64), ("skipped", C.c_uint64), ("nonfinite", C.c_uint64), ("invalid", C.c_uint64),
                ("hits", C.c_uint64), ("escaped", C.c_uint64), ("batches", C.c_uint64), ("kernel_ms", C.c_double), ("trace_ms", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


# the frame-sized planes of pt_reflect_planes: 32-bit words per pixel (the scratch, one batch of rays, is pt_reflect_layout's)
REFLECT_PLANES = {"hit": 8, "position": 4, "hit2": 8, "position2": 4, "ray": 8, "sky": 4}
REFLECT_OUTPUTS = ("hit2", "position2", "ray", "sky")


PT_SHADOW_MAX_LIGHTS = 4
PT_SHADOW_MAX_RAYS = 32  # the sum of the lights' rays
PT_SHADOW_DEFAULT_RAYS_IN_FLIGHT = 1 << 23
PT_SHADOW_JITTER = 1  # pt_shadow_flags


class ShadowLight(C.Structure):  # pt_shadow_light
    _fields_ = [("dir", C.c_float * 3), ("spread", C.c_float), ("radiance", C.c_float * 3), ("rays", C.c_uint32)]


class ShadowDesc(C.Structure):  # pt_shadow_desc
    _fields_ = [("hit", C.c_void_p), ("position", C.c_void_p), ("view_ray", C.c_void_p), ("visibility", C.c_void_p), ("light", C.c_void_p),
                ("scratch", C.c_void_p), ("block_mask", C.c_void_p), ("lights", C.c_void_p), ("num_lights", C.c_uint32),
                ("max_rays_in_flight", C.c_uint32), ("max_distance", C.c_float), ("bias", C.c_float), ("seed", C.c_uint32), ("flags", C.c_uint32)]


class ShadowStats(C.Structure):  # pt_shadow_stats
    _fields_ = [("pixels", C.c_uint64), ("traced", C.c_uint64), ("skipped", C.c_uint64), ("nonfinite", C.c_uint64), ("backfacing", C.c_uint64),
                ("rays", C.c_uint64), ("occluded", C.c_uint64), ("invalid", C.c_uint64), ("batches", C.c_uint64), ("kernel_ms", C.c_double),
                ("trace_ms", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


# the frame-sized planes of pt_shadow_planes: 32-bit words per pixel (the scratch, one batch of rays, is pt_shadow_layout's)
SHADOW_PLANES = {"hit": 8, "position": 4, "view_ray": 8, "visibility": 4, "light": 4}
SHADOW_OUTPUTS = ("visibility", "light")


PT_TMOM_CLEAR_COLOR, PT_TMOM_CLAMP = 1, 2  # pt_tmom_flags


class TMomDesc(C.Structure):  # pt_tmom_desc
    _fields_ = [("color", C.c_void_p), ("albedo", C.c_void_p), ("motion", C.c_void_p), ("hit", C.c_void_p), ("position", C.c_void_p),
                ("prev_hit", C.c_void_p), ("prev_position", C.c_void_p), ("history_in", C.c_void_p), ("moments_in", C.c_void_p),
                ("length_in", C.c_void_p), ("history_out", C.c_void_p), ("moments_out", C.c_void_p), ("length_out", C.c_void_p),
                ("variance_out", C.c_void_p), ("block_mask", C.c_void_p),
                ("color_scale", C.c_float), ("albedo_min", C.c_float), ("normal_cos", C.c_float), ("plane_eps", C.c_float),
                ("min_weight", C.c_float), ("clamp_k", C.c_float), ("max_history", C.c_uint32), ("flags", C.c_uint32)]


class TMomStats(C.Structure):  # pt_tmom_stats
    _fields_ = [("pixels", C.c_uint64), ("reprojected", C.c_uint64), ("clamped", C.c_uint64), ("kernel_ms", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


# the planes of pt_temporal_moments: float32 words per pixel
TMOM_PLANES = {"color": 4, "albedo": 4, "motion": 2, "hit": 8, "position": 4, "prev_hit": 8, "prev_position": 4, "history_in": 4,
               "moments_in": 2, "length_in": 1, "history_out": 4, "moments_out": 2, "length_out": 1, "variance_out": 1}
TMOM_OUTPUTS = ("history_out", "moments_out", "length_out", "variance_out")


class ModulateDesc(C.Structure):  # pt_modulate_desc
    _fields_ = [("color", C.c_void_p), ("albedo", C.c_void_p), ("out", C.c_void_p), ("frame_rgba8", C.c_void_p), ("block_mask", C.c_void_p),
                ("albedo_min", C.c_float), ("flags", C.c_uint32)]


class ModulateStats(C.Structure):  # pt_modulate_stats
    _fields_ = [("pixels", C.c_uint64), ("kernel_ms", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


# the planes of pt_modulate_planes: 32-bit words per pixel (frame_rgba8 holds packed bytes, the others float32)
MODULATE_PLANES = {"color": 4, "albedo": 4, "out": 4, "frame_rgba8": 1}
MODULATE_OUTPUTS = ("out", "frame_rgba8")


class PlanDesc(C.Structure):  # pt_plan_desc
    _fields_ = [("motion", C.c_void_p), ("hit", C.c_void_p), ("position", C.c_void_p), ("prev_hit", C.c_void_p), ("prev_position", C.c_void_p),
                ("history_in", C.c_void_p), ("moments_in", C.c_void_p), ("length_in", C.c_void_p), ("block_mask", C.c_void_p),
                ("block_mask_out", C.c_void_p),
                ("normal_cos", C.c_float), ("plane_eps", C.c_float), ("min_weight", C.c_float), ("threshold", C.c_float), ("dark_floor", C.c_float),
                ("min_length", C.c_uint32), ("min_pixels", C.c_uint32), ("refresh_period", C.c_uint32), ("frame_index", C.c_uint32),
                ("flags", C.c_uint32)]


class PlanStats(C.Structure):  # pt_plan_stats
    _fields_ = [("blocks", C.c_uint64), ("sampled", C.c_uint64), ("by_lost", C.c_uint64), ("by_need", C.c_uint64), ("by_refresh", C.c_uint64),
                ("pixels", C.c_uint64), ("lost", C.c_uint64), ("needy", C.c_uint64), ("kernel_ms", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class CarryDesc(C.Structure):  # pt_carry_desc
    _fields_ = [("motion", C.c_void_p), ("hit", C.c_void_p), ("position", C.c_void_p), ("prev_hit", C.c_void_p), ("prev_position", C.c_void_p),
                ("history_in", C.c_void_p), ("moments_in", C.c_void_p), ("length_in", C.c_void_p), ("history_out", C.c_void_p),
                ("moments_out", C.c_void_p), ("length_out", C.c_void_p), ("variance_out", C.c_void_p), ("block_mask", C.c_void_p),
                ("normal_cos", C.c_float), ("plane_eps", C.c_float), ("min_weight", C.c_float), ("flags", C.c_uint32)]


class CarryStats(C.Structure):  # pt_carry_stats
    _fields_ = [("pixels", C.c_uint64), ("carried", C.c_uint64), ("lost", C.c_uint64), ("kernel_ms", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


# the planes of pt_sample_plan and pt_temporal_carry: float32 words per pixel
PLAN_PLANES = {"motion": 2, "hit": 8, "position": 4, "prev_hit": 8, "prev_position": 4, "history_in": 4, "moments_in": 2, "length_in": 1}
CARRY_PLANES = dict(PLAN_PLANES, history_out=4, moments_out=2, length_out=1, variance_out=1)
CARRY_OUTPUTS = ("history_out", "moments_out", "length_out", "variance_out")


class AdaptiveParams(C.Structure):  # pt_adaptive_params
    _fields_ = [("threshold", C.c_float), ("dark_floor", C.c_float), ("min_subframes", C.c_uint32), ("max_subframes", C.c_uint32)]


class AdaptiveStats(C.Structure):  # pt_adaptive_stats
    _fields_ = [("blocks", C.c_uint32), ("active_blocks", C.c_uint32), ("active_pixels", C.c_uint64), ("pixel_subframes", C.c_uint64),
                ("decide_ms", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class MeshUpdate(C.Structure):  # pt_mesh_update
    _fields_ = [("mesh", C.c_uint32), ("vertex", C.POINTER(C.c_float)), ("num_vertices", C.c_uint32)]


class MeshTransform(C.Structure):  # pt_mesh_transform
    _fields_ = [("mesh", C.c_uint32), ("m", C.c_float * 12)]


class DenoiseParams(C.Structure):  # pt_denoise_params
    _fields_ = [("iterations", C.c_int32), ("sigma_color", C.c_float), ("sigma_normal", C.c_float), ("sigma_albedo", C.c_float),
                ("input", C.c_int32), ("epilogue", C.c_int32)]


class Material(C.Structure):  # pt_material == Material.h:47-68
    _fields_ = [
        ("emission", C.c_float * 3), ("color", C.c_float * 3), ("absorption", C.c_float * 3),
        ("eta", C.c_float), ("metallic", C.c_float), ("subsurface", C.c_float), ("specular", C.c_float),
        ("roughness", C.c_float), ("specularTint", C.c_float), ("anisotropic", C.c_float), ("sheen", C.c_float),
        ("sheenTint", C.c_float), ("clearcoat", C.c_float), ("clearcoatGloss", C.c_float), ("transmission", C.c_float),
        ("bump", C.c_float), ("bumpTile", C.c_float * 3), ("flags", C.c_int32),
    ]


class ObjMesh(C.Structure):  # pt_obj_mesh
    _fields_ = [
        ("vertex", C.POINTER(C.c_float)), ("normal", C.POINTER(C.c_float)), ("texcoord", C.POINTER(C.c_float)), ("index", C.POINTER(C.c_uint32)),
        ("num_vertices", C.c_uint32), ("num_triangles", C.c_uint32), ("material", Material), ("texture_ref", C.c_int32),
    ]


class MeshDesc(C.Structure):
    _fields_ = [
        ("vertex", C.c_void_p), ("num_vertices", C.c_uint32), ("index", C.c_void_p), ("num_triangles", C.c_uint32),
        ("material", Material), ("diffuse_texture_id", C.c_int32), ("texcoord", C.c_void_p),
    ]


class TextureDesc(C.Structure):
    _fields_ = [("pixel", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32)]


class SceneDesc(C.Structure):
    _fields_ = [("meshes", C.POINTER(MeshDesc)), ("num_meshes", C.c_uint32), ("textures", C.POINTER(TextureDesc)), ("num_textures", C.c_uint32)]


class Options(C.Structure):
    _fields_ = [
        ("max_depth", C.c_int32), ("bsdf_mode", C.c_int32), ("max_paths", C.c_uint32), ("kernel_timing", C.c_int32),
        ("bvh_kind", C.c_int32), ("trace_kernel", C.c_int32), ("streams", C.c_int32), ("split_shadow", C.c_int32),
        ("frames_in_flight", C.c_int32),
    ]


class Region(C.Structure):  # pt_region
    _fields_ = [
        ("launch_w", C.c_uint32), ("launch_h", C.c_uint32), ("factor_x", C.c_uint32), ("factor_y", C.c_uint32),
        ("fill_size", C.c_int32), ("cx", C.c_uint32), ("cy", C.c_uint32), ("r_inner", C.c_float), ("r_outer", C.c_float),
        ("offset_x", C.c_uint32), ("offset_y", C.c_uint32), ("redraw", C.c_uint32), ("spp", C.c_uint32), ("subframe_index", C.c_uint32),
    ]


class Variant(C.Structure):  # pt_variant
    _fields_ = [("radiance_tmin", C.c_float), ("cull_back_occlusion", C.c_int32), ("tonemap", C.c_int32), ("exposure", C.c_float), ("white", C.c_float),
                ("initial_depth", C.c_int32), ("write_aov", C.c_int32)]


class Stats(C.Structure):
    _fields_ = [
        ("radiance_rays", C.c_uint64), ("shadow_rays", C.c_uint64), ("paths", C.c_uint64),
        ("render_ms", C.c_double), ("trace_ms", C.c_double), ("shadow_ms", C.c_double), ("shade_ms", C.c_double),
        ("other_ms", C.c_double),
        ("trace_launches", C.c_uint32), ("shadow_launches", C.c_uint32), ("shade_launches", C.c_uint32),
        ("bvh_nodes", C.c_uint32), ("bvh_bytes", C.c_uint64), ("bvh_build_ms", C.c_double), ("bvh_levels", C.c_uint32), ("shaded_hits", C.c_uint64),
        ("frames", C.c_uint64), ("total_radiance_rays", C.c_uint64), ("total_shadow_rays", C.c_uint64),
        ("bvh_builder", C.c_uint32), ("fused_passes", C.c_uint32), ("path_state_allocs", C.c_uint32),
        ("bvh_challengers_skipped", C.c_uint32), ("schedule", C.c_uint32), ("sched_chain_ms", C.c_double), ("sched_fused_ms", C.c_double), ("create_ms", C.c_double),
        ("marg_lds_words_full", C.c_uint32), ("marg_lds_words_lean", C.c_uint32),
    ]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class MultiStats(C.Structure):  # pt_multi_stats
    _fields_ = [("sum", Stats), ("gather_ms", C.c_double), ("exchange", C.c_int32), ("ndev", C.c_int32), ("enqueue_ms", C.c_double), ("threads", C.c_int32),
                ("frames_handed_over", C.c_uint64)]


assert C.sizeof(Material) == 104
assert C.sizeof(Hit) == 32 == HIT_DTYPE.itemsize

_lib = None


def build_library(force: bool = False) -> str:
    """Compile libptamd.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    srcdir = os.path.join(HERE, "csrc")
    if force:
        subprocess.check_call(["make", "-C", srcdir, "clean"], stdout=subprocess.DEVNULL)
    subprocess.check_call(["make", "-C", srcdir, "-j2"], stdout=subprocess.DEVNULL)
    return LIB_PATH


def load_library() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C optixpathtracer_amd/csrc`). There is no CPU fallback for the render path."
        )
    # One HIP runtime per process: the PyTorch-ROCm wheel bundles its own libamdhip64 (same SONAME as
    # /opt/rocm's).  If torch is importable, load it first so that libptamd binds to the runtime torch will
    # use for device tensors / RCCL later in the same process (the other order leaves torch without devices).
    try:
        import torch  # noqa: F401
    except Exception:
        pass
    L = C.CDLL(LIB_PATH)
    for name in EXPORTS:
        if not hasattr(L, name):
            raise RuntimeError(f"libptamd.so does not export {name}")
    vp, i, u32, f = C.c_void_p, C.c_int, C.c_uint32, C.c_float
    L.pt_create.argtypes = [C.POINTER(SceneDesc), i, C.POINTER(vp)]
    L.pt_destroy.argtypes = [vp]
    L.pt_last_error.restype = C.c_char_p
    L.pt_last_error.argtypes = [vp]
    L.pt_set_options.argtypes = [vp, C.POINTER(Options)]
    L.pt_get_options.argtypes = [vp, C.POINTER(Options)]
    L.pt_set_probe.argtypes = [vp, vp, vp, vp, vp, vp, i, i]
    L.pt_build_cdf.argtypes = [vp, i, i, vp, vp, vp, vp]
    L.pt_set_probe_image.argtypes = [vp, vp, i, i]
    L.pt_get_probe_cdf.argtypes = [vp, vp, vp, vp, vp]
    L.pt_resize.argtypes = [vp, i, i]
    L.pt_set_camera.argtypes = [vp, C.POINTER(f * 3), C.POINTER(f * 3), C.POINTER(f * 3), C.POINTER(f * 3)]
    L.pt_uvw_frame.argtypes = [C.POINTER(f * 3), C.POINTER(f * 3), C.POINTER(f * 3), f, f, C.POINTER(f * 3), C.POINTER(f * 3), C.POINTER(f * 3)]
    L.pt_set_partition.argtypes = [vp, i, i, i, i]
    L.pt_render.argtypes = [vp, u32, u32, vp]
    L.pt_render_batch.argtypes = [vp, u32, u32, u32, vp]
    L.pt_sync.argtypes = [vp]
    L.pt_render_device.argtypes = [vp, u32, u32, vp]
    L.pt_load_obj.argtypes = [C.c_char_p, i, C.POINTER(vp)]
    L.pt_obj_free.argtypes = [vp]
    L.pt_obj_free.restype = None
    L.pt_obj_num_meshes.argtypes = [vp]
    L.pt_obj_num_meshes.restype = u32
    L.pt_obj_get_mesh.argtypes = [vp, u32, C.POINTER(ObjMesh)]
    L.pt_obj_num_textures.argtypes = [vp]
    L.pt_obj_num_textures.restype = u32
    L.pt_obj_texture_path.argtypes = [vp, u32]
    L.pt_obj_texture_path.restype = C.c_char_p
    L.pt_obj_last_error.restype = C.c_char_p
    L.pt_stream.restype = vp
    L.pt_stream.argtypes = [vp]
    L.pt_wait_event.argtypes = [vp, vp]
    L.pt_get_stats_n.argtypes = [vp, vp, C.c_size_t]
    L.pt_stats_size.restype = C.c_size_t
    L.pt_render_regions.argtypes = [vp, C.POINTER(Region), u32, C.POINTER(Variant), vp]
    L.pt_download.argtypes = [vp, i, vp, C.c_size_t]
    L.pt_upload_accum.argtypes = [vp, vp, C.c_size_t]
    L.pt_device_buffer.restype = vp
    L.pt_device_buffer.argtypes = [vp, i]
    L.pt_tonemap_sqrt.argtypes = [vp, vp]
    L.pt_denoise.argtypes = [vp, C.POINTER(DenoiseParams), vp, C.POINTER(C.c_double)]
    L.pt_owned_pixels.argtypes = [vp, C.POINTER(u32), C.POINTER(u32)]
    L.pt_pack.argtypes = [vp, i, vp]
    L.pt_unpack.argtypes = [vp, i, vp]
    L.pt_get_stats.argtypes = [vp, C.POINTER(Stats)]
    L.pt_pack_async.argtypes = [vp, i, vp, i]
    L.pt_pack_wait.argtypes = [vp, i]
    L.pt_unpack_display.argtypes = [vp, i, vp]
    L.pt_display_sync.argtypes = [vp]
    L.pt_display_buffer.restype = vp
    L.pt_display_buffer.argtypes = [vp, i]
    L.pt_download_display.argtypes = [vp, i, vp, C.c_size_t]
    L.pt_trace.argtypes = [vp, vp, u32, i, vp, vp, i, C.POINTER(C.c_double)]
    L.pt_eval_table.argtypes = [vp, i, vp, i, vp, u32, vp]
    L.pt_export_bvh.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, C.POINTER(u32), C.POINTER(u32)]
    L.pt_update_meshes.argtypes = [vp, C.POINTER(MeshUpdate), u32, i, C.POINTER(C.c_double)]
    L.pt_multi_update_meshes.argtypes = [vp, C.POINTER(MeshUpdate), u32, i, C.POINTER(C.c_double)]
    L.pt_update_meshes_device.argtypes = [vp, C.POINTER(MeshUpdate), u32, i, C.POINTER(C.c_double)]
    L.pt_transform_meshes.argtypes = [vp, C.POINTER(MeshTransform), u32, i, i, C.POINTER(C.c_double)]
    L.pt_multi_transform_meshes.argtypes = [vp, C.POINTER(MeshTransform), u32, i, i, C.POINTER(C.c_double)]
    L.pt_download_vertices.argtypes = [vp, u32, i, vp, C.c_size_t]
    L.pt_render_mask.argtypes = [vp, u32, u32, vp, vp, C.POINTER(u32)]
    L.pt_adaptive_begin.argtypes = [vp, C.POINTER(AdaptiveParams)]
    L.pt_render_adaptive.argtypes = [vp, u32, u32, vp, C.POINTER(AdaptiveStats)]
    L.pt_adaptive_end.argtypes = [vp]
    L.pt_download_adaptive.argtypes = [vp, i, vp, C.c_size_t]
    L.pt_trace_device.argtypes = [vp, vp, u32, u32, vp, C.POINTER(QueryStats)]
    L.pt_query_wait.argtypes = [vp, C.POINTER(QueryStats)]
    L.pt_render_gbuffer.argtypes = [vp, C.POINTER(GBufferDesc), C.POINTER(GBufferStats)]
    L.pt_temporal_accumulate.argtypes = [vp, C.POINTER(TemporalDesc), C.POINTER(TemporalStats)]
    L.pt_filter_planes.argtypes = [vp, C.POINTER(FilterDesc), C.POINTER(FilterStats)]
    L.pt_vertex_count.argtypes = [vp, C.POINTER(u32), C.POINTER(u32)]
    L.pt_copy_vertices_device.argtypes = [vp, vp, C.c_size_t]
    L.pt_motion_planes.argtypes = [vp, C.POINTER(MotionDesc), C.POINTER(MotionStats)]
    L.pt_copy_texcoords_device.argtypes = [vp, vp, C.c_size_t]
    L.pt_surface_planes.argtypes = [vp, C.POINTER(SurfaceDesc), C.POINTER(SurfaceStats)]
    L.pt_texture_mips_layout.argtypes = [vp, C.POINTER(u32), vp, C.POINTER(C.c_size_t)]
    L.pt_copy_texture_mips_device.argtypes = [vp, vp, C.c_size_t]
    L.pt_surface_lod_planes.argtypes = [vp, C.POINTER(SurfaceLodDesc), C.POINTER(SurfaceLodStats)]
    L.pt_surface_aniso_planes.argtypes = [vp, C.POINTER(SurfaceAnisoDesc), C.POINTER(SurfaceAnisoStats)]
    L.pt_upsample_planes.argtypes = [vp, C.POINTER(UpsampleDesc), C.POINTER(UpsampleStats)]
    L.pt_edge_aa_planes.argtypes = [vp, C.POINTER(EdgeAaDesc), C.POINTER(EdgeAaStats)]
    L.pt_exposure_planes.argtypes = [vp, C.POINTER(ExposureDesc), C.POINTER(ExposureStats)]
    L.pt_tonemap_planes.argtypes = [vp, C.POINTER(TonemapDesc), C.POINTER(TonemapStats)]
    L.pt_bloom_layout.argtypes = [vp, u32, vp, C.POINTER(C.c_size_t)]
    L.pt_bloom_planes.argtypes = [vp, C.POINTER(BloomDesc), C.POINTER(BloomStats)]
    L.pt_motion_blur_layout.argtypes = [vp, vp, C.POINTER(C.c_size_t)]
    L.pt_motion_blur_planes.argtypes = [vp, C.POINTER(MotionBlurDesc), C.POINTER(MotionBlurStats)]
    L.pt_dof_layout.argtypes = [vp, vp, C.POINTER(C.c_size_t)]
    L.pt_dof_planes.argtypes = [vp, C.POINTER(DofDesc), C.POINTER(DofStats)]
    L.pt_lens_warp_planes.argtypes = [vp, C.POINTER(LensWarpDesc), C.POINTER(LensWarpStats)]
    L.pt_warp_matrix.argtypes = [vp, vp, u32, u32, vp]
    L.pt_ao_layout.argtypes = [vp, u32, u32, C.POINTER(C.c_size_t)]
    L.pt_ao_planes.argtypes = [vp, C.POINTER(AoDesc), C.POINTER(AoStats)]
    L.pt_reflect_layout.argtypes = [vp, u32, C.POINTER(C.c_size_t)]
    L.pt_reflect_planes.argtypes = [vp, C.POINTER(ReflectDesc), C.POINTER(ReflectStats)]
    L.pt_shadow_layout.argtypes = [vp, C.POINTER(ShadowLight), u32, u32, C.POINTER(C.c_size_t)]
    L.pt_shadow_planes.argtypes = [vp, C.POINTER(ShadowDesc), C.POINTER(ShadowStats)]
    L.pt_temporal_moments.argtypes = [vp, C.POINTER(TMomDesc), C.POINTER(TMomStats)]
    L.pt_modulate_planes.argtypes = [vp, C.POINTER(ModulateDesc), C.POINTER(ModulateStats)]
    L.pt_sample_plan.argtypes = [vp, C.POINTER(PlanDesc), C.POINTER(PlanStats)]
    L.pt_temporal_carry.argtypes = [vp, C.POINTER(CarryDesc), C.POINTER(CarryStats)]
    L.pt_set_views.argtypes = [vp, C.POINTER(View), u32]
    L.pt_get_views.argtypes = [vp, C.POINTER(View), u32, C.POINTER(u32)]
    L.pt_set_view_cameras.argtypes = [vp, vp, u32]
    L.pt_set_view_cameras_device.argtypes = [vp, vp, u32]
    L.pt_multi_set_views.argtypes = [vp, C.POINTER(View), u32]
    L.pt_multi_set_view_cameras.argtypes = [vp, vp, u32]
    L.pt_version.restype = C.c_char_p
    f3p = C.POINTER(f * 3)
    L.pt_create_multi.argtypes = [C.POINTER(SceneDesc), C.POINTER(C.c_int), i, C.POINTER(vp)]
    L.pt_multi_destroy.argtypes = [vp]
    L.pt_multi_last_error.restype = C.c_char_p
    L.pt_multi_last_error.argtypes = [vp]
    L.pt_multi_size.argtypes = [vp]
    L.pt_multi_ctx.restype = vp
    L.pt_multi_ctx.argtypes = [vp, i]
    L.pt_multi_set_options.argtypes = [vp, C.POINTER(Options)]
    L.pt_multi_set_probe.argtypes = [vp, vp, vp, vp, vp, vp, i, i]
    L.pt_multi_set_probe_image.argtypes = [vp, vp, i, i]
    L.pt_multi_resize.argtypes = [vp, i, i, i, i]
    L.pt_multi_set_camera.argtypes = [vp, f3p, f3p, f3p, f3p]
    L.pt_multi_render.argtypes = [vp, u32, u32, u32, vp]
    L.pt_multi_render_batch.argtypes = [vp, u32, u32, u32, u32, vp]
    L.pt_multi_render_regions.argtypes = [vp, C.POINTER(Region), u32, C.POINTER(Variant), u32, vp]
    L.pt_multi_gather.argtypes = [vp, i]
    L.pt_multi_flush.argtypes = [vp, vp]
    L.pt_multi_get_stats.argtypes = [vp, C.POINTER(MultiStats)]
    _lib = L
    return L


def build_cdf(data: np.ndarray, width: int, height: int):
    """ProbeData::BuildCDF through the native host implementation (pt_build_cdf)."""
    L = load_library()
    data = np.ascontiguousarray(data, np.float32)
    pdfX = np.empty((height, width), np.float32)
    cdfX = np.empty((height, width), np.float32)
    pdfY = np.empty(height, np.float32)
    cdfY = np.empty(height, np.float32)
    rc = L.pt_build_cdf(data.ctypes.data, width, height, pdfX.ctypes.data, cdfX.ctypes.data, pdfY.ctypes.data, cdfY.ctypes.data)
    if rc:
        raise RuntimeError(f"pt_build_cdf failed ({rc})")
    return pdfX, cdfX, pdfY, cdfY
