"""Host-side mirror of the reference's library API over the C ABI of libbendy_hip.so.

The reference is a Rust crate; `src/main.rs` drives it through `Scene`, `Tracer`,
`Config`, `RenderConfig`, `Subsample`, `Output`, `Status`, `Buffer`, `ColorSpace`
(tracer/mod.rs:16-203, tracer/buffer.rs:11-179, scene/mod.rs:84-146).  Rust is not
available in this image, so this module re-exposes the same names, argument meaning and
error behaviour in Python (panics become exceptions), calling the HIP implementation
through `include/bendy_hip.h`.  There is NO CPU fallback: importing this module fails if
the shared library has not been built, and rendering fails without a gfx950 device.
"""
from __future__ import annotations

import ctypes as C
import enum
import os
from dataclasses import dataclass
from typing import Optional

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libbendy_hip.so")
BT_TILE = 16


class BendyError(RuntimeError):
    """A reference panic / serde error, surfaced as a negative bt_status."""

    def __init__(self, code, message):
        super().__init__(f"[bt_status {code}] {message}")
        self.code = code


class Output(enum.IntEnum):  # tracer/mod.rs:108-115
    Full = 0
    Albedo = 1
    Normal = 2
    Depth = 3


class ColorSpace(enum.IntEnum):  # tracer/buffer.rs:11-17
    NONE = 0
    Normal = 1
    Linear = 2
    SRgb = 3


class Tonemap(enum.IntEnum):  # include/bendy_hip.h `bt_tonemap` (extension)
    Clip = 0
    Reinhard = 1
    Aces = 2


class Filter(enum.IntEnum):  # include/bendy_hip.h `bt_resample_filter` (extension)
    Box = 0
    Tent = 1
    Mitchell = 2
    Lanczos3 = 3


class Status(enum.IntEnum):  # tracer/mod.rs:159-163
    Done = 0
    InProgress = 1


@dataclass(frozen=True)
class Subsample:  # tracer/mod.rs:47-106
    n: int = 0  # 0 = Subsample::None, n = Subsample::Subpixel(n)

    @staticmethod
    def none():
        return Subsample(0)

    @staticmethod
    def subpixel(n):
        return Subsample(int(n))

    def subpixel_size(self):  # :55-60
        return 1.0 if self.n == 0 else float(np.float32(1.0) / np.float32(self.n))

    def subpixel_count(self):  # :62-67
        return 1 if self.n == 0 else self.n * self.n

    def __iter__(self):  # :87-106: (i/n, j/n), i fastest
        if self.n == 0:
            yield (0.0, 0.0)
            return
        w = np.float32(1.0) / np.float32(self.n)
        for c in range(self.n * self.n):
            yield (float(np.float32(c % self.n) * w), float(np.float32(c // self.n) * w))


@dataclass
class Config:  # tracer/mod.rs:16-45
    max_bounces: int = 8
    max_volume_bounces: int = 32
    clip_min: float = 0.01
    clip_max: float = 1000.0
    volume_step: float = 0.1
    chunks_x: int = 4
    chunks_y: int = 2
    output: Output = Output.Full


@dataclass
class RenderConfig:  # tracer/mod.rs:117-157
    subsample: Subsample = Subsample(0)
    samples: int = 64
    output: Optional[Output] = None
    max_bounces: Optional[int] = None
    max_volume_bounces: Optional[int] = None
    volume_step: Optional[float] = None

    @staticmethod
    def with_samples(samples):  # :137-142
        return RenderConfig(samples=samples)

    @staticmethod
    def with_samples_subsample(samples, subsample):  # :144-150
        return RenderConfig(samples=samples, subsample=subsample)


class _CConfig(C.Structure):
    _fields_ = [("max_bounces", C.c_uint32), ("max_volume_bounces", C.c_uint32), ("clip_min", C.c_float),
                ("clip_max", C.c_float), ("volume_step", C.c_float), ("chunks_x", C.c_uint32),
                ("chunks_y", C.c_uint32), ("output", C.c_int32)]


class _CRenderConfig(C.Structure):
    _fields_ = [("subsample_n", C.c_uint32), ("samples", C.c_uint32), ("has_output", C.c_int32),
                ("output", C.c_int32), ("has_max_bounces", C.c_int32), ("max_bounces", C.c_uint32),
                ("has_max_volume_bounces", C.c_int32), ("max_volume_bounces", C.c_uint32),
                ("has_volume_step", C.c_int32), ("volume_step", C.c_float), ("sample_base", C.c_uint32)]


class Stats(C.Structure):
    _fields_ = [("samples", C.c_uint64), ("segments", C.c_uint64), ("pixels", C.c_uint64), ("kernel_ms", C.c_float),
                ("lens_steps", C.c_uint64), ("slices", C.c_uint32), ("launches", C.c_uint32),
                ("scratch_bytes", C.c_uint64), ("parked_bytes", C.c_uint64), ("workgroups", C.c_uint32), ("packed", C.c_uint32)]


class _CTuning(C.Structure):  # include/bendy_hip.h `bt_tuning`
    _fields_ = [("slices", C.c_uint32), ("phase_vote", C.c_int32), ("scratch_cap_bytes", C.c_uint64), ("packed", C.c_int32),
                ("reserved", C.c_int32)]


class _CDenoiseParams(C.Structure):  # include/bendy_hip.h `bt_denoise_params` (extension)
    _fields_ = [("levels", C.c_uint32), ("sigma_color", C.c_float), ("sigma_normal", C.c_float), ("sigma_depth", C.c_float),
                ("eps_albedo", C.c_float)]


class _CAdaptiveParams(C.Structure):  # include/bendy_hip.h `bt_adaptive_params` (extension)
    _fields_ = [("threshold", C.c_float), ("min_samples", C.c_uint32), ("max_samples", C.c_uint32), ("eps", C.c_float)]


class AdaptiveStats(C.Structure):  # include/bendy_hip.h `bt_adaptive_stats` (extension)
    _fields_ = [("active_tiles", C.c_uint32), ("tiles", C.c_uint32), ("min_count", C.c_uint32), ("max_count", C.c_uint32),
                ("pixel_samples", C.c_uint64), ("passes", C.c_uint32), ("reserved", C.c_uint32)]


class View(C.Structure):  # include/bendy_hip.h `bt_view` (extension): the camera as data
    _fields_ = [("to_world", C.c_float * 12), ("yfov", C.c_float), ("xfov", C.c_float), ("clip_min", C.c_float),
                ("clip_max", C.c_float), ("width", C.c_uint32), ("height", C.c_uint32), ("subsample_n", C.c_uint32)]

    def copy(self):
        return View.from_buffer_copy(self)

    def matrix(self):
        """to_world as float32 [12]: columns x, y, z, then the translation."""
        return np.array(self.to_world, dtype=np.float32)


class _CTemporalParams(C.Structure):  # include/bendy_hip.h `bt_temporal_params` (extension)
    _fields_ = [("alpha_min", C.c_float), ("max_history", C.c_float), ("depth_tolerance", C.c_float), ("normal_min", C.c_float)]


class _CDisplayParams(C.Structure):  # include/bendy_hip.h `bt_display_params` (extension)
    _fields_ = [("key", C.c_double), ("tonemap", C.c_int32), ("auto_exposure", C.c_int32), ("ev", C.c_float), ("p_low", C.c_float),
                ("p_high", C.c_float), ("adapt", C.c_float), ("ev_min", C.c_float), ("ev_max", C.c_float), ("white", C.c_float)]


class _CGlareParams(C.Structure):  # include/bendy_hip.h `bt_glare_params` (extension)
    _fields_ = [("levels", C.c_uint32), ("spread", C.c_float), ("strength", C.c_float), ("max_value", C.c_float)]


class _CResampleParams(C.Structure):  # include/bendy_hip.h `bt_resample_params` (extension)
    _fields_ = [("filter", C.c_int32), ("max_value", C.c_float), ("clamp_negative", C.c_int32)]


class _CDespeckleParams(C.Structure):  # include/bendy_hip.h `bt_despeckle_params` (extension)
    _fields_ = [("radius", C.c_uint32), ("rank", C.c_uint32), ("ratio", C.c_float), ("floor", C.c_float), ("max_value", C.c_float)]


class DespeckleStats(C.Structure):  # include/bendy_hip.h `bt_despeckle_stats` (extension)
    _fields_ = [("flagged", C.c_uint32), ("sanitised", C.c_uint32), ("pixels", C.c_uint32), ("reserved", C.c_uint32)]


class _CUpscaleParams(C.Structure):  # include/bendy_hip.h `bt_upscale_params` (extension)
    _fields_ = [("sigma_depth", C.c_float), ("sigma_albedo", C.c_float), ("normal_squarings", C.c_uint32), ("min_weight", C.c_float),
                ("max_value", C.c_float)]


class _CUpscaleGuides(C.Structure):  # include/bendy_hip.h `bt_upscale_guides` (extension)
    _fields_ = [("albedo", C.c_void_p), ("albedo_samples", C.c_uint32), ("normal", C.c_void_p), ("normal_samples", C.c_uint32),
                ("depth", C.c_void_p), ("depth_samples", C.c_uint32)]


class UpscaleStats(C.Structure):  # include/bendy_hip.h `bt_upscale_stats` (extension)
    _fields_ = [("tier2", C.c_uint32), ("tier3", C.c_uint32), ("pixels", C.c_uint32), ("reserved", C.c_uint32)]


class _CCompareParams(C.Structure):  # include/bendy_hip.h `bt_compare_params` (extension)
    _fields_ = [("epsilon", C.c_double), ("peak", C.c_double)]


class CompareStats(C.Structure):  # include/bendy_hip.h `bt_compare_stats` (extension)
    _fields_ = [("pixels", C.c_uint64), ("valid", C.c_uint64), ("nonfinite", C.c_uint64), ("max_index", C.c_uint64),
                ("mse", C.c_double), ("rel_mse", C.c_double), ("ssim", C.c_double), ("max_abs", C.c_double), ("psnr", C.c_double)]

    def __repr__(self):
        return "CompareStats(" + ", ".join(f"{k}={getattr(self, k)!r}" for k, _ in self._fields_) + ")"


# include/bendy_hip.h `bt_ray` (32 B) and `bt_hit` (64 B) (extension): numpy views of the query's buffers
RAY_DTYPE = np.dtype([("origin", "<f4", 3), ("tmin", "<f4"), ("dir", "<f4", 3), ("tmax", "<f4")])
HIT_DTYPE = np.dtype([("position", "<f4", 3), ("t", "<f4"), ("normal", "<f4", 3), ("face", "<i4"), ("object_ref", "<u8"),
                      ("material_ref", "<u8"), ("volume_ref", "<u8"), ("prim", "<i4"), ("reserved", "<u4")])
FACE_MISS, FACE_FRONT, FACE_BACK, FACE_VOLUME_FRONT, FACE_VOLUME_BACK = -1, 0, 1, 3, 4
NO_REF = 0xFFFFFFFFFFFFFFFF


class _CRay(C.Structure):  # include/bendy_hip.h `bt_ray` (extension)
    _fields_ = [("origin", C.c_float * 3), ("tmin", C.c_float), ("dir", C.c_float * 3), ("tmax", C.c_float)]


class _CHit(C.Structure):  # include/bendy_hip.h `bt_hit` (extension)
    _fields_ = [("position", C.c_float * 3), ("t", C.c_float), ("normal", C.c_float * 3), ("face", C.c_int32),
                ("object_ref", C.c_uint64), ("material_ref", C.c_uint64), ("volume_ref", C.c_uint64), ("prim", C.c_int32),
                ("reserved", C.c_uint32)]


class _CLens(C.Structure):
    _fields_ = [("centre", C.c_float * 3), ("rs", C.c_float), ("step", C.c_float), ("radius", C.c_float),
                ("max_steps", C.c_uint32)]


EXPORTS = [
    "bt_config_default", "bt_render_config_default", "bt_last_error", "bt_last_error_code", "bt_version", "bt_scene_load",
    "bt_scene_from_json", "bt_scene_free", "bt_scene_find_by_tag", "bt_scene_set_camera_aspect", "bt_scene_set_lens",
    "bt_scene_object_count", "bt_scene_data_count", "bt_scene_export_prims", "bt_render", "bt_render_device",
    "bt_shard_floats", "bt_render_shard_device", "bt_unshard_device", "bt_preview_device", "bt_preview",
    "bt_comm_unique_id", "bt_comm_init", "bt_comm_free", "bt_comm_rank", "bt_comm_world", "bt_allgather_shards_device",
    "bt_exchange_frame_device", "bt_scene_last_stats", "bt_tuning_default", "bt_scene_set_tuning", "bt_scene_get_tuning", "bt_scene_default", "bt_scene_to_json", "bt_scene_save", "bt_write_png",
    "bt_scene_trim", "bt_denoise_params_default", "bt_denoiser_new", "bt_denoiser_free", "bt_denoise_device",
    "bt_denoise", "bt_debug_primary_mask", "bt_debug_block_masks_device", "bt_debug_mask_key", "bt_debug_block_order", "bt_debug_block_order_device", "bt_debug_philox_device", "bt_debug_set_object",
    "bt_debug_plan_launch",
    "bt_render_guided_device", "bt_adaptive_params_default", "bt_adaptive_new", "bt_adaptive_free", "bt_adaptive_reset",
    "bt_render_adaptive_device", "bt_adaptive_poll", "bt_adaptive_counts", "bt_adaptive_errors", "bt_debug_adaptive_moments",
    "bt_adaptive_resolve_device",
    "bt_scene_camera_view", "bt_scene_set_camera_pose", "bt_temporal_params_default", "bt_temporal_new", "bt_temporal_free",
    "bt_temporal_reset", "bt_temporal_accumulate_device", "bt_debug_temporal_history", "bt_debug_reproject",
    "bt_display_params_default", "bt_display_new", "bt_display_free", "bt_display_reset", "bt_display_device",
    "bt_display_exposure", "bt_debug_display_histogram", "bt_write_pfm", "bt_scene_export_sorted_rows",
    "bt_debug_abs_limit",
    "bt_glare_params_default", "bt_glare_new", "bt_glare_free", "bt_glare_device", "bt_debug_glare_plane", "bt_debug_glare_host",
    "bt_resample_params_default", "bt_resample_new", "bt_resample_free", "bt_resample_device", "bt_debug_resample_weights",
    "bt_debug_resample_plane", "bt_debug_resample_host",
    "bt_despeckle_params_default", "bt_despeckle_new", "bt_despeckle_free", "bt_despeckle_device", "bt_despeckle_poll",
    "bt_debug_despeckle_host",
    "bt_upscale_params_default", "bt_upscale_new", "bt_upscale_free", "bt_upscale_device", "bt_upscale_poll",
    "bt_debug_upscale_weights", "bt_debug_upscale_plane", "bt_debug_upscale_host",
    "bt_compare_params_default", "bt_compare_new", "bt_compare_free", "bt_compare_device", "bt_compare_poll", "bt_compare_tail",
    "bt_compare_map_device", "bt_debug_compare_plane", "bt_debug_compare_host", "bt_read_pfm",
    "bt_query_rays_device", "bt_view_rays_device", "bt_scene_pick", "bt_scene_set_camera_focus",
]


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: the HIP extension has not been built (run `python -c 'import __graft_entry__ "
            "as g; g.build()'` or `make -C bendy_tracer_amd/csrc`).  There is no CPU fallback.")
    # PyTorch bundles its own HIP / HSA runtime.  Two copies of the runtime in one process cannot both own
    # the GPU (the second one reports "no ROCm-capable device"), so when torch is installed it is imported
    # FIRST and libbendy_hip.so then binds to the runtime torch has already loaded.  Standalone C/C++ users
    # (the CLI) use /opt/rocm's runtime.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    vp, fp = C.c_void_p, C.POINTER(C.c_float)
    L.bt_last_error.restype = C.c_char_p
    L.bt_version.restype = C.c_char_p
    L.bt_config_default.argtypes = [C.POINTER(_CConfig)]
    L.bt_render_config_default.argtypes = [C.POINTER(_CRenderConfig)]
    L.bt_scene_load.restype = vp
    L.bt_scene_load.argtypes = [C.c_char_p]
    L.bt_scene_from_json.restype = vp
    L.bt_scene_from_json.argtypes = [C.c_char_p, C.c_size_t]
    L.bt_scene_free.argtypes = [vp]
    L.bt_scene_default.restype = vp
    L.bt_scene_to_json.argtypes = [vp, C.c_char_p, C.c_size_t]
    L.bt_scene_save.argtypes = [vp, C.c_char_p]
    L.bt_write_png.argtypes = [C.c_char_p, C.POINTER(C.c_uint8), C.c_uint32, C.c_uint32]
    L.bt_scene_find_by_tag.argtypes = [vp, C.c_char_p, C.POINTER(C.c_uint64)]
    L.bt_scene_set_camera_aspect.argtypes = [vp, C.c_uint64, C.c_float]
    L.bt_scene_set_lens.argtypes = [vp, C.POINTER(_CLens)]
    L.bt_scene_object_count.argtypes = [vp]
    L.bt_scene_data_count.argtypes = [vp]
    L.bt_scene_export_prims.argtypes = [vp, fp, C.c_int]
    L.bt_scene_export_sorted_rows.argtypes = [vp, C.POINTER(C.c_uint32), C.c_int]
    L.bt_debug_abs_limit.restype = C.c_float
    L.bt_debug_abs_limit.argtypes = [C.c_float]
    L.bt_debug_primary_mask.argtypes = [vp, C.c_uint64, C.POINTER(_CConfig), C.POINTER(_CRenderConfig), C.c_uint32, C.c_uint32,
                                        C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64), C.c_uint32]
    L.bt_debug_set_object.argtypes = [vp, C.c_uint64, fp, C.c_float]
    L.bt_debug_block_masks_device.argtypes = L.bt_debug_primary_mask.argtypes
    L.bt_debug_mask_key.argtypes = [vp, C.c_uint64, C.POINTER(_CConfig), C.POINTER(_CRenderConfig), C.c_uint32, C.c_uint32,
                                    C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint8), C.c_uint32]
    L.bt_debug_block_order.argtypes = [C.POINTER(C.c_uint64), C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.bt_debug_block_order_device.argtypes = L.bt_debug_block_order.argtypes
    L.bt_debug_philox_device.argtypes = [C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(C.c_uint32)]
    L.bt_debug_plan_launch.argtypes = [vp, C.c_uint64, C.POINTER(_CConfig), C.POINTER(_CRenderConfig), C.c_uint32, C.c_uint32,
                                       C.c_uint32, C.c_uint32, C.c_int32, C.c_uint32, C.c_int32, C.c_uint32, C.c_uint64,
                                       C.POINTER(Stats)]
    L.bt_render.argtypes = [vp, C.c_uint64, C.POINTER(_CConfig), C.POINTER(_CRenderConfig), fp, C.c_uint32,
                            C.c_uint32, C.c_uint64]
    L.bt_render_device.argtypes = [vp, C.c_uint64, C.POINTER(_CConfig), C.POINTER(_CRenderConfig), vp, C.c_uint32,
                                   C.c_uint32, C.c_uint64, vp]
    L.bt_render_guided_device.argtypes = [vp, C.c_uint64, C.POINTER(_CConfig), C.POINTER(_CRenderConfig), vp, vp, vp, vp,
                                          C.c_uint32, C.c_uint32, C.c_uint64, vp]
    L.bt_shard_floats.restype = C.c_size_t
    L.bt_shard_floats.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32]
    L.bt_render_shard_device.argtypes = [vp, C.c_uint64, C.POINTER(_CConfig), C.POINTER(_CRenderConfig), vp,
                                         C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, vp]
    L.bt_unshard_device.argtypes = [vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, vp]
    L.bt_preview_device.argtypes = [vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int32, vp]
    L.bt_preview.argtypes = [fp, C.POINTER(C.c_uint8), C.c_uint32, C.c_uint32, C.c_uint32, C.c_int32]
    L.bt_scene_last_stats.argtypes = [vp, C.POINTER(Stats)]
    L.bt_comm_unique_id.argtypes = [C.c_void_p, C.c_size_t]
    L.bt_comm_init.restype = vp
    L.bt_comm_init.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t]
    L.bt_comm_free.argtypes = [vp]
    L.bt_comm_rank.argtypes = [vp]
    L.bt_comm_world.argtypes = [vp]
    L.bt_allgather_shards_device.argtypes = [vp, vp, vp, C.c_uint32, C.c_uint32, vp]
    L.bt_exchange_frame_device.argtypes = [vp, vp, vp, vp, C.c_uint32, C.c_uint32, vp]
    L.bt_tuning_default.argtypes = [C.POINTER(_CTuning)]
    L.bt_scene_set_tuning.argtypes = [vp, C.POINTER(_CTuning)]
    L.bt_scene_get_tuning.argtypes = [vp, C.POINTER(_CTuning)]
    L.bt_scene_trim.argtypes = [vp]
    L.bt_denoise_params_default.argtypes = [C.POINTER(_CDenoiseParams)]
    L.bt_denoiser_new.restype = vp
    L.bt_denoiser_free.argtypes = [vp]
    L.bt_denoise_device.argtypes = [vp, vp, C.c_uint32, vp, C.c_uint32, vp, C.c_uint32, vp, C.c_uint32, vp, C.c_uint32,
                                    C.c_uint32, C.POINTER(_CDenoiseParams), vp]
    L.bt_denoise.argtypes = [vp, fp, C.c_uint32, fp, C.c_uint32, fp, C.c_uint32, fp, C.c_uint32, fp, C.c_uint32, C.c_uint32,
                             C.POINTER(_CDenoiseParams)]
    L.bt_adaptive_params_default.argtypes = [C.POINTER(_CAdaptiveParams)]
    L.bt_adaptive_new.restype = vp
    L.bt_adaptive_new.argtypes = [C.c_uint32, C.c_uint32]
    L.bt_adaptive_free.argtypes = [vp]
    L.bt_adaptive_reset.argtypes = [vp]
    L.bt_render_adaptive_device.argtypes = [vp, C.c_uint64, C.POINTER(_CConfig), C.POINTER(_CRenderConfig), vp,
                                            C.POINTER(_CAdaptiveParams), vp, C.c_uint32, C.c_uint32, C.c_uint64, vp]
    L.bt_adaptive_poll.argtypes = [vp, C.POINTER(AdaptiveStats)]
    L.bt_adaptive_counts.argtypes = [vp, C.POINTER(C.c_uint32), C.c_uint32]
    L.bt_adaptive_errors.argtypes = [vp, fp, C.c_uint32]
    L.bt_debug_adaptive_moments.argtypes = [vp, fp, C.c_uint32]
    L.bt_adaptive_resolve_device.argtypes = [vp, vp, vp, vp]
    L.bt_scene_camera_view.argtypes = [vp, C.c_uint64, C.POINTER(_CConfig), C.POINTER(_CRenderConfig), C.c_uint32, C.c_uint32,
                                       C.POINTER(View)]
    L.bt_scene_set_camera_pose.argtypes = [vp, C.c_uint64, fp]
    L.bt_temporal_params_default.argtypes = [C.POINTER(_CTemporalParams)]
    L.bt_temporal_new.restype = vp
    L.bt_temporal_new.argtypes = [C.c_uint32, C.c_uint32]
    L.bt_temporal_free.argtypes = [vp]
    L.bt_temporal_reset.argtypes = [vp]
    L.bt_temporal_accumulate_device.argtypes = [vp, C.POINTER(View), vp, C.c_uint32, vp, C.c_uint32, vp, C.c_uint32, vp,
                                                C.POINTER(_CTemporalParams), vp]
    L.bt_debug_temporal_history.argtypes = [vp, fp, C.c_uint32]
    L.bt_debug_reproject.argtypes = [C.POINTER(View), C.POINTER(View), C.c_float, C.c_float, C.c_float, fp]
    L.bt_display_params_default.argtypes = [C.POINTER(_CDisplayParams)]
    L.bt_display_new.restype = vp
    L.bt_display_new.argtypes = []
    L.bt_display_free.argtypes = [vp]
    L.bt_display_reset.argtypes = [vp]
    L.bt_display_device.argtypes = [vp, vp, C.c_uint32, vp, C.c_uint32, C.c_uint32, C.c_int32, C.POINTER(_CDisplayParams), vp]
    L.bt_display_exposure.argtypes = [vp, fp, fp]
    L.bt_debug_display_histogram.argtypes = [vp, C.POINTER(C.c_uint32), C.c_uint32]
    L.bt_write_pfm.argtypes = [C.c_char_p, fp, C.c_uint32, C.c_uint32, C.c_uint32]
    L.bt_glare_params_default.argtypes = [C.POINTER(_CGlareParams)]
    L.bt_glare_new.restype = vp
    L.bt_glare_new.argtypes = []
    L.bt_glare_free.argtypes = [vp]
    L.bt_glare_device.argtypes = [vp, vp, C.c_uint32, vp, C.c_uint32, C.c_uint32, C.POINTER(_CGlareParams), vp]
    L.bt_debug_glare_plane.argtypes = [vp, C.c_uint32, fp, C.c_uint32]
    L.bt_debug_glare_host.argtypes = [fp, C.c_uint32, fp, C.c_uint32, C.c_uint32, C.POINTER(_CGlareParams)]
    L.bt_resample_params_default.argtypes = [C.POINTER(_CResampleParams)]
    L.bt_resample_new.restype = vp
    L.bt_resample_new.argtypes = []
    L.bt_resample_free.argtypes = [vp]
    L.bt_resample_device.argtypes = [vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, C.c_uint32, C.c_uint32, C.POINTER(_CResampleParams), vp]
    L.bt_debug_resample_weights.argtypes = [vp, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_int32), fp, C.POINTER(C.c_uint32)]
    L.bt_debug_resample_plane.argtypes = [vp, fp, C.c_uint32]
    L.bt_debug_resample_host.argtypes = [vp, fp, C.c_uint32, C.c_uint32, C.c_uint32, fp, C.c_uint32, C.c_uint32, C.POINTER(_CResampleParams)]
    L.bt_despeckle_params_default.argtypes = [C.POINTER(_CDespeckleParams)]
    L.bt_despeckle_new.restype = vp
    L.bt_despeckle_new.argtypes = []
    L.bt_despeckle_free.argtypes = [vp]
    L.bt_despeckle_device.argtypes = [vp, vp, C.c_uint32, vp, C.c_uint32, C.c_uint32, C.POINTER(_CDespeckleParams), vp]
    L.bt_despeckle_poll.argtypes = [vp, C.POINTER(DespeckleStats)]
    L.bt_debug_despeckle_host.argtypes = [fp, C.c_uint32, fp, C.c_uint32, C.c_uint32, C.POINTER(_CDespeckleParams), C.POINTER(DespeckleStats)]
    L.bt_upscale_params_default.argtypes = [C.POINTER(_CUpscaleParams)]
    L.bt_upscale_new.restype = vp
    L.bt_upscale_new.argtypes = []
    L.bt_upscale_free.argtypes = [vp]
    gp = C.POINTER(_CUpscaleGuides)
    L.bt_upscale_device.argtypes = [vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, gp, gp, vp, C.c_uint32, C.c_uint32, C.POINTER(_CUpscaleParams), vp]
    L.bt_upscale_poll.argtypes = [vp, C.POINTER(UpscaleStats)]
    L.bt_debug_upscale_weights.argtypes = [vp, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_int32), fp, C.POINTER(C.c_uint32)]
    L.bt_debug_upscale_plane.argtypes = [vp, C.c_uint32, fp, C.c_uint32]
    L.bt_debug_upscale_host.argtypes = [vp, fp, C.c_uint32, C.c_uint32, C.c_uint32, gp, gp, fp, C.c_uint32, C.c_uint32,
                                        C.POINTER(_CUpscaleParams), C.POINTER(UpscaleStats)]
    cpp, dp = C.POINTER(_CCompareParams), C.POINTER(C.c_double)
    L.bt_compare_params_default.argtypes = [cpp]
    L.bt_compare_new.restype = vp
    L.bt_compare_new.argtypes = []
    L.bt_compare_free.argtypes = [vp]
    L.bt_compare_device.argtypes = [vp, vp, C.c_uint32, vp, C.c_uint32, C.c_uint32, C.c_uint32, cpp, vp]
    L.bt_compare_poll.argtypes = [vp, C.POINTER(CompareStats)]
    L.bt_compare_tail.argtypes = [vp, C.c_double, dp, fp]
    L.bt_compare_map_device.argtypes = [vp, vp, C.c_float, vp]
    L.bt_debug_compare_plane.argtypes = [vp, C.c_uint32, vp, C.c_uint32]
    L.bt_debug_compare_host.argtypes = [fp, C.c_uint32, fp, C.c_uint32, C.c_uint32, C.c_uint32, cpp, C.POINTER(CompareStats), fp, dp, dp,
                                        C.c_uint32, dp, dp, fp]
    L.bt_read_pfm.argtypes = [C.c_char_p, fp, C.c_size_t, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.bt_query_rays_device.argtypes = [vp, vp, C.c_uint32, vp, vp]
    L.bt_view_rays_device.argtypes = [C.POINTER(View), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp]
    L.bt_scene_pick.argtypes = [vp, C.c_uint64, C.POINTER(_CConfig), C.POINTER(_CRenderConfig), C.c_uint32, C.c_uint32, C.c_uint32,
                                C.c_uint32, C.POINTER(_CHit), fp]
    L.bt_scene_set_camera_focus.argtypes = [vp, C.c_uint64, C.c_int, C.c_float]
    return L


lib = _load()


def _check(rc):
    if rc < 0:
        raise BendyError(rc, lib.bt_last_error().decode("utf-8", "replace"))
    return rc


def _c_configs(config: Config, render: RenderConfig, sample_base: int):
    c = _CConfig(config.max_bounces, config.max_volume_bounces, config.clip_min, config.clip_max, config.volume_step,
                 config.chunks_x, config.chunks_y, int(config.output))
    r = _CRenderConfig()
    r.subsample_n = render.subsample.n
    r.samples = render.samples
    r.has_output = render.output is not None
    r.output = int(render.output) if render.output is not None else 0
    r.has_max_bounces = render.max_bounces is not None
    r.max_bounces = render.max_bounces or 0
    r.has_max_volume_bounces = render.max_volume_bounces is not None
    r.max_volume_bounces = render.max_volume_bounces or 0
    r.has_volume_step = render.volume_step is not None
    r.volume_step = render.volume_step or 0.0
    r.sample_base = sample_base
    return c, r


class Scene:
    """`Scene` (scene/mod.rs:84-146) as loaded by main.rs:93-102."""

    def __init__(self, handle):
        if not handle:
            raise BendyError(lib.bt_last_error_code(), lib.bt_last_error().decode("utf-8", "replace"))
        self._h = C.c_void_p(handle)

    @classmethod
    def load(cls, path):
        return cls(lib.bt_scene_load(os.fspath(path).encode()))

    @classmethod
    def from_json(cls, text):
        data = text.encode() if isinstance(text, str) else bytes(text)
        return cls(lib.bt_scene_from_json(data, len(data)))

    @classmethod
    def default(cls):
        """The built-in Cornell scene of main.rs:107-214."""
        return cls(lib.bt_scene_default())

    def to_json(self) -> str:
        """serde_json::to_string_pretty(&scene)."""
        n = _check(lib.bt_scene_to_json(self._h, None, 0))
        buf = C.create_string_buffer(n + 1)
        _check(lib.bt_scene_to_json(self._h, buf, n + 1))
        return buf.value.decode()

    def save(self, path):
        """Ctrl+K in main.rs:299-313: pretty JSON, gzip when the extension is .gz."""
        _check(lib.bt_scene_save(self._h, os.fspath(path).encode()))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            lib.bt_scene_free(h)
            self._h = None

    def find_by_tag(self, tag) -> Optional[int]:
        """Scene::find_by_tag (scene/mod.rs:124-129): ObjectRef or None."""
        ref = C.c_uint64()
        rc = lib.bt_scene_find_by_tag(self._h, tag.encode(), C.byref(ref))
        return ref.value if rc == 0 else None

    def set_camera_aspect(self, camera_ref, aspect_ratio):
        """main.rs:218-223."""
        _check(lib.bt_scene_set_camera_aspect(self._h, camera_ref, aspect_ratio))

    def debug_set_object(self, object_ref, translation=None, radius=0.0):
        """bt_debug_set_object (tests): move an object / resize a sphere in place on this handle."""
        t = None if translation is None else (C.c_float * 3)(*[float(v) for v in translation])
        _check(lib.bt_debug_set_object(self._h, object_ref, t, float(radius)))

    def camera_view(self, camera, config: "Config", render: "RenderConfig", width, height) -> View:
        """EXTENSION, not in the reference (bt_scene_camera_view): the camera as data -- what a render with
        these arguments puts into its launch.  Touches no device."""
        c, r = _c_configs(config, render, 0)
        v = View()
        _check(lib.bt_scene_camera_view(self._h, camera, C.byref(c), C.byref(r), width, height, C.byref(v)))
        return v

    def set_camera_pose(self, camera, to_world):
        """EXTENSION, not in the reference (bt_scene_set_camera_pose): replaces the camera's transform_world in place on this
        handle; 12 floats, columns x, y, z, then the translation.  The JSON that `save` / `to_json` write is not updated."""
        m = [float(v) for v in np.asarray(to_world, dtype=np.float32).reshape(-1)]
        if len(m) != 12:
            raise BendyError(-1, f"to_world needs 12 floats, not {len(m)}")
        _check(lib.bt_scene_set_camera_pose(self._h, camera, (C.c_float * 12)(*m)))

    def set_camera_focus(self, camera, focus):
        """EXTENSION, not in the reference (bt_scene_set_camera_focus): replaces the camera's focus distance in place on this
        handle; None clears it (no depth of field).  The JSON that `save` / `to_json` write is not updated."""
        _check(lib.bt_scene_set_camera_focus(self._h, camera, 0 if focus is None else 1, 0.0 if focus is None else float(focus)))

    def query(self, rays, out=None):
        """EXTENSION, not in the reference (bt_query_rays_device): the closest hit of each ray -- `try_hit`
        (tracer/mod.rs:389-402) with the clip taken from the ray.  `rays`: a contiguous CUDA float32 tensor [n, 8], a row being
        a `bt_ray` (origin, tmin, dir, tmax; `dir` is used as given).  Returns a uint8 tensor [n, 64] of `bt_hit` records on the
        same device, enqueued on the current stream and not synchronised; `hits_numpy` views it as HIT_DTYPE."""
        import torch
        if not (isinstance(rays, torch.Tensor) and rays.is_cuda and rays.dtype == torch.float32 and rays.dim() == 2
                and rays.shape[1] == 8 and rays.is_contiguous()):
            raise BendyError(-1, "rays must be a contiguous CUDA float32 tensor [n, 8]")
        n = rays.shape[0]
        if out is None:
            out = torch.empty((n, 64), dtype=torch.uint8, device=rays.device)
        elif not (out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == (n, 64) and out.is_contiguous()):
            raise BendyError(-1, f"out must be a contiguous CUDA uint8 tensor [{n}, 64]")
        if n:
            _check(lib.bt_query_rays_device(self._h, rays.data_ptr(), n, out.data_ptr(), torch.cuda.current_stream().cuda_stream))
        return out

    def pick(self, camera, config: "Config", render: "RenderConfig", width, height, x, y):
        """EXTENSION, not in the reference (bt_scene_pick; synchronises): what the ray through the centre of pixel (x, y) hits --
        None, or a dict of the `bt_hit` fields plus `focus`, the camera focus that puts the hit point in the focal plane."""
        c, r = _c_configs(config, render, 0)
        hit, focus = _CHit(), C.c_float(0.0)
        if _check(lib.bt_scene_pick(self._h, camera, C.byref(c), C.byref(r), width, height, x, y, C.byref(hit), C.byref(focus))) == 0:
            return None
        return {"position": [float(v) for v in hit.position], "t": float(hit.t), "normal": [float(v) for v in hit.normal],
                "face": int(hit.face), "object_ref": int(hit.object_ref), "material_ref": int(hit.material_ref),
                "volume_ref": None if hit.volume_ref == NO_REF else int(hit.volume_ref), "prim": int(hit.prim),
                "focus": float(focus.value)}

    def set_lens(self, centre, rs, step, radius, max_steps=4096):
        """EXTENSION, not in the reference (include/bendy_hip.h `bt_lens`): bend rays around a point mass."""
        lens = _CLens((C.c_float * 3)(*[float(v) for v in centre]), rs, step, radius, max_steps)
        _check(lib.bt_scene_set_lens(self._h, C.byref(lens)))

    def clear_lens(self):
        _check(lib.bt_scene_set_lens(self._h, None))

    @property
    def object_count(self):
        return lib.bt_scene_object_count(self._h)

    @property
    def data_count(self):
        return lib.bt_scene_data_count(self._h)

    def export_prims(self):
        """The flattened primitive table exactly as uploaded to the GPU ([n, 36] float32 view)."""
        n = _check(lib.bt_scene_export_prims(self._h, None, 0))
        out = np.zeros(n, dtype=np.float32)
        _check(lib.bt_scene_export_prims(self._h, out.ctypes.data_as(C.POINTER(C.c_float)), n))
        return out.reshape(-1, 36)

    AAN_ROW = np.dtype([("it_a", "<f4"), ("it_b", "<f4"), ("lim_a", "<f4"), ("lim_b", "<f4"), ("t_w", "<f4"),
                        ("sgn_mask", "<u4"), ("prio", "<u4"), ("pad", "<u4")])                       # bt_types.h BtRectAAN
    LA_ROW = np.dtype([("n", "<f4", 3), ("first_of_normal", "<u4"), ("t", "<f4", 3), ("prio", "<u4"), ("a_x", "<f4", 2),
                       ("a_y", "<f4", 2), ("a_z", "<f4", 2), ("a_w", "<f4", 2), ("lim", "<f4", 2), ("pad", "<u4", 2)])  # BtRectLA

    def export_sorted_rows(self):
        """bt_scene_export_sorted_rows (tests): the sorted view of the primitive table exactly as uploaded to the GPU --
        {"n_aan": int32 [3], "aan": AAN_ROW records, "la": LA_ROW records, "other": int32 rows of export_prims()}."""
        n = _check(lib.bt_scene_export_sorted_rows(self._h, None, 0))
        w = np.zeros(n, dtype=np.uint32)
        _check(lib.bt_scene_export_sorted_rows(self._h, w.ctypes.data_as(C.POINTER(C.c_uint32)), n))
        n_aan, n_la, n_other = w[:3].astype(np.int32), int(w[3]), int(w[4])
        a0, l0 = 5, 5 + 8 * int(n_aan.sum())
        o0 = l0 + 20 * n_la
        assert o0 + n_other == n
        return {"n_aan": n_aan, "aan": w[a0:l0].view(self.AAN_ROW), "la": w[l0:o0].view(self.LA_ROW),
                "other": w[o0:].view(np.int32)}

    def set_tuning(self, **knobs):
        """bt_scene_set_tuning: pins launch-shape knobs of this handle (tests and A/B tools; none of them changes a
        pixel).  Keywords = fields of `bt_tuning` (slices, phase_vote, scratch_cap_bytes, packed);
        fields not named keep their current value; no keywords = defaults."""
        t = _CTuning()
        if not knobs:
            _check(lib.bt_scene_set_tuning(self._h, None))
            return
        _check(lib.bt_scene_get_tuning(self._h, C.byref(t)))
        for k, v in knobs.items():
            if not hasattr(t, k):
                raise TypeError(f"bt_tuning has no field {k!r}")
            setattr(t, k, int(v))
        _check(lib.bt_scene_set_tuning(self._h, C.byref(t)))

    def tuning(self) -> dict:
        t = _CTuning()
        _check(lib.bt_scene_get_tuning(self._h, C.byref(t)))
        return {k: getattr(t, k) for k, _ in _CTuning._fields_}

    def tuning_from_env(self, environ=None):
        """Developer convenience for tools/ and tests/: BT_SLICES, BT_PHASE_VOTE, BT_SCRATCH_CAP, BT_PACKED -> set_tuning().  The library itself never reads the environment."""
        env = os.environ if environ is None else environ
        names = {"BT_SLICES": "slices", "BT_PHASE_VOTE": "phase_vote", "BT_SCRATCH_CAP": "scratch_cap_bytes", "BT_PACKED": "packed"}
        knobs = {f: int(env[e]) for e, f in names.items() if env.get(e) not in (None, "", "-")}
        if knobs:
            self.set_tuning(**knobs)
        return knobs

    def trim(self):
        """Returns the scratch / cached frame the handle keeps between calls to the device (bt_scene_trim)."""
        _check(lib.bt_scene_trim(self._h))

    def last_stats(self) -> Stats:
        st = Stats()
        _check(lib.bt_scene_last_stats(self._h, C.byref(st)))
        return st


class Buffer:
    """`Buffer` (tracer/buffer.rs:32-179): RGBA32F running sums + sample counter.

    device="cuda" keeps the sums in HBM (a torch tensor, plumbing only); device="cpu" keeps
    a numpy array and every render call copies it through the device."""

    def __init__(self, width, height, color_space=ColorSpace.SRgb, device="cuda"):
        self.width, self.height = int(width), int(height)
        self.color_space = ColorSpace(color_space)
        self.samples = 0
        self.device = device
        if device == "cpu":
            self.data = np.zeros((self.height, self.width, 4), dtype=np.float32)
            self.data[..., 3] = 1.0  # BLACK_ALPHA_ONE, buffer.rs:9,43
        else:
            import torch
            self.data = torch.zeros((self.height, self.width, 4), dtype=torch.float32, device=device)
            self.data[..., 3] = 1.0

    @classmethod
    def new(cls, width, height, color_space=ColorSpace.SRgb, device="cuda"):
        return cls(width, height, color_space, device)

    def dimensions(self):
        return (self.width, self.height)

    def pixel_width(self):  # buffer.rs:68-71
        return float(np.float32(2.0) * (np.float32(1.0) / np.float32(self.width)))

    def pixel_height(self):  # buffer.rs:73-76
        return float(np.float32(2.0) * (np.float32(1.0) / np.float32(self.height)))

    def clear(self):  # buffer.rs:82-87
        self.data[...] = 0.0
        self.data[..., 3] = 1.0
        self.samples = 0

    def inc_samples(self, n):  # buffer.rs:155-157
        self.samples += n

    def chunks(self, chunks_x, chunks_y):
        """Buffer::chunks (buffer.rs:102-115, 293-326): list of (min_x, min_y, max_x, max_y)."""
        cw = self.width // chunks_x + (1 if self.width % chunks_x else 0)
        ch = self.height // chunks_y + (1 if self.height % chunks_y else 0)
        out, oy = [], 0
        while oy < self.height:
            h = min(ch, self.height - oy)
            ox = 0
            while ox < self.width:
                w = min(cw, self.width - ox)
                out.append((ox, oy, ox + w, oy + h))
                ox += w
            oy += h
        return out

    def numpy(self):
        return self.data if self.device == "cpu" else self.data.cpu().numpy()

    def mean(self):
        """sum / samples as buffer.rs:124-127 does before the colour-space conversion."""
        return self.numpy()[..., :3] / np.float32(max(self.samples, 1))

    def preview(self):
        """Buffer::preview (buffer.rs:117-138) -> uint8 [H, W, 4] on the host."""
        if self.device == "cpu":
            out = np.zeros((self.height, self.width, 4), dtype=np.uint8)
            _check(lib.bt_preview(self.data.ctypes.data_as(C.POINTER(C.c_float)),
                                  out.ctypes.data_as(C.POINTER(C.c_uint8)), self.width, self.height,
                                  max(self.samples, 1), int(self.color_space)))
            return out
        import torch
        out = torch.empty((self.height, self.width, 4), dtype=torch.uint8, device=self.data.device)
        _check(lib.bt_preview_device(self.data.data_ptr(), out.data_ptr(), self.width, self.height,
                                     max(self.samples, 1), int(self.color_space),
                                     torch.cuda.current_stream().cuda_stream))
        return out.cpu().numpy()


class Tracer:
    """`Tracer` (tracer/mod.rs:165-203)."""

    DEFAULT_SEED = 0x5EED

    def __init__(self, config: Optional[Config] = None):
        self.config = config or Config()

    @classmethod
    def new(cls):
        return cls()

    @classmethod
    def with_config(cls, config):
        return cls(config)

    def render(self, scene: Scene, camera: int, config: RenderConfig, buffer: Buffer, seed: Optional[int] = None,
               sample_base: Optional[int] = None) -> Status:
        """Tracer::render (mod.rs:179-202).  `seed` stands in for SmallRng::from_entropy()
        (mod.rs:239-242); `sample_base` defaults to buffer.samples / n^2 so that successive
        calls on one buffer draw fresh samples from the same seed."""
        seed = self.DEFAULT_SEED if seed is None else seed
        nn = config.subsample.subpixel_count()
        if sample_base is None:
            # the next unused sample index: ceil, so that a change of `subsample` between calls never replays indices
            sample_base = (buffer.samples + nn - 1) // nn
        c, r = _c_configs(self.config, config, sample_base)
        if buffer.device == "cpu":
            rc = lib.bt_render(scene._h, camera, C.byref(c), C.byref(r),
                               buffer.data.ctypes.data_as(C.POINTER(C.c_float)), buffer.width, buffer.height, seed)
        else:
            import torch
            rc = lib.bt_render_device(scene._h, camera, C.byref(c), C.byref(r), buffer.data.data_ptr(), buffer.width,
                                      buffer.height, seed, torch.cuda.current_stream().cuda_stream)
        _check(rc)
        if rc == Status.InProgress:
            buffer.inc_samples(config.samples * nn)  # mod.rs:199
        return Status(rc)

    def render_guided(self, scene: Scene, camera: int, config: RenderConfig, color: Buffer, albedo: Optional[Buffer] = None,
                      normal: Optional[Buffer] = None, depth: Optional[Buffer] = None, seed: Optional[int] = None,
                      sample_base: Optional[int] = None) -> Status:
        """EXTENSION, not in the reference (bt_render_guided_device): one pass that adds the colour samples
        to `color` and, from the same paths, the Output.Albedo / Normal / Depth values to the guide buffers that are given
        -- every buffer ends up bit-identical to what `render` writes into it with the corresponding output.  GPU buffers
        of one size only; the effective output must be Output.Full; `seed` and `sample_base` default as in `render`
        (taken from `color`)."""
        seed = self.DEFAULT_SEED if seed is None else seed
        output = config.output if config.output is not None else self.config.output
        if int(output) != int(Output.Full):
            raise BendyError(-1, f"render_guided renders Output.Full plus its guides, not output {int(output)}")
        guides = [albedo, normal, depth]
        for b in [color] + [g for g in guides if g is not None]:
            if b.device == "cpu":
                raise BendyError(-1, "render_guided needs device-resident buffers (there is no host-buffer variant)")
            if (b.width, b.height) != (color.width, color.height):
                raise BendyError(-1, f"buffer of {b.width}x{b.height} next to a {color.width}x{color.height} colour buffer")
        nn = config.subsample.subpixel_count()
        if sample_base is None:
            sample_base = (color.samples + nn - 1) // nn
        c, r = _c_configs(self.config, config, sample_base)
        import torch
        rc = lib.bt_render_guided_device(scene._h, camera, C.byref(c), C.byref(r), color.data.data_ptr(),
                                         *[g.data.data_ptr() if g is not None else None for g in guides], color.width,
                                         color.height, seed, torch.cuda.current_stream().cuda_stream)
        _check(rc)
        if rc == Status.InProgress:
            for b in [color] + [g for g in guides if g is not None]:
                b.inc_samples(config.samples * nn)
        return Status(rc)

    def render_adaptive(self, scene: Scene, camera: int, config: RenderConfig, buffer: Buffer, adaptive: "Adaptive",
                        seed: Optional[int] = None) -> Status:
        """EXTENSION, not in the reference (bt_render_adaptive_device + bt_adaptive_poll): one adaptive pass
        of `config.samples` x n^2 samples per pixel into the tiles of `buffer` that `adaptive` still holds active, then a
        poll.  Status.Done once no tile is active.  `buffer.samples` is left alone: the tiles of an adaptively sampled
        frame hold different numbers of samples, and the per-tile counts live on the handle (`adaptive.counts()`,
        `adaptive.resolve(buffer)` for the mean).  The sample index continues from the handle's earlier passes.
        A GPU buffer of the handle's size only; the effective output must be Output.Full."""
        seed = self.DEFAULT_SEED if seed is None else seed
        if buffer.device == "cpu":
            raise BendyError(-1, "render_adaptive needs a device-resident buffer (there is no host-buffer variant)")
        c, r = _c_configs(self.config, config, 0)
        p = adaptive.params._c()
        import torch
        rc = _check(lib.bt_render_adaptive_device(scene._h, camera, C.byref(c), C.byref(r), adaptive._h, C.byref(p),
                                                  buffer.data.data_ptr(), buffer.width, buffer.height, seed,
                                                  torch.cuda.current_stream().cuda_stream))
        if rc == Status.Done:
            return Status.Done
        return Status(_check(lib.bt_adaptive_poll(adaptive._h, None)))

    def primary_masks(self, scene: Scene, camera: int, config: RenderConfig, width, height, slices, rank=0, world=1):
        """bt_debug_primary_mask (tests): per block of a launch with `slices` blocks per tile, in launch order, the
        sphere rows a primary ray of the block may hit (uint64 bit masks)."""
        c, r = _c_configs(self.config, config, 0)
        n = _check(lib.bt_debug_primary_mask(scene._h, camera, C.byref(c), C.byref(r), width, height, slices, rank, world,
                                             None, 0))
        out = np.zeros(n, dtype=np.uint64)
        _check(lib.bt_debug_primary_mask(scene._h, camera, C.byref(c), C.byref(r), width, height, slices, rank, world,
                                         out.ctypes.data_as(C.POINTER(C.c_uint64)), n))
        return out

    def block_masks_device(self, scene: Scene, camera: int, config: RenderConfig, width, height, slices, rank=0, world=1):
        """bt_debug_block_masks_device (tests): the same masks, written by bt_block_mask_kernel on the GPU."""
        c, r = _c_configs(self.config, config, 0)
        n = _check(lib.bt_debug_block_masks_device(scene._h, camera, C.byref(c), C.byref(r), width, height, slices, rank,
                                                   world, None, 0))
        out = np.zeros(n, dtype=np.uint64)
        _check(lib.bt_debug_block_masks_device(scene._h, camera, C.byref(c), C.byref(r), width, height, slices, rank, world,
                                               out.ctypes.data_as(C.POINTER(C.c_uint64)), n))
        return out

    @staticmethod
    def block_order(masks, device=False):
        """bt_debug_block_order / bt_debug_block_order_device (tests): the order in which a launch takes blocks with these
        masks -- non-zero masks first, each part ascending -- and the counts (n_live, n_empty); device=True: as the GPU
        kernel writes them."""
        m = np.ascontiguousarray(masks, dtype=np.uint64)
        order, header = np.zeros(m.size, dtype=np.uint32), np.zeros(2, dtype=np.uint32)
        fn = lib.bt_debug_block_order_device if device else lib.bt_debug_block_order
        _check(fn(m.ctypes.data_as(C.POINTER(C.c_uint64)), m.size, order.ctypes.data_as(C.POINTER(C.c_uint32)),
                  header.ctypes.data_as(C.POINTER(C.c_uint32))))
        return order, (int(header[0]), int(header[1]))

    @staticmethod
    def philox_device(counters, keys):
        """bt_debug_philox_device (tests): the device's Philox4x32-10, in the form the sphere-only render builds run it, over
        counters [n, 4] and keys [n, 2] (uint32); returns the words [n, 4]."""
        c = np.ascontiguousarray(counters, dtype=np.uint32).reshape(-1, 4)
        k = np.ascontiguousarray(keys, dtype=np.uint32).reshape(-1, 2)
        if c.shape[0] != k.shape[0]:
            raise ValueError("as many keys as counters")
        pairs = np.ascontiguousarray(np.concatenate([c, k], axis=1))
        out = np.zeros((c.shape[0], 4), dtype=np.uint32)
        _check(lib.bt_debug_philox_device(pairs.ctypes.data_as(C.POINTER(C.c_uint32)), c.shape[0],
                                          out.ctypes.data_as(C.POINTER(C.c_uint32))))
        return out

    def mask_key(self, scene: Scene, camera: int, config: RenderConfig, width, height, slices, rank=0, world=1) -> bytes:
        """bt_debug_mask_key (tests): the key under which the handle would keep these masks between renders."""
        c, r = _c_configs(self.config, config, 0)
        n = _check(lib.bt_debug_mask_key(scene._h, camera, C.byref(c), C.byref(r), width, height, slices, rank, world, None, 0))
        out = (C.c_uint8 * n)()
        _check(lib.bt_debug_mask_key(scene._h, camera, C.byref(c), C.byref(r), width, height, slices, rank, world, out, n))
        return bytes(out)

    def plan_launch(self, scene: Scene, camera: int, config: RenderConfig, width, height, n_cu, rank=0, world=1, sharded=False,
                    kind=0, guides=0, alloc_limit=0) -> Stats:
        """bt_debug_plan_launch (tests): the launch-shape fields of the bt_stats a render of these arguments would leave on a
        device of `n_cu` compute units, planned without a GPU.  kind: 0 plain, 1 guided (`guides`: bit mask of the guides
        present), 2 adaptive; allocations above `alloc_limit` bytes fail (0: none does)."""
        c, r = _c_configs(self.config, config, 0)
        st = Stats()
        _check(lib.bt_debug_plan_launch(scene._h, camera, C.byref(c), C.byref(r), width, height, rank, world, int(sharded),
                                        n_cu, kind, guides, alloc_limit, C.byref(st)))
        return st

    # ---- multi-GPU tile sharding (DESIGN.md "Multi-GPU") ----
    def render_shard(self, scene: Scene, camera: int, config: RenderConfig, shard, width, height, rank, world,
                     seed: Optional[int] = None, sample_base: int = 0) -> Status:
        import torch
        seed = self.DEFAULT_SEED if seed is None else seed
        c, r = _c_configs(self.config, config, sample_base)
        assert shard.numel() == shard_floats(width, height, world) and shard.dtype == torch.float32
        rc = lib.bt_render_shard_device(scene._h, camera, C.byref(c), C.byref(r), shard.data_ptr(), width, height, rank,
                                        world, seed, torch.cuda.current_stream().cuda_stream)
        return Status(_check(rc))


class Comm:
    """`bt_comm` (include/bendy_hip.h): the RCCL communicator of the frame exchange, behind the C ABI -- what a host
    without an RCCL binding of its own calls.  One process per GPU; `unique_id()` on rank 0, its 128 bytes handed to
    the other ranks by any host-side channel, then `Comm(rank, world, uid)` on every rank (collective)."""

    ID_BYTES = 128

    @staticmethod
    def unique_id() -> bytes:
        buf = C.create_string_buffer(Comm.ID_BYTES)
        _check(lib.bt_comm_unique_id(buf, Comm.ID_BYTES))
        return buf.raw

    def __init__(self, rank, world, uid: bytes):
        assert len(uid) == self.ID_BYTES
        h = lib.bt_comm_init(rank, world, uid, len(uid))
        if not h:
            raise BendyError(lib.bt_last_error_code(), lib.bt_last_error().decode("utf-8", "replace"))
        self._h = C.c_void_p(h)
        self.rank, self.world = rank, world

    def close(self):
        if getattr(self, "_h", None):
            lib.bt_comm_free(self._h)
            self._h = None

    __del__ = close

    def allgather(self, shard, gathered, width, height):
        import torch
        assert gathered.numel() == self.world * shard.numel() == self.world * shard_floats(width, height, self.world)
        _check(lib.bt_allgather_shards_device(self._h, shard.data_ptr(), gathered.data_ptr(), width, height,
                                              torch.cuda.current_stream().cuda_stream))

    def exchange(self, shard, gathered, buffer: "Buffer"):
        """All-gather + un-permute: every rank's `buffer` then holds the whole frame of running sums."""
        import torch
        _check(lib.bt_exchange_frame_device(self._h, shard.data_ptr(), gathered.data_ptr(), buffer.data.data_ptr(),
                                            buffer.width, buffer.height, torch.cuda.current_stream().cuda_stream))


@dataclass
class DenoiseParams:
    """`bt_denoise_params` (include/bendy_hip.h): EXTENSION, not in the reference.  Defaults = bt_denoise_params_default."""
    levels: int = 2
    sigma_color: float = 16.0
    sigma_normal: float = 16.0
    sigma_depth: float = 1.0
    eps_albedo: float = 1e-3

    def _c(self):
        return _CDenoiseParams(int(self.levels), self.sigma_color, self.sigma_normal, self.sigma_depth, self.eps_albedo)


class Denoiser:
    """`bt_denoiser` (include/bendy_hip.h): EXTENSION, not in the reference -- the AOV-guided a-trous denoiser.  The handle
    owns the scratch (48 B per pixel, grown on demand), so a caller that denoises every displayed frame keeps one."""

    def __init__(self):
        h = lib.bt_denoiser_new()
        if not h:
            raise BendyError(-1, "bt_denoiser_new failed")
        self._h = C.c_void_p(h)

    def close(self):
        if getattr(self, "_h", None):
            lib.bt_denoiser_free(self._h)
            self._h = None

    __del__ = close

    def denoise(self, color: Buffer, albedo: Optional[Buffer] = None, normal: Optional[Buffer] = None,
                depth: Optional[Buffer] = None, *, out: Optional[Buffer] = None, **params) -> Buffer:
        """Filters `color` guided by the BT_OUTPUT_ALBEDO / _NORMAL / _DEPTH sums of the same frame (any of them may be
        None), each divided by its own `.samples`.  Returns `out` (a new Buffer by default) holding the MEAN with
        samples = 1 and the colour buffer's color_space, so `.preview()` works unchanged.  Keywords = DenoiseParams fields."""
        p = DenoiseParams(**params)
        bufs = [b for b in (albedo, normal, depth) if b is not None]
        for b in bufs + ([out] if out is not None else []):
            if (b.width, b.height) != (color.width, color.height):
                raise BendyError(-1, f"buffer of {b.width}x{b.height} next to a {color.width}x{color.height} colour buffer")
            if b.device != color.device or (color.device != "cpu" and b.data.device != color.data.device):
                raise BendyError(-1, f"buffer on {b.device} next to a colour buffer on {color.device}")
        if out is not None and any(out is b or out.data is b.data for b in [color] + bufs):
            raise BendyError(-1, "out must not be one of the inputs: the inputs are running sums, out is a mean")
        if out is None:
            out = Buffer(color.width, color.height, color.color_space, device=color.device)
        out.color_space = color.color_space

        def arg(b):
            if b is None:
                return None, 0
            if b.device == "cpu":
                return b.data.ctypes.data_as(C.POINTER(C.c_float)), b.samples
            return b.data.data_ptr(), b.samples

        args = []
        for b in (color, albedo, normal, depth):
            args += list(arg(b))
        cp = p._c()
        if color.device == "cpu":
            _check(lib.bt_denoise(self._h, *args, arg(out)[0], color.width, color.height, C.byref(cp)))
        else:
            import torch
            _check(lib.bt_denoise_device(self._h, *args, out.data.data_ptr(), color.width, color.height, C.byref(cp),
                                         torch.cuda.current_stream().cuda_stream))
        out.samples = 1
        return out


def _adaptive_defaults():
    p = _CAdaptiveParams()
    lib.bt_adaptive_params_default(C.byref(p))
    return p


@dataclass
class AdaptiveParams:
    """`bt_adaptive_params` (include/bendy_hip.h): EXTENSION, not in the reference.  Fields left None take
    bt_adaptive_params_default's value."""
    threshold: Optional[float] = None
    min_samples: Optional[int] = None
    max_samples: Optional[int] = None
    eps: Optional[float] = None

    def __post_init__(self):
        d = _adaptive_defaults()
        for k, _ in _CAdaptiveParams._fields_:
            if getattr(self, k) is None:
                setattr(self, k, getattr(d, k))

    def _c(self):
        return _CAdaptiveParams(float(self.threshold), int(self.min_samples), int(self.max_samples), float(self.eps))


class Adaptive:
    """`bt_adaptive` (include/bendy_hip.h): EXTENSION, not in the reference -- the state of variance-driven adaptive
    sampling for one frame size: a per-pixel second moment and, per 16x16 tile, a sample count, an error
    estimate and an activity flag.  Keywords = AdaptiveParams fields; `Tracer.render_adaptive` runs the passes."""

    def __init__(self, width, height, **params):
        self.params = AdaptiveParams(**params)
        self.width, self.height = int(width), int(height)
        self.tiles_x, self.tiles_y = (self.width + BT_TILE - 1) // BT_TILE, (self.height + BT_TILE - 1) // BT_TILE
        h = lib.bt_adaptive_new(self.width, self.height)
        if not h:
            raise BendyError(lib.bt_last_error_code(), lib.bt_last_error().decode("utf-8", "replace"))
        self._h = C.c_void_p(h)

    def close(self):
        if getattr(self, "_h", None):
            lib.bt_adaptive_free(self._h)
            self._h = None

    __del__ = close

    def reset(self):
        """Zero moments, counts and errors; every tile active again; the next pass starts at sample index 0."""
        _check(lib.bt_adaptive_reset(self._h))

    def poll(self) -> AdaptiveStats:
        """bt_adaptive_poll (synchronises): `.active_tiles == 0` is Status.Done."""
        st = AdaptiveStats()
        _check(lib.bt_adaptive_poll(self._h, C.byref(st)))
        return st

    def counts(self):
        """Samples per pixel each tile holds, uint32 [tiles_y, tiles_x]."""
        n = _check(lib.bt_adaptive_counts(self._h, None, 0))
        out = np.zeros(n, dtype=np.uint32)
        _check(lib.bt_adaptive_counts(self._h, out.ctypes.data_as(C.POINTER(C.c_uint32)), n))
        return out.reshape(self.tiles_y, self.tiles_x)

    def errors(self):
        """Each tile's last error estimate e_t, float32 [tiles_y, tiles_x]."""
        n = _check(lib.bt_adaptive_errors(self._h, None, 0))
        out = np.zeros(n, dtype=np.float32)
        _check(lib.bt_adaptive_errors(self._h, out.ctypes.data_as(C.POINTER(C.c_float)), n))
        return out.reshape(self.tiles_y, self.tiles_x)

    def moments(self):
        """bt_debug_adaptive_moments (tests): each pixel's running sum of squared luminance, float32 [height, width]."""
        n = _check(lib.bt_debug_adaptive_moments(self._h, None, 0))
        out = np.zeros(n, dtype=np.float32)
        _check(lib.bt_debug_adaptive_moments(self._h, out.ctypes.data_as(C.POINTER(C.c_float)), n))
        return out.reshape(self.height, self.width)

    def resolve(self, buffer: Buffer, out: Optional[Buffer] = None) -> Buffer:
        """The MEAN of an adaptively sampled frame: every pixel of `buffer` divided by its own tile's count.  Returns `out`
        (a new Buffer by default) with samples = 1 and `buffer`'s color_space, as `Denoiser.denoise` does, so `.preview()`
        and `denoise(...)` work unchanged."""
        if buffer.device == "cpu":
            raise BendyError(-1, "resolve needs a device-resident buffer")
        if (buffer.width, buffer.height) != (self.width, self.height):
            raise BendyError(-1, f"buffer of {buffer.width}x{buffer.height} on an adaptive handle of {self.width}x{self.height}")
        if out is not None and (out is buffer or out.data is buffer.data):
            raise BendyError(-1, "out must not be the input: the input holds running sums, out is a mean")
        if out is None:
            out = Buffer(buffer.width, buffer.height, buffer.color_space, device=buffer.device)
        if (out.width, out.height) != (self.width, self.height) or out.device == "cpu":
            raise BendyError(-1, "out must be a device-resident buffer of the handle's size")
        out.color_space = buffer.color_space
        import torch
        _check(lib.bt_adaptive_resolve_device(self._h, buffer.data.data_ptr(), out.data.data_ptr(),
                                              torch.cuda.current_stream().cuda_stream))
        out.samples = 1
        return out


def _temporal_defaults():
    p = _CTemporalParams()
    lib.bt_temporal_params_default(C.byref(p))
    return p


@dataclass
class TemporalParams:
    """`bt_temporal_params` (include/bendy_hip.h): EXTENSION, not in the reference.  Fields left None take
    bt_temporal_params_default's value."""
    alpha_min: Optional[float] = None
    max_history: Optional[float] = None
    depth_tolerance: Optional[float] = None
    normal_min: Optional[float] = None

    def __post_init__(self):
        d = _temporal_defaults()
        for k, _ in _CTemporalParams._fields_:
            if getattr(self, k) is None:
                setattr(self, k, getattr(d, k))

    def _c(self):
        return _CTemporalParams(float(self.alpha_min), float(self.max_history), float(self.depth_tolerance), float(self.normal_min))


class Temporal:
    """`bt_temporal` (include/bendy_hip.h): EXTENSION, not in the reference -- temporal accumulation with reprojection for one
    frame size.  The handle owns the previous frame's accumulated colour and guides (64 B per pixel) and the
    previous view.  Keywords = TemporalParams fields."""

    def __init__(self, width, height, **params):
        self.params = TemporalParams(**params)
        self.width, self.height = int(width), int(height)
        h = lib.bt_temporal_new(self.width, self.height)
        if not h:
            raise BendyError(lib.bt_last_error_code(), lib.bt_last_error().decode("utf-8", "replace"))
        self._h = C.c_void_p(h)

    def close(self):
        if getattr(self, "_h", None):
            lib.bt_temporal_free(self._h)
            self._h = None

    __del__ = close

    def reset(self):
        """Forgets the history and the previous view."""
        _check(lib.bt_temporal_reset(self._h))

    def accumulate(self, view: View, color: Buffer, normal: Optional[Buffer] = None, depth: Optional[Buffer] = None, *,
                   out: Optional[Buffer] = None, **params) -> Buffer:
        """Blends this frame's running sums (`color`, `normal`, `depth`, each divided by its own `.samples`; what
        `Tracer.render_guided` wrote into cleared buffers under `view`) into the history reprojected from the previous call's
        view.  `depth` is required, `normal` may be None.  Returns `out` (a new Buffer by default) holding the MEAN with
        samples = 1 and the colour buffer's color_space, so `.preview()` and `denoise(...)` work unchanged.  Keywords
        override the handle's TemporalParams for this call."""
        p = TemporalParams(**{**{k: getattr(self.params, k) for k, _ in _CTemporalParams._fields_}, **params})
        if depth is None:
            raise BendyError(-1, "accumulate needs the frame's depth buffer")
        bufs = [b for b in (normal, depth) if b is not None]
        for b in [color] + bufs + ([out] if out is not None else []):
            if b.device == "cpu":
                raise BendyError(-1, "accumulate needs device-resident buffers (there is no host-buffer variant)")
            if (b.width, b.height) != (self.width, self.height):
                raise BendyError(-1, f"buffer of {b.width}x{b.height} on a temporal handle of {self.width}x{self.height}")
        if out is not None and any(out is b or out.data is b.data for b in [color] + bufs):
            raise BendyError(-1, "out must not be one of the inputs: the inputs are running sums, out is a mean")
        if out is None:
            out = Buffer(color.width, color.height, color.color_space, device=color.device)
        out.color_space = color.color_space
        cp = p._c()
        import torch
        _check(lib.bt_temporal_accumulate_device(self._h, C.byref(view), color.data.data_ptr(), color.samples,
                                                 normal.data.data_ptr() if normal is not None else None,
                                                 normal.samples if normal is not None else 0, depth.data.data_ptr(),
                                                 depth.samples, out.data.data_ptr(), C.byref(cp),
                                                 torch.cuda.current_stream().cuda_stream))
        out.samples = 1
        return out

    def history(self):
        """bt_debug_temporal_history (tests; synchronises): float32 [height, width, 4], rgb = the accumulated mean, a = the
        history length in samples per pixel; zeros while there is no history."""
        n = _check(lib.bt_debug_temporal_history(self._h, None, 0))
        out = np.zeros(n, dtype=np.float32)
        _check(lib.bt_debug_temporal_history(self._h, out.ctypes.data_as(C.POINTER(C.c_float)), n))
        return out.reshape(self.height, self.width, 4)


def reproject(cur: View, prev: View, x, y, z):
    """bt_debug_reproject (tests; host code, no device): where pixel (x, y) of `cur` at normalised depth z (z >= 1: at
    infinity) lies in `prev`: (x_f, y_f, z')."""
    out = (C.c_float * 3)()
    _check(lib.bt_debug_reproject(C.byref(cur), C.byref(prev), x, y, z, out))
    return (out[0], out[1], out[2])


def _display_defaults():
    p = _CDisplayParams()
    lib.bt_display_params_default(C.byref(p))
    return p


@dataclass
class DisplayParams:
    """`bt_display_params` (include/bendy_hip.h): EXTENSION, not in the reference.  Fields left None take
    bt_display_params_default's value; `tonemap` is a Tonemap, its name ("aces") or its number."""
    tonemap: Optional[int] = None
    auto_exposure: Optional[int] = None
    ev: Optional[float] = None
    key: Optional[float] = None
    p_low: Optional[float] = None
    p_high: Optional[float] = None
    adapt: Optional[float] = None
    ev_min: Optional[float] = None
    ev_max: Optional[float] = None
    white: Optional[float] = None

    def __post_init__(self):
        d = _display_defaults()
        for k, _ in _CDisplayParams._fields_:
            if getattr(self, k) is None:
                setattr(self, k, getattr(d, k))
        if isinstance(self.tonemap, str):
            self.tonemap = {t.name.lower(): t for t in Tonemap}[self.tonemap.lower()]

    def _c(self):
        return _CDisplayParams(float(self.key), int(self.tonemap), int(self.auto_exposure),
                               *(float(getattr(self, k)) for k, _ in _CDisplayParams._fields_[3:]))


class Display:
    """`bt_display` (include/bendy_hip.h): EXTENSION, not in the reference -- the display stage: metered auto-exposure, adapted
    from call to call, and a tone operator between the mean and the colour space.  The handle owns the
    luminance counters and the adaptation state on the device.  Keywords = DisplayParams fields."""

    def __init__(self, **params):
        self.params = DisplayParams(**params)
        h = lib.bt_display_new()
        if not h:
            raise BendyError(lib.bt_last_error_code(), lib.bt_last_error().decode("utf-8", "replace"))
        self._h = C.c_void_p(h)

    def close(self):
        if getattr(self, "_h", None):
            lib.bt_display_free(self._h)
            self._h = None

    __del__ = close

    def reset(self):
        """Forgets the adaptation state and the last call."""
        _check(lib.bt_display_reset(self._h))

    def present(self, buffer: Buffer, **params):
        """The frame of `buffer` (running sums of `.samples` samples, or a mean with samples = 1) metered, exposed and mapped
        through the tone operator and the buffer's colour space -> uint8 [H, W, 4] on the host.  Keywords override the
        handle's DisplayParams for this call."""
        p = DisplayParams(**{**{k: getattr(self.params, k) for k, _ in _CDisplayParams._fields_}, **params})
        if buffer.device == "cpu":
            raise BendyError(-1, "present needs a device-resident buffer (there is no host-buffer variant)")
        import torch
        out = torch.empty((buffer.height, buffer.width, 4), dtype=torch.uint8, device=buffer.data.device)
        cp = p._c()
        _check(lib.bt_display_device(self._h, buffer.data.data_ptr(), max(buffer.samples, 1), out.data_ptr(), buffer.width,
                                     buffer.height, int(buffer.color_space), C.byref(cp),
                                     torch.cuda.current_stream().cuda_stream))
        return out.cpu().numpy()

    def exposure(self):
        """(ev, mult) the last `present` showed its frame with (synchronises)."""
        ev, mult = C.c_float(), C.c_float()
        _check(lib.bt_display_exposure(self._h, C.byref(ev), C.byref(mult)))
        return ev.value, mult.value

    def histogram(self):
        """bt_debug_display_histogram (tests; synchronises): (uint32 [256] luminance bins, under, over) of the last metered call."""
        out = np.zeros(258, dtype=np.uint32)
        _check(lib.bt_debug_display_histogram(self._h, out.ctypes.data_as(C.POINTER(C.c_uint32)), 258))
        return out[:256].copy(), int(out[256]), int(out[257])


def _glare_defaults():
    p = _CGlareParams()
    lib.bt_glare_params_default(C.byref(p))
    return p


@dataclass
class GlareParams:
    """`bt_glare_params` (include/bendy_hip.h): EXTENSION, not in the reference.  Fields left None take
    bt_glare_params_default's value."""
    levels: Optional[int] = None
    spread: Optional[float] = None
    strength: Optional[float] = None
    max_value: Optional[float] = None

    def __post_init__(self):
        d = _glare_defaults()
        for k, _ in _CGlareParams._fields_:
            if getattr(self, k) is None:
                setattr(self, k, getattr(d, k))

    def _c(self):
        return _CGlareParams(int(self.levels), float(self.spread), float(self.strength), float(self.max_value))


class Glare:
    """`bt_glare` (include/bendy_hip.h): EXTENSION, not in the reference -- the glare stage: an energy-conserving bloom in
    scene-linear light, ahead of the display stage.  The handle owns the pyramid on the device (< 5.4 B per
    pixel, grown on demand).  Keywords = GlareParams fields."""

    def __init__(self, **params):
        self.params = GlareParams(**params)
        h = lib.bt_glare_new()
        if not h:
            raise BendyError(lib.bt_last_error_code(), lib.bt_last_error().decode("utf-8", "replace"))
        self._h = C.c_void_p(h)

    def close(self):
        if getattr(self, "_h", None):
            lib.bt_glare_free(self._h)
            self._h = None

    __del__ = close

    def apply(self, buffer: Buffer, *, out: Optional[Buffer] = None, **params) -> Buffer:
        """The frame of `buffer` (running sums of `.samples` samples, or a mean with samples = 1) with the glare added -> a
        Buffer holding the MEAN (samples = 1), as `denoise` returns.  Keywords override the handle's GlareParams for this
        call."""
        p = GlareParams(**{**{k: getattr(self.params, k) for k, _ in _CGlareParams._fields_}, **params})
        if buffer.device == "cpu":
            raise BendyError(-1, "apply needs a device-resident buffer (there is no host-buffer variant)")
        import torch
        if out is None:
            out = Buffer(buffer.width, buffer.height, buffer.color_space, device=buffer.device)
        elif (out.width, out.height) != (buffer.width, buffer.height) or out.device == "cpu" or out.data.device != buffer.data.device:
            raise BendyError(-1, f"out must be a {buffer.width}x{buffer.height} buffer on the input's device")
        out.color_space = buffer.color_space
        cp = p._c()
        self._dims = (buffer.width, buffer.height)
        _check(lib.bt_glare_device(self._h, buffer.data.data_ptr(), max(buffer.samples, 1), out.data.data_ptr(), buffer.width,
                                   buffer.height, C.byref(cp), torch.cuda.current_stream().cuda_stream))
        out.samples = 1
        return out

    def plane(self, level):
        """bt_debug_glare_plane (tests; synchronises): A_level of the last `apply` as float32 [h_k, w_k, 4]."""
        n = _check(lib.bt_debug_glare_plane(self._h, int(level), None, 0))
        flat = np.zeros(n, dtype=np.float32)
        _check(lib.bt_debug_glare_plane(self._h, int(level), flat.ctypes.data_as(C.POINTER(C.c_float)), n))
        w, h = self._dims
        for _ in range(int(level)):
            w, h = (w + 1) // 2, (h + 1) // 2
        return flat.reshape(h, w, 4)


def glare_host(array, samples=1, **params):
    """bt_debug_glare_host (tests, no device): the whole glare stage on the host through csrc/bt_glare.hpp's own functions.
    `array`: float32 [H, W, 4] running sums -> the glared mean, float32 [H, W, 4]."""
    a = np.ascontiguousarray(array, dtype=np.float32)
    if a.ndim != 3 or a.shape[2] != 4:
        raise BendyError(-1, "glare_host expects a [H, W, 4] array")
    out = np.empty_like(a)
    cp = GlareParams(**params)._c()
    _check(lib.bt_debug_glare_host(a.ctypes.data_as(C.POINTER(C.c_float)), int(samples), out.ctypes.data_as(C.POINTER(C.c_float)),
                                   a.shape[1], a.shape[0], C.byref(cp)))
    return out


def _resample_defaults():
    p = _CResampleParams()
    lib.bt_resample_params_default(C.byref(p))
    return p


@dataclass
class ResampleParams:
    """`bt_resample_params` (include/bendy_hip.h): EXTENSION, not in the reference.  Fields left None take
    bt_resample_params_default's value; `filter` is a Filter, its name ("lanczos3") or its number."""
    filter: Optional[int] = None
    max_value: Optional[float] = None
    clamp_negative: Optional[int] = None

    def __post_init__(self):
        d = _resample_defaults()
        for k, _ in _CResampleParams._fields_:
            if getattr(self, k) is None:
                setattr(self, k, getattr(d, k))
        if isinstance(self.filter, str):
            names = {f.name.lower(): f for f in Filter}
            if self.filter.lower() not in names:
                raise BendyError(-1, f"unknown filter {self.filter!r}: one of {', '.join(names)}")
            self.filter = names[self.filter.lower()]

    def _c(self):
        return _CResampleParams(int(self.filter), float(self.max_value), int(self.clamp_negative))


class Resample:
    """`bt_resample` (include/bendy_hip.h): EXTENSION, not in the reference -- the resample stage: render at one size, show at
    another, through a separable filter in scene-linear light, after the glare stage and ahead of the display stage
    (DESIGN.md 17).  The handle owns the intermediate plane and both weight tables.  Keywords = ResampleParams fields."""

    def __init__(self, **params):
        self.params = ResampleParams(**params)
        h = lib.bt_resample_new()
        if not h:
            raise BendyError(lib.bt_last_error_code(), lib.bt_last_error().decode("utf-8", "replace"))
        self._h = C.c_void_p(h)
        self._plane_dims = None

    def close(self):
        if getattr(self, "_h", None):
            lib.bt_resample_free(self._h)
            self._h = None

    __del__ = close

    def _params(self, params):
        return ResampleParams(**{**{k: getattr(self.params, k) for k, _ in _CResampleParams._fields_}, **params})

    def apply(self, buffer: Buffer, width, height, *, out: Optional[Buffer] = None, **params) -> Buffer:
        """The frame of `buffer` (running sums of `.samples` samples, or a mean with samples = 1) resampled to width x height ->
        a Buffer holding the MEAN (samples = 1) with the input's colour space, as `Glare.apply` returns.  Keywords override the
        handle's ResampleParams for this call."""
        p = self._params(params)
        width, height = int(width), int(height)
        if buffer.device == "cpu":
            raise BendyError(-1, "apply needs a device-resident buffer (there is no host-buffer variant)")
        if width < 1 or height < 1:
            raise BendyError(-1, f"cannot resample to {width}x{height}")
        import torch
        if out is None:
            out = Buffer(width, height, buffer.color_space, device=buffer.device)
        elif (out.width, out.height) != (width, height) or out.device == "cpu" or out.data.device != buffer.data.device:
            raise BendyError(-1, f"out must be a {width}x{height} buffer on the input's device")
        out.color_space = buffer.color_space
        cp = p._c()
        _check(lib.bt_resample_device(self._h, buffer.data.data_ptr(), max(buffer.samples, 1), buffer.width, buffer.height,
                                      out.data.data_ptr(), width, height, C.byref(cp), torch.cuda.current_stream().cuda_stream))
        self._plane_dims = (width, buffer.height)
        out.samples = 1
        return out

    def host(self, array, samples, width, height, **params):
        """bt_debug_resample_host on this handle (tests, no device): as `resample_host`, and the handle keeps the tables the call
        used, for `weights`."""
        return resample_host(array, samples, width, height, _handle=self._h, **{**{k: getattr(self.params, k) for k, _ in _CResampleParams._fields_}, **params})

    def weights(self, axis):
        """bt_debug_resample_weights (tests): the table of axis 0 / "x" or 1 / "y" of the handle's last call ->
        (first int32 [dst], T, weights float32 [dst, T], nearest uint32 [dst])."""
        axis = {"x": 0, "y": 1}.get(axis, axis)
        sides = (C.c_uint32 * 3)()
        taps = _check(lib.bt_debug_resample_weights(self._h, int(axis), sides, None, None, None))
        dst = int(sides[1])
        first, w, near = np.zeros(dst, dtype=np.int32), np.zeros((dst, taps), dtype=np.float32), np.zeros(dst, dtype=np.uint32)
        _check(lib.bt_debug_resample_weights(self._h, int(axis), sides, first.ctypes.data_as(C.POINTER(C.c_int32)),
                                             w.ctypes.data_as(C.POINTER(C.c_float)), near.ctypes.data_as(C.POINTER(C.c_uint32))))
        return first, taps, w, near

    def plane(self):
        """bt_debug_resample_plane (tests; synchronises): P of the last `apply` as float32 [h, W, 4]."""
        n = _check(lib.bt_debug_resample_plane(self._h, None, 0))
        flat = np.zeros(n, dtype=np.float32)
        _check(lib.bt_debug_resample_plane(self._h, flat.ctypes.data_as(C.POINTER(C.c_float)), n))
        w, h = self._plane_dims
        return flat.reshape(h, w, 4)


def resample_host(array, samples, width, height, _handle=None, **params):
    """bt_debug_resample_host (tests, no device): the whole resample stage on the host through csrc/bt_resample.hpp's own
    functions.  `array`: float32 [h, w, 4] running sums -> the resampled mean, float32 [height, width, 4]."""
    a = np.ascontiguousarray(array, dtype=np.float32)
    if a.ndim != 3 or a.shape[2] != 4:
        raise BendyError(-1, "resample_host expects a [H, W, 4] array")
    out = np.empty((max(int(height), 0), max(int(width), 0), 4), dtype=np.float32)
    cp = ResampleParams(**params)._c()
    _check(lib.bt_debug_resample_host(_handle, a.ctypes.data_as(C.POINTER(C.c_float)), int(samples), a.shape[1], a.shape[0],
                                      out.ctypes.data_as(C.POINTER(C.c_float)), int(width), int(height), C.byref(cp)))
    return out


def _despeckle_defaults():
    p = _CDespeckleParams()
    lib.bt_despeckle_params_default(C.byref(p))
    return p


@dataclass
class DespeckleParams:
    """`bt_despeckle_params` (include/bendy_hip.h): EXTENSION, not in the reference.  Fields left None take
    bt_despeckle_params_default's value."""
    radius: Optional[int] = None
    rank: Optional[int] = None
    ratio: Optional[float] = None
    floor: Optional[float] = None
    max_value: Optional[float] = None

    def __post_init__(self):
        d = _despeckle_defaults()
        for k, _ in _CDespeckleParams._fields_:
            if getattr(self, k) is None:
                setattr(self, k, getattr(d, k))

    def _c(self):
        return _CDespeckleParams(int(self.radius), int(self.rank), float(self.ratio), float(self.floor), float(self.max_value))


class Despeckle:
    """`bt_despeckle` (include/bendy_hip.h): EXTENSION, not in the reference -- the despeckle stage: rank-order firefly rejection
    on a frame of running sums, ahead of every other stage.  The handle owns two counters on the device.
    Keywords = DespeckleParams fields."""

    def __init__(self, **params):
        self.params = DespeckleParams(**params)
        h = lib.bt_despeckle_new()
        if not h:
            raise BendyError(lib.bt_last_error_code(), lib.bt_last_error().decode("utf-8", "replace"))
        self._h = C.c_void_p(h)

    def close(self):
        if getattr(self, "_h", None):
            lib.bt_despeckle_free(self._h)
            self._h = None

    __del__ = close

    def apply(self, buffer: Buffer, *, out: Optional[Buffer] = None, **params) -> Buffer:
        """The frame of `buffer` (running sums of `.samples` samples, or a mean with samples = 1) with its outliers pulled down
        -> a Buffer of SUMS of the same `.samples`, with the input's colour space: it takes the input's place anywhere in the
        chain.  Keywords override the handle's DespeckleParams for this call."""
        p = DespeckleParams(**{**{k: getattr(self.params, k) for k, _ in _CDespeckleParams._fields_}, **params})
        if buffer.device == "cpu":
            raise BendyError(-1, "apply needs a device-resident buffer (there is no host-buffer variant)")
        import torch
        if out is None:
            out = Buffer(buffer.width, buffer.height, buffer.color_space, device=buffer.device)
        elif out is buffer:
            raise BendyError(-1, "out must not be the input: every neighbour value is the input's")
        elif (out.width, out.height) != (buffer.width, buffer.height) or out.device == "cpu" or out.data.device != buffer.data.device:
            raise BendyError(-1, f"out must be a {buffer.width}x{buffer.height} buffer on the input's device")
        out.color_space = buffer.color_space
        cp = p._c()
        _check(lib.bt_despeckle_device(self._h, buffer.data.data_ptr(), max(buffer.samples, 1), out.data.data_ptr(), buffer.width,
                                       buffer.height, C.byref(cp), torch.cuda.current_stream().cuda_stream))
        out.samples = buffer.samples
        return out

    def poll(self) -> DespeckleStats:
        """bt_despeckle_poll (synchronises): the last `apply`'s DespeckleStats -- flagged, sanitised, pixels."""
        st = DespeckleStats()
        _check(lib.bt_despeckle_poll(self._h, C.byref(st)))
        return st


def despeckle_host(array, samples=1, stats=False, **params):
    """bt_debug_despeckle_host (tests, no device): the whole despeckle stage on the host through csrc/bt_despeckle.hpp's own
    functions.  `array`: float32 [H, W, 4] running sums -> the despeckled sums, float32 [H, W, 4]; with stats=True also the
    DespeckleStats."""
    a = np.ascontiguousarray(array, dtype=np.float32)
    if a.ndim != 3 or a.shape[2] != 4:
        raise BendyError(-1, "despeckle_host expects a [H, W, 4] array")
    out = np.empty_like(a)
    cp = DespeckleParams(**params)._c()
    st = DespeckleStats()
    _check(lib.bt_debug_despeckle_host(a.ctypes.data_as(C.POINTER(C.c_float)), int(samples), out.ctypes.data_as(C.POINTER(C.c_float)),
                                       a.shape[1], a.shape[0], C.byref(cp), C.byref(st)))
    return (out, st) if stats else out


def _upscale_defaults():
    p = _CUpscaleParams()
    lib.bt_upscale_params_default(C.byref(p))
    return p


@dataclass
class UpscaleParams:
    """`bt_upscale_params` (include/bendy_hip.h): EXTENSION, not in the reference.  Fields left None take
    bt_upscale_params_default's value."""
    sigma_depth: Optional[float] = None
    sigma_albedo: Optional[float] = None
    normal_squarings: Optional[int] = None
    min_weight: Optional[float] = None
    max_value: Optional[float] = None

    def __post_init__(self):
        d = _upscale_defaults()
        for k, _ in _CUpscaleParams._fields_:
            if getattr(self, k) is None:
                setattr(self, k, getattr(d, k))

    def _c(self):
        return _CUpscaleParams(float(self.sigma_depth), float(self.sigma_albedo), int(self.normal_squarings), float(self.min_weight),
                               float(self.max_value))


def _guide_triple(guides, what):
    g = (None, None, None) if guides is None else tuple(guides)
    if len(g) != 3:
        raise BendyError(-1, f"{what} must be (albedo, normal, depth), any of them None")
    return g


class Upscale:
    """`bt_upscale` (include/bendy_hip.h): EXTENSION, not in the reference -- the upscale stage: a small colour frame shown at a
    larger size, every lo texel weighed by how well its albedo, normal and depth match the output pixel's own (joint bilateral
    upsampling).  It sits after the denoiser and before the glare stage.  The handle owns the prepared planes, both
    tables and the tier counter.  Keywords = UpscaleParams fields."""

    def __init__(self, **params):
        self.params = UpscaleParams(**params)
        h = lib.bt_upscale_new()
        if not h:
            raise BendyError(lib.bt_last_error_code(), lib.bt_last_error().decode("utf-8", "replace"))
        self._h = C.c_void_p(h)
        self._plane_dims = None

    def close(self):
        if getattr(self, "_h", None):
            lib.bt_upscale_free(self._h)
            self._h = None

    __del__ = close

    def _merged(self, params):
        return {**{k: getattr(self.params, k) for k, _ in _CUpscaleParams._fields_}, **params}

    def apply(self, color: Buffer, width, height, *, lo=None, hi=None, out: Optional[Buffer] = None, **params) -> Buffer:
        """The frame of `color` (running sums of `.samples` samples, or a mean with samples = 1) upsampled to width x height ->
        a Buffer holding the MEAN (samples = 1) with the input's colour space.  `lo` = (albedo, normal, depth) Buffers of the
        input's size, `hi` the same at width x height; any element may be None, but a guide is given at both sizes or at
        neither.  Keywords override the handle's UpscaleParams for this call."""
        p = UpscaleParams(**self._merged(params))
        width, height = int(width), int(height)
        lo, hi = _guide_triple(lo, "lo"), _guide_triple(hi, "hi")
        if color.device == "cpu" or any(g is not None and g.device == "cpu" for g in lo + hi):
            raise BendyError(-1, "apply needs device-resident buffers (there is no host-buffer variant)")
        if width < 1 or height < 1:
            raise BendyError(-1, f"cannot upscale to {width}x{height}")
        for g in lo:
            if g is not None and (g.width, g.height) != (color.width, color.height):
                raise BendyError(-1, f"a lo guide must be {color.width}x{color.height}, the colour frame's size")
        for g in hi:
            if g is not None and (g.width, g.height) != (width, height):
                raise BendyError(-1, f"a hi guide must be {width}x{height}, the output's size")
        import torch
        if out is None:
            out = Buffer(width, height, color.color_space, device=color.device)
        elif (out.width, out.height) != (width, height) or out.device == "cpu" or out.data.device != color.data.device:
            raise BendyError(-1, f"out must be a {width}x{height} buffer on the input's device")
        out.color_space = color.color_space
        cp, gl, gh = p._c(), _device_guides(lo), _device_guides(hi)
        _check(lib.bt_upscale_device(self._h, color.data.data_ptr(), max(color.samples, 1), color.width, color.height, C.byref(gl),
                                     C.byref(gh), out.data.data_ptr(), width, height, C.byref(cp), torch.cuda.current_stream().cuda_stream))
        self._plane_dims = (color.width, color.height)
        out.samples = 1
        return out

    def poll(self) -> UpscaleStats:
        """bt_upscale_poll (synchronises): the last `apply`'s UpscaleStats -- tier2, tier3, pixels."""
        st = UpscaleStats()
        _check(lib.bt_upscale_poll(self._h, C.byref(st)))
        return st

    def host(self, color, samples, width, height, **kw):
        """bt_debug_upscale_host on this handle (tests, no device): as `upscale_host`, and the handle keeps the tables the call
        used, for `weights`."""
        return upscale_host(color, samples, width, height, _handle=self._h, **self._merged(kw))

    def weights(self, axis):
        """bt_debug_upscale_weights (tests): the table of axis 0 / "x" or 1 / "y" of the handle's last call ->
        (first int32 [dst], weights float32 [dst, 8] -- the narrow four, then the wide four --, nearest uint32 [dst])."""
        axis = {"x": 0, "y": 1}.get(axis, axis)
        sides = (C.c_uint32 * 2)()
        n = _check(lib.bt_debug_upscale_weights(self._h, int(axis), sides, None, None, None))
        dst = int(sides[1])
        first, w, near = np.zeros(dst, dtype=np.int32), np.zeros((dst, n), dtype=np.float32), np.zeros(dst, dtype=np.uint32)
        _check(lib.bt_debug_upscale_weights(self._h, int(axis), sides, first.ctypes.data_as(C.POINTER(C.c_int32)),
                                            w.ctypes.data_as(C.POINTER(C.c_float)), near.ctypes.data_as(C.POINTER(C.c_uint32))))
        return first, w, near

    def plane(self, which):
        """bt_debug_upscale_plane (tests; synchronises): a prepared lo plane of the last `apply` as float32 [h, w, 4] -- 0 /
        "colour": (c.rgb, z), 1 / "normal": (n.xyz, 0), 2 / "albedo": (a.rgb, 0)."""
        which = {"colour": 0, "color": 0, "normal": 1, "albedo": 2}.get(which, which)
        n = _check(lib.bt_debug_upscale_plane(self._h, int(which), None, 0))
        flat = np.zeros(n, dtype=np.float32)
        _check(lib.bt_debug_upscale_plane(self._h, int(which), flat.ctypes.data_as(C.POINTER(C.c_float)), n))
        w, h = self._plane_dims
        return flat.reshape(h, w, 4)


def _device_guides(triple):
    g = _CUpscaleGuides()
    for name, b in zip(("albedo", "normal", "depth"), triple):
        if b is not None:
            setattr(g, name, b.data.data_ptr())
            setattr(g, name + "_samples", max(b.samples, 1))
    return g


def _host_guides(triple, shape, what, keep):
    """(albedo, normal, depth), each None, an array [H, W, 4] (a mean) or (array, samples) -> bt_upscale_guides."""
    g = _CUpscaleGuides()
    for name, v in zip(("albedo", "normal", "depth"), triple):
        if v is None:
            continue
        arr, n = v if isinstance(v, tuple) else (v, 1)
        a = np.ascontiguousarray(arr, dtype=np.float32)
        if a.shape != shape:
            raise BendyError(-1, f"a {what} guide must be an array of shape {shape}")
        keep.append(a)
        setattr(g, name, a.ctypes.data)
        setattr(g, name + "_samples", int(n))
    return g


def upscale_host(color, samples, width, height, *, lo=None, hi=None, stats=False, _handle=None, **params):
    """bt_debug_upscale_host (tests, no device): the whole upscale stage on the host through csrc/bt_upscale.hpp's own functions.
    `color`: float32 [h, w, 4] running sums of `samples`; `lo` / `hi`: (albedo, normal, depth), each None, an array of sums with
    count 1 or (array, count) -> the mean, float32 [height, width, 4]; with stats=True also the UpscaleStats."""
    a = np.ascontiguousarray(color, dtype=np.float32)
    if a.ndim != 3 or a.shape[2] != 4:
        raise BendyError(-1, "upscale_host expects a [H, W, 4] array")
    width, height = int(width), int(height)
    out = np.empty((max(height, 0), max(width, 0), 4), dtype=np.float32)
    keep = []
    gl = _host_guides(_guide_triple(lo, "lo"), a.shape, "lo", keep)
    gh = _host_guides(_guide_triple(hi, "hi"), out.shape, "hi", keep)
    cp = UpscaleParams(**params)._c()
    st = UpscaleStats()
    _check(lib.bt_debug_upscale_host(_handle, a.ctypes.data_as(C.POINTER(C.c_float)), int(samples), a.shape[1], a.shape[0], C.byref(gl),
                                     C.byref(gh), out.ctypes.data_as(C.POINTER(C.c_float)), width, height, C.byref(cp), C.byref(st)))
    return (out, st) if stats else out


_default_denoiser = None


def _compare_defaults():
    p = _CCompareParams()
    lib.bt_compare_params_default(C.byref(p))
    return p


@dataclass
class CompareParams:
    """`bt_compare_params` (include/bendy_hip.h): EXTENSION, not in the reference.  Fields left None take
    bt_compare_params_default's value."""
    epsilon: Optional[float] = None
    peak: Optional[float] = None

    def __post_init__(self):
        d = _compare_defaults()
        for k, _ in _CCompareParams._fields_:
            if getattr(self, k) is None:
                setattr(self, k, getattr(d, k))

    def _c(self):
        return _CCompareParams(float(self.epsilon), float(self.peak))


class Compare:
    """`bt_compare` (include/bendy_hip.h): EXTENSION, not in the reference -- the compare stage: how far a test frame is from a
    reference frame (MSE, relMSE, PSNR, SSIM, the largest difference, the tail share, an error map), bit-identical
    between the device, the host entry point and numpy.  It measures the chain and changes no frame.  The handle owns three planes
    (28 B per pixel), a slab of one slot per tile and the histograms.  Keywords = CompareParams fields."""

    def __init__(self, **params):
        self.params = CompareParams(**params)
        h = lib.bt_compare_new()
        if not h:
            raise BendyError(lib.bt_last_error_code(), lib.bt_last_error().decode("utf-8", "replace"))
        self._h = C.c_void_p(h)
        self._size = None

    def close(self):
        if getattr(self, "_h", None):
            lib.bt_compare_free(self._h)
            self._h = None

    __del__ = close

    def measure(self, test: Buffer, reference: Buffer, **params) -> CompareStats:
        """bt_compare_device, then bt_compare_poll (synchronises): `test` against `reference`, device Buffers of equal size, each
        running sums of its `.samples` (or a mean with samples = 1); they may be the same Buffer.  Keywords override the handle's
        CompareParams for this call."""
        p = CompareParams(**{**{k: getattr(self.params, k) for k, _ in _CCompareParams._fields_}, **params})
        if test.device == "cpu" or reference.device == "cpu":
            raise BendyError(-1, "measure needs device-resident buffers (there is no host-buffer variant)")
        if (test.width, test.height) != (reference.width, reference.height) or test.data.device != reference.data.device:
            raise BendyError(-1, f"the frames differ: {test.width}x{test.height} against {reference.width}x{reference.height}, or in device")
        import torch
        cp = p._c()
        _check(lib.bt_compare_device(self._h, test.data.data_ptr(), max(test.samples, 1), reference.data.data_ptr(), max(reference.samples, 1),
                                     test.width, test.height, C.byref(cp), torch.cuda.current_stream().cuda_stream))
        self._size = (test.width, test.height, test.data.device)
        return self.poll()

    def poll(self) -> CompareStats:
        """bt_compare_poll (synchronises): the last `measure`'s CompareStats."""
        st = CompareStats()
        _check(lib.bt_compare_poll(self._h, C.byref(st)))
        return st

    def tail(self, fraction=0.01):
        """bt_compare_tail (synchronises) -> (share, threshold): the share of the summed error plane that the worst `fraction` of
        the last `measure`'s valid pixels carry, and the error of the last of them."""
        share, threshold = C.c_double(0.0), C.c_float(0.0)
        _check(lib.bt_compare_tail(self._h, float(fraction), C.byref(share), C.byref(threshold)))
        return share.value, threshold.value

    def map(self, scale=1.0, out=None):
        """bt_compare_map_device: the last `measure`'s error plane in false colour (black, red, yellow, white at `scale`; a
        non-finite pixel magenta) -> an RGBA8 device tensor [H, W, 4]."""
        import torch
        if self._size is None:
            raise BendyError(-1, "map before a measure call")
        w, h, dev = self._size
        if out is None:
            out = torch.empty((h, w, 4), dtype=torch.uint8, device=dev)
        elif tuple(out.shape) != (h, w, 4) or out.dtype != torch.uint8 or out.device != dev or not out.is_contiguous():
            raise BendyError(-1, f"out must be a contiguous uint8 [{h}, {w}, 4] tensor on the frames' device")
        _check(lib.bt_compare_map_device(self._h, out.data_ptr(), float(scale), torch.cuda.current_stream().cuda_stream))
        return out

    def plane(self, which):
        """bt_debug_compare_plane (tests; synchronises): 0 / "E" -> float32 [h, w]; 1 / "v" -> float64 [h, w, 2]; 2 / "s" ->
        float64 [h, w]."""
        which = {"E": 0, "v": 1, "s": 2}.get(which, which)
        n = _check(lib.bt_debug_compare_plane(self._h, int(which), None, 0))
        flat = np.empty(n, dtype=np.float32 if which == 0 else np.float64)
        _check(lib.bt_debug_compare_plane(self._h, int(which), flat.ctypes.data_as(C.c_void_p), n))
        w, h, _ = self._size
        return flat.reshape(h, w, 2) if which == 1 else flat.reshape(h, w)


def compare_host(test, reference, test_samples=1, reference_samples=1, tail=(), **params):
    """bt_debug_compare_host (tests, no device): the whole compare stage on the host through csrc/bt_compare.hpp's own functions.
    `test`, `reference`: float32 [H, W, 4] running sums -> (CompareStats, E float32 [H, W], v float64 [H, W, 2], s float64 [H, W],
    [(share, threshold) for each fraction of `tail`])."""
    a = np.ascontiguousarray(test, dtype=np.float32)
    b = np.ascontiguousarray(reference, dtype=np.float32)
    if a.ndim != 3 or a.shape[2] != 4 or a.shape != b.shape:
        raise BendyError(-1, "compare_host expects two [H, W, 4] arrays of one shape")
    h, w = a.shape[:2]
    E, V, S = np.empty((h, w), dtype=np.float32), np.empty((h, w, 2), dtype=np.float64), np.empty((h, w), dtype=np.float64)
    fr = np.asarray(list(tail), dtype=np.float64)
    shares, thresholds = np.zeros(len(fr), dtype=np.float64), np.zeros(len(fr), dtype=np.float32)
    cp = CompareParams(**params)._c()
    st = CompareStats()
    fp, dp = C.POINTER(C.c_float), C.POINTER(C.c_double)
    _check(lib.bt_debug_compare_host(a.ctypes.data_as(fp), int(test_samples), b.ctypes.data_as(fp), int(reference_samples), w, h, C.byref(cp),
                                     C.byref(st), E.ctypes.data_as(fp), V.ctypes.data_as(dp), S.ctypes.data_as(dp), len(fr),
                                     fr.ctypes.data_as(dp), shares.ctypes.data_as(dp), thresholds.ctypes.data_as(fp)))
    return st, E, V, S, [(float(s), float(t)) for s, t in zip(shares, thresholds)]


def hits_numpy(hits):
    """The uint8 [n, 64] tensor of `Scene.query` as a numpy array of HIT_DTYPE records (synchronises; copies to the host)."""
    return hits.cpu().numpy().reshape(-1).view(HIT_DTYPE)


def view_rays(view: View, x0, y0, w, h, out=None):
    """EXTENSION, not in the reference (bt_view_rays_device): the rays through the footprint centres of the pixels
    of a rectangle of `view`'s frame, row-major -- a CUDA float32 tensor [w * h, 8] that `Scene.query` takes.  Enqueued on the
    current stream, not synchronised."""
    import torch
    if out is None:
        out = torch.empty((max(int(w) * int(h), 0), 8), dtype=torch.float32, device="cuda")
    elif not (out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (w * h, 8) and out.is_contiguous()):
        raise BendyError(-1, f"out must be a contiguous CUDA float32 tensor [{w * h}, 8]")
    _check(lib.bt_view_rays_device(C.byref(view), x0, y0, w, h, out.data_ptr(), torch.cuda.current_stream().cuda_stream))
    return out


def read_pfm(path):
    """bt_read_pfm -> (float32 [H, W, 4] with the rows top-down and alpha 1, width, height)."""
    w, h = C.c_uint32(0), C.c_uint32(0)
    _check(lib.bt_read_pfm(os.fsencode(path), None, 0, C.byref(w), C.byref(h)))
    a = np.empty((h.value, w.value, 4), dtype=np.float32)
    _check(lib.bt_read_pfm(os.fsencode(path), a.ctypes.data_as(C.POINTER(C.c_float)), a.size, C.byref(w), C.byref(h)))
    return a, w.value, h.value


def denoise(color: Buffer, albedo: Optional[Buffer] = None, normal: Optional[Buffer] = None, depth: Optional[Buffer] = None,
            *, out: Optional[Buffer] = None, **params) -> Buffer:
    """EXTENSION, not in the reference: Denoiser.denoise on a process-wide handle (see there)."""
    global _default_denoiser
    if _default_denoiser is None:
        _default_denoiser = Denoiser()
    return _default_denoiser.denoise(color, albedo, normal, depth, out=out, **params)


def write_png(path, rgba8):
    """buffer.preview().save(path) (main.rs:275-298)."""
    a = np.ascontiguousarray(rgba8, dtype=np.uint8)
    _check(lib.bt_write_png(os.fspath(path).encode(), a.ctypes.data_as(C.POINTER(C.c_uint8)), a.shape[1], a.shape[0]))


def write_pfm(path, rgba, samples=1):
    """EXTENSION, not in the reference: the linear mean rgb * (1 / samples) of a float32 [H, W, 4] frame as a Portable Float Map."""
    a = np.ascontiguousarray(rgba, dtype=np.float32)
    _check(lib.bt_write_pfm(os.fspath(path).encode(), a.ctypes.data_as(C.POINTER(C.c_float)), a.shape[1], a.shape[0], int(samples)))


def shard_floats(width, height, world):
    return lib.bt_shard_floats(width, height, world)


def new_shard(width, height, world, device="cuda"):
    """A fresh shard accumulator: zeros with alpha = 1 (Buffer::new, buffer.rs:41-50)."""
    import torch
    s = torch.zeros(shard_floats(width, height, world), dtype=torch.float32, device=device)
    s.view(-1, 4)[:, 3] = 1.0
    return s


def unshard(gathered, buffer: Buffer, world):
    import torch
    _check(lib.bt_unshard_device(gathered.data_ptr(), buffer.data.data_ptr(), buffer.width, buffer.height, world,
                                 torch.cuda.current_stream().cuda_stream))


def tile_owner_map(width, height, world):
    """Which rank owns each BT_TILE x BT_TILE tile: tile t (row-major) -> t % world."""
    tx, ty = (width + BT_TILE - 1) // BT_TILE, (height + BT_TILE - 1) // BT_TILE
    return (np.arange(tx * ty) % world).reshape(ty, tx)
