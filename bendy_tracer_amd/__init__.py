"""bendy_tracer_amd -- MI355X (gfx950) implementation of bendy-tracer's per-sample hot path.

Only what the path needs lives here: `csrc/` (HIP kernels + scene loader + C ABI, built
into `libbendy_hip.so`) and `api.py` (host-side mirror of the reference's Rust API).
Importing the package loads the shared library; a missing library is an ImportError.
"""
from .api import (Adaptive, AdaptiveParams, AdaptiveStats, BendyError, Buffer, ColorSpace, Comm, Compare, CompareParams, CompareStats, Config, DenoiseParams, Denoiser, Despeckle, DespeckleParams, DespeckleStats, Display, DisplayParams, Filter, Glare, GlareParams, Output, RenderConfig, Resample, ResampleParams, Scene, Stats,
                  Status, Subsample, Temporal, TemporalParams, Tonemap, Tracer, Upscale, UpscaleParams, UpscaleStats, View, HIT_DTYPE, RAY_DTYPE, compare_host, denoise, despeckle_host, glare_host, hits_numpy, new_shard, read_pfm, reproject, resample_host, shard_floats, tile_owner_map, unshard, upscale_host, view_rays, write_pfm, write_png)

__all__ = ["Adaptive", "AdaptiveParams", "AdaptiveStats", "BendyError", "Buffer", "ColorSpace", "Comm", "Compare", "CompareParams", "CompareStats", "Config", "DenoiseParams", "Denoiser", "Despeckle", "DespeckleParams", "DespeckleStats", "Display", "DisplayParams", "Filter", "Glare", "GlareParams", "Output", "RenderConfig", "Resample", "ResampleParams",
           "Scene", "Stats", "Status", "Subsample", "Temporal", "TemporalParams", "Tonemap", "Tracer", "Upscale", "UpscaleParams", "UpscaleStats", "View", "HIT_DTYPE", "RAY_DTYPE", "compare_host", "denoise", "despeckle_host", "glare_host", "hits_numpy", "new_shard", "read_pfm", "reproject", "resample_host", "shard_floats", "tile_owner_map",
           "unshard", "upscale_host", "view_rays", "write_pfm", "write_png"]
