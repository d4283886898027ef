"""nart_amd: MI355X-native render path for shanesimmsart/nart's tiled path tracer.

The package holds the C-ABI libraries (built in-tree into nart_amd/lib) and their Python
bindings; see DESIGN.md for the architecture and INTEGRATION.md for the drop-in boundary.
"""
from .api import (HIP_SYMBOLS, PIXEL_FLOATS, SCENE_SYMBOLS, HipRenderer, bvh_info, bvh_dump, NartError, NativeLibraryMissing,  # noqa: F401
                  RenderParams, RenderStats, Scene, combine_tiles, default_params, filter_table, finalize,
                  hip_lib, load_sessions, parse_args, read_exr, scene_lib, session_geometry, shard_buckets,
                  write_exr, DenoiseParams, sample_variance, AdaptiveParams, adaptive_levels, spp_image,
                  CascadeParams, cascade_levels, MatteParams, matte_ids, GuideParams, LIGHT_GROUPS_MAX,
                  DEPTH_CUTS_MAX, EVAL_OPS, EVAL_WORDS, EVAL_MASKS, FT_ALL, cost_grid, half_mean,
                  TRACE_VARIANTS, TRACE_IN_WORDS, TRACE_OUT_WORDS, TRACE_NO_HIT, TRACE_CLOSEST, TRACE_ANY, trace_rays,
                  SCENE_OPS, SCENE_IN_WORDS, SCENE_OUT_WORDS, SCENE_WALK_SEGMENTS, SCENE_BUILDS, SCENE_BUILD_MASKS,
                  scene_builds_fitting)

__all__ = ["HipRenderer", "bvh_info", "bvh_dump", "NartError", "NativeLibraryMissing", "RenderParams", "RenderStats", "Scene",
           "combine_tiles", "default_params", "filter_table", "finalize", "load_sessions", "parse_args", "read_exr",
           "write_exr", "hip_lib", "scene_lib", "session_geometry", "PIXEL_FLOATS", "HIP_SYMBOLS", "SCENE_SYMBOLS",
           "DenoiseParams", "sample_variance", "AdaptiveParams", "adaptive_levels", "spp_image",
           "CascadeParams", "cascade_levels", "MatteParams", "matte_ids", "GuideParams", "LIGHT_GROUPS_MAX",
           "DEPTH_CUTS_MAX", "EVAL_OPS", "EVAL_WORDS", "EVAL_MASKS", "FT_ALL", "cost_grid", "half_mean",
           "TRACE_VARIANTS", "TRACE_IN_WORDS", "TRACE_OUT_WORDS", "TRACE_NO_HIT", "TRACE_CLOSEST", "TRACE_ANY", "trace_rays",
           "SCENE_OPS", "SCENE_IN_WORDS", "SCENE_OUT_WORDS", "SCENE_WALK_SEGMENTS", "SCENE_BUILDS", "SCENE_BUILD_MASKS",
           "scene_builds_fitting"]
