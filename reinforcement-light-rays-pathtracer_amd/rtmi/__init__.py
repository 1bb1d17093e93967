"""rtmi — MI355X-native Monte Carlo path tracer (Python binding).

The compute path is librtmi.so (hand-written HIP kernels for gfx950 behind
the C ABI in include/rtmi.h); this package only binds it.  Importing rtmi
does not touch the GPU.
"""
from ._lib import (LIB_PATH, RT_HIT_NONE, RT_HIT_RULE_CPU, RT_HIT_RULE_GPU, RT_HIT_TYPE_LIGHT,
                   RT_HIT_TYPE_SURFACE, RT_PRESET_CPU, RT_PRESET_GPU, RT_SAMPLER_COSINE,
                   RT_SAMPLER_UNIFORM, RT_KT_RENDER_PS, RT_KT_RENDER, RT_KT_SARSA_RENDER, RT_KT_SARSA_APPLY,
                   RT_KT_DQN_MLP, RT_KT_DQN_BOUNCE, RT_KT_DQN_CAMERA, RT_KT_SARSA_VIEW, RT_KT_SARSA_NEAREST, RT_KT_PROBE, RT_KT_BAKE, RT_KT_COUNT, RtCamera, RtError,
                   RtParams, RtIrrOpts, RT_SARSA_KNN_MAX, RT_IRR_MEAN, RT_IRR_CONE, RtDqnViewOpts,
                   RT_DQN_VIEW_IRRADIANCE, RtGlyphViewOpts, RT_GLYPH_MAX, RT_GLYPH_SECTORS, RT_GLYPH_TRIS,
                   RT_GLYPH_RATIO, RT_GLYPH_MAGNITUDE, RT_NEE_DIRECT_ONLY, check, lib)
from .api import (CAMERAS, OBJ_KINDS, Context, Geometry, Scene, camera, cornell_geometry,
                  default_params, filter_records, intersect, intersect_device, intersect_method, intersect_cand,
                  CAND_TABLE, CAND_GIVEN, CAND_CAP_TABLE, CAND_CAP_SHARED, ISECT_SCAN,
                  ISECT_FILTER, ISECT_MFMA, ISECT_BVH, ACCEL_AUTO, ACCEL_SCAN, ACCEL_BVH,
                  obj_geometry, pack_argb,
                  rect_candidates, ctab_candidates, render, render_tiles_device, save_bmp, save_png,
                  ktime_enable, ktime_read, ktime_name, render_nee, render_nee_tiles_device, nee_light_table,
                  nee_sample)
from . import dist, dqn, glyphs, metrics, probe, sarsa, tiles
from .glyphs import Glyphs, glyph_colours, glyph_mesh, read_selected

__all__ = [
    "LIB_PATH", "RT_HIT_NONE", "RT_HIT_RULE_CPU", "RT_HIT_RULE_GPU", "RT_HIT_TYPE_LIGHT",
    "RT_HIT_TYPE_SURFACE", "RT_PRESET_CPU", "RT_PRESET_GPU", "RT_SAMPLER_COSINE",
    "RT_SAMPLER_UNIFORM", "RtCamera", "RtError", "RtParams", "lib", "CAMERAS", "OBJ_KINDS",
    "Context", "Geometry", "Scene", "camera", "cornell_geometry", "default_params", "filter_records", "intersect",
    "intersect_device", "obj_geometry", "pack_argb", "rect_candidates", "ctab_candidates", "render", "render_tiles_device", "save_bmp", "save_png",
    "dist", "dqn", "metrics", "probe", "sarsa", "tiles", "check", "ktime_enable", "ktime_read", "ktime_name",
    "RT_KT_RENDER_PS", "RT_KT_RENDER", "RT_KT_SARSA_RENDER", "RT_KT_SARSA_APPLY", "RT_KT_DQN_MLP",
    "RT_KT_DQN_BOUNCE", "RT_KT_DQN_CAMERA", "RT_KT_SARSA_VIEW", "RT_KT_SARSA_NEAREST", "RT_KT_PROBE", "RT_KT_BAKE", "RT_KT_COUNT",
    "RtIrrOpts", "RT_SARSA_KNN_MAX", "RT_IRR_MEAN", "RT_IRR_CONE", "RtDqnViewOpts", "RT_DQN_VIEW_IRRADIANCE",
    "intersect_cand", "CAND_TABLE", "CAND_GIVEN", "CAND_CAP_TABLE", "CAND_CAP_SHARED",
    "glyphs", "Glyphs", "glyph_colours", "glyph_mesh", "read_selected", "RtGlyphViewOpts", "RT_GLYPH_MAX",
    "RT_GLYPH_SECTORS", "RT_GLYPH_TRIS", "RT_GLYPH_RATIO", "RT_GLYPH_MAGNITUDE",
    "RT_NEE_DIRECT_ONLY", "render_nee", "render_nee_tiles_device", "nee_light_table", "nee_sample",
]
