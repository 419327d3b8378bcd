"""paintfe_amd — MI355X-native raster pixel pipeline behind PaintFE's operator surface.

The product is ``libpfx.so`` (hand-written gfx950 HIP kernels + a C ABI, see ``include/pfx.h``); this package is
the thin host-side mirror of the reference's operator interface used by the tests and the bench harness.
Importing it does not load the library; constructing a ``GpuRenderer`` does, and fails loudly when the library
or the GPU is missing.  There is no CPU fallback anywhere in this package.
"""
from ._lib import LIB_PATH, PfxError, load  # noqa: F401
from .renderer import (ADJUST_OPS, BLEND_MODES, DENSE, FROM_FLAT, IN_PLACE, RHAI_OPS, SHAPE_FILLS, SHAPE_KINDS, GpuRenderer, Shape, inpaint_ring_offsets, png_decode,  # noqa: F401
                       overlay, overlay_geometry, script_check, select_span, shape_bounds, text_block, text_effects, text_effects_plan, text_rotate_plan, text_warp, text_warp_plan, textfx_span,
                       tolerance_threshold, GRADIENT_PRESETS, GRADIENT_SHAPES, gradient, gradient_bake_eraser_lut, gradient_drag_scale, gradient_lut, gradient_preset_stops,
                       perspective_crop_plan, clone_stamp_tool, heal_ring_tool, pencil_line_cells, stroke_line_points, line_tool, line_bounds, line_plan,
                       LINE_PATTERNS, LINE_CAPS, LINE_END_SHAPES, LINE_ARROW_SIDES, matte_settings, CustomPath, custom_shape_segments)

from .project import PfeError, Project  # noqa: F401,E402

__all__ = ["GpuRenderer", "PfxError", "load", "LIB_PATH", "BLEND_MODES", "ADJUST_OPS", "RHAI_OPS", "DENSE", "FROM_FLAT",
           "IN_PLACE", "script_check", "png_decode", "Project", "Shape", "SHAPE_KINDS", "SHAPE_FILLS", "shape_bounds", "inpaint_ring_offsets",
           "tolerance_threshold", "select_span", "overlay", "overlay_geometry", "text_effects", "text_effects_plan", "textfx_span",
           "text_warp", "text_warp_plan", "text_rotate_plan", "text_block", "GRADIENT_SHAPES", "GRADIENT_PRESETS", "gradient", "gradient_lut",
           "gradient_preset_stops", "gradient_bake_eraser_lut", "gradient_drag_scale", "perspective_crop_plan", "clone_stamp_tool",
           "heal_ring_tool", "stroke_line_points", "pencil_line_cells", "line_tool", "line_bounds", "line_plan", "LINE_PATTERNS", "LINE_CAPS",
           "LINE_END_SHAPES", "LINE_ARROW_SIDES", "matte_settings", "CustomPath", "custom_shape_segments"]
