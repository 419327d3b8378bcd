"""ctypes binding of libpfx.so (the C ABI declared in include/pfx.h).

This is the reference-side binding a maintainer would write in Rust as an ``extern "C"`` block;
here it is Python because the tests and the bench harness are.  It is a *binding only*: no pixel arithmetic
happens in this package, and it fails loudly when the HIP library is missing — there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# PFX_LIB_PATH: development override for A/B timing of two builds of the same ABI (never a fallback: the file must exist)
LIB_PATH = os.environ.get("PFX_LIB_PATH") or os.path.join(_HERE, "libpfx.so")

OK, ERR_INVALID, ERR_NO_DEVICE, ERR_HIP, ERR_OOM, ERR_UNSUPPORTED, ERR_SCRIPT = 0, -1, -2, -3, -4, -5, -6
STATUS_NAMES = {0: "PFX_OK", -1: "PFX_ERR_INVALID", -2: "PFX_ERR_NO_DEVICE", -3: "PFX_ERR_HIP", -4: "PFX_ERR_OOM",
                -5: "PFX_ERR_UNSUPPORTED", -6: "PFX_ERR_SCRIPT"}


class PfxError(RuntimeError):
    def __init__(self, status: int, message: str):
        super().__init__(f"{STATUS_NAMES.get(status, status)}: {message}")
        self.status = status


class LayerInfo(C.Structure):
    _fields_ = [("layer_idx", C.c_uint32), ("opacity", C.c_float), ("visible", C.c_uint8), ("blend_mode", C.c_uint8),
                ("kind", C.c_uint8), ("_pad", C.c_uint8), ("adj", C.c_float * 16)]


class Brush(C.Structure):
    _fields_ = [("size", C.c_float), ("hardness", C.c_float), ("flow", C.c_float), ("color", C.c_float * 4),
                ("anti_aliased", C.c_int32), ("is_eraser", C.c_int32), ("mode", C.c_int32)]


class ScriptResult(C.Structure):
    _fields_ = [("error", C.c_char * 512), ("error_line", C.c_int32), ("error_col", C.c_int32),
                ("ops_executed", C.c_uint32), ("console", C.c_char * 2048)]


class BrushDynamics(C.Structure):
    _fields_ = [("scatter", C.c_float), ("hue_jitter", C.c_float), ("brightness_jitter", C.c_float), ("stamp_counter", C.c_uint32),
                ("tip_mask", C.c_void_p), ("tip_mask_size", C.c_uint32), ("tip_rotation", C.c_float), ("tip_random_rotation", C.c_int32),
                ("tip_rotation_lo", C.c_float), ("tip_rotation_hi", C.c_float)]


class DispDab(C.Structure):
    _fields_ = [("mode", C.c_int32), ("cx", C.c_float), ("cy", C.c_float), ("delta_x", C.c_float), ("delta_y", C.c_float), ("radius", C.c_float),
                ("strength", C.c_float)]


class Preview(C.Structure):
    _fields_ = [("active_layer", C.c_uint32), ("blend_mode", C.c_uint8), ("is_eraser", C.c_uint8), ("replaces_layer", C.c_uint8), ("_pad", C.c_uint8)]


class ChainOp(C.Structure):
    _fields_ = [("kind", C.c_int32), ("op", C.c_int32), ("n_params", C.c_uint32), ("params", C.c_float * 12), ("lut", C.c_void_p)]


class CanvasOp(C.Structure):
    _fields_ = [("kind", C.c_int32), ("w", C.c_uint32), ("h", C.c_uint32), ("anchor_x", C.c_uint32), ("anchor_y", C.c_uint32)]


class Shape(C.Structure):   # pfx_shape
    _fields_ = [("cx", C.c_float), ("cy", C.c_float), ("hw", C.c_float), ("hh", C.c_float), ("rotation", C.c_float), ("outline_width", C.c_float),
                ("corner_radius", C.c_float), ("primary", C.c_uint8 * 4), ("secondary", C.c_uint8 * 4), ("kind", C.c_uint8), ("fill_mode", C.c_uint8),
                ("anti_alias", C.c_uint8), ("_pad", C.c_uint8)]


class CustomPath(C.Structure):   # pfx_custom_path
    _fields_ = [("points_xy", C.c_void_p), ("polyline_points", C.c_void_p), ("n_polylines", C.c_uint32), ("bounds", C.c_float * 4)]


class InpaintDab(C.Structure):   # pfx_inpaint_dab
    _fields_ = [("cx", C.c_float), ("cy", C.c_float), ("brush_radius", C.c_float), ("sample_radius", C.c_float), ("hardness", C.c_float)]


class Flood(C.Structure):   # pfx_flood
    _fields_ = [("seed_x", C.c_uint32), ("seed_y", C.c_uint32), ("target", C.c_uint8 * 4), ("distance_mode", C.c_uint8), ("connectivity", C.c_uint8),
                ("global_", C.c_uint8), ("_pad", C.c_uint8)]


class ColorToAlpha(C.Structure):   # pfx_color_to_alpha
    _fields_ = [("target", C.c_uint8 * 3), ("_pad", C.c_uint8), ("tolerance", C.c_float), ("softness", C.c_float), ("strength", C.c_float),
                ("spill_suppression", C.c_float), ("alpha_floor", C.c_float), ("alpha_ceiling", C.c_float), ("protect_luminance", C.c_float)]


class ColorRemoval(C.Structure):   # pfx_color_removal_req
    _fields_ = [("seed_x", C.c_uint32), ("seed_y", C.c_uint32), ("tolerance", C.c_float), ("smoothness", C.c_uint32), ("contiguous", C.c_uint8),
                ("_pad", C.c_uint8 * 3)]


class Overlay(C.Structure):   # pfx_overlay
    _fields_ = [("source_w", C.c_uint32), ("source_h", C.c_uint32), ("doc_w", C.c_uint32), ("doc_h", C.c_uint32), ("center_x", C.c_float), ("center_y", C.c_float),
                ("rotation", C.c_float), ("scale_x", C.c_float), ("scale_y", C.c_float), ("anchor_x", C.c_float), ("anchor_y", C.c_float),
                ("interpolation", C.c_int32), ("anti_aliasing", C.c_uint8), ("overwrite_transparent", C.c_uint8), ("_pad", C.c_uint8 * 2)]


class OverlayGeom(C.Structure):   # pfx_overlay_geom
    _fields_ = [("scaled_w", C.c_uint32), ("scaled_h", C.c_uint32), ("cos_r", C.c_float), ("sin_r", C.c_float), ("corners", C.c_float * 8),
                ("row_start", C.c_uint32), ("row_end", C.c_uint32), ("col_start", C.c_uint32), ("col_end", C.c_uint32),
                ("has_bounds", C.c_uint32), ("bounds", C.c_uint32 * 4), ("raster_col", C.c_int32), ("raster_row", C.c_int32),
                ("raster_w", C.c_uint32), ("raster_h", C.c_uint32)]


class TextEffects(C.Structure):   # pfx_text_fx
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("flags", C.c_uint32),
                ("outline_color", C.c_uint8 * 4), ("outline_width", C.c_float), ("outline_position", C.c_int32),
                ("shadow_color", C.c_uint8 * 4), ("shadow_offset_x", C.c_float), ("shadow_offset_y", C.c_float), ("shadow_blur_radius", C.c_float),
                ("shadow_spread", C.c_float),
                ("inner_color", C.c_uint8 * 4), ("inner_offset_x", C.c_float), ("inner_offset_y", C.c_float), ("inner_blur_radius", C.c_float),
                ("gradient_start", C.c_uint8 * 4), ("gradient_end", C.c_uint8 * 4), ("gradient_angle_degrees", C.c_float), ("gradient_scale", C.c_float),
                ("gradient_offset", C.c_float * 2), ("gradient_repeat", C.c_uint32),
                ("tex_w", C.c_uint32), ("tex_h", C.c_uint32), ("texture_scale", C.c_float), ("texture_offset", C.c_float * 2)]


class TextRegion(C.Structure):   # pfx_text_region
    _fields_ = [("x", C.c_uint32), ("y", C.c_uint32), ("w", C.c_uint32), ("h", C.c_uint32), ("pad_px", C.c_uint32), ("full_canvas", C.c_uint32)]


class TextWarp(C.Structure):   # pfx_text_warp_desc
    _fields_ = [("src_w", C.c_uint32), ("src_h", C.c_uint32), ("kind", C.c_int32), ("arc_bend", C.c_float), ("arc_hdist", C.c_float), ("arc_vdist", C.c_float),
                ("circ_radius", C.c_float), ("circ_start_angle", C.c_float), ("circ_clockwise", C.c_uint32), ("path_points", C.c_uint32),
                ("path", C.c_float * 2 * 4), ("top_points", C.c_uint32), ("bottom_points", C.c_uint32), ("top", C.c_float * 2 * 4), ("bottom", C.c_float * 2 * 4)]


class TextWarpGeom(C.Structure):   # pfx_text_warp_geom
    _fields_ = [("out_w", C.c_uint32), ("out_h", C.c_uint32), ("off_x", C.c_int32), ("off_y", C.c_int32), ("identity", C.c_uint32),
                ("min_x", C.c_float), ("min_y", C.c_float), ("max_x", C.c_float), ("max_y", C.c_float)]


class TextBlock(C.Structure):   # pfx_text_block
    _fields_ = [("warp", TextWarp), ("off_x", C.c_int32), ("off_y", C.c_int32), ("rotation", C.c_float), ("has_pivot", C.c_uint32), ("pivot", C.c_float * 2),
                ("canvas_w", C.c_uint32), ("canvas_h", C.c_uint32)]


class GradientStop(C.Structure):   # pfx_gradient_stop
    _fields_ = [("position", C.c_float), ("color", C.c_uint8 * 4)]


class Gradient(C.Structure):   # pfx_gradient
    _fields_ = [("start_x", C.c_float), ("start_y", C.c_float), ("end_x", C.c_float), ("end_y", C.c_float), ("shape", C.c_int32), ("repeat", C.c_int32),
                ("mode", C.c_int32), ("preview_scale", C.c_uint32)]


class CloneStampTool(C.Structure):   # pfx_clone_stamp_tool
    _fields_ = [("size", C.c_float), ("hardness", C.c_float), ("anti_aliased", C.c_int32), ("offset_x", C.c_float), ("offset_y", C.c_float)]


class HealRingTool(C.Structure):   # pfx_heal_ring_tool
    _fields_ = [("size", C.c_float), ("hardness", C.c_float), ("sample_radius", C.c_float)]


class LineTool(C.Structure):   # pfx_line_tool
    _fields_ = [("p", C.c_float * 8), ("size", C.c_float), ("color", C.c_uint8 * 4), ("pattern", C.c_int32), ("cap_style", C.c_int32), ("end_shape", C.c_int32),
                ("arrow_side", C.c_int32), ("anti_alias", C.c_int32)]


class HueBand(C.Structure):   # pfx_hue_band
    _fields_ = [("hue", C.c_float), ("saturation", C.c_float), ("lightness", C.c_float)]


class MatteSettings(C.Structure):   # pfx_matte_settings
    _fields_ = [("threshold", C.c_float), ("edge_feather", C.c_float), ("mask_expansion", C.c_int32), ("smooth_edges", C.c_int32), ("fill_holes", C.c_uint32)]


_lib = None


def load() -> C.CDLL:
    """Load libpfx.so or raise.  Never falls back to anything else."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                          f"or `make -C paintfe_amd/csrc` (hipcc, gfx950). There is no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    lib.pfx_last_error.restype = C.c_char_p
    lib.pfx_last_error.argtypes = [C.c_void_p]
    lib.pfx_ctx_stream.restype = C.c_void_p
    lib.pfx_ctx_stream.argtypes = [C.c_void_p]
    lib.pfx_layer_memory.restype = C.c_size_t
    lib.pfx_layer_count.restype = C.c_uint32
    lib.pfx_tolerance_threshold.restype = C.c_uint8
    lib.pfx_tolerance_threshold.argtypes = [C.c_float]
    lib.pfx_int_select_span.restype = C.c_int
    lib.pfx_int_select_span.argtypes = [C.c_uint32, C.c_uint32]
    lib.pfx_int_textfx_span.restype = C.c_int
    lib.pfx_int_textfx_span.argtypes = [C.c_float, C.c_int32]
    lib.pfx_int_textfx_disc_dev.restype = C.c_int
    lib.pfx_int_textfx_disc_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_float, C.c_int]
    lib.pfx_text_effects_dev.argtypes = [C.c_void_p, C.POINTER(TextEffects), C.c_void_p, C.c_void_p, C.c_void_p]
    lib.pfx_text_effects.argtypes = [C.c_void_p, C.POINTER(TextEffects), C.c_void_p, C.c_void_p, C.c_void_p]
    lib.pfx_text_effects_plan.argtypes = [C.POINTER(TextEffects), C.POINTER(C.c_uint32), C.POINTER(TextRegion)]
    lib.pfx_text_layer_effects_dev.argtypes = [C.c_void_p, C.POINTER(TextEffects), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(TextRegion)]
    lib.pfx_text_warp_plan.argtypes = [C.POINTER(TextWarp), C.POINTER(TextWarpGeom)]
    lib.pfx_text_warp_dev.argtypes = [C.c_void_p, C.POINTER(TextWarp), C.c_void_p, C.c_void_p]
    lib.pfx_text_warp.argtypes = [C.c_void_p, C.POINTER(TextWarp), C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(TextWarpGeom)]
    lib.pfx_text_rotate_plan.argtypes = [C.c_uint32, C.c_uint32, C.c_float, C.POINTER(C.c_float), C.POINTER(TextWarpGeom)]
    lib.pfx_text_rotate_dev.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_float, C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    lib.pfx_text_block_place_dev.argtypes = [C.c_void_p, C.POINTER(TextBlock), C.c_void_p, C.c_void_p]
    lib.pfx_gradient_build_lut.argtypes = [C.POINTER(GradientStop), C.c_uint32, C.c_void_p]
    lib.pfx_gradient_preset_stops.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.POINTER(GradientStop), C.POINTER(C.c_uint32)]
    lib.pfx_gradient_bake_eraser_lut.argtypes = [C.c_void_p, C.c_void_p]
    lib.pfx_gradient_drag_scale.restype = C.c_uint32
    lib.pfx_gradient_drag_scale.argtypes = [C.c_uint32, C.c_uint32]
    lib.pfx_gradient_render_dev.argtypes = [C.c_void_p, C.POINTER(Gradient), C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    lib.pfx_gradient_render.argtypes = [C.c_void_p, C.POINTER(Gradient), C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    lib.pfx_gradient_commit_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int]
    lib.pfx_gradient_commit.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int]
    lib.pfx_gradient_apply_dev.argtypes = [C.c_void_p, C.POINTER(Gradient), C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
    lib.pfx_perspective_crop_plan.argtypes = [C.POINTER(C.c_float), C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    lib.pfx_perspective_crop_dev.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_uint32, C.c_uint32, C.c_uint32]
    lib.pfx_perspective_crop.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32]
    _line = [C.c_float] * 4 + [C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
    lib.pfx_stroke_line_points.argtypes = _line
    lib.pfx_pencil_line_cells.argtypes = _line
    _stroke = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]   # after the context and the tool
    lib.pfx_clone_stamp_dev.argtypes = lib.pfx_clone_stamp.argtypes = [C.c_void_p, C.POINTER(CloneStampTool)] + _stroke
    lib.pfx_heal_ring_dev.argtypes = lib.pfx_heal_ring.argtypes = [C.c_void_p, C.POINTER(HealRingTool)] + _stroke
    lib.pfx_pencil_dev.argtypes = lib.pfx_pencil.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32,
                                                             C.c_void_p]
    lib.pfx_stroke_commit_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint8, C.c_int]
    lib.pfx_line_bounds.argtypes = [C.POINTER(LineTool), C.c_uint32, C.c_uint32, C.POINTER(C.c_float)]
    lib.pfx_line_plan.argtypes = [C.POINTER(LineTool), C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_float), C.POINTER(C.c_uint32)]
    lib.pfx_line_render_dev.argtypes = lib.pfx_line_render.argtypes = [C.c_void_p, C.POINTER(LineTool), C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_float),
                                                                       C.POINTER(C.c_float)]
    lib.pfx_stroke_commit_mask_dev.argtypes = lib.pfx_stroke_commit_mask.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int]
    lib.pfx_histogram.argtypes = lib.pfx_histogram_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    lib.pfx_hsl_bands.argtypes = lib.pfx_hsl_bands_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_float, C.c_float, C.c_float,
                                                                   C.POINTER(HueBand), C.c_void_p, C.c_int]
    lib.pfx_select_color_range.argtypes = lib.pfx_select_color_range_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_float, C.c_float,
                                                                                     C.c_float, C.c_float, C.c_uint8, C.c_void_p]
    lib.pfx_int_colorrange_info.restype = C.c_int
    lib.pfx_int_colorrange_info.argtypes = [C.c_int]
    _u32 = C.c_uint32
    lib.pfx_matte_tensor.argtypes = lib.pfx_matte_tensor_dev.argtypes = [C.c_void_p, C.c_void_p, _u32, _u32, _u32, C.c_void_p]
    lib.pfx_matte_score.argtypes = lib.pfx_matte_score_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_int32), C.POINTER(C.c_double)]
    lib.pfx_matte_pick_output.argtypes = [_u32, _u32, C.POINTER(C.c_double), _u32, C.POINTER(_u32)]
    lib.pfx_matte_byte_dev.argtypes = [C.c_void_p, C.c_void_p, _u32, _u32, C.c_int32, C.POINTER(MatteSettings), C.c_void_p]
    lib.pfx_matte_expand_dev.argtypes = [C.c_void_p, C.c_void_p, _u32, _u32, C.c_int32, C.c_void_p]
    lib.pfx_matte_resize_dev.argtypes = [C.c_void_p, C.c_void_p, _u32, _u32, C.c_void_p, _u32, _u32]
    lib.pfx_matte_feather_dev.argtypes = [C.c_void_p, C.c_void_p, _u32, _u32, C.c_float, C.c_void_p]
    lib.pfx_matte_apply_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, _u32, _u32, C.c_void_p]
    lib.pfx_matte_postprocess.argtypes = lib.pfx_matte_postprocess_dev.argtypes = [C.c_void_p, C.c_void_p, _u32, _u32, C.c_int32, C.c_void_p, _u32, _u32,
                                                                                   C.POINTER(MatteSettings), C.c_void_p, C.c_void_p]
    lib.pfx_int_matte_info.restype = C.c_int
    lib.pfx_int_matte_info.argtypes = [C.c_int]
    _cs = [C.c_void_p, C.POINTER(Shape), C.POINTER(CustomPath), _u32, _u32, C.c_void_p]
    lib.pfx_custom_shape_rasterize.argtypes = lib.pfx_custom_shape_rasterize_dev.argtypes = _cs
    lib.pfx_custom_shape_preview.argtypes = lib.pfx_custom_shape_preview_dev.argtypes = _cs
    lib.pfx_custom_shape_draw_dev.argtypes = [C.c_void_p, C.c_void_p, _u32, _u32, C.POINTER(Shape), C.POINTER(CustomPath), C.c_uint8, C.c_void_p]
    lib.pfx_custom_shape_icon.argtypes = lib.pfx_custom_shape_icon_dev.argtypes = [C.c_void_p, C.POINTER(CustomPath), _u32, C.c_int, C.c_void_p]
    lib.pfx_custom_shape_segments.argtypes = [C.POINTER(CustomPath), C.c_void_p, _u32, C.POINTER(_u32)]
    lib.pfx_int_customshape_info.restype = lib.pfx_int_customshape_cull.restype = C.c_int
    lib.pfx_int_customshape_info.argtypes = lib.pfx_int_customshape_cull.argtypes = [C.c_int]
    lib.pfx_int_warp_last.restype = lib.pfx_int_warp_info.restype = C.c_int
    lib.pfx_int_warp_last.argtypes = [C.c_void_p, C.c_int]
    lib.pfx_int_warp_info.argtypes = [C.c_int]
    _lib = lib
    return lib
