"""Host-side mirror of the reference's operator surface, over the C ABI.

``GpuRenderer`` keeps the method names and argument meaning of ``paintfe::gpu::GpuRenderer``
(ref: src/gpu/renderer.rs:249-947) and of the pure ``_core`` functions the dialogs / Rhai host call
(ref: SURVEY.md §8b B1-B4).  Images are ``numpy.uint8`` arrays of shape (h, w, 4) — the Python spelling of the
reference's ``&[u8]`` + ``(w, h)``.  All pixel work happens in libpfx.so's HIP kernels.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Iterable, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import Brush, ChainOp, LayerInfo, PfxError, ScriptResult

DENSE, FROM_FLAT, IN_PLACE = 0, 1, 2

ADJUST_OPS = ["invert", "invert_alpha", "sepia", "brightness_contrast", "hsl", "exposure", "highlights_shadows",
              "temperature_tint", "threshold", "posterize", "color_balance", "gradient_map", "black_and_white",
              "vibrance", "lut_rgba", "desaturate"]
RHAI_OPS = ["invert", "desaturate", "sepia", "sepia_strength", "brightness_contrast", "hsl", "exposure", "levels"]
BLEND_MODES = ["normal", "multiply", "screen", "additive", "reflect", "glow", "color_burn", "color_dodge", "overlay",
               "difference", "negation", "lighten", "darken", "xor", "overwrite", "hard_light", "soft_light",
               "exclusion", "subtract", "divide", "linear_burn", "vivid_light", "linear_light", "pin_light",
               "hard_mix"]  # BlendMode::to_u8 order, ref: src/canvas/layers.rs:125-153
LAYER_RASTER, ADJ_EXPOSURE, ADJ_BRIGHTNESS_CONTRAST, ADJ_INVERT, ADJ_CHANNEL_MIXER = range(5)


def _u8(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.uint8)


def _p(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _fparams(params: Sequence[float]):
    arr = (C.c_float * max(len(params), 1))(*[float(x) for x in params])
    return arr, C.c_uint32(len(params))


NOISE_TYPES = ["uniform", "gaussian", "perlin"]                       # NoiseType
HALFTONE_SHAPES = ["circle", "square", "diamond", "line"]             # HalftoneShape
GRID_STYLES = ["lines", "checkerboard"]                               # GridStyle
OUTLINE_MODES = ["outside", "inside", "center"]                       # OutlineMode
COLOR_FILTER_MODES = ["multiply", "screen", "overlay", "soft_light"]  # ColorFilterMode
RESIZE_FILTERS = ["nearest", "bilinear", "bicubic", "lanczos3"]       # ScriptFilterType / Interpolation
SHAPE_KINDS = ["ellipse", "rectangle", "rounded_rect", "trapezoid", "parallelogram", "triangle", "right_triangle", "pentagon", "hexagon", "octagon", "cross",
               "check", "heart", "diamond", "star5", "star6", "arrow"]       # ShapeKind, shapes.rs:159-178
SHAPE_FILLS = ["outline", "filled", "both"]                                   # ShapeFillMode, shapes.rs:268-272
CANVAS_OPS = ["flip_horizontal", "flip_vertical", "rotate_90cw", "rotate_90ccw", "rotate_180", "resize_image", "resize_canvas"]  # CanvasOpRequest


def _enum(names, v):
    return C.c_int(names.index(v) if isinstance(v, str) else int(v))


def _c4(color):
    return (C.c_uint8 * 4)(*[int(v) for v in color])


def _f4(color):
    return None if color is None else (C.c_float * 4)(*[float(v) for v in color])


# The rest of the effect bank (ref: src/ops/effects/*.rs `*_core`): name -> marshaller of the reference's parameters, in the
# reference's order.  GpuRenderer grows `<name>_core(img, ..., mask=None)` and `<name>_dev(src_ptr, dst_ptr, w, h, ..., mask_ptr=0)`.
_EFFECTS = {
    "zoom_blur": lambda center_x, center_y, strength, samples, tint_color=None, tint_strength=0.0: [
        C.c_float(center_x), C.c_float(center_y), C.c_float(strength), C.c_uint32(samples), _f4(tint_color), C.c_float(tint_strength)],
    "crystallize": lambda cell_size, seed: [C.c_float(cell_size), C.c_uint32(seed)],
    "dents": lambda scale, amount, seed, octaves, roughness, pinch=False, wrap=False: [
        C.c_float(scale), C.c_float(amount), C.c_uint32(seed), C.c_uint32(octaves), C.c_float(roughness), C.c_int(int(pinch)), C.c_int(int(wrap))],
    "bulge": lambda amount, origin=(0.5, 0.5): [C.c_float(amount), C.c_float(origin[0]), C.c_float(origin[1])],
    "twist": lambda angle_deg, origin=(0.5, 0.5): [C.c_float(angle_deg), C.c_float(origin[0]), C.c_float(origin[1])],
    "add_noise": lambda amount, noise_type, monochrome, seed, scale, octaves: [
        C.c_float(amount), _enum(NOISE_TYPES, noise_type), C.c_int(int(monochrome)), C.c_uint32(seed), C.c_float(scale), C.c_uint32(octaves)],
    "reduce_noise": lambda strength, radius: [C.c_float(strength), C.c_uint32(radius)],
    "vignette": lambda amount, softness: [C.c_float(amount), C.c_float(softness)],
    "halftone": lambda dot_size, angle_deg, shape="circle": [C.c_float(dot_size), C.c_float(angle_deg), _enum(HALFTONE_SHAPES, shape)],
    "grid": lambda cell_w, cell_h, line_width, color, style="lines", opacity=1.0: [
        C.c_uint32(cell_w), C.c_uint32(cell_h), C.c_uint32(line_width), _c4(color), _enum(GRID_STYLES, style), C.c_float(opacity)],
    "canvas_border": lambda width, color: [C.c_uint32(width), _c4(color)],
    "shadow": lambda offset_x, offset_y, blur_radius, widen_radius, color, opacity: [
        C.c_int32(offset_x), C.c_int32(offset_y), C.c_float(blur_radius), C.c_int(int(widen_radius)), _c4(color), C.c_float(opacity)],
    "outline": lambda width, color, mode="outside", anti_alias=True: [
        C.c_uint32(width), _c4(color), _enum(OUTLINE_MODES, mode), C.c_int(int(anti_alias))],
    "pixel_drag": lambda seed, amount, distance, direction: [C.c_uint32(seed), C.c_float(amount), C.c_uint32(distance), C.c_float(direction)],
    "rgb_displace": lambda r_off, g_off, b_off: [C.c_int32(r_off[0]), C.c_int32(r_off[1]), C.c_int32(g_off[0]), C.c_int32(g_off[1]),
                                                 C.c_int32(b_off[0]), C.c_int32(b_off[1])],
    "ink": lambda edge_strength, threshold: [C.c_float(edge_strength), C.c_float(threshold)],
    "oil_painting": lambda radius, levels: [C.c_uint32(radius), C.c_uint32(levels)],
    "color_filter": lambda filter_color, intensity, mode="multiply": [_c4(filter_color), C.c_float(intensity), _enum(COLOR_FILTER_MODES, mode)],
    "contours": lambda scale, frequency, line_width, line_color, seed, octaves, blend: [
        C.c_float(scale), C.c_float(frequency), C.c_float(line_width), _c4(line_color), C.c_uint32(seed), C.c_uint32(octaves), C.c_float(blend)],
}


@dataclass
class Shape:
    """PlacedShape (ref: src/ops/shapes.rs:322): the fields the rasteriser reads.  `kind` / `fill` are names from SHAPE_KINDS / SHAPE_FILLS or their indices."""
    kind: object
    fill: object = "both"
    cx: float = 0.0
    cy: float = 0.0
    hw: float = 0.0
    hh: float = 0.0
    rotation: float = 0.0
    outline_width: float = 1.0
    corner_radius: float = 0.0
    primary: Tuple[int, int, int, int] = (0, 0, 0, 255)
    secondary: Tuple[int, int, int, int] = (255, 255, 255, 255)
    anti_alias: bool = True

    def to_c(self) -> "_lib.Shape":
        kind = SHAPE_KINDS.index(self.kind) if isinstance(self.kind, str) else int(self.kind)
        fill = SHAPE_FILLS.index(self.fill) if isinstance(self.fill, str) else int(self.fill)
        return _lib.Shape(self.cx, self.cy, self.hw, self.hh, self.rotation, self.outline_width, self.corner_radius, _c4(self.primary), _c4(self.secondary),
                          kind, fill, int(bool(self.anti_alias)), 0)


def shape_bounds(shape: Shape, canvas_w: int, canvas_h: int):
    """(x0, y0, bw, bh) of the shape's rasterised box (rasterize_shape, shapes.rs:1175-1207); an empty box is (0, 0, 0, 0).  Host only."""
    box = (C.c_int32 * 4)()
    st = _lib.load().pfx_shape_bounds(C.byref(shape.to_c()), C.c_uint32(canvas_w), C.c_uint32(canvas_h), box)
    if st != 0:
        raise PfxError(st, "pfx_shape_bounds: bad shape or canvas size")
    return tuple(int(v) for v in box)


class CustomPath:
    """CustomShapeRenderData (ref: src/ops/shapes.rs:13) for the custom_shape_* calls: `polylines` a list of (n, 2) float32 arrays, `bounds` =
    (min_x, min_y, max_x, max_y).  Host memory; every call flattens, checks and stages it anew."""

    def __init__(self, polylines, bounds):
        polys = [np.ascontiguousarray(p, np.float32).reshape(-1, 2) for p in polylines]
        self._points = np.ascontiguousarray(np.concatenate(polys) if polys else np.zeros((0, 2), np.float32))
        self._counts = np.array([len(p) for p in polys], np.uint32)
        self.c = _lib.CustomPath(self._points.ctypes.data if self._points.size else None, self._counts.ctypes.data if self._counts.size else None,
                                 len(polys), (C.c_float * 4)(*[float(b) for b in bounds]))


def custom_shape_segments(path: CustomPath) -> np.ndarray:
    """the (n, 4) float32 segments x1 y1 x2 y2 the kernel reads: windows(2) of every polyline, in order (pfx_custom_shape_segments).  Host only."""
    lib, n = _lib.load(), C.c_uint32(0)
    st = lib.pfx_custom_shape_segments(C.byref(path.c), None, C.c_uint32(0), C.byref(n))
    if st != 0:
        raise PfxError(st, "pfx_custom_shape_segments: bad path")
    out = np.zeros((n.value, 4), np.float32)
    if n.value and lib.pfx_custom_shape_segments(C.byref(path.c), out.ctypes.data_as(C.c_void_p), n, C.byref(n)) != 0:
        raise PfxError(-1, "pfx_custom_shape_segments: bad path")
    return out


def inpaint_ring_offsets(sample_radius: float) -> np.ndarray:
    """the instant heal brush's 32 candidate offsets as 64 f32, x and y interleaved (inpaint.rs:141-147).  Host only."""
    out = np.zeros(64, np.float32)
    fn = _lib.load().pfx_inpaint_ring_offsets
    fn.restype = None
    fn(C.c_float(sample_radius), out.ctypes.data_as(C.c_void_p))
    return out


def _dab_array(dabs):
    rows = [tuple(float(v) for v in d) for d in dabs]
    if any(len(r) != 5 for r in rows):
        raise ValueError("a dab is (cx, cy, brush_radius, sample_radius, hardness)")
    return (_lib.InpaintDab * max(len(rows), 1))(*[_lib.InpaintDab(*r) for r in rows]), len(rows)


DISTANCE_MODES = ["legacy", "perceptual"]                  # WandDistanceMode
COMBINE_MODES = ["replace", "add", "subtract", "intersect"]   # SelectionMode, as merge_magic_wand_masks reads it (fill_magic.rs:486)


def tolerance_threshold(tolerance: float) -> int:
    """tolerance_threshold_u8 (fill_magic.rs:78): the tools' 0..100 tolerance as a distance threshold"""
    return int(_lib.load().pfx_tolerance_threshold(C.c_float(tolerance)))


def select_span(r: int, k: int) -> int:
    """floor(sqrt(r^2 - k^2)), an entry of the span table the expand / contract kernels walk (-1: k > r or r above 46340); host only"""
    return int(_lib.load().pfx_int_select_span(C.c_uint32(r), C.c_uint32(k)))


def _flood(seed, target, distance_mode, connectivity, global_scope):
    mode = DISTANCE_MODES.index(distance_mode) if isinstance(distance_mode, str) else int(distance_mode)
    return _lib.Flood(int(seed[0]), int(seed[1]), _c4(target), mode, int(connectivity), int(bool(global_scope)), 0)


def _color_to_alpha(target, tolerance, softness, strength, spill_suppression, alpha_floor, alpha_ceiling, protect_luminance):
    s = _lib.ColorToAlpha()
    s.target[:] = [int(v) for v in target[:3]]
    s.tolerance, s.softness, s.strength, s.spill_suppression = tolerance, softness, strength, spill_suppression
    s.alpha_floor, s.alpha_ceiling, s.protect_luminance = alpha_floor, alpha_ceiling, protect_luminance
    return s


def _hue_bands(bands):
    """six pfx_hue_band from up to six (hue, saturation, lightness) triples"""
    b = (_lib.HueBand * 6)()
    for i, (hue, sat, light) in enumerate(bands):
        b[i] = _lib.HueBand(float(hue), float(sat), float(light))
    return b


def matte_settings(threshold: float = 0.5, edge_feather: float = 0.0, mask_expansion: int = 0, smooth_edges: bool = True, fill_holes: int = 0):
    """pfx_matte_settings (RemoveBgSettings, ref: src/ops/ai.rs:19-49; the defaults are its Default)"""
    return _lib.MatteSettings(float(threshold), float(edge_feather), int(mask_expansion), int(bool(smooth_edges)), int(fill_holes))


def _color_removal(seed, tolerance, smoothness, contiguous):
    r = _lib.ColorRemoval()
    r.seed_x, r.seed_y, r.tolerance, r.smoothness, r.contiguous = int(seed[0]), int(seed[1]), tolerance, int(smoothness), int(contiguous)
    return r


INTERPOLATIONS = ["nearest", "bilinear", "bicubic", "lanczos3"]         # PFX_RESIZE_*


def overlay(source_size, doc_size, center, rotation: float = 0.0, scale=(1.0, 1.0), anchor=(0.0, 0.0), interpolation="bilinear", anti_aliasing: bool = True,
            overwrite_transparent: bool = False) -> _lib.Overlay:
    """a pfx_overlay: PasteOverlay's transform plus the sizes, (w, h) each; the defaults are PasteOverlay::new's"""
    interp = INTERPOLATIONS.index(interpolation) if isinstance(interpolation, str) else int(interpolation)
    return _lib.Overlay(int(source_size[0]), int(source_size[1]), int(doc_size[0]), int(doc_size[1]), float(center[0]), float(center[1]), float(rotation),
                        float(scale[0]), float(scale[1]), float(anchor[0]), float(anchor[1]), interp, int(bool(anti_aliasing)), int(bool(overwrite_transparent)))


def overlay_geometry(ov: _lib.Overlay) -> _lib.OverlayGeom:
    """pfx_overlay_geometry: the scaled size, cos / sin, corners, commit box, transformed bounds and clipboard raster window of an overlay; host only"""
    g = _lib.OverlayGeom()
    st = _lib.load().pfx_overlay_geometry(C.byref(ov), C.byref(g))
    if st != _lib.OK:
        raise PfxError(st, "pfx_overlay_geometry refused the descriptor")
    return g


GRADIENT_SHAPES = ["linear", "linear_reflected", "radial", "diamond"]                        # GradientShape, PFX_GRADIENT_*
GRADIENT_MODES = ["color", "transparency"]                                                   # GradientMode
GRADIENT_PRESETS = ["primary_secondary", "black_white", "foreground_transparent", "rainbow"]  # GradientPreset, less Custom


def gradient(start, end, shape="linear", repeat: bool = False, mode="color", preview_scale: int = 1) -> _lib.Gradient:
    """a pfx_gradient: the drag's start and end in canvas coordinates, (x, y) each, and the tool's settings"""
    sh = GRADIENT_SHAPES.index(shape) if isinstance(shape, str) else int(shape)
    md = GRADIENT_MODES.index(mode) if isinstance(mode, str) else int(mode)
    return _lib.Gradient(float(start[0]), float(start[1]), float(end[0]), float(end[1]), sh, int(bool(repeat)), md, int(preview_scale))


def _stop_array(stops):
    rows = [(float(p), _c4(c)) for p, c in stops]
    return (_lib.GradientStop * max(len(rows), 1))(*[_lib.GradientStop(p, c) for p, c in rows]), len(rows)


def gradient_lut(stops) -> np.ndarray:
    """pfx_gradient_build_lut (rebuild_lut): the (256, 4) RGBA8 table of stops = [(position, (r, g, b, a)), ...]; host only"""
    arr, n = _stop_array(stops)
    lut = np.zeros((256, 4), np.uint8)
    st = _lib.load().pfx_gradient_build_lut(arr, C.c_uint32(n), _p(lut))
    if st != _lib.OK:
        raise PfxError(st, "pfx_gradient_build_lut refused the stops")
    return lut


def gradient_preset_stops(preset, primary, secondary):
    """pfx_gradient_preset_stops (apply_preset): [(position, (r, g, b, a)), ...] of one of GRADIENT_PRESETS; host only"""
    out, n = (_lib.GradientStop * 7)(), C.c_uint32(0)
    st = _lib.load().pfx_gradient_preset_stops(_enum(GRADIENT_PRESETS, preset), _c4(primary), _c4(secondary), out, C.byref(n))
    if st != _lib.OK:
        raise PfxError(st, "pfx_gradient_preset_stops: unknown preset")
    return [(float(out[i].position), tuple(int(v) for v in out[i].color)) for i in range(n.value)]


def gradient_bake_eraser_lut(lut) -> np.ndarray:
    """pfx_gradient_bake_eraser_lut: the transparency mode's table (rgb 255, alpha = luminance * alpha / 255) of a raw (256, 4) table; host only"""
    raw = _u8(lut).reshape(256, 4)
    baked = np.zeros_like(raw)
    st = _lib.load().pfx_gradient_bake_eraser_lut(_p(raw), _p(baked))
    if st != _lib.OK:
        raise PfxError(st, "pfx_gradient_bake_eraser_lut refused its arguments")
    return baked


def gradient_drag_scale(w: int, h: int) -> int:
    """pfx_gradient_drag_scale: the reference's preview scale while dragging on a w x h canvas; host only"""
    return int(_lib.load().pfx_gradient_drag_scale(C.c_uint32(w), C.c_uint32(h)))


def clone_stamp_tool(size: float, hardness: float, anti_aliased: bool = True, offset=(0.0, 0.0)) -> _lib.CloneStampTool:
    """a pfx_clone_stamp_tool: the tool's properties and clone_stamp_state.offset (source = pixel + offset)"""
    return _lib.CloneStampTool(float(size), float(hardness), int(bool(anti_aliased)), float(offset[0]), float(offset[1]))


def heal_ring_tool(size: float, hardness: float, sample_radius: float) -> _lib.HealRingTool:
    """a pfx_heal_ring_tool: the tool's properties and content_aware_state.sample_radius"""
    return _lib.HealRingTool(float(size), float(hardness), float(sample_radius))


def _line_list(fn, name, start, end, w, h, dtype):
    n = C.c_uint32(0)
    args = [C.c_float(start[0]), C.c_float(start[1]), C.c_float(end[0]), C.c_float(end[1]), C.c_uint32(w), C.c_uint32(h)]
    st = fn(*args, None, C.c_uint32(0), C.byref(n))
    out = np.empty((n.value, 2), dtype)
    if st == _lib.OK and n.value:
        st = fn(*args, _p(out), C.c_uint32(n.value), C.byref(n))
    if st != _lib.OK:
        raise PfxError(st, f"{name} refused its arguments")
    return out


def stroke_line_points(start, end, w: int, h: int) -> np.ndarray:
    """pfx_stroke_line_points: the (n, 2) f32 dab centres clone_stamp_line / heal_line step through from start to end on a w x h canvas; host only"""
    return _line_list(_lib.load().pfx_stroke_line_points, "pfx_stroke_line_points", start, end, w, h, np.float32)


def pencil_line_cells(start, end, w: int, h: int) -> np.ndarray:
    """pfx_pencil_line_cells: the (n, 2) i32 in-canvas cells of draw_pixel_line_and_get_bounds' Bresenham walk; host only"""
    return _line_list(_lib.load().pfx_pencil_line_cells, "pfx_pencil_line_cells", start, end, w, h, np.int32)


LINE_PATTERNS = ["solid", "dotted", "dashed"]     # LinePattern
LINE_CAPS = ["round", "flat"]                     # CapStyle
LINE_END_SHAPES = ["none", "arrow"]               # LineEndShape
LINE_ARROW_SIDES = ["end", "start", "both"]       # ArrowSide


def line_tool(points, size: float, color, pattern="solid", cap_style="round", end_shape="none", arrow_side="end", anti_alias: bool = True) -> _lib.LineTool:
    """a pfx_line_tool: the four control points p0..p3 in canvas pixels, properties.size, the Color32 and the line options (names or their numbers)"""
    flat = [float(v) for p in points for v in p]
    if len(flat) != 8:
        raise ValueError("points are four (x, y) pairs: p0, p1, p2, p3")
    return _lib.LineTool((C.c_float * 8)(*flat), float(size), (C.c_uint8 * 4)(*[int(c) for c in color]), _enum(LINE_PATTERNS, pattern), _enum(LINE_CAPS, cap_style),
                         _enum(LINE_END_SHAPES, end_shape), _enum(LINE_ARROW_SIDES, arrow_side), int(bool(anti_alias)))


def line_bounds(tool, w: int, h: int):
    """pfx_line_bounds: get_bezier_bounds as four f32 (min_x, min_y, max_x, max_y); host only"""
    out = (C.c_float * 4)()
    st = _lib.load().pfx_line_bounds(C.byref(tool), C.c_uint32(w), C.c_uint32(h), out)
    if st != _lib.OK:
        raise PfxError(st, "pfx_line_bounds refused its arguments")
    return np.array(out, np.float32)


def line_plan(tool, w: int, h: int):
    """pfx_line_plan: ((n, 2) f32 dot centres after the canvas test, the pattern and the cap rule but before the selection test, (k, 3, 2) f32 arrowheads in
    draw order, each tip, wing1, wing2); host only"""
    lib, n, nt, tri = _lib.load(), C.c_uint32(0), C.c_uint32(0), (C.c_float * 12)()
    st = lib.pfx_line_plan(C.byref(tool), C.c_uint32(w), C.c_uint32(h), None, C.c_uint32(0), C.byref(n), tri, C.byref(nt))
    dots = np.empty((n.value, 2), np.float32)
    if st == _lib.OK and n.value:
        st = lib.pfx_line_plan(C.byref(tool), C.c_uint32(w), C.c_uint32(h), _p(dots), C.c_uint32(n.value), C.byref(n), tri, C.byref(nt))
    if st != _lib.OK:
        raise PfxError(st, "pfx_line_plan refused its arguments")
    return dots, np.array(tri, np.float32)[:6 * nt.value].reshape(nt.value, 3, 2)


def _corners(corners):
    flat = [float(v) for c in corners for v in c]
    if len(flat) != 8:
        raise ValueError("corners are four (x, y) pairs: TL, TR, BR, BL")
    return (C.c_float * 8)(*flat)


def perspective_crop_plan(corners, w: int, h: int):
    """pfx_perspective_crop_plan: (out_w, out_h) of the crop of a w x h canvas through corners = [TL, TR, BR, BL], or None where the reference returns None; host only"""
    ow, oh = C.c_uint32(0), C.c_uint32(0)
    st = _lib.load().pfx_perspective_crop_plan(_corners(corners), C.c_uint32(w), C.c_uint32(h), C.byref(ow), C.byref(oh))
    if st != _lib.OK:
        raise PfxError(st, "pfx_perspective_crop_plan refused its arguments")
    return (ow.value, oh.value) if ow.value else None


OUTLINE_POSITIONS = ["inside", "outside", "center"]                     # OutlinePosition, PFX_TEXT_OUTLINE_*
TEXT_FX_OUTLINE, TEXT_FX_SHADOW, TEXT_FX_INNER_SHADOW, TEXT_FX_GRADIENT_FILL, TEXT_FX_TEXTURE_FILL = 1, 2, 4, 8, 16
TEXT_FX_MAX_RADIUS = 64


def text_effects(size, outline=None, shadow=None, inner_shadow=None, gradient_fill=None, texture_fill=None) -> _lib.TextEffects:
    """a pfx_text_fx for a (w, h) image: TextEffects (core.rs:299-364), each member None or a dict of the reference's field names; a missing field takes
    the member's Default.  outline: color, width, position; shadow: color, offset_x, offset_y, blur_radius, spread; inner_shadow: color, offset_x, offset_y,
    blur_radius; gradient_fill: start_color, end_color, angle_degrees, scale, offset, repeat; texture_fill: texture_width, texture_height, scale, offset (the
    decoded texture itself goes to the call)"""
    fx = _lib.TextEffects()
    fx.width, fx.height = int(size[0]), int(size[1])
    fx.outline_position = 1
    if outline is not None:
        o = dict(color=(0, 0, 0, 255), width=2.0, position="outside") | outline
        fx.flags |= TEXT_FX_OUTLINE
        fx.outline_color[:] = [int(v) for v in o["color"]]
        fx.outline_width = float(o["width"])
        fx.outline_position = OUTLINE_POSITIONS.index(o["position"]) if isinstance(o["position"], str) else int(o["position"])
    if shadow is not None:
        s = dict(color=(0, 0, 0, 180), offset_x=4.0, offset_y=4.0, blur_radius=5.0, spread=0.0) | shadow
        fx.flags |= TEXT_FX_SHADOW
        fx.shadow_color[:] = [int(v) for v in s["color"]]
        fx.shadow_offset_x, fx.shadow_offset_y = float(s["offset_x"]), float(s["offset_y"])
        fx.shadow_blur_radius, fx.shadow_spread = float(s["blur_radius"]), float(s["spread"])
    if inner_shadow is not None:
        s = dict(color=(0, 0, 0, 128), offset_x=2.0, offset_y=2.0, blur_radius=3.0) | inner_shadow
        fx.flags |= TEXT_FX_INNER_SHADOW
        fx.inner_color[:] = [int(v) for v in s["color"]]
        fx.inner_offset_x, fx.inner_offset_y, fx.inner_blur_radius = float(s["offset_x"]), float(s["offset_y"]), float(s["blur_radius"])
    if gradient_fill is not None:
        g = dict(start_color=(255, 255, 255, 255), end_color=(0, 0, 0, 255), angle_degrees=0.0, scale=200.0, offset=(0.0, 0.0), repeat=False) | gradient_fill
        fx.flags |= TEXT_FX_GRADIENT_FILL
        fx.gradient_start[:] = [int(v) for v in g["start_color"]]
        fx.gradient_end[:] = [int(v) for v in g["end_color"]]
        fx.gradient_angle_degrees, fx.gradient_scale = float(g["angle_degrees"]), float(g["scale"])
        fx.gradient_offset[:] = [float(v) for v in g["offset"]]
        fx.gradient_repeat = int(bool(g["repeat"]))
    if texture_fill is not None:
        t = dict(texture_width=0, texture_height=0, scale=1.0, offset=(0.0, 0.0)) | texture_fill
        fx.flags |= TEXT_FX_TEXTURE_FILL
        fx.tex_w, fx.tex_h, fx.texture_scale = int(t["texture_width"]), int(t["texture_height"]), float(t["scale"])
        fx.texture_offset[:] = [float(v) for v in t["offset"]]
    return fx


def text_effects_plan(fx: _lib.TextEffects, bounds) -> _lib.TextRegion:
    """pfx_text_effects_plan: the padded, clamped region of a text whose pixels with alpha > 0 span bounds = (x, y, w, h) on the fx.width x fx.height canvas, and
    whether the effects run on the whole canvas instead; host only"""
    r = _lib.TextRegion()
    b = (C.c_uint32 * 4)(*[int(v) for v in bounds])
    st = _lib.load().pfx_text_effects_plan(C.byref(fx), b, C.byref(r))
    if st != _lib.OK:
        raise PfxError(st, "pfx_text_effects_plan refused its arguments")
    return r


def textfx_span(radius: float, dy: int) -> int:
    """the half-width of row dy of dilate_mask's disc as the text styles' kernels walk it (-1: the row is skipped or the radius is refused); host only"""
    return int(_lib.load().pfx_int_textfx_span(C.c_float(radius), C.c_int32(dy)))


TEXT_WARP_KINDS = ["none", "arc", "circular", "path", "envelope"]        # TextWarp, PFX_TEXT_WARP_*


def text_warp(size, kind="none", **fields) -> _lib.TextWarp:
    """a pfx_text_warp_desc for a (w, h) block raster: TextWarp (core.rs:171-294) with the reference's field names; a missing field takes the variant's
    Default.  arc: bend, horizontal_distortion, vertical_distortion; circular: radius, start_angle, clockwise; path: control_points; envelope: top_curve,
    bottom_curve (lists of (x, y); their length travels, the first four points are used)"""
    wd = _lib.TextWarp()
    wd.src_w, wd.src_h = int(size[0]), int(size[1])
    wd.kind = TEXT_WARP_KINDS.index(kind) if isinstance(kind, str) else int(kind)
    f = dict(bend=0.5, horizontal_distortion=0.0, vertical_distortion=0.0, radius=150.0, start_angle=float(np.float32(-np.pi / 2)), clockwise=True,
             control_points=[(0.0, 0.0), (100.0, -50.0), (200.0, -50.0), (300.0, 0.0)],
             top_curve=[(0.0, -30.0), (100.0, -60.0), (200.0, -60.0), (300.0, -30.0)],
             bottom_curve=[(0.0, 30.0), (100.0, 60.0), (200.0, 60.0), (300.0, 30.0)]) | fields
    wd.arc_bend, wd.arc_hdist, wd.arc_vdist = float(f["bend"]), float(f["horizontal_distortion"]), float(f["vertical_distortion"])
    wd.circ_radius, wd.circ_start_angle, wd.circ_clockwise = float(f["radius"]), float(f["start_angle"]), int(bool(f["clockwise"]))
    for count, dst, pts in (("path_points", wd.path, f["control_points"]), ("top_points", wd.top, f["top_curve"]), ("bottom_points", wd.bottom, f["bottom_curve"])):
        setattr(wd, count, len(pts))
        for i, p in enumerate(list(pts)[:4]):
            dst[i][0], dst[i][1] = float(p[0]), float(p[1])
    return wd


def text_warp_plan(warp: _lib.TextWarp) -> _lib.TextWarpGeom:
    """pfx_text_warp_plan: the warped output's size, its offset from the source's origin and whether it is the source itself; host only"""
    g = _lib.TextWarpGeom()
    st = _lib.load().pfx_text_warp_plan(C.byref(warp), C.byref(g))
    if st != _lib.OK:
        raise PfxError(st, "pfx_text_warp_plan refused its arguments")
    return g


def _pivot(pivot):
    return None if pivot is None else (C.c_float * 2)(float(pivot[0]), float(pivot[1]))


def text_rotate_plan(w: int, h: int, angle: float, pivot=None) -> _lib.TextWarpGeom:
    """pfx_text_rotate_plan: rotate_glyph_buffer's output size and offset for a w x h buffer (pivot in buffer coordinates, None = the centre); host only"""
    g = _lib.TextWarpGeom()
    st = _lib.load().pfx_text_rotate_plan(C.c_uint32(w), C.c_uint32(h), C.c_float(angle), _pivot(pivot), C.byref(g))
    if st != _lib.OK:
        raise PfxError(st, "pfx_text_rotate_plan refused its arguments")
    return g


def text_block(warp: _lib.TextWarp, offset, canvas, rotation=0.0, pivot=None) -> _lib.TextBlock:
    """a pfx_text_block: the block raster described by `warp` at offset = (x, y) on a canvas = (w, h), rotated by `rotation` radians around pivot (canvas
    coordinates; None = the buffer's centre)"""
    b = _lib.TextBlock()
    C.memmove(C.byref(b.warp), C.byref(warp), C.sizeof(_lib.TextWarp))
    b.off_x, b.off_y, b.rotation = int(offset[0]), int(offset[1]), float(rotation)
    b.canvas_w, b.canvas_h = int(canvas[0]), int(canvas[1])
    if pivot is not None:
        b.has_pivot, b.pivot[0], b.pivot[1] = 1, float(pivot[0]), float(pivot[1])
    return b


def script_check(source: str, w: int = 64, h: int = 64):
    """Language-only evaluation of a script (no device, no image functions; ref: compile_script, scripting.rs:1489): returns
    the console lines or raises PfxError with .line / .col."""
    lib = _lib.load()
    res = ScriptResult()
    st = lib.pfx_script_check(source.encode(), C.c_uint32(w), C.c_uint32(h), C.byref(res))
    if st != _lib.OK:
        err = PfxError(st, res.error.decode(errors="replace"))
        err.line, err.col = res.error_line, res.error_col
        raise err
    return [s for s in res.console.decode(errors="replace").split("\n") if s]


def png_decode(raw: bytes) -> np.ndarray:
    """The CLI's PNG reader on a buffer (pfx_png_decode_mem; ref: load_image_sync, src/io.rs:693-723): (h, w, 4) uint8.  No device needed."""
    lib = _lib.load()
    lib.pfx_png_decode_mem.restype = C.c_int
    lib.pfx_png_free.restype = None
    out, w, h = C.POINTER(C.c_uint8)(), C.c_uint32(), C.c_uint32()
    err = C.create_string_buffer(256)
    buf = (C.c_uint8 * max(len(raw), 1)).from_buffer_copy(raw if raw else b"\0")
    st = lib.pfx_png_decode_mem(buf, C.c_size_t(len(raw)), C.byref(out), C.byref(w), C.byref(h), err, C.c_size_t(256))
    if st != _lib.OK:
        raise PfxError(st, err.value.decode(errors="replace"))
    try:
        return np.ctypeslib.as_array(out, shape=(h.value, w.value, 4)).copy()
    finally:
        lib.pfx_png_free(out)


def _install_effects(cls):
    def make(name, marshal):
        def core(self, img, *a, mask=None, out=None, **kw):
            return self._img_call(getattr(self._lib, f"pfx_{name}_core"), img, *marshal(*a, **kw), mask=mask, out=out)

        def dev(self, src_ptr, dst_ptr, w, h, *a, mask_ptr=0, **kw):
            self._check(getattr(self._lib, f"pfx_{name}_dev")(self._h, C.c_void_p(src_ptr), C.c_void_p(dst_ptr), C.c_uint32(w), C.c_uint32(h),
                                                              *marshal(*a, **kw), C.c_void_p(mask_ptr or None)))
        core.__name__, dev.__name__ = f"{name}_core", f"{name}_dev"
        core.__doc__ = dev.__doc__ = f"{name}_core of src/ops/effects/ (see include/pfx.h: pfx_{name}_core / pfx_{name}_dev)"
        setattr(cls, f"{name}_core", core)
        setattr(cls, f"{name}_dev", dev)
    for name, marshal in _EFFECTS.items():
        make(name, marshal)
    return cls


@_install_effects
class GpuRenderer:
    """One HIP device + stream (ref: GpuRenderer::try_new, src/gpu/renderer.rs:261)."""

    def __init__(self, device: int = 0):
        self._lib = _lib.load()
        h = C.c_void_p()
        st = self._lib.pfx_ctx_create(C.c_int(device), C.byref(h))
        if st != _lib.OK:
            raise PfxError(st, self._lib.pfx_last_error(None).decode())
        self._h = h
        self.available = True  # ref: renderer.rs:241

    @classmethod
    def try_new(cls, device: int = 0) -> Optional["GpuRenderer"]:
        try:
            return cls(device)
        except (PfxError, ImportError, OSError):
            return None

    def close(self):
        if getattr(self, "_h", None):
            self._lib.pfx_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ plumbing
    def _check(self, st: int):
        if st != _lib.OK:
            raise PfxError(st, self._lib.pfx_last_error(self._h).decode())

    @property
    def handle(self):
        return self._h

    @property
    def stream(self) -> int:
        return int(self._lib.pfx_ctx_stream(self._h) or 0)

    def set_stream(self, hip_stream: int):
        """hip_stream: an integer hipStream_t (0 = the device's default stream, e.g. torch's default), or None to go
        back to the context's own stream."""
        if hip_stream is None:
            self._check(self._lib.pfx_ctx_set_stream(self._h, None, C.c_int(0)))
        else:
            self._check(self._lib.pfx_ctx_set_stream(self._h, C.c_void_p(hip_stream or None), C.c_int(1)))

    def set_exact(self, exact: bool):
        self._check(self._lib.pfx_ctx_set_exact(self._h, C.c_int(int(exact))))

    def synchronize(self):
        self._check(self._lib.pfx_ctx_synchronize(self._h))

    def _img_call(self, fn, img, *args, mask=None, has_mask=True, out=None):
        src = _u8(img)
        h, w = src.shape[:2]
        dst = np.empty_like(src) if out is None else out   # out: a caller's buffer (e.g. page-locked: host_alloc)
        m = None if mask is None else _u8(mask)
        a = [self._h, _p(src), _p(dst), C.c_uint32(w), C.c_uint32(h), *args]
        if has_mask:
            a.append(_p(m))
        self._check(fn(*a))
        return dst

    # ------------------------------------------------------------------ B1: GpuRenderer filter methods
    def blur_rgba(self, data, sigma: float):
        return self._img_call(self._lib.pfx_blur_rgba, data, C.c_float(sigma), has_mask=False)

    def brightness_contrast_rgba(self, data, brightness: float, contrast: float):
        return self._img_call(self._lib.pfx_brightness_contrast_rgba, data, C.c_float(brightness), C.c_float(contrast),
                              has_mask=False)

    def hsl_rgba(self, data, hue: float, sat: float, light: float):
        return self._img_call(self._lib.pfx_hsl_rgba, data, C.c_float(hue), C.c_float(sat), C.c_float(light),
                              has_mask=False)

    def invert_rgba(self, data, out=None):
        return self._img_call(self._lib.pfx_invert_rgba, data, has_mask=False, out=out)

    def median_rgba(self, data, radius: int):
        """Returns None where the reference does (device path does not cover the radius)."""
        try:
            return self._img_call(self._lib.pfx_median_rgba, data, C.c_uint32(radius), has_mask=False)
        except PfxError as e:
            if e.status == _lib.ERR_UNSUPPORTED:
                return None
            raise

    # ------------------------------------------------------------------ B4: `_core` functions
    def gaussian_blur_core(self, img, sigma: float, mask=None):
        return self._img_call(self._lib.pfx_gaussian_blur_core, img, C.c_float(sigma), mask=mask)

    def box_blur_core(self, img, radius: float, mask=None):
        return self._img_call(self._lib.pfx_box_blur_core, img, C.c_float(radius), mask=mask)

    # GpuLiquifyPipeline source cache (liquify.rs:166-176)
    def warp_set_source(self, src):
        a = _u8(src)
        self._check(self._lib.pfx_warp_set_source(self._h, _p(a), C.c_uint32(a.shape[1]), C.c_uint32(a.shape[0])))

    def warp_invalidate_source(self):
        self._check(self._lib.pfx_warp_invalidate_source(self._h))

    def warp_displacement_cached(self, disp, w: int, h: int):
        d = np.ascontiguousarray(disp, dtype=np.float32)
        out = np.zeros((h, w, 4), np.uint8)
        self._check(self._lib.pfx_warp_displacement_cached(self._h, d.ctypes.data_as(C.c_void_p), C.c_uint32(w), C.c_uint32(h), _p(out)))
        return out

    def median_core(self, img, radius: int, mask=None):
        return self._img_call(self._lib.pfx_median_core, img, C.c_uint32(radius), mask=mask)

    def pixelate_core(self, img, block_size: int, mask=None):
        return self._img_call(self._lib.pfx_pixelate_core, img, C.c_uint32(block_size), mask=mask)

    def sharpen_core(self, img, amount: float, radius: float, mask=None, out=None):      # stylize.rs:96
        return self._img_call(self._lib.pfx_sharpen_core, img, C.c_float(amount), C.c_float(radius), mask=mask, out=out)

    def glow_core(self, img, radius: float, intensity: float, mask=None, out=None):      # stylize.rs:26
        return self._img_call(self._lib.pfx_glow_core, img, C.c_float(radius), C.c_float(intensity), mask=mask, out=out)

    def bokeh_blur_core(self, img, radius: float, mask=None, out=None):                   # blur.rs:22
        return self._img_call(self._lib.pfx_bokeh_blur_core, img, C.c_float(radius), mask=mask, out=out)

    def motion_blur_core(self, img, angle_deg: float, distance: float, mask=None, out=None):  # blur.rs:144
        return self._img_call(self._lib.pfx_motion_blur_core, img, C.c_float(angle_deg), C.c_float(distance), mask=mask, out=out)

    def adjust(self, img, op, params: Sequence[float] = (), lut=None, mask=None, sparse: int = DENSE):
        opi = ADJUST_OPS.index(op) if isinstance(op, str) else int(op)
        src = _u8(img)
        h, w = src.shape[:2]
        dst = np.empty_like(src)
        arr, n = _fparams(params)
        l = None if lut is None else _u8(lut)
        m = None if mask is None else _u8(mask)
        self._check(self._lib.pfx_adjust(self._h, _p(src), _p(dst), C.c_uint32(w), C.c_uint32(h), C.c_int(opi), arr, n,
                                         _p(l), _p(m), C.c_int(sparse)))
        return dst

    def rhai_adjust(self, img, op, params: Sequence[float] = ()):
        opi = RHAI_OPS.index(op) if isinstance(op, str) else int(op)
        px = _u8(img).copy()
        h, w = px.shape[:2]
        arr, n = _fparams(params)
        self._check(self._lib.pfx_rhai_adjust(self._h, _p(px), C.c_uint32(w), C.c_uint32(h), C.c_int(opi), arr, n))
        return px

    def auto_levels(self, img, mask=None):
        return self._img_call(self._lib.pfx_auto_levels, img, mask=mask)

    def levels(self, img, in_black, in_white, gamma, out_black, out_white, mask=None, sparse=FROM_FLAT):
        lv = self.build_levels_lut(in_black, in_white, gamma, out_black, out_white)
        luts = np.stack([lv, lv, lv, np.arange(256, dtype=np.uint8)])
        return self.adjust(img, "lut_rgba", lut=luts, mask=mask, sparse=sparse)

    def build_levels_lut(self, in_black, in_white, gamma, out_black, out_white) -> np.ndarray:
        lut = np.zeros(256, np.uint8)
        self._lib.pfx_build_levels_lut(C.c_float(in_black), C.c_float(in_white), C.c_float(gamma), C.c_float(out_black),
                                       C.c_float(out_white), _p(lut))
        return lut

    def build_curves_lut(self, points) -> np.ndarray:
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 2)
        lut = np.zeros(256, np.uint8)
        self._lib.pfx_build_curves_lut(_p(pts), C.c_uint32(len(pts)), _p(lut))
        return lut

    def tiled_roundtrip(self, img):
        return self._img_call(self._lib.pfx_tiled_roundtrip, img, has_mask=False)

    def chunk_populated(self, img):
        src = _u8(img)
        h, w = src.shape[:2]
        out = np.zeros(((h + 63) // 64, (w + 63) // 64), np.uint8)
        self._check(self._lib.pfx_chunk_populated(self._h, _p(src), C.c_uint32(w), C.c_uint32(h), _p(out)))
        return out

    # ------------------------------------------------------------------ B2: compositor
    def ensure_layer_texture(self, layer_idx: int, data, generation: int):
        src = _u8(data)
        h, w = src.shape[:2]
        self._check(self._lib.pfx_layer_upload(self._h, C.c_uint32(layer_idx), C.c_uint32(w), C.c_uint32(h), _p(src),
                                               C.c_uint64(generation)))

    def update_layer_rect(self, layer_idx: int, x: int, y: int, data):
        reg = _u8(data)
        rh, rw = reg.shape[:2]
        self._check(self._lib.pfx_layer_update_rect(self._h, C.c_uint32(layer_idx), C.c_uint32(x), C.c_uint32(y),
                                                    C.c_uint32(rw), C.c_uint32(rh), _p(reg)))

    def set_layer_mask(self, layer_idx: int, conceal):
        m = None if conceal is None else _u8(conceal)
        self._check(self._lib.pfx_layer_set_mask(self._h, C.c_uint32(layer_idx), _p(m)))

    def remove_layer(self, layer_idx: int):
        self._check(self._lib.pfx_layer_remove(self._h, C.c_uint32(layer_idx)))

    def clear_layers(self):
        self._check(self._lib.pfx_layer_clear(self._h))

    def active_texture_count(self) -> int:
        return int(self._lib.pfx_layer_count(self._h))

    def active_texture_memory(self) -> int:
        return int(self._lib.pfx_layer_memory(self._h))

    @staticmethod
    def _infos(layer_info: Iterable):
        """layer_info: tuples (layer_idx, opacity, visible, blend_mode_u8[, kind, adj]) bottom -> top."""
        items = list(layer_info)
        arr = (LayerInfo * max(len(items), 1))()
        for i, t in enumerate(items):
            arr[i].layer_idx, arr[i].opacity, arr[i].visible, arr[i].blend_mode = int(t[0]), float(t[1]), int(bool(t[2])), int(t[3])
            if len(t) > 4:
                arr[i].kind = int(t[4])
                for j, v in enumerate(t[5] if len(t) > 5 else ()):
                    arr[i].adj[j] = float(v)
        return arr, len(items)

    def composite(self, canvas_w: int, canvas_h: int, layer_info: Iterable):
        arr, n = self._infos(layer_info)
        dst = np.empty((canvas_h, canvas_w, 4), np.uint8)
        self._check(self._lib.pfx_composite(self._h, C.c_uint32(canvas_w), C.c_uint32(canvas_h), arr, C.c_uint32(n), _p(dst)))
        return dst

    def composite_preview(self, canvas_w: int, canvas_h: int, layer_info: Iterable, preview_pixels, active_layer: int, blend_mode: int = 0,
                          is_eraser: bool = False, replaces_layer: bool = False, chunk_present=None):
        """composite with the tool preview layer folded into layer_info[active_layer] (ref: canvas_state.rs:593-658)"""
        arr, n = self._infos(layer_info)
        dst = np.empty((canvas_h, canvas_w, 4), np.uint8)
        pv = _lib.Preview(active_layer, blend_mode, int(is_eraser), int(replaces_layer), 0)
        px = _u8(preview_pixels)
        cp = None if chunk_present is None else _u8(chunk_present)
        self._check(self._lib.pfx_composite_preview(self._h, C.c_uint32(canvas_w), C.c_uint32(canvas_h), arr, C.c_uint32(n), _p(px), _p(cp),
                                                    C.byref(pv), _p(dst)))
        return dst

    def composite_dirty_readback(self, canvas_w, canvas_h, layer_info, rect):
        x, y, rw, rh = rect
        arr, n = self._infos(layer_info)
        dst = np.empty((rh, rw, 4), np.uint8)
        self._check(self._lib.pfx_composite_region(self._h, C.c_uint32(canvas_w), C.c_uint32(canvas_h), arr, C.c_uint32(n),
                                                   C.c_uint32(x), C.c_uint32(y), C.c_uint32(rw), C.c_uint32(rh), _p(dst)))
        return dst

    def blend_pixels(self, base, top, mode: int, opacity: float):
        b, t = _u8(base).reshape(-1, 4), _u8(top).reshape(-1, 4)
        dst = np.empty_like(b)
        self._check(self._lib.pfx_blend_pixels(self._h, _p(b), _p(t), _p(dst), C.c_size_t(len(b)), C.c_uint8(mode),
                                               C.c_float(opacity)))
        return dst

    # ------------------------------------------------------------------ B3: warp
    def warp_displacement(self, src, disp):
        s = _u8(src)
        d = np.ascontiguousarray(disp, np.float32)
        sh, sw = s.shape[:2]
        h, w = d.shape[:2]
        dst = np.empty((h, w, 4), np.uint8)
        self._check(self._lib.pfx_warp_displacement(self._h, _p(s), C.c_uint32(sw), C.c_uint32(sh), _p(d), C.c_uint32(w),
                                                    C.c_uint32(h), _p(dst)))
        return dst

    def generate_displacement(self, deformed_points, cols, rows, w, h, original_points=None):
        d = np.ascontiguousarray(deformed_points, np.float32)
        o = None if original_points is None else np.ascontiguousarray(original_points, np.float32)
        out = np.empty((h, w, 2), np.float32)
        self._check(self._lib.pfx_mesh_displacement(self._h, _p(o), _p(d), C.c_uint32(cols), C.c_uint32(rows), C.c_uint32(w),
                                                    C.c_uint32(h), _p(out)))
        return out

    def warp_mesh_catmull_rom(self, src, original_points, deformed_points, cols, rows):
        s = _u8(src)
        h, w = s.shape[:2]
        o = np.ascontiguousarray(original_points, np.float32)
        d = np.ascontiguousarray(deformed_points, np.float32)
        dst = np.empty_like(s)
        self._check(self._lib.pfx_warp_mesh_catmull_rom(self._h, _p(s), _p(o), _p(d), C.c_uint32(cols), C.c_uint32(rows),
                                                        C.c_uint32(w), C.c_uint32(h), _p(dst)))
        return dst

    def displacement_brush(self, disp: np.ndarray, mode, cx, cy, dx, dy, radius, strength):
        assert disp.dtype == np.float32 and disp.flags.c_contiguous
        h, w = disp.shape[:2]
        self._lib.pfx_displacement_brush(_p(disp), C.c_uint32(w), C.c_uint32(h), C.c_int(mode), C.c_float(cx), C.c_float(cy),
                                         C.c_float(dx), C.c_float(dy), C.c_float(radius), C.c_float(strength))
        return disp

    # ------------------------------------------------------------------ brush
    @staticmethod
    def make_brush(size, hardness, anti_aliased, color=(0, 0, 0, 1), flow=1.0, is_eraser=False, mode=0) -> Brush:
        b = Brush()
        b.size, b.hardness, b.flow = size, hardness, flow
        for i in range(4):
            b.color[i] = color[i]
        b.anti_aliased, b.is_eraser, b.mode = int(anti_aliased), int(is_eraser), int(mode)
        return b

    @staticmethod
    def make_dynamics(scatter=0.0, hue_jitter=0.0, brightness_jitter=0.0, stamp_counter=0, tip_mask=None, tip_rotation=0.0,
                      tip_random_rotation=False, tip_rotation_range=(0.0, 360.0)):
        """pfx_brush_dynamics (ToolProperties scatter / jitter / image tip; ref: state.rs:112-128).  Returns (struct, keep-alive)."""
        d = _lib.BrushDynamics(scatter, hue_jitter, brightness_jitter, stamp_counter, None, 0, tip_rotation, int(tip_random_rotation),
                               tip_rotation_range[0], tip_rotation_range[1])
        keep = None
        if tip_mask is not None:
            keep = _u8(tip_mask)
            d.tip_mask = keep.ctypes.data
            d.tip_mask_size = keep.shape[0]
        return d, keep

    def brush_tip_rescale(self, src_mask, brush_size: float, hardness: float):        # rebuild_tip_mask, brush_render.rs:404
        src = _u8(src_mask)
        n = max(int(np.ceil(np.float32(brush_size))), 1)
        out = np.zeros((n, n), np.uint8)
        self._lib.pfx_brush_tip_rescale.restype = C.c_uint32
        got = self._lib.pfx_brush_tip_rescale(_p(src), C.c_uint32(src.shape[0]), C.c_float(brush_size), C.c_float(hardness), _p(out))
        assert got == n
        return out

    def brush_stamps(self, target, brush: Brush, points, selection=None, dyn=None):
        t = _u8(target).copy()
        h, w = t.shape[:2]
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 2)
        sel = None if selection is None else _u8(selection)
        d, keep = self.make_dynamics(**dyn) if dyn is not None else (None, None)
        self._check(self._lib.pfx_brush_stamps_ex(self._h, _p(t), C.c_uint32(w), C.c_uint32(h), C.byref(brush), C.byref(d) if d is not None else None,
                                                  _p(pts), C.c_uint32(len(pts)), _p(sel)))
        return t

    def brush_line(self, target, brush: Brush, p0, p1, selection=None, dyn=None):
        t = _u8(target).copy()
        h, w = t.shape[:2]
        sel = None if selection is None else _u8(selection)
        d, keep = self.make_dynamics(**dyn) if dyn is not None else (None, None)
        self._check(self._lib.pfx_brush_line_ex(self._h, _p(t), C.c_uint32(w), C.c_uint32(h), C.byref(brush), C.byref(d) if d is not None else None,
                                                C.c_float(p0[0]), C.c_float(p0[1]), C.c_float(p1[0]), C.c_float(p1[1]), _p(sel)))
        return t

    def brush_commit(self, layer, preview, blend_mode: int, is_eraser=False, selection=None):
        l = _u8(layer).copy()
        h, w = l.shape[:2]
        p = _u8(preview)
        sel = None if selection is None else _u8(selection)
        self._check(self._lib.pfx_brush_commit(self._h, _p(l), _p(p), C.c_uint32(w), C.c_uint32(h), C.c_uint8(blend_mode),
                                               C.c_int(int(is_eraser)), _p(sel)))
        return l

    # ------------------------------------------------------------------ shape tool (ref: src/ops/shapes.rs:1169-1305)
    shape_bounds = staticmethod(shape_bounds)

    def rasterize_shape(self, shape: Shape, canvas_w: int, canvas_h: int):
        """rasterize_shape: (buf, (x0, y0, bw, bh)) with buf the (bh, bw, 4) box buffer"""
        box = shape_bounds(shape, canvas_w, canvas_h)
        buf = np.zeros((box[3], box[2], 4), np.uint8)
        if buf.size:
            self._check(self._lib.pfx_shape_rasterize(self._h, C.byref(shape.to_c()), C.c_uint32(canvas_w), C.c_uint32(canvas_h), _p(buf)))
        return buf, box

    def shape_preview(self, shape: Shape, canvas_w: int, canvas_h: int):
        """the shape on a zeroed canvas (the tool's preview layer; tests/visual_shapes.rs rasterize_to_canvas)"""
        out = np.empty((canvas_h, canvas_w, 4), np.uint8)
        self._check(self._lib.pfx_shape_preview(self._h, C.byref(shape.to_c()), C.c_uint32(canvas_w), C.c_uint32(canvas_h), _p(out)))
        return out

    def draw_shape(self, layer, shape: Shape, blend_mode: int = 0, selection=None):
        """rasterise and commit into a copy of `layer` on the device (pfx_shape_draw_dev): shape_preview + brush_commit in one kernel"""
        l = _u8(layer)
        h, w = l.shape[:2]
        sel = None if selection is None else _u8(selection)
        d_layer = self.dev_alloc(l.nbytes)
        d_sel = self.dev_alloc(sel.nbytes) if sel is not None else 0
        try:
            self.dev_upload(d_layer, l)
            if sel is not None:
                self.dev_upload(d_sel, sel)
            self.draw_shape_dev(d_layer, w, h, shape, blend_mode, d_sel)
            return self.dev_download(d_layer, l.shape)
        finally:
            self.dev_free(d_layer)
            if d_sel:
                self.dev_free(d_sel)

    def draw_shape_dev(self, layer_ptr: int, w: int, h: int, shape: Shape, blend_mode: int = 0, selection_ptr: int = 0):
        self._check(self._lib.pfx_shape_draw_dev(self._h, C.c_void_p(layer_ptr), C.c_uint32(w), C.c_uint32(h), C.byref(shape.to_c()), C.c_uint8(blend_mode),
                                                 C.c_void_p(selection_ptr or None)))

    def shape_preview_dev(self, shape: Shape, w: int, h: int, canvas_ptr: int):
        self._check(self._lib.pfx_shape_preview_dev(self._h, C.byref(shape.to_c()), C.c_uint32(w), C.c_uint32(h), C.c_void_p(canvas_ptr)))

    def rasterize_shape_dev(self, shape: Shape, w: int, h: int, box_ptr: int):
        self._check(self._lib.pfx_shape_rasterize_dev(self._h, C.byref(shape.to_c()), C.c_uint32(w), C.c_uint32(h), C.c_void_p(box_ptr)))

    # ------------------------------------------------------------------ shape tool, custom path shapes (ref: src/ops/shapes.rs:1065-1163, :122-155)
    custom_shape_segments = staticmethod(custom_shape_segments)

    def rasterize_custom_shape(self, shape: Shape, path: CustomPath, canvas_w: int, canvas_h: int):
        """rasterize_shape with custom_shape_data: (buf, (x0, y0, bw, bh)); shape.kind only shapes the box"""
        box = shape_bounds(shape, canvas_w, canvas_h)
        buf = np.zeros((box[3], box[2], 4), np.uint8)
        if buf.size:
            self._check(self._lib.pfx_custom_shape_rasterize(self._h, C.byref(shape.to_c()), C.byref(path.c), canvas_w, canvas_h, _p(buf)))
        return buf, box

    def custom_shape_preview(self, shape: Shape, path: CustomPath, canvas_w: int, canvas_h: int):
        out = np.empty((canvas_h, canvas_w, 4), np.uint8)
        self._check(self._lib.pfx_custom_shape_preview(self._h, C.byref(shape.to_c()), C.byref(path.c), canvas_w, canvas_h, _p(out)))
        return out

    def draw_custom_shape(self, layer, shape: Shape, path: CustomPath, blend_mode: int = 0, selection=None):
        """rasterise and commit into a copy of `layer` on the device (pfx_custom_shape_draw_dev): custom_shape_preview + brush_commit in one kernel"""
        l = _u8(layer)
        h, w = l.shape[:2]
        sel = None if selection is None else _u8(selection)
        d_layer = self.dev_alloc(l.nbytes)
        d_sel = self.dev_alloc(sel.nbytes) if sel is not None else 0
        try:
            self.dev_upload(d_layer, l)
            if sel is not None:
                self.dev_upload(d_sel, sel)
            self.draw_custom_shape_dev(d_layer, w, h, shape, path, blend_mode, d_sel)
            return self.dev_download(d_layer, l.shape)
        finally:
            self.dev_free(d_layer)
            if d_sel:
                self.dev_free(d_sel)

    def draw_custom_shape_dev(self, layer_ptr: int, w: int, h: int, shape: Shape, path: CustomPath, blend_mode: int = 0, selection_ptr: int = 0):
        self._check(self._lib.pfx_custom_shape_draw_dev(self._h, C.c_void_p(layer_ptr), w, h, C.byref(shape.to_c()), C.byref(path.c), blend_mode,
                                                        C.c_void_p(selection_ptr or None)))

    def custom_shape_preview_dev(self, shape: Shape, path: CustomPath, w: int, h: int, canvas_ptr: int):
        self._check(self._lib.pfx_custom_shape_preview_dev(self._h, C.byref(shape.to_c()), C.byref(path.c), w, h, C.c_void_p(canvas_ptr)))

    def rasterize_custom_shape_dev(self, shape: Shape, path: CustomPath, w: int, h: int, box_ptr: int):
        self._check(self._lib.pfx_custom_shape_rasterize_dev(self._h, C.byref(shape.to_c()), C.byref(path.c), w, h, C.c_void_p(box_ptr)))

    def custom_shape_icon(self, path: CustomPath, size: int, dark: bool):
        """render_custom_shape_icon: (size, size, 4)"""
        out = np.empty((size, size, 4), np.uint8)
        self._check(self._lib.pfx_custom_shape_icon(self._h, C.byref(path.c), size, int(bool(dark)), _p(out)))
        return out

    def custom_shape_icon_dev(self, path: CustomPath, size: int, dark: bool, rgba_ptr: int):
        self._check(self._lib.pfx_custom_shape_icon_dev(self._h, C.byref(path.c), size, int(bool(dark)), C.c_void_p(rgba_ptr)))

    def customshape_info(self, which: int) -> int:
        """0 the segments of one batch of the custom-shape kernel, 1 the slots of its LDS segment lists, 2 whether culling is on (pfx_int_customshape_info;
        for tests and profiles)"""
        return int(self._lib.pfx_int_customshape_info(which))

    def customshape_cull(self, on: bool) -> bool:
        """switch the kernel's segment culling (process-wide; results do not depend on it); returns the previous setting.  For tests and profiles"""
        return bool(self._lib.pfx_int_customshape_cull(int(bool(on))))

    # ------------------------------------------------------------------ content-aware fill (ref: src/ops/inpaint.rs)
    inpaint_ring_offsets = staticmethod(inpaint_ring_offsets)

    def inpaint_instant(self, src, mask, out, dabs):
        """inpaint_instant_brush for every dab (cx, cy, brush_radius, sample_radius, hardness) of the list in order, on a copy of `out`"""
        s, m, o = _u8(src), _u8(mask), _u8(out).copy()
        h, w = m.shape[:2]
        arr, n = _dab_array(dabs)
        self._check(self._lib.pfx_inpaint_instant(self._h, _p(s), _p(m), _p(o), C.c_uint32(w), C.c_uint32(h), arr, C.c_uint32(n)))
        return o

    def inpaint_instant_dev(self, src_ptr: int, mask_ptr: int, out_ptr: int, w: int, h: int, dabs):
        arr, n = _dab_array(dabs)
        self._check(self._lib.pfx_inpaint_instant_dev(self._h, C.c_void_p(src_ptr), C.c_void_p(mask_ptr), C.c_void_p(out_ptr), C.c_uint32(w), C.c_uint32(h), arr,
                                                      C.c_uint32(n)))

    def inpaint_patchmatch(self, src, mask, patch_size: int = 5, iterations: int = 3):
        """fill_region_patchmatch: the filled image"""
        s, m = _u8(src), _u8(mask)
        h, w = m.shape[:2]
        dst = np.empty_like(s)
        self._check(self._lib.pfx_inpaint_patchmatch(self._h, _p(s), _p(m), _p(dst), C.c_uint32(w), C.c_uint32(h), C.c_uint32(patch_size), C.c_uint32(iterations)))
        return dst

    def inpaint_patchmatch_dev(self, src_ptr: int, mask_ptr: int, dst_ptr: int, w: int, h: int, patch_size: int = 5, iterations: int = 3):
        """dst_ptr == src_ptr fills in place"""
        self._check(self._lib.pfx_inpaint_patchmatch_dev(self._h, C.c_void_p(src_ptr), C.c_void_p(mask_ptr), C.c_void_p(dst_ptr), C.c_uint32(w), C.c_uint32(h),
                                                         C.c_uint32(patch_size), C.c_uint32(iterations)))

    # ------------------------------------------------------------------ bucket fill and magic wand (ref: tools/behavior/raster/fill_magic.rs)
    tolerance_threshold = staticmethod(tolerance_threshold)

    def flood_distance(self, img, seed, target=None, distance_mode="legacy", connectivity: int = 4, global_scope: bool = False):
        """compute_flood_distance_map / compute_global_distance_map: the (h, w) distance map from seed = (x, y); target None = the seed's pixel"""
        s = _u8(img)
        h, w = s.shape[:2]
        if target is None and 0 <= seed[0] < w and 0 <= seed[1] < h:
            target = s[seed[1], seed[0]]
        f = _flood(seed, (0, 0, 0, 0) if target is None else target, distance_mode, connectivity, global_scope)
        dist = np.empty((h, w), np.uint8)
        self._check(self._lib.pfx_flood_distance(self._h, _p(s), C.c_uint32(w), C.c_uint32(h), C.byref(f), _p(dist)))
        return dist

    def flood_distance_dev(self, src_ptr: int, w: int, h: int, seed, target, dist_ptr: int, distance_mode="legacy", connectivity: int = 4, global_scope: bool = False):
        f = _flood(seed, target, distance_mode, connectivity, global_scope)
        self._check(self._lib.pfx_flood_distance_dev(self._h, C.c_void_p(src_ptr), C.c_uint32(w), C.c_uint32(h), C.byref(f), C.c_void_p(dist_ptr)))

    def flood_bboxes_dev(self, dist_ptr: int, w: int, h: int) -> np.ndarray:
        """the 256 cumulative bounding boxes (x0, y0, x1, y1; -1s = none) of {d <= t}: a (256, 4) int32 array"""
        boxes = np.empty((256, 4), np.int32)
        self._check(self._lib.pfx_flood_bboxes_dev(self._h, C.c_void_p(dist_ptr), C.c_uint32(w), C.c_uint32(h), _p(boxes)))
        return boxes

    def wand_mask(self, dist, threshold: int, anti_aliased: bool = False, combine="replace", base=None, out=None):
        """the selection mask of a distance map; out may be `base` itself (in place)"""
        d = _u8(dist)
        h, w = d.shape[:2]
        b = None if base is None else _u8(base)
        o = np.empty((h, w), np.uint8) if out is None else out
        self._check(self._lib.pfx_wand_mask(self._h, _p(d), _p(b), C.c_uint32(w), C.c_uint32(h), C.c_uint8(threshold), C.c_uint8(int(anti_aliased)),
                                            C.c_uint8(_enum(COMBINE_MODES, combine).value), _p(o)))
        return o

    def wand_mask_dev(self, dist_ptr: int, w: int, h: int, threshold: int, out_ptr: int, anti_aliased: bool = False, combine="replace", base_ptr: int = 0):
        self._check(self._lib.pfx_wand_mask_dev(self._h, C.c_void_p(dist_ptr), C.c_void_p(base_ptr or None), C.c_uint32(w), C.c_uint32(h), C.c_uint8(threshold),
                                                C.c_uint8(int(anti_aliased)), C.c_uint8(_enum(COMBINE_MODES, combine).value), C.c_void_p(out_ptr)))

    def fill_preview(self, dist, threshold: int, fill, selection=None):
        """the fill tool's preview layer over the whole canvas, the form composite_preview takes; fill = 4 bytes"""
        d = _u8(dist)
        h, w = d.shape[:2]
        sel = None if selection is None else _u8(selection)
        out = np.empty((h, w, 4), np.uint8)
        self._check(self._lib.pfx_fill_preview(self._h, _p(d), _p(sel), C.c_uint32(w), C.c_uint32(h), C.c_uint8(threshold), _c4(fill), _p(out)))
        return out

    def fill_preview_dev(self, dist_ptr: int, w: int, h: int, threshold: int, fill, canvas_ptr: int, selection_ptr: int = 0):
        self._check(self._lib.pfx_fill_preview_dev(self._h, C.c_void_p(dist_ptr), C.c_void_p(selection_ptr or None), C.c_uint32(w), C.c_uint32(h), C.c_uint8(threshold),
                                                   _c4(fill), C.c_void_p(canvas_ptr)))

    def fill_commit_dev(self, layer_ptr: int, dist_ptr: int, w: int, h: int, threshold: int, fill, blend_mode: int = 0, selection_ptr: int = 0):
        """fill_preview + brush_commit in one kernel, in place in the layer"""
        self._check(self._lib.pfx_fill_commit_dev(self._h, C.c_void_p(layer_ptr), C.c_void_p(dist_ptr), C.c_void_p(selection_ptr or None), C.c_uint32(w), C.c_uint32(h),
                                                  C.c_uint8(threshold), _c4(fill), C.c_uint8(blend_mode)))

    def bucket_fill(self, layer, seed, tolerance: float, fill, blend_mode: int = 0, global_fill: bool = False, selection=None):
        """perform_flood_fill + commit on a copy of `layer`: target = the layer pixel at seed = (x, y), LegacyRgba, 4-connected"""
        l = _u8(layer).copy()
        h, w = l.shape[:2]
        sel = None if selection is None else _u8(selection)
        self._check(self._lib.pfx_bucket_fill(self._h, _p(l), C.c_uint32(w), C.c_uint32(h), C.c_uint32(seed[0]), C.c_uint32(seed[1]), C.c_float(tolerance), _c4(fill),
                                              C.c_uint8(blend_mode), C.c_int(int(global_fill)), _p(sel)))
        return l

    def flood_last(self, which: int) -> int:
        """the last flood_distance's 0 passes, 1 kernel launches, 2 tile edge, 3 tile visits (pfx_int_flood_last; for tests and profiles)"""
        return int(self._lib.pfx_int_flood_last(self._h, C.c_int(which)))

    # ------------------------------------------------------------------ selection masks (ref: canvas/selection.rs, canvas_state.rs:1632-1887, adjustments.rs:1448-1591)
    def _select(self, fn, size, args, combine, base, out):
        w, h = int(size[0]), int(size[1])
        b = None if base is None else _u8(base)
        o = np.empty((h, w), np.uint8) if out is None else out
        self._check(fn(self._h, _p(b), C.c_uint32(w), C.c_uint32(h), *args, C.c_uint8(_enum(COMBINE_MODES, combine).value), _p(o)))
        return o

    def _select_dev(self, fn, w, h, args, combine, base_ptr, out_ptr):
        self._check(fn(self._h, C.c_void_p(base_ptr or None), C.c_uint32(w), C.c_uint32(h), *args, C.c_uint8(_enum(COMBINE_MODES, combine).value), C.c_void_p(out_ptr)))

    def select_rect(self, size, min_x: int, min_y: int, max_x: int, max_y: int, combine="replace", base=None, out=None):
        """apply_selection_shape with a rectangle (inclusive corners) on a (w, h) canvas: the (h, w) mask; out may be `base` itself (in place)"""
        return self._select(self._lib.pfx_select_rect, size, [C.c_uint32(v) for v in (min_x, min_y, max_x, max_y)], combine, base, out)

    def select_rect_dev(self, w: int, h: int, min_x: int, min_y: int, max_x: int, max_y: int, out_ptr: int, combine="replace", base_ptr: int = 0):
        self._select_dev(self._lib.pfx_select_rect_dev, w, h, [C.c_uint32(v) for v in (min_x, min_y, max_x, max_y)], combine, base_ptr, out_ptr)

    def select_ellipse(self, size, cx: float, cy: float, rx: float, ry: float, combine="replace", base=None, out=None):
        return self._select(self._lib.pfx_select_ellipse, size, [C.c_float(v) for v in (cx, cy, rx, ry)], combine, base, out)

    def select_ellipse_dev(self, w: int, h: int, cx: float, cy: float, rx: float, ry: float, out_ptr: int, combine="replace", base_ptr: int = 0):
        self._select_dev(self._lib.pfx_select_ellipse_dev, w, h, [C.c_float(v) for v in (cx, cy, rx, ry)], combine, base_ptr, out_ptr)

    def select_lasso(self, size, points, combine="replace", base=None, out=None):
        """apply_lasso_selection: points = (n, 2) floats, the closed polygon's (x, y) vertices"""
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 2)
        return self._select(self._lib.pfx_select_lasso, size, [_p(pts), C.c_uint32(len(pts))], combine, base, out)

    def select_lasso_dev(self, w: int, h: int, points, out_ptr: int, combine="replace", base_ptr: int = 0):
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 2)   # host memory in this form too
        self._select_dev(self._lib.pfx_select_lasso_dev, w, h, [_p(pts), C.c_uint32(len(pts))], combine, base_ptr, out_ptr)

    def _selection_op(self, fn, mask, arg, out):
        m = _u8(mask)
        h, w = m.shape[:2]
        o = np.empty((h, w), np.uint8) if out is None else out
        self._check(fn(self._h, _p(m), C.c_uint32(w), C.c_uint32(h), *arg, _p(o)))
        return o

    def selection_translate(self, mask, dx: int, dy: int, out=None):
        """translate_selection: out[x, y] = mask[x - dx, y - dy] or 0; out may not be `mask`"""
        return self._selection_op(self._lib.pfx_selection_translate, mask, [C.c_int32(dx), C.c_int32(dy)], out)

    def selection_translate_dev(self, mask_ptr: int, w: int, h: int, dx: int, dy: int, out_ptr: int):
        self._check(self._lib.pfx_selection_translate_dev(self._h, C.c_void_p(mask_ptr), C.c_uint32(w), C.c_uint32(h), C.c_int32(dx), C.c_int32(dy), C.c_void_p(out_ptr)))

    def selection_feather(self, mask, radius: float, out=None):
        """feather_selection; out may be `mask` itself (in place), as for expand and contract"""
        return self._selection_op(self._lib.pfx_selection_feather, mask, [C.c_float(radius)], out)

    def selection_feather_dev(self, mask_ptr: int, w: int, h: int, radius: float, out_ptr: int):
        self._check(self._lib.pfx_selection_feather_dev(self._h, C.c_void_p(mask_ptr), C.c_uint32(w), C.c_uint32(h), C.c_float(radius), C.c_void_p(out_ptr)))

    def selection_expand(self, mask, radius: int, out=None):
        return self._selection_op(self._lib.pfx_selection_expand, mask, [C.c_int32(radius)], out)

    def selection_expand_dev(self, mask_ptr: int, w: int, h: int, radius: int, out_ptr: int):
        self._check(self._lib.pfx_selection_expand_dev(self._h, C.c_void_p(mask_ptr), C.c_uint32(w), C.c_uint32(h), C.c_int32(radius), C.c_void_p(out_ptr)))

    def selection_contract(self, mask, radius: int, out=None):
        return self._selection_op(self._lib.pfx_selection_contract, mask, [C.c_int32(radius)], out)

    def selection_contract_dev(self, mask_ptr: int, w: int, h: int, radius: int, out_ptr: int):
        self._check(self._lib.pfx_selection_contract_dev(self._h, C.c_void_p(mask_ptr), C.c_uint32(w), C.c_uint32(h), C.c_int32(radius), C.c_void_p(out_ptr)))

    def selection_bounds_dev(self, mask_ptr: int, w: int, h: int) -> np.ndarray:
        """selection_mask_bounds: the inclusive box x0, y0, x1, y1 of mask != 0 as a (4,) int32 array; four -1 = empty"""
        box = np.empty(4, np.int32)
        self._check(self._lib.pfx_selection_bounds_dev(self._h, C.c_void_p(mask_ptr), C.c_uint32(w), C.c_uint32(h), _p(box)))
        return box

    def selection_fill_dev(self, layer_ptr: int, mask_ptr: int, w: int, h: int, color):
        """fill_selected_pixels, in place in the RGBA8 layer; color = 4 bytes"""
        self._check(self._lib.pfx_selection_fill_dev(self._h, C.c_void_p(layer_ptr), C.c_void_p(mask_ptr), C.c_uint32(w), C.c_uint32(h), _c4(color)))

    def selection_delete_dev(self, layer_ptr: int, mask_ptr: int, w: int, h: int):
        self._check(self._lib.pfx_selection_delete_dev(self._h, C.c_void_p(layer_ptr), C.c_void_p(mask_ptr), C.c_uint32(w), C.c_uint32(h)))

    def select_last(self, which: int) -> int:
        """0 pixels per step of a row-walking workgroup, 1 rows of the feather's smallest band, 2 bytes per lane of the shape kernel, 3 the lasso's point cap,
        4 / 5 passes / kernel launches of the last feather, expand or contract (pfx_int_select_last; for tests and profiles)"""
        return int(self._lib.pfx_int_select_last(self._h, C.c_int(which)))

    # ------------------------------------------------------------------ removal by colour (ref: src/ops/color_removal.rs)
    def color_to_alpha(self, img, target, tolerance: float = 18.0, softness: float = 35.0, strength: float = 1.0, spill_suppression: float = 0.35,
                       alpha_floor: float = 0.0, alpha_ceiling: float = 1.0, protect_luminance: float = 0.15, mask=None, out=None):
        """color_to_alpha_core: the image with `target` = (r, g, b) keyed out; the defaults are ColorToAlphaSettings::default()'s; out may be `img` itself"""
        s = _color_to_alpha(target, tolerance, softness, strength, spill_suppression, alpha_floor, alpha_ceiling, protect_luminance)
        return self._img_call(self._lib.pfx_color_to_alpha_core, img, C.byref(s), mask=mask, out=out)

    def color_to_alpha_dev(self, src_ptr: int, dst_ptr: int, w: int, h: int, target, tolerance: float = 18.0, softness: float = 35.0, strength: float = 1.0,
                           spill_suppression: float = 0.35, alpha_floor: float = 0.0, alpha_ceiling: float = 1.0, protect_luminance: float = 0.15, mask_ptr: int = 0):
        """dst_ptr == src_ptr works in place"""
        s = _color_to_alpha(target, tolerance, softness, strength, spill_suppression, alpha_floor, alpha_ceiling, protect_luminance)
        self._check(self._lib.pfx_color_to_alpha_dev(self._h, C.c_void_p(src_ptr), C.c_void_p(dst_ptr), C.c_uint32(w), C.c_uint32(h), C.byref(s), C.c_void_p(mask_ptr or None)))

    def color_removal(self, img, seed, tolerance: float, smoothness: int = 3, contiguous: bool = True, selection=None, out=None):
        """compute_color_removal + apply_color_removal on a copy of `img`: the Color Remover clicked at seed = (x, y); out may be `img` itself"""
        r = _color_removal(seed, tolerance, smoothness, contiguous)
        return self._img_call(self._lib.pfx_color_removal, img, C.byref(r), mask=selection, out=out)

    def color_removal_dev(self, src_ptr: int, dst_ptr: int, w: int, h: int, seed, tolerance: float, smoothness: int = 3, contiguous: bool = True, selection_ptr: int = 0):
        """dst_ptr == src_ptr works in place"""
        r = _color_removal(seed, tolerance, smoothness, contiguous)
        self._check(self._lib.pfx_color_removal_dev(self._h, C.c_void_p(src_ptr), C.c_void_p(dst_ptr), C.c_uint32(w), C.c_uint32(h), C.byref(r), C.c_void_p(selection_ptr or None)))

    def colorkey_last(self, which: int) -> int:
        """the last color_removal's 0 flood passes, 1 ring launches, 2 the ring kernel's tile edge, 3 its chunk (levels per launch), 4 kernel launches
        (pfx_int_colorkey_last; for tests and profiles)"""
        return int(self._lib.pfx_int_colorkey_last(self._h, C.c_int(which)))

    # ------------------------------------------------------------------ histogram, per-band Hue/Saturation, colour range (ref: src/ops/adjustments.rs:883, :1635, :1684)
    def histogram(self, img, mask=None) -> np.ndarray:
        """compute_histogram: a (4, 256) uint32 array, rows R, G, B, luminance, over the pixels with alpha != 0 that `mask` (if any) selects"""
        s = _u8(img)
        h, w = s.shape[:2]
        m = None if mask is None else _u8(mask)
        hist = np.empty((4, 256), np.uint32)
        self._check(self._lib.pfx_histogram(self._h, _p(s), C.c_uint32(w), C.c_uint32(h), _p(m), _p(hist)))
        return hist

    def histogram_dev(self, src_ptr: int, w: int, h: int, mask_ptr: int = 0) -> np.ndarray:
        """the same of a device-resident image; waits for the device"""
        hist = np.empty((4, 256), np.uint32)
        self._check(self._lib.pfx_histogram_dev(self._h, C.c_void_p(src_ptr), C.c_uint32(w), C.c_uint32(h), C.c_void_p(mask_ptr or None), _p(hist)))
        return hist

    def hsl_bands(self, img, global_hue: float = 0.0, global_sat: float = 0.0, global_light: float = 0.0, bands=(), mask=None, sparse: int = FROM_FLAT, out=None):
        """hue_saturation_per_band_from_flat: bands = up to six (hue degrees, saturation percent, lightness percent) for Reds, Yellows, Greens, Cyans, Blues,
        Magentas (missing ones are zero); out may be `img` itself"""
        src = _u8(img)
        h, w = src.shape[:2]
        dst = np.empty_like(src) if out is None else out
        m = None if mask is None else _u8(mask)
        self._check(self._lib.pfx_hsl_bands(self._h, _p(src), _p(dst), C.c_uint32(w), C.c_uint32(h), C.c_float(global_hue), C.c_float(global_sat), C.c_float(global_light),
                                            _hue_bands(bands), _p(m), C.c_int(sparse)))
        return dst

    def hsl_bands_dev(self, src_ptr: int, dst_ptr: int, w: int, h: int, global_hue: float = 0.0, global_sat: float = 0.0, global_light: float = 0.0, bands=(),
                      mask_ptr: int = 0, sparse: int = FROM_FLAT):
        """dst_ptr == src_ptr works in place"""
        self._check(self._lib.pfx_hsl_bands_dev(self._h, C.c_void_p(src_ptr), C.c_void_p(dst_ptr), C.c_uint32(w), C.c_uint32(h), C.c_float(global_hue), C.c_float(global_sat),
                                                C.c_float(global_light), _hue_bands(bands), C.c_void_p(mask_ptr or None), C.c_int(sparse)))

    def select_color_range(self, img, hue_center: float, hue_tolerance: float, sat_min: float, fuzziness: float, combine="replace", base=None, out=None):
        """select_color_range: the (h, w) mask of the pixels within hue_tolerance degrees of hue_center (0 .. 360) whose saturation is at least sat_min, merged
        with `base` by the function's own rule (add = max, subtract = saturating, intersect = product / 255); out may be `base` itself (in place)"""
        s = _u8(img)
        h, w = s.shape[:2]
        b = None if base is None else _u8(base)
        o = np.empty((h, w), np.uint8) if out is None else out
        self._check(self._lib.pfx_select_color_range(self._h, _p(s), _p(b), C.c_uint32(w), C.c_uint32(h), C.c_float(hue_center), C.c_float(hue_tolerance),
                                                     C.c_float(sat_min), C.c_float(fuzziness), C.c_uint8(_enum(COMBINE_MODES, combine).value), _p(o)))
        return o

    def select_color_range_dev(self, src_ptr: int, w: int, h: int, hue_center: float, hue_tolerance: float, sat_min: float, fuzziness: float, out_ptr: int,
                               combine="replace", base_ptr: int = 0):
        self._check(self._lib.pfx_select_color_range_dev(self._h, C.c_void_p(src_ptr), C.c_void_p(base_ptr or None), C.c_uint32(w), C.c_uint32(h), C.c_float(hue_center),
                                                         C.c_float(hue_tolerance), C.c_float(sat_min), C.c_float(fuzziness),
                                                         C.c_uint8(_enum(COMBINE_MODES, combine).value), C.c_void_p(out_ptr)))

    def colorrange_info(self, which: int) -> int:
        """0 the most workgroups of one histogram launch, 1 a workgroup's private copies of the counters (pfx_int_colorrange_info; for tests and profiles)"""
        return int(self._lib.pfx_int_colorrange_info(C.c_int(which)))

    # ------------------------------------------------------------------ background removal around the model (ref: src/ops/ai.rs); settings: matte_settings(...)
    def matte_tensor(self, img, tensor_size: int) -> np.ndarray:
        """preprocess_image: the (3, S, S) float32 model input of an RGBA8 image — Lanczos3 to S x S, ImageNet normalisation, alpha ignored"""
        s = _u8(img)
        h, w = s.shape[:2]
        out = np.empty((3, tensor_size, tensor_size), np.float32)
        self._check(self._lib.pfx_matte_tensor(self._h, _p(s), C.c_uint32(w), C.c_uint32(h), C.c_uint32(tensor_size), _p(out)))
        return out

    def matte_tensor_dev(self, image_ptr: int, w: int, h: int, tensor_size: int, tensor_ptr: int):
        self._check(self._lib.pfx_matte_tensor_dev(self._h, C.c_void_p(image_ptr), C.c_uint32(w), C.c_uint32(h), C.c_uint32(tensor_size), C.c_void_p(tensor_ptr)))

    def _matte_score(self, fn, values, n):
        is_prob, conf = C.c_int32(-7), C.c_double(-7.0)
        self._check(fn(self._h, values, C.c_size_t(n), C.byref(is_prob), C.byref(conf)))
        return bool(is_prob.value), float(conf.value)

    def matte_score(self, values):
        """(is_probability_space, mask_confidence_score) of one output tensor of the model"""
        v = np.ascontiguousarray(values, np.float32)
        return self._matte_score(self._lib.pfx_matte_score, _p(v), v.size)

    def matte_score_dev(self, values_ptr: int, n_values: int):
        """the same of a device-resident tensor; waits for the device"""
        return self._matte_score(self._lib.pfx_matte_score_dev, C.c_void_p(values_ptr), n_values)

    def matte_byte_dev(self, values_ptr: int, prob_w: int, prob_h: int, settings, grey_ptr: int, is_probability: int = -1):
        """to_probability + the threshold / sigmoid edge; is_probability -1 detects as the reference does (and waits for the device)"""
        self._check(self._lib.pfx_matte_byte_dev(self._h, C.c_void_p(values_ptr), C.c_uint32(prob_w), C.c_uint32(prob_h), C.c_int32(is_probability), C.byref(settings),
                                                 C.c_void_p(grey_ptr)))

    def matte_expand_dev(self, grey_ptr: int, prob_w: int, prob_h: int, expansion: int, out_ptr: int):
        """apply_mask_expansion: |expansion| conditional 3 x 3 dilations (> 0) or erosions (< 0)"""
        self._check(self._lib.pfx_matte_expand_dev(self._h, C.c_void_p(grey_ptr), C.c_uint32(prob_w), C.c_uint32(prob_h), C.c_int32(expansion), C.c_void_p(out_ptr)))

    def matte_resize_dev(self, grey_ptr: int, prob_w: int, prob_h: int, matte_ptr: int, w: int, h: int):
        self._check(self._lib.pfx_matte_resize_dev(self._h, C.c_void_p(grey_ptr), C.c_uint32(prob_w), C.c_uint32(prob_h), C.c_void_p(matte_ptr), C.c_uint32(w), C.c_uint32(h)))

    def matte_feather_dev(self, grey_ptr: int, w: int, h: int, edge_feather: float, matte_ptr: int):
        self._check(self._lib.pfx_matte_feather_dev(self._h, C.c_void_p(grey_ptr), C.c_uint32(w), C.c_uint32(h), C.c_float(edge_feather), C.c_void_p(matte_ptr)))

    def matte_apply_dev(self, image_ptr: int, matte_ptr: int, w: int, h: int, result_ptr: int):
        """the image's alpha times the matte; result_ptr == image_ptr works in place"""
        self._check(self._lib.pfx_matte_apply_dev(self._h, C.c_void_p(image_ptr), C.c_void_p(matte_ptr), C.c_uint32(w), C.c_uint32(h), C.c_void_p(result_ptr)))

    def matte_postprocess_dev(self, values_ptr: int, prob_w: int, prob_h: int, image_ptr: int, w: int, h: int, settings, result_ptr: int, matte_ptr: int = 0,
                              is_probability: int = -1):
        """postprocess_mask in one call: equal to matte_byte_dev, matte_expand_dev (expansion, then the close), matte_resize_dev, matte_feather_dev and
        matte_apply_dev composed; result_ptr == image_ptr works in place; matte_ptr (optional) receives the final w x h matte"""
        self._check(self._lib.pfx_matte_postprocess_dev(self._h, C.c_void_p(values_ptr), C.c_uint32(prob_w), C.c_uint32(prob_h), C.c_int32(is_probability),
                                                        C.c_void_p(image_ptr), C.c_uint32(w), C.c_uint32(h), C.byref(settings), C.c_void_p(result_ptr),
                                                        C.c_void_p(matte_ptr or None)))

    def matte_postprocess(self, values, img, settings, is_probability: int = -1, with_matte: bool = False):
        """the same on host arrays: values (prob_h, prob_w) float32, img (h, w, 4); returns the image, or (image, matte) with with_matte"""
        v = np.ascontiguousarray(values, np.float32)
        s = _u8(img)
        h, w = s.shape[:2]
        out = np.empty_like(s)
        matte = np.empty((h, w), np.uint8) if with_matte else None
        self._check(self._lib.pfx_matte_postprocess(self._h, _p(v), C.c_uint32(v.shape[1]), C.c_uint32(v.shape[0]), C.c_int32(is_probability), _p(s), C.c_uint32(w),
                                                    C.c_uint32(h), C.byref(settings), _p(out), _p(matte)))
        return (out, matte) if with_matte else out

    def matte_info(self, which: int) -> int:
        """0 the morphology's tile edge, 1 its iterations per launch, 2 / 3 the resize's output tile columns / rows, 4 the feather's row-pass outputs per workgroup,
        5 its column-pass columns per workgroup, 6 the resize tile's source-column cap, 7 the widest span of a full-height tile, 8 the tile's rows beyond it
        (pfx_int_matte_info; for tests and profiles)"""
        return int(self._lib.pfx_int_matte_info(C.c_int(which)))

    # ---- the floating selection (pfx_overlay_*): `ov` is an `overlay(...)` descriptor ----
    def overlay_commit(self, ov, source, base, overwrite_mask=None) -> np.ndarray:
        """PasteOverlay::commit on a copy of `base` (doc_h, doc_w, 4); source is (source_h, source_w, 4), overwrite_mask (source_h, source_w) or None"""
        src, b = _u8(source), _u8(base)
        m = None if overwrite_mask is None else _u8(overwrite_mask)
        out = np.empty_like(b)
        self._check(self._lib.pfx_overlay_commit(self._h, C.byref(ov), _p(src), _p(m), _p(b), _p(out)))
        return out

    def overlay_commit_dev(self, ov, source_ptr: int, base_ptr: int, out_ptr: int, overwrite_mask_ptr: int = 0):
        """out_ptr == base_ptr is commit (only the commit box is written); any other out_ptr is render_replacement_preview (every byte written)"""
        self._check(self._lib.pfx_overlay_commit_dev(self._h, C.byref(ov), C.c_void_p(source_ptr), C.c_void_p(overwrite_mask_ptr or None), C.c_void_p(base_ptr),
                                                     C.c_void_p(out_ptr)))

    def overlay_preview_dev(self, ov, source_ptr: int, preview_ptr: int):
        """render_preview: a doc_w x doc_h RGBA8 image, every byte written, ready for composite_with_preview_dev"""
        self._check(self._lib.pfx_overlay_preview_dev(self._h, C.byref(ov), C.c_void_p(source_ptr), C.c_void_p(preview_ptr)))

    def overlay_rasterize_dev(self, ov, source_ptr: int, out_ptr: int) -> bool:
        """rasterize_for_clipboard into overlay_geometry(ov)'s raster window (raster_w x raster_h RGBA8); False = the reference's None"""
        has = C.c_int(0)
        self._check(self._lib.pfx_overlay_rasterize_dev(self._h, C.byref(ov), C.c_void_p(source_ptr), C.c_void_p(out_ptr), C.byref(has)))
        return bool(has.value)

    def overlay_extract_dev(self, layer_ptr: int, selection_ptr: int, w: int, h: int, clip_ptr: int, clip_mask_ptr: int = 0):
        """extract_to_overlay: lifts the selected pixels (selection_ptr 0: the whole layer) into clip / clip_mask, blanks them on the layer and returns the
        overlay descriptor, or None where the reference does (nothing selected / nothing on the layer; the layer is then untouched)"""
        ov = _lib.Overlay()
        self._check(self._lib.pfx_overlay_extract_dev(self._h, C.c_void_p(layer_ptr), C.c_void_p(selection_ptr or None), C.c_uint32(w), C.c_uint32(h),
                                                      C.c_void_p(clip_ptr), C.c_void_p(clip_mask_ptr or None), C.byref(ov)))
        return ov if ov.source_w else None

    # ---- the text layer's styles (pfx_text_effects*): `fx` is a `text_effects(...)` descriptor ----
    def text_effects(self, fx, text, texture=None) -> np.ndarray:
        """apply_text_effects on the rasterised text (fx.height, fx.width, 4); texture is the decoded RGBA8 (fx.tex_h, fx.tex_w, 4) of a texture fill or None"""
        t = _u8(text)
        tex = None if texture is None else _u8(texture)
        out = np.empty_like(t)
        self._check(self._lib.pfx_text_effects(self._h, C.byref(fx), _p(t), _p(tex), _p(out)))
        return out

    def text_effects_dev(self, fx, text_ptr: int, out_ptr: int, texture_ptr: int = 0):
        """apply_text_effects between two device images of fx.width x fx.height; asynchronous"""
        self._check(self._lib.pfx_text_effects_dev(self._h, C.byref(fx), C.c_void_p(text_ptr), C.c_void_p(texture_ptr or None), C.c_void_p(out_ptr)))

    def text_layer_effects_dev(self, fx, text_ptr: int, out_ptr: int, texture_ptr: int = 0):
        """TextLayerData::rasterize's effect step on a canvas-sized text image: tight bounds, the padded region or the whole canvas, the result in an otherwise
        zero canvas; returns the plan as a pfx_text_region (w == 0: no visible text); waits for the device once"""
        r = _lib.TextRegion()
        self._check(self._lib.pfx_text_layer_effects_dev(self._h, C.byref(fx), C.c_void_p(text_ptr), C.c_void_p(texture_ptr or None), C.c_void_p(out_ptr), C.byref(r)))
        return r

    # ---- the text block's warps and placement (pfx_text_warp*, pfx_text_rotate*, pfx_text_block_place_dev) ----
    def text_warp(self, warp, src):
        """apply_block_warp on the block raster (warp.src_h, warp.src_w, 4): returns the warped image and its plan (pfx_text_warp_geom)"""
        s = _u8(src)
        g = text_warp_plan(warp)
        out = np.empty((g.out_h, g.out_w, 4), np.uint8)
        self._check(self._lib.pfx_text_warp(self._h, C.byref(warp), _p(s), _p(out), C.c_size_t(out.nbytes), C.byref(g)))
        return out, g

    def text_warp_dev(self, warp, src_ptr: int, out_ptr: int):
        """apply_block_warp between two device images: the source and the out_w x out_h of text_warp_plan(warp); asynchronous"""
        self._check(self._lib.pfx_text_warp_dev(self._h, C.byref(warp), C.c_void_p(src_ptr), C.c_void_p(out_ptr)))

    def text_rotate_dev(self, w: int, h: int, angle: float, src_ptr: int, out_ptr: int, pivot=None):
        """rotate_glyph_buffer between two device images: w x h and the out_w x out_h of text_rotate_plan; asynchronous"""
        self._check(self._lib.pfx_text_rotate_dev(self._h, C.c_uint32(w), C.c_uint32(h), C.c_float(angle), _pivot(pivot), C.c_void_p(src_ptr), C.c_void_p(out_ptr)))

    def text_block_place_dev(self, block, src_ptr: int, canvas_ptr: int):
        """a block raster's way into the layer image: warp, rotate, blit into the device canvas in place; asynchronous"""
        self._check(self._lib.pfx_text_block_place_dev(self._h, C.byref(block), C.c_void_p(src_ptr), C.c_void_p(canvas_ptr)))

    def textfx_disc_dev(self, src_ptr: int, dst_ptr: int, w: int, h: int, radius: float, take_min: bool = False):
        """the text styles' disc kernel alone between two tight w x h u8 planes on the device: the maximum over dilate_mask's disc, or the erosion's minimum
        (pfx_int_textfx_disc_dev; for tests); asynchronous"""
        self._check(self._lib.pfx_int_textfx_disc_dev(self._h, C.c_void_p(src_ptr or None), C.c_void_p(dst_ptr or None), C.c_uint32(w), C.c_uint32(h),
                                                      C.c_float(radius), C.c_int(int(take_min))))

    # ---- the gradient tool and the perspective crop (pfx_gradient_*, pfx_perspective_crop*): `g` is a `gradient(...)` descriptor, `lut` a raw (256, 4) table ----
    def gradient_render(self, g, lut, w: int, h: int, selection=None, premultiplied: bool = False):
        """render_gradient_to_preview's CPU path: the (gen_h, gen_w, 4) preview of a w x h canvas, gen = ceil(dim / g.preview_scale); with premultiplied=True
        also preview_flat_buffer, as a second array"""
        table = _u8(lut).reshape(256, 4)
        sel = None if selection is None else _u8(selection)
        shape = (-(-h // max(g.preview_scale, 1)), -(-w // max(g.preview_scale, 1)), 4)
        out = np.empty(shape, np.uint8)
        pm = np.empty(shape, np.uint8) if premultiplied else None
        self._check(self._lib.pfx_gradient_render(self._h, C.byref(g), _p(table), _p(sel), C.c_uint32(w), C.c_uint32(h), _p(out), _p(pm)))
        return (out, pm) if premultiplied else out

    def gradient_render_dev(self, g, lut, w: int, h: int, preview_ptr: int, selection_ptr: int = 0, premul_ptr: int = 0):
        """the same between device buffers (selection w * h bytes; preview and premultiplied copy gen_w * gen_h RGBA8); asynchronous"""
        table = _u8(lut).reshape(256, 4)
        self._check(self._lib.pfx_gradient_render_dev(self._h, C.byref(g), _p(table), C.c_void_p(selection_ptr or None), C.c_uint32(w), C.c_uint32(h),
                                                      C.c_void_p(preview_ptr), C.c_void_p(premul_ptr or None)))

    def gradient_commit(self, layer, preview, is_eraser: bool = False) -> np.ndarray:
        """commit_gradient: the layer with the full-resolution preview committed onto it"""
        out, pv = _u8(layer).copy(), _u8(preview)
        h, w = out.shape[:2]
        self._check(self._lib.pfx_gradient_commit(self._h, _p(out), _p(pv), C.c_uint32(w), C.c_uint32(h), C.c_int(int(is_eraser))))
        return out

    def gradient_commit_dev(self, layer_ptr: int, preview_ptr: int, w: int, h: int, is_eraser: bool = False):
        """commit_gradient on a device layer in place; asynchronous"""
        self._check(self._lib.pfx_gradient_commit_dev(self._h, C.c_void_p(layer_ptr), C.c_void_p(preview_ptr), C.c_uint32(w), C.c_uint32(h), C.c_int(int(is_eraser))))

    def gradient_apply_dev(self, g, lut, layer_ptr: int, w: int, h: int, selection_ptr: int = 0):
        """the mouse release in one kernel: render at scale 1 and commit onto the device layer in place (g.mode says which commit); asynchronous"""
        table = _u8(lut).reshape(256, 4)
        self._check(self._lib.pfx_gradient_apply_dev(self._h, C.byref(g), _p(table), C.c_void_p(selection_ptr or None), C.c_void_p(layer_ptr), C.c_uint32(w), C.c_uint32(h)))

    def perspective_crop(self, corners, layer) -> np.ndarray:
        """apply_perspective_crop on one layer (h, w, 4) through corners = [TL, TR, BR, BL]; PfxError where the reference returns None"""
        src = _u8(layer)
        h, w = src.shape[:2]
        plan = perspective_crop_plan(corners, w, h) or (0, 0)
        out = np.empty((plan[1], plan[0], 4), np.uint8)
        self._check(self._lib.pfx_perspective_crop(self._h, _corners(corners), _p(src), _p(out), C.c_size_t(out.nbytes), C.c_uint32(w), C.c_uint32(h)))
        return out

    def perspective_crop_dev(self, corners, layer_ptrs, cropped_ptrs, w: int, h: int):
        """every layer of a w x h document through the same quad in one launch: device pointers in, device pointers (out_w * out_h RGBA8 of the plan) out"""
        n = len(layer_ptrs)
        ins = (C.c_void_p * max(n, 1))(*[int(p) for p in layer_ptrs])
        outs = (C.c_void_p * max(n, 1))(*[int(p) for p in cropped_ptrs])
        self._check(self._lib.pfx_perspective_crop_dev(self._h, _corners(corners), ins, outs, C.c_uint32(n), C.c_uint32(w), C.c_uint32(h)))

    # ---- clone stamp, heal brush (live stroke), pencil (pfx_clone_stamp*, pfx_heal_ring*, pfx_pencil*, pfx_stroke_commit_dev): `tool` is a clone_stamp_tool(...)
    # or heal_ring_tool(...) descriptor, `points` (n, 2) dab centres, `cells` (n, 2) integer cells; each returns the dirty box (x0, y0, x1, y1) ----
    def _dab_stroke(self, fn, tool, source, preview, points, selection):
        src, out = _u8(source), _u8(preview).copy()
        h, w = out.shape[:2]
        sel = None if selection is None else _u8(selection)
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 2)
        dirty = (C.c_uint32 * 4)()
        self._check(fn(self._h, C.byref(tool), _p(src), _p(out), _p(sel), C.c_uint32(w), C.c_uint32(h), _p(pts), C.c_uint32(len(pts)), dirty))
        return out, tuple(dirty)

    def _dab_stroke_dev(self, fn, tool, source_ptr, preview_ptr, w, h, points, selection_ptr):
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 2)
        dirty = (C.c_uint32 * 4)()
        self._check(fn(self._h, C.byref(tool), C.c_void_p(source_ptr), C.c_void_p(preview_ptr), C.c_void_p(selection_ptr or None), C.c_uint32(w), C.c_uint32(h), _p(pts),
                       C.c_uint32(len(pts)), dirty))
        return tuple(dirty)

    def clone_stamp(self, tool, source, preview, points, selection=None):
        """clone_stamp_circle for every point in order: (the preview (h, w, 4) with the dabs stamped from `source`, the dirty box)"""
        return self._dab_stroke(self._lib.pfx_clone_stamp, tool, source, preview, points, selection)

    def clone_stamp_dev(self, tool, source_ptr: int, preview_ptr: int, w: int, h: int, points, selection_ptr: int = 0):
        """the same onto a device-resident preview in place (source, preview w * h RGBA8; selection w * h bytes); asynchronous; returns the dirty box"""
        return self._dab_stroke_dev(self._lib.pfx_clone_stamp_dev, tool, source_ptr, preview_ptr, w, h, points, selection_ptr)

    def heal_ring(self, tool, source, preview, points, selection=None):
        """heal_circle for every point in order: (the preview with the ring averages of `source` written under the dabs, the dirty box)"""
        return self._dab_stroke(self._lib.pfx_heal_ring, tool, source, preview, points, selection)

    def heal_ring_dev(self, tool, source_ptr: int, preview_ptr: int, w: int, h: int, points, selection_ptr: int = 0):
        """the same onto a device-resident preview in place; asynchronous; returns the dirty box"""
        return self._dab_stroke_dev(self._lib.pfx_heal_ring_dev, tool, source_ptr, preview_ptr, w, h, points, selection_ptr)

    def pencil(self, color, preview, cells, selection=None):
        """draw_pixel_and_get_bounds for every cell: (the preview with `color` (four f32 channels) written, the dirty box of the in-canvas cells)"""
        out = _u8(preview).copy()
        h, w = out.shape[:2]
        sel = None if selection is None else _u8(selection)
        cl = np.ascontiguousarray(cells, np.int32).reshape(-1, 2)
        dirty = (C.c_uint32 * 4)()
        self._check(self._lib.pfx_pencil(self._h, _f4(color), _p(out), _p(sel), C.c_uint32(w), C.c_uint32(h), _p(cl), C.c_uint32(len(cl)), dirty))
        return out, tuple(dirty)

    def pencil_dev(self, color, preview_ptr: int, w: int, h: int, cells, selection_ptr: int = 0):
        """the same onto a device-resident preview in place; asynchronous; returns the dirty box"""
        cl = np.ascontiguousarray(cells, np.int32).reshape(-1, 2)
        dirty = (C.c_uint32 * 4)()
        self._check(self._lib.pfx_pencil_dev(self._h, _f4(color), C.c_void_p(preview_ptr), C.c_void_p(selection_ptr or None), C.c_uint32(w), C.c_uint32(h), _p(cl),
                                             C.c_uint32(len(cl)), dirty))
        return tuple(dirty)

    def stroke_commit_dev(self, layer_ptr: int, preview_ptr: int, w: int, h: int, blend_mode: int = 0, is_eraser: bool = False, selection_ptr: int = 0):
        """the release of a stroke: brush_commit on a device layer in place; asynchronous"""
        self._check(self._lib.pfx_stroke_commit_dev(self._h, C.c_void_p(layer_ptr), C.c_void_p(preview_ptr), C.c_void_p(selection_ptr or None), C.c_uint32(w),
                                                    C.c_uint32(h), C.c_uint8(blend_mode), C.c_int(int(is_eraser))))

    # ---- line / curve tool (pfx_line_render*, pfx_stroke_commit_mask*): `tool` is a line_tool(...) descriptor, `last_bounds` the four floats the previous
    # frame returned (None: first frame, the whole preview is cleared); each render returns this frame's bounds ----
    line_bounds = staticmethod(line_bounds)
    line_plan = staticmethod(line_plan)

    @staticmethod
    def _bounds4(last_bounds):
        return None if last_bounds is None else (C.c_float * 4)(*[float(v) for v in last_bounds])

    def line_render(self, tool, preview, last_bounds=None, selection=None):
        """rasterize_bezier onto a copy of the preview (h, w, 4): (the preview, the frame's bounds as four f32)"""
        out = _u8(preview).copy()
        h, w = out.shape[:2]
        sel = None if selection is None else _u8(selection)
        bounds = (C.c_float * 4)()
        self._check(self._lib.pfx_line_render(self._h, C.byref(tool), _p(out), _p(sel), C.c_uint32(w), C.c_uint32(h), self._bounds4(last_bounds), bounds))
        return out, np.array(bounds, np.float32)

    def line_render_dev(self, tool, preview_ptr: int, w: int, h: int, last_bounds=None, selection_ptr: int = 0):
        """the same onto a device-resident preview in place (w * h RGBA8; selection w * h bytes); asynchronous; returns the frame's bounds"""
        bounds = (C.c_float * 4)()
        self._check(self._lib.pfx_line_render_dev(self._h, C.byref(tool), C.c_void_p(preview_ptr), C.c_void_p(selection_ptr or None), C.c_uint32(w), C.c_uint32(h),
                                                  self._bounds4(last_bounds), bounds))
        return np.array(bounds, np.float32)

    def stroke_commit_mask(self, conceal, preview, reveal: bool = False, selection=None):
        """commit_preview_to_layer_mask: the (h, w) conceal bytes with the preview's alpha committed (reveal: the mask eraser)"""
        out, pv = _u8(conceal).copy(), _u8(preview)
        h, w = pv.shape[:2]
        sel = None if selection is None else _u8(selection)
        self._check(self._lib.pfx_stroke_commit_mask(self._h, _p(out), _p(pv), _p(sel), C.c_uint32(w), C.c_uint32(h), C.c_int(int(bool(reveal)))))
        return out

    def stroke_commit_mask_dev(self, conceal_ptr: int, preview_ptr: int, w: int, h: int, reveal: bool = False, selection_ptr: int = 0):
        """the same on device-resident conceal bytes in place; asynchronous"""
        self._check(self._lib.pfx_stroke_commit_mask_dev(self._h, C.c_void_p(conceal_ptr), C.c_void_p(preview_ptr), C.c_void_p(selection_ptr or None), C.c_uint32(w),
                                                         C.c_uint32(h), C.c_int(int(bool(reveal)))))

    # ------------------------------------------------------------------ script front-end
    def resize_image(self, img, new_w: int, new_h: int, filter="bilinear"):   # transform.rs:347 (imageops::resize)
        src = _u8(img)
        h, w = src.shape[:2]
        dst = np.empty((new_h, new_w, 4), np.uint8)
        self._check(self._lib.pfx_resize_image(self._h, _p(src), C.c_uint32(w), C.c_uint32(h), _p(dst), C.c_uint32(new_w), C.c_uint32(new_h),
                                               _enum(RESIZE_FILTERS, filter)))
        return dst

    def affine_transform(self, img, canvas_w: int, canvas_h: int, rotation_z=0.0, rotation_x=0.0, rotation_y=0.0, scale=1.0, offset=(0.0, 0.0),
                         interpolation="bilinear"):                            # transform.rs:826 apply_affine
        src = _u8(img)
        h, w = src.shape[:2]
        dst = np.empty((canvas_h, canvas_w, 4), np.uint8)
        self._check(self._lib.pfx_affine_transform(self._h, _p(src), C.c_uint32(w), C.c_uint32(h), _p(dst), C.c_uint32(canvas_w), C.c_uint32(canvas_h),
                                                   C.c_float(rotation_z), C.c_float(rotation_x), C.c_float(rotation_y), C.c_float(scale),
                                                   C.c_float(offset[0]), C.c_float(offset[1]), _enum(RESIZE_FILTERS, interpolation)))
        return dst

    def affine_transform_dev(self, src_ptr: int, w: int, h: int, dst_ptr: int, canvas_w: int, canvas_h: int, rotation_z=0.0, rotation_x=0.0, rotation_y=0.0,
                             scale=1.0, offset=(0.0, 0.0), interpolation="bilinear"):
        self._check(self._lib.pfx_affine_transform_dev(self._h, C.c_void_p(src_ptr), C.c_uint32(w), C.c_uint32(h), C.c_void_p(dst_ptr), C.c_uint32(canvas_w),
                                                       C.c_uint32(canvas_h), C.c_float(rotation_z), C.c_float(rotation_x), C.c_float(rotation_y), C.c_float(scale),
                                                       C.c_float(offset[0]), C.c_float(offset[1]), _enum(RESIZE_FILTERS, interpolation)))

    def flip_rotate(self, img, op):                                            # transform.rs flip_canvas_* / rotate_canvas_*
        src = _u8(img)
        h, w = src.shape[:2]
        opi = _enum(CANVAS_OPS, op)
        dst = np.empty((w, h, 4) if opi.value in (2, 3) else (h, w, 4), np.uint8)
        self._check(self._lib.pfx_flip_rotate(self._h, _p(src), C.c_uint32(w), C.c_uint32(h), _p(dst), opi))
        return dst

    def resize_canvas(self, img, new_w: int, new_h: int, anchor=(0, 0), fill=(0, 0, 0, 0)):   # transform.rs:382
        src = _u8(img)
        h, w = src.shape[:2]
        dst = np.empty((new_h, new_w, 4), np.uint8)
        self._check(self._lib.pfx_resize_canvas(self._h, _p(src), C.c_uint32(w), C.c_uint32(h), _p(dst), C.c_uint32(new_w), C.c_uint32(new_h),
                                                C.c_uint32(anchor[0]), C.c_uint32(anchor[1]), _c4(fill)))
        return dst

    def displacement_brushes_dev(self, disp_ptr: int, w: int, h: int, dabs):
        """DisplacementField::apply_* on a device-resident w*h*2 f32 field; dabs = [(mode, cx, cy, delta_x, delta_y, radius, strength), ...]"""
        arr = (_lib.DispDab * max(len(dabs), 1))(*[_lib.DispDab(int(d[0]), *[float(v) for v in d[1:]]) for d in dabs])
        self._check(self._lib.pfx_displacement_brushes_dev(self._h, C.c_void_p(disp_ptr), C.c_uint32(w), C.c_uint32(h), arr, C.c_uint32(len(dabs))))

    def brush_stamps_dev(self, target_ptr: int, w: int, h: int, brush: Brush, points, selection_ptr: int = 0, dyn=None):
        """pfx_brush_stamps_ex_dev: the stamp loop into a device-resident w*h RGBA8 target (the interactive path: the preview layer stays on the GPU)"""
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 2)
        d, keep = self.make_dynamics(**dyn) if dyn is not None else (None, None)
        self._check(self._lib.pfx_brush_stamps_ex_dev(self._h, C.c_void_p(target_ptr), C.c_uint32(w), C.c_uint32(h), C.byref(brush),
                                                      C.byref(d) if d is not None else None, _p(pts), C.c_uint32(len(pts)), C.c_void_p(selection_ptr or None)))

    def resize_image_dev(self, src_ptr, w, h, dst_ptr, new_w, new_h, filter="bilinear"):
        self._check(self._lib.pfx_resize_image_dev(self._h, C.c_void_p(src_ptr), C.c_uint32(w), C.c_uint32(h), C.c_void_p(dst_ptr), C.c_uint32(new_w),
                                                   C.c_uint32(new_h), _enum(RESIZE_FILTERS, filter)))

    def execute_script_sync(self, source: str, pixels, mask=None, with_ops: bool = False):
        """execute_script_sync (ref: src/ops/scripting.rs:1733): returns (result_pixels, console_output) — the result may have
        another size than the input (rotate_canvas_90*, resize_canvas) — plus the CanvasOpRequest list with with_ops=True, as
        (kind, w, h, anchor_x, anchor_y) tuples."""
        px = _u8(pixels)
        h, w = px.shape[:2]
        m = None if mask is None else _u8(mask)
        res = ScriptResult()
        out = C.c_void_p()
        st = self._lib.pfx_script_execute(self._h, source.encode(), _p(px), C.c_uint32(w), C.c_uint32(h), _p(m), C.byref(out), C.byref(res))
        if st != _lib.OK:
            msg = res.error.decode(errors="replace") or self._lib.pfx_last_error(self._h).decode()
            err = PfxError(st, msg)
            err.line, err.col = res.error_line, res.error_col
            raise err
        try:
            ow, oh = C.c_uint32(), C.c_uint32()
            self._lib.pfx_script_output_pixels.restype = C.POINTER(C.c_uint8)
            self._lib.pfx_script_output_console_line.restype = C.c_char_p
            p = self._lib.pfx_script_output_pixels(out, C.byref(ow), C.byref(oh))
            result = np.ctypeslib.as_array(p, shape=(oh.value, ow.value, 4)).copy()
            console = [self._lib.pfx_script_output_console_line(out, C.c_uint32(k)).decode(errors="replace")
                       for k in range(self._lib.pfx_script_output_console_lines(out))]
            n_ops = self._lib.pfx_script_output_canvas_ops(out, None, C.c_uint32(0))
            ops_arr = (_lib.CanvasOp * max(n_ops, 1))()
            self._lib.pfx_script_output_canvas_ops(out, ops_arr, C.c_uint32(n_ops))
            ops = [(o.kind, o.w, o.h, o.anchor_x, o.anchor_y) for o in ops_arr[:n_ops]]
        finally:
            self._lib.pfx_script_output_free(out)
        return (result, console, ops) if with_ops else (result, console)

    def script_check(self, source: str, w: int = 64, h: int = 64):
        return script_check(source, w, h)

    # ------------------------------------------------------------------ device tier (raw device pointers as ints)
    def host_alloc(self, shape, dtype=np.uint8) -> np.ndarray:
        """a numpy array on page-locked host memory (pfx_host_alloc): host-buffer calls on it move at the link's rate; release with host_free(array)"""
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = C.c_void_p()
        self._check(self._lib.pfx_host_alloc(self._h, C.c_size_t(n), C.byref(p)))
        buf = (C.c_uint8 * n).from_address(p.value)
        arr = np.frombuffer(buf, dtype=dtype).reshape(shape)
        self._pinned = getattr(self, "_pinned", {})
        self._pinned[arr.ctypes.data] = p.value
        return arr

    def host_free(self, arr: np.ndarray):
        p = getattr(self, "_pinned", {}).pop(arr.ctypes.data, None)
        if p is not None:
            self._check(self._lib.pfx_host_free(self._h, C.c_void_p(p)))

    def dev_alloc(self, nbytes: int) -> int:
        p = C.c_void_p()
        self._check(self._lib.pfx_dev_alloc(self._h, C.c_size_t(nbytes), C.byref(p)))
        return int(p.value)

    def dev_free(self, ptr: int):
        self._check(self._lib.pfx_dev_free(self._h, C.c_void_p(ptr)))

    def dev_upload(self, ptr: int, host: np.ndarray):
        a = np.ascontiguousarray(host)
        self._check(self._lib.pfx_dev_upload(self._h, C.c_void_p(ptr), _p(a), C.c_size_t(a.nbytes)))

    def dev_download(self, ptr: int, shape, dtype=np.uint8) -> np.ndarray:
        out = np.empty(shape, dtype)
        self._check(self._lib.pfx_dev_download(self._h, _p(out), C.c_void_p(ptr), C.c_size_t(out.nbytes)))
        return out

    def flatten_dev(self, layer_ptrs: Sequence[int], layer_info: Iterable, w: int, h: int, dst_ptr: int, mask_ptrs=None):
        arr, n = self._infos(layer_info)
        lp = (C.c_void_p * max(n, 1))(*[C.c_void_p(p) for p in layer_ptrs])
        mp = None
        if mask_ptrs is not None:
            mp = (C.c_void_p * max(n, 1))(*[C.c_void_p(p or 0) for p in mask_ptrs])
        self._check(self._lib.pfx_flatten_dev(self._h, lp, mp, arr, C.c_uint32(n), C.c_uint32(w), C.c_uint32(h),
                                              C.c_void_p(dst_ptr)))

    def flatten_preview_dev(self, layer_ptrs: Sequence[int], layer_info: Iterable, w: int, h: int, dst_ptr: int, preview_ptr: int, active_layer: int,
                            blend_mode: int = 0, is_eraser: bool = False, replaces_layer: bool = False, chunk_present_ptr: int = 0, mask_ptrs=None):
        """flatten_dev with the tool preview (a w x h RGBA image on the device) folded into layer_info[active_layer]; chunk_present_ptr: one byte per
        64 x 64 chunk on the device, 0 = derive it from the preview's alpha (pfx_flatten_preview_dev; ref: canvas_state.rs:541-548, 593-658)"""
        arr, n = self._infos(layer_info)
        lp = (C.c_void_p * max(n, 1))(*[C.c_void_p(p) for p in layer_ptrs])
        mp = None
        if mask_ptrs is not None:
            mp = (C.c_void_p * max(n, 1))(*[C.c_void_p(p or 0) for p in mask_ptrs])
        pv = _lib.Preview(active_layer, blend_mode, int(is_eraser), int(replaces_layer), 0)
        self._check(self._lib.pfx_flatten_preview_dev(self._h, lp, mp, arr, C.c_uint32(n), C.c_uint32(w), C.c_uint32(h), C.c_void_p(preview_ptr or None),
                                                      C.c_void_p(chunk_present_ptr or None), C.byref(pv), C.c_void_p(dst_ptr)))

    def gaussian_blur_dev(self, src_ptr: int, dst_ptr: int, w: int, h: int, sigma: float, tmp_ptr: int = 0, first_row: int = 0):
        """first_row: index of the buffer's row 0 in the whole image when the buffer is a band of it (pfx_gaussian_blur_band_dev)"""
        self._check(self._lib.pfx_gaussian_blur_band_dev(self._h, C.c_void_p(src_ptr), C.c_void_p(dst_ptr), C.c_uint32(w),
                                                         C.c_uint32(h), C.c_float(sigma), C.c_void_p(tmp_ptr or None), C.c_uint32(first_row)))

    def pixelate_dev(self, src_ptr, dst_ptr, w, h, block_size, mask_ptr=0):
        self._check(self._lib.pfx_pixelate_dev(self._h, C.c_void_p(src_ptr), C.c_void_p(dst_ptr), C.c_uint32(w), C.c_uint32(h), C.c_uint32(block_size),
                                               C.c_void_p(mask_ptr or None)))

    def tiled_roundtrip_dev(self, src_ptr, dst_ptr, w, h):
        """TiledImage::from_rgba_image -> to_rgba_image on device buffers (tiled_image.rs:50-104, 271-293): chunks whose alpha is all zero are dropped"""
        self._check(self._lib.pfx_tiled_roundtrip_dev(self._h, C.c_void_p(src_ptr), C.c_void_p(dst_ptr), C.c_uint32(w), C.c_uint32(h)))

    def adjust_dev(self, src_ptr, dst_ptr, w, h, op, params=(), lut=None, mask_ptr=0, sparse=DENSE):
        opi = ADJUST_OPS.index(op) if isinstance(op, str) else int(op)
        arr, n = _fparams(params)
        l = None if lut is None else _u8(lut)
        self._check(self._lib.pfx_adjust_dev(self._h, C.c_void_p(src_ptr), C.c_void_p(dst_ptr), C.c_uint32(w), C.c_uint32(h),
                                             C.c_int(opi), arr, n, _p(l), C.c_void_p(mask_ptr or None), C.c_int(sparse)))

    def chain_dev(self, src_ptr, dst_ptr, w, h, ops):
        """pfx_chain_dev: ops = [("gaussian", sigma) | ("box", radius) | ("adjust", name, params[, lut]) | ("rhai", name, params)], applied in order with as few
        passes over memory as the kernels allow; equals the single-op calls one after the other, bit for bit"""
        arr = (ChainOp * max(len(ops), 1))()
        keep = []
        for k, o in enumerate(ops):
            kind = o[0]
            if kind in ("gaussian", "box"):
                arr[k].kind = 2 if kind == "gaussian" else 3
                arr[k].n_params = 1
                arr[k].params[0] = float(o[1])
            else:
                names = ADJUST_OPS if kind == "adjust" else RHAI_OPS
                arr[k].kind = 0 if kind == "adjust" else 1
                arr[k].op = names.index(o[1]) if isinstance(o[1], str) else int(o[1])
                ps = list(o[2]) if len(o) > 2 and o[2] is not None else []
                arr[k].n_params = len(ps)
                for i, v in enumerate(ps):
                    arr[k].params[i] = float(v)
                if len(o) > 3 and o[3] is not None:
                    l = _u8(o[3]); keep.append(l)
                    arr[k].lut = l.ctypes.data
        self._check(self._lib.pfx_chain_dev(self._h, C.c_void_p(src_ptr), C.c_void_p(dst_ptr), C.c_uint32(w), C.c_uint32(h), arr, C.c_uint32(len(ops))))

    def sharpen_dev(self, src_ptr, dst_ptr, w, h, amount, radius, mask_ptr=0):
        self._check(self._lib.pfx_sharpen_dev(self._h, C.c_void_p(src_ptr), C.c_void_p(dst_ptr), C.c_uint32(w), C.c_uint32(h), C.c_float(amount), C.c_float(radius),
                                              C.c_void_p(mask_ptr or None)))

    def glow_dev(self, src_ptr, dst_ptr, w, h, radius, intensity, mask_ptr=0):
        self._check(self._lib.pfx_glow_dev(self._h, C.c_void_p(src_ptr), C.c_void_p(dst_ptr), C.c_uint32(w), C.c_uint32(h), C.c_float(radius), C.c_float(intensity),
                                           C.c_void_p(mask_ptr or None)))

    def box_blur_dev(self, src_ptr, dst_ptr, w, h, radius, mask_ptr=0, tmp_ptr=0):
        self._check(self._lib.pfx_box_blur_dev(self._h, C.c_void_p(src_ptr), C.c_void_p(dst_ptr), C.c_uint32(w), C.c_uint32(h),
                                               C.c_float(radius), C.c_void_p(mask_ptr or None), C.c_void_p(tmp_ptr or None)))

    def box_blur_band_dev(self, src_ptr, dst_ptr, w, h, radius, mask_ptr=0, tmp_ptr=0, first_row=0):
        """pfx_box_blur_band_dev: a band with its halo rows (rows at least ceil(radius) from the buffer's ends equal the whole image's)"""
        self._check(self._lib.pfx_box_blur_band_dev(self._h, C.c_void_p(src_ptr), C.c_void_p(dst_ptr), C.c_uint32(w), C.c_uint32(h), C.c_float(radius),
                                                    C.c_void_p(mask_ptr or None), C.c_void_p(tmp_ptr or None), C.c_uint32(first_row)))

    def median_band_dev(self, src_ptr, dst_ptr, w, h, radius, mask_ptr=0, first_row=0):
        self._check(self._lib.pfx_median_band_dev(self._h, C.c_void_p(src_ptr), C.c_void_p(dst_ptr), C.c_uint32(w), C.c_uint32(h), C.c_uint32(radius),
                                                  C.c_void_p(mask_ptr or None), C.c_uint32(first_row)))

    def median_dev(self, src_ptr, dst_ptr, w, h, radius, mask_ptr=0):
        self._check(self._lib.pfx_median_dev(self._h, C.c_void_p(src_ptr), C.c_void_p(dst_ptr), C.c_uint32(w), C.c_uint32(h),
                                             C.c_uint32(radius), C.c_void_p(mask_ptr or None)))

    def warp_mesh_catmull_rom_dev(self, src_ptr, orig, deformed, cols, rows, w, h, dst_ptr):
        o = None if orig is None else np.ascontiguousarray(orig, np.float32)
        d = np.ascontiguousarray(deformed, np.float32)
        self._check(self._lib.pfx_warp_mesh_catmull_rom_dev(self._h, C.c_void_p(src_ptr), _p(o), _p(d), C.c_uint32(cols),
                                                            C.c_uint32(rows), C.c_uint32(w), C.c_uint32(h), C.c_void_p(dst_ptr)))

    def mesh_displacement_dev(self, orig, deformed, cols, rows, w, h, disp_ptr):
        o = None if orig is None else np.ascontiguousarray(orig, np.float32)
        d = np.ascontiguousarray(deformed, np.float32)
        self._check(self._lib.pfx_mesh_displacement_dev(self._h, _p(o), _p(d), C.c_uint32(cols), C.c_uint32(rows), C.c_uint32(w), C.c_uint32(h),
                                                        C.c_void_p(disp_ptr)))

    def warp_displacement_dev(self, src_ptr, sw, sh, disp_ptr, w, h, dst_ptr):
        self._check(self._lib.pfx_warp_displacement_dev(self._h, C.c_void_p(src_ptr), C.c_uint32(sw), C.c_uint32(sh),
                                                        C.c_void_p(disp_ptr), C.c_uint32(w), C.c_uint32(h), C.c_void_p(dst_ptr)))

    def warp_displacement_band_dev(self, src_ptr, sw, sh, disp_band_ptr, w, band_rows, dst_band_ptr, first_row):
        """rows [first_row, first_row + band_rows) of the warp: the field and the output are bands, the source is whole (pfx_warp_displacement_band_dev)"""
        self._check(self._lib.pfx_warp_displacement_band_dev(self._h, C.c_void_p(src_ptr), C.c_uint32(sw), C.c_uint32(sh), C.c_void_p(disp_band_ptr),
                                                             C.c_uint32(w), C.c_uint32(band_rows), C.c_void_p(dst_band_ptr), C.c_uint32(first_row)))

    def warp_mesh_catmull_rom_band_dev(self, src_ptr, orig, deformed, cols, rows, w, h, dst_band_ptr, first_row, band_rows):
        o = None if orig is None else np.ascontiguousarray(orig, np.float32)
        d = np.ascontiguousarray(deformed, np.float32)
        self._check(self._lib.pfx_warp_mesh_catmull_rom_band_dev(self._h, C.c_void_p(src_ptr), _p(o), _p(d), C.c_uint32(cols), C.c_uint32(rows), C.c_uint32(w),
                                                                 C.c_uint32(h), C.c_void_p(dst_band_ptr), C.c_uint32(first_row), C.c_uint32(band_rows)))

    def warp_last(self, which: int) -> int:
        """what the last call into the warp kernels launched: 0 the bits (1 control points in LDS, 2 PAIR, 4 BUF32, 8 XCD tile order) of the last mesh warp,
        displacement warp or mesh field, 1 / 2 its grid in x / y, 3 the last displacement_brushes_dev (0 no launch, 1 bounding box, 2 chunk list), 4 its chunks;
        -1 = none yet (pfx_int_warp_last; for tests)"""
        return int(self._lib.pfx_int_warp_last(self._h, C.c_int(which)))

    def warp_info(self, which: int) -> int:
        """0 MESH_WALK, 1 MESH_WX, 2 MESH_LDS_PTS, 3 WARP_YR, 4 the tile rows from which the mesh warp takes the XCD order, 5 the dabs culled per trip
        (pfx_int_warp_info; for tests)"""
        return int(self._lib.pfx_int_warp_info(C.c_int(which)))

    def selftest_round_pack(self):
        """(mismatches, signalling-NaN mismatches) of the device's round-and-pack against the step-by-step formula over all 2^32 floats"""
        bad, snan = C.c_uint64(0), C.c_uint64(0)
        self._check(self._lib.pfx_selftest_round_pack(self._h, C.byref(bad), C.byref(snan)))
        return bad.value, snan.value

    def selftest_unorm_store(self) -> int:
        bad = C.c_uint64(0)
        self._check(self._lib.pfx_selftest_unorm_store(self._h, C.byref(bad)))
        return int(bad.value)

    def selftest_division(self, seed: int, n_millions: int) -> int:
        bad = C.c_uint64(0)
        self._check(self._lib.pfx_selftest_division(self._h, C.c_uint64(seed), C.c_uint32(n_millions), C.byref(bad)))
        return int(bad.value)

    def selftest_division_range(self, seed: int, n_millions: int, num_exp, den_exp) -> int:
        """rdiv vs `/` on operands with exponents num_exp = (lo, hi) over den_exp = (lo, hi); the mismatch count"""
        bad = C.c_uint64(0)
        self._check(self._lib.pfx_selftest_division_range(self._h, C.c_uint64(seed), C.c_uint32(n_millions), C.c_int32(num_exp[0]), C.c_int32(num_exp[1]),
                                                          C.c_int32(den_exp[0]), C.c_int32(den_exp[1]), C.byref(bad)))
        return int(bad.value)

    def tune(self, key: str, value: int):
        self._check(self._lib.pfx_tune(self._h, key.encode(), C.c_int(value)))

    def flatten_stats(self, reset: bool = False):
        """work counters of the compositor's dead-layer elimination (pfx_flatten_stats)"""
        out = (C.c_uint64 * 8)()
        self._check(self._lib.pfx_flatten_stats(self._h, out, C.c_int(int(reset))))
        keys = ("rounds", "round_px", "round_layers", "nat_units", "nat_layers", "alpha_reads", "queue_units", "reserved")
        return dict(zip(keys, [int(v) for v in out]))

    def flatten_trace(self, reset: bool = False):
        """per-phase wave clocks of the class-sorting compositor's diagnostic build (pfx_flatten_trace; tune("dle_stats", 4) first)"""
        out = (C.c_uint64 * 16)()
        self._check(self._lib.pfx_flatten_trace(self._h, out, C.c_int(int(reset))))
        v = [int(x) for x in out]
        keys = ("classify", "deal_early", "natural", "store", "early_wait", "early_blend", "natural_wait", "natural_blend")
        return {"wave_clocks": v[0], "waves": v[1], **dict(zip(keys, v[8:16]))}

    def timing_enable(self, on: bool):
        self._check(self._lib.pfx_timing_enable(self._h, C.c_int(int(on))))

    def timing_reset(self):
        self._check(self._lib.pfx_timing_reset(self._h))

    def timing_read(self, name: str):
        ms, n = C.c_double(), C.c_uint64()
        self._check(self._lib.pfx_timing_read(self._h, name.encode(), C.byref(ms), C.byref(n)))
        return ms.value, n.value
