"""A stateful model of the script host API: what a sequence of host-function calls leaves in the image, the selection mask, the console and the
canvas-op list.  Restated from the reference's registrations (src/ops/scripting.rs; the line numbers at each method), not from pfx_script_host.cpp.
The effects go through the CPU oracle; everything else is a few lines of numpy.  Statements arrive as the tuples of tests/script_cases.py.

One rule follows the device instead of the reference: a resize_canvas / resize_image that changes the size drops the selection mask (the reference
keeps the vector of the old size: is_selected then reads it flat, the `_core` effects see an all-zero mask or its first w * h bytes, and
fill_selected / delete_selected index past its end).  pfx_script_host.cpp's header records the divergence.
"""
from __future__ import annotations

import numpy as np

from . import oracle_lib as O

U32 = 0xFFFFFFFF
ANCHORS = {  # parse_anchor, :69-82
    (0, 0): ("top-left", "tl", "nw"), (1, 0): ("top-center", "tc", "n", "top"), (2, 0): ("top-right", "tr", "ne"),
    (0, 1): ("center-left", "cl", "w", "left"), (1, 1): ("center", "c", "middle"), (2, 1): ("center-right", "cr", "e", "right"),
    (0, 2): ("bottom-left", "bl", "sw"), (1, 2): ("bottom-center", "bc", "s", "bottom"), (2, 2): ("bottom-right", "br", "se"),
}
FILTERS = {"nearest": ("nearest", "nn"), "bicubic": ("bicubic", "catmull", "catmullrom"), "lanczos3": ("lanczos", "lanczos3")}  # parse_script_filter, :60-67
FILTER_IDS = {"nearest": 0, "bilinear": 1, "bicubic": 2, "lanczos3": 3}
OP_FLIP_H, OP_FLIP_V, OP_ROT_CW, OP_ROT_CCW, OP_ROT_180, OP_RESIZE_IMAGE, OP_RESIZE_CANVAS = range(7)


def parse_anchor(name):
    n = name.lower()
    return next((k for k, names in ANCHORS.items() if n in names), (0, 0))


def parse_filter(name):
    n = name.lower()
    return next((k for k, names in FILTERS.items() if n in names), "bilinear")


def clamp_size(v):
    """`(v.max(1) as u32).min(32768)`, :750, :782"""
    return min(max(int(v), 1) & U32, 32768)


def trunc_div2(d):
    """i32 `/ 2`: toward zero"""
    return -((-d) // 2) if d < 0 else d // 2


def u8(v):
    return min(max(int(v), 0), 255)


def flip_rotate_np(img, mode):
    """imageops::flip_horizontal / flip_vertical / rotate90 / rotate270 / rotate180"""
    if mode == "flip_horizontal":
        out = img[:, ::-1]
    elif mode == "flip_vertical":
        out = img[::-1]
    elif mode == "rotate_180":
        out = img[::-1, ::-1]
    elif mode == "rotate_90cw":
        out = np.rot90(img, -1)
    elif mode == "rotate_90ccw":
        out = np.rot90(img, 1)
    else:
        raise KeyError(mode)
    return np.ascontiguousarray(out)


def anchor_offset(anchor, new, old):
    return 0 if anchor == 0 else (trunc_div2(new - old) if anchor == 1 else new - old)


def resize_canvas_np(img, new_w, new_h, anchor, fill=(0, 0, 0, 0)):
    """:786-812: every old pixel goes to (x + offset_x, y + offset_y) if that is inside the new image"""
    h, w = img.shape[:2]
    ox, oy = anchor_offset(anchor[0], new_w, w), anchor_offset(anchor[1], new_h, h)
    out = np.empty((new_h, new_w, 4), np.uint8)
    out[:] = np.asarray(fill, np.uint8)
    x0, x1, y0, y1 = max(ox, 0), min(ox + w, new_w), max(oy, 0), min(oy + h, new_h)
    if x0 < x1 and y0 < y1:
        out[y0:y1, x0:x1] = img[y0 - oy:y1 - oy, x0 - ox:x1 - ox]
    return out


def fmt(v):
    """how print() shows a bool, an integer and an array of integers"""
    if isinstance(v, (bool, np.bool_)):
        return "true" if v else "false"
    if isinstance(v, (list, tuple)):
        return "[" + ", ".join(str(int(x)) for x in v) + "]"
    return str(int(v))


class ScriptFailure(Exception):
    def __init__(self, line):
        super().__init__(f"the statement on line {line} fails")
        self.line = line


class Model:
    def __init__(self, pixels, mask=None):
        self.pixels = np.array(pixels, np.uint8)
        self.mask = None if mask is None else np.array(mask, np.uint8).reshape(-1)
        self.console = []
        self.ops = []

    @property
    def w(self):
        return self.pixels.shape[1]

    @property
    def h(self):
        return self.pixels.shape[0]

    def run(self, statements):
        """one statement per line; raises ScriptFailure with the line of a failing statement"""
        for k, st in enumerate(statements):
            if st[0] in ("fail_div", "fail_unknown"):
                raise ScriptFailure(k + 1)
            if st[0] == "print":
                self.console.append(fmt(getattr(self, st[1])(*st[2:])))
            else:
                getattr(self, st[0])(*st[1:])
        return self

    def _inside(self, x, y):
        return 0 <= x < self.w and 0 <= y < self.h

    def _mask2d(self):
        """:627-630 GrayImage::from_raw(w, h, mask): the flat bytes read as h rows of w"""
        if self.mask is None:
            return None
        assert self.mask.size == self.w * self.h   # kept so by resize_canvas / resize_image below
        return self.mask.reshape(self.h, self.w)

    def _selected(self):
        m = self._mask2d()
        return np.ones((self.h, self.w), bool) if m is None else m > 0

    # ---------------------------------------------------------------- canvas info :323-349
    def width(self):
        return self.w

    def height(self):
        return self.h

    def is_selected(self, x, y):
        if not self._inside(x, y):
            return False
        if self.mask is None:
            return True
        idx = y * self.w + x
        return idx < self.mask.size and self.mask[idx] > 0

    # ---------------------------------------------------------------- pixel access :355-435
    def get_pixel(self, x, y):
        return [int(v) for v in self.pixels[y, x]] if self._inside(x, y) else [0, 0, 0, 0]

    def set_pixel(self, x, y, r, g, b, a):
        if self._inside(x, y):
            self.pixels[y, x] = [u8(r), u8(g), u8(b), u8(a)]

    def _get(self, c, x, y):
        return int(self.pixels[y, x, c]) if self._inside(x, y) else 0

    def _set(self, c, x, y, v):
        if self._inside(x, y):
            self.pixels[y, x, c] = u8(v)

    def get_r(self, x, y): return self._get(0, x, y)
    def get_g(self, x, y): return self._get(1, x, y)
    def get_b(self, x, y): return self._get(2, x, y)
    def get_a(self, x, y): return self._get(3, x, y)
    def set_r(self, x, y, v): self._set(0, x, y, v)
    def set_g(self, x, y, v): self._set(1, x, y, v)
    def set_b(self, x, y, v): self._set(2, x, y, v)
    def set_a(self, x, y, v): self._set(3, x, y, v)

    # ---------------------------------------------------------------- the three fixed closures :442-609
    def closure_map_invert(self):
        """map_channels(|r, g, b, a| [255 - r, 255 - g, 255 - b, a])"""
        self.pixels[..., :3] = 255 - self.pixels[..., :3]

    def closure_each_selected(self):
        """for_each_pixel: invert where is_selected(x, y), which reads the mask flat (:337-348)"""
        sel = self._selected()
        self.pixels[..., :3] = np.where(sel[..., None], 255 - self.pixels[..., :3], self.pixels[..., :3])

    def closure_region(self, rx, ry, rw, rh):
        """for_region(rx, ry, rw, rh, |x, y, r, g, b, a| [b, g, r, a]), bounds :513-516"""
        x0, y0 = max(rx, 0) & U32, max(ry, 0) & U32
        x1, y1 = min((rx + rw) & U32, self.w), min((ry + rh) & U32, self.h)
        if x0 < x1 and y0 < y1:
            self.pixels[y0:y1, x0:x1, :3] = self.pixels[y0:y1, x0:x1, 2::-1].copy()

    # ---------------------------------------------------------------- transforms :640-819
    def _permute(self, mode, op):
        self.pixels = flip_rotate_np(self.pixels, mode)   # the mask is not touched: its bytes are read flat at the new width afterwards
        if op is not None:
            self.ops.append((op, 0, 0, 0, 0))

    def flip_horizontal(self): self._permute("flip_horizontal", None)
    def flip_vertical(self): self._permute("flip_vertical", None)
    def rotate_180(self): self._permute("rotate_180", None)
    def flip_canvas_horizontal(self): self._permute("flip_horizontal", OP_FLIP_H)
    def flip_canvas_vertical(self): self._permute("flip_vertical", OP_FLIP_V)
    def rotate_canvas_90cw(self): self._permute("rotate_90cw", OP_ROT_CW)
    def rotate_canvas_90ccw(self): self._permute("rotate_90ccw", OP_ROT_CCW)
    def rotate_canvas_180(self): self._permute("rotate_180", OP_ROT_180)

    def resize_image(self, new_w, new_h, method):   # :749-770
        nw, nh, filt = clamp_size(new_w), clamp_size(new_h), parse_filter(method)
        if (nw, nh) == (self.w, self.h):
            return
        self.pixels = O.resize(self.pixels, nw, nh, filt)
        self.ops.append((OP_RESIZE_IMAGE, nw, nh, FILTER_IDS[filt], 0))
        self.mask = None   # the device's rule, see the module text

    def resize_canvas(self, new_w, new_h, anchor):   # :781-818
        nw, nh, an = clamp_size(new_w), clamp_size(new_h), parse_anchor(anchor)
        changed = (nw, nh) != (self.w, self.h)
        self.pixels = resize_canvas_np(self.pixels, nw, nh, an)
        self.ops.append((OP_RESIZE_CANVAS, nw, nh, an[0], an[1]))
        if changed:
            self.mask = None   # the device's rule, see the module text

    # ---------------------------------------------------------------- `_core` effects :616-634, :822-1165: the mask limits them
    def _core(self, fn, *args):
        self.pixels = fn(np.ascontiguousarray(self.pixels), *args, mask=self._mask2d())

    def apply_blur(self, sigma): self._core(O.gaussian_blur, sigma)                                   # :825
    def apply_box_blur(self, radius): self._core(O.box_blur, float(radius))                           # :832
    def apply_sharpen(self, amount): self._core(O.sharpen, amount, 1.0)                               # :847
    def apply_reduce_noise(self, strength): self._core(O.reduce_noise, strength, 2)                   # :854
    def apply_median(self, radius): self._core(O.median, max(radius, 1) & U32)                        # :861
    def apply_noise(self, amount, mono): self._core(O.add_noise, amount, "gaussian", mono, 42, 1.0, 1)  # :1079
    def apply_pixelate(self, size): self._core(O.pixelate, max(size, 1) & U32)                        # :1096
    def apply_crystallize(self, size): self._core(O.crystallize, float(max(size, 1)), 42)             # :1103
    def apply_bulge(self, amount): self._core(O.bulge, amount, (0.5, 0.5))                            # :1110
    def apply_glow(self, radius, intensity): self._core(O.glow, radius, intensity)                    # :1125
    def apply_vignette(self, strength, softness): self._core(O.vignette, strength, softness)          # :1132
    def apply_halftone(self, dot): self._core(O.halftone, dot, 45.0, "circle")                        # :1139
    def apply_ink(self, strength, threshold): self._core(O.ink, strength, threshold)                  # :1153
    def apply_oil_painting(self, radius): self._core(O.oil_painting, max(radius, 1) & U32, 20)        # :1160

    # ---------------------------------------------------------------- inline effects :869-1075: the mask is ignored
    def _inline(self, op, params=()):
        self.pixels = O.rhai_adjust(self.pixels, op, list(params))

    def apply_invert(self): self._inline("invert")
    def apply_desaturate(self): self._inline("desaturate")
    def apply_sepia(self, strength=None):
        if strength is None:
            self._inline("sepia")
        else:
            self._inline("sepia_strength", [min(max(strength, 0.0), 1.0)])   # clamped in f64 before the cast, :921
    def apply_brightness_contrast(self, b, c): self._inline("brightness_contrast", [b, c])
    def apply_hsl(self, hue, sat, light): self._inline("hsl", [hue, sat, light])
    def apply_exposure(self, ev): self._inline("exposure", [ev])
    def apply_levels(self, black, white, gamma): self._inline("levels", [black, white, gamma])

    # ---------------------------------------------------------------- selection :1356-1481
    def select_rect(self, x1, y1, x2, y2):
        def cl(v, lim):
            return min(max(v, 0) & U32, lim)   # `as u32` on an i64 truncates
        m = np.zeros((self.h, self.w), np.uint8)
        m[cl(y1, self.h):cl(y2, self.h), cl(x1, self.w):cl(x2, self.w)] = 255
        self.mask = m.reshape(-1)

    def select_ellipse(self, cx, cy, rx, ry):
        with np.errstate(over="ignore", invalid="ignore"):
            rx2, ry2 = max(np.float64(rx) * np.float64(rx), 0.001), max(np.float64(ry) * np.float64(ry), 0.001)
            yy, xx = np.mgrid[0:self.h, 0:self.w].astype(np.float64)
            dx, dy = xx - np.float64(cx), yy - np.float64(cy)
            inside = (dx * dx) / rx2 + (dy * dy) / ry2 <= 1.0
        self.mask = np.where(inside, 255, 0).astype(np.uint8).reshape(-1)

    def clear_selection(self):
        self.mask = None

    def has_selection(self):
        return self.mask is not None

    def invert_selection(self):
        self.mask = np.zeros(self.w * self.h, np.uint8) if self.mask is None else (255 - self.mask)

    def fill_selected(self, r, g, b, a):
        self.pixels[self._selected()] = [u8(r), u8(g), u8(b), u8(a)]

    def delete_selected(self):
        self.pixels[self._selected()] = 0
