/*
 * pfx.h — C ABI of libpfx: the MI355X (gfx950) raster pixel pipeline behind PaintFE's operator surface.
 *
 * This is the drop-in boundary.  Every entry point replaces one reference interface (cited as
 * `ref: file:line`, relative to the PaintFE checkout) and keeps its argument meaning and results:
 *   - numerics are those of the reference's **CPU** path (src/ops, src/canvas), not of its WGSL shaders:
 *     bit-exact for the compositor and the integer filters, +-1 LSB worst case (normally 0) for the
 *     float-intermediate filters;
 *   - images are tight row-major straight-alpha RGBA8 (`image::RgbaImage`), `w*h*4` bytes;
 *   - selection masks are `w*h` bytes (`image::GrayImage`), 0 = leave the pixel alone (ref: src/ops/effects.rs:34-41);
 *   - all calls are blocking with respect to the host (like the reference's `device.poll(Wait)` readback,
 *     ref: src/gpu/compute/helpers.rs:147-206) unless the name ends in `_dev`;
 *   - on any error the function returns a negative pfx_status and leaves `dst` untouched, so the caller
 *     can fall back to its CPU path (the reference's own contract, ref: src/ops/adjustments.rs:1045).
 *
 * Two tiers:
 *   host-buffer calls   (`pfx_blur_rgba`, ...)   = the literal `GpuRenderer` / `_core` signatures;
 *   device-resident calls (`..._dev`)            = same kernels on caller-owned device memory and the
 *                                                  context's HIP stream: upload once, chain ops, download once.
 *
 * Device pointers handed to `_dev` calls must be 16-byte aligned (hipMalloc / pfx_dev_alloc results and row-aligned sub-buffers
 * are): the kernels move pixels in 16-byte vectors.  No C++ exception leaves the library: entry points that parse untrusted bytes or run
 * scripts convert allocation failures into PFX_ERR_OOM.
 *
 * Arguments are checked before anything is touched: a NULL context, buffer or description, a zero-sized image, an image of more than 256 000 000 pixels
 * (the reference's document limit, src/canvas/tiled_image.rs:15-26 — the kernels index pixels in 32 bits under it), a rectangle outside its image or a
 * parameter that would set an unbounded per-pixel loop count returns PFX_ERR_INVALID / PFX_ERR_UNSUPPORTED with pfx_last_error() saying which
 * (tests/test_abi_hostile.py sweeps every prototype of this header).
 *
 * One pfx_ctx = one HIP device + one stream.  A context is not thread-safe (neither is the reference's
 * `&mut GpuRenderer`); distinct contexts are independent.  No torch / C++ types cross this boundary.
 */
#ifndef PFX_H
#define PFX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PFX_ABI_VERSION 1
#define PFX_CHUNK 64   /* ref: src/canvas/defs.rs:7 CHUNK_SIZE */
#define PFX_MAX_LAYERS 256 /* ref: src/io.rs:503 MAX_LAYERS */

typedef enum pfx_status {
    PFX_OK = 0,
    PFX_ERR_INVALID = -1,     /* bad argument (null pointer, zero size, unknown id) */
    PFX_ERR_NO_DEVICE = -2,   /* no usable HIP device: GpuRenderer::try_new -> None (ref: src/gpu/renderer.rs:261) */
    PFX_ERR_HIP = -3,         /* a HIP call failed; pfx_last_error() has the text */
    PFX_ERR_OOM = -4,
    PFX_ERR_UNSUPPORTED = -5, /* e.g. median radius beyond the device path: caller uses its CPU path (ref: renderer.rs:945) */
    PFX_ERR_SCRIPT = -6       /* script front-end error; see pfx_script_result */
} pfx_status;

typedef struct pfx_ctx pfx_ctx;

/* ---- context (ref: GpuRenderer::try_new / new / Drop, src/gpu/renderer.rs:249-300,969) ---- */
int         pfx_ctx_create(int device, pfx_ctx** out);
void        pfx_ctx_destroy(pfx_ctx* ctx);
const char* pfx_last_error(const pfx_ctx* ctx);          /* never NULL */
int         pfx_device_count(void);
int         pfx_abi_version(void);
/* Numeric mode for the float-intermediate stencil (Gaussian): 0 = fused multiply-add allowed (default,
 * +-1 LSB class), 1 = reference evaluation order without FMA contraction (bit-exact with the CPU path). */
int         pfx_ctx_set_exact(pfx_ctx* ctx, int exact);
void*       pfx_ctx_stream(pfx_ctx* ctx);                 /* hipStream_t of this context */
/* adopt != 0: run on the caller's hipStream_t (NULL = the device's default stream, which is what torch's default
 * stream is); adopt == 0: back to the context's own stream.  Lets `_dev` calls interleave in order with a host
 * framework's kernels and RCCL collectives without host synchronisation. */
int         pfx_ctx_set_stream(pfx_ctx* ctx, void* hip_stream, int adopt);
int         pfx_ctx_synchronize(pfx_ctx* ctx);

/* ---- device memory helpers for the `_dev` tier ---- */
int pfx_dev_alloc(pfx_ctx* ctx, size_t bytes, void** out_dev);
int pfx_dev_free(pfx_ctx* ctx, void* dev);
int pfx_dev_upload(pfx_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes);   /* async on ctx stream + sync */
int pfx_dev_download(pfx_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes);
int pfx_dev_memset(pfx_ctx* ctx, void* dst_dev, int value, size_t bytes);
/* Page-locked host memory for the host-buffer entry points (the reference's `&[u8]` in, `Vec<u8>` out seams, src/gpu/renderer.rs:915-947): a caller that keeps its
 * pixels in such buffers moves them at the link's rate (~55 GB/s per direction) instead of the pageable path's ~20 (8K invert_rgba: 13.9 -> ~6 ms, both directions).
 * Ordinary malloc'ed / Vec memory stays valid everywhere; this is an optimisation the caller may take. */
int pfx_host_alloc(pfx_ctx* ctx, size_t bytes, void** out_host);
int pfx_host_free(pfx_ctx* ctx, void* host);

/* ================= B1: GpuRenderer filter methods (ref: src/gpu/renderer.rs:915-947) ================= */
/* blur_rgba(&[u8], w, h, sigma) -> Vec<u8>; numerics: ops::filters::parallel_gaussian_blur (ref: src/ops/filters.rs:242-316) */
int pfx_blur_rgba(pfx_ctx* ctx, const uint8_t* src, uint8_t* dst, uint32_t w, uint32_t h, float sigma);
/* brightness_contrast_rgba; numerics: ops::adjustments::brightness_contrast (ref: src/ops/adjustments.rs:265-294) */
int pfx_brightness_contrast_rgba(pfx_ctx* ctx, const uint8_t* src, uint8_t* dst, uint32_t w, uint32_t h,
                                 float brightness, float contrast);
/* hsl_rgba(hue deg, sat, light); numerics: hue_saturation_lightness (ref: src/ops/adjustments.rs:300-347) */
int pfx_hsl_rgba(pfx_ctx* ctx, const uint8_t* src, uint8_t* dst, uint32_t w, uint32_t h, float hue, float sat, float light);
/* invert_rgba; numerics: invert_colors (ref: src/ops/adjustments.rs:115) */
int pfx_invert_rgba(pfx_ctx* ctx, const uint8_t* src, uint8_t* dst, uint32_t w, uint32_t h);
/* median_rgba(radius) -> Option<Vec<u8>>; numerics: median_core (ref: src/ops/effects/noise.rs:357-410).
 * The reference's GPU method returns None for radius > 7 and its CPU median_core has no cap; here radii up to 24 run the tile
 * kernels (selection networks / binary search) and larger ones a sliding-histogram kernel; PFX_ERR_UNSUPPORTED only beyond
 * PFX_MEDIAN_MAX_RADIUS (a 255 x 255 window, the 16-bit histogram counters' limit). */
#define PFX_MEDIAN_MAX_RADIUS 127
int pfx_median_rgba(pfx_ctx* ctx, const uint8_t* src, uint8_t* dst, uint32_t w, uint32_t h, uint32_t radius);

/* ================= B4: pure `_core` functions with optional selection mask ================= */
/* blur_with_selection_pub (ref: src/ops/filters.rs:130-207) */
int pfx_gaussian_blur_core(pfx_ctx* ctx, const uint8_t* src, uint8_t* dst, uint32_t w, uint32_t h, float sigma,
                           const uint8_t* mask);
/* box_blur_core (ref: src/ops/effects/blur.rs:233-318) */
int pfx_box_blur_core(pfx_ctx* ctx, const uint8_t* src, uint8_t* dst, uint32_t w, uint32_t h, float radius,
                      const uint8_t* mask);
/* median_core (ref: src/ops/effects/noise.rs:357-410) */
int pfx_median_core(pfx_ctx* ctx, const uint8_t* src, uint8_t* dst, uint32_t w, uint32_t h, uint32_t radius,
                    const uint8_t* mask);
/* pixelate_core (ref: src/ops/effects/distort.rs:333-373) */
int pfx_pixelate_core(pfx_ctx* ctx, const uint8_t* src, uint8_t* dst, uint32_t w, uint32_t h, uint32_t block_size,
                      const uint8_t* mask);
/* effects that reuse the same kernels.  sharpen / glow / drop shadow feed a Gaussian into a gain, so they run the BIT-EXACT Gaussian in every
 * context (the reference's tests hold them at tolerance 0: tests/visual_filters.rs:43-55,154-165); pfx_tune(ctx, "gauss_fast_effects", 1) opts a context into the
 * default-mode Gaussian there too (faster; its +-1 LSB then enters `amount` / `intensity` times). */
/* sharpen_core(flat, amount, radius, mask) (ref: src/ops/effects/stylize.rs:96-143) */
int pfx_sharpen_core(pfx_ctx* ctx, const uint8_t* src, uint8_t* dst, uint32_t w, uint32_t h, float amount, float radius,
                     const uint8_t* mask);
/* glow_core(flat, radius, intensity, mask) (ref: src/ops/effects/stylize.rs:26-70) */
int pfx_glow_core(pfx_ctx* ctx, const uint8_t* src, uint8_t* dst, uint32_t w, uint32_t h, float radius, float intensity,
                  const uint8_t* mask);
/* bokeh_blur_core(flat, radius, mask) (ref: src/ops/effects/blur.rs:22-115) */
int pfx_bokeh_blur_core(pfx_ctx* ctx, const uint8_t* src, uint8_t* dst, uint32_t w, uint32_t h, float radius,
                        const uint8_t* mask);
/* motion_blur_core(flat, angle_deg, distance, mask) (ref: src/ops/effects/blur.rs:144-210) */
int pfx_motion_blur_core(pfx_ctx* ctx, const uint8_t* src, uint8_t* dst, uint32_t w, uint32_t h, float angle_deg,
                         float distance, const uint8_t* mask);

/* ---- the rest of the effect bank: every remaining `*_core(flat, params.., mask) -> RgbaImage` of src/ops/effects/ ----
 * Same convention as above (caller-allocated dst, mask = w*h bytes or NULL, 0 leaves the pixel).  Integer / hash based
 * effects are bit-exact with the CPU path; twist, gaussian noise, reduce_noise and vignette evaluate one libm function
 * per pixel and are in the +-1 LSB class.  Enumerations mirror the reference enums in declaration order. */
enum { PFX_NOISE_UNIFORM = 0, PFX_NOISE_GAUSSIAN = 1, PFX_NOISE_PERLIN = 2 };                        /* NoiseType, distort.rs:501-506 */
enum { PFX_HALFTONE_CIRCLE = 0, PFX_HALFTONE_SQUARE = 1, PFX_HALFTONE_DIAMOND = 2, PFX_HALFTONE_LINE = 3 }; /* HalftoneShape, stylize.rs:195-201 */
enum { PFX_GRID_LINES = 0, PFX_GRID_CHECKERBOARD = 1 };                                              /* GridStyle, stylize.rs:285-289 */
enum { PFX_OUTLINE_OUTSIDE = 0, PFX_OUTLINE_INSIDE = 1, PFX_OUTLINE_CENTER = 2 };                    /* OutlineMode, render.rs:353-358 */
enum { PFX_COLOR_FILTER_MULTIPLY = 0, PFX_COLOR_FILTER_SCREEN = 1, PFX_COLOR_FILTER_OVERLAY = 2, PFX_COLOR_FILTER_SOFT_LIGHT = 3 }; /* artistic.rs:219-225 */
/* zoom_blur_core (ref: src/ops/effects/blur.rs:322-427); tint_color = RGBA in 0..1, may be NULL (= no tint) */
int pfx_zoom_blur_core(pfx_ctx* ctx, const uint8_t* src, uint8_t* dst, uint32_t w, uint32_t h, float center_x, float center_y, float strength,
                       uint32_t samples, const float tint_color[4], float tint_strength, const uint8_t* mask);
/* crystallize_core (ref: src/ops/effects/distort.rs:26-169) */
int pfx_crystallize_core(pfx_ctx* ctx, const uint8_t* src, uint8_t* dst, uint32_t w, uint32_t h, float cell_size, uint32_t seed, const uint8_t* mask);
/* dents_core (ref: src/ops/effects/distort.rs:248-310) */
int pfx_dents_core(pfx_ctx* ctx, const uint8_t* src, uint8_t* dst, uint32_t w, uint32_t h, float scale, float amount, uint32_t seed,
                   uint32_t octaves, float roughness, int pinch, int wrap, const uint8_t* mask);
/* bulge_core_at / twist_core_at (ref: src/ops/effects/distort.rs:400-437, 464-493); bulge_core / twist_core = origin (0.5, 0.5) */
int pfx_bulge_core(pfx_ctx* ctx, const uint8_t* src, uint8_t* dst, uint32_t w, uint32_t h, float amount, float origin_x, float origin_y,
                   const uint8_t* mask);
int pfx_twist_core(pfx_ctx* ctx, const uint8_t* src, uint8_t* dst, uint32_t w, uint32_t h, float angle_deg, float origin_x, float origin_y,
                   const uint8_t* mask);
/* add_noise_core (ref: src/ops/effects/noise.rs:73-143) */
int pfx_add_noise_core(pfx_ctx* ctx, const uint8_t* src, uint8_t* dst, uint32_t w, uint32_t h, float amount, int noise_type, int monochrome,
                       uint32_t seed, float scale, uint32_t octaves, const uint8_t* mask);
/* reduce_noise_core (ref: src/ops/effects/noise.rs:172-261) */
int pfx_reduce_noise_core(pfx_ctx* ctx, const uint8_t* src, uint8_t* dst, uint32_t w, uint32_t h, float strength, uint32_t radius,
                          const uint8_t* mask);
/* vignette_core (ref: src/ops/effects/stylize.rs:170-191) */
int pfx_vignette_core(pfx_ctx* ctx, const uint8_t* src, uint8_t* dst, uint32_t w, uint32_t h, float amount, float softness, const uint8_t* mask);
/* halftone_core (ref: src/ops/effects/stylize.rs:242-277) */
int pfx_halftone_core(pfx_ctx* ctx, const uint8_t* src, uint8_t* dst, uint32_t w, uint32_t h, float dot_size, float angle_deg, int shape,
                      const uint8_t* mask);
/* grid_core (ref: src/ops/effects/render.rs:52-92) */
int pfx_grid_core(pfx_ctx* ctx, const uint8_t* src, uint8_t* dst, uint32_t w, uint32_t h, uint32_t cell_w, uint32_t cell_h, uint32_t line_width,
                  const uint8_t color[4], int style, float opacity, const uint8_t* mask);
/* canvas_border_core (ref: src/ops/effects/render.rs:114-165) */
int pfx_canvas_border_core(pfx_ctx* ctx, const uint8_t* src, uint8_t* dst, uint32_t w, uint32_t h, uint32_t width, const uint8_t color[4],
                           const uint8_t* mask);
/* shadow_core (ref: src/ops/effects/render.rs:220-349); the Gaussian inside follows pfx_ctx_set_exact */
int pfx_shadow_core(pfx_ctx* ctx, const uint8_t* src, uint8_t* dst, uint32_t w, uint32_t h, int32_t offset_x, int32_t offset_y, float blur_radius,
                    int widen_radius, const uint8_t color[4], float opacity, const uint8_t* mask);
/* outline_core (ref: src/ops/effects/render.rs:403-572) */
int pfx_outline_core(pfx_ctx* ctx, const uint8_t* src, uint8_t* dst, uint32_t w, uint32_t h, uint32_t width, const uint8_t color[4], int mode,
                     int anti_alias, const uint8_t* mask);
/* pixel_drag_core (ref: src/ops/effects/glitch.rs:44-99) */
int pfx_pixel_drag_core(pfx_ctx* ctx, const uint8_t* src, uint8_t* dst, uint32_t w, uint32_t h, uint32_t seed, float amount, uint32_t distance,
                        float direction, const uint8_t* mask);
/* rgb_displace_core(flat, r_off, g_off, b_off, mask) (ref: src/ops/effects/glitch.rs:142-196) */
int pfx_rgb_displace_core(pfx_ctx* ctx, const uint8_t* src, uint8_t* dst, uint32_t w, uint32_t h, int32_t r_dx, int32_t r_dy, int32_t g_dx,
                          int32_t g_dy, int32_t b_dx, int32_t b_dy, const uint8_t* mask);
/* ink_core (ref: src/ops/effects/artistic.rs:31-99) */
int pfx_ink_core(pfx_ctx* ctx, const uint8_t* src, uint8_t* dst, uint32_t w, uint32_t h, float edge_strength, float threshold, const uint8_t* mask);
/* oil_painting_core (ref: src/ops/effects/artistic.rs:123-215) */
int pfx_oil_painting_core(pfx_ctx* ctx, const uint8_t* src, uint8_t* dst, uint32_t w, uint32_t h, uint32_t radius, uint32_t levels,
                          const uint8_t* mask);
/* color_filter_core (ref: src/ops/effects/artistic.rs:266-309) */
int pfx_color_filter_core(pfx_ctx* ctx, const uint8_t* src, uint8_t* dst, uint32_t w, uint32_t h, const uint8_t filter_color[4], float intensity,
                          int mode, const uint8_t* mask);
/* contours_core (ref: src/ops/effects/contours.rs:56-112) */
int pfx_contours_core(pfx_ctx* ctx, const uint8_t* src, uint8_t* dst, uint32_t w, uint32_t h, float scale, float frequency, float line_width,
                      const uint8_t line_color[4], uint32_t seed, uint32_t octaves, float blend, const uint8_t* mask);

/* ---- the pointwise adjustment bank: one entry point, op id + parameter block ----
 * ops::adjustments flavour (f32, `.round().clamp(0,255) as u8`), ref: src/ops/adjustments.rs:21-108 */
typedef enum pfx_adjust_op {
    PFX_OP_INVERT = 0,           /* :115   params: -                                   */
    PFX_OP_INVERT_ALPHA,         /* :123   params: -                                   */
    PFX_OP_SEPIA,                /* :133   params: -                                   */
    PFX_OP_BRIGHTNESS_CONTRAST,  /* :265   params: brightness, contrast                */
    PFX_OP_HSL,                  /* :300   params: hue_shift(deg), saturation, lightness */
    PFX_OP_EXPOSURE,             /* :352   params: ev  (gain = powf(2, ev) on the host) */
    PFX_OP_HIGHLIGHTS_SHADOWS,   /* :374   params: shadows, highlights                 */
    PFX_OP_TEMPERATURE_TINT,     /* :517   params: temperature, tint                   */
    PFX_OP_THRESHOLD,            /* :1240  params: level                               */
    PFX_OP_POSTERIZE,            /* :1267  params: levels (>= 2)                       */
    PFX_OP_COLOR_BALANCE,        /* :1294  params: shadows[3], midtones[3], highlights[3] */
    PFX_OP_GRADIENT_MAP,         /* :1344  lut: 256 x RGBA                             */
    PFX_OP_BLACK_AND_WHITE,      /* :1373  params: r_weight, g_weight, b_weight        */
    PFX_OP_VIBRANCE,             /* :1408  params: amount                              */
    PFX_OP_LUT_RGBA,             /* levels :465 / curves :584 / auto-levels :144; lut: R[256] G[256] B[256] A[256] */
    PFX_OP_DESATURATE,           /* filters.rs:321 (BT.709, round)                     */
    PFX_OP_COUNT
} pfx_adjust_op;

/* How TiledImage sparsity leaks into the result (ref: src/canvas/tiled_image.rs:50-104,905-932):
 *   PFX_DENSE      arithmetic on every pixel, no chunk effects;
 *   PFX_FROM_FLAT  `*_from_flat` + `TiledImage::from_rgba_image(&out)`: 64x64 chunks of the result whose alpha is
 *                  all zero read back as zeros (ref: src/ops/adjustments.rs:105);
 *   PFX_IN_PLACE   `apply_pixel_transform`: only chunks populated in the input are visited, the others read
 *                  back as zeros (ref: src/ops/adjustments.rs:21-42). */
typedef enum pfx_sparse_mode { PFX_DENSE = 0, PFX_FROM_FLAT = 1, PFX_IN_PLACE = 2 } pfx_sparse_mode;

int pfx_adjust(pfx_ctx* ctx, const uint8_t* src, uint8_t* dst, uint32_t w, uint32_t h, int op,
               const float* params, uint32_t n_params, const uint8_t* lut, const uint8_t* mask, int sparse_mode);

/* Rhai-inline flavour (truncating `as u8`, alpha untouched, selection ignored), ref: src/ops/scripting.rs:869-1075 */
typedef enum pfx_rhai_op {
    PFX_RHAI_INVERT = 0, PFX_RHAI_DESATURATE, PFX_RHAI_SEPIA, PFX_RHAI_SEPIA_STRENGTH,
    PFX_RHAI_BRIGHTNESS_CONTRAST, PFX_RHAI_HSL, PFX_RHAI_EXPOSURE, PFX_RHAI_LEVELS, PFX_RHAI_COUNT
} pfx_rhai_op;
int pfx_rhai_adjust(pfx_ctx* ctx, uint8_t* pixels_inout, uint32_t w, uint32_t h, int op, const float* params,
                    uint32_t n_params);

/* LUT builders (host-side in the reference as well; glibc powf/sqrtf like Rust's f32 methods on Linux) */
void pfx_build_levels_lut(float in_black, float in_white, float gamma, float out_black, float out_white,
                          uint8_t lut[256]);                                   /* ref: adjustments.rs:465-488 */
void pfx_build_curves_lut(const float* points_xy, uint32_t n_points, uint8_t lut[256]); /* ref: adjustments.rs:640-729 */
void pfx_build_stretch_lut(uint8_t min, uint8_t max, uint8_t lut[256]);        /* ref: adjustments.rs:235-256 */
/* auto_levels: device min/max reduction over selected non-transparent pixels, then stretch LUTs (ref: :144-233) */
int  pfx_auto_levels(pfx_ctx* ctx, const uint8_t* src, uint8_t* dst, uint32_t w, uint32_t h, const uint8_t* mask);

/* ================= B2: compositor (ref: src/gpu/renderer.rs:324-586, numerics src/canvas/canvas_state.rs:505-698) ===== */
/* ensure_layer_texture(idx, w, h, data, generation): upload skipped when (generation, w, h) unchanged */
int pfx_layer_upload(pfx_ctx* ctx, uint32_t layer_idx, uint32_t w, uint32_t h, const uint8_t* rgba, uint64_t generation);
/* update_layer_rect(idx, region, data): `data` is the tight region (rw*rh*4) */
int pfx_layer_update_rect(pfx_ctx* ctx, uint32_t layer_idx, uint32_t x, uint32_t y, uint32_t rw, uint32_t rh,
                          const uint8_t* rgba);
/* optional live layer mask ("conceal" alpha, w*h bytes; NULL removes it) (ref: src/canvas/layers.rs:606-620) */
int pfx_layer_set_mask(pfx_ctx* ctx, uint32_t layer_idx, const uint8_t* conceal);
int pfx_layer_remove(pfx_ctx* ctx, uint32_t layer_idx);
int pfx_layer_clear(pfx_ctx* ctx);
uint32_t pfx_layer_count(const pfx_ctx* ctx);
size_t   pfx_layer_memory(const pfx_ctx* ctx);     /* active_texture_memory, ref: renderer.rs:956 */

typedef enum pfx_layer_kind { /* ref: src/canvas/layers.rs:249-262 AdjustmentKind */
    PFX_LAYER_RASTER = 0, PFX_ADJ_EXPOSURE = 1, PFX_ADJ_BRIGHTNESS_CONTRAST = 2, PFX_ADJ_INVERT = 3, PFX_ADJ_CHANNEL_MIXER = 4
} pfx_layer_kind;

typedef struct pfx_layer_info { /* the `(layer_idx, opacity, visible, blend_mode_u8)` tuple, bottom -> top */
    uint32_t layer_idx;
    float    opacity;
    uint8_t  visible;
    uint8_t  blend_mode;   /* BlendMode::to_u8, ref: src/canvas/layers.rs:125-153; unknown ids = Normal */
    uint8_t  kind;         /* pfx_layer_kind; adjustment layers need no uploaded pixels */
    uint8_t  _pad;
    float    adj[16];      /* Exposure [ev]; B/C [brightness, contrast]; ChannelMixer red[4] green[4] blue[4] alpha[4] */
} pfx_layer_info;

/* composite(canvas_w, canvas_h, layer_info) -> Option<Vec<u8>>; `dst` = w*h*4 */
int pfx_composite(pfx_ctx* ctx, uint32_t w, uint32_t h, const pfx_layer_info* layers, uint32_t n_layers, uint8_t* dst);
/* composite_dirty_readback: composite, read back only (x, y, rw, rh) into the tight `dst_region` */
int pfx_composite_region(pfx_ctx* ctx, uint32_t w, uint32_t h, const pfx_layer_info* layers, uint32_t n_layers,
                         uint32_t x, uint32_t y, uint32_t rw, uint32_t rh, uint8_t* dst_region);
/* The tool preview layer (CanvasState::preview_layer + preview_blend_mode / preview_is_eraser / preview_replaces_layer,
 * ref: src/canvas/canvas_state.rs:541-548,556-560,593-658): while a stroke is in flight its pixels are folded into the ACTIVE
 * layer's pixel before that layer's mask, blend mode and opacity apply — replaced outright, used as an eraser mask, lerped by
 * coverage for Overwrite / Xor, or blended with the tool's mode.  The reference's wgpu compositor does not handle it (only
 * the CPU one does); here it rides on the same kernel.  `preview_pixels` is the preview flattened to w*h RGBA8;
 * `preview_chunk_present` (one byte per 64x64 chunk, row-major) tells which chunks the preview TiledImage holds — NULL means
 * "every chunk with a non-zero alpha", TiledImage::from_rgba_image's rule. */
typedef struct pfx_preview {
    uint32_t active_layer;   /* index into the pfx_layer_info array of the call (CanvasState::active_layer_index) */
    uint8_t  blend_mode;     /* BlendMode::to_u8 */
    uint8_t  is_eraser;
    uint8_t  replaces_layer;
    uint8_t  _pad;
} pfx_preview;
int pfx_composite_preview(pfx_ctx* ctx, uint32_t w, uint32_t h, const pfx_layer_info* layers, uint32_t n_layers,
                          const uint8_t* preview_pixels, const uint8_t* preview_chunk_present /* may be NULL */,
                          const pfx_preview* preview, uint8_t* dst);
/* one blend_pixel_static on the host-visible side of the ABI (kept for spot checks; runs a 1-pixel launch) */
int pfx_blend_pixels(pfx_ctx* ctx, const uint8_t* base, const uint8_t* top, uint8_t* dst, size_t n_pixels,
                     uint8_t blend_mode, float opacity);

/* ================= B3: warp pipelines ================= */
/* GpuLiquifyPipeline::warp_into (ref: src/gpu/compute/liquify.rs:176); numerics warp_displacement_full
 * (ref: src/ops/transform.rs:1288-1345).  Field and output are w*h; source is sw*sh. */
int pfx_warp_displacement(pfx_ctx* ctx, const uint8_t* src, uint32_t sw, uint32_t sh, const float* disp_xy,
                          uint32_t w, uint32_t h, uint8_t* dst);
/* The pipeline's source cache (ref: src/gpu/compute/liquify.rs:166-176): warp_into uploads the source texture once and reuses it
 * until invalidate_source; an interactive session then only sends displacement fields.  _cached fails with PFX_ERR_INVALID when
 * no source is set (or it was invalidated) and leaves dst untouched. */
int pfx_warp_set_source(pfx_ctx* ctx, const uint8_t* src, uint32_t sw, uint32_t sh);
int pfx_warp_invalidate_source(pfx_ctx* ctx);
int pfx_warp_displacement_cached(pfx_ctx* ctx, const float* disp_xy, uint32_t w, uint32_t h, uint8_t* dst);
/* generate_displacement_from_mesh (ref: src/ops/transform.rs:1670-1705); orig_pts may be NULL =>
 * generate_displacement_from_mesh_fast / GpuMeshWarpDisplacementPipeline::generate_displacement
 * (ref: src/ops/transform.rs:1712, src/gpu/compute/mesh_warp.rs:131) */
int pfx_mesh_displacement(pfx_ctx* ctx, const float* orig_pts_xy, const float* deformed_pts_xy, uint32_t cols,
                          uint32_t rows, uint32_t w, uint32_t h, float* disp_xy_out);
/* warp_mesh_catmull_rom (ref: src/ops/transform.rs:1743-1761): fused field + gather, no field in memory */
int pfx_warp_mesh_catmull_rom(pfx_ctx* ctx, const uint8_t* src, const float* orig_pts_xy, const float* deformed_pts_xy,
                              uint32_t cols, uint32_t rows, uint32_t w, uint32_t h, uint8_t* dst);
/* DisplacementField::apply_push/expand/contract/twirl (ref: src/ops/transform.rs:1051-1200): host-side scatter-add
 * exactly as in the reference (serial, glibc expf). mode: 0 push, 1 expand, 2 contract, 3 twirl cw, 4 twirl ccw */
void pfx_displacement_brush(float* disp_xy, uint32_t w, uint32_t h, int mode, float cx, float cy,
                            float delta_x, float delta_y, float radius, float strength);
/* the same brushes on a DEVICE-resident field (the Liquify interactive loop: dabs accumulate into the field that
 * pfx_warp_displacement_dev then samples; no field traffic over PCIe).  A dab list is applied in order.  The Gaussian
 * falloff's exp() is evaluated on the device: weights may differ from the CPU path in the last ulp (+-1 LSB class after
 * the warp). */
typedef struct pfx_disp_dab { int32_t mode; float cx, cy, delta_x, delta_y, radius, strength; } pfx_disp_dab;
int pfx_displacement_brushes_dev(pfx_ctx* ctx, void* disp_dev /* w*h*2 f32 */, uint32_t w, uint32_t h, const pfx_disp_dab* dabs, uint32_t n_dabs);

/* ================= brush stamp loop (ref: src/ui/panels/tools/behavior/raster/brush_render.rs) ================= */
typedef enum pfx_brush_mode { PFX_BRUSH_NORMAL = 0, PFX_BRUSH_DODGE = 1, PFX_BRUSH_BURN = 2, PFX_BRUSH_SPONGE = 3 } pfx_brush_mode;
typedef struct pfx_brush { /* the ToolProperties fields the circle-tip path reads (ref: state.rs:98-157) */
    float size, hardness, flow;
    float color[4];       /* straight RGBA in 0..1 (primary/secondary_color_f32) */
    int32_t anti_aliased;
    int32_t is_eraser;
    int32_t mode;         /* pfx_brush_mode */
} pfx_brush;
/* draw_circle_no_dirty for every point of `points_xy` in order (ref: brush_render.rs:135-400) into `target_inout` */
int pfx_brush_stamps(pfx_ctx* ctx, uint8_t* target_inout, uint32_t w, uint32_t h, const pfx_brush* brush,
                     const float* points_xy, uint32_t n_points, const uint8_t* selection);
/* draw_line_no_dirty (ref: brush_render.rs:762-835): dense 1-px stepping, then the stamp loop */
int pfx_brush_line(pfx_ctx* ctx, uint8_t* target_inout, uint32_t w, uint32_t h, const pfx_brush* brush,
                   float x0, float y0, float x1, float y1, const uint8_t* selection);
/* Brush dynamics — the remaining ToolProperties fields draw_circle_no_dirty reads (ref: state.rs:112-128, brush_render.rs:148-256,
 * 533-760) plus ToolsPanel::stamp_counter: per-stamp scatter, hue / brightness jitter (hashed from the stamp position), and image
 * brush tips with fixed or random rotation.  `tip_mask` is brush_tip_mask: the tip's coverage image already rescaled to the
 * brush size (pfx_brush_tip_rescale does what rebuild_tip_mask does, brush_render.rs:404-528); NULL = the round tip.
 * Image tips stamp with max-alpha or erase only (the reference ignores brush->mode for them). */
typedef struct pfx_brush_dynamics {
    float    scatter, hue_jitter, brightness_jitter;
    uint32_t stamp_counter;
    const uint8_t* tip_mask;      /* tip_mask_size^2 bytes (host memory), or NULL */
    uint32_t tip_mask_size;
    float    tip_rotation;        /* degrees */
    int32_t  tip_random_rotation;
    float    tip_rotation_lo, tip_rotation_hi; /* tip_rotation_range */
} pfx_brush_dynamics;
int pfx_brush_stamps_ex(pfx_ctx* ctx, uint8_t* target_inout, uint32_t w, uint32_t h, const pfx_brush* brush, const pfx_brush_dynamics* dyn /* may be NULL */,
                        const float* points_xy, uint32_t n_points, const uint8_t* selection);
int pfx_brush_line_ex(pfx_ctx* ctx, uint8_t* target_inout, uint32_t w, uint32_t h, const pfx_brush* brush, const pfx_brush_dynamics* dyn,
                      float x0, float y0, float x1, float y1, const uint8_t* selection);
/* rebuild_tip_mask (host side, like the reference): bilinear rescale of a square source mask to ceil(brush_size), hardness contrast,
 * anti-alias box passes.  `out` needs ceil(brush_size)^2 bytes; returns that side length (0 = no source). */
uint32_t pfx_brush_tip_rescale(const uint8_t* src_mask, uint32_t src_size, float brush_size, float hardness, uint8_t* out);
/* commit_bezier_to_layer / commit_eraser_to_layer (ref: bezier_commit.rs:103-225) */
int pfx_brush_commit(pfx_ctx* ctx, uint8_t* layer_inout, const uint8_t* preview, uint32_t w, uint32_t h,
                     uint8_t blend_mode, int is_eraser, const uint8_t* selection);

/* ================= A0: TiledImage import/export rule ================= */
/* from_rgba_image + to_rgba_image: chunks with no alpha read back as zeros (ref: tiled_image.rs:50-104,271-293) */
int pfx_tiled_roundtrip(pfx_ctx* ctx, const uint8_t* src, uint8_t* dst, uint32_t w, uint32_t h);
/* chunk_keys(): one byte per 64x64 chunk, row-major, 1 = populated */
int pfx_chunk_populated(pfx_ctx* ctx, const uint8_t* src, uint32_t w, uint32_t h, uint8_t* populated);

/* ================= device-resident tier (`_dev`): same kernels, caller-owned device memory, asynchronous ========= */
/* Aliasing: `src_dev == dst_dev` (in place) is accepted by the pointwise calls (pfx_adjust_dev, pfx_lut_apply-style ops) and by
 * pfx_gaussian_blur_dev / pfx_box_blur_dev, which then run their two-pass kernels through `tmp_dev` — for the Gaussian that is the
 * f32 path, so an in-place call can differ from an out-of-place one by the +-1 LSB of the default (MFMA) mode unless the context is
 * in exact mode.  Every other call that reads a neighbourhood or gathers (median, pixelate, warps, the effect bank) returns
 * PFX_ERR_INVALID when the two images overlap; partially overlapping buffers are always refused. */
/* pfx_flatten_dev: `dst_dev` may be one of the layers (the result replaces it: every pixel is written after its last read) but must not partially
 * overlap any. */
int pfx_flatten_dev(pfx_ctx* ctx, const void* const* layer_ptrs_dev, const void* const* mask_ptrs_dev /* may be NULL */,
                    const pfx_layer_info* layers, uint32_t n_layers, uint32_t w, uint32_t h, void* dst_dev);
int pfx_flatten_preview_dev(pfx_ctx* ctx, const void* const* layer_ptrs_dev, const void* const* mask_ptrs_dev, const pfx_layer_info* layers,
                            uint32_t n_layers, uint32_t w, uint32_t h, const void* preview_dev, const void* preview_chunk_present_dev /* may be NULL */,
                            const pfx_preview* preview, void* dst_dev);
/* `tmp_dev` = w*h*16 bytes of scratch for the f32 horizontal pass (ref: filters.rs:255 buf_h); NULL = context scratch */
int pfx_gaussian_blur_dev(pfx_ctx* ctx, const void* src_dev, void* dst_dev, uint32_t w, uint32_t h, float sigma,
                          void* tmp_dev);
/* the same on a BAND of a taller image (rows [first_row, first_row + h) of it, halo rows included): results equal, bit for bit,
 * the rows a whole-image call produces wherever the band holds the full +-ceil(3 sigma) neighbourhood (row-band sharding) */
int pfx_gaussian_blur_band_dev(pfx_ctx* ctx, const void* src_dev, void* dst_dev, uint32_t w, uint32_t h, float sigma,
                               void* tmp_dev, uint32_t first_row);
/* box blur / median of a band with its halo rows (ceil(radius) / max(radius, 1) of them on each side that is not an image edge): the
 * arithmetic is integer per pixel, so every row at least `radius` rows away from the buffer's first and last row equals the same row of
 * the whole image's filter bit for bit, wherever the band was cut; `first_row` is accepted for symmetry with the Gaussian and unused. */
int pfx_box_blur_band_dev(pfx_ctx* ctx, const void* src_dev, void* dst_dev, uint32_t w, uint32_t h, float radius, const void* mask_dev,
                          void* tmp_dev, uint32_t first_row);
int pfx_median_band_dev(pfx_ctx* ctx, const void* src_dev, void* dst_dev, uint32_t w, uint32_t h, uint32_t radius, const void* mask_dev,
                        uint32_t first_row);
int pfx_box_blur_dev(pfx_ctx* ctx, const void* src_dev, void* dst_dev, uint32_t w, uint32_t h, float radius,
                     const void* mask_dev, void* tmp_dev /* w*h*4 or NULL */);
int pfx_median_dev(pfx_ctx* ctx, const void* src_dev, void* dst_dev, uint32_t w, uint32_t h, uint32_t radius,
                   const void* mask_dev);
int pfx_pixelate_dev(pfx_ctx* ctx, const void* src_dev, void* dst_dev, uint32_t w, uint32_t h, uint32_t block_size,
                     const void* mask_dev);
int pfx_adjust_dev(pfx_ctx* ctx, const void* src_dev, void* dst_dev, uint32_t w, uint32_t h, int op,
                   const float* params, uint32_t n_params, const uint8_t* lut_host, const void* mask_dev, int sparse_mode);
int pfx_rhai_adjust_dev(pfx_ctx* ctx, void* pixels_dev, uint32_t w, uint32_t h, int op, const float* params,
                        uint32_t n_params);
/* Chains (round 6): several ops on a device-resident image in as few passes over memory as the kernels allow.  The result equals calling the single-op entry
 * points one after the other — pfx_gaussian_blur_dev / pfx_box_blur_dev (no selection) / pfx_adjust_dev (PFX_DENSE, no selection) / pfx_rhai_adjust_dev — bit for
 * bit, in the context's current Gaussian mode: every op still rounds to u8, only the trips through memory go.  A run of pointwise ops is one launch; a bit-exact
 * Gaussian of radius <= 16 followed by pointwise ops is one launch (the blurred image never exists in memory).  This is what a script's
 * `apply_gaussian_blur(4.0); apply_hsl(..); apply_invert();` (ref: src/ops/scripting.rs:869-1075 and :1095-1140, each call a full pass over the image on the CPU) and the batch
 * pipeline run through.  src_dev == dst_dev is allowed for chains without a blur. */
typedef enum pfx_chain_kind { PFX_CHAIN_ADJUST = 0 /* op = pfx_adjust_op */, PFX_CHAIN_RHAI = 1 /* op = pfx_rhai_op */, PFX_CHAIN_GAUSSIAN = 2 /* params[0] = sigma */,
                              PFX_CHAIN_BOX = 3 /* params[0] = radius */ } pfx_chain_kind;
typedef struct pfx_chain_op {
    int32_t  kind;          /* pfx_chain_kind */
    int32_t  op;            /* PFX_CHAIN_ADJUST / PFX_CHAIN_RHAI: the op id; otherwise ignored */
    uint32_t n_params;
    float    params[12];    /* as for the op's own entry point */
    const uint8_t* lut;     /* host, 1024 bytes: PFX_OP_GRADIENT_MAP / PFX_OP_LUT_RGBA; NULL otherwise */
} pfx_chain_op;
int pfx_chain_dev(pfx_ctx* ctx, const void* src_dev, void* dst_dev, uint32_t w, uint32_t h, const pfx_chain_op* ops, uint32_t n_ops);
int pfx_warp_displacement_dev(pfx_ctx* ctx, const void* src_dev, uint32_t sw, uint32_t sh, const void* disp_dev,
                              uint32_t w, uint32_t h, void* dst_dev);
int pfx_mesh_displacement_dev(pfx_ctx* ctx, const float* orig_pts_xy, const float* deformed_pts_xy, uint32_t cols,
                              uint32_t rows, uint32_t w, uint32_t h, void* disp_dev);
int pfx_warp_mesh_catmull_rom_dev(pfx_ctx* ctx, const void* src_dev, const float* orig_pts_xy,
                                  const float* deformed_pts_xy, uint32_t cols, uint32_t rows, uint32_t w, uint32_t h,
                                  void* dst_dev);
/* Band forms of the two warps for a document sharded by rows ("replicate the source, warp bands of the output"; the CPU path's
 * `par_chunks_mut(w * 4)` rows, ref: src/ops/transform.rs:1288-1345, 1687-1761): `dst_band_dev` / `disp_band_dev` hold rows [first_row, first_row +
 * band_rows) of the output / the field, the source is whole.  Bit-identical to the same rows of the whole-image call. */
int pfx_warp_displacement_band_dev(pfx_ctx* ctx, const void* src_dev, uint32_t sw, uint32_t sh, const void* disp_band_dev, uint32_t w,
                                   uint32_t band_rows, void* dst_band_dev, uint32_t first_row);
int pfx_warp_mesh_catmull_rom_band_dev(pfx_ctx* ctx, const void* src_dev, const float* orig_pts_xy, const float* deformed_pts_xy,
                                       uint32_t cols, uint32_t rows, uint32_t w, uint32_t h, void* dst_band_dev, uint32_t first_row,
                                       uint32_t band_rows);
int pfx_brush_stamps_dev(pfx_ctx* ctx, void* target_dev, uint32_t w, uint32_t h, const pfx_brush* brush,
                         const float* points_xy, uint32_t n_points, const void* selection_dev);
int pfx_brush_stamps_ex_dev(pfx_ctx* ctx, void* target_dev, uint32_t w, uint32_t h, const pfx_brush* brush, const pfx_brush_dynamics* dyn,
                            const float* points_xy, uint32_t n_points, const void* selection_dev);
int pfx_tiled_roundtrip_dev(pfx_ctx* ctx, const void* src_dev, void* dst_dev, uint32_t w, uint32_t h);
int pfx_sharpen_dev(pfx_ctx* ctx, const void* src_dev, void* dst_dev, uint32_t w, uint32_t h, float amount, float radius,
                    const void* mask_dev);
int pfx_glow_dev(pfx_ctx* ctx, const void* src_dev, void* dst_dev, uint32_t w, uint32_t h, float radius, float intensity,
                 const void* mask_dev);
int pfx_bokeh_blur_dev(pfx_ctx* ctx, const void* src_dev, void* dst_dev, uint32_t w, uint32_t h, float radius,
                       const void* mask_dev);
int pfx_motion_blur_dev(pfx_ctx* ctx, const void* src_dev, void* dst_dev, uint32_t w, uint32_t h, float angle_deg,
                        float distance, const void* mask_dev);
/* the rest of the effect bank on device-resident images (src_dev != dst_dev except for the purely pointwise ones) */
int pfx_zoom_blur_dev(pfx_ctx* ctx, const void* src_dev, void* dst_dev, uint32_t w, uint32_t h, float center_x, float center_y, float strength,
                      uint32_t samples, const float tint_color[4], float tint_strength, const void* mask_dev);
int pfx_crystallize_dev(pfx_ctx* ctx, const void* src_dev, void* dst_dev, uint32_t w, uint32_t h, float cell_size, uint32_t seed,
                        const void* mask_dev);
int pfx_dents_dev(pfx_ctx* ctx, const void* src_dev, void* dst_dev, uint32_t w, uint32_t h, float scale, float amount, uint32_t seed,
                  uint32_t octaves, float roughness, int pinch, int wrap, const void* mask_dev);
int pfx_bulge_dev(pfx_ctx* ctx, const void* src_dev, void* dst_dev, uint32_t w, uint32_t h, float amount, float origin_x, float origin_y,
                  const void* mask_dev);
int pfx_twist_dev(pfx_ctx* ctx, const void* src_dev, void* dst_dev, uint32_t w, uint32_t h, float angle_deg, float origin_x, float origin_y,
                  const void* mask_dev);
int pfx_add_noise_dev(pfx_ctx* ctx, const void* src_dev, void* dst_dev, uint32_t w, uint32_t h, float amount, int noise_type, int monochrome,
                      uint32_t seed, float scale, uint32_t octaves, const void* mask_dev);
int pfx_reduce_noise_dev(pfx_ctx* ctx, const void* src_dev, void* dst_dev, uint32_t w, uint32_t h, float strength, uint32_t radius,
                         const void* mask_dev);
int pfx_vignette_dev(pfx_ctx* ctx, const void* src_dev, void* dst_dev, uint32_t w, uint32_t h, float amount, float softness, const void* mask_dev);
int pfx_halftone_dev(pfx_ctx* ctx, const void* src_dev, void* dst_dev, uint32_t w, uint32_t h, float dot_size, float angle_deg, int shape,
                     const void* mask_dev);
int pfx_grid_dev(pfx_ctx* ctx, const void* src_dev, void* dst_dev, uint32_t w, uint32_t h, uint32_t cell_w, uint32_t cell_h, uint32_t line_width,
                 const uint8_t color[4], int style, float opacity, const void* mask_dev);
int pfx_canvas_border_dev(pfx_ctx* ctx, const void* src_dev, void* dst_dev, uint32_t w, uint32_t h, uint32_t width, const uint8_t color[4],
                          const void* mask_dev);
int pfx_shadow_dev(pfx_ctx* ctx, const void* src_dev, void* dst_dev, uint32_t w, uint32_t h, int32_t offset_x, int32_t offset_y, float blur_radius,
                   int widen_radius, const uint8_t color[4], float opacity, const void* mask_dev);
int pfx_outline_dev(pfx_ctx* ctx, const void* src_dev, void* dst_dev, uint32_t w, uint32_t h, uint32_t width, const uint8_t color[4], int mode,
                    int anti_alias, const void* mask_dev);
int pfx_pixel_drag_dev(pfx_ctx* ctx, const void* src_dev, void* dst_dev, uint32_t w, uint32_t h, uint32_t seed, float amount, uint32_t distance,
                       float direction, const void* mask_dev);
int pfx_rgb_displace_dev(pfx_ctx* ctx, const void* src_dev, void* dst_dev, uint32_t w, uint32_t h, int32_t r_dx, int32_t r_dy, int32_t g_dx,
                         int32_t g_dy, int32_t b_dx, int32_t b_dy, const void* mask_dev);
int pfx_ink_dev(pfx_ctx* ctx, const void* src_dev, void* dst_dev, uint32_t w, uint32_t h, float edge_strength, float threshold, const void* mask_dev);
int pfx_oil_painting_dev(pfx_ctx* ctx, const void* src_dev, void* dst_dev, uint32_t w, uint32_t h, uint32_t radius, uint32_t levels,
                         const void* mask_dev);
int pfx_color_filter_dev(pfx_ctx* ctx, const void* src_dev, void* dst_dev, uint32_t w, uint32_t h, const uint8_t filter_color[4], float intensity,
                         int mode, const void* mask_dev);
int pfx_contours_dev(pfx_ctx* ctx, const void* src_dev, void* dst_dev, uint32_t w, uint32_t h, float scale, float frequency, float line_width,
                     const uint8_t line_color[4], uint32_t seed, uint32_t octaves, float blend, const void* mask_dev);

/* device self-test: compares the compositor's shared-reciprocal division with the compiler's IEEE f32 divide on
 * n_millions*1e6 random operand pairs drawn from the kernel's operand range; *mismatches must come back 0 */
int pfx_selftest_division(pfx_ctx* ctx, uint64_t seed, uint32_t n_millions, uint64_t* mismatches);
/* the same comparison with the operand range given: random significands, numerator exponents num_exp_lo .. num_exp_hi (a quarter of the
 * numerators are 0), denominator exponents den_exp_lo .. den_exp_hi, all within -126 .. 127; n_millions in 1 .. 4096.  The library's
 * documented range is numerators 2^-100 .. 2^20 over denominators 2^-48 .. 2^20; reduce_noise divides integers up to 195075 (exponents
 * 0 .. 17) by its range divisor, exponents -10 .. 100. */
int pfx_selftest_division_range(pfx_ctx* ctx, uint64_t seed, uint32_t n_millions, int32_t num_exp_lo, int32_t num_exp_hi, int32_t den_exp_lo,
                                int32_t den_exp_hi, uint64_t* mismatches);
/* device self-test: the three-instruction round-and-pack (`v.round().clamp(0.0, 255.0) as u8` of every pointwise op, resampler, effect and
 * warp) against the step-by-step formula for ALL 2^32 f32 bit patterns; *mismatches must come back 0.  Signalling NaNs, which no
 * arithmetic instruction produces, are counted separately (they convert to 255 instead of 0). */
int pfx_selftest_round_pack(pfx_ctx* ctx, uint64_t* mismatches, uint64_t* signalling_nan_mismatches);

/* device self-test: the texture path's conversions the compositor relies on — a typed UNORM8 buffer store of RN(k / 255) writes the byte k and a
 * typed load of the byte k returns RN(k / 255), for all 256 k on every channel; *mismatches must come back 0 (the class-sorting compositor, which reads every
 * layer through these conversions, is only used on a device where they hold: checked once per context). */
int pfx_selftest_unorm_store(pfx_ctx* ctx, uint64_t* mismatches);

/* host-side: the f16 tap tables of the matrix-core Gaussian for `sigma` (radius 1 .. 80), as the library uploads them: three parts of 256 entries,
 * tap t at index 48 + t — [0] and [1] the two-piece split w * 256 = w1 + w2, [2] the single-piece table the default mode multiplies with (every weight
 * one f16, the table's sum nudged to the exact weights' sum).  *bias_split / *bias_single = 1024 * the tables' sums (the sample encoding's offset).
 * Returns the number of taps, or a negative PFX_ERR_* (diagnostics for tests/: the kernel's +-1 LSB bound rests on these tables). */
int pfx_gaussian_f16_tables(float sigma, uint16_t out_768[768], float* bias_split, float* bias_single);

/* development tuning knobs (kernel tile configurations); unknown keys return PFX_ERR_INVALID.  Results never change — except under "gauss_parts", which
 * selects among +-1 LSB class variants of the default-mode Gaussian (f16 pieces per weight / per horizontal result: 12 shipped, 22, 11).  The knobs that select among
 * kernel shapes of the compositor ("flatten_variant", "dle_*") are process-wide (one setting for every context), the rest per context. */
int pfx_tune(pfx_ctx* ctx, const char* key, int value);
/* work counters of the compositor's dead-layer elimination since the last reset (diagnostics for profiles/ and the tests; the call
 * synchronises the device): out[0] compacted rounds, [1] pixels in them, [2] sum of layers over rounds, [3] natural 192-pixel units,
 * [4] sum of layers over natural units, [5] candidate alpha reads (units), [6] units that used the queue, [7] reserved */
int pfx_flatten_stats(pfx_ctx* ctx, uint64_t out[8], int reset);
/* diagnostic build of the class-sorting compositor (pfx_tune "dle_stats" = 4; results stay bit-exact, the launch is slower): wave clocks (s_memtime) summed over
 * the waves of the launches since the last reset — out[0] wave lifetimes, [1] waves, [8] classification, [9] deal + early passes, [10] natural passes,
 * [11] lane order + store, [12] / [13] waiting for layer pixels / blending in the early passes, [14] / [15] the same in the natural passes.  The stand-in for an
 * instruction-level thread trace: rocprofv3 --att needs the rocprof-trace-decoder library, which this image does not hold (profiles/r05_tuning.md) */
int pfx_flatten_trace(pfx_ctx* ctx, uint64_t out[16], int reset);

/* per-launch timing of the most recent `_dev` call family, measured with HIP events on the context stream
 * (used by bench.py for the roofline line).  Enable, run, then read the accumulated milliseconds / launches. */
int pfx_timing_enable(pfx_ctx* ctx, int on);
int pfx_timing_read(pfx_ctx* ctx, const char* kernel_name, double* total_ms, uint64_t* launches);
int pfx_timing_reset(pfx_ctx* ctx);

/* ---- resize_image: imageops::resize(&flat, new_w, new_h, filter) per layer (ref: src/ops/transform.rs:347-359; script
 * function resize_image src/ops/scripting.rs:749-770).  Filters = ScriptFilterType (scripting.rs:22-37): Nearest, Bilinear
 * (Triangle), Bicubic (CatmullRom), Lanczos (Lanczos3).  The resampling algorithm is the `image` crate's (0.25.9), restated;
 * nearest / bilinear / lanczos3 are pinned by the reference's goldens, bicubic is unpinned.  Bit-exact class. */
enum { PFX_RESIZE_NEAREST = 0, PFX_RESIZE_BILINEAR = 1, PFX_RESIZE_BICUBIC = 2, PFX_RESIZE_LANCZOS3 = 3 };
int pfx_resize_image(pfx_ctx* ctx, const uint8_t* src, uint32_t w, uint32_t h, uint8_t* dst /* new_w*new_h*4 */, uint32_t new_w, uint32_t new_h,
                     int filter);
int pfx_resize_image_dev(pfx_ctx* ctx, const void* src_dev, uint32_t w, uint32_t h, void* dst_dev, uint32_t new_w, uint32_t new_h, int filter);
/* apply_affine / affine_transform_layer(state, idx, rotation_z, rotation_x, rotation_y, scale, offset) (ref: src/ops/transform.rs:750-946):
 * Rz*Ry*Rx homography about the canvas centre (angles in degrees), inverse-mapped; PFX_RESIZE_BILINEAR (the layer transform's
 * mode, against a transparent outside) or PFX_RESIZE_NEAREST.  dst is canvas_w x canvas_h; unmapped pixels are (0,0,0,0). */
int pfx_affine_transform(pfx_ctx* ctx, const uint8_t* src, uint32_t src_w, uint32_t src_h, uint8_t* dst, uint32_t canvas_w, uint32_t canvas_h,
                         float rotation_z, float rotation_x, float rotation_y, float scale, float offset_x, float offset_y, int interpolation);
int pfx_affine_transform_dev(pfx_ctx* ctx, const void* src_dev, uint32_t src_w, uint32_t src_h, void* dst_dev, uint32_t canvas_w, uint32_t canvas_h,
                             float rotation_z, float rotation_x, float rotation_y, float scale, float offset_x, float offset_y, int interpolation);

/* ================= B5/B6: script front-end and CLI (ref: src/ops/scripting.rs:1733-1821, src/cli.rs) ================= */
typedef struct pfx_script_result {
    char     error[512];      /* ScriptError::friendly_message-style text, empty on success */
    int32_t  error_line;      /* 1-based, 0 if unknown */
    int32_t  error_col;
    uint32_t ops_executed;
    char     console[2048];   /* print_line output, '\n' separated (truncated) */
} pfx_script_result;
/* execute_script_sync(source, pixels, w, h, mask) (ref: scripting.rs:1733-1821).  The script language is the Rhai subset of
 * paintfe_amd/csrc/pfx_rhai.h (let / if / loops / fn / closures, strict i64-f64 typing, checked integer arithmetic); the
 * registered host API keeps the reference's names, arity and numeric flavour (scripting.rs:323-1482).  Bulk work runs on
 * the device: effects through the kernels above, per-pixel closures (map_channels / for_each_pixel / for_region) compiled
 * to a bytecode kernel; get_pixel / set_pixel touch a host mirror of the image.  Constructs outside the subset
 * return PFX_ERR_UNSUPPORTED.  Pixels are untouched on error. */
/* fixed-size form: the script must leave the image size unchanged (PFX_ERR_UNSUPPORTED otherwise) */
int pfx_script_run(pfx_ctx* ctx, const char* source, uint8_t* pixels_inout, uint32_t w, uint32_t h,
                   const uint8_t* mask, pfx_script_result* result);
/* CanvasOpRequest (ref: scripting.rs:41-58): canvas-wide transforms the caller replays on its other layers */
enum { PFX_CANVAS_FLIP_HORIZONTAL = 0, PFX_CANVAS_FLIP_VERTICAL = 1, PFX_CANVAS_ROTATE_90CW = 2, PFX_CANVAS_ROTATE_90CCW = 3,
       PFX_CANVAS_ROTATE_180 = 4, PFX_CANVAS_RESIZE_IMAGE = 5, PFX_CANVAS_RESIZE_CANVAS = 6 };
typedef struct pfx_canvas_op {
    int32_t  kind;           /* PFX_CANVAS_* */
    uint32_t w, h;           /* RESIZE_IMAGE / RESIZE_CANVAS: new size */
    uint32_t anchor_x, anchor_y; /* RESIZE_CANVAS: 0 / 1 / 2 per axis (parse_anchor, scripting.rs:69-82); RESIZE_IMAGE: anchor_x = PFX_RESIZE_* filter */
} pfx_canvas_op;
/* the same canvas-wide transforms applied to one layer image, for replaying a pfx_canvas_op list on the other layers
 * (ref: apply_canvas_ops, scripting.rs:1640-1723; ops::transform::flip_canvas_* / rotate_canvas_* / resize_canvas, transform.rs:382-424).
 * op = PFX_CANVAS_FLIP_HORIZONTAL .. PFX_CANVAS_ROTATE_180; 90-degree rotations swap the output's width and height. */
int pfx_flip_rotate(pfx_ctx* ctx, const uint8_t* src, uint32_t w, uint32_t h, uint8_t* dst, int op);
int pfx_flip_rotate_dev(pfx_ctx* ctx, const void* src_dev, uint32_t w, uint32_t h, void* dst_dev, int op);
/* anchor 0 / 1 / 2 per axis; fill = colour of the new area (NULL = transparent) */
int pfx_resize_canvas(pfx_ctx* ctx, const uint8_t* src, uint32_t w, uint32_t h, uint8_t* dst /* new_w*new_h*4 */, uint32_t new_w, uint32_t new_h,
                      uint32_t anchor_x, uint32_t anchor_y, const uint8_t fill[4]);
int pfx_resize_canvas_dev(pfx_ctx* ctx, const void* src_dev, uint32_t w, uint32_t h, void* dst_dev, uint32_t new_w, uint32_t new_h, uint32_t anchor_x,
                          uint32_t anchor_y, const uint8_t fill[4]);
/* full form: returns (result_pixels, final_w, final_h, console_output, canvas_ops) like the reference.  *out is an opaque
 * result owned by the library until pfx_script_output_free; NULL on error. */
typedef struct pfx_script_output pfx_script_output;
int pfx_script_execute(pfx_ctx* ctx, const char* source, const uint8_t* pixels, uint32_t w, uint32_t h, const uint8_t* mask,
                       pfx_script_output** out, pfx_script_result* result);
const uint8_t* pfx_script_output_pixels(const pfx_script_output* out, uint32_t* w, uint32_t* h);
uint32_t    pfx_script_output_console_lines(const pfx_script_output* out);
const char* pfx_script_output_console_line(const pfx_script_output* out, uint32_t index);
uint32_t    pfx_script_output_canvas_ops(const pfx_script_output* out, pfx_canvas_op* ops, uint32_t capacity); /* returns the count */
void        pfx_script_output_free(pfx_script_output* out);
/* language-only evaluation (no device, no image functions): syntax / typing / console checks, e.g. from an editor's
 * "compile" button (ref: compile_script, scripting.rs:1489-1508).  ctx may be NULL. */
int pfx_script_check(const char* source, uint32_t w, uint32_t h, pfx_script_result* result);
/* the `pfx` batch CLI main (same flags as src/cli.rs:43-89); returns the process exit code */
int pfx_cli_main(int argc, char** argv);
/* the CLI's PNG reader on a buffer (ref: load_image_sync -> image::open(..) -> to_rgba8, src/io.rs:693-723, called from src/cli.rs:234): every colour type and bit depth, Adam7, tRNS.
 * *rgba_out is malloc'd w*h*4 bytes, released with pfx_png_free.  Malformed input -> PFX_ERR_INVALID + message; never reads or allocates beyond what
 * the IDAT data can inflate to.  No device needed. */
int  pfx_png_decode_mem(const uint8_t* bytes, size_t n_bytes, uint8_t** rgba_out, uint32_t* w_out, uint32_t* h_out, char* err, size_t err_cap);
void pfx_png_free(uint8_t* rgba);

/* ================= N2: PFE project files and TiledImage import / export on the device =====================================
 * A .pfe file is the bincode 1.x (little-endian, fixed-width integers, u64 lengths) image of ProjectFileV0..V3
 * (ref: src/io.rs:85-208): the layer stack the compositor wants, each raster layer stored as its sparse list of 64x64 chunks.
 * pfx_project is the host-side document: size, active layer, folders, layers (name, visibility, opacity, blend mode, kind,
 * chunk list, and every V2/V3 payload kept verbatim so that re-saving loses nothing).  Parity: no .pfe fixture exists in the
 * reference tree (its tests are save->load round trips), so the byte layout is pinned by an independent Python bincode
 * restatement under tests/ — "parity unpinned" against real reference output. */
typedef struct pfx_project pfx_project;
typedef struct pfx_project_layer {
    const char* name;                /* owned by the project, valid until it is modified or freed */
    uint8_t  visible;                /* Layer::visible */
    uint8_t  effectively_visible;    /* visible and not inside a hidden folder (ref: canvas_state.rs:216-227) */
    uint8_t  blend_mode;             /* BlendMode::to_u8 as stored */
    uint8_t  layer_type;             /* 0 raster, 1 text (its rasterised chunks are used), 2 adjustment */
    float    opacity;
    int64_t  folder_id;              /* -1 = none */
    uint32_t n_chunks;               /* stored chunks */
    uint8_t  kind;                   /* pfx_layer_kind the compositor will use (an adjustment payload that fails to parse
                                        falls back to raster, io.rs:864-869) */
    uint8_t  _pad[3];
    float    adj[16];                /* parameters as in pfx_layer_info.adj */
} pfx_project_layer;

/* load_pfe_from_bytes (ref: io.rs:477-499; V3 :813, V2 :957, V1 :1110, V0 :1233): NULL + message in err on malformed input,
 * zero / oversized dimensions (validate_open_dimensions, :505), more than 256 layers, wrong chunk sizes, no layers */
pfx_project* pfx_project_load(const uint8_t* bytes, size_t n_bytes, char* err, size_t err_cap);
pfx_project* pfx_project_load_file(const char* path, char* err, size_t err_cap);
/* CanvasState::new-like empty document (no layers yet) */
pfx_project* pfx_project_new(uint32_t w, uint32_t h);
void     pfx_project_free(pfx_project* p);
uint32_t pfx_project_width(const pfx_project* p);
uint32_t pfx_project_height(const pfx_project* p);
uint32_t pfx_project_layer_count(const pfx_project* p);
uint32_t pfx_project_active_layer(const pfx_project* p);
int      pfx_project_version(const pfx_project* p);      /* 0..3: the version it was loaded from (new documents: 1) */
int      pfx_project_layer_get(const pfx_project* p, uint32_t index, pfx_project_layer* out);
/* Layer::pixels.to_rgba_image(): the layer flattened to w*h*4 on the host (missing chunks = zeros) */
int      pfx_project_layer_pixels(const pfx_project* p, uint32_t index, uint8_t* dst);
/* append a layer; rgba (w*h*4) is tiled with from_rgba_image's rule (all-transparent chunks dropped); rgba NULL = empty layer.
 * kind != PFX_LAYER_RASTER appends an adjustment layer with parameters adj[] (document becomes V3 on save). */
int      pfx_project_add_layer(pfx_project* p, const char* name, const uint8_t* rgba, float opacity, uint8_t blend_mode, uint8_t visible,
                               uint8_t kind, const float* adj);
int      pfx_project_set_active_layer(pfx_project* p, uint32_t index);
int      pfx_project_set_layer_folder(pfx_project* p, uint32_t index, int64_t folder_id /* -1 = none */);
int      pfx_project_add_folder(pfx_project* p, uint64_t id, const char* name, uint8_t visible);
/* replace a layer's pixels (and the document size when new_w/new_h differ is NOT changed: use pfx_project_resize) */
int      pfx_project_set_layer_pixels(pfx_project* p, uint32_t index, const uint8_t* rgba);
/* build_pfe + bincode::serialize (ref: io.rs:254-282): V3 if any folder / adjustment layer / experimental payload, V2 if any
 * text layer, else V1; chunks are written in row-major (cy, cx) order.  *bytes_out is malloc'ed: release with pfx_bytes_free. */
int      pfx_project_save(const pfx_project* p, uint8_t** bytes_out, size_t* n_out);
int      pfx_project_save_file(const pfx_project* p, const char* path);
void     pfx_bytes_free(uint8_t* bytes);
/* CanvasState::composite() of the document (ref: canvas_state.rs:482-698) on the device: only the stored chunks cross PCIe, a
 * kernel scatters them into flat layers (TiledImage import), then the compositor runs.  dst = w*h*4 */
int      pfx_project_composite(pfx_ctx* ctx, const pfx_project* p, uint8_t* dst);
int      pfx_project_composite_dev(pfx_ctx* ctx, const pfx_project* p, void* dst_dev);
/* run_one's script step (ref: cli.rs:238-270): the script runs on the active layer, its canvas ops are replayed on every other
 * layer (apply_canvas_ops, scripting.rs:1640-1723) and the document size follows */
int      pfx_project_run_script(pfx_ctx* ctx, pfx_project* p, const char* source, pfx_script_result* result);

/* TiledImage <-> flat image on the device.  packed = n stored chunks of 64*64*4 bytes (edge chunks zero-padded), slot[c] for
 * chunk c = cy * ceil(w/64) + cx is the chunk's index in `packed` or 0xffffffff when the TiledImage has no such chunk.
 * import = to_rgba_image (ref: tiled_image.rs:271-293), export = from_rgba_image given the populated set (:50-104). */
#define PFX_NO_CHUNK 0xffffffffu
int pfx_tiled_import_dev(pfx_ctx* ctx, const void* packed_dev, const uint32_t* slot_host, uint32_t w, uint32_t h, void* flat_dev);
int pfx_tiled_export_dev(pfx_ctx* ctx, const void* flat_dev, uint32_t w, uint32_t h, const uint32_t* slot_host, void* packed_dev);

/* ================= multi-GPU: one document across the GPUs of a node =================
 * The reference has no multi-device layer.  Its unit of independence is the 64x64 TiledImage chunk: the compositor is
 * `populated_chunks.par_iter()` (ref: src/canvas/canvas_state.rs:565), filters are row-parallel (ref: src/ops/filters.rs:258-313),
 * and one level up the CLI loops over independent files (ref: src/cli.rs:159-216).  A pfx_group maps that onto N HIP devices driven
 * by ONE process: a document is cut into bands of whole chunk rows, member k keeps its band of every layer resident, flatten needs
 * no communication, the Gaussian pulls ceil(3 sigma) rows of the flattened u8 neighbours' bands over xGMI (peer-to-peer copies
 * ordered by events), and an optional all-gather leaves the whole result on every member.  All work is asynchronous on the
 * members' streams.  Results are bit-identical to the single-GPU calls on the whole document. */
typedef struct pfx_group pfx_group;
/* rows [y0, y1) of `rank`'s band of an h-row image cut for `world` members: whole chunk rows, remainder to the first members */
void        pfx_band_rows(uint32_t h, uint32_t world, uint32_t rank, uint32_t* y0, uint32_t* y1);
/* one context per entry of `devices` (the same device may appear more than once: a 1-GPU box can exercise the whole path) */
int         pfx_group_create(const int* devices, uint32_t n, pfx_group** out);
void        pfx_group_destroy(pfx_group* g);
uint32_t    pfx_group_size(const pfx_group* g);
pfx_ctx*    pfx_group_ctx(pfx_group* g, uint32_t rank);
const char* pfx_group_last_error(const pfx_group* g);   /* never NULL */
/* allocate the members' bands for a w x h document of n_layers raster layers */
int         pfx_group_set_document(pfx_group* g, uint32_t w, uint32_t h, uint32_t n_layers);
int         pfx_group_band(const pfx_group* g, uint32_t rank, uint32_t* y0, uint32_t* y1);
/* scatter one full-size host layer (w*h*4) to the members' bands; blocking */
int         pfx_group_upload_layer(pfx_group* g, uint32_t index, const uint8_t* rgba_host);
/* device pointer of member `rank`'s band of layer `index` ((y1-y0)*w*4 bytes), for producers that already live on the device */
void*       pfx_group_layer_band_dev(pfx_group* g, uint32_t rank, uint32_t index);
/* CanvasState::composite() of the document followed by parallel_gaussian_blur(sigma) (sigma <= 0: flatten only).
 * layers[k].layer_idx indexes the document's layers.  all_gather != 0: afterwards every member holds the whole result. */
int         pfx_group_flatten_blur(pfx_group* g, const pfx_layer_info* layers, uint32_t n_layers, float sigma, int all_gather);
/* the same with any of the band filters behind the flatten (the Gaussian, box and median vertical passes need halo rows):
 * PFX_BAND_GAUSSIAN param = sigma (halo ceil(3 sigma)); PFX_BAND_BOX param = radius (halo ceil(radius), ref: blur.rs:233-318);
 * PFX_BAND_MEDIAN param = radius (halo max(radius, 1), ref: noise.rs:357-410); PFX_BAND_NONE = flatten only */
enum { PFX_BAND_NONE = 0, PFX_BAND_GAUSSIAN = 1, PFX_BAND_BOX = 2, PFX_BAND_MEDIAN = 3 };
int         pfx_group_flatten_filter(pfx_group* g, const pfx_layer_info* layers, uint32_t n_layers, int filter, float param, int all_gather);
/* how halo rows and gathered bands travel between the members.  PFX_GROUP_PEER (default): hipMemcpyPeerAsync over xGMI, pair by pair
 * replaced by staged copies where peer access cannot be enabled; PFX_GROUP_STAGED: always through pinned host memory;
 * PFX_GROUP_RCCL: one ncclSend / ncclRecv group for the halos and one ncclBroadcast group (one broadcast per ragged band) for the
 * all-gather — librccl is loaded with dlopen on first use (PFX_ERR_UNSUPPORTED if it is missing or two members share a device).
 * Results are identical under every transport. */
enum { PFX_GROUP_PEER = 0, PFX_GROUP_RCCL = 1, PFX_GROUP_STAGED = 2 };
int         pfx_group_set_transport(pfx_group* g, int transport);
int         pfx_group_transport(const pfx_group* g);
int         pfx_group_synchronize(pfx_group* g);
/* Watchdog: the next `calls` pipeline calls (0xFFFFFFFF: all) end with a host-side wait of at most `timeout_ms` for every member's streams; a member
 * that does not finish turns a hang (a mis-paired RCCL group, a peer that never sends) into PFX_ERR_HIP whose message names the busy members and the
 * halo transfers (consumer <- producer, rows) they take part in.  An RCCL transport that times out has its communicators aborted and is replaced by
 * PEER.  timeout_ms == 0 switches it off.  Selecting PFX_GROUP_RCCL arms it for the first two calls (20 s) unless it was configured before. */
int         pfx_group_set_watchdog(pfx_group* g, uint32_t timeout_ms, uint32_t calls);
int         pfx_group_synchronize_timeout(pfx_group* g, uint32_t timeout_ms); /* pfx_group_synchronize with the same bounded wait and report */
/* Per-phase clocks of the pipeline calls (off by default): with timing on, every member records HIP events around its phases, and pfx_group_phase_ms returns
 * for member `rank` of the LAST call (it waits for that member's work): out_ms[0] flatten, [1] from the end of its flatten to the arrival of its last halo row
 * (waiting for the neighbours' flattens + the transfer), [2] the band filter, [3] its all-gather pushes (0 without all_gather).  What a first run on a real
 * multi-GPU node should print beside the step time (bench.py --gpus N: "c_abi_group"). */
int         pfx_group_set_phase_timing(pfx_group* g, int on);
int         pfx_group_phase_ms(pfx_group* g, uint32_t rank, double out_ms[4]);
/* Warps of the sharded document ("replicate the source, warp bands of the output"; ref: src/ops/transform.rs:1288-1345, 1687-1761): the
 * flattened bands are all-gathered so that every member holds the whole source, then every member warps its band of the output with
 * pfx_warp_displacement_band_dev (`disp_host` = w*h xy pairs, scattered to the members by rows; blocking until the field has been copied) or
 * pfx_warp_mesh_catmull_rom_band_dev.  The result stays sharded (pfx_group_result_band_dev / pfx_group_download); bit-identical to the single-GPU calls. */
int         pfx_group_flatten_warp_displacement(pfx_group* g, const pfx_layer_info* layers, uint32_t n_layers, const float* disp_host);
int         pfx_group_flatten_warp_mesh(pfx_group* g, const pfx_layer_info* layers, uint32_t n_layers, const float* orig_pts_xy /* may be NULL */,
                                        const float* deformed_pts_xy, uint32_t cols, uint32_t rows);
void*       pfx_group_result_band_dev(pfx_group* g, uint32_t rank);  /* rows [y0, y1) of the last result on member `rank` */
void*       pfx_group_gathered_dev(pfx_group* g, uint32_t rank);     /* w*h*4 on member `rank` after an all_gather call */
int         pfx_group_download(pfx_group* g, uint8_t* dst_host);     /* concatenated bands -> host w*h*4; blocking */

/* ================= batch of independent images across the GPUs of a node (BASELINE config 5; ref: src/cli.rs:159-216) =========
 * The reference's CLI runs `run_one` per input file, serially.  pfx_batch_pipeline streams a batch through the devices instead:
 * image i goes to device i mod n_devices (no data-path collective), and on every device a ring of `slots` buffer sets keeps the
 * upload of one image, the kernels of another and the download of a third in flight (pinned host memory; one in-order stream each
 * for uploads, kernels and downloads, chained by events).  Per image:
 * parallel_gaussian_blur(sigma) -> hue_saturation_lightness(hue, saturation, lightness) -> CanvasState::composite() of the result
 * under `n_overlays` overlay layers (resident on every device).  Sources are taken round-robin from a pool of host images
 * (image i = pool[i mod n_pool]; the pool is pinned for the duration of the call); results of the images listed in keep_indices
 * are copied to keep_out[k] (w*h*4 each) — the rest only cross PCIe. */
typedef struct pfx_batch_params {
    uint32_t w, h;
    float    sigma;
    float    hue, saturation, lightness;
    uint32_t n_overlays;                  /* <= 8 */
    const uint8_t* const* overlays_host;  /* n_overlays x w*h*4 */
    const uint8_t* overlay_modes;         /* BlendMode::to_u8 per overlay */
    const float*   overlay_opacity;       /* NULL = 1.0 */
    uint32_t slots;                       /* buffer sets per device, 2..8 (0 = 3: measured best; more sets let the upload queue run ahead and the rate drops) */
    uint32_t n_keep;
    const uint32_t* keep_indices;
    uint8_t* const* keep_out;
    uint32_t out_of_contract_fast_gaussian; /* 0 (default) = the bit-exact f32 Gaussian: every result equals the CPU path exactly.  1 leaves the +-1 LSB contract: the
                                             default-mode Gaussian (f16 taps, +-1 LSB) feeds HSL, which amplifies it — up to 4 LSB in the result (measured); a
                                             development / comparison switch, never a production setting (the stream is PCIe-bound either way) */
} pfx_batch_params;
typedef struct pfx_batch_stats {
    double   seconds;              /* first enqueue .. last result back on the host, slowest device */
    double   images_per_s;         /* whole job */
    double   h2d_gbs, d2h_gbs;     /* whole job, each direction */
    double   kernel_ms_per_image;  /* blur + HSL + flatten on resident data (HIP events on every 8th image) */
    uint32_t images, devices;
} pfx_batch_stats;
int pfx_batch_pipeline(const int* devices, uint32_t n_devices, uint32_t n_images, const pfx_batch_params* params,
                       const uint8_t* const* image_pool_host, uint32_t n_pool, pfx_batch_stats* stats, char* err, size_t err_cap);

/* ================= shape tool: the 17 built-in SDF shapes (ref: src/ops/shapes.rs:1169-1305 rasterize_shape) =================
 * A pure per-pixel map over the shape's bounding box: the signed distance at the pixel centre (shape_sdf, :827), a smoothstep coverage, the fill / outline /
 * both colour mix.  Everything that is uniform over the image (rotation, angles, vertex lists, the heart's path) is computed on the host with the host libm, as
 * the reference does.  Bit-exact class, except pentagon, hexagon, octagon, star5 and star6, which evaluate atan2 / cos / sin per pixel: +-1 LSB class (the f64
 * routine rounded once, like pfx_twist_core).  The reference's 20 shape goldens are reproduced with tolerance 0.
 * Custom path shapes (PlacedShape::custom_shape_data — polylines with 4-sample supersampling, :1065-1163) have their own section below: pfx_custom_shape_*.
 * The struct is always passed by pointer.  kind >= PFX_SHAPE_COUNT, fill_mode > PFX_SHAPE_BOTH or a non-finite cx / cy / hw / hh / rotation (the reference's
 * `as i32` would saturate the box to the whole canvas) return PFX_ERR_INVALID. */
typedef enum pfx_shape_kind { /* ShapeKind's declaration order, shapes.rs:159-178 */
    PFX_SHAPE_ELLIPSE = 0, PFX_SHAPE_RECTANGLE, PFX_SHAPE_ROUNDED_RECT, PFX_SHAPE_TRAPEZOID, PFX_SHAPE_PARALLELOGRAM,
    PFX_SHAPE_TRIANGLE, PFX_SHAPE_RIGHT_TRIANGLE, PFX_SHAPE_PENTAGON, PFX_SHAPE_HEXAGON, PFX_SHAPE_OCTAGON, PFX_SHAPE_CROSS,
    PFX_SHAPE_CHECK, PFX_SHAPE_HEART, PFX_SHAPE_DIAMOND, PFX_SHAPE_STAR5, PFX_SHAPE_STAR6, PFX_SHAPE_ARROW, PFX_SHAPE_COUNT
} pfx_shape_kind;
typedef enum pfx_shape_fill { PFX_SHAPE_OUTLINE = 0, PFX_SHAPE_FILLED, PFX_SHAPE_BOTH } pfx_shape_fill; /* ShapeFillMode, shapes.rs:268-272 */
typedef struct pfx_shape {          /* PlacedShape, shapes.rs:322 — the fields the rasteriser reads */
    float cx, cy, hw, hh, rotation, outline_width, corner_radius;
    uint8_t primary[4], secondary[4];
    uint8_t kind, fill_mode, anti_alias, _pad;
} pfx_shape;
/* the rasteriser's bounding box (:1175-1207): rotated corners of shape_local_corners, padded by 2, floor / ceil, clamped to the canvas.
 * box = x0, y0, bw, bh; an empty box is 0, 0, 0, 0 and PFX_OK.  Host only, no context. */
int pfx_shape_bounds(const pfx_shape* shape, uint32_t canvas_w, uint32_t canvas_h, int32_t box[4]);
/* the reference's `buf` over that box, bit for bit (box_rgba = bw*bh*4 bytes): pixels with coverage <= 0.001 are zero, pixels whose alpha rounds to 0 keep
 * their colour bytes.  An empty box returns PFX_OK and leaves the buffer untouched. */
int pfx_shape_rasterize(pfx_ctx* ctx, const pfx_shape* shape, uint32_t canvas_w, uint32_t canvas_h, uint8_t* box_rgba);
int pfx_shape_rasterize_dev(pfx_ctx* ctx, const pfx_shape* shape, uint32_t canvas_w, uint32_t canvas_h, void* box_dev);
/* the whole canvas (canvas_w*canvas_h*4, every byte written): zero outside the box, inside it the box pixels with a > 0 — the tool's preview layer
 * (ref: src/ui/panels/tools/behavior/advanced.rs:979-1021; tests/visual_shapes.rs:18-41 rasterize_to_canvas), the form pfx_composite_preview takes */
int pfx_shape_preview(pfx_ctx* ctx, const pfx_shape* shape, uint32_t canvas_w, uint32_t canvas_h, uint8_t* canvas_rgba);
int pfx_shape_preview_dev(pfx_ctx* ctx, const pfx_shape* shape, uint32_t canvas_w, uint32_t canvas_h, void* canvas_dev);
/* rasterise and commit in one kernel over the box, no intermediate buffer (advanced.rs:1054 onward): equals pfx_shape_preview followed by pfx_brush_commit with
 * the same blend mode and selection (canvas_w*canvas_h bytes or NULL).  Layer pixels outside the box are neither read nor written. */
int pfx_shape_draw_dev(pfx_ctx* ctx, void* layer_dev, uint32_t canvas_w, uint32_t canvas_h, const pfx_shape* shape, uint8_t blend_mode,
                       const void* selection_dev /* may be NULL */);

/* ================= shape tool: custom path shapes (ref: src/ops/shapes.rs:1065-1163, the custom branch of rasterize_shape :1241-1248) =================
 * A PlacedShape with custom_shape_data: per pixel four sub-samples at (+-0.25, +-0.25); each sample is mapped into the path's bounds, tested for crossing parity
 * over every segment of every polyline (even-odd fill) and, in Outline and Both mode, for its distance to the nearest segment against max(outline_width, 1).
 * Coverage is the count of samples times 0.25; the colour is `primary` in all three fill modes.  `+ - * /`, sqrt and comparisons only: bit-exact class.  The
 * reference has no golden of these functions; the yardstick is tests/customshape_model.py, itself held to a scalar transcription and hand-derived answers.
 * Of pfx_shape, `secondary`, `anti_alias` and `corner_radius` are ignored, and `kind` is used for the bounding box alone (the reference leaves the previously
 * selected built-in kind in PlacedShape::kind, and shape_local_corners reads it): the box is pfx_shape_bounds, unchanged.
 * The path is HOST memory in every tier, `_dev` calls included: polylines in, pixels out.  It is flattened to segments, checked and staged into context scratch
 * once per call; nothing is cached between calls.  A polyline of 0 or 1 points contributes no segment; a path without any segment is accepted and draws nothing.
 * PFX_ERR_INVALID, with the output untouched: a NULL pointer, a non-finite point or bound, more than PFX_CUSTOM_SHAPE_MAX_SEGMENTS segments, what
 * pfx_shape_bounds refuses (kind, fill_mode > PFX_SHAPE_BOTH, non-finite cx / cy / hw / hh / rotation), a non-finite outline_width, an icon size of 0 or above 1024.
 * Out of scope: extract_svg_path_data / parse_custom_shape (:27-120: kurbo's BezPath::from_svg and flatten, a third-party crate whose flattening cannot be
 * pinned here), the texture upload of the icon, the picker UI. */
typedef struct pfx_custom_path {          /* CustomShapeRenderData, shapes.rs:13 */
    const float*    points_xy;            /* every polyline's points, x y interleaved, host memory */
    const uint32_t* polyline_points;      /* points per polyline */
    uint32_t        n_polylines;
    float           bounds[4];            /* min_x, min_y, max_x, max_y */
} pfx_custom_path;
#define PFX_CUSTOM_SHAPE_MAX_SEGMENTS 65536u
/* host only, no context: windows(2) of every polyline, in order, as x1 y1 x2 y2 (what the kernel reads).  *n_segments is the path's count; seg_xyxy may be NULL
 * with cap 0 to ask for the count alone.  PFX_ERR_INVALID for a refused path (above) or a count above cap. */
int pfx_custom_shape_segments(const pfx_custom_path* path, float* seg_xyxy, uint32_t cap, uint32_t* n_segments);
/* the three forms of pfx_shape_rasterize / pfx_shape_preview / pfx_shape_draw_dev, with the same contracts; w, h are the canvas.  buf = the box buffer, bit for
 * bit the reference's `buf` (bw*bh*4 bytes; an empty box: PFX_OK, buffer untouched); preview = the whole canvas, every byte written; draw on image_dev, the
 * layer (w*h*4), equals preview followed by pfx_brush_commit with sel_dev as the selection (w*h bytes) and neither reads nor writes outside the box. */
int pfx_custom_shape_rasterize(pfx_ctx* ctx, const pfx_shape* shape, const pfx_custom_path* path, uint32_t w, uint32_t h, uint8_t* buf_rgba);
int pfx_custom_shape_rasterize_dev(pfx_ctx* ctx, const pfx_shape* shape, const pfx_custom_path* path, uint32_t w, uint32_t h, void* buf_dev);
int pfx_custom_shape_preview(pfx_ctx* ctx, const pfx_shape* shape, const pfx_custom_path* path, uint32_t w, uint32_t h, uint8_t* preview_rgba);
int pfx_custom_shape_preview_dev(pfx_ctx* ctx, const pfx_shape* shape, const pfx_custom_path* path, uint32_t w, uint32_t h, void* preview_dev);
int pfx_custom_shape_draw_dev(pfx_ctx* ctx, void* image_dev, uint32_t w, uint32_t h, const pfx_shape* shape, const pfx_custom_path* path, uint8_t blend_mode,
                              const void* sel_dev /* may be NULL */);
/* the shape picker's icon (render_custom_shape_icon :122-155): size x size RGBA8, 16 samples per pixel at (x + (s + 0.5) * 0.25) / size * 2 - 1, the path fitted
 * to half extents 0.82, Filled.  Where the coverage is above 0: grey 235 (dark != 0) or 30 in r, g, b and alpha (255 * cov).round(); every other pixel is zero. */
int pfx_custom_shape_icon(pfx_ctx* ctx, const pfx_custom_path* path, uint32_t size, int dark, uint8_t* rgba /* size*size*4 */);
int pfx_custom_shape_icon_dev(pfx_ctx* ctx, const pfx_custom_path* path, uint32_t size, int dark, void* rgba_dev);

/* ================= content-aware fill (ref: src/ops/inpaint.rs) =================
 * Images are w*h RGBA8, the hole mask is w*h bytes (> 0 = pixel to fill).  Both routines are in the bit-exact class: the reference's two inpaint goldens are
 * reproduced with tolerance 0.  The one per-pixel transcendental is exp, evaluated as glibc's expf bit for bit; the ring's cos / sin are uniform over the image
 * and computed on the host.
 *
 * Instant heal dabs (inpaint_instant_brush :76-192): each pixel of the mask under a dab becomes the colour-similarity-weighted mean of 32 ring samples of `src`
 * around it, blended into `out` by the dab's hardness-aware alpha.  A dab list is applied in order, in one launch.  src and the mask are only read; `out` must
 * not overlap either (PFX_ERR_INVALID).  Non-finite dab fields are refused.  n_dabs == 0 is a no-op (PFX_OK), like the brush calls. */
typedef struct pfx_inpaint_dab { float cx, cy, brush_radius, sample_radius, hardness; } pfx_inpaint_dab;
/* the 32 candidate offsets (cos(angle_i) * rr_i, sin(angle_i) * rr_i) of a sample radius, x and y interleaved (:141-147).  Host only; NULL out is a no-op. */
void pfx_inpaint_ring_offsets(float sample_radius, float out_xy[64]);
int pfx_inpaint_instant(pfx_ctx* ctx, const uint8_t* src, const uint8_t* hole_mask, uint8_t* out_inout, uint32_t w, uint32_t h, const pfx_inpaint_dab* dabs,
                        uint32_t n_dabs);
int pfx_inpaint_instant_dev(pfx_ctx* ctx, const void* src_dev, const void* hole_mask_dev, void* out_dev, uint32_t w, uint32_t h, const pfx_inpaint_dab* dabs,
                            uint32_t n_dabs);
/* Onion-peeling PatchMatch (fill_region_patchmatch :394-520), the reference's result bit for bit, its scan orders included: per peel the hole's boundary
 * pixels get a random-initialised nearest-neighbour field, 2 (iterations <= 3) or 4 propagation / random-search passes, and the colour of their best source.
 * patch_size: values below 3 count as 3, values above 11 (the tool's range) are refused.  An empty mask or a mask without a non-hole pixel gives a copy of
 * src.  dst == src (in place) is allowed; any other overlap of dst with src or the mask is refused.  Working memory (about 5 bytes per canvas pixel) is
 * allocated before dst is touched: PFX_ERR_OOM leaves dst as it was.  The host waits for the device once per peel. */
int pfx_inpaint_patchmatch(pfx_ctx* ctx, const uint8_t* src, const uint8_t* hole_mask, uint8_t* dst, uint32_t w, uint32_t h, uint32_t patch_size,
                           uint32_t iterations);
int pfx_inpaint_patchmatch_dev(pfx_ctx* ctx, const void* src_dev, const void* hole_mask_dev, void* dst_dev, uint32_t w, uint32_t h, uint32_t patch_size,
                               uint32_t iterations);

/* ================= bucket fill and magic wand: flood distance maps (ref: src/ui/panels/tools/behavior/raster/fill_magic.rs, tools/state.rs:574-735) =================
 * The CPU flavour of the two tools, bit for bit (the reference's WGSL variants — 5-step AA band, pow 2.2, boundary softening — are not implemented).
 * Images are w*h RGBA8; distance maps, masks and selections are w*h bytes.  Everything is in the bit-exact class.
 *
 * Per-pixel colour distance to `target` (pixel_color_distance :1048): legacy = 0 when both alphas are 0, else the largest channel difference; perceptual
 * (perceptual_distance :93, srgb_to_linear :84) = the reference's f32 expression in its association order — the 256 powf values come from the host libm.
 * Distance map: global scope = that distance per pixel (compute_global_distance_map :1024); contiguous scope = the bottleneck distance from the seed
 * (compute_flood_distance_map :950): d[seed] = c[seed], elsewhere the minimum over 4- or 8-connected paths of the largest c on the path; a pixel no path
 * reaches keeps 255.  The map is unique, whatever algorithm computes it.
 * Refused with PFX_ERR_INVALID: a seed outside the image (the reference ignores the click, perform_flood_fill :1242), connectivity other than 4 or 8,
 * distance_mode or global above 1, combine_mode above 3, blend_mode above 24, a distance map that overlaps an output, an RGBA8 device pointer (src_dev,
 * canvas_out_dev, layer_dev) that is not 4-byte aligned.  Outputs are untouched on any error: every refusal comes before the first launch, and the connected
 * flood runs in working memory and copies the map out last (the global scope writes dist_dev directly; past the checks only its launch could fail). */
typedef struct pfx_flood {
    uint32_t seed_x, seed_y;
    uint8_t  target[4];
    uint8_t  distance_mode;  /* 0 LegacyRgba, 1 Perceptual (WandDistanceMode) */
    uint8_t  connectivity;   /* 4 or 8 (FloodConnectivity) */
    uint8_t  global;         /* 0 contiguous, 1 global scope */
    uint8_t  _pad;
} pfx_flood;
/* tolerance_threshold_u8 (:78): round(clamp(tolerance / 100, 0, 1) * 255); NaN gives 0.  Host only, no context. */
uint8_t pfx_tolerance_threshold(float tolerance);
int pfx_flood_distance(pfx_ctx* ctx, const uint8_t* src, uint32_t w, uint32_t h, const pfx_flood* flood, uint8_t* dist);
int pfx_flood_distance_dev(pfx_ctx* ctx, const void* src_dev, uint32_t w, uint32_t h, const pfx_flood* flood, void* dist_dev);
/* ThresholdRegionIndex::from_distances' cumulative boxes (state.rs:693, threshold_bbox :732): for every t in 0..255 the inclusive box x0, y0, x1, y1 of
 * {d <= t} at boxes[4 t ..], or -1, -1, -1, -1 when the set is empty.  `boxes` is host memory; the call waits for the device. */
int pfx_flood_bboxes_dev(pfx_ctx* ctx, const void* dist_dev, uint32_t w, uint32_t h, int32_t boxes[1024]);
/* threshold_alpha (:415) then merge_magic_wand_masks (:486): raw = 255 where d <= threshold, with anti_aliased 128 where d == sat_add(threshold, 1), else 0;
 * combine_mode 0 replace = raw, 1 add = max(base, raw), 2 subtract = sat(base - raw), 3 intersect = base * raw / 255.  base_mask NULL = all zero
 * (replay_magic_wand_selection :495).  mask_out == base_mask (in place) is allowed; any other overlap is refused. */
int pfx_wand_mask(pfx_ctx* ctx, const uint8_t* dist, const uint8_t* base_mask /* may be NULL */, uint32_t w, uint32_t h, uint8_t threshold, uint8_t anti_aliased,
                  uint8_t combine_mode, uint8_t* mask_out);
int pfx_wand_mask_dev(pfx_ctx* ctx, const void* dist_dev, const void* base_mask_dev /* may be NULL */, uint32_t w, uint32_t h, uint8_t threshold,
                      uint8_t anti_aliased, uint8_t combine_mode, void* mask_out_dev);
/* the fill tool's preview layer over the whole canvas (build_fill_preview_region :550; the fill mask is the threshold mask without the AA band, :775):
 * fill.rgb with alpha (fill.a * 255 + 127) / 255 where d <= threshold and the selection (NULL = none) is > 0, else 0, 0, 0, 0 — the form
 * pfx_composite_preview takes.  Every byte of canvas_out (w*h*4) is written. */
int pfx_fill_preview(pfx_ctx* ctx, const uint8_t* dist, const uint8_t* selection /* may be NULL */, uint32_t w, uint32_t h, uint8_t threshold, const uint8_t fill[4],
                     uint8_t* canvas_out);
int pfx_fill_preview_dev(pfx_ctx* ctx, const void* dist_dev, const void* selection_dev /* may be NULL */, uint32_t w, uint32_t h, uint8_t threshold,
                         const uint8_t fill[4], void* canvas_out_dev);
/* preview and commit in one kernel (commit_fill_preview_impl :1414-1446): equals pfx_fill_preview followed by pfx_brush_commit with is_eraser = 0 */
int pfx_fill_commit_dev(pfx_ctx* ctx, void* layer_dev, const void* dist_dev, const void* selection_dev /* may be NULL */, uint32_t w, uint32_t h, uint8_t threshold,
                        const uint8_t fill[4], uint8_t blend_mode);
/* the bucket tool (perform_flood_fill :1231-1273): target = the layer pixel at the seed, LegacyRgba, 4-connected, global_fill != 0 = global scope,
 * threshold = pfx_tolerance_threshold(tolerance); `fill` is the tool's colour as bytes ((c * 255) as u8, truncating) */
int pfx_bucket_fill(pfx_ctx* ctx, uint8_t* layer_inout, uint32_t w, uint32_t h, uint32_t seed_x, uint32_t seed_y, float tolerance, const uint8_t fill[4],
                    uint8_t blend_mode, int global_fill, const uint8_t* selection /* may be NULL */);

/* ================= pfx_select: selection masks, the CanvasState / tools flavour (ref: src/canvas/selection.rs:66-116, src/canvas/canvas_state.rs:1632-1887,
 * src/ui/panels/tools/behavior/raster/perspective_gradient.rs:2-86, src/ops/adjustments.rs:1448-1591) =================
 * Produces and edits the w*h-byte selection masks the other operators take.  Everything is integer or single-rounded f32 arithmetic: the bit-exact class.
 * (The script flavour — select_rect, fill_selected, ... of pfx_script_execute — has other rules and is not touched by this section.)
 *
 * Combine rule of rectangle, ellipse and lasso (apply_selection_shape :1713, the lasso merge :40-86; one rule for every byte value of the base): where the
 * shape covers a pixel the result is 255 (replace, add), 0 (subtract) or base (intersect); elsewhere it is base (add, subtract) or 0 (replace, intersect).
 * combine_mode as in pfx_wand_mask: 0 replace, 1 add, 2 subtract, 3 intersect.  base_mask NULL = an all-zero base.  mask_out == base_mask (in place) is
 * allowed; any other overlap is refused.  Every byte of mask_out is written.
 * Refused with PFX_ERR_INVALID: combine_mode above 3, an overlap as above, a lasso coordinate that is not finite or beyond 1e9 in magnitude (the reference's
 * sort is then order-dependent or its intermediate overflows), a feather radius that is not finite, an expand / contract radius above 46340 (the reference's
 * i32 square overflows), a layer_dev that is not 4-byte aligned or overlaps the mask.  Refused with PFX_ERR_UNSUPPORTED: more than 8192 lasso points (one
 * row's crossings are sorted in 32 KB of on-chip memory) and a feather radius above 512 — the reference has no cap, but its pass count is radius / 2 and a
 * hostile radius would be billions of passes on a shared device.  Outputs are untouched on any error: every refusal comes before the first launch, and the
 * feather runs in working memory and copies out last. */
/* inclusive min / max (SelectionShape::Rectangle, contains :70-80, bounds :96-106): max is clamped to the canvas, min > max selects nothing (no error) */
int pfx_select_rect(pfx_ctx* ctx, const uint8_t* base_mask /* may be NULL */, uint32_t w, uint32_t h, uint32_t min_x, uint32_t min_y, uint32_t max_x, uint32_t max_y,
                    uint8_t combine_mode, uint8_t* mask_out);
int pfx_select_rect_dev(pfx_ctx* ctx, const void* base_mask_dev /* may be NULL */, uint32_t w, uint32_t h, uint32_t min_x, uint32_t min_y, uint32_t max_x,
                        uint32_t max_y, uint8_t combine_mode, void* mask_out_dev);
/* ((x - cx) / rx)^2 + ((y - cy) / ry)^2 <= 1 in f32, one rounding per operation (contains :82-89), evaluated only inside the reference's bounding box
 * floor(max(c - r, 0)) .. min(ceil(c + r) as u32, dim - 1) (bounds :107-113); rx <= 0 or ry <= 0 selects nothing, and so does a NaN */
int pfx_select_ellipse(pfx_ctx* ctx, const uint8_t* base_mask /* may be NULL */, uint32_t w, uint32_t h, float cx, float cy, float rx, float ry, uint8_t combine_mode,
                       uint8_t* mask_out);
int pfx_select_ellipse_dev(pfx_ctx* ctx, const void* base_mask_dev /* may be NULL */, uint32_t w, uint32_t h, float cx, float cy, float rx, float ry,
                           uint8_t combine_mode, void* mask_out_dev);
/* the lasso's scanline fill (apply_lasso_selection :2-38): per row the crossings of y + 0.5 with the closed polygon, sorted, filled pairwise from
 * trunc(max(n0, 0)) to trunc(max(n1 + 1, 0)) exclusive.  points_xy: n_points (x, y) pairs in HOST memory in both forms; fewer than 3 points are accepted
 * (same arithmetic, usually an empty shape) */
int pfx_select_lasso(pfx_ctx* ctx, const uint8_t* base_mask /* may be NULL */, uint32_t w, uint32_t h, const float* points_xy, uint32_t n_points, uint8_t combine_mode,
                     uint8_t* mask_out);
int pfx_select_lasso_dev(pfx_ctx* ctx, const void* base_mask_dev /* may be NULL */, uint32_t w, uint32_t h, const float* points_xy, uint32_t n_points,
                         uint8_t combine_mode, void* mask_out_dev);
/* translate_selection (:1677): out[x, y] = mask[x - dx, y - dy] where that is inside the image, else 0.  Not in place: any overlap is refused */
int pfx_selection_translate(pfx_ctx* ctx, const uint8_t* mask, uint32_t w, uint32_t h, int32_t dx, int32_t dy, uint8_t* mask_out);
int pfx_selection_translate_dev(pfx_ctx* ctx, const void* mask_dev, uint32_t w, uint32_t h, int32_t dx, int32_t dy, void* mask_out_dev);
/* feather_selection (adjustments.rs:1448): max(trunc(radius / 2), 1) passes of a horizontal then a vertical box over [p - r, p + r] cut at the image edge,
 * r = max(trunc(radius), 1), each `sum / count` truncating through u8 (a negative radius: r = 1, one pass).  radius at most 512 (see above).
 * feather, expand and contract allow mask_out == mask (in place) and refuse any other overlap */
int pfx_selection_feather(pfx_ctx* ctx, const uint8_t* mask, uint32_t w, uint32_t h, float radius, uint8_t* mask_out);
int pfx_selection_feather_dev(pfx_ctx* ctx, const void* mask_dev, uint32_t w, uint32_t h, float radius, void* mask_out_dev);
/* expand_selection (:1500): a pixel <= 127 becomes 255 when a pixel > 127 of the image lies within dx^2 + dy^2 <= r^2, r = max(radius, 0); others keep their value.
 * contract_selection (:1547): a pixel != 0 becomes 0 when a pixel == 0 of the image lies within the disc; outside the image is not zero (the canvas edge does
 * not erode).  radius at most 46340; radius <= 0 is the identity */
int pfx_selection_expand(pfx_ctx* ctx, const uint8_t* mask, uint32_t w, uint32_t h, int32_t radius, uint8_t* mask_out);
int pfx_selection_expand_dev(pfx_ctx* ctx, const void* mask_dev, uint32_t w, uint32_t h, int32_t radius, void* mask_out_dev);
int pfx_selection_contract(pfx_ctx* ctx, const uint8_t* mask, uint32_t w, uint32_t h, int32_t radius, uint8_t* mask_out);
int pfx_selection_contract_dev(pfx_ctx* ctx, const void* mask_dev, uint32_t w, uint32_t h, int32_t radius, void* mask_out_dev);
/* selection_mask_bounds (:1632): the inclusive box x0, y0, x1, y1 of {mask != 0}, or -1, -1, -1, -1 when the mask is empty.  `box` is host memory; the call
 * waits for the device */
int pfx_selection_bounds_dev(pfx_ctx* ctx, const void* mask_dev, uint32_t w, uint32_t h, int32_t box[4]);
/* fill_selected_pixels (:1844) / delete_selected_pixels (:1806) on an RGBA8 layer, in place, through a mask that may be grey: 0 leaves the pixel, 255 writes
 * the colour (0, 0, 0, 0 for delete), otherwise t = sel / 255 and every channel becomes round(old * (1 - t) + new * t) (fill) or alpha becomes
 * round(a * (1 - t)) with rgb kept (delete) — f32, unfused, half away from zero.  Not the script's fill_selected / delete_selected */
int pfx_selection_fill_dev(pfx_ctx* ctx, void* layer_dev, const void* mask_dev, uint32_t w, uint32_t h, const uint8_t color[4]);
int pfx_selection_delete_dev(pfx_ctx* ctx, void* layer_dev, const void* mask_dev, uint32_t w, uint32_t h);

/* ================= removal by colour: colour to alpha and the colour remover (ref: src/ops/color_removal.rs) =================
 * The Colour to Alpha dialog (color_to_alpha_core :32-150) and the Color Remover tool, the "smart contiguous eraser" (compute_color_removal :161-418 followed
 * by apply_color_removal :421).  Images are w*h RGBA8; masks and selections are w*h bytes, 0 = unselected, anything else = selected (the reference also takes
 * a smaller mask; this surface does not).  Everything is in the bit-exact class: u8 -> f32, one rounding per written operation, IEEE division, round() half
 * away from zero.  dst is src with the changed pixels replaced — the dialog's returned image, or img.clone() then apply_color_removal for the tool; every
 * byte of dst is written.  dst == src (in place) is allowed; any other overlap of dst with src or the mask is refused.
 * Refused with PFX_ERR_INVALID: a NULL struct, a float of either struct that is not finite, a seed outside the image (as in pfx_flood_distance; the
 * reference ignores the click), contiguous above 1, an RGBA8 device pointer that is not 4-byte aligned, the overlaps above.  Refused with
 * PFX_ERR_UNSUPPORTED: smoothness above 1024 — the reference has no cap, but the launch count grows with it on a shared device (the tool offers 0..20).
 * PFX_OK with dst a copy of src, like the reference's empty change list: a seed pixel with alpha 0 (:185), a selection that is 0 at the seed (:175-181).
 * Outputs are untouched on any error: every refusal comes before the first launch, all working memory is allocated before dst is touched, and only the last
 * launch writes dst.  The colour remover waits for the device once for the clicked pixel and, in the contiguous scope, once per flood pass. */
typedef struct pfx_color_to_alpha {      /* ColorToAlphaSettings :6-30; the defaults there: target 255, 0, 0; 18; 35; 1; 0.35; 0; 1; 0.15 */
    uint8_t target[3], _pad;
    float tolerance, softness;           /* 0..255: full removal within tolerance, fading out over softness (softness / 255 is at least 0.001) */
    float strength, spill_suppression, alpha_floor, alpha_ceiling, protect_luminance;   /* clamped to 0..1; alpha_ceiling to alpha_floor..1 */
} pfx_color_to_alpha;
int pfx_color_to_alpha_core(pfx_ctx* ctx, const uint8_t* src, uint8_t* dst, uint32_t w, uint32_t h, const pfx_color_to_alpha* settings, const uint8_t* mask /* may be NULL */);
int pfx_color_to_alpha_dev(pfx_ctx* ctx, const void* src_dev, void* dst_dev, uint32_t w, uint32_t h, const pfx_color_to_alpha* settings, const void* mask_dev /* may be NULL */);
/* The tool in three steps.  1, the core: contiguous = the 4-connected component of the seed over pixels that are selected and either fully transparent or
 * within (tolerance * 2.55)^2 of the seed's rgb in squared distance (the flood runs through transparent pixels); global = every selected pixel within that
 * distance with alpha != 0.  2, rings: `smoothness` one-pixel rings around the core, a 4-connected breadth-first dilation that never enters an unselected
 * pixel (a geodesic distance, not a masked L1 distance).  3, colour to alpha against the seed's colour with rgb recovery, fading linearly over the rings.
 * (The struct cannot share the entry point's name in C: it carries the reference's, ColorRemovalRequest.) */
typedef struct pfx_color_removal_req {   /* ColorRemovalRequest, tools/state.rs:1723 */
    uint32_t seed_x, seed_y;
    float    tolerance;                  /* 0..100, the tool's slider; a negative value acts like its magnitude */
    uint32_t smoothness;                 /* rings, at most 1024 */
    uint8_t  contiguous, _pad[3];        /* 1 contiguous, 0 global scope */
} pfx_color_removal_req;
int pfx_color_removal(pfx_ctx* ctx, const uint8_t* src, uint8_t* dst, uint32_t w, uint32_t h, const pfx_color_removal_req* req, const uint8_t* selection /* may be NULL */);
int pfx_color_removal_dev(pfx_ctx* ctx, const void* src_dev, void* dst_dev, uint32_t w, uint32_t h, const pfx_color_removal_req* req, const void* selection_dev /* may be NULL */);

/* ================= the floating selection: lift, transform, preview, commit (ref: src/ops/clipboard.rs, PasteOverlay :818) =================
 * What the Move Pixels tool, every paste and "selection -> new transform" go through: extract_to_overlay :729 lifts the pixels, render_preview :2168 runs on
 * every drag frame, commit :2032 stamps the transformed pixels back; render_replacement_preview :1144 and rasterize_for_clipboard :1048 are the same sampling
 * with other windows.  All geometry travels in one descriptor, and pfx_overlay_geometry is the one place that derives sizes and boxes from it.  Images are
 * RGBA8, `source` is source_w * source_h, the layer / base / preview are doc_w * doc_h; the overwrite mask is source_w * source_h bytes.  Everything is in the
 * bit-exact class: every f32 expression as the reference writes it, one rounding per operation, round() half away from zero, `as u32` / `as i32` saturating
 * and truncating; cos and sin of the rotation are taken once per call on the host (cosf / sinf).  The scale step is pfx_resize_image_dev's; the one-byte
 * overwrite mask follows that resize's NEAREST rule (an index lookup).
 * Refused with PFX_ERR_INVALID: a NULL descriptor or required pointer, a float of the descriptor that is not finite, interpolation outside PFX_RESIZE_*,
 * a document, a source or a scaled size (max(round(source * scale), 1)) outside the document limit — the reference would try to allocate it —, a clipboard
 * raster window outside that limit, an RGBA8 device pointer that is not 4-byte aligned, any overlap of an output with another buffer other than
 * out == base.  Outputs are untouched on any error: every refusal comes before the first launch.
 * Two deviations, both in pfx_overlay_preview_dev: in the translation-only path the reference wraps (origin + scaled size) as u32 when that sum is negative
 * and then indexes outside the scaled image (a panic) — here such an overlay draws nothing; and the reference's row strips keep the column in 16 bits —
 * here the true column is drawn on documents wider than 65535. */
typedef struct pfx_overlay {           /* PasteOverlay :818-837, plus the sizes */
    uint32_t source_w, source_h;       /* the un-transformed source image (and its overwrite mask) */
    uint32_t doc_w, doc_h;             /* the layer / canvas */
    float    center_x, center_y;       /* canvas coordinates of the source's centre */
    float    rotation;                 /* radians */
    float    scale_x, scale_y;
    float    anchor_x, anchor_y;       /* anchor_offset, relative to the centre */
    int32_t  interpolation;            /* PFX_RESIZE_*: Interpolation::to_filter, transform.rs:29-58 */
    uint8_t  anti_aliasing, overwrite_transparent, _pad[2];
} pfx_overlay;
typedef struct pfx_overlay_geom {
    uint32_t scaled_w, scaled_h;       /* max(round(source * scale), 1) as u32 */
    float    cos_r, sin_r;
    float    corners[8];               /* corners_canvas :1313: x, y of top-left, top-right, bottom-left, bottom-right, from the unrounded half size */
    uint32_t row_start, row_end, col_start, col_end;   /* the commit box :2054-2069, inclusive; empty when a start is above its end */
    uint32_t has_bounds, bounds[4];    /* transformed_bounds :939-959: x0, y0, x1, y1 (exclusive ends), has_bounds 0 = None */
    int32_t  raster_col, raster_row;   /* rasterize_for_clipboard's window :1060-1081, not clipped to the document */
    uint32_t raster_w, raster_h;       /* 0 where the reference returns None; saturates at UINT32_MAX */
} pfx_overlay_geom;
/* host only, no context: the derived quantities of a descriptor; the calls below start with it */
int pfx_overlay_geometry(const pfx_overlay* ov, pfx_overlay_geom* out);
/* commit (out == base: only pixels of the commit box are written) or render_replacement_preview (any other out: a copy of base, then the same stamp; every
 * byte is written).  Per pixel of the box: the inverse rotation about centre + anchor, the +-0.5 window (the tight one without anti-aliasing), sample_bilinear
 * :2326 or the truncating nearest pick, then either the overwrite (overwrite_transparent, where overwrite_mask_allows :1150) or alpha_blend :2368 of samples
 * with alpha > 0.  The mask is read only when overwrite_transparent is set */
int pfx_overlay_commit_dev(pfx_ctx* ctx, const pfx_overlay* ov, const void* source_dev, const void* overwrite_mask_dev /* may be NULL */, const void* base_dev,
                           void* out_dev);
int pfx_overlay_commit(pfx_ctx* ctx, const pfx_overlay* ov, const uint8_t* source, const uint8_t* overwrite_mask /* may be NULL */, const uint8_t* base, uint8_t* out);
/* render_preview: a doc_w * doc_h image, every byte written, (0, 0, 0, 0) where nothing is drawn: ready for pfx_flatten_preview_dev.  Always the NEAREST
 * scale; |rotation| < 1e-4 and |anchor| < 1e-3 take the translation-only path with the rounded integer origin, anything else the general one (tight window,
 * nearest pick); only pixels with alpha > 0 are drawn.  interpolation is checked but not used; anti_aliasing and overwrite_transparent are not looked at */
int pfx_overlay_preview_dev(pfx_ctx* ctx, const pfx_overlay* ov, const void* source_dev, void* preview_dev);
/* rasterize_for_clipboard: commit's sampler into the geometry's raster window (raster_w * raster_h RGBA8, tightly packed), no blending: samples with
 * alpha > 0 are stored over zero.  *has_pixels (host memory; the call waits for the device) is 0 where the reference returns None */
int pfx_overlay_rasterize_dev(pfx_ctx* ctx, const pfx_overlay* ov, const void* source_dev, void* out_dev, int* has_pixels);
/* extract_to_overlay.  With a selection (doc_w * doc_h bytes): clip = the box of {selection > 0}, tightly packed, the layer's pixel where selection > 0 and
 * zero elsewhere; clip_mask = 255 / 0 likewise; the layer is blanked as pfx_selection_delete_dev does (grey-aware); *out = the box's size, its centre
 * (min + size / 2) and PasteOverlay::new's defaults (scale 1, rotation 0, Bilinear, anti-aliasing on, overwrite off).  Without one: the whole layer becomes
 * the clip, the layer becomes zero, clip_mask is not written (and may be NULL), the centre is the document's.  The reference's None — nothing selected, or no
 * selection and no alpha anywhere in the layer — is PFX_OK with out->source_w == 0 and nothing written.  clip_dev and clip_mask_dev need room for the
 * whole document; the call waits for the device once */
int pfx_overlay_extract_dev(pfx_ctx* ctx, void* layer_dev, const void* selection_dev /* may be NULL */, uint32_t doc_w, uint32_t doc_h, void* clip_dev,
                            void* clip_mask_dev, pfx_overlay* out);

/* ================= text layer styles: shadow, outline, fills, inner shadow (ref: src/ops/text_layer/effects.rs, apply_text_effects) =================
 * What TextLayerData::rasterize (data_impl.rs:132-194) runs behind the glyphs after every keystroke and style-slider tick: it takes the rasterised text as
 * RGBA8 and returns RGBA8.  Fonts, layout and glyph rasterisation are not here; the warps are the next section.  All sizes and parameters travel in one descriptor that mirrors
 * TextEffects (core.rs:299-364); `flags` says which of its five Options are Some.  coverage = alpha / 255.0f.  The stages, in this order, each through the
 * integer composite_over of effects.rs:47-71 (u32 arithmetic) onto an output that starts as zero:
 *   1 shadow        the coverage shifted by (round(offset_x), round(offset_y)) (half away from zero, then a saturating `as i32`; zero from outside), dilated
 *                   by `spread` when spread > 0.5, alpha = round(mask * colour alpha); blur_radius > 0.5: the (colour rgb, alpha) image through
 *                   parallel_gaussian_blur_pub (sigma = blur_radius; the bit-exact Gaussian, unless the context opted out with pfx_tune "gauss_fast_effects")
 *                   and composite_over of the blurred pixel — with clamp-to-edge and one colour everywhere the blurred rgb is the colour itself, so rows that
 *                   allow it blur the alpha plane alone —; else the colour with that alpha, alpha 0 skipped.
 *   2 outline       Outside at radius = width, Center at radius = width * 0.5 (its outside half only; render_outline_inside is never reached for Center);
 *                   nothing when radius <= 0: alpha = clamp(dilated - coverage, 0, 1) * (colour alpha / 255.0), skipped below 1.0 / 255.0, then round(. * 255).
 *   3 fill          the gradient when its flag is set; else the texture when its flag is set; else the text itself.  Gradient: to_radians, cosf / sinf once
 *                   per call on the host, scale.max(1.0), proj = ((x - offset[0]) * cos + (y - offset[1]) * sin) / scale, t = proj.rem_euclid(1.0) (fmodf,
 *                   + 1 when negative: can be exactly 1.0) with `repeat`, else clamp(proj, 0, 1); rgb = round(start * (1 - t) + end * t), alpha =
 *                   round((start alpha * (1 - t) + end alpha * t) * coverage).  Texture: scale.max(0.01), tx = ((fmodf((x - offset[0]) / scale, tex_w) + tex_w)
 *                   as usize) % tex_w, likewise ty; rgb of that texel, alpha = min(round(coverage * 255), texel alpha).  The texture is decoded RGBA8
 *                   (tex_w * tex_h, tightly packed; pfx_png_decode_mem decodes a PNG); a zero tex_w or tex_h is the plain text fill.  Both skip coverage < 1 / 255.
 *   4 inside outline  radius = width: alpha = clamp(coverage - eroded, 0, 1) * (colour alpha / 255.0) as in 2, eroded = max(1 - dilate(1 - coverage), 0).
 *   5 inner shadow  1 - coverage shifted like the shadow's (1.0 from outside the image); blur_radius > 0.5: alpha = round(that * colour alpha), the image
 *                   blurred as in 1, then round(blurred alpha * coverage); else round((that * colour alpha) * coverage).  Both skip coverage < 1 / 255.
 * With no flag set the result is composite_over(text, zeros).
 * The dilation is dilate_mask :167-214: the maximum over the disc dx * dx + dy * dy <= radius * radius (f32, the square rounded once) clipped to the image,
 * starting from 0; rows reach ceil(radius), so a radius of 0.5 changes nothing.  Coverage is monotone in alpha, so the device takes the disc's maximum (the
 * erosion: minimum) on the u8 alpha plane, row span by row span, not tap by tap.
 * Everything is in the bit-exact class: every f32 expression as the reference writes it, one rounding per operation, round() half away from zero.
 * Refused with PFX_ERR_INVALID, before the first launch and with outputs untouched: a NULL descriptor or required pointer; a float of the descriptor that is
 * not finite (whatever the flags say); an outline position outside PFX_TEXT_OUTLINE_*; width * height outside the document limit; with the texture flag and a
 * non-zero tex_w * tex_h, a NULL texture or a texture outside the document limit; a device pointer that is not 4-byte aligned; any overlap of the output
 * with an input (nothing runs in place).  PFX_ERR_UNSUPPORTED, likewise before the first launch: a dilation radius (the outline's, the shadow's spread above
 * 0.5) whose ceil is above PFX_TEXT_FX_MAX_RADIUS — the editor's sliders reach 50 and 30 —, and a blur radius beyond what the Gaussian accepts
 * (ceil(3 * blur_radius) above its tile limit, as pfx_gaussian_blur_dev).
 * One deviation, in the region rule: the reference computes `bx as i32 - pad_px as i32` and `bx + bw + pad_px` in 32 bits, which wrap or panic for a padding
 * of 2^31 and more; here that arithmetic is 64 bits wide, so such a padding just covers the canvas. */
#define PFX_TEXT_FX_OUTLINE       1u
#define PFX_TEXT_FX_SHADOW        2u
#define PFX_TEXT_FX_INNER_SHADOW  4u
#define PFX_TEXT_FX_GRADIENT_FILL 8u
#define PFX_TEXT_FX_TEXTURE_FILL  16u
#define PFX_TEXT_FX_MAX_RADIUS    64
enum { PFX_TEXT_OUTLINE_INSIDE = 0, PFX_TEXT_OUTLINE_OUTSIDE = 1, PFX_TEXT_OUTLINE_CENTER = 2 };   /* OutlinePosition, core.rs:314-319 */
typedef struct pfx_text_fx {              /* TextEffects core.rs:299-364, plus the image size (C has one namespace: pfx_text_effects is the host-tier call below) */
    uint32_t width, height;               /* of the text image; the canvas for pfx_text_effects_plan and pfx_text_layer_effects_dev */
    uint32_t flags;                       /* PFX_TEXT_FX_*: which members below are Some */
    uint8_t  outline_color[4];            /* OutlineEffect */
    float    outline_width;
    int32_t  outline_position;            /* PFX_TEXT_OUTLINE_* */
    uint8_t  shadow_color[4];             /* ShadowEffect */
    float    shadow_offset_x, shadow_offset_y, shadow_blur_radius, shadow_spread;
    uint8_t  inner_color[4];              /* InnerShadowEffect */
    float    inner_offset_x, inner_offset_y, inner_blur_radius;
    uint8_t  gradient_start[4], gradient_end[4];   /* GradientFillEffect */
    float    gradient_angle_degrees, gradient_scale, gradient_offset[2];
    uint32_t gradient_repeat;             /* 0 / 1 */
    uint32_t tex_w, tex_h;                /* TextureFillEffect: the decoded texture's size */
    float    texture_scale, texture_offset[2];
} pfx_text_fx;
typedef struct pfx_text_region {          /* what data_impl.rs:132-172 derives from the text's tight bounds */
    uint32_t x, y, w, h;                  /* the bounds grown by pad_px and clamped to the canvas; all zero when there is no visible text */
    uint32_t pad_px;                      /* max(ceil(pad) as u32, 4) */
    uint32_t full_canvas;                 /* 1: region area * 2 >= canvas area, the effects run on the whole canvas */
} pfx_text_region;
/* apply_text_effects on a width * height image: text and out are RGBA8 of that size, every byte of out is written; asynchronous on the context's stream */
int pfx_text_effects_dev(pfx_ctx* ctx, const pfx_text_fx* fx, const void* text_dev, const void* texture_dev /* may be NULL */, void* out_dev);
int pfx_text_effects(pfx_ctx* ctx, const pfx_text_fx* fx, const uint8_t* text, const uint8_t* texture /* may be NULL */, uint8_t* out);
/* host only, no context: the padding and region rule.  bounds = x, y, w, h of the pixels with alpha > 0 (find_tight_bounds_rgba, raster.rs:23-41), inside the
 * canvas; a zero w or h is "no visible text": *out is all zero.  pad = max(|ox| + |oy| + 3 * blur + spread of the shadow, ceil(outline width) + 2, |ox| +
 * |oy| + 3 * blur of the inner shadow), over the members whose flag is set, in f32 as written; pad_px = max(ceil(pad) as u32 (saturating), 4) */
int pfx_text_effects_plan(const pfx_text_fx* fx, const uint32_t bounds[4], pfx_text_region* out);
/* data_impl.rs:132-194 for a canvas-sized text image (width * height of the descriptor): the tight bounds of alpha > 0 on the device (one wait for the
 * device), the plan, the effects on the cropped region or on the whole canvas, the result blitted into an otherwise zero canvas: every byte of out is written.
 * No visible text is a zero canvas and PFX_OK.  *region_out (host memory) receives the plan */
int pfx_text_layer_effects_dev(pfx_ctx* ctx, const pfx_text_fx* fx, const void* text_dev, const void* texture_dev /* may be NULL */, void* out_dev,
                               pfx_text_region* region_out /* may be NULL */);

/* ================= text warps and block placement: arc, circle, path, envelope, rotate, blit (ref: src/ops/text_layer/warp.rs, raster.rs:374-417) =================
 * What rasterize_block runs on a block's tight raster after every keystroke and every drag of a warp handle, one stage in front of the styles above: the
 * warp (apply_block_warp, warp.rs:80-93), the rotation (rotate_glyph_buffer, raster.rs:561-653) and the blit into the layer image (maybe_rotate_and_blit,
 * selection.rs:77-106; blit_rgba_buffer, warp.rs:39-70).  Every warp is an inverse map per output pixel followed by bilinear_sample :707-740 (transparent
 * outside, p00 (1 - fx)(1 - fy) + p10 fx (1 - fy) + p01 (1 - fx) fy + p11 fx fy, round half away from zero); every f32 expression is the reference's, one
 * rounding per operation.
 *   plan      the output's size and offset, on the host, from the reference's own sampling loops (arc :118-150 with glibc sinf / cosf, circular :283-300,
 *             path :368-406, envelope :460-490).  Identity (the reference's `src.to_vec()` returns; out = src size, offset 0, 0; the device call copies):
 *             kind NONE; arc with |bend| < 0.001 or an output side of 0 or above 8192; path / envelope with fewer than 4 points or a zero side.
 *   arc       apply_arc_warp :155-176 with arc_inverse_map :222-274 as written: a distortion of -1 divides by zero and the comparisons then reject the pixel.
 *   circular  :305-349: radius = max(radius, 10), the annulus test first, the angle normalised by the reference's two loops of f32 additions of tau.
 *   path      inverse_path_follow :627-695: 65 coarse points (strict <, the first minimum wins), eight refinement steps, tangent, normal, the 257-entry
 *             arc-length table of build_arc_length_table :575-591.
 *   envelope  :495-536, with the reference's t measured from the margin-shifted min_x.
 *   rotate    rotate_glyph_buffer: cosf / sinf once on the host, clamped +1 taps, new_w = ceil(..) + 1; skipped when |rotation| <= 0.001.
 *   blit      a source pixel with alpha 0 leaves the canvas pixel alone, any other replaces it; clipped to the canvas.
 * Path, envelope, rotate and blit are in the bit-exact class.  Arc and circular call atan2 per pixel: the device evaluates the f64 atan2 rounded once to
 * f32, which differs from glibc's atan2f by one ulp on rare arguments: +-1 on fewer than 0.1 % of channels (the LIBM class of the shape rasteriser).
 * Refused with PFX_ERR_INVALID, before the first launch and with outputs untouched: a NULL descriptor or required pointer; an unknown kind; a zero src_w or
 * src_h (buf_w, buf_h for the rotation; canvas_w, canvas_h for the placement); any float of the descriptor that is not finite, whatever kind says; a device pointer
 * that is not 4-byte aligned; an output that overlaps an input; out_bytes too small (host tier).  PFX_ERR_UNSUPPORTED, likewise: |circ_start_angle| above
 * 8 pi (the reference's loops do not end for a large one; the bound keeps them to a handful of steps); a source, planned output or canvas over the 256 Mpx
 * document limit (the circular output side ceil(2 (r + h) + 4) is unbounded in the reference). */
enum { PFX_TEXT_WARP_NONE = 0, PFX_TEXT_WARP_ARC = 1, PFX_TEXT_WARP_CIRCULAR = 2, PFX_TEXT_WARP_PATH = 3, PFX_TEXT_WARP_ENVELOPE = 4 };
typedef struct pfx_text_warp_desc {       /* TextWarp core.rs:171-294, plus the block raster's size (C has one namespace: pfx_text_warp is the host-tier call) */
    uint32_t src_w, src_h;
    int32_t  kind;                        /* PFX_TEXT_WARP_* */
    float    arc_bend, arc_hdist, arc_vdist;                  /* ArcWarp: bend, horizontal_distortion, vertical_distortion */
    float    circ_radius, circ_start_angle;                   /* CircularWarp */
    uint32_t circ_clockwise;
    uint32_t path_points;                 /* PathFollowWarp: control_points.len() and its first four */
    float    path[4][2];
    uint32_t top_points, bottom_points;   /* EnvelopeWarp: top_curve.len(), bottom_curve.len() and the first four of each */
    float    top[4][2], bottom[4][2];
} pfx_text_warp_desc;
typedef struct pfx_text_warp_geom {       /* what the warps' and the rotation's bounds loops derive */
    uint32_t out_w, out_h;
    int32_t  off_x, off_y;                /* of the output relative to the source's origin */
    uint32_t identity;                    /* 1: the output is the source */
    float    min_x, min_y, max_x, max_y;  /* the f32 bounds, margins included (arc, path, envelope, rotate); 0 otherwise */
} pfx_text_warp_geom;
int pfx_text_warp_plan(const pfx_text_warp_desc* warp, pfx_text_warp_geom* out);   /* host only, no context */
/* src_dev: src_w * src_h RGBA8; out_dev: out_w * out_h RGBA8 of the plan, every byte written (zeros where the reference skips); asynchronous */
int pfx_text_warp_dev(pfx_ctx* ctx, const pfx_text_warp_desc* warp, const void* src_dev, void* out_dev);
/* host tier: out_bytes >= out_w * out_h * 4 of the plan, which *plan_out (may be NULL) receives */
int pfx_text_warp(pfx_ctx* ctx, const pfx_text_warp_desc* warp, const uint8_t* src, uint8_t* out, size_t out_bytes, pfx_text_warp_geom* plan_out);
/* rotate_glyph_buffer of a buf_w * buf_h buffer by `angle` radians around pivot_xy (buffer coordinates; NULL = the centre).  |angle| <= 0.001 is the identity */
int pfx_text_rotate_plan(uint32_t buf_w, uint32_t buf_h, float angle, const float* pivot_xy, pfx_text_warp_geom* out);   /* host only, no context */
int pfx_text_rotate_dev(pfx_ctx* ctx, uint32_t buf_w, uint32_t buf_h, float angle, const float* pivot_xy, const void* src_dev, void* out_dev);
typedef struct pfx_text_block {           /* one block's tight raster on its way into the layer image */
    pfx_text_warp_desc warp;              /* its src_w * src_h is the raster */
    int32_t  off_x, off_y;                /* of the raster on the canvas */
    float    rotation;                    /* block.rotation, radians */
    uint32_t has_pivot;                   /* 0: rotate around the (warped) buffer's centre */
    float    pivot[2];                    /* rot_pivot, canvas coordinates */
    uint32_t canvas_w, canvas_h;
} pfx_text_block;
/* raster.rs:374-417: the warp, the rotation around the pivot, the blit into canvas_dev (canvas_w * canvas_h RGBA8, changed in place); asynchronous.  One
 * deviation: the reference adds the offsets in 32 bits (a debug build panics on overflow); here the sums are 64 bits wide and a block that lands outside
 * the canvas changes nothing */
int pfx_text_block_place_dev(pfx_ctx* ctx, const pfx_text_block* block, const void* src_dev, void* canvas_dev);

/* ================= gradient tool and perspective crop (ref: src/ui/panels/tools/behavior/raster/perspective_gradient.rs, tools/state.rs:1063-1171,
 * gradient_text/gradient_controls.rs:63-122) =================
 * The Gradient tool's drag frame, release and commit, and the PerspectiveCrop tool's re-sampling of every layer.  The gradient follows the reference's CPU
 * path :386-548 (start and end are NOT divided by the preview scale, unlike its WGSL branch) and that loop's own `t` formulas, not
 * GradientToolState::compute_t.  A drag frame stays on the device: pfx_gradient_render_dev, then pfx_flatten_preview_dev with that preview
 * (pfx_preview.is_eraser set in transparency mode).
 *   LUT      256 RGBA8 entries (1024 bytes), built on the host by pfx_gradient_build_lut as rebuild_lut does: no stop -> zeros; one stop -> its colour;
 *            else a stable sort by position, entry i at t = i / 255.0f: t <= first position -> first colour, t >= last -> last, else the FIRST pair with
 *            left <= t <= right, local_t = span > 0 ? (t - left) / span : 0, round(l * (1 - local_t) + r * local_t) per channel.
 *   render   per generated pixel (x, y) of gen_w x gen_h, gen = ceil(dim / preview_scale): px = x * scale + scale * 0.5 (f32), the selection byte at
 *            (x * scale, y * scale): 0 leaves (0, 0, 0, 0).  With d = end - start, len_sq = dx dx + dy dy, len = sqrt(len_sq), inv_len = len > 1e-6 ? 1 / len :
 *            0, inv_len_sq likewise on len_sq, u = d * inv_len, r = p - start:  linear raw = (rx dx + ry dy) * inv_len_sq, t = clamp(raw, 0, 1) or
 *            raw.rem_euclid(1) with repeat;  reflected t = 1 - |2 clamp(raw, 0, 1) - 1|, or m = raw.rem_euclid(2), t = m > 1 ? 2 - m : m;  radial raw =
 *            sqrt(rx rx + ry ry) * inv_len;  diamond raw = |rx ux + ry uy| * inv_len + |rx (-uy) + ry ux| * inv_len;  both then clamped or rem_euclid(1).
 *            idx = (t * 255.0) truncated (NaN -> 0), a = lut[idx].a, a selection byte below 255 gives a = a * sel / 255 in integers; a == 0 leaves
 *            (0, 0, 0, 0), else the LUT's rgb and a.  In transparency mode the LUT is first baked as :395-409 does (rgb = 255, a = lum * a / 255 with lum =
 *            (0.299 r + 0.587 g + 0.114 b) truncated): callers hand over the RAW LUT.  The optional second output is preview_flat_buffer :559-572, the
 *            premultiplied copy ((c * a + 128) / 255, alpha copied).  Every byte of both outputs is written.
 *   commit   the full-resolution preview onto the layer in place: preview alpha 0 keeps the pixel; transparency mode (is_eraser) a = round(max(cur_a *
 *            (1 - strength), 0) * 255), rgb kept; colour mode src-over in f32 :99-117, round() half away from zero.  The selection is not consulted.
 *   apply    render at preview_scale 1 plus commit in one kernel, no preview buffer; equals the two calls.
 *   crop     pfx_perspective_crop_plan :100-125: min / max over the four corners (TL, TR, BR, BL), clamped to [0, w] x [0, h], out = round(max - min); where
 *            the reference returns None (out_w < 2 or out_h < 2) the plan is PFX_OK with 0 x 0 and the crop calls return PFX_ERR_INVALID.  Per output pixel
 *            u = (ox + 0.5) / out_w, v likewise, src = (1-u)(1-v) c0 + u (1-v) c1 + u v c2 + (1-u) v c3, then bilinear_sample :186-233: x0 = clamp(floor(x),
 *            0, w - 1), x1 = min(x0 + 1, w - 1), fx = x - floor(x) from the unclamped coordinate, three lerps per channel each rounded to u8.  Every layer
 *            goes through the same map in one launch; outputs are out_w * out_h RGBA8 each, every byte written.
 * Everything is in the bit-exact class: single correctly rounded f32 operations (+, *, /, sqrt, an exact remainder), comparisons and integer arithmetic.
 * Refused with PFX_ERR_INVALID before anything is launched and with outputs untouched: a NULL descriptor, LUT or required pointer; a start or end that is
 * not finite; a shape outside PFX_GRADIENT_*; a mode other than 0 / 1; preview_scale 0 (pfx_gradient_apply_dev: other than 1); w * h outside the document
 * limit; an RGBA8 device pointer that is not 4-byte aligned; an output that overlaps an input or another output (the layer of commit / apply IS in place;
 * it must not overlap the preview or the selection); for the crop, a corner that is not finite, n_layers 0 or above PFX_CROP_MAX_LAYERS, a planned size
 * of 0 x 0.  The context-free helpers return PFX_ERR_INVALID (pfx_gradient_drag_scale: 1) for NULL or non-finite arguments.
 * `layer_ptrs_dev` / `cropped_ptrs_dev` are host arrays of device pointers, as pfx_flatten_dev's are. */
enum { PFX_GRADIENT_LINEAR = 0, PFX_GRADIENT_LINEAR_REFLECTED = 1, PFX_GRADIENT_RADIAL = 2, PFX_GRADIENT_DIAMOND = 3 };   /* GradientShape */
enum { PFX_GRADIENT_MODE_COLOR = 0, PFX_GRADIENT_MODE_TRANSPARENCY = 1 };                                                /* GradientMode */
enum { PFX_GRADIENT_PRESET_PRIMARY_SECONDARY = 0, PFX_GRADIENT_PRESET_BLACK_WHITE = 1, PFX_GRADIENT_PRESET_FOREGROUND_TRANSPARENT = 2,
       PFX_GRADIENT_PRESET_RAINBOW = 3 };                                                                                /* GradientPreset, less Custom */
#define PFX_GRADIENT_MAX_PRESET_STOPS 7
#define PFX_CROP_MAX_LAYERS 1024
typedef struct pfx_gradient_stop { float position; uint8_t color[4]; } pfx_gradient_stop;   /* GradientStop */
typedef struct pfx_gradient {
    float    start_x, start_y, end_x, end_y;   /* drag_start, drag_end in canvas coordinates */
    int32_t  shape;                            /* PFX_GRADIENT_* */
    int32_t  repeat;                           /* 0 / non-zero */
    int32_t  mode;                             /* PFX_GRADIENT_MODE_* */
    uint32_t preview_scale;                    /* >= 1; pfx_gradient_drag_scale while dragging, 1 on release */
} pfx_gradient;
/* host only, no context */
int pfx_gradient_build_lut(const pfx_gradient_stop* stops, uint32_t n_stops, uint8_t lut[1024]);   /* stops may be NULL when n_stops is 0 */
int pfx_gradient_preset_stops(int preset, const uint8_t primary[4], const uint8_t secondary[4], pfx_gradient_stop stops_out[PFX_GRADIENT_MAX_PRESET_STOPS],
                              uint32_t* n_stops_out);
int pfx_gradient_bake_eraser_lut(const uint8_t lut[1024], uint8_t baked[1024]);
uint32_t pfx_gradient_drag_scale(uint32_t w, uint32_t h);   /* :291-300: 1 up to 1 500 000 pixels, else max(2, ceil(sqrt(pixels / 1e6))) in f64 */
/* sel_dev: w * h bytes or NULL; preview_dev, premul_dev (may be NULL): gen_w * gen_h RGBA8; asynchronous on the context's stream */
int pfx_gradient_render_dev(pfx_ctx* ctx, const pfx_gradient* g, const uint8_t* lut, const void* sel_dev /* may be NULL */, uint32_t w, uint32_t h,
                            void* preview_dev, void* premul_dev /* may be NULL */);
int pfx_gradient_render(pfx_ctx* ctx, const pfx_gradient* g, const uint8_t* lut, const uint8_t* sel /* may be NULL */, uint32_t w, uint32_t h,
                        uint8_t* preview, uint8_t* premul /* may be NULL */);
int pfx_gradient_commit_dev(pfx_ctx* ctx, void* active_layer_dev, const void* preview_dev, uint32_t w, uint32_t h, int is_eraser);
int pfx_gradient_commit(pfx_ctx* ctx, uint8_t* active_layer_inout, const uint8_t* preview, uint32_t w, uint32_t h, int is_eraser);
int pfx_gradient_apply_dev(pfx_ctx* ctx, const pfx_gradient* g, const uint8_t* lut, const void* sel_dev /* may be NULL */, void* active_layer_dev, uint32_t w,
                           uint32_t h);
int pfx_perspective_crop_plan(const float corners_xy[8], uint32_t w, uint32_t h, uint32_t* out_w, uint32_t* out_h);   /* host only, no context */
int pfx_perspective_crop_dev(pfx_ctx* ctx, const float corners_xy[8], const void* const* layer_ptrs_dev, void* const* cropped_ptrs_dev, uint32_t n_layers,
                             uint32_t w, uint32_t h);
/* one layer through host buffers: cropped_bytes >= out_w * out_h * 4 of the plan */
int pfx_perspective_crop(pfx_ctx* ctx, const float corners_xy[8], const uint8_t* layer, uint8_t* cropped, size_t cropped_bytes, uint32_t w, uint32_t h);

/* ================= clone stamp, heal brush (live stroke), pencil (ref: src/ui/panels/tools/behavior/raster/clone_heal.rs) =================
 * The three dab-list tools that write into the preview layer besides the brush: clone_stamp_circle / _line :6-132, heal_circle / _line :141-292,
 * draw_pixel_and_get_bounds / draw_pixel_line_and_get_bounds :295-431.  A drag frame on the device is pfx_*_dev with that frame's points onto the resident
 * preview, then pfx_flatten_preview_dev; the release is pfx_stroke_commit_dev (commit_bezier_to_layer / commit_eraser_to_layer, the kernel of pfx_brush_commit).
 * The pointer-event smoothing of the callers is input handling: callers hand over the smoothed positions.  Smudge is not covered.
 *   lines    pfx_stroke_line_points, the stepping of clone_stamp_line / heal_line: d = end - start, distance = sqrt(dx dx + dy dy); below 0.1 the start point
 *            alone, with no canvas test; else steps = ceil(distance), t = i / steps for i in 0 ..= steps, p = start + d * t, kept only if x >= 0 && (x as u32) < w
 *            and likewise y.  The single circle of a stroke's first event has no such test: callers put that point into the list themselves.
 *            pfx_pencil_line_cells: Bresenham from floor(start) to floor(end) (err = dx - dy; e2 = 2 err; e2 > -dy steps x, e2 < dx steps y); only cells inside
 *            the canvas are listed.  Both fill at most `capacity` entries and always return the full count in *n_out: a caller whose buffer was too small comes
 *            back with room for *n_out.  PFX_ERR_INVALID: NULL n_out, a NULL list with a capacity, a non-finite coordinate, a bad size, a segment longer
 *            than 2^24 steps (pencil: a coordinate beyond +-2^24).
 *   shared   radius = size / 2.  Per dab the box is min = (c - radius).max(0) as u32, max = ((c + radius) as u32).min(dim - 1) with saturating casts (a dab left
 *            of the canvas still tests column 0).  Per pixel of the box: a selection byte of 0 skips; dist = sqrt(dx dx + dy dy) with d = pixel - centre;
 *            dist > radius skips.  Dabs apply in list order: `>=` below compares with the preview's current, quantised alpha byte.
 *   clone    geom = compute_brush_alpha(dist, radius) (the brush's: hardness, anti_aliased), geom < 0.01 skips; sx = round(x + offset_x) as i32 (half away
 *            from zero), sy likewise, a source outside the canvas skips; alpha = geom * (sa / 255.0); alpha >= old_a / 255.0 writes ((s / 255.0) * 255.0) as u8
 *            per colour channel — which need not be s — and (alpha * 255.0) as u8.  A source alpha of 0 over an empty preview writes rgb under alpha 0.
 *   heal     t = clamp(dist / radius, 0, 1), hard_t = clamp(hardness * 0.9 + 0.1, 0, 1); geom = 1 below hard_t, else s = (t - hard_t) / (1 - hard_t + 1e-6),
 *            geom = 1 - s s (3 - 2 s); geom < 0.01 skips.  seed = x * 1619 + y * 3929 wrapping in u32, angle_offset = seed as f32 / 4294967296.0 * TAU; for i in
 *            0..24: angle = angle_offset + (i as f32 / 24.0) * TAU, radii sample_radius * 0.75 then sample_radius: sx = round(x as f32 + cos(angle) * rr) as
 *            i32, sy with sin; samples inside the canvas add r, g, b to f32 sums and 1 to count.  count < 1 skips; geom >= old_a / 255.0 writes (sum / count)
 *            as u8 per channel and (geom * 255.0) as u8.
 *   pencil   per listed cell inside the canvas whose selection byte is not 0: color[3] >= old_a / 255.0 writes (c * 255.0) as u8 four times.  Idempotent: a
 *            cell listed twice is harmless.
 *   dirty    optional output {x0, y0, x1, y1}: Rect::union (componentwise min / max) of the rects the reference returns per dab, (min - 1 saturating, min(max
 *            + 2, dim)), computed on the host with the reference's float operations; zeros when nothing was listed.  A lone dab right of or below the canvas
 *            gives the reference's inverted rect (x0 >= x1): empty.  The pencil's box is taken over the listed in-canvas cells WITHOUT the selection (the
 *            device tier's selection lives on the device): it contains the reference's, and equals it without a selection.
 * All arithmetic is single correctly rounded f32 operations in the reference's order, except cos / sin: the f64 routine rounded once, within one ulp of the
 * reference's cosf / sinf, so that a heal pixel can differ only where a sample coordinate sits within that ulp of a rounding boundary.
 * n_points / n_cells == 0 is a no-op with PFX_OK (sizes, descriptor and buffers are still checked).  Refused with PFX_ERR_INVALID before anything is launched
 * and with nothing written: a NULL tool / colour, source, preview or list; a tool field, colour channel or point that is not finite; an RGBA8 device pointer
 * that is not 4-byte aligned; a preview that overlaps the source or the selection (pfx_stroke_commit_dev: a layer that overlaps the preview or the selection);
 * w * h outside the document limit. */
typedef struct pfx_clone_stamp_tool { float size, hardness; int32_t anti_aliased; float offset_x, offset_y; } pfx_clone_stamp_tool;   /* properties + clone_stamp_state.offset */
typedef struct pfx_heal_ring_tool { float size, hardness, sample_radius; } pfx_heal_ring_tool;                                       /* properties + content_aware_state */
/* host only, no context */
int pfx_stroke_line_points(float x0, float y0, float x1, float y1, uint32_t w, uint32_t h, float* points_xy, uint32_t capacity, uint32_t* n_out);
int pfx_pencil_line_cells(float x0, float y0, float x1, float y1, uint32_t w, uint32_t h, int32_t* cells_xy, uint32_t capacity, uint32_t* n_out);
/* source_dev, preview_dev: w * h RGBA8; sel_dev: w * h bytes or NULL; points_xy / cells_xy: host arrays of n pairs; asynchronous on the context's stream */
int pfx_clone_stamp_dev(pfx_ctx* ctx, const pfx_clone_stamp_tool* tool, const void* source_dev, void* preview_dev, const void* sel_dev /* may be NULL */, uint32_t w,
                        uint32_t h, const float* points_xy, uint32_t n_points, uint32_t dirty[4] /* may be NULL */);
int pfx_heal_ring_dev(pfx_ctx* ctx, const pfx_heal_ring_tool* tool, const void* source_dev, void* preview_dev, const void* sel_dev /* may be NULL */, uint32_t w,
                      uint32_t h, const float* points_xy, uint32_t n_points, uint32_t dirty[4] /* may be NULL */);
int pfx_pencil_dev(pfx_ctx* ctx, const float color[4], void* preview_dev, const void* sel_dev /* may be NULL */, uint32_t w, uint32_t h, const int32_t* cells_xy,
                   uint32_t n_cells, uint32_t dirty[4] /* may be NULL */);
/* the same through host buffers: the preview is changed in place */
int pfx_clone_stamp(pfx_ctx* ctx, const pfx_clone_stamp_tool* tool, const uint8_t* source, uint8_t* preview_inout, const uint8_t* sel /* may be NULL */, uint32_t w,
                    uint32_t h, const float* points_xy, uint32_t n_points, uint32_t dirty[4] /* may be NULL */);
int pfx_heal_ring(pfx_ctx* ctx, const pfx_heal_ring_tool* tool, const uint8_t* source, uint8_t* preview_inout, const uint8_t* sel /* may be NULL */, uint32_t w,
                  uint32_t h, const float* points_xy, uint32_t n_points, uint32_t dirty[4] /* may be NULL */);
int pfx_pencil(pfx_ctx* ctx, const float color[4], uint8_t* preview_inout, const uint8_t* sel /* may be NULL */, uint32_t w, uint32_t h, const int32_t* cells_xy,
               uint32_t n_cells, uint32_t dirty[4] /* may be NULL */);
/* the release of a stroke on device memory, the layer in place: what pfx_brush_commit does through host buffers (a blend_mode above 24 commits as Normal) */
int pfx_stroke_commit_dev(pfx_ctx* ctx, void* active_layer_dev, const void* preview_dev, const void* sel_dev /* may be NULL */, uint32_t w, uint32_t h,
                          uint8_t blend_mode, int is_eraser);

/* ================= line / curve tool (ref: src/ui/panels/tools/behavior/raster/bezier_math.rs, bezier_commit.rs) =================
 * rasterize_bezier :76-286 redraws a cubic Bezier on every pointer event: 20 to 5000 anti-aliased dots at a spacing of a tenth of the size, then up to two
 * arrowheads.  A drag frame on the device is pfx_line_render_dev onto the resident preview, then pfx_flatten_preview_dev with the tool's blend mode; the release
 * is pfx_stroke_commit_dev, and in mask-edit mode pfx_stroke_commit_mask_dev (commit_preview_to_layer_mask, bezier_commit.rs:229-295) on the w * h conceal bytes
 * that pfx_layer_set_mask takes.  Out of scope: showing a mask-target preview in the compositor (preview_targets_mask), the handle overlay, Shift-snapping and
 * the tool's stage machine, which are UI.
 *   bounds   get_bezier_bounds :41-73: min / max of the four control points, padded by size / 2 + 2, plus max(3 size, 8) + max(1.5 size, 4) with an Arrow end
 *            shape, clamped to [0, w] x [0, h]; four floats {min_x, min_y, max_x, max_y}, as the reference returns them.
 *   clear    last_bounds NULL: the whole preview is cleared.  Else min = floor(b.min).max(0) as u32, max = ceil(b.max).min(dim) as u32 and
 *            TiledImage::clear_region: every 64 x 64 chunk with cx in min_x / 64 .. ceil_div(max_x, 64), likewise cy, is cleared — whole chunks, not a
 *            rectangle.  Pixels of other chunks stay as they were, stale ones of an earlier frame included.
 *   dots     spacing = max(0.1 size, 0.5); steps = clamp(ceil((control net + chord) / spacing) as usize, 20, 5000); for i in 0 ..= steps: t = i / steps, the
 *            point of :27-38, the running f32 length over ALL samples; kept if x >= 0 && y >= 0 && (x as u32) < w && (y as u32) < h (saturating casts); a
 *            pattern (Dotted: on 0.5 size, off 1.5 size; Dashed: on 2 size, off 1.5 size) keeps it if length % (on + off) < on (fmodf; a NaN compares false);
 *            with a selection the byte AT THE DOT'S OWN CELL (x as u32, y as u32) must not be 0; Flat caps drop i == 0 and i == steps.
 *            Vec2::length is taken to be emath's x.hypot(y): that is a recollection, not verified against emath's source.  It enters `steps` and a pattern's
 *            phase only, never a pixel's arithmetic.
 *   dot      draw_bezier_circle_with_hardness :456-526, hardness 0.95: radius = size / 2, aa_pad = 1.5 below radius 1.5, else max(0.05 radius, 2) + 2 (1 without
 *            AA); box min = (c - outer).max(0) as u32, max = (ceil(c + outer) as u32).min(dim - 1).  Per pixel: a selection byte of 0 skips; d = pixel - centre
 *            (no half-pixel offset), dist = sqrt(dx dx + dy dy); compute_line_alpha (brush_render.rs:85-133: three regimes, radius < 1.5, < 3, else; without AA
 *            dist < radius); alpha <= 0 skips; pixel_alpha = alpha * (a / 255.0); written iff pixel_alpha > old_a / 255.0: ((c / 255.0) * 255.0) as u8 per colour
 *            channel — which need not be c — and (pixel_alpha * 255.0) as u8.
 *   arrows   :212-284, End first, then Start, after all dots: tangents 3 (p3 - p2) and 3 (p1 - p0), length floored at 0.001, tip advanced by 1.5 size, length
 *            max(3 size, 8), half width max(1.5 size, 4).  draw_filled_triangle :289-373: box padded by 1, pixel centres at + 0.5, three edge distances times
 *            the winding sign (a cross product of 0 counts as positive), min_dist < -1 skips, full alpha at >= 1, else smoothstep of (min_dist + 1) / 2; the
 *            same strict `>` write rule.
 *   plan     pfx_line_plan lists the dots after the canvas test, the pattern and the Flat-cap rule but BEFORE the selection test, and the triangles in draw
 *            order (tip, wing1, wing2 each; triangles_xy and n_triangles may be NULL).  It fills at most `capacity` dots and always reports the full count.
 *   mask     pfx_stroke_commit_mask[_dev]: per pixel whose selection byte is not 0 and whose preview alpha s is not 0: reveal ? old (255 - s) / 255 :
 *            old + (255 - old) s / 255, integer divisions.
 * All arithmetic is single correctly rounded f32 operations in the reference's order; no libm call per pixel: the result equals the reference's bit for bit.
 * Control points far outside the canvas are legal: the saturating casts and NaN rules above decide what is drawn, which may be nothing.
 * Refused with PFX_ERR_INVALID before anything is launched and with nothing written: a NULL tool, preview or mask; a control point or a size that is not
 * finite (any finite size is taken, as by the clone stamp); an enum out of range; a last_bounds value that is not finite; an RGBA8 device pointer that is not
 * 4-byte aligned; a preview that overlaps the selection or the mask; w * h outside the document limit. */
typedef struct pfx_line_tool {
    float    p[8];        /* control points p0..p3, canvas pixels */
    float    size;        /* properties.size */
    uint8_t  color[4];    /* Color32 */
    int32_t  pattern;     /* 0 solid, 1 dotted, 2 dashed   (LinePattern) */
    int32_t  cap_style;   /* 0 round, 1 flat               (CapStyle) */
    int32_t  end_shape;   /* 0 none, 1 arrow               (LineEndShape) */
    int32_t  arrow_side;  /* 0 end, 1 start, 2 both        (ArrowSide) */
    int32_t  anti_alias;
} pfx_line_tool;
/* host only, no context */
int pfx_line_bounds(const pfx_line_tool* tool, uint32_t w, uint32_t h, float bounds[4]);
int pfx_line_plan(const pfx_line_tool* tool, uint32_t w, uint32_t h, float* dots_xy, uint32_t capacity, uint32_t* n_out, float triangles_xy[12] /* may be NULL */,
                  uint32_t* n_triangles /* may be NULL */);
/* preview_dev: w * h RGBA8, changed in place; sel_dev: w * h bytes or NULL; asynchronous on the context's stream */
int pfx_line_render_dev(pfx_ctx* ctx, const pfx_line_tool* tool, void* preview_dev, const void* sel_dev /* may be NULL */, uint32_t w, uint32_t h,
                        const float last_bounds[4] /* NULL: first frame, clear all */, float bounds_out[4] /* may be NULL */);
int pfx_line_render(pfx_ctx* ctx, const pfx_line_tool* tool, uint8_t* preview_inout, const uint8_t* sel /* may be NULL */, uint32_t w, uint32_t h,
                    const float last_bounds[4] /* NULL: first frame, clear all */, float bounds_out[4] /* may be NULL */);
/* conceal: w * h bytes, changed in place */
int pfx_stroke_commit_mask_dev(pfx_ctx* ctx, void* conceal_dev, const void* preview_dev, const void* sel_dev /* may be NULL */, uint32_t w, uint32_t h, int reveal);
int pfx_stroke_commit_mask(pfx_ctx* ctx, uint8_t* conceal_inout, const uint8_t* preview, const uint8_t* sel /* may be NULL */, uint32_t w, uint32_t h, int reveal);

/* ================= histogram, per-band Hue/Saturation, colour range (ref: src/ops/adjustments.rs :883-937, :1594-1674, :1684-1792) =================
 * The last pixel loops of the colour dialogs: the Levels dialog's histograms, Hue/Saturation with six colour bands, and the Colour Range dialog's mask.
 * Images are w * h RGBA8; masks are w * h bytes, 0 = unselected, anything else = selected (the reference also takes a smaller mask; this surface does not).
 * The `_dev` forms take device pointers (an RGBA8 one 4-byte aligned) and are asynchronous on the context's stream unless stated; the others stage host
 * buffers.  A NULL context, a zero side, more than 256 Mpx, a NULL required pointer and the overlaps named below are PFX_ERR_INVALID before any launch; a
 * refused call leaves its outputs untouched.
 *
 * compute_histogram: hist_out = R[256], G[256], B[256], L[256] counts in host memory; the call waits for the device (as pfx_selection_bounds_dev does).  A
 * pixel is counted when sel is NULL or its mask byte is not 0, and its alpha is not 0.  L = min(round(0.2126f * r + 0.7152f * g + 0.0722f * b), 255), f32, left
 * to right, unfused, half away from zero.  Exact: integer sums.  The counters are 32-bit: 2^32 pixels would wrap one, the 256 Mpx document limit is below it. */
int pfx_histogram(pfx_ctx* ctx, const uint8_t* image, uint32_t w, uint32_t h, const uint8_t* sel /* may be NULL */, uint32_t hist_out[1024]);
int pfx_histogram_dev(pfx_ctx* ctx, const void* image_dev, uint32_t w, uint32_t h, const void* sel_dev /* may be NULL */, uint32_t hist_out[1024]);
/* hue_saturation_per_band_from_flat: bands[0 .. 5] = Reds, Yellows, Greens, Cyans, Blues, Magentas, centred on 0, 60, .. 300 degrees; a pixel's hue is in a
 * band with weight 1 within 30 degrees of the centre, falling linearly to 0 at 45.  Hue shifts, saturation factors and lightness offsets of the global
 * sliders and of every band of weight above 0 add up, in band order.  Bit-exact class; alpha is untouched; mask byte 0 copies the source pixel.  sparse_mode as
 * pfx_adjust: the dialog's path is PFX_FROM_FLAT; PFX_DENSE skips the chunk zeroing; PFX_IN_PLACE works too (the bank's own chunk code runs here), though the
 * reference has no such caller.  bands is host memory in both forms.  result == image (in place) is allowed, any other overlap of result with image or sel is
 * refused, as is a slider value that is not finite.  Not part of pfx_chain_dev. */
typedef struct pfx_hue_band { float hue, saturation, lightness; } pfx_hue_band;   /* HueBandAdjust: degrees -180 .. 180, percent -100 .. 100, percent -100 .. 100 */
int pfx_hsl_bands(pfx_ctx* ctx, const uint8_t* image, uint8_t* result, uint32_t w, uint32_t h, float global_hue, float global_sat, float global_light,
                  const pfx_hue_band bands[6], const uint8_t* sel /* may be NULL */, int sparse_mode);
int pfx_hsl_bands_dev(pfx_ctx* ctx, const void* image_dev, void* result_dev, uint32_t w, uint32_t h, float global_hue, float global_sat, float global_light,
                      const pfx_hue_band bands[6], const void* sel_dev /* may be NULL */, int sparse_mode);
/* select_color_range: the new mask is 0 where alpha is 0, where the HSL saturation is below sat_min, or where the hue is further than hue_tolerance_deg (at
 * least 0.36 degrees) from hue_center_deg around the wheel; elsewhere 255 * (1 - (distance / tolerance) ^ (1 / max(clamp(fuzziness, 0.001, 1), 0.01))),
 * truncated.  It is combined with base_sel (NULL = all zero) by THIS function's rule, not apply_selection_shape's: combine_mode 0 replace, 1 add = max(new,
 * base), 2 subtract = base saturating-minus new, 3 intersect = new * base / 255 in integers.  Every byte of sel_out is written; sel_out == base_sel (in place)
 * is allowed, any other overlap of sel_out is refused.  The power is a libm call: off the few pixels where one f32 ulp of it moves the byte the result equals
 * the reference's on glibc; on those it is within 1 (tests/colorrange_model.py).
 * Also PFX_ERR_INVALID: combine_mode above 3, a setting that is not finite, hue_center_deg outside [0, 360] — beyond that range the reference's folded distance
 * can go negative and its powf return NaN; the dialog's slider runs from 0 to 360 (src/ui/dialogs/core/selection.rs:58), so this refuses nothing it can send. */
int pfx_select_color_range(pfx_ctx* ctx, const uint8_t* image, const uint8_t* base_sel /* may be NULL */, uint32_t w, uint32_t h, float hue_center_deg,
                           float hue_tolerance_deg, float sat_min, float fuzziness, uint8_t combine_mode, uint8_t* sel_out);
int pfx_select_color_range_dev(pfx_ctx* ctx, const void* image_dev, const void* base_sel_dev /* may be NULL */, uint32_t w, uint32_t h, float hue_center_deg,
                               float hue_tolerance_deg, float sat_min, float fuzziness, uint8_t combine_mode, void* sel_out_dev);

/* ================= background removal around the model (ref: src/ops/ai.rs :615-949, :1324-1445) =================
 * Filter -> Remove Background runs a segmentation model in the caller's ONNX runtime; these are the reference's own pixel loops in front of the model and
 * behind it, so that the layer, the model's input tensor, its outputs and the layer's new alpha stay on the device.  Images are w * h RGBA8; grey images and
 * mattes are one byte per pixel; values are f32.  The `_dev` forms take device pointers (an RGBA8 or f32 one 4-byte aligned) and are asynchronous on the context's
 * stream unless stated; the others stage host buffers.  Bit-exact class: f32 with one rounding per operation, glibc's expf, the bit-exact Lanczos3 resize.
 * PFX_ERR_INVALID before any launch, outputs untouched: a NULL context, settings or required pointer; a zero side or more than 256 Mpx (values: 256 M); a
 * tensor_size of 0; a threshold or edge_feather that is not finite; an is_probability outside -1 .. 1; a misaligned RGBA8 / f32 device pointer; an output that
 * shares a byte with an input, except result == image where stated.  PFX_ERR_UNSUPPORTED: |mask_expansion| or |expansion| above 64, fill_holes above 64,
 * ceil(edge_feather) above 256 (the dialog's sliders stop at 10, 20 and 20), and a resize in which one 64-column output tile reaches more than 2048 source
 * columns (a model output wider than 2048 shrunk to a few dozen pixels).
 *
 * Tensor (preprocess_image): imageops::resize(image, S, S, Lanczos3) — pfx_resize_image, the same-size copy included — then plane c of the [3][S][S] tensor =
 * ((p as f32 / 255.0) - MEAN[c]) / STD[c] for c = R, G, B; MEAN = {0.485, 0.456, 0.406}, STD = {0.229, 0.224, 0.225}; alpha is ignored.
 * Score (is_probability_space, mask_confidence_score) of n_values f32: step = max(n / 10000, 1); min / max over the indices 0, step, 2 step, .. ignoring NaN, from
 * f32::MAX / f32::MIN; is_probability = min >= -0.05 && max <= 1.05; prob = is_probability ? clamp(v, 0, 1) : 1 / (1 + expf(-v)), a NaN stays NaN; a value is
 * decisive when prob as f64 lies outside 0.1 ..= 0.9, a NaN counts; confidence = decisive / n, 0.0 for n = 0 (with is_probability 0).  The call waits for its
 * 16 bytes of result, as pfx_histogram_dev does.  Exact.
 * Pick (ModelProfile::detect, preferred_output_index, the selection :1356-1380): host only, no context.  confidence[i] < 0 (or NaN) marks an output the caller
 * could not read; it is skipped.  Among the outputs within 0.01 of the best confidence the profile's preferred index wins — the last output of a 1024 x 1024
 * model with five or more outputs (BiRefNet), else the first — otherwise the highest confidence, the last of equal ones.  PFX_ERR_INVALID for NULL, n_outputs 0
 * or no usable output.
 * Post-process (postprocess_mask) on prob_w x prob_h values: (1) byte: prob as above with the given is_probability (-1: detected on these values, which waits
 * for the device), then with smooth_edges r = 1 / (1 + expf(-(prob - threshold) * 12.0)), (r * 255.0).clamp(0, 255) as u8 (truncating, NaN -> 0), else prob >=
 * threshold ? 255 : 0.  (2) expansion: |mask_expansion| iterations, each reading the previous image whole: dilating, a pixel with centre < 128 becomes the maximum
 * of its in-image 3 x 3 neighbourhood; eroding, one with centre > 128 the minimum; 128 never changes and a pixel that has crossed 128 is frozen, so n iterations
 * are not a (2n + 1)^2 window.  (3) close: fill_holes dilations, then fill_holes erosions.  (4) imageops::resize(GrayImage, w, h, Lanczos3) unless the sizes are
 * equal.  (5) feather, if edge_feather > 0.5: r = max(ceil(edge_feather), 1), a row pass then a column pass of (sum / count) as u8 over 2r + 1 edge-clamped
 * samples.  (6) a' = ((a / 255.0) * (m / 255.0) * 255.0).clamp(0, 255) as u8; the rgb is copied.
 * pfx_matte_postprocess[_dev] is steps 1 - 6 and equals the stage calls composed; matte (may be NULL) receives the final w * h matte.  result == image (in place)
 * is allowed there and in pfx_matte_apply_dev; no other overlap of an output is.  pfx_matte_expand_dev: a negative expansion erodes, 0 copies.
 * pfx_matte_feather_dev copies at edge_feather <= 0.5. */
typedef struct pfx_matte_settings { float threshold, edge_feather; int32_t mask_expansion, smooth_edges; uint32_t fill_holes; } pfx_matte_settings;  /* RemoveBgSettings */
int pfx_matte_tensor(pfx_ctx* ctx, const uint8_t* image, uint32_t w, uint32_t h, uint32_t tensor_size, float* tensor /* 3 * tensor_size^2 */);
int pfx_matte_tensor_dev(pfx_ctx* ctx, const void* image_dev, uint32_t w, uint32_t h, uint32_t tensor_size, void* tensor_dev);
int pfx_matte_score(pfx_ctx* ctx, const float* values, size_t n_values, int32_t* is_probability, double* confidence);
int pfx_matte_score_dev(pfx_ctx* ctx, const void* values_dev, size_t n_values, int32_t* is_probability /* host */, double* confidence /* host */);
int pfx_matte_pick_output(uint32_t input_w, uint32_t input_h, const double* confidence, uint32_t n_outputs, uint32_t* picked);
int pfx_matte_byte_dev(pfx_ctx* ctx, const void* values_dev, uint32_t prob_w, uint32_t prob_h, int32_t is_probability, const pfx_matte_settings* settings, void* grey_dev);
int pfx_matte_expand_dev(pfx_ctx* ctx, const void* grey_dev, uint32_t prob_w, uint32_t prob_h, int32_t expansion, void* grey_out_dev);
int pfx_matte_resize_dev(pfx_ctx* ctx, const void* grey_dev, uint32_t prob_w, uint32_t prob_h, void* matte_dev, uint32_t w, uint32_t h);
int pfx_matte_feather_dev(pfx_ctx* ctx, const void* grey_dev, uint32_t w, uint32_t h, float edge_feather, void* matte_dev);
int pfx_matte_apply_dev(pfx_ctx* ctx, const void* image_dev, const void* matte_dev, uint32_t w, uint32_t h, void* result_dev);
int pfx_matte_postprocess_dev(pfx_ctx* ctx, const void* values_dev, uint32_t prob_w, uint32_t prob_h, int32_t is_probability, const void* image_dev, uint32_t w, uint32_t h,
                              const pfx_matte_settings* settings, void* result_dev, void* matte_dev /* may be NULL */);
int pfx_matte_postprocess(pfx_ctx* ctx, const float* values, uint32_t prob_w, uint32_t prob_h, int32_t is_probability, const uint8_t* image, uint32_t w, uint32_t h,
                          const pfx_matte_settings* settings, uint8_t* result, uint8_t* matte /* may be NULL */);

#ifdef __cplusplus
}
#endif
#endif /* PFX_H */
