// pfx_kernels.h — launch entry points of the gfx950 kernels (internal; the public ABI is include/pfx.h).
// Every launcher enqueues on `stream`, never synchronises, and returns hipGetLastError().
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { PFXK_LAYER_RASTER = 0, PFXK_ADJ_EXPOSURE = 1, PFXK_ADJ_BRIGHTNESS_CONTRAST = 2, PFXK_ADJ_INVERT = 3,
       PFXK_ADJ_CHANNEL_MIXER = 4 };

// one entry of the layer stack, bottom -> top (32 bytes, read with scalar loads: uniform per wave)
typedef struct pfxk_layer_desc {
    const uint8_t* pixels; // device RGBA8, tight w*h*4 (NULL for adjustment layers)
    const uint8_t* mask;   // device w*h "conceal" bytes or NULL
    float    opacity;      // as stored (unclamped: the >= 1.0 fast path looks at the raw value)
    uint32_t mode;         // BlendMode::to_u8
    uint32_t kind;         // PFXK_LAYER_RASTER or PFXK_ADJ_*
    uint32_t adj_off;      // adjustment layers: offset (floats) of the 16 parameters in the adj table; raster layers: bit pattern of
                           // opacity.clamp(0, 1) (the streaming compositor kernels read this instead of clamping per wave and layer)
} pfxk_layer_desc;

// parameter block of the pointwise kernels (passed by value: lands in SGPRs)
typedef struct pfxk_params { float p[12]; } pfxk_params;

// ids mirror include/pfx.h (pfx_adjust_op / pfx_rhai_op); static_asserts in pfx_api.cpp keep them in sync
enum { PFXK_OP_INVERT = 0, PFXK_OP_INVERT_ALPHA, PFXK_OP_SEPIA, PFXK_OP_BRIGHTNESS_CONTRAST, PFXK_OP_HSL,
       PFXK_OP_EXPOSURE, PFXK_OP_HIGHLIGHTS_SHADOWS, PFXK_OP_TEMPERATURE_TINT, PFXK_OP_THRESHOLD, PFXK_OP_POSTERIZE,
       PFXK_OP_COLOR_BALANCE, PFXK_OP_GRADIENT_MAP, PFXK_OP_BLACK_AND_WHITE, PFXK_OP_VIBRANCE, PFXK_OP_LUT_RGBA,
       PFXK_OP_DESATURATE, PFXK_OP_COUNT };
enum { PFXK_RHAI_INVERT = 0, PFXK_RHAI_DESATURATE, PFXK_RHAI_SEPIA, PFXK_RHAI_SEPIA_STRENGTH,
       PFXK_RHAI_BRIGHTNESS_CONTRAST, PFXK_RHAI_HSL, PFXK_RHAI_EXPOSURE, PFXK_RHAI_LEVELS, PFXK_RHAI_COUNT };

// ---- k_flatten.hip ----
// fast_div: 1 = shared-reciprocal division (bit-identical to '/' for opacities that are 0 or >= 2^-40), 0 = plain '/'
// tool preview layer folded into the active layer (canvas_state.rs:541-548,593-658); all pointers are device memory
typedef struct pfxk_preview {
    const uint8_t* pixels;              // w*h*4, NULL = no preview
    const uint8_t* chunk_present;       // per 64x64 chunk: the preview TiledImage has this chunk
    const uint8_t* layer_chunk_present; // per chunk: the ACTIVE LAYER has this chunk (a missing chunk reads as (0,0,0,0))
    uint32_t active_pos;                // position of the active layer in d_layers, 0xFFFFFFFF = not in the stack (hidden)
    uint32_t mode, is_eraser, replaces; // preview_blend_mode (normalised 0..24), preview_is_eraser, preview_replaces_layer
} pfxk_preview;
// dirty rectangle: composite only [x0, x0+rw) x [y0, y0+rh) into a compact rw x rh destination (rw == 0: whole canvas)
typedef struct pfxk_region { uint32_t x0, y0, rw, rh; } pfxk_region;
// Candidate "reset" layers of a stack (positions in the descriptor array, ascending): layers whose result does not depend on what is
// below them wherever their alpha qualifies — kind 0: Overwrite, alpha != 0 (canvas_state.rs:1275-1281); kind 1: Normal at
// opacity >= 1, alpha == 255 (:1258).  The compositor skips the layers below a pixel's topmost reset (k_flatten.hip, flatten_dle_kernel).
#define PFXK_DLE_MAX 4
#define PFXK_DESC_PAD 16 /* copies of the last layer descriptor the host appends (valid indices end at n + PFXK_DESC_PAD - 1): the shipped compositor loops (k_flatten.hip: srt_layers_pipe, srt_early_pipe) read up to descriptor n and fetch nothing through it; the PFX_SRT_PIPE 0 and TR builds' srt_layers reads up to n + 2, srt_early<NB> up to n + 2 NB - 2 */
typedef struct pfxk_dle_cands { uint32_t n; uint32_t layer[PFXK_DLE_MAX]; uint32_t kind[PFXK_DLE_MAX]; uint32_t stats; /* set by the launcher from the plan */ } pfxk_dle_cands;
// What pfxk_flatten launches, decided by pfx_int_flatten_plan (pfx_flatten.cpp) and by nothing else.  The schedule and the re-deal plan are kernel arguments of the
// elimination kernels (k_flatten.hip).
typedef struct pfxk_dle_sched { uint32_t wavesA, UA, wavesB, UB, UC; } pfxk_dle_sched; // waves [0, wavesA) own UA units each, the next wavesB UB, the rest UC
typedef struct pfxk_dle_plan { uint32_t s1, seg; } pfxk_dle_plan; // re-deal attempts in front of layers s1, s1 + seg, s1 + 2 seg, ... (seg == 0: none)
// kernel: the low four bits of `path`, and which of the fields below count.  path: the kernel, then the template kernel's GENERAL and F arguments (the streaming and
// elimination kernels always run under the fast-division precondition, without GENERAL), a dirty rectangle, a tool preview, the per-chunk start table
enum { PFXK_FLATTEN_TEMPLATE = 0, PFXK_FLATTEN_STREAM = 1, PFXK_FLATTEN_DLE = 2, PFXK_FLATTEN_SRT = 3,
       PFXK_FLATTEN_GENERAL = 1 << 4, PFXK_FLATTEN_FAST_DIV = 1 << 5, PFXK_FLATTEN_REGION = 1 << 6, PFXK_FLATTEN_PREVIEW = 1 << 7, PFXK_FLATTEN_CHUNK_START = 1 << 8 };
typedef struct pfxk_flatten_plan {
    int kernel, path;
    int general, fast_div;   // _TEMPLATE: flatten_kernel<GENERAL, F>
    int px, nb;              // _STREAM: flatten_stream_kernel<PX, NB>; _DLE: flatten_dle_kernel<PX, ring, 1, NB>; _SRT: flatten_srt_kernel<PX> (nb 0)
    int ring;                // _DLE: RING_LOG2
    int diag;                // _SRT: 0, or the diagnostic build `stats` asks for: 2 = the load stream without the arithmetic, 4 = per-phase wave clocks
    uint32_t grid;           // _TEMPLATE, _STREAM: workgroups of 256 lanes
    uint32_t waves;          // _DLE, _SRT: one-wave workgroups, sched.wavesA + sched.wavesB + what the units left over need
    uint32_t stats;          // _DLE, _SRT: pfxk_dle_cands.stats (pfx_tune "dle_stats")
    pfxk_dle_sched sched;    // _DLE, _SRT
    pfxk_dle_plan redeal;    // _SRT
} pfxk_flatten_plan;
// launches what *plan says; the chunk-activity pre-pass of a GENERAL launch runs first unless the caller filled d_chunk_active itself
hipError_t pfxk_flatten(hipStream_t stream, const pfxk_flatten_plan* plan, const pfxk_layer_desc* d_layers, uint32_t n_layers, const float* d_adj_table,
                        uint8_t* d_chunk_active, int chunk_active_ready, uint32_t w, uint32_t h, uint8_t* d_dst, const pfxk_preview* preview /* may be NULL */,
                        const pfxk_region* region /* may be NULL */, const pfxk_dle_cands* cands /* read by _DLE and _SRT */,
                        const uint8_t* d_chunk_start /* may be NULL: per-chunk first layer that can show (pfxk_chunk_start) */);
// per-chunk alpha summary of a stored layer (bit 0: all 255, bit 1: none 0) over the chunk rectangle [cx0, cx0+ncx) x [cy0, cy0+ncy), and the
// per-chunk start table of a stack (want[k]: 1 = Normal at opacity >= 1 needs bit 0, 2 = Overwrite needs bit 1, 0 = layer k never resets)
hipError_t pfxk_chunk_alpha_flags(hipStream_t s, const uint8_t* d_px, uint32_t w, uint32_t h, uint32_t cx0, uint32_t cy0, uint32_t ncx, uint32_t ncy,
                                  uint8_t* d_flags);
hipError_t pfxk_chunk_start(hipStream_t s, const uint8_t* const* d_flag_ptrs, const uint8_t* d_want, uint32_t n_layers, uint32_t n_chunks,
                            uint8_t* d_start, uint32_t* useful_pinned /* may be NULL: receives `tag` if any chunk starts above layer 0 */, uint32_t tag);
/* samples 256 units against the topmost reset candidate; *verdict_pinned = tag | 0x80000000 when at least half start at it outright (k_flatten.hip: dle_probe_kernel) */
hipError_t pfxk_dle_probe(hipStream_t s, const pfxk_layer_desc* d_layers, uint32_t cand_layer, uint32_t cand_kind, uint32_t n_px, uint32_t* verdict_pinned, uint32_t tag);
hipError_t pfxk_flatten_dle_stats(unsigned long long* out16 /* may be NULL */, int reset); // synchronises the device
// out[0] += byte values for which a typed UNORM8 store of RN(k / 255) does not write k or the typed load does not return RN(k / 255)
hipError_t pfxk_unorm_store_check(hipStream_t s, uint8_t* d_scratch1k, unsigned long long* d_out);
// counts (into *d_out) operand pairs for which the shared-reciprocal division differs from the IEEE divide
hipError_t pfxk_rdiv_check(hipStream_t s, uint64_t seed, uint32_t blocks, uint32_t iters, unsigned long long* d_out);
// the same count with explicit biased-exponent ranges [lo, hi] (1 .. 254) for numerator and denominator (k_effects2.hip); a quarter of the numerators are 0
hipError_t pfxk_rdiv_check_range(hipStream_t s, uint64_t seed, uint32_t blocks, uint32_t iters, uint32_t num_lo, uint32_t num_hi, uint32_t den_lo,
                                 uint32_t den_hi, unsigned long long* d_out);
hipError_t pfxk_round_pack_check(hipStream_t s, unsigned long long* d_out /* [2]: mismatches, signalling-NaN mismatches */);

// ---- k_gauss.hip ---- (d_wts_tap0 points at tap 0 of a device array with pfxk_gauss_weight_pad() zeros on both sides)
int        pfxk_gauss_max_radius(void);
int        pfxk_gauss_weight_pad(void);
void       pfxk_gauss_set_v_config(int cfg); // tuning knob, 0 = shipped
/* pure: the vertical pass's tile for a radius under a value of that knob (low byte: 1 .. 4 force a shape up to radius 340, 0 = by radius, others = config 0).
   Returns the config index 0 .. 4; fills in (each may be NULL) the tile's columns, its output rows and the LDS bytes the launch requests (refused above 160 KiB) */
int        pfxk_gauss_v_tile(int radius, int cfg_knob, int* tx, int* rows, size_t* lds_bytes);
size_t     pfxk_gauss_h_lds_bytes(int radius); // pure: the LDS bytes the horizontal pass's launch requests
void       pfxk_gauss_set_mfma_segments(int n); // tuning knob of the matrix-core kernel, 0 = automatic
/* bit-exact mode, radii 1 .. pfxk_gauss_fused_exact_max_radius() (the compiled limit): both passes in one kernel, the f32 intermediate in an LDS ring (k_gauss_exact.hip);
   _enabled: the process-wide A/B knob, read where the path is chosen (pfx_gauss.cpp), not by the launchers */
void pfxk_gauss_set_fused_exact(int on);
int pfxk_gauss_fused_exact_enabled(void);
int pfxk_gauss_fused_exact_max_radius(void);
/* one-channel form (w % 4 == 0, tight rows, radii 1 .. pfxk_gauss_fused_exact_max_radius()): element by element what one channel of pfxk_gauss_fused_exact gives on (a, a, a, a) */
hipError_t pfxk_gauss_plane_exact(hipStream_t stream, const uint8_t* d_src, uint8_t* d_dst, const float* d_wts_tap0, int radius, uint32_t w, uint32_t h);
hipError_t pfxk_gauss_fused_exact(hipStream_t stream, const uint8_t* d_src, uint8_t* d_dst, const float* d_wts_tap0, int radius, uint32_t w, uint32_t h,
                                  int epilogue /* 0 the blur, 1 sharpen, 2 glow: combine with the source in the store (k_effects.hip: combine_kernel) */, float p0, const uint8_t* d_mask);
hipError_t pfxk_gauss_h(hipStream_t stream, const uint8_t* d_src, float* d_tmp, const float* d_wts_tap0, int radius,
                        uint32_t w, uint32_t h, int exact);
int        pfxk_gauss_mfma_max_radius(void);
int        pfxk_gauss_mfma_wlen(void);
int        pfxk_gauss_mfma_woff(void);
hipError_t pfxk_gauss_mfma(hipStream_t stream, const uint8_t* d_src, uint8_t* d_dst, const uint16_t* d_wsplit,
                           int radius, float inv_scale2, float bias_c, float bias_single, uint32_t w, uint32_t h, uint32_t first_row, int n_cus);
hipError_t pfxk_gauss_mfma_chain(hipStream_t stream, const uint8_t* d_src, uint8_t* d_dst, const uint16_t* d_wsplit, int radius, float inv_scale2, float bias_c,
                                 float bias_single, uint32_t w, uint32_t h, uint32_t first_row, int n_cus, const struct pfxk_chain* chain);
void       pfxk_gauss_set_mfma_cols64(int mask); // bit 0 / 1 / 2: launches with 4 / 6 / 8 K blocks (sigma <= 5.3 / 10.6 / 16) on 64-column strips instead of 32-column ones (bit-identical results)
void       pfxk_gauss_set_mfma_parts(int weight_parts, int h_parts); // f16 pieces per weight (2 or 1) / per horizontal result (2, or 1 with single weights)
hipError_t pfxk_gauss_v(hipStream_t stream, const float* d_tmp, uint8_t* d_dst, const float* d_wts_tap0, int radius,
                        uint32_t w, uint32_t h, int exact);

// ---- chains of pointwise ops (round 6: pfx_chain_dev) ----
// op[i] = a PFXK_OP_* id (ops::adjustments flavour) or PFXK_CHAIN_RHAI | a PFXK_RHAI_* id (Rhai-inline flavour); P[i] = its prepared parameter block;
// lut_slot[i] = which 1024-byte table of the chain's LUT buffer the op reads (ops without a table: 0).
#define PFXK_CHAIN_MAX 8
#define PFXK_CHAIN_LUTS 4
#define PFXK_CHAIN_RHAI 0x100u
typedef struct pfxk_chain {
    uint32_t n, n_luts;
    uint32_t op[PFXK_CHAIN_MAX];
    uint32_t lut_slot[PFXK_CHAIN_MAX];
    pfxk_params P[PFXK_CHAIN_MAX];
} pfxk_chain;
// every op of the chain on every pixel, one pass over memory (d_src == d_dst allowed); d_luts: n_luts x 1024 bytes
hipError_t pfxk_pointwise_chain(hipStream_t s, const uint8_t* d_src, uint8_t* d_dst, const uint8_t* d_luts, const pfxk_chain* C, uint32_t w, uint32_t h);
// the bit-exact fused Gaussian with the chain applied to every blurred pixel in its store (epilogue 3 of pfxk_gauss_fused_exact)
hipError_t pfxk_gauss_fused_exact_chain(hipStream_t stream, const uint8_t* d_src, uint8_t* d_dst, const float* d_wts_tap0, int radius, uint32_t w, uint32_t h,
                                        const pfxk_chain* C, const uint8_t* d_luts);

// ---- k_pointwise.hip ---- (d_lut: 1024 readable bytes when the op uses a LUT)
hipError_t pfxk_adjust(hipStream_t s, const uint8_t* d_src, uint8_t* d_dst, const uint8_t* d_mask, const uint8_t* d_lut,
                       int op, const pfxk_params* P, int sparse_mode, uint32_t w, uint32_t h);
hipError_t pfxk_rhai_adjust(hipStream_t s, uint8_t* d_px, const uint8_t* d_lut, int op, const pfxk_params* P,
                            uint32_t w, uint32_t h);

// ---- k_tiled.hip ----
hipError_t pfxk_chunk_populated(hipStream_t s, const uint8_t* d_src, uint32_t w, uint32_t h, uint8_t* d_populated);
hipError_t pfxk_tiled_roundtrip(hipStream_t s, const uint8_t* d_src, uint8_t* d_dst, uint32_t w, uint32_t h);
// TiledImage <-> flat: packed 64x64 chunks + a slot table per canvas chunk (0xffffffff = no chunk); ref: tiled_image.rs:50-104,271-293
hipError_t pfxk_chunks_import(hipStream_t s, const uint8_t* d_packed, const uint32_t* d_slot, uint32_t w, uint32_t h, uint8_t* d_flat);
hipError_t pfxk_chunks_export(hipStream_t s, const uint8_t* d_flat, const uint32_t* d_slot, uint32_t w, uint32_t h, uint8_t* d_packed);
// dst = mask ? blurred : src   (blur_with_selection's copy-back, ref: src/ops/filters.rs:186-200)
hipError_t pfxk_select_by_mask(hipStream_t s, const uint8_t* d_src, const uint8_t* d_fx, const uint8_t* d_mask,
                               uint8_t* d_dst, uint32_t w, uint32_t h);
// per-channel min/max over selected pixels with alpha != 0 -> out[6] = {minR,maxR,minG,maxG,minB,maxB} (u32)
hipError_t pfxk_minmax_rgb(hipStream_t s, const uint8_t* d_src, const uint8_t* d_mask, uint32_t w, uint32_t h,
                           uint32_t* d_out6);

// ---- k_stencil.hip ---- box blur / median / pixelate.  Which kernel runs is chosen in pfx_stencil.cpp; the launchers take that choice and launch it
enum { PFX_BOX_TILE = 0 /* both passes on a 64 x 64 tile */, PFX_BOX_STRIP /* fused strip walk */, PFX_BOX_TWO_PASS /* u8 intermediate in d_tmp */,
       PFX_BOX_SLIDING = 0, PFX_BOX_PREFIX /* h_kind, the horizontal pass of PFX_BOX_TWO_PASS: sliding window | prefix sums */ };
typedef struct pfx_box_plan { int kind, h_kind, px /* 4 | 8 | 16 columns per lane (sliding) */, py /* 16 | 32 | 64 | 128 rows per lane */; } pfx_box_plan;
int pfxk_box_tile_max_radius(void), pfxk_box_strip_max_radius(void), pfxk_box_prefix_max_radius(void);   // the compiled limits: tile kernel, strip walk, prefix-sum pass (its LDS footprint)
hipError_t pfxk_box_blur(hipStream_t s, const uint8_t* d_src, uint8_t* d_tmp, uint8_t* d_dst, const uint8_t* d_mask, int radius, uint32_t w, uint32_t h,
                         const pfx_box_plan* plan, int strip_fill /* chip fill in % of one round of workgroups */, int strip_nseg /* forced segment count, 0 = auto */);
#define PFXK_MEDIAN_TILE_MAX_RADIUS 24 /* beyond: sliding histograms */
enum { PFX_MEDIAN_UNSUPPORTED = -1, PFX_MEDIAN_NET3 = 0, PFX_MEDIAN_XLANE, PFX_MEDIAN_XLANE_ROWS2, PFX_MEDIAN_XLANE7, PFX_MEDIAN_SHARED, PFX_MEDIAN_SINGLE_NET,
       PFX_MEDIAN_BITS_PAIR, PFX_MEDIAN_BITS, PFX_MEDIAN_SEARCH4, PFX_MEDIAN_SEARCH1, PFX_MEDIAN_HIST };
hipError_t pfxk_median(hipStream_t s, const uint8_t* d_src, uint8_t* d_dst, const uint8_t* d_mask, int path /* any but the two _BITS */, int radius, uint32_t w, uint32_t h);
// ---- k_median_bits.hip ---- radii 2..8 as a bit-sliced radix select over bit planes of the image (scratch: pfxk_median_bits_scratch bytes)
size_t pfxk_median_bits_scratch(int radius, uint32_t w, uint32_t h);
hipError_t pfxk_median_bits(hipStream_t s, const uint8_t* d_src, uint8_t* d_dst, const uint8_t* d_mask, uint32_t* d_planes, int radius, uint32_t w, uint32_t h,
                            int pair /* radii 2..7: two adjacent columns per lane on shared plane registers (PFX_MEDIAN_BITS_PAIR); 0: one column per lane */);
hipError_t pfxk_pixelate(hipStream_t s, const uint8_t* d_src, uint8_t* d_dst, const uint8_t* d_mask, uint32_t bs,
                         uint32_t w, uint32_t h);

// ---- k_effects.hip ---- sharpen / glow combine pass, bokeh disc blur, motion blur
enum { PFXK_FX_SHARPEN = 0, PFXK_FX_GLOW = 1 };
hipError_t pfxk_combine(hipStream_t s, const uint8_t* d_src, const uint8_t* d_blur, const uint8_t* d_mask, uint8_t* d_dst,
                        uint32_t w, uint32_t h, int op, float p0);
hipError_t pfxk_bokeh(hipStream_t s, const uint8_t* d_src, uint8_t* d_dst, const uint8_t* d_mask, const int32_t* d_spans_dy_hw,
                      int n_spans, float inv_count, uint32_t w, uint32_t h);
hipError_t pfxk_motion(hipStream_t s, const uint8_t* d_src, uint8_t* d_dst, const uint8_t* d_mask, int steps, float dx, float dy,
                       float inv_steps, uint32_t w, uint32_t h);

// ---- k_effects2.hip ---- the rest of the effect bank: one template kernel, parameter block by value (layout per effect
// documented next to each fx_pixel branch)
typedef struct pfxk_fx_params { float f[16]; int32_t i[8]; uint32_t u[4]; const void* aux0; } pfxk_fx_params;
enum { PFXK_FX2_ZOOM = 0, PFXK_FX2_DENTS, PFXK_FX2_BULGE, PFXK_FX2_TWIST, PFXK_FX2_NOISE, PFXK_FX2_REDUCE_NOISE, PFXK_FX2_VIGNETTE,
       PFXK_FX2_HALFTONE, PFXK_FX2_GRID, PFXK_FX2_BORDER, PFXK_FX2_SHADOW, PFXK_FX2_OUTLINE, PFXK_FX2_PIXEL_DRAG, PFXK_FX2_RGB_DISPLACE,
       PFXK_FX2_INK, PFXK_FX2_COLOR_FILTER, PFXK_FX2_CONTOURS };
hipError_t pfxk_fx(hipStream_t s, int fx, const uint8_t* d_src, uint8_t* d_dst, const uint8_t* d_mask, const pfxk_fx_params* P,
                   uint32_t w, uint32_t h);
// outline: one bit per pixel (alpha != 0), rows of pfxk_alpha_bits_stride(w) dwords; fx params aux0 = the plane, i[3] = the stride
uint32_t pfxk_alpha_bits_stride(uint32_t w);
hipError_t pfxk_alpha_bits(hipStream_t s, const uint8_t* d_src, uint32_t* d_bits, uint32_t w, uint32_t h);
hipError_t pfxk_crystallize(hipStream_t s, const uint8_t* d_src, uint8_t* d_dst, const uint8_t* d_mask, const float* d_seeds_xy,
                            unsigned long long* d_acc /* cells*5 */, uint32_t* d_avg /* cells */, int cells_x, int cells_y, float cs,
                            uint32_t w, uint32_t h);
hipError_t pfxk_oil_painting(hipStream_t s, const uint8_t* d_src, uint8_t* d_dst, const uint8_t* d_mask, int radius, int levels,
                             uint32_t w, uint32_t h);
// offset alpha plane -> optional separable max of radius `spread` -> aaaa RGBA image (input of the shadow's Gaussian)
hipError_t pfxk_shadow_alpha(hipStream_t s, const uint8_t* d_src, uint8_t* d_plane_a, uint8_t* d_plane_b, uint8_t* d_rgba, int ox, int oy,
                             int spread, uint32_t w, uint32_t h);

// ---- k_script.hip ---- per-pixel closure VM + the pixel-moving functions of the script transform / selection API
typedef struct pfxk_vm_args {
    const uint32_t* src;      // pre-call image (what the closure's parameters, get_pixel and get_r..a see)
    uint32_t* dst;            // result image (must not alias src)
    const uint8_t* mask;      // selection for is_selected(), or NULL
    const void* code;         // rhai::BcIns[n_code]
    const uint64_t* consts;
    unsigned long long* err;  // initialised to ~0: min over failing pixels of (row-major index << 24 | code << 16 | line)
    int n_code, n_regs, n_params;
    int n_pre;                // code[0 .. n_pre): constant loads a lane executes once, in front of its first pixel (pfx_rhai.cpp: hoist_constants); a pixel starts at n_pre
    int heavy;                // the program uses fmod / pow / sin / cos / tan / atan2 / exp / ln (selects the kernel that carries them)
    int w, h;
    int x0, y0, x1, y1;       // region processed (for_region); the rest of dst must already equal src
    uint32_t step_budget;     // bytecode steps one pixel may execute before the launch reports 'Too many operations'
} pfxk_vm_args;
hipError_t pfxk_vm_run(hipStream_t s, const pfxk_vm_args* A);
// the launch shape pfxk_vm_run picks for a program (host only; the shape probe of the tests reports it too): lanes per workgroup from the register
// count (the register file fills 64 KiB of LDS at most), the program staged in LDS behind it when both fit (lcode = 1), the dynamic LDS bytes.
// Returns 0 for a program no launch can take (more than 128 registers).
#define PFXK_VM_MAX_BLOCKS (256 * 32) // grid size cap: larger regions are walked with a grid stride
typedef struct pfxk_vm_shape_t {
    int lanes;
    int lcode;
    size_t lds_bytes;
} pfxk_vm_shape_t;
int pfxk_vm_shape(int n_regs, int n_code, pfxk_vm_shape_t* out);
// mode: 0 flip_horizontal, 1 flip_vertical, 2 rotate180, 3 rotate90 (cw), 4 rotate270 (ccw); (w, h) = source size
hipError_t pfxk_permute(hipStream_t s, const uint8_t* d_src, uint8_t* d_dst, int mode, uint32_t w, uint32_t h);
hipError_t pfxk_recanvas(hipStream_t s, const uint8_t* d_src, uint8_t* d_dst, uint32_t ow, uint32_t oh, uint32_t nw, uint32_t nh, int off_x, int off_y,
                         uint32_t fill_rgba);
// op: 0 rect [x0,x1)x[y0,y1), 1 ellipse (centre cx,cy; squared radii), 2 invert, 3 clear
hipError_t pfxk_mask_op(hipStream_t s, uint8_t* d_mask, int op, int x0, int y0, int x1, int y1, double cx, double cy, double rx2, double ry2,
                        uint32_t w, uint32_t h);
hipError_t pfxk_fill_masked(hipStream_t s, uint8_t* d_img, const uint8_t* d_mask, uint32_t rgba, uint32_t w, uint32_t h);

// ---- k_resize.hip ---- separable resampling with per-axis window / weight tables (v_*: per output row, h_*: per output column)
hipError_t pfxk_resize(hipStream_t s, const uint8_t* d_src, float* d_tmp /* w*nh*4 f32 */, uint8_t* d_dst, const uint32_t* v_left, const uint32_t* v_count,
                       const uint32_t* v_off, const float* v_wts, const uint32_t* h_left, const uint32_t* h_count, const uint32_t* h_off, const float* h_wts,
                       uint32_t w, uint32_t h, uint32_t nw, uint32_t nh, uint32_t span_max /* 0: two passes through d_tmp */);
int pfxk_resize_tile_cols(void);

typedef struct pfxk_affine_params { float hi[9]; float cx, cy, off_x, off_y, inv_scale; int32_t nearest; } pfxk_affine_params;
hipError_t pfxk_affine(hipStream_t s, const uint8_t* d_src, uint32_t sw, uint32_t sh, uint8_t* d_dst, uint32_t canvas_w, uint32_t canvas_h,
                       const pfxk_affine_params* P);

// ---- k_warp.hip ----
// what a launcher below ran (for pfx_int_warp_last; `plan` may be NULL): PFXK_WARP_* bits and the tile grid; all 0 = nothing launched
enum { PFXK_WARP_IN_LDS = 1, PFXK_WARP_PAIR = 2, PFXK_WARP_BUF32 = 4, PFXK_WARP_XCD = 8 };
typedef struct pfxk_warp_plan { int flags; uint32_t gx, gy; } pfxk_warp_plan;
void pfxk_warp_set_buf32(int on);   // 0: the 64-bit-address instantiations of both warps whatever the source's size (default 1: below 4 GiB, 32-bit offsets through a buffer resource)
int pfxk_warp_info(int which);      // compile-time shape: 0 MESH_WALK, 1 MESH_WX, 2 MESH_LDS_PTS, 3 WARP_YR, 4 tile rows from which the mesh warp takes the XCD order, 5 dabs culled per trip; -1 = unknown
// first_row: index of d_disp's / d_dst's row 0 in the whole output when they are a band of it (0: whole image)
hipError_t pfxk_warp_displacement(hipStream_t s, const uint8_t* d_src, uint32_t sw, uint32_t sh, const float* d_disp,
                                  uint32_t w, uint32_t h, uint8_t* d_dst, uint32_t first_row, pfxk_warp_plan* plan);
// d_pts: orig points (may be NULL => "fast" identity original) then deformed points, (cols+1)*(rows+1) xy pairs each
hipError_t pfxk_mesh_displacement(hipStream_t s, const float* d_orig, const float* d_def, uint32_t cols, uint32_t rows,
                                  uint32_t w, uint32_t h, float* d_disp, pfxk_warp_plan* plan);
// d_dst = rows [first_row, first_row + h) of the h_full-row result; d_src = the whole w x h_full source (first_row = 0, h_full = h: whole image)
void pfxk_warp_set_mesh_xcd(int on);
hipError_t pfxk_warp_mesh(hipStream_t s, const uint8_t* d_src, const float* d_orig, const float* d_def, uint32_t cols,
                          uint32_t rows, uint32_t w, uint32_t h, uint8_t* d_dst, uint32_t first_row, uint32_t h_full, pfxk_warp_plan* plan);

// DisplacementField dabs (k_warp.hip): bounds and Gaussian constants are prepared on the host like the reference's prologue
typedef struct pfxk_disp_dab { int32_t mode, x0, y0, x1, y1; float cx, cy, delta_x, delta_y, r, sigma_sq_2, strength; } pfxk_disp_dab;
hipError_t pfxk_disp_brushes(hipStream_t s, float* d_disp, uint32_t w, uint32_t h, const pfxk_disp_dab* d_dabs, uint32_t n, int bx0, int by0, int bx1,
                             int by1);
/* … over the 64 x 64 chunks a dab's box touches (d_chunks: chunk x | chunk y << 16) instead of the whole bounding box */
hipError_t pfxk_disp_brushes_chunked(hipStream_t s, float* d_disp, uint32_t w, uint32_t h, const pfxk_disp_dab* d_dabs, uint32_t n, int bx0, int by0, int bx1, int by1,
                                     const uint32_t* d_chunks, uint32_t n_chunks);

// ---- k_brush.hip ----
typedef struct pfxk_brush {
    float radius, radius_sq, draw_radius, draw_radius_sq, inv_radius_sq, hardness, flow;
    float src_r, src_g, src_b, src_a;
    uint32_t rgb8;          // (c*255) as u8, packed r | g<<8 | b<<16
    int32_t anti_aliased, use_direct_alpha, is_eraser, mode;
    uint32_t tip_size;      // side of the square image-tip mask, 0 = circle tip
} pfxk_brush;
// one stamp after the host prologue of draw_circle_no_dirty / draw_image_tip_no_dirty: scattered centre, jittered colour bytes,
// inverse-rotation cosine / sine of an image tip
// … and the stamp's pixel box [x0, x1] x [y0, y1] (brush_render.rs:209-215 / :584-587), 16-byte aligned: x0 > x1 = the stamp touches no pixel
typedef struct pfxk_stamp { float cx, cy; uint32_t rgb8; uint32_t rotated; uint32_t x0, x1, y0, y1; float cos_a, sin_a; uint32_t pad[2]; } pfxk_stamp;
hipError_t pfxk_brush_stamps(hipStream_t s, uint8_t* d_target, uint32_t w, uint32_t h, const pfxk_brush* B,
                             const pfxk_stamp* d_stamps, uint32_t n_stamps, const uint8_t* d_lut256, const uint8_t* d_tip_mask,
                             const uint8_t* d_selection, int bx0, int by0, int bx1, int by1);
/* the same with the stamps dealt to the 64 x 64 chunks their boxes touch: d_chunks = n_chunks x {chunk x, chunk y, first entry, entries}, d_bins = stamp indices (stroke order per chunk) */
hipError_t pfxk_brush_stamps_binned(hipStream_t s, uint8_t* d_target, uint32_t w, uint32_t h, const pfxk_brush* B, const pfxk_stamp* d_stamps, uint32_t n_points,
                                    const uint8_t* d_lut256, const uint8_t* d_tip_mask, const uint8_t* d_selection, const uint32_t* d_chunks, uint32_t n_chunks,
                                    const uint32_t* d_bins);
hipError_t pfxk_brush_commit(hipStream_t s, uint8_t* d_layer, const uint8_t* d_preview, const uint8_t* d_selection,
                             uint32_t w, uint32_t h, uint32_t mode, int is_eraser);
// element-wise blend_pixel_static over two pixel arrays (spot checks / stroke commit)
hipError_t pfxk_blend_arrays(hipStream_t s, const uint8_t* d_base, const uint8_t* d_top, uint8_t* d_dst, size_t n_px,
                             uint32_t mode, float opacity, int fast_div);

// ---- k_shapes.hip ---- the shape tool's SDF rasteriser (shapes.rs:1169-1305); the host side (pfx_shapes.cpp) prepares everything that is uniform over the image
enum { PFXK_SDF_ELLIPSE = 0, PFXK_SDF_BOX, PFXK_SDF_ROUNDED, PFXK_SDF_CONVEX /* trapezoid, parallelogram, right triangle */, PFXK_SDF_TRIANGLE,
       PFXK_SDF_POLYGON /* pentagon, hexagon, octagon */, PFXK_SDF_CROSS, PFXK_SDF_CHECK, PFXK_SDF_HEART, PFXK_SDF_DIAMOND, PFXK_SDF_STAR /* star5, star6 */,
       PFXK_SDF_ARROW };
enum { PFXK_SHAPE_BOX = 0 /* d_out = bw*bh pixels */, PFXK_SHAPE_CANVAS = 1 /* d_out = the whole canvas, every pixel written */,
       PFXK_SHAPE_COMMIT = 2 /* d_out = the layer, blended in place over the box */ };
#define PFXK_SHAPE_MAX_VERTS 96
typedef struct pfxk_shape_params { // passed by value: lands in SGPRs / scalar loads
    int32_t  x0, y0, bw, bh;       // the box in canvas pixels (inside the canvas; bw or bh == 0: empty)
    float    cx, cy, inv_cos, inv_sin, hx, hy, outline_width /* .max(0.0) applied */, corner_radius;
    uint32_t primary, secondary;   // r | g << 8 | b << 16 | a << 24
    int32_t  fill_mode, anti_alias;
    float    k[12];                // per-SDF constants, layout next to each branch of shape_sdf (k_shapes.hip)
    int32_t  n_verts;
    float    verts[PFXK_SHAPE_MAX_VERTS][2]; // PFXK_SDF_CONVEX: 3 or 4 vertices; PFXK_SDF_HEART: the 96-vertex path
} pfxk_shape_params;
hipError_t pfxk_shape(hipStream_t s, int form, int sdf, const pfxk_shape_params* P, uint8_t* d_out, const uint8_t* d_selection /* COMMIT only, may be NULL */,
                      uint32_t mode /* COMMIT only: BlendMode::to_u8 */, uint32_t canvas_w, uint32_t canvas_h);

// ---- k_customshape.hip ---- the shape tool with a custom path (shapes.rs:1065-1163) and the picker's icon (:122-155); host side: pfx_customshape.cpp
#define PFXK_CUSTOM_BATCH 256   // segments a workgroup looks at per step, one per lane
#define PFXK_CUSTOM_LIST 1024   // slots of each LDS segment list: consumed after every fourth batch
typedef struct pfxk_custom_params { // passed by value; the forms and the box are k_shapes.hip's
    int32_t  x0, y0, bw, bh;
    float    cx, cy, inv_cos, inv_sin, hx, hy;
    float    sx, sy, min_x, min_y;   // custom_shape_coverage_sample :1097-1101
    float    max_scale;              // sx.max(sy)
    float    outline_width;          // .max(1.0) applied
    float    reach;                  // max(outline_width, 1) * max(sx, sy) * (1 + 2^-10), not rounded down: the distance cull's radius before its 2^-16 M
    float    seg_abs;                // the largest |coordinate| of the segments
    uint32_t primary;                // r | g << 8 | b << 16 | a << 24
    int32_t  fill_mode;              // 0 outline, 1 filled, 2 both
    uint32_t n_segments;
    int32_t  cull;                   // 0: every segment goes on both lists (profiles/custom_shapes.md)
} pfxk_custom_params;
hipError_t pfxk_custom_shape(hipStream_t s, int form /* PFXK_SHAPE_* */, const pfxk_custom_params* P, const float* d_segs /* n_segments * 4, 16-byte aligned */,
                             uint8_t* d_out, const uint8_t* d_selection /* COMMIT only, may be NULL */, uint32_t mode, uint32_t canvas_w, uint32_t canvas_h);
hipError_t pfxk_custom_icon(hipStream_t s, const pfxk_custom_params* P /* hx, hy, sx, sy, min_x, min_y, seg_abs, n_segments, cull */, const float* d_segs,
                            uint8_t* d_out /* size * size pixels */, uint32_t size, uint32_t fg);

// ---- k_inpaint.hip ---- content-aware fill (inpaint.rs): instant heal dabs :76-192 and the onion-peeling PatchMatch :394-520; host side: pfx_inpaint.cpp
// a dab as the kernel reads it: r = brush_radius.max(1.0), hard_t = (hardness * 0.9 + 0.1).clamp(0, 1), soft_den = 1.0 - hard_t + 1e-6, the dab's own pixel loop
// bounds [x0, x1] x [y0, y1] (:93-96; x0 > x1 = none), ring = which 64-float set of d_rings (pfx_inpaint_ring_offsets of its sample radius)
typedef struct pfxk_inpaint_dab { float cx, cy, r, hard_t, soft_den; uint32_t x0, x1, y0, y1, ring, pad[2]; } pfxk_inpaint_dab;
hipError_t pfxk_inpaint_instant(hipStream_t s, const uint8_t* d_src, const uint8_t* d_mask, uint8_t* d_out, uint32_t w, uint32_t h, const pfxk_inpaint_dab* d_dabs,
                                uint32_t n_dabs, const float* d_rings, uint32_t bx0, uint32_t by0, uint32_t bx1, uint32_t by1 /* the boxes' union, inclusive */);
// PatchMatch geometry: the canvas, the hole's bounding box (the NNF arrays hold (bw + 2) * (bh + 2) entries: the box plus one pixel), half = max(patch, 3) / 2
// (1..5), min_valid = max((2 half + 1)^2, 4) / 4, max_radius = max(w, h) as f32
typedef struct pfxk_pm_geom { uint32_t w, h, x0, y0, bw, bh, half, min_valid; float max_radius; } pfxk_pm_geom;
// d_stats[0..8): ~min x, ~min y, max x, max y of the pixels with mask != 0, then their count (zeroed first)
hipError_t pfxk_pm_stats(hipStream_t s, const uint8_t* d_mask, uint32_t w, uint32_t h, uint32_t* d_stats);
// stable row-major compaction over the rectangle of pixel indices y * w + x — kind 0: mask == 0, kind 1: boundary pixels of the hole (a hole pixel with a
// 4-neighbour outside it).  phase 0: per-1024-element counts into d_counts, scanned in place, *d_total = how many; phase 1: the indices to d_list[0 .. total)
hipError_t pfxk_pm_compact(hipStream_t s, int kind, const uint8_t* d_mask, uint32_t w, uint32_t h, uint32_t rx0, uint32_t ry0, uint32_t rw, uint32_t rh,
                           uint32_t* d_counts, uint32_t* d_total, uint32_t* d_list, int phase);
hipError_t pfxk_pm_nnf_reset(hipStream_t s, const pfxk_pm_geom* g, float* d_nnf_ssd);   // every SSD = f32::MAX
// one peel over the nb boundary pixels stored at d_sources[src_count .. src_count + nb): bucket by anti-diagonal, random init, pm_iters passes (one workgroup
// each), fill, clear the live mask.  d_diag_start: bw + bh words, d_cursor: bw + bh - 1, d_diag_list: nb
hipError_t pfxk_pm_peel(hipStream_t s, const pfxk_pm_geom* g, uint8_t* d_img, uint8_t* d_live, const uint32_t* d_sources, uint32_t src_count, uint32_t nb,
                        int pm_iters, int32_t* d_nnf_ox, int32_t* d_nnf_oy, float* d_nnf_ssd, uint32_t* d_diag_start, uint32_t* d_cursor, uint32_t* d_diag_list);

// ---- k_flood.hip ---- bucket fill / magic wand (fill_magic.rs): colour distance, tile-converging minimax flood, threshold masks, bounding boxes; host side: pfx_flood.cpp
#define PFXK_FLOOD_TILE 64          // a workgroup's tile edge
#define PFXK_FLOOD_TILE_ITERS 64    // cap on a tile's sweep rounds per visit; a tile that reaches it schedules itself again
// what is uniform over the image in a colour distance: the target's bytes and, for the perceptual mode, its premultiplied linear rgb and alpha / 255
typedef struct pfxk_flood_target { uint32_t rgba; float lin[3]; float ta; } pfxk_flood_target;
// c[i] = pixel_color_distance(src[i], target) for n pixels; mode 0 legacy, 1 perceptual (d_table: 256 floats, srgb_to_linear(k / 255))
hipError_t pfxk_color_distance(hipStream_t s, const uint8_t* d_src, uint8_t* d_out, size_t n, int mode, const pfxk_flood_target* T, const float* d_table);
// d_list[0] = the seed's tile (d stays all 255: the first pass plants the seed)
hipError_t pfxk_flood_seed(hipStream_t s, uint32_t w, uint32_t seed_x, uint32_t seed_y, uint32_t* d_list);
// one pass: every tile of d_list[0 .. n) relaxes to its fixed point (or the round cap) and is written back.  A tile whose border pixel dropped below the
// neighbour's pixel beside it appends that neighbour to d_next (once per pass: d_mark[tile] == stamp), itself when it hit the cap; d_state[0] counts the
// entries of d_next, d_state[1] becomes non-zero when any byte decreased.  conn = 4 or 8.  The first pass gets the seed and lowers d[seed] to c[seed] inside its
// tile — a decrease like any other, so a seed on a tile border schedules the tile across it; later passes get seed_x >= w
hipError_t pfxk_flood_pass(hipStream_t s, int conn, const uint8_t* d_c, uint8_t* d_d, uint32_t w, uint32_t h, const uint32_t* d_list, uint32_t n,
                           uint32_t* d_next, uint32_t* d_state, uint32_t* d_mark, uint32_t stamp, uint32_t seed_x, uint32_t seed_y);
// d_table[4 t ..] = ~min x, ~min y, max x, max y of {d == t} (zeroed first: ~min x == 0 means none), atomically merged
hipError_t pfxk_flood_bboxes(hipStream_t s, const uint8_t* d_dist, uint32_t w, uint32_t h, uint32_t* d_table);
hipError_t pfxk_wand_mask(hipStream_t s, const uint8_t* d_dist, const uint8_t* d_base /* may be NULL */, uint8_t* d_out, size_t n, uint32_t threshold, int aa, int combine);
hipError_t pfxk_fill_preview(hipStream_t s, const uint8_t* d_dist, const uint8_t* d_sel /* may be NULL */, uint8_t* d_out, size_t n, uint32_t threshold, uint32_t fill_rgba);
hipError_t pfxk_fill_commit(hipStream_t s, uint8_t* d_layer, const uint8_t* d_dist, const uint8_t* d_sel /* may be NULL */, size_t n, uint32_t threshold,
                            uint32_t fill_rgba, uint32_t mode);

// ---- k_select.hip ---- selection masks (selection.rs, canvas_state.rs:1632-1887, perspective_gradient.rs:2-86, adjustments.rs:1448-1591); host side: pfx_select.cpp
#define PFXK_SELECT_SEG 256           // pixels a row-walking workgroup takes per step; a row segment is pfxk_select_segment(r) of them
#define PFXK_SELECT_BAND 32           // rows of the feather's vertical band at r <= 8; pfxk_select_band(r) beyond
#define PFXK_SELECT_VEC 4             // mask bytes per lane of the shape kernel when base and output are that aligned
#define PFXK_SELECT_LASSO_MAX 8192    // polygon points = the most crossings of one row: 32 KB of LDS
#define PFXK_SELECT_FEATHER_MAX 512   // the feather's radius cap (the prefix ring of the H pass is sized for it)
#define PFXK_SELECT_MORPH_MAX 46340   // grow / shrink: the reference's i32 r * r overflows beyond
// a shape inside its bounding box (inclusive; x0 > x1 or y0 > y1 = empty): kind 0 rectangle, 1 ellipse ((x - cx) / rx)^2 + ((y - cy) / ry)^2 <= 1
typedef struct pfxk_select_shape { uint32_t kind, x0, y0, x1, y1; float cx, cy, rx, ry; } pfxk_select_shape;
// out = combine(base, shape) over every byte; mode 0 replace, 1 add, 2 subtract, 3 intersect; d_base may be NULL (all zero) or d_out itself
hipError_t pfxk_select_shape_combine(hipStream_t s, const uint8_t* d_base, uint8_t* d_out, uint32_t w, uint32_t h, const pfxk_select_shape* S, int mode);
// the scanline polygon fill fused with the combine rule; d_points_xy: n_points (x, y) pairs, 8-byte aligned; d_base as above
hipError_t pfxk_select_lasso(hipStream_t s, const float* d_points_xy, uint32_t n_points, const uint8_t* d_base, uint8_t* d_out, uint32_t w, uint32_t h, int mode);
hipError_t pfxk_select_translate(hipStream_t s, const uint8_t* d_src, uint8_t* d_out, uint32_t w, uint32_t h, int32_t dx, int32_t dy);   // not in place
// d_box[0 .. 4) = ~min x, ~min y, max x, max y of {mask != 0} (zeroed first: ~min x == 0 means none), atomically merged
hipError_t pfxk_select_bounds(hipStream_t s, const uint8_t* d_mask, uint32_t w, uint32_t h, uint32_t* d_box);
hipError_t pfxk_select_fill(hipStream_t s, uint8_t* d_layer, const uint8_t* d_mask, uint32_t w, uint32_t h, uint32_t color_rgba, int erase);
uint32_t pfxk_select_segment(uint32_t r);   // the row segment a workgroup owns at radius r: its halo of 2 r stays below half of it
uint32_t pfxk_select_band(uint32_t r);      // likewise the band of the feather's vertical pass
// grow (expand != 0) or shrink by the disc of radius r in 1 .. PFXK_SELECT_MORPH_MAX: d_rowdist is w * h u16 of working memory, d_span r + 1 entries
// floor(sqrt(r^2 - k^2)); d_out may be d_mask
hipError_t pfxk_select_morph(hipStream_t s, int expand, const uint8_t* d_mask, uint16_t* d_rowdist, const uint16_t* d_span, uint8_t* d_out, uint32_t w,
                             uint32_t h, uint32_t r);
// one feather pass, r in 1 .. PFXK_SELECT_FEATHER_MAX: horizontal d_src -> d_tmp, vertical d_tmp -> d_dst (d_dst may be d_src; d_tmp is neither)
hipError_t pfxk_select_feather_pass(hipStream_t s, const uint8_t* d_src, uint8_t* d_tmp, uint8_t* d_dst, uint32_t w, uint32_t h, uint32_t r);

// ---- k_colorkey.hip ---- removal by colour (src/ops/color_removal.rs): colour to alpha, and the colour remover's passability map, ring levels and write-out; host side: pfx_colorkey.cpp
#define PFXK_COLORKEY_TILE 64              // the ring kernel's tile edge
#define PFXK_COLORKEY_CHUNK 32             // ring levels one launch adds: the tile's halo, 128 x 128 state bytes = 16 KB of LDS
#define PFXK_COLORKEY_MAX_SMOOTHNESS 1024  // the host's cap: 32 ring launches
#define PFXK_COLORKEY_NONE 0xffffu         // a level map's "not reached"
// the dialog's settings as the reference prepares them (:51-58), all in 0 .. 1 but target (0 .. 255) and target_luma
typedef struct pfxk_cta { float target[3], tolerance, softness, strength, spill, alpha_floor, alpha_ceiling, protect, target_luma; } pfxk_cta;
// the tool's click: the seed's colour as floats and bytes, (tolerance * 2.55)^2, smoothness and smoothness as f32 + 1.0, the scope
typedef struct pfxk_ckey { float seed[3]; uint32_t seed_rgb; float tol_sq; uint32_t smoothness; float fade_den; uint32_t global; } pfxk_ckey;
// color_to_alpha_core :64-133 over n pixels; d_mask may be NULL; d_dst may be d_src
hipError_t pfxk_color_to_alpha(hipStream_t s, const uint8_t* d_src, uint8_t* d_dst, const uint8_t* d_mask, size_t n, const pfxk_cta* S);
// c[i] = 0 where the flood may pass (selected and: alpha 0 or within the tolerance), else 255; in the global scope 0 marks the core itself (alpha 0 is not core, :249)
hipError_t pfxk_ckey_passable(hipStream_t s, const uint8_t* d_src, const uint8_t* d_sel /* may be NULL */, uint8_t* d_out, size_t n, const pfxk_ckey* P);
// smoothness 0: step 3 (:344-415) where d_core is 0, a copy of src elsewhere; d_dst may be d_src
hipError_t pfxk_ckey_apply_core(hipStream_t s, const uint8_t* d_src, const uint8_t* d_core, uint8_t* d_dst, size_t n, const pfxk_ckey* P);
// k more ring levels (1 .. PFXK_COLORKEY_CHUNK) on top of `base` known ones.  The known levels come from d_lin (u16, base > 0) or, with d_lin NULL and base 0,
// from d_core (0 = level 0).  With d_lout the new map is written there (not d_lin); with d_lout NULL this is the last launch and step 3 writes d_dst (may be d_src)
hipError_t pfxk_ckey_rings(hipStream_t s, const uint8_t* d_core, const uint16_t* d_lin, const uint8_t* d_sel /* may be NULL */, uint16_t* d_lout, const uint8_t* d_src,
                           uint8_t* d_dst, uint32_t w, uint32_t h, uint32_t base, uint32_t k, const pfxk_ckey* P);

// ---- k_overlay.hip ---- the floating selection (src/ops/clipboard.rs: commit :2032, render_preview :2168, rasterize_for_clipboard :1048, extract_to_overlay :729); host side: pfx_overlay.cpp
// What the sampling kernels share, all derived on the host (pfx_overlay_geometry): the anchor in canvas coordinates, cos / sin of the rotation, origin =
// centre - scaled / 2, the scaled image and the source it was scaled from with ratio = (f32)source / (f32)scaled — the NEAREST rule of the resize's
// per-axis tables is source index min(floor((o + 0.5) * ratio), source - 1), weight 1 — and the window: box_w x box_h pixels from (x0, y0), written at
// row pitch `pitch` pixels from pixel (x0 - out_x0, y0 - out_y0) of the output
typedef struct pfxk_overlay {
    float ax, ay, cos_r, sin_r, origin_x, origin_y, ratio_x, ratio_y;
    uint32_t scaled_w, scaled_h, source_w, source_h;
    int32_t x0, y0, out_x0, out_y0;
    uint32_t box_w, box_h, pitch;
} pfxk_overlay;
// commit's stamp over the box, in place on d_img (the document): aa = the +-0.5 window and sample_bilinear, else the tight window and the nearest pick;
// overwrite 0 = alpha_blend only, 1 = every sample overwrites, 2 = where d_mask (source_w x source_h bytes, through the NEAREST rule) allows.  d_scaled is scaled_w x scaled_h
hipError_t pfxk_overlay_commit(hipStream_t s, const uint8_t* d_scaled, const uint8_t* d_mask, uint8_t* d_img, const pfxk_overlay* P, int aa, int overwrite);
// rasterize_for_clipboard: the same sampler, samples with alpha > 0 stored into d_out (zeroed by the caller); *d_any |= 1 when one was
hipError_t pfxk_overlay_rasterize(hipStream_t s, const uint8_t* d_scaled, uint8_t* d_out, const pfxk_overlay* P, int aa, uint32_t* d_any);
// render_preview over every pixel of the doc_w x doc_h output, NEAREST-scaled straight from d_source.  translate: the pixels of [x0, x0 + box_w) x [y0, y0 +
// box_h) are scaled pixel (x - out_x0, y - out_y0), out_x0 / out_y0 being the rounded origin; else the general path over the box.  Zero where nothing is drawn
hipError_t pfxk_overlay_preview(hipStream_t s, const uint8_t* d_source, uint8_t* d_out, uint32_t doc_w, uint32_t doc_h, const pfxk_overlay* P, int translate);
// extract_to_overlay with a selection: clip / clip_mask over the box (x0, y0, bw x bh), tightly packed
hipError_t pfxk_overlay_lift(hipStream_t s, const uint8_t* d_layer, const uint8_t* d_sel, uint8_t* d_clip, uint8_t* d_clip_mask, uint32_t w, uint32_t x0, uint32_t y0,
                             uint32_t bw, uint32_t bh);
// *d_any |= 1 when a pixel of the n has alpha > 0
hipError_t pfxk_overlay_any_alpha(hipStream_t s, const uint8_t* d_img, size_t n, uint32_t* d_any);

// ---- k_textfx.hip ---- the text layer's styles (src/ops/text_layer/effects.rs: apply_text_effects :1, dilate_mask :167); host side: pfx_textfx.cpp
#define PFXK_TEXTFX_MAX_RADIUS 64
// dilate_mask's disc as row spans, built on the host with the reference's f32 test: span[dy + radius] for dy in [-radius, radius] is PFXK_DISC_SKIP where
// dy * dy > r_sq, else half | level << 8 | reads << 16: the span [x - half, x + half] is covered by `reads` (1..4) windows of 4^level columns
#define PFXK_DISC_SKIP 0xffffffffu
typedef struct pfxk_disc {
    int32_t  radius;                                   // ceil(r), 1 .. PFXK_TEXTFX_MAX_RADIUS
    uint32_t levels;                                   // window tables the kernel builds: 4^0 .. 4^(levels - 1) columns
    uint32_t span[2 * PFXK_TEXTFX_MAX_RADIUS + 1];
} pfxk_disc;
// the disc's maximum (take_min: minimum) over a w x h u8 plane read as d_src[(y * w + x) * src_stride + src_offset] (1, 0: a plane; 4, 3: the alpha of an
// RGBA8 image), clipped to the image, the maximum starting at 0 (the minimum at 255), into the plane d_dst
hipError_t pfxk_textfx_disc(hipStream_t s, const uint8_t* d_src, uint32_t src_stride, uint32_t src_offset, uint8_t* d_dst, uint32_t w, uint32_t h,
                            const pfxk_disc* D, int take_min);
// the shadows' alpha plane: the text's alpha read at (x - dx, y - dy); inner 0: round((a / 255) * alpha), 0 from outside the image; inner 1:
// round((1 - a / 255) * alpha), `alpha` from outside
hipError_t pfxk_textfx_plane(hipStream_t s, const uint8_t* d_text, uint8_t* d_plane, uint32_t w, uint32_t h, int32_t dx, int32_t dy, uint32_t alpha, int inner);
// d_rgba[i] = (rgb, d_plane[i]): the image the reference hands to its Gaussian
hipError_t pfxk_textfx_expand(hipStream_t s, const uint8_t* d_plane, uint8_t* d_rgba, size_t n, uint32_t rgb);
enum { PFXK_TFX_SHADOW = 1, PFXK_TFX_SHADOW_RGBA = 2,   // a shadow stage; its alpha is the blurred RGBA image `shadow` (rgb read there too), not a plane
       PFXK_TFX_OUTLINE_OUT = 4, PFXK_TFX_GRADIENT = 8, PFXK_TFX_GRADIENT_REPEAT = 16, PFXK_TFX_TEXTURE = 32, PFXK_TFX_OUTLINE_IN = 64,
       PFXK_TFX_INNER = 128,         // an inner shadow stage; without _BLURRED it reads the shifted text itself
       PFXK_TFX_INNER_BLURRED = 256, PFXK_TFX_INNER_RGBA = 512 };
typedef struct pfxk_textfx {
    uint32_t w, h, flags;
    const uint8_t *shadow, *dilated, *eroded, *inner;   // planes of w * h bytes (or RGBA8 images, see the flags); read only where a flag says so
    uint32_t shadow_rgb, outline_rgb, inner_rgb;        // r | g << 8 | b << 16
    float    outline_oa;                                // colour alpha as f32 / 255.0
    int32_t  inner_dx, inner_dy;
    float    inner_ia;                                  // colour alpha as f32
    float    g_dir_x, g_dir_y, g_scale, g_off_x, g_off_y;
    uint32_t g_start, g_end;                            // packed RGBA8
    uint32_t tex_w, tex_h;
    float    t_scale, t_off_x, t_off_y;
} pfxk_textfx;
// every per-pixel stage of apply_text_effects in order, the output written once
hipError_t pfxk_textfx_compose(hipStream_t s, const uint8_t* d_text, const uint8_t* d_texture, uint8_t* d_out, const pfxk_textfx* P);
// find_tight_bounds_rgba: d_got[0..5) (zeroed by the caller) = max(~x), max(~y), max(x), max(y) over the pixels with alpha > 0, and 1 when there is one
hipError_t pfxk_textfx_bounds(hipStream_t s, const uint8_t* d_img, uint32_t w, uint32_t h, uint32_t* d_got);

// ---- k_textwarp.hip ---- the text block's warps, rotation and blit (src/ops/text_layer/warp.rs, raster.rs:561-653); host side: pfx_textwarp.cpp
// What is uniform over the image, derived on the host through the reference's own f32 expressions.  Every kernel writes all out_w * out_h pixels
typedef struct pfxk_textwarp {
    uint32_t src_w, src_h, out_w, out_h;
    float w, h, min_x, min_y;                            // src_w / src_h as f32; the bounds' corner (margins included)
    // arc :222-274
    float cx, r_abs, r_sign, half_angle, theta_lim;      // w / 2, |radius|, +-1, angle / 2, |angle / 2| + 0.1
    float half_w, half_h, h_r_sign;                      // w / 2, h / 2, h * r_sign
    float one_hdist, one_vdist;                          // 1 + hdist, 1 + vdist
    uint32_t curved, undo_h, undo_v;                     // |angle| > 0.01, |hdist| > 0.001, |vdist| > 0.001
    // circular :305-349
    float r, r_outer, out_c, start_angle, dir;
    // path :413-441 and envelope :495-536: the curves' control points; the envelope's t denominator max(max_x - min_x - 2 margin, 1)
    float top[4][2], bottom[4][2], t_den;
} pfxk_textwarp;
// the path's tables: eval_cubic_bezier at i / 64 and build_arc_length_table's 257 cumulative lengths
typedef struct pfxk_textwarp_tables { float cx[65], cy[65], len[257]; } pfxk_textwarp_tables;
hipError_t pfxk_textwarp_arc(hipStream_t s, const uint8_t* d_src, uint8_t* d_out, const pfxk_textwarp* P);
hipError_t pfxk_textwarp_circular(hipStream_t s, const uint8_t* d_src, uint8_t* d_out, const pfxk_textwarp* P);
hipError_t pfxk_textwarp_path(hipStream_t s, const uint8_t* d_src, uint8_t* d_out, const pfxk_textwarp* P, const pfxk_textwarp_tables* T);   // P->top = the path
hipError_t pfxk_textwarp_envelope(hipStream_t s, const uint8_t* d_src, uint8_t* d_out, const pfxk_textwarp* P);
// rotate_glyph_buffer's loop :605-647: (cx, cy) the pivot, (new_cx, new_cy) the pivot in the output
typedef struct pfxk_textrotate { uint32_t w, h, new_w, new_h; float cos_a, sin_a, cx, cy, new_cx, new_cy; } pfxk_textrotate;
hipError_t pfxk_textwarp_rotate(hipStream_t s, const uint8_t* d_src, uint8_t* d_out, const pfxk_textrotate* R);
// blit_rgba_buffer: the bw x bh buffer at (off_x, off_y) on the cw x ch canvas; alpha 0 keeps the canvas pixel, any other pixel replaces it
hipError_t pfxk_textwarp_blit(hipStream_t s, const uint8_t* d_buf, uint32_t bw, uint32_t bh, int64_t off_x, int64_t off_y, uint8_t* d_canvas, uint32_t cw, uint32_t ch);

// ---- k_gradient.hip ---- the gradient tool and the perspective crop (src/ui/panels/tools/behavior/raster/perspective_gradient.rs, gradient_text/
// gradient_controls.rs:63-122); host side: pfx_gradient.cpp
// What render_gradient_to_preview's CPU path hoists out of its loops :415-430, derived on the host through the reference's own f32 expressions
typedef struct pfxk_gradient {
    float ax, ay, dx, dy;                  // the drag's start; end - start
    float inv_len, inv_len_sq, ux, uy;     // len > 1e-6 ? 1 / len : 0, likewise on len_sq; dx * inv_len, dy * inv_len
    float scale_f;                         // preview_scale as f32
    uint32_t scale, gen_w, gen_h, w;       // preview_scale; the generated size div_ceil(w, scale) x div_ceil(h, scale); the selection's row pitch
    int32_t shape, repeat, eraser;         // PFX_GRADIENT_*; 0 / 1; transparency mode
} pfxk_gradient;
// d_lut: 256 packed RGBA8 entries, already baked in transparency mode.  Every pixel of d_preview (and of d_premul, when given) is written
hipError_t pfxk_gradient_render(hipStream_t s, const uint32_t* d_lut, const uint8_t* d_sel, uint8_t* d_preview, uint8_t* d_premul, const pfxk_gradient* P);
// commit_gradient over n pixels, the layer in place
hipError_t pfxk_gradient_commit(hipStream_t s, uint8_t* d_layer, const uint8_t* d_preview, size_t n, int is_eraser);
// render at scale 1 and commit in one pass over the layer (P->scale == 1, P->gen_w x P->gen_h the layer's size)
hipError_t pfxk_gradient_apply(hipStream_t s, const uint32_t* d_lut, const uint8_t* d_sel, uint8_t* d_layer, const pfxk_gradient* P);
// apply_perspective_crop's loop :150-165 for n_layers images of w x h into as many of out_w x out_h through one map; the pointer arrays live on the device
typedef struct pfxk_crop { float cx[4], cy[4]; uint32_t w, h, out_w, out_h, n_layers; } pfxk_crop;   // corners TL, TR, BR, BL
hipError_t pfxk_perspective_crop(hipStream_t s, const uint8_t* const* d_layers, uint8_t* const* d_outs, const pfxk_crop* P);

// ---- k_dabtools.hip ---- the clone stamp, the heal brush's live stroke and the pencil (src/ui/panels/tools/behavior/raster/clone_heal.rs); host side:
// pfx_dabtools.cpp
enum { PFXK_DAB_CLONE = 0, PFXK_DAB_HEAL = 1 };
// what is uniform over a stroke: radius = size / 2; hard_t = clamp(hardness * 0.9 + 0.1, 0, 1) and hard_den = 1 - hard_t + 1e-6 (heal_circle :194, :198)
typedef struct pfxk_dabtool { float radius, hardness, hard_t, hard_den, sample_radius, offset_x, offset_y; int32_t tool, anti_aliased; } pfxk_dabtool;
// one dab after the host prologue: its centre and its pixel box [x0, x1] x [y0, y1] (:17-20, :149-152), 16-byte aligned: x0 > x1 = the dab touches no pixel
typedef struct pfxk_dab { float cx, cy; uint32_t pad[2]; uint32_t x0, x1, y0, y1; } pfxk_dab;
// the dabs dealt to the 64 x 64 chunks their boxes touch, as pfxk_brush_stamps_binned takes them: d_chunks = n_chunks x {chunk x, chunk y, first entry,
// entries}, d_bins = dab indices in stroke order per chunk.  d_source is only read; it shares no byte with d_preview
hipError_t pfxk_dab_stroke(hipStream_t s, const pfxk_dabtool* T, const uint8_t* d_source, uint8_t* d_preview, const uint8_t* d_sel, uint32_t w, uint32_t h,
                           const pfxk_dab* d_dabs, const uint32_t* d_chunks, uint32_t n_chunks, const uint32_t* d_bins);
// draw_pixel_and_get_bounds :295-367 for n cells (x, y pairs); a cell outside the canvas is skipped.  color: the four f32 channels
hipError_t pfxk_pencil_cells(hipStream_t s, uint8_t* d_preview, const uint8_t* d_sel, uint32_t w, uint32_t h, const int32_t* d_cells, uint32_t n, float r, float g,
                             float b, float a);

// ---- k_linetool.hip ---- the line / curve tool's rasteriser (src/ui/panels/tools/behavior/raster/bezier_math.rs:76-526) and the mask-target release
// (bezier_commit.rs:229-295); host side: pfx_linetool.cpp
// one arrowhead after the host prologue (draw_filled_triangle :304-328): vertex k is (vx[k], vy[k]) in draw order a, b, c; edge k runs from vertex k to vertex
// (k + 1) % 3 with e = v1 - v0 and len = sqrt(ex ex + ey ey).max(0.001); sign = the winding; the pixel box [x0, x1] x [y0, y1], x0 > x1 = no pixel
typedef struct pfxk_line_tri { float vx[3], vy[3], ex[3], ey[3], len[3], sign; uint32_t x0, x1, y0, y1; } pfxk_line_tri;
// what is uniform over a call: compute_line_alpha's (effective_radius, fade_width, solid_radius) of the radius (brush_render.rs:103-118), the radius itself
// for the non-AA `dist < radius`, src_a = color.a / 255.0, rgb = the three colour bytes after their round trip ((c / 255.0) * 255.0) as u8, alpha byte 0
typedef struct pfxk_line { float radius, eff_radius, fade_width, solid_radius, src_a; uint32_t rgb; int32_t anti_alias; uint32_t n_tris; pfxk_line_tri tri[2]; } pfxk_line;
// one dot: its centre, the cell (fx as u32, fy as u32) whose selection byte gates the whole dot, its pixel box (:482-485); the layout of pfxk_dab
typedef struct pfxk_line_dot { float cx, cy; uint32_t cell_x, cell_y; uint32_t x0, x1, y0, y1; } pfxk_line_dot;
// a chunk of the launch: d_chunks = n_chunks x {chunk x, chunk y, first entry, entries, flags, 0, 0, 0} (two uint4), d_bins = dot indices per chunk
enum { PFXK_LINE_CLEAR = 1, PFXK_LINE_TRI0 = 2, PFXK_LINE_TRI1 = 4 };   // flags: the chunk starts from 0, not from the preview; triangle k's box touches it
hipError_t pfxk_line_render(hipStream_t s, const pfxk_line* L, uint8_t* d_preview, const uint8_t* d_sel, uint32_t w, uint32_t h, const pfxk_line_dot* d_dots,
                            const uint32_t* d_chunks, uint32_t n_chunks, const uint32_t* d_bins);
// commit_preview_to_layer_mask: conceal bytes in place from the preview's alpha; reveal: old (255 - s) / 255, else old + (255 - old) s / 255
hipError_t pfxk_line_commit_mask(hipStream_t s, uint8_t* d_conceal, const uint8_t* d_preview, const uint8_t* d_sel, uint32_t w, uint32_t h, int reveal);

// ---- k_colorrange.hip ---- the colour dialogs' last pixel loops (src/ops/adjustments.rs): compute_histogram :883, hue_saturation_per_band_from_flat :1635,
// select_color_range :1684; host side: pfx_colorrange.cpp
// the histogram kernel's grid never exceeds this many workgroups of 256 lanes (a lane takes 4 pixels per step on the 16-byte path, 1 on the byte path); a
// workgroup keeps PFXK_HIST_COPIES private copies of the 1024 counters in LDS
#define PFXK_HIST_MAX_BLOCKS 1024
#define PFXK_HIST_COPIES 8
// d_hist: 1024 u32 counters R[256] G[256] B[256] L[256], zeroed by a launch of its own, then counted into; d_mask may be NULL
hipError_t pfxk_histogram(hipStream_t s, const uint8_t* d_src, const uint8_t* d_mask, size_t n, uint32_t* d_hist);
// what is uniform over a per-band call: the global sliders after the host's f32 expressions (:1644-1645) and, per band, the factors that do not depend on the
// pixel: hue, saturation / 100.0, lightness * 255.0 / 100.0
typedef struct pfxk_hsl_bands { float g_hue, g_sat, g_light; float hue[6], sat[6], light[6]; } pfxk_hsl_bands;
// the pointwise bank's chunk walk (k_pointwise.h: chunk_walk) with the per-band pixel function: d_mask may be NULL, d_dst may be d_src, sparse_mode as pfxk_adjust
hipError_t pfxk_hsl_bands_apply(hipStream_t s, const uint8_t* d_src, uint8_t* d_dst, const uint8_t* d_mask, const pfxk_hsl_bands* B, int sparse_mode, uint32_t w, uint32_t h);
// :1705-1707 prepared on the host, with expo = 1.0 / fuzz.max(0.01); combine: 0 replace, 1 add, 2 subtract, 3 intersect (:1742-1787)
typedef struct pfxk_color_range { float hue_center, hue_tol, sat_min, expo; uint32_t combine; } pfxk_color_range;
// d_base may be NULL (all zero) and may be d_out; every byte of d_out is written
hipError_t pfxk_color_range_select(hipStream_t s, const uint8_t* d_src, const uint8_t* d_base, uint8_t* d_out, size_t n, const pfxk_color_range* R);

// ---- k_matte.hip ---- background removal around the model (src/ops/ai.rs): preprocess_image :731, is_probability_space :675, mask_confidence_score :706,
// postprocess_mask :766, apply_mask_expansion :850, blur_grayscale :913; host side: pfx_matte.cpp
// the morphology's workgroup owns a PFXK_MATTE_TILE^2 tile and runs up to PFXK_MATTE_K iterations per launch on it and an apron of that many cells in LDS; the
// one-channel resize's output tile (TOY rows while a tile reaches at most TALL_SPAN source columns, TOY_WIDE beyond); the most source columns a tile may reach; the outputs of one workgroup of the feather's row pass and
// the columns of one workgroup of its column pass; the feather's largest radius
#define PFXK_MATTE_TILE 64
#define PFXK_MATTE_K 16
#define PFXK_MATTE_RZ_TOX 64
#define PFXK_MATTE_RZ_TOY 32
#define PFXK_MATTE_RZ_TALL_SPAN 512
#define PFXK_MATTE_RZ_TOY_WIDE 8
#define PFXK_MATTE_RZ_MAX_SPAN 2048
#define PFXK_MATTE_BOX_CHUNK 1024
#define PFXK_MATTE_BOX_COLS 256
#define PFXK_MATTE_MAX_FEATHER 256
// plane c of d_tensor (n floats each) = d_table[c * 256 + channel c of the pixel]; d_table: 768 floats built on the host
hipError_t pfxk_matte_tensor(hipStream_t s, const uint8_t* d_rgba, const float* d_table, float* d_tensor, size_t n);
// d_out[0 .. 3] = the sampled minimum and maximum over the indices 0, step, 2 step, .. as order-preserving u32 keys (PFXK_MATTE_KEY; NaN skipped, the start
// values are FLT_MAX and -FLT_MAX), the decisive count with the values read as probabilities, the decisive count with them read as logits
hipError_t pfxk_matte_score(hipStream_t s, const float* d_values, uint32_t n, uint32_t step, uint32_t* d_out);
#define PFXK_MATTE_KEY(f32_bits) (((f32_bits) & 0x80000000u) ? ~(f32_bits) : ((f32_bits) | 0x80000000u))
// to_probability + postprocess_mask's byte step
hipError_t pfxk_matte_byte(hipStream_t s, const float* d_values, uint8_t* d_grey, size_t n, int is_prob, int smooth, float threshold);
// `iters` (1 .. PFXK_MATTE_K) iterations of apply_mask_expansion's conditional 3 x 3 dilate (or erode) from d_src into d_dst, which share no byte
hipError_t pfxk_matte_morph(hipStream_t s, const uint8_t* d_src, uint8_t* d_dst, uint32_t w, uint32_t h, uint32_t iters, int dilate);
// imageops::resize of one byte per sample, tables as pfxk_resize; span_max at most PFXK_MATTE_RZ_MAX_SPAN.  d_matte (may be NULL) receives the nw x nh matte; with
// d_image the tile's epilogue also writes d_result = d_image with its alpha multiplied by the matte (d_result may be d_image)
hipError_t pfxk_matte_resize(hipStream_t s, const uint8_t* d_grey, const uint32_t* v_left, const uint32_t* v_count, const uint32_t* v_off, const float* v_wts,
                             const uint32_t* h_left, const uint32_t* h_count, const uint32_t* h_off, const float* h_wts, uint32_t w, uint32_t nw, uint32_t nh,
                             uint32_t span_max, uint8_t* d_matte, const uint8_t* d_image, uint8_t* d_result);
// blur_grayscale's two passes, r = 1 .. PFXK_MATTE_MAX_FEATHER: edge-clamped windows of 2 r + 1 samples, integer sums, (sum / count) as u8.  The column pass walks
// bands of `band` rows.  d_src and d_dst share no byte
hipError_t pfxk_matte_box_h(hipStream_t s, const uint8_t* d_src, uint8_t* d_dst, uint32_t w, uint32_t h, uint32_t r);
hipError_t pfxk_matte_box_v(hipStream_t s, const uint8_t* d_src, uint8_t* d_dst, uint32_t w, uint32_t h, uint32_t r, uint32_t band);
// a' = ((a / 255.0) * (m / 255.0) * 255.0).clamp(0, 255) as u8, the rgb copied; d_result may be d_image
hipError_t pfxk_matte_apply(hipStream_t s, const uint8_t* d_image, const uint8_t* d_matte, uint8_t* d_result, size_t n);

#ifdef __cplusplus
}
#endif
