// pfx_internal.h — context object and host-side helpers behind the C ABI (include/pfx.h).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <initializer_list>
#include <map>
#include <string>
#include <vector>

#include "../../include/pfx.h"
#include "pfx_kernels.h"

struct pfx_devbuf { // grow-on-demand device allocation (never shrinks; freed with the context)
    void* p = nullptr;
    size_t cap = 0;
};

struct pfx_layer_state { // GpuLayerState (ref: src/gpu/renderer.rs:206-209): device-resident, versioned
    pfx_devbuf pixels;
    pfx_devbuf mask;
    pfx_devbuf chunk_flags; // per 64 x 64 chunk: bit 0 = every alpha 255, bit 1 = no alpha 0 (pfxk_chunk_alpha_flags; refreshed with the pixels)
    bool has_mask = false;
    uint32_t w = 0, h = 0;
    uint64_t generation = 0;
};

struct pfx_matte_axes {   // the matte resize's tables on the device, kept for the next call of the same sizes (pfx_matte.cpp: prepare_resize)
    pfx_devbuf buf;
    bool valid = false;
    uint32_t pw = 0, ph = 0, w = 0, h = 0, span_max = 0;
    size_t n_u32 = 0, v_wts = 0;   // u32 entries in front of the weights; vertical weights in front of the horizontal ones
};

struct pfx_timing_rec {
    std::string name;
    hipEvent_t start, stop;
};

struct pfx_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    bool exact = false;
    // sharpen / glow / drop shadow feed a Gaussian into a gain (stylize.rs:96-143, :26-70, render.rs:297): a +-1 LSB input would come out as +-amount, so these
    // effects run the bit-exact Gaussian whatever `exact` says, unless the caller opts out (pfx_tune "gauss_fast_effects" = 1)
    bool gauss_fast_effects = false;
    bool resize_two_pass = false;       // pfx_tune("resize_two_pass"): keep the resamplers' f32 intermediate in HBM (the pre-fusion path)
    std::string err;
    // staging for the host-buffer tier (the reference keeps cached staging/ping-pong textures the same way,
    // ref: src/gpu/renderer.rs:232-236)
    pfx_devbuf st_in, st_out, st_mask, st_tmp, st_aux, st_aux2;
    bool outline_bits = true;  // pfx_tune "outline_bits": the outline's window search on a bit plane of alpha != 0 (0: the per-element scan)
    bool brush_binning = true; // pfx_tune "brush_binning": strokes of more than 64 stamps are dealt to 64 x 64 chunks on the host (pfx_brush_stamps_ex_dev)
    int median_bits_min = 3;   // pfx_tune "median_bits_min", the one per-context knob of pfx_stencil.cpp (see pfx_int_median_path there)
    int last_median_path = -1, last_box_plan = -1;   // what pfx_stencil_median / _box last launched; pfx_int_stencil_last_path reads them, nothing else does
    int last_resize_path = -1, last_resize_span = -1;   // what pfx_resize_image_dev last launched; pfx_int_resize_last reads them, nothing else does
    pfxk_flatten_plan last_flatten_plan = {-1, -1};     // what pfxk_flatten last launched for this context (path -1: nothing yet); pfx_int_flatten_last_path / _plan read it, nothing else does
    pfxk_warp_plan last_warp = {-1, 0u, 0u};            // what the context's last mesh / displacement warp or mesh field launched (flags -1: nothing yet); pfx_int_warp_last reads it, nothing else does
    int last_dab_launch = -1, last_dab_chunks = -1;     // likewise for pfx_displacement_brushes_dev: 0 no launch, 1 the bounding-box launch, 2 the chunk list and its length
    int last_brush_path = -1;                           // what pfx_brush_stamps_ex_dev last did; pfx_int_brush_last reads it, nothing else does
    pfx_devbuf fx_a, fx_b; // effect-bank scratch (crystallize cell table, drop-shadow planes)
    // small parameter buffers
    pfx_devbuf d_desc, d_adj, d_chunks, d_wts, d_lut, d_pts, d_misc;
    bool shadow_plane_blur = true;       // pfx_tune "shadow_plane": the drop shadow blurs its one-channel alpha plane (1) or the reference's (a, a, a, a) image (0); same bits
    bool chain_fuse_heavy = false;       // pfx_tune "chain_fuse_heavy": HSL / vibrance ride in a Gaussian's store as well (A/B; parity tests run both)
    bool chain_mfma_epilogue = true;     // pfx_tune "chain_mfma": 0 = a default-mode Gaussian in a chain runs as its own launch (A/B of the fused store)
    pfx_devbuf st_chain, d_chain_luts;   // pfx_chain_dev: ping-pong image between two stencil stages; the tables of a chain's LUT ops (PFXK_CHAIN_LUTS x 1024)
    pfx_devbuf d_chunk_meta, d_chunk_start;     // per-layer summary pointers + wanted bits, and the per-chunk start table built from them
    std::vector<uint8_t> chunk_meta_cache;
    // whether the table of the stack in chunk_meta_cache skips anything: written by the table kernel into pinned memory (tag), read on a later
    // composite of the same stack once `ev_chunk_useful` has fired — 0 = not built, 1 = pending, 2 = useful (table kept), 3 = useless (no table)
    uint32_t* h_chunk_useful = nullptr;
    hipEvent_t ev_chunk_useful = nullptr;
    // shallow stacks (below dle_min_layers) with a reset layer: whether the elimination kernel pays depends on how coherent the reset layer's alpha is, which a
    // probe kernel samples once per stack; its verdict arrives through pinned memory and is used from a later composite of the same stack on
    // 0 = no probe, 1 = pending, 2 = elimination pays, 3 = it does not
    int dle_probe_state = 0;
    uint32_t* h_dle_verdict = nullptr;
    uint32_t dle_probe_tag = 0;
    hipEvent_t ev_dle_probe = nullptr;
    std::vector<uint8_t> dle_probe_key;   // the probed stack's descriptors + size
    bool dle_adaptive = true;             // pfx_tune "dle_adaptive"
    uint32_t chunk_tag = 0;
    int chunk_state = 0;
    uint64_t store_epoch = 0, chunk_epoch = 0;  // store_epoch moves whenever a stored layer's pixels or mask change
    std::vector<uint8_t> desc_cache, adj_cache; // host copies of what d_desc / d_adj hold (build_stack skips identical uploads)
    std::map<uint32_t, pfx_layer_state> layers;
    bool timing = false;
    std::vector<pfx_timing_rec> timings;
    int n_cus = 0;                  // multiProcessorCount of `device` (persistent-kernel grids)
    // Gaussian tap weights currently resident in d_wts / d_wsplit (re-uploaded only when sigma changes)
    uint32_t wts_sigma_bits = 0, wsplit_sigma_bits = 0;
    bool use_chunk_start = true; // stored layers: per-chunk start table from their alpha summaries (pfx_tune "chunk_start")
    int unorm_store_ok = -1;  // -1 not checked yet, 1 = typed UNORM8 stores round-trip RN(k / 255) exactly on this device (pfxk_unorm_store_check), 0 = they do not
    int stack_mode_class = 0; // set by build_stack: 0 heavy / unknown, 1 medium, 2 light blend arithmetic (pfx_int_flatten_plan picks the streaming kernel's shape from it)
    int dle_min_layers = 16;  // stacks at least this deep may take the compositor's dead-layer elimination kernel (pfx_flatten.cpp: pfx_int_flatten_cands)
    bool wts_valid = false, wsplit_valid = false; // explicit flags: every 32-bit pattern is some sigma (0xffffffff is a NaN)
    float wsplit_inv_scale = 1.0f, wsplit_bias = 0.0f, wsplit_bias_single = 0.0f;
    pfx_devbuf d_wsplit;
    // GpuLiquifyPipeline's cached source texture (ref: src/gpu/compute/liquify.rs:166-176); 0 x 0 = none / invalidated
    pfx_devbuf warp_src;
    uint32_t warp_src_w = 0, warp_src_h = 0;
    pfx_devbuf inpaint_ws;                              // PatchMatch working memory (pfx_inpaint.cpp)
    uint32_t inpaint_peels = 0, inpaint_launches = 0;   // of the context's last PatchMatch call; pfx_int_inpaint_last reads them, nothing else does
    pfx_devbuf flood_ws, flood_lut;                     // flood working memory; the 256-entry srgb_to_linear table, uploaded once (pfx_flood.cpp)
    bool flood_lut_valid = false;
    uint64_t flood_passes = 0, flood_launches = 0, flood_visits = 0;   // of the context's last pfx_flood_distance[_dev]; pfx_int_flood_last reads them
    pfx_devbuf select_ws, select_span, select_pts;      // selection masks (pfx_select.cpp): working memory; the disc's row spans of radius select_span_r; the lasso's points
    uint32_t select_span_r = 0;
    uint32_t select_passes = 0, select_launches = 0;    // of the context's last feather / expand / contract; pfx_int_select_last reads them
    pfx_devbuf colorkey_ws;                             // the colour remover's two u16 level maps, smoothness above one ring chunk only (pfx_colorkey.cpp)
    uint64_t colorkey_flood_passes = 0;                 // of the context's last pfx_color_removal[_dev]; pfx_int_colorkey_last reads them
    uint32_t colorkey_ring_launches = 0, colorkey_launches = 0;
    pfx_devbuf overlay_ws;                              // the floating selection's scaled source (pfx_overlay.cpp); pfx_resize_image_dev itself uses fx_a and st_tmp
    pfx_devbuf textfx_ws;                               // the text styles' planes, blur images and cropped region (pfx_textfx.cpp); the Gaussian itself uses st_tmp
    pfx_devbuf textwarp_ws;                             // a placed text block's warped and rotated buffers (pfx_textwarp.cpp)
    pfx_devbuf matte_ws, matte_tab;                     // background removal (pfx_matte.cpp): the stages' byte planes and the scaled model input; the 768-entry
    bool matte_tab_valid = false;                       // normalisation table, uploaded once
    pfx_matte_axes matte_axes;
};

// ---- error plumbing ----
int pfx_fail(pfx_ctx* ctx, int status, const char* fmt, ...);
#define PFX_HIP(ctx, call)                                                                      \
    do {                                                                                        \
        hipError_t _e = (call);                                                                 \
        if (_e != hipSuccess)                                                                   \
            return pfx_fail((ctx), _e == hipErrorOutOfMemory ? PFX_ERR_OOM : PFX_ERR_HIP,       \
                            "%s failed: %s", #call, hipGetErrorString(_e));                     \
    } while (0)
#define PFX_TRY(expr)            \
    do {                         \
        int _s = (expr);         \
        if (_s != PFX_OK) return _s; \
    } while (0)
#define PFX_REQUIRE(ctx, cond, msg) \
    do {                            \
        if (!(cond)) return pfx_fail((ctx), PFX_ERR_INVALID, "%s", (msg)); \
    } while (0)

// The document-size limit every entry point enforces: non-zero sides and at most 256 M pixels (TiledImage::new clamps beyond that, ref: src/canvas/tiled_image.rs:15-26;
// io.rs:500 refuses sides over 25 000).  The kernels index pixels with 32-bit arithmetic under this bound.
inline bool pfx_dims_ok(uint32_t w, uint32_t h) { return w != 0 && h != 0 && (uint64_t)w * h <= 256000000ull; }
// [x, x + rw) x [y, y + rh) inside w x h, without the 32-bit wrap of x + rw
inline bool pfx_rect_inside(uint32_t x, uint32_t y, uint32_t rw, uint32_t rh, uint32_t w, uint32_t h)
{
    return rw != 0 && rh != 0 && (uint64_t)x + rw <= w && (uint64_t)y + rh <= h;
}

// do [a, a + a_bytes) and [b, b + b_bytes) share a byte?  (aliasing rule of the `_dev` entry points, include/pfx.h)
inline bool pfx_ranges_overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes)
{
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + b_bytes && y < x + a_bytes;
}

// ---- small host helpers every module shares ----
inline size_t pfx_img_bytes(uint32_t w, uint32_t h) { return (size_t)w * h * 4; }
inline size_t pfx_align256(size_t n) { return (n + 255u) & ~(size_t)255u; }
inline uint32_t pfx_pack_rgba8(const uint8_t c[4]) { return (uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16) | ((uint32_t)c[3] << 24); }
inline int pfx_sat_int(uint64_t v) { return v > 0x7fffffffull ? 0x7fffffff : (int)v; }
inline uint32_t pfx_f32_as_u32(float v) { return !(v > 0.0f) ? 0u : (v >= 4294967296.0f ? 0xffffffffu : (uint32_t)v); }   // Rust's `v as u32`: truncates, saturates, NaN -> 0

// ---- helpers (pfx_ctx.cpp) ----
int pfx_use(pfx_ctx* ctx);                                     // hipSetDevice
int pfx_reserve(pfx_ctx* ctx, pfx_devbuf& b, size_t bytes);    // grow-on-demand
int pfx_h2d(pfx_ctx* ctx, void* dst, const void* src, size_t bytes);
int pfx_d2h(pfx_ctx* ctx, void* dst, const void* src, size_t bytes);
int pfx_sync(pfx_ctx* ctx);

// ---- the argument rule of every entry point that takes an image or a mask (pfx_ctx.cpp; the contract itself: include/pfx.h) ----
// An entry point runs its pfx_check_dims line(s), then declares its buffers to pfx_check_args: a required pointer is non-NULL; an OUT buffer shares no byte
// with any other declared buffer, except that it may BE `in_place_with` (the same pointer); a DWORD buffer is 4-byte aligned in a `_dev` call (the kernels
// read a pixel as one dword).  A pointer that is only required (a settings struct, a colour) is declared with 0 bytes.  Every refusal is PFX_ERR_INVALID,
// "<who>: <what is wrong with which argument>"; checks of a single operation (ranges, seeds, finite settings) follow in the entry point.
enum { PFX_ARG_IN = 0, PFX_ARG_OUT = 1, PFX_ARG_OPTIONAL = 2, PFX_ARG_DWORD = 4,
       PFX_ARG_STAGED_OUT = PFX_ARG_IN };   // an output of the older host-buffer wrappers, written from a staged copy once every input has been read: no aliasing rule
struct pfx_buf_arg { const void* p; size_t bytes; int flags; const char* name; };
int pfx_check_dims(pfx_ctx* ctx, const char* who, uint32_t w, uint32_t h);   // NULL ctx: PFX_ERR_INVALID without a message; then pfx_dims_ok
int pfx_check_args(pfx_ctx* ctx, const char* who, bool dev, std::initializer_list<pfx_buf_arg> bufs, const void* in_place_with = nullptr);   // ends in pfx_use(ctx)
// the decision, pure, on plain integers: PFX_ARG_FINE or the kind of the first violation — every NULL first, then every alignment, then every overlap, each
// in declaration order — with *which the offending buffer and *other the buffer it overlaps.  Exported as a test seam (not in include/pfx.h)
enum { PFX_ARG_FINE = 0, PFX_ARG_IS_NULL = 1, PFX_ARG_MISALIGNED = 2, PFX_ARG_OVERLAPS = 3 };
struct pfx_arg_case { uint64_t addr, bytes; int32_t flags; };
extern "C" int pfx_int_check_args(const pfx_arg_case* bufs, int n, int dev, uint64_t in_place_with, int* which, int* other);

// ---- the host-buffer tier's staging pair (pfx_ctx.cpp): the wrapper picks the staging buffer, since several `_dev` calls use some as their own scratch ----
int pfx_stage(pfx_ctx* ctx, pfx_devbuf& buf, const void* host_or_null, size_t bytes, void** dev_ptr);   // reserve, and upload when a host pointer is given
int pfx_unstage(pfx_ctx* ctx, void* host_dst, const pfx_devbuf& buf, size_t bytes);                     // download and sync: the one step that writes the caller's output
inline int pfx_stage_opt(pfx_ctx* ctx, pfx_devbuf& buf, const void* host_or_null, size_t bytes, const void** dev_ptr)   // an optional mask: NULL stays NULL
{
    *dev_ptr = nullptr;
    return host_or_null ? pfx_stage(ctx, buf, host_or_null, bytes, const_cast<void**>(dev_ptr)) : PFX_OK;
}

// RAII-less timing scope: records two events around a launch sequence when ctx->timing is on
struct pfx_timer {
    pfx_ctx* ctx;
    bool on;
    pfx_timing_rec rec;
    pfx_timer(pfx_ctx* c, const char* name);
    ~pfx_timer();
};

// ---- the compositor's host side (pfx_flatten.cpp): pfx_tune's knobs, the layer stack, the one decision which kernel runs and in what shape, the entry points ----
// FAST instantiation of the compositor (k_flatten.hip): requires opacity.clamp(0,1) in [2^-40, 1] for every layer, so
// that (a) every division operand of blend_pixel_static stays in the normal range where v_div_scale / v_div_fixup
// are identities and (b) top_a > 0 for every non-skipped pixel (out_a > 0: no zero check, no clamp).  Anything else
// (zero, negative, tiny or NaN opacity) runs the plain instantiation with IEEE '/', clamps and zero checks.
inline bool opacity_allows_fast_div(float opacity) { return opacity >= 9.094947017729282e-13f; /* 2^-40 */ }
struct pfx_flatten_case {   // plain ints: the test seam fills it from Python
    // the stack: visible layers that became descriptors; the canvas; a live mask or an adjustment layer; a tool preview; the dirty rectangle (0 x 0: whole canvas);
    // every opacity of the call allows the shared-reciprocal division; arithmetic weight of the blend modes (0 heavy / unknown, 1 medium, 2 light)
    int n_desc; uint32_t w, h; int general, has_preview; uint32_t rw, rh; int fast_div, mode_class;
    // reset-layer candidates that survived the depth threshold and the probe, the topmost one's position; the device's UNORM8 conversions are verified exact
    // (pfxk_unorm_store_check: the class-sorting kernel may run); the per-chunk start table is handed to the streaming kernel
    int n_cands, cand_top, unorm_ok, chunk_start;
    // the process-wide knobs as the call found them: pfx_tune "flatten_variant", then "dle_" + units, cfg, sched, frac_a, frac_b, kernel, s1, s2, stats
    int variant, units, cfg, sched, fracA, fracB, kernel, s1, s2, stats;
};
// the decisions, pure, exported as test seams (not in include/pfx.h): the plan's kernel with *plan filled (pfx_kernels.h); the candidate count with *cands and
// *shallow (the stack is below min_layers and `adaptive` leaves the decision to the probe) filled; bit 0 the stack keeps its candidates, bit 1 it is probed now
extern "C" int pfx_int_flatten_plan(const pfx_flatten_case* c, pfxk_flatten_plan* plan);
extern "C" int pfx_int_flatten_cands(const int* modes /* < 0: not a raster layer */, const float* opacities, const uint8_t* masked, uint32_t n, int min_layers, int adaptive,
                                     pfxk_dle_cands* cands, int* shallow);
extern "C" int pfx_int_flatten_verdict(int usable, int same, int probe_state);
// for the tests, what the context's last composite launched (every pfx_composite* / pfx_flatten*_dev entry point ends in pfxk_flatten): the plan, and its path word
// alone — a PFXK_FLATTEN_* kernel (0 the flatten_kernel<GENERAL, F> template, 1 streaming, 2 elimination, 3 class-sorting) | GENERAL << 4 | fast_div << 5 |
// region << 6 | preview << 7 | chunk-start table used << 8 (pfx_kernels.h); -1 = none yet
extern "C" int pfx_int_flatten_last_path(pfx_ctx* ctx);
extern "C" int pfx_int_flatten_last_plan(pfx_ctx* ctx, pfxk_flatten_plan* plan);
int pfx_flatten_tune(pfx_ctx* ctx, const char* key, int value);   // pfx_tune's flatten_variant, dle_* and chunk_start keys
// flatten of device-resident flat layers + the union of the visible layers' TiledImage chunk keys
extern "C" int pfx_int_flatten_with_chunk_keys_dev(pfx_ctx* ctx, const void* const* layer_ptrs_dev, const pfx_layer_info* layers, uint32_t n_layers,
                                                   uint32_t w, uint32_t h, void* dst_dev, const uint8_t* chunk_keys_host);

// ---- the Gaussian's host side (pfx_gauss.cpp): the tap-table caches, the one decision which kernel runs, the launches ----
enum { PFX_GAUSS_PLAIN = 0, PFX_GAUSS_SHARPEN = 1, PFX_GAUSS_GLOW = 2, PFX_GAUSS_CHAIN = 3, PFX_GAUSS_PLANE = 4 };   // what rides in the Gaussian's store
// a path: radius beyond pfxk_gauss_max_radius() | the blur alone (a rider gets a launch of its own behind it) | with the chain / the sharpen, glow or chain in
// its store | the drop shadow's one-channel plane form
enum { PFX_GAUSS_UNSUPPORTED = -1, PFX_GAUSS_MFMA = 0, PFX_GAUSS_FUSED, PFX_GAUSS_TWO_PASS, PFX_GAUSS_MFMA_RIDE, PFX_GAUSS_FUSED_RIDE, PFX_GAUSS_PLANE_FUSED };
struct pfx_gauss_case {   // plain ints: the test seam fills it from Python
    // exact: the effective mode — ctx->exact for a plain blur or a chain, pfx_effect_exact() inside an effect; same: src == dst; overlap: the two images share
    // a byte (src == dst included); ride: PFX_GAUSS_PLAIN ..
    int exact, radius, same, overlap, ride;
    // chain: tables its ops read; pfx_tune "chain_mfma"; it holds an HSL / vibrance op (pfx_chain_dev); pfx_tune "chain_fuse_heavy"
    uint32_t n_luts; int chain_mfma, heavy, fuse_heavy;
    // plane: image width; pfx_tune "shadow_plane", "gauss_fast_effects".  fused_enabled: pfx_tune "gauss_fused_exact" (process-wide)
    uint32_t w; int shadow_plane, fast_effects, fused_enabled;
};
// the decision, pure: a PFX_GAUSS_* path.  Exported as a test seam (not in include/pfx.h)
extern "C" int pfx_int_gauss_path(const pfx_gauss_case* c);
// The Gaussian inside sharpen / glow / drop shadow: bit-exact unless the caller opted out (gauss_fast_effects above).  The reference's tests hold these effects
// at tolerance 0 (tests/visual_filters.rs:43-55,154-165), and the default-mode Gaussian's +-1 LSB would be multiplied by `amount` / `intensity`.
inline bool pfx_effect_exact(const pfx_ctx* ctx) { return ctx->exact || !ctx->gauss_fast_effects; }
// arguments are the caller's to check; `exact` as in pfx_gauss_case
int pfx_gauss_blur(pfx_ctx* ctx, bool exact, const void* src_dev, void* dst_dev, uint32_t w, uint32_t h, float sigma, void* tmp_dev, uint32_t first_row);
int pfx_gauss_combine(pfx_ctx* ctx, bool exact, const void* src_dev, void* dst_dev, uint32_t w, uint32_t h, float sigma, int ride /* _SHARPEN | _GLOW */, float p0, const void* mask_dev, const char* timer);
int pfx_gauss_chain(pfx_ctx* ctx, bool exact, const void* src_dev, void* dst_dev, uint32_t w, uint32_t h, float sigma, const pfxk_chain* C, bool heavy, bool* rode);
bool pfx_gauss_plane_applies(const pfx_ctx* ctx, bool exact, uint32_t w, uint32_t h, int radius);
int pfx_gauss_plane(pfx_ctx* ctx, const void* src_plane, void* dst_plane, uint32_t w, uint32_t h, float sigma);

// ---- the median's and the box blur's host side (pfx_stencil.cpp): pfx_tune's knobs, the one decision which kernel runs, the launches ----
struct pfx_median_case { int radius /* after max(radius, 1) */, bits_min, xlane, single, search1, pair; };   // plain ints: the knobs under their pfx_tune names less "median_"
struct pfx_box_case { int radius /* ceil, >= 1 */, in_place; uint32_t w, h; int strip, two_pass, prefix_from, px_force, py_force, px_switch, py_switch; };
// the decisions, pure, exported as test seams (not in include/pfx.h): a PFX_MEDIAN_* path; the plan's kind with *plan filled (pfx_kernels.h)
extern "C" int pfx_int_median_path(const pfx_median_case* c);
extern "C" int pfx_int_box_plan(const pfx_box_case* c, pfx_box_plan* plan);
extern "C" int pfx_int_stencil_last_path(pfx_ctx* ctx, int which);   // for the tests, what the context's last call ran: which = 0 the median's path, 1 the box blur's kind | h_kind << 4 | px << 8 | py << 16; -1 = none yet
// for the tests, what the context's last pfx_resize_image[_dev] ran: which = 0 the path (0 the device copy of an unchanged size, 1 the fused kernel, 2 the two
// passes through the f32 intermediate), 1 span_max, the widest source-column range of one output tile; -1 = none yet (not in include/pfx.h)
extern "C" int pfx_int_resize_last(pfx_ctx* ctx, int which);
// likewise for the context's last pfx_brush_stamps[_ex][_dev] / pfx_brush_line[_ex]: 0 no launch (no stamp touches a pixel, or the brush is below the radius
// skip), 1 the bounding-box kernel, 2 the binned kernel; -1 = none yet
extern "C" int pfx_int_brush_last(pfx_ctx* ctx);
int pfx_stencil_tune(pfx_ctx* ctx, const char* key, int value);   // pfx_tune's median_* and box_* keys
int pfx_stencil_median(pfx_ctx* ctx, const void* src_dev, void* dst_dev, uint32_t w, uint32_t h, int radius, const void* mask_dev);   // arguments are the caller's to check
int pfx_stencil_box(pfx_ctx* ctx, const void* src_dev, void* dst_dev, uint32_t w, uint32_t h, int radius, const void* mask_dev, void* tmp_dev /* NULL: st_tmp */);

// for the tests, what the context's last call into k_warp.hip launched (not in include/pfx.h).  which = 0 the PFXK_WARP_* bits of the last mesh warp, displacement
// warp or mesh field (1 control points in LDS, 2 PAIR, 4 BUF32, 8 XCD tile order; a launcher sets only the bits it has), 1 / 2 its grid in x / y (the mesh warp's
// tile grid, also when the XCD order launches it in one dimension); 3 the last pfx_displacement_brushes_dev: 0 no launch (no dab reaches the field), 1 the
// launch over the dabs' common bounding box, 2 the launch over the 64 x 64 chunks their boxes touch, 4 the chunks of that list (0 for the others); -1 = none yet
extern "C" int pfx_int_warp_last(pfx_ctx* ctx, int which);
// the compile-time shape of those kernels: which = 0 MESH_WALK, 1 MESH_WX, 2 MESH_LDS_PTS, 3 WARP_YR, 4 the tile rows from which the mesh warp takes the XCD
// order, 5 the dabs culled per trip of the dab loop; -1 = unknown `which`
extern "C" int pfx_int_warp_info(int which);

// for the tests and the profile notes, what the context's last pfx_inpaint_patchmatch[_dev] ran: which = 0 peels, 1 kernel launches (not in include/pfx.h)
extern "C" int pfx_int_inpaint_last(pfx_ctx* ctx, int which);

// for the tests and the profile notes, what the context's last pfx_flood_distance[_dev] (or the contiguous pfx_color_removal[_dev], which runs the same pass
// loop) ran: which = 0 passes, 1 kernel launches, 2 the tile edge, 3 tile visits (the lengths of the passes' tile lists, summed); -1 = unknown `which` or NULL
// context, counts saturate at INT_MAX (not in include/pfx.h)
extern "C" int pfx_int_flood_last(pfx_ctx* ctx, int which);
// the connected flood's working memory carved from ctx->flood_ws, and its pass loop over a device cost map (pfx_flood.cpp): fill W->c, converge, read W->d.
// converge adds to ctx->flood_passes / _launches / _visits; the caller zeroes them first
struct pfx_flood_work { uint32_t* state; uint8_t *c, *d; uint32_t* lists[2]; uint32_t* mark; size_t tiles; };
int pfx_flood_work_reserve(pfx_ctx* ctx, uint32_t w, uint32_t h, pfx_flood_work* W);
int pfx_flood_converge(pfx_ctx* ctx, const pfx_flood_work* W, uint32_t w, uint32_t h, uint32_t seed_x, uint32_t seed_y, int connectivity, const char* who);

// for the tests and the profile notes, what the context's last pfx_color_removal[_dev] ran: which = 0 flood passes (0 in the global scope), 1 ring launches,
// 2 the ring kernel's tile edge, 3 its chunk (levels per launch), 4 kernel launches in all; -1 = unknown `which` or NULL context (not in include/pfx.h)
extern "C" int pfx_int_colorkey_last(pfx_ctx* ctx, int which);

// for the tests and the profile notes, the selection kernels' shape and what the context's last feather / expand / contract ran: which = 0 the pixels of a
// row-walking workgroup's step (a row segment is a multiple of it), 1 the rows of the feather's smallest vertical band, 2 the shape kernel's bytes per lane,
// 3 the lasso's point cap, 4 passes, 5 kernel launches; -1 = unknown `which` or NULL context (not in include/pfx.h)
extern "C" int pfx_int_select_last(pfx_ctx* ctx, int which);
// floor(sqrt(r^2 - k^2)) as the grow / shrink kernels' span table holds it; -1 = k > r or r beyond the cap
extern "C" int pfx_int_select_span(uint32_t r, uint32_t k);

// the half-width of row dy of dilate_mask's disc as the text styles' span table holds it (pfx_textfx.cpp); -1 = the row is skipped, |dy| > ceil(radius), or
// a radius the module refuses (not in include/pfx.h)
extern "C" int pfx_int_textfx_span(float radius, int32_t dy);
// the disc kernel alone, as the text styles' stages run it: build_disc(radius), then one launch between two tight w x h u8 planes on the device (take_min: the
// erosion's minimum).  PFX_ERR_INVALID for a radius that is not finite or not above 0, a bad size, a NULL plane or planes that share a byte, PFX_ERR_UNSUPPORTED
// for ceil(radius) above PFX_TEXT_FX_MAX_RADIUS, each before anything is launched; asynchronous (not in include/pfx.h)
extern "C" int pfx_int_textfx_disc_dev(pfx_ctx* ctx, const void* src_plane, void* dst_plane, uint32_t w, uint32_t h, float radius, int take_min);

// for the tests: the most chunk-list entries pfx_clone_stamp[_dev] / pfx_heal_ring[_dev] put into one launch (a longer stroke goes in consecutive pieces);
// process-wide, 0 = back to the default (8 Mi); returns the previous value (not in include/pfx.h)
extern "C" uint64_t pfx_int_dab_piece_entries(uint64_t entries);
// the same for pfx_line_render[_dev]'s dots (pfx_linetool.cpp): the clear rides with the first piece, the arrowheads with the last
extern "C" uint64_t pfx_int_line_piece_entries(uint64_t entries);

// for the tests: the shape of the histogram kernel (k_colorrange.hip): which = 0 the most workgroups of one launch, 1 the private LDS copies of a workgroup; -1 =
// unknown `which` (not in include/pfx.h)
extern "C" int pfx_int_colorrange_info(int which);

// for the tests: the shape of the matte kernels (k_matte.hip): which = 0 the morphology's tile edge, 1 its iterations per launch (= its apron), 2 / 3 the columns /
// rows of the one-channel resize's output tile, 4 the outputs of one workgroup of the feather's row pass, 5 the columns of one workgroup of its column pass, 6 the
// most source columns one resize tile may reach, 7 the most at which the tile keeps its full height, 8 its rows beyond that; -1 = unknown `which` (not in include/pfx.h)
extern "C" int pfx_int_matte_info(int which);

// for the tests and profiles: the custom-shape kernel (k_customshape.hip): which = 0 the segments of one batch, 1 the slots of an LDS segment list, 2 whether
// culling is on; -1 = unknown `which`.  pfx_int_customshape_cull switches the culling (process-wide, default on) and returns the previous setting: results do
// not depend on it (not in include/pfx.h)
extern "C" int pfx_int_customshape_info(int which);
extern "C" int pfx_int_customshape_cull(int on);

// blur_with_selection on device-resident images (pfx_api.cpp); mask_host may be NULL (= no selection)
int pfx_int_blur_with_selection_dev(pfx_ctx* ctx, const void* d_src, void* d_dst, uint32_t w, uint32_t h, float sigma,
                                    const uint8_t* mask_host, const void* d_mask);

// script front-end on the device image held in ctx->st_in (pfx_script_host.cpp).  On success the result is in ctx->st_in and
// *w / *h hold the final size; console / ops may be NULL.
int pfx_int_script_run_dev(pfx_ctx* ctx, const char* source, uint32_t* w, uint32_t* h, const uint8_t* mask, pfx_script_result* result,
                           std::vector<std::string>* console, std::vector<pfx_canvas_op>* ops);

extern "C" int pfx_int_script_check_limited(const char* source, uint32_t w, uint32_t h, pfx_script_result* result, uint64_t max_ops);
// test seams of the per-pixel closure path (not in include/pfx.h): the compiled form and launch shape of a script's first bulk-iterator closure
// (out[0 .. 9) = n_params, n_regs, n_code, n_pre, heavy, lanes, lcode, LDS bytes, BC_COUNT; then a count per opcode; cap >= 9 + BC_COUNT), and
// pfx_script_check with the whole console
#define PFX_CLOSURE_SHAPE_FIELDS 9
extern "C" int pfx_int_script_closure_shape(const char* source, uint32_t w, uint32_t h, int64_t* out, int cap);
extern "C" int pfx_int_script_check_console(const char* source, uint32_t w, uint32_t h, pfx_script_result* result, char* console, size_t cap, size_t* len);
// the interpreter's f64 libm calls inside closure bodies: trace them, or answer them from a table (pfx_script_host.cpp)
extern "C" int pfx_int_script_libm_hook(int mode, const uint64_t* table, size_t rows);
extern "C" int pfx_int_script_libm_trace(uint64_t* out, size_t cap, size_t* n, uint64_t* misses);

// run_one's script step on a document (pfx_project.cpp): pfx_project_run_script plus the console lines for --verbose
int pfx_int_project_run_script(pfx_ctx* ctx, pfx_project* p, const char* source, pfx_script_result* result, std::vector<std::string>* console);

// host-side restatements that the reference also runs on the host (pfx_host_math.cpp)
int  pfx_host_gaussian_radius(float sigma);                            // ceil(3 sigma) as the reference casts it
int  pfx_host_gaussian_kernel(float sigma, std::vector<float>& out);  // ref: src/ops/filters.rs:214-234
// w * 2^s = w1 + w2 as two f16 arrays (pfxk_gauss_mfma layout); returns 2^-2s, *bias = 1024 * sum(w1 + w2)
float pfx_host_gaussian_split_f16(const std::vector<float>& k, int wlen, int woff, std::vector<uint16_t>& out, float* bias, float* bias_single);
float pfx_host_bc_factor(float contrast);                             // ref: src/ops/adjustments.rs:273
float pfx_host_exposure_gain(float ev);                               // ref: src/ops/adjustments.rs:353
