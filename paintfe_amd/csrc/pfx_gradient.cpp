// pfx_gradient.cpp — C ABI of the gradient tool and the perspective crop (k_gradient.hip).  Reference: src/ui/panels/tools/state.rs — rebuild_lut :1063,
// apply_preset :1144; src/ui/panels/tools/behavior/raster/perspective_gradient.rs — apply_perspective_crop :94, render_gradient_to_preview :244 (its CPU path
// :386-548); gradient_text/gradient_controls.rs — commit_gradient :63.  The LUT builder, the presets, the eraser bake, the drag scale and the crop plan are plain
// host code, callable without a context; what is uniform over the image (the direction terms of :415-422) is derived here with the reference's own f32
// expressions (no contraction).  Every entry point checks its sizes, then its descriptor and buffers, and only then uploads and launches.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "pfx_internal.h"

namespace {

inline uint8_t round_u8(float v) { return (uint8_t)std::min(pfx_f32_as_u32(roundf(v)), 255u); }   // `.round() as u8`: half away from zero, saturating, NaN -> 0
// u32::div_ceil without the wrap of dim + scale - 1
inline uint32_t div_ceil(uint32_t dim, uint32_t scale) { return (uint32_t)(((uint64_t)dim + scale - 1u) / scale); }

// the descriptor's own checks; `who` names the entry point
int check_gradient(pfx_ctx* ctx, const char* who, const pfx_gradient* g, const uint8_t* lut)
{
    if (!g || !lut) return pfx_fail(ctx, PFX_ERR_INVALID, "%s: the descriptor or the LUT is null", who);
    for (float v : {g->start_x, g->start_y, g->end_x, g->end_y})
        if (!std::isfinite(v)) return pfx_fail(ctx, PFX_ERR_INVALID, "%s: start or end is not finite", who);
    if (g->shape < PFX_GRADIENT_LINEAR || g->shape > PFX_GRADIENT_DIAMOND) return pfx_fail(ctx, PFX_ERR_INVALID, "%s: unknown shape %d", who, g->shape);
    if (g->mode != PFX_GRADIENT_MODE_COLOR && g->mode != PFX_GRADIENT_MODE_TRANSPARENCY) return pfx_fail(ctx, PFX_ERR_INVALID, "%s: unknown mode %d", who, g->mode);
    if (g->preview_scale == 0u) return pfx_fail(ctx, PFX_ERR_INVALID, "%s: preview_scale is 0", who);
    return PFX_OK;
}

// :415-430
pfxk_gradient kernel_params(const pfx_gradient* g, uint32_t w, uint32_t h)
{
    pfxk_gradient P;
    std::memset(&P, 0, sizeof P);
    P.ax = g->start_x; P.ay = g->start_y;
    P.dx = g->end_x - g->start_x;
    P.dy = g->end_y - g->start_y;
    const float len_sq = P.dx * P.dx + P.dy * P.dy;
    const float len = sqrtf(len_sq);
    P.inv_len = len > 1e-6f ? 1.0f / len : 0.0f;
    P.inv_len_sq = len_sq > 1e-6f ? 1.0f / len_sq : 0.0f;
    P.ux = P.dx * P.inv_len;
    P.uy = P.dy * P.inv_len;
    P.scale = g->preview_scale;
    P.scale_f = (float)g->preview_scale;
    P.gen_w = div_ceil(w, P.scale);   // :301-310
    P.gen_h = div_ceil(h, P.scale);
    P.w = w;
    P.shape = g->shape;
    P.repeat = g->repeat != 0;
    P.eraser = g->mode == PFX_GRADIENT_MODE_TRANSPARENCY;
    return P;
}

// the LUT the kernels read: baked in transparency mode, uploaded into ctx->d_lut
int upload_lut(pfx_ctx* ctx, const pfx_gradient* g, const uint8_t* lut)
{
    uint8_t baked[1024];
    if (g->mode == PFX_GRADIENT_MODE_TRANSPARENCY) pfx_gradient_bake_eraser_lut(lut, baked);
    else std::memcpy(baked, lut, sizeof baked);
    PFX_TRY(pfx_reserve(ctx, ctx->d_lut, 1024));
    return pfx_h2d(ctx, ctx->d_lut.p, baked, sizeof baked);
}

struct crop_plan { uint32_t out_w, out_h; };
int plan_crop(const float* c, uint32_t w, uint32_t h, crop_plan* out)
{
    if (!c || !out || !pfx_dims_ok(w, h)) return PFX_ERR_INVALID;
    for (int k = 0; k < 8; ++k)
        if (!std::isfinite(c[k])) return PFX_ERR_INVALID;
    float min_x = INFINITY, min_y = INFINITY, max_x = -INFINITY, max_y = -INFINITY;   // the folds of :100-119: f32::min / max are fminf / fmaxf
    for (int k = 0; k < 4; ++k) {
        min_x = fminf(min_x, c[2 * k]);     min_y = fminf(min_y, c[2 * k + 1]);
        max_x = fmaxf(max_x, c[2 * k]);     max_y = fmaxf(max_y, c[2 * k + 1]);
    }
    min_x = fmaxf(min_x, 0.0f);             min_y = fmaxf(min_y, 0.0f);
    max_x = fminf(max_x, (float)w);         max_y = fminf(max_y, (float)h);
    out->out_w = pfx_f32_as_u32(roundf(max_x - min_x));   // :121
    out->out_h = pfx_f32_as_u32(roundf(max_y - min_y));
    if (out->out_w < 2u || out->out_h < 2u) out->out_w = out->out_h = 0u;   // the reference's None :123
    return PFX_OK;
}

} // namespace

extern "C" {

int pfx_gradient_build_lut(const pfx_gradient_stop* stops, uint32_t n_stops, uint8_t lut[1024])
{
    if (!lut || (n_stops && !stops)) return PFX_ERR_INVALID;
    for (uint32_t i = 0; i < n_stops; ++i)
        if (!std::isfinite(stops[i].position)) return PFX_ERR_INVALID;
    if (n_stops == 0u) { std::memset(lut, 0, 1024); return PFX_OK; }                         // :1066
    if (n_stops == 1u) {                                                                     // :1071
        for (int i = 0; i < 256; ++i) std::memcpy(lut + 4 * i, stops[0].color, 4);
        return PFX_OK;
    }
    std::vector<pfx_gradient_stop> sorted(stops, stops + n_stops);
    std::stable_sort(sorted.begin(), sorted.end(), [](const pfx_gradient_stop& a, const pfx_gradient_stop& b) { return a.position < b.position; });   // :1085, positions are finite
    const pfx_gradient_stop &first = sorted.front(), &last = sorted.back();
    for (int i = 0; i < 256; ++i) {
        const float t = (float)i / 255.0f;
        uint8_t* o = lut + 4 * i;
        if (t <= first.position) { std::memcpy(o, first.color, 4); continue; }
        if (t >= last.position) { std::memcpy(o, last.color, 4); continue; }
        const pfx_gradient_stop *left = &first, *right = &last;
        for (size_t j = 0; j + 1 < sorted.size(); ++j)
            if (sorted[j].position <= t && sorted[j + 1].position >= t) { left = &sorted[j]; right = &sorted[j + 1]; break; }   // the first bracketing pair wins
        const float span = right->position - left->position;
        const float local_t = span > 0.0f ? (t - left->position) / span : 0.0f;
        const float inv = 1.0f - local_t;
        for (int k = 0; k < 4; ++k) o[k] = round_u8((float)left->color[k] * inv + (float)right->color[k] * local_t);
    }
    return PFX_OK;
}

int pfx_gradient_preset_stops(int preset, const uint8_t primary[4], const uint8_t secondary[4], pfx_gradient_stop stops_out[PFX_GRADIENT_MAX_PRESET_STOPS],
                              uint32_t* n_stops_out)
{
    if (!primary || !secondary || !stops_out || !n_stops_out) return PFX_ERR_INVALID;
    auto stop = [](float position, uint8_t r, uint8_t g, uint8_t b, uint8_t a) { return pfx_gradient_stop{position, {r, g, b, a}}; };
    switch (preset) {
    case PFX_GRADIENT_PRESET_PRIMARY_SECONDARY:
        stops_out[0] = stop(0.0f, primary[0], primary[1], primary[2], primary[3]);
        stops_out[1] = stop(1.0f, secondary[0], secondary[1], secondary[2], secondary[3]);
        *n_stops_out = 2;
        return PFX_OK;
    case PFX_GRADIENT_PRESET_BLACK_WHITE:
        stops_out[0] = stop(0.0f, 0, 0, 0, 255);
        stops_out[1] = stop(1.0f, 255, 255, 255, 255);
        *n_stops_out = 2;
        return PFX_OK;
    case PFX_GRADIENT_PRESET_FOREGROUND_TRANSPARENT:
        stops_out[0] = stop(0.0f, primary[0], primary[1], primary[2], primary[3]);
        stops_out[1] = stop(1.0f, primary[0], primary[1], primary[2], 0);
        *n_stops_out = 2;
        return PFX_OK;
    case PFX_GRADIENT_PRESET_RAINBOW:
        stops_out[0] = stop(0.0f, 255, 0, 0, 255);
        stops_out[1] = stop(0.17f, 255, 165, 0, 255);
        stops_out[2] = stop(0.33f, 255, 255, 0, 255);
        stops_out[3] = stop(0.5f, 0, 200, 0, 255);
        stops_out[4] = stop(0.67f, 0, 100, 255, 255);
        stops_out[5] = stop(0.83f, 75, 0, 130, 255);
        stops_out[6] = stop(1.0f, 148, 0, 211, 255);
        *n_stops_out = 7;
        return PFX_OK;
    default:
        return PFX_ERR_INVALID;   // Custom leaves the stops alone: nothing to return
    }
}

int pfx_gradient_bake_eraser_lut(const uint8_t lut[1024], uint8_t baked[1024])
{
    if (!lut || !baked) return PFX_ERR_INVALID;
    for (int i = 0; i < 256; ++i) {
        const uint8_t* s = lut + 4 * i;
        const uint32_t lum = pfx_f32_as_u32(0.299f * (float)s[0] + 0.587f * (float)s[1] + 0.114f * (float)s[2]);   // `as u8`: at most 255.00002, saturating
        const uint32_t a = std::min(lum, 255u) * s[3] / 255u;
        baked[4 * i] = baked[4 * i + 1] = baked[4 * i + 2] = 255;
        baked[4 * i + 3] = (uint8_t)a;
    }
    return PFX_OK;
}

uint32_t pfx_gradient_drag_scale(uint32_t w, uint32_t h)
{
    const uint64_t total = (uint64_t)w * h;
    if (total <= 1500000ull) return 1u;
    const double s = ceil(sqrt((double)total / 1000000.0));   // at most 4294.97 for u32 sides: the `as u32` cast never saturates
    return std::max((uint32_t)s, 2u);
}

int pfx_gradient_render_dev(pfx_ctx* ctx, const pfx_gradient* g, const uint8_t* lut, const void* sel_dev, uint32_t w, uint32_t h, void* preview_dev, void* premul_dev)
{
    const char* who = "pfx_gradient_render_dev";
    PFX_TRY(pfx_check_dims(ctx, who, w, h));
    PFX_TRY(check_gradient(ctx, who, g, lut));
    const size_t gen = pfx_img_bytes(div_ceil(w, g->preview_scale), div_ceil(h, g->preview_scale));
    PFX_TRY(pfx_check_args(ctx, who, true, {{sel_dev, (size_t)w * h, PFX_ARG_OPTIONAL, "sel_dev"}, {preview_dev, gen, PFX_ARG_OUT | PFX_ARG_DWORD, "preview_dev"},
                                            {premul_dev, gen, PFX_ARG_OUT | PFX_ARG_OPTIONAL | PFX_ARG_DWORD, "premul_dev"}}));
    const pfxk_gradient P = kernel_params(g, w, h);
    PFX_TRY(upload_lut(ctx, g, lut));
    pfx_timer t(ctx, "gradient_render");
    PFX_HIP(ctx, pfxk_gradient_render(ctx->stream, (const uint32_t*)ctx->d_lut.p, (const uint8_t*)sel_dev, (uint8_t*)preview_dev, (uint8_t*)premul_dev, &P));
    return PFX_OK;
}

int pfx_gradient_render(pfx_ctx* ctx, const pfx_gradient* g, const uint8_t* lut, const uint8_t* sel, uint32_t w, uint32_t h, uint8_t* preview, uint8_t* premul)
{
    const char* who = "pfx_gradient_render";
    PFX_TRY(pfx_check_dims(ctx, who, w, h));
    PFX_TRY(check_gradient(ctx, who, g, lut));
    const size_t gen = pfx_img_bytes(div_ceil(w, g->preview_scale), div_ceil(h, g->preview_scale));
    PFX_TRY(pfx_check_args(ctx, who, false, {{sel, (size_t)w * h, PFX_ARG_OPTIONAL, "sel"}, {preview, gen, PFX_ARG_OUT, "preview"},
                                             {premul, gen, PFX_ARG_OUT | PFX_ARG_OPTIONAL, "premul"}}));
    const void* d_sel;
    void *d_preview, *d_premul = nullptr;
    PFX_TRY(pfx_stage_opt(ctx, ctx->st_mask, sel, (size_t)w * h, &d_sel));
    PFX_TRY(pfx_stage(ctx, ctx->st_out, nullptr, gen, &d_preview));
    if (premul) PFX_TRY(pfx_stage(ctx, ctx->st_aux, nullptr, gen, &d_premul));
    PFX_TRY(pfx_gradient_render_dev(ctx, g, lut, d_sel, w, h, d_preview, d_premul));
    if (premul) PFX_TRY(pfx_d2h(ctx, premul, d_premul, gen));
    return pfx_unstage(ctx, preview, ctx->st_out, gen);
}

int pfx_gradient_commit_dev(pfx_ctx* ctx, void* active_layer_dev, const void* preview_dev, uint32_t w, uint32_t h, int is_eraser)
{
    const char* who = "pfx_gradient_commit_dev";
    PFX_TRY(pfx_check_dims(ctx, who, w, h));
    PFX_TRY(pfx_check_args(ctx, who, true, {{active_layer_dev, pfx_img_bytes(w, h), PFX_ARG_OUT | PFX_ARG_DWORD, "active_layer_dev"},
                                            {preview_dev, pfx_img_bytes(w, h), PFX_ARG_DWORD, "preview_dev"}}));
    pfx_timer t(ctx, "gradient_commit");
    PFX_HIP(ctx, pfxk_gradient_commit(ctx->stream, (uint8_t*)active_layer_dev, (const uint8_t*)preview_dev, (size_t)w * h, is_eraser != 0));
    return PFX_OK;
}

int pfx_gradient_commit(pfx_ctx* ctx, uint8_t* active_layer_inout, const uint8_t* preview, uint32_t w, uint32_t h, int is_eraser)
{
    const char* who = "pfx_gradient_commit";
    PFX_TRY(pfx_check_dims(ctx, who, w, h));
    const size_t bytes = pfx_img_bytes(w, h);
    PFX_TRY(pfx_check_args(ctx, who, false, {{active_layer_inout, bytes, PFX_ARG_OUT, "active_layer_inout"}, {preview, bytes, PFX_ARG_IN, "preview"}}));
    void *d_layer, *d_preview;
    PFX_TRY(pfx_stage(ctx, ctx->st_in, active_layer_inout, bytes, &d_layer));
    PFX_TRY(pfx_stage(ctx, ctx->st_out, preview, bytes, &d_preview));
    PFX_TRY(pfx_gradient_commit_dev(ctx, d_layer, d_preview, w, h, is_eraser));
    return pfx_unstage(ctx, active_layer_inout, ctx->st_in, bytes);
}

int pfx_gradient_apply_dev(pfx_ctx* ctx, const pfx_gradient* g, const uint8_t* lut, const void* sel_dev, void* active_layer_dev, uint32_t w, uint32_t h)
{
    const char* who = "pfx_gradient_apply_dev";
    PFX_TRY(pfx_check_dims(ctx, who, w, h));
    PFX_TRY(check_gradient(ctx, who, g, lut));
    if (g->preview_scale != 1u) return pfx_fail(ctx, PFX_ERR_INVALID, "%s: preview_scale is %u (the release renders at 1)", who, g->preview_scale);
    PFX_TRY(pfx_check_args(ctx, who, true, {{sel_dev, (size_t)w * h, PFX_ARG_OPTIONAL, "sel_dev"},
                                            {active_layer_dev, pfx_img_bytes(w, h), PFX_ARG_OUT | PFX_ARG_DWORD, "active_layer_dev"}}));
    const pfxk_gradient P = kernel_params(g, w, h);   // scale 1: gen_w x gen_h is w x h
    PFX_TRY(upload_lut(ctx, g, lut));
    pfx_timer t(ctx, "gradient_apply");
    PFX_HIP(ctx, pfxk_gradient_apply(ctx->stream, (const uint32_t*)ctx->d_lut.p, (const uint8_t*)sel_dev, (uint8_t*)active_layer_dev, &P));
    return PFX_OK;
}

int pfx_perspective_crop_plan(const float corners_xy[8], uint32_t w, uint32_t h, uint32_t* out_w, uint32_t* out_h)
{
    crop_plan p;
    if (!out_w || !out_h) return PFX_ERR_INVALID;
    PFX_TRY(plan_crop(corners_xy, w, h, &p));
    *out_w = p.out_w;
    *out_h = p.out_h;
    return PFX_OK;
}

int pfx_perspective_crop_dev(pfx_ctx* ctx, const float corners_xy[8], const void* const* layer_ptrs_dev, void* const* cropped_ptrs_dev, uint32_t n_layers, uint32_t w,
                             uint32_t h)
{
    const char* who = "pfx_perspective_crop_dev";
    PFX_TRY(pfx_check_dims(ctx, who, w, h));
    if (!corners_xy || !layer_ptrs_dev || !cropped_ptrs_dev) return pfx_fail(ctx, PFX_ERR_INVALID, "%s: the corners or a pointer array is null", who);
    if (n_layers == 0u || n_layers > PFX_CROP_MAX_LAYERS) return pfx_fail(ctx, PFX_ERR_INVALID, "%s: %u layers (1 .. %d)", who, n_layers, PFX_CROP_MAX_LAYERS);
    crop_plan plan;
    if (plan_crop(corners_xy, w, h, &plan) != PFX_OK) return pfx_fail(ctx, PFX_ERR_INVALID, "%s: a corner is not finite", who);
    if (!pfx_dims_ok(plan.out_w, plan.out_h)) return pfx_fail(ctx, PFX_ERR_INVALID, "%s: the quad crops to nothing (%ux%u)", who, plan.out_w, plan.out_h);
    const size_t in_bytes = pfx_img_bytes(w, h), out_bytes = pfx_img_bytes(plan.out_w, plan.out_h);
    for (uint32_t l = 0; l < n_layers; ++l) {
        const void *in = layer_ptrs_dev[l], *out = cropped_ptrs_dev[l];
        if (!in || !out) return pfx_fail(ctx, PFX_ERR_INVALID, "%s: layer %u: a null pointer", who, l);
        if (((uintptr_t)in | (uintptr_t)out) & 3u) return pfx_fail(ctx, PFX_ERR_INVALID, "%s: layer %u: a pointer is not 4-byte aligned", who, l);
    }
    for (uint32_t o = 0; o < n_layers; ++o) {   // an output shares no byte with any input or any other output
        for (uint32_t l = 0; l < n_layers; ++l) {
            if (pfx_ranges_overlap(cropped_ptrs_dev[o], out_bytes, layer_ptrs_dev[l], in_bytes))
                return pfx_fail(ctx, PFX_ERR_INVALID, "%s: output %u overlaps layer %u", who, o, l);
            if (l != o && pfx_ranges_overlap(cropped_ptrs_dev[o], out_bytes, cropped_ptrs_dev[l], out_bytes))
                return pfx_fail(ctx, PFX_ERR_INVALID, "%s: output %u overlaps output %u", who, o, l);
        }
    }
    PFX_TRY(pfx_use(ctx));
    pfxk_crop P;
    std::memset(&P, 0, sizeof P);
    for (int k = 0; k < 4; ++k) { P.cx[k] = corners_xy[2 * k]; P.cy[k] = corners_xy[2 * k + 1]; }
    P.w = w; P.h = h; P.out_w = plan.out_w; P.out_h = plan.out_h; P.n_layers = n_layers;
    const size_t table = (size_t)n_layers * sizeof(void*);
    PFX_TRY(pfx_reserve(ctx, ctx->d_misc, std::max<size_t>(2 * table, 4096)));
    PFX_TRY(pfx_h2d(ctx, ctx->d_misc.p, layer_ptrs_dev, table));
    PFX_TRY(pfx_h2d(ctx, (uint8_t*)ctx->d_misc.p + table, cropped_ptrs_dev, table));
    pfx_timer t(ctx, "perspective_crop");
    PFX_HIP(ctx, pfxk_perspective_crop(ctx->stream, (const uint8_t* const*)ctx->d_misc.p, (uint8_t* const*)((uint8_t*)ctx->d_misc.p + table), &P));
    return PFX_OK;
}

int pfx_perspective_crop(pfx_ctx* ctx, const float corners_xy[8], const uint8_t* layer, uint8_t* cropped, size_t cropped_bytes, uint32_t w, uint32_t h)
{
    const char* who = "pfx_perspective_crop";
    PFX_TRY(pfx_check_dims(ctx, who, w, h));
    crop_plan plan;
    if (plan_crop(corners_xy, w, h, &plan) != PFX_OK) return pfx_fail(ctx, PFX_ERR_INVALID, "%s: the corners are null or not finite", who);
    if (!pfx_dims_ok(plan.out_w, plan.out_h)) return pfx_fail(ctx, PFX_ERR_INVALID, "%s: the quad crops to nothing (%ux%u)", who, plan.out_w, plan.out_h);
    const size_t in_bytes = pfx_img_bytes(w, h), out_bytes = pfx_img_bytes(plan.out_w, plan.out_h);
    if (cropped_bytes < out_bytes) return pfx_fail(ctx, PFX_ERR_INVALID, "%s: cropped_bytes %zu is below the plan's %zu", who, cropped_bytes, out_bytes);
    PFX_TRY(pfx_check_args(ctx, who, false, {{layer, in_bytes, PFX_ARG_IN, "layer"}, {cropped, out_bytes, PFX_ARG_OUT, "cropped"}}));
    void *d_in, *d_out;
    PFX_TRY(pfx_stage(ctx, ctx->st_in, layer, in_bytes, &d_in));
    PFX_TRY(pfx_stage(ctx, ctx->st_out, nullptr, out_bytes, &d_out));
    const void* ins[1] = {d_in};
    void* outs[1] = {d_out};
    PFX_TRY(pfx_perspective_crop_dev(ctx, corners_xy, ins, outs, 1u, w, h));
    return pfx_unstage(ctx, cropped, ctx->st_out, out_bytes);
}

} // extern "C"
