// pfx_select.cpp — C ABI of the selection masks (k_select.hip).  Reference: src/canvas/selection.rs:66-116 (contains, bounds), src/canvas/canvas_state.rs —
// selection_mask_bounds :1632, translate_selection :1677, apply_selection_shape :1713, delete_selected_pixels :1806, fill_selected_pixels :1844;
// src/ui/panels/tools/behavior/raster/perspective_gradient.rs:2-86 (lasso); src/ops/adjustments.rs — feather_selection :1448, expand_selection :1500,
// contract_selection :1547.
// The host computes what is uniform over the image with the reference's own casts (Rust's `as u32` truncates, saturates and sends NaN to 0): the shapes'
// bounding boxes, the feather's pass count and radius, the disc's row spans.  Every check comes before the first launch; the multi-pass ops (feather) run in
// working memory and copy out last, so a failed call leaves the output untouched.
#include <cmath>
#include <vector>

#include "pfx_internal.h"

namespace {

// a mask-to-mask op's declaration: `in` (may be NULL unless in_required) may be `out` itself when same_ok, any other shared byte is refused
int check_masks(pfx_ctx* ctx, const void* in, bool in_required, const void* out, bool same_ok, uint32_t w, uint32_t h, const char* who)
{
    PFX_TRY(pfx_check_dims(ctx, who, w, h));
    const size_t px = (size_t)w * h;
    return pfx_check_args(ctx, who, false, {{in, px, in_required ? PFX_ARG_IN : PFX_ARG_OPTIONAL, in_required ? "mask" : "base_mask"}, {out, px, PFX_ARG_OUT, "mask_out"}},
                          same_ok ? in : nullptr);
}

int check_combine(pfx_ctx* ctx, const void* base, const void* out, uint32_t w, uint32_t h, uint8_t mode, const char* who)
{
    PFX_TRY(check_masks(ctx, base, false, out, true, w, h, who));
    if (mode > 3) return pfx_fail(ctx, PFX_ERR_INVALID, "%s: unknown combine mode %u", who, mode);
    return PFX_OK;
}

pfxk_select_shape rect_shape(uint32_t w, uint32_t h, uint32_t min_x, uint32_t min_y, uint32_t max_x, uint32_t max_y)
{
    pfxk_select_shape S{};
    S.kind = 0;
    S.x0 = min_x; S.y0 = min_y; S.x1 = std::min(max_x, w - 1u); S.y1 = std::min(max_y, h - 1u);   // bounds :96-106
    return S;
}

pfxk_select_shape ellipse_shape(uint32_t w, uint32_t h, float cx, float cy, float rx, float ry)
{
    pfxk_select_shape S{};
    S.kind = 1; S.cx = cx; S.cy = cy; S.rx = rx; S.ry = ry;
    if (rx <= 0.0f || ry <= 0.0f) { S.x0 = S.y0 = 1u; S.x1 = S.y1 = 0u; return S; }   // contains :83
    S.x0 = pfx_f32_as_u32(floorf(fmaxf(cx - rx, 0.0f)));   // bounds :107-113; f32::max and fmaxf both drop a NaN operand
    S.y0 = pfx_f32_as_u32(floorf(fmaxf(cy - ry, 0.0f)));
    S.x1 = std::min(pfx_f32_as_u32(ceilf(cx + rx)), w - 1u);
    S.y1 = std::min(pfx_f32_as_u32(ceilf(cy + ry)), h - 1u);
    return S;
}

int check_lasso(pfx_ctx* ctx, const float* pts, uint32_t n, const char* who)
{
    if (n != 0 && !pts) return pfx_fail(ctx, PFX_ERR_INVALID, "%s: null points", who);
    if (n > PFXK_SELECT_LASSO_MAX) return pfx_fail(ctx, PFX_ERR_UNSUPPORTED, "%s: %u points (at most %d)", who, n, PFXK_SELECT_LASSO_MAX);
    for (size_t i = 0; i < (size_t)n * 2u; ++i)
        if (!(fabsf(pts[i]) <= 1e9f)) return pfx_fail(ctx, PFX_ERR_INVALID, "%s: coordinate %zu is not finite or beyond 1e9", who, i);
    return PFX_OK;
}

int check_feather(pfx_ctx* ctx, float radius, const char* who)
{
    if (!std::isfinite(radius)) return pfx_fail(ctx, PFX_ERR_INVALID, "%s: radius is not finite", who);
    if (radius > (float)PFXK_SELECT_FEATHER_MAX) return pfx_fail(ctx, PFX_ERR_UNSUPPORTED, "%s: radius %g (at most %d)", who, radius, PFXK_SELECT_FEATHER_MAX);
    return PFX_OK;
}

int check_morph(pfx_ctx* ctx, int32_t radius, const char* who)
{
    if (radius > PFXK_SELECT_MORPH_MAX) return pfx_fail(ctx, PFX_ERR_INVALID, "%s: radius %d (at most %d: the square must fit an i32)", who, radius, PFXK_SELECT_MORPH_MAX);
    return PFX_OK;
}

// floor(sqrt(r^2 - k^2)) for k <= r <= PFXK_SELECT_MORPH_MAX: the double root is only a first guess, integer squares decide
uint32_t disc_span(uint32_t r, uint32_t k)
{
    const uint64_t v = (uint64_t)r * r - (uint64_t)k * k;
    uint64_t s = (uint64_t)sqrt((double)v);
    while (s * s > v) --s;
    while ((s + 1u) * (s + 1u) <= v) ++s;
    return (uint32_t)s;
}

// the disc's row spans, uploaded once per radius
int span_table(pfx_ctx* ctx, uint32_t r)
{
    if (ctx->select_span_r == r && ctx->select_span.p) return PFX_OK;
    std::vector<uint16_t> span(r + 1u);
    for (uint32_t k = 0; k <= r; ++k) span[k] = (uint16_t)disc_span(r, k);
    ctx->select_span_r = 0;
    PFX_TRY(pfx_reserve(ctx, ctx->select_span, span.size() * 2u));
    PFX_TRY(pfx_h2d(ctx, ctx->select_span.p, span.data(), span.size() * 2u));
    PFX_TRY(pfx_sync(ctx));   // `span` is pageable host memory about to go out of scope
    ctx->select_span_r = r;
    return PFX_OK;
}

int morph_dev(pfx_ctx* ctx, bool expand, const void* mask_dev, uint32_t w, uint32_t h, int32_t radius, void* out_dev, const char* who)
{
    PFX_TRY(check_masks(ctx, mask_dev, true, out_dev, true, w, h, who));
    PFX_TRY(check_morph(ctx, radius, who));
    const size_t px = (size_t)w * h;
    const uint32_t r = radius > 0 ? (uint32_t)radius : 0u;
    ctx->select_passes = 0; ctx->select_launches = 0;
    if (r == 0u) {   // the disc is the pixel itself, which the rule skips: the identity
        if (out_dev != mask_dev) PFX_HIP(ctx, hipMemcpyAsync(out_dev, mask_dev, px, hipMemcpyDeviceToDevice, ctx->stream));
        return PFX_OK;
    }
    PFX_TRY(span_table(ctx, r));
    PFX_TRY(pfx_reserve(ctx, ctx->select_ws, px * 2u));
    pfx_timer t(ctx, expand ? "selection_expand" : "selection_contract");
    PFX_HIP(ctx, pfxk_select_morph(ctx->stream, expand, (const uint8_t*)mask_dev, (uint16_t*)ctx->select_ws.p, (const uint16_t*)ctx->select_span.p, (uint8_t*)out_dev, w, h, r));
    ctx->select_passes = 1; ctx->select_launches = 2;
    return PFX_OK;
}

// a mask-to-mask op through the staging pair, in place on st_mask: `in` (NULL for a combine op without a base) is uploaded there, dev_call(in, out) runs
template <class F>
int staged(pfx_ctx* ctx, const uint8_t* in, uint32_t w, uint32_t h, uint8_t* out, F&& dev_call)
{
    const size_t px = (size_t)w * h;
    void* m;
    PFX_TRY(pfx_stage(ctx, ctx->st_mask, in, px, &m));
    PFX_TRY(dev_call(in ? m : nullptr, m));
    return pfx_unstage(ctx, out, ctx->st_mask, px);
}

int fill_delete_dev(pfx_ctx* ctx, void* layer_dev, const void* mask_dev, uint32_t w, uint32_t h, const uint8_t* color, bool erase, const char* who)
{
    PFX_TRY(pfx_check_dims(ctx, who, w, h));
    const size_t px = (size_t)w * h;
    PFX_TRY(pfx_check_args(ctx, who, true, {{layer_dev, px * 4, PFX_ARG_OUT | PFX_ARG_DWORD, "layer_dev"}, {mask_dev, px, PFX_ARG_IN, "mask_dev"},
                                            {color, 0, erase ? PFX_ARG_OPTIONAL : PFX_ARG_IN, "color"}}));
    pfx_timer t(ctx, erase ? "selection_delete" : "selection_fill");
    PFX_HIP(ctx, pfxk_select_fill(ctx->stream, (uint8_t*)layer_dev, (const uint8_t*)mask_dev, w, h, erase ? 0u : pfx_pack_rgba8(color), erase));
    return PFX_OK;
}

} // namespace

extern "C" {

int pfx_select_rect_dev(pfx_ctx* ctx, const void* base_mask_dev, uint32_t w, uint32_t h, uint32_t min_x, uint32_t min_y, uint32_t max_x, uint32_t max_y,
                        uint8_t combine_mode, void* mask_out_dev)
{
    PFX_TRY(check_combine(ctx, base_mask_dev, mask_out_dev, w, h, combine_mode, "pfx_select_rect_dev"));
    const pfxk_select_shape S = rect_shape(w, h, min_x, min_y, max_x, max_y);
    pfx_timer t(ctx, "select_rect");
    PFX_HIP(ctx, pfxk_select_shape_combine(ctx->stream, (const uint8_t*)base_mask_dev, (uint8_t*)mask_out_dev, w, h, &S, combine_mode));
    return PFX_OK;
}

int pfx_select_rect(pfx_ctx* ctx, const uint8_t* base_mask, uint32_t w, uint32_t h, uint32_t min_x, uint32_t min_y, uint32_t max_x, uint32_t max_y,
                    uint8_t combine_mode, uint8_t* mask_out)
{
    PFX_TRY(check_combine(ctx, base_mask, mask_out, w, h, combine_mode, "pfx_select_rect"));
    return staged(ctx, base_mask, w, h, mask_out,
                          [&](const void* b, void* o) { return pfx_select_rect_dev(ctx, b, w, h, min_x, min_y, max_x, max_y, combine_mode, o); });
}

int pfx_select_ellipse_dev(pfx_ctx* ctx, const void* base_mask_dev, uint32_t w, uint32_t h, float cx, float cy, float rx, float ry, uint8_t combine_mode,
                           void* mask_out_dev)
{
    PFX_TRY(check_combine(ctx, base_mask_dev, mask_out_dev, w, h, combine_mode, "pfx_select_ellipse_dev"));
    const pfxk_select_shape S = ellipse_shape(w, h, cx, cy, rx, ry);
    pfx_timer t(ctx, "select_ellipse");
    PFX_HIP(ctx, pfxk_select_shape_combine(ctx->stream, (const uint8_t*)base_mask_dev, (uint8_t*)mask_out_dev, w, h, &S, combine_mode));
    return PFX_OK;
}

int pfx_select_ellipse(pfx_ctx* ctx, const uint8_t* base_mask, uint32_t w, uint32_t h, float cx, float cy, float rx, float ry, uint8_t combine_mode,
                       uint8_t* mask_out)
{
    PFX_TRY(check_combine(ctx, base_mask, mask_out, w, h, combine_mode, "pfx_select_ellipse"));
    return staged(ctx, base_mask, w, h, mask_out, [&](const void* b, void* o) { return pfx_select_ellipse_dev(ctx, b, w, h, cx, cy, rx, ry, combine_mode, o); });
}

int pfx_select_lasso_dev(pfx_ctx* ctx, const void* base_mask_dev, uint32_t w, uint32_t h, const float* points_xy, uint32_t n_points, uint8_t combine_mode,
                         void* mask_out_dev)
{
    PFX_TRY(check_combine(ctx, base_mask_dev, mask_out_dev, w, h, combine_mode, "pfx_select_lasso_dev"));
    PFX_TRY(check_lasso(ctx, points_xy, n_points, "pfx_select_lasso_dev"));
    const size_t bytes = (size_t)n_points * 8u;
    PFX_TRY(pfx_reserve(ctx, ctx->select_pts, bytes));
    if (n_points) {
        PFX_TRY(pfx_h2d(ctx, ctx->select_pts.p, points_xy, bytes));
        PFX_TRY(pfx_sync(ctx));   // the points are the caller's pageable memory
    }
    pfx_timer t(ctx, "select_lasso");
    PFX_HIP(ctx, pfxk_select_lasso(ctx->stream, (const float*)ctx->select_pts.p, n_points, (const uint8_t*)base_mask_dev, (uint8_t*)mask_out_dev, w, h, combine_mode));
    return PFX_OK;
}

int pfx_select_lasso(pfx_ctx* ctx, const uint8_t* base_mask, uint32_t w, uint32_t h, const float* points_xy, uint32_t n_points, uint8_t combine_mode,
                     uint8_t* mask_out)
{
    PFX_TRY(check_combine(ctx, base_mask, mask_out, w, h, combine_mode, "pfx_select_lasso"));
    PFX_TRY(check_lasso(ctx, points_xy, n_points, "pfx_select_lasso"));
    return staged(ctx, base_mask, w, h, mask_out, [&](const void* b, void* o) { return pfx_select_lasso_dev(ctx, b, w, h, points_xy, n_points, combine_mode, o); });
}

int pfx_selection_translate_dev(pfx_ctx* ctx, const void* mask_dev, uint32_t w, uint32_t h, int32_t dx, int32_t dy, void* mask_out_dev)
{
    PFX_TRY(check_masks(ctx, mask_dev, true, mask_out_dev, false, w, h, "pfx_selection_translate_dev"));
    pfx_timer t(ctx, "selection_translate");
    PFX_HIP(ctx, pfxk_select_translate(ctx->stream, (const uint8_t*)mask_dev, (uint8_t*)mask_out_dev, w, h, dx, dy));
    return PFX_OK;
}

int pfx_selection_translate(pfx_ctx* ctx, const uint8_t* mask, uint32_t w, uint32_t h, int32_t dx, int32_t dy, uint8_t* mask_out)
{
    PFX_TRY(check_masks(ctx, mask, true, mask_out, false, w, h, "pfx_selection_translate"));
    const size_t px = (size_t)w * h;
    void *d_in, *d_out;
    PFX_TRY(pfx_stage(ctx, ctx->st_tmp, mask, px, &d_in));
    PFX_TRY(pfx_stage(ctx, ctx->st_mask, nullptr, px, &d_out));
    PFX_TRY(pfx_selection_translate_dev(ctx, d_in, w, h, dx, dy, d_out));
    return pfx_unstage(ctx, mask_out, ctx->st_mask, px);
}

int pfx_selection_feather_dev(pfx_ctx* ctx, const void* mask_dev, uint32_t w, uint32_t h, float radius, void* mask_out_dev)
{
    PFX_TRY(check_masks(ctx, mask_dev, true, mask_out_dev, true, w, h, "pfx_selection_feather_dev"));
    PFX_TRY(check_feather(ctx, radius, "pfx_selection_feather_dev"));
    const uint32_t passes = std::max(pfx_f32_as_u32(radius / 2.0f), 1u), r = std::max(pfx_f32_as_u32(radius), 1u);   // :1457-1458
    const size_t px = (size_t)w * h;
    ctx->select_passes = 0; ctx->select_launches = 0;
    PFX_TRY(pfx_reserve(ctx, ctx->select_ws, 2u * pfx_align256(px)));   // a failure leaves mask_out untouched
    uint8_t *a = (uint8_t*)ctx->select_ws.p, *tmp = a + pfx_align256(px);
    pfx_timer t(ctx, "selection_feather");
    for (uint32_t p = 0; p < passes; ++p) {
        PFX_HIP(ctx, pfxk_select_feather_pass(ctx->stream, p == 0 ? (const uint8_t*)mask_dev : a, tmp, a, w, h, r));
        ctx->select_passes += 1; ctx->select_launches += 2;
    }
    PFX_HIP(ctx, hipMemcpyAsync(mask_out_dev, a, px, hipMemcpyDeviceToDevice, ctx->stream));
    return PFX_OK;
}

int pfx_selection_feather(pfx_ctx* ctx, const uint8_t* mask, uint32_t w, uint32_t h, float radius, uint8_t* mask_out)
{
    PFX_TRY(check_masks(ctx, mask, true, mask_out, true, w, h, "pfx_selection_feather"));
    PFX_TRY(check_feather(ctx, radius, "pfx_selection_feather"));
    return staged(ctx, mask, w, h, mask_out, [&](const void* m, void* o) { return pfx_selection_feather_dev(ctx, m, w, h, radius, o); });
}

int pfx_selection_expand_dev(pfx_ctx* ctx, const void* mask_dev, uint32_t w, uint32_t h, int32_t radius, void* mask_out_dev)
{
    return morph_dev(ctx, true, mask_dev, w, h, radius, mask_out_dev, "pfx_selection_expand_dev");
}

int pfx_selection_expand(pfx_ctx* ctx, const uint8_t* mask, uint32_t w, uint32_t h, int32_t radius, uint8_t* mask_out)
{
    PFX_TRY(check_masks(ctx, mask, true, mask_out, true, w, h, "pfx_selection_expand"));
    PFX_TRY(check_morph(ctx, radius, "pfx_selection_expand"));
    return staged(ctx, mask, w, h, mask_out, [&](const void* m, void* o) { return pfx_selection_expand_dev(ctx, m, w, h, radius, o); });
}

int pfx_selection_contract_dev(pfx_ctx* ctx, const void* mask_dev, uint32_t w, uint32_t h, int32_t radius, void* mask_out_dev)
{
    return morph_dev(ctx, false, mask_dev, w, h, radius, mask_out_dev, "pfx_selection_contract_dev");
}

int pfx_selection_contract(pfx_ctx* ctx, const uint8_t* mask, uint32_t w, uint32_t h, int32_t radius, uint8_t* mask_out)
{
    PFX_TRY(check_masks(ctx, mask, true, mask_out, true, w, h, "pfx_selection_contract"));
    PFX_TRY(check_morph(ctx, radius, "pfx_selection_contract"));
    return staged(ctx, mask, w, h, mask_out, [&](const void* m, void* o) { return pfx_selection_contract_dev(ctx, m, w, h, radius, o); });
}

int pfx_selection_bounds_dev(pfx_ctx* ctx, const void* mask_dev, uint32_t w, uint32_t h, int32_t box[4])
{
    PFX_TRY(pfx_check_dims(ctx, "pfx_selection_bounds_dev", w, h));
    PFX_TRY(pfx_check_args(ctx, "pfx_selection_bounds_dev", true, {{mask_dev, (size_t)w * h, PFX_ARG_IN, "mask_dev"}, {box, 0, PFX_ARG_IN, "box"}}));
    PFX_TRY(pfx_reserve(ctx, ctx->d_misc, 4096));
    uint32_t got[4];
    {
        pfx_timer t(ctx, "selection_bounds");
        PFX_HIP(ctx, hipMemsetAsync(ctx->d_misc.p, 0, sizeof got, ctx->stream));
        PFX_HIP(ctx, pfxk_select_bounds(ctx->stream, (const uint8_t*)mask_dev, w, h, (uint32_t*)ctx->d_misc.p));
    }
    PFX_TRY(pfx_d2h(ctx, got, ctx->d_misc.p, sizeof got));
    PFX_TRY(pfx_sync(ctx));
    const bool any = got[0] != 0u;
    box[0] = any ? (int32_t)~got[0] : -1; box[1] = any ? (int32_t)~got[1] : -1;
    box[2] = any ? (int32_t)got[2] : -1;  box[3] = any ? (int32_t)got[3] : -1;
    return PFX_OK;
}

int pfx_selection_fill_dev(pfx_ctx* ctx, void* layer_dev, const void* mask_dev, uint32_t w, uint32_t h, const uint8_t color[4])
{
    return fill_delete_dev(ctx, layer_dev, mask_dev, w, h, color, false, "pfx_selection_fill_dev");
}

int pfx_selection_delete_dev(pfx_ctx* ctx, void* layer_dev, const void* mask_dev, uint32_t w, uint32_t h)
{
    return fill_delete_dev(ctx, layer_dev, mask_dev, w, h, nullptr, true, "pfx_selection_delete_dev");
}

int pfx_int_select_last(pfx_ctx* ctx, int which)
{
    if (!ctx) return -1;
    switch (which) {
        case 0: return PFXK_SELECT_SEG;
        case 1: return PFXK_SELECT_BAND;
        case 2: return PFXK_SELECT_VEC;
        case 3: return PFXK_SELECT_LASSO_MAX;
        case 4: return (int)ctx->select_passes;
        case 5: return (int)ctx->select_launches;
        default: return -1;
    }
}

int pfx_int_select_span(uint32_t r, uint32_t k)
{
    if (r > PFXK_SELECT_MORPH_MAX || k > r) return -1;
    return (int)disc_span(r, k);
}

} // extern "C"
