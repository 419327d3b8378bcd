// pfx_overlay.cpp — C ABI of the floating selection (k_overlay.hip).  Reference: src/ops/clipboard.rs — PasteOverlay :818, extract_to_overlay :729,
// transformed_bounds :939, rasterize_for_clipboard :1048, render_replacement_preview :1144, corners_canvas :1313, commit :2032, render_preview :2168.
// pfx_overlay_geometry derives everything that is uniform over the image with the reference's own f32 expressions (no contraction; cosf / sinf once per
// call): the scaled size, the corners, the three boxes.  Every entry point starts with it, checks its buffers, and only then reserves and launches.  The scale
// step is pfx_resize_image_dev into ctx->overlay_ws (that call keeps its tables in fx_a and, for strong downscales, an f32 plane in st_tmp: neither is used
// here); a scaled size equal to the source's reads the source itself, which is what the resize would copy.  The preview needs no scaled image at all: its
// scale is always NEAREST, an index lookup.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "pfx_internal.h"

namespace {

inline float rs_round(float v) { return roundf(v); }   // f32::round: half away from zero
inline int32_t f32_as_i32(float v)                     // Rust's `v as i32`: truncates, saturates, NaN -> 0
{
    if (v != v) return 0;
    return v <= -2147483648.0f ? INT32_MIN : (v >= 2147483648.0f ? INT32_MAX : (int32_t)v);
}

struct bbox { float min_x, min_y, max_x, max_y; };
bbox fold_corners(const float c[8], float min_x, float min_y, float max_x, float max_y)   // f32::min / max: fminf / fmaxf
{
    bbox b{min_x, min_y, max_x, max_y};
    for (int k = 0; k < 4; ++k) {
        b.min_x = fminf(b.min_x, c[2 * k]);     b.min_y = fminf(b.min_y, c[2 * k + 1]);
        b.max_x = fmaxf(b.max_x, c[2 * k]);     b.max_y = fmaxf(b.max_y, c[2 * k + 1]);
    }
    return b;
}

int geometry(pfx_ctx* ctx, const char* who, const pfx_overlay* ov, pfx_overlay_geom* G)
{
    if (!ov || !G) return pfx_fail(ctx, PFX_ERR_INVALID, "%s: the descriptor is null", who);
    const float f[7] = {ov->center_x, ov->center_y, ov->rotation, ov->scale_x, ov->scale_y, ov->anchor_x, ov->anchor_y};
    for (float v : f)
        if (!std::isfinite(v)) return pfx_fail(ctx, PFX_ERR_INVALID, "%s: a float of the descriptor is not finite", who);
    if (ov->interpolation < PFX_RESIZE_NEAREST || ov->interpolation > PFX_RESIZE_LANCZOS3)
        return pfx_fail(ctx, PFX_ERR_INVALID, "%s: unknown interpolation %d", who, ov->interpolation);
    if (!pfx_dims_ok(ov->doc_w, ov->doc_h)) return pfx_fail(ctx, PFX_ERR_INVALID, "%s: bad document size %ux%u", who, ov->doc_w, ov->doc_h);
    if (!pfx_dims_ok(ov->source_w, ov->source_h)) return pfx_fail(ctx, PFX_ERR_INVALID, "%s: bad source size %ux%u", who, ov->source_w, ov->source_h);
    const float src_w = (float)ov->source_w, src_h = (float)ov->source_h, cw = (float)ov->doc_w, ch = (float)ov->doc_h;
    pfx_overlay_geom g;
    std::memset(&g, 0, sizeof g);
    g.scaled_w = pfx_f32_as_u32(fmaxf(rs_round(src_w * ov->scale_x), 1.0f));   // :2046
    g.scaled_h = pfx_f32_as_u32(fmaxf(rs_round(src_h * ov->scale_y), 1.0f));
    if (!pfx_dims_ok(g.scaled_w, g.scaled_h)) return pfx_fail(ctx, PFX_ERR_INVALID, "%s: bad scaled size %ux%u", who, g.scaled_w, g.scaled_h);
    g.cos_r = cosf(ov->rotation);
    g.sin_r = sinf(ov->rotation);
    // corners_canvas :1313 through rotate_point :1300, from scaled_half :1269 (not the rounded size)
    const float hx = src_w * ov->scale_x / 2.0f, hy = src_h * ov->scale_y / 2.0f;
    const float ax = ov->center_x + ov->anchor_x, ay = ov->center_y + ov->anchor_y;
    const float px[4] = {ov->center_x - hx, ov->center_x + hx, ov->center_x - hx, ov->center_x + hx};
    const float py[4] = {ov->center_y - hy, ov->center_y - hy, ov->center_y + hy, ov->center_y + hy};
    for (int k = 0; k < 4; ++k) {
        const float dx = px[k] - ax, dy = py[k] - ay;
        g.corners[2 * k] = ax + dx * g.cos_r - dy * g.sin_r;
        g.corners[2 * k + 1] = ay + dx * g.sin_r + dy * g.cos_r;
    }
    const bbox b = fold_corners(g.corners, cw, ch, 0.0f, 0.0f);   // :2056-2065
    g.row_start = pfx_f32_as_u32(fmaxf(floorf(b.min_y), 0.0f));
    g.row_end = pfx_f32_as_u32(fminf(ceilf(b.max_y), ch - 1.0f));
    g.col_start = pfx_f32_as_u32(fmaxf(floorf(b.min_x), 0.0f));
    g.col_end = pfx_f32_as_u32(fminf(ceilf(b.max_x), cw - 1.0f));
    g.bounds[0] = pfx_f32_as_u32(fminf(fmaxf(floorf(b.min_x), 0.0f), cw));   // :954-958, the same folds
    g.bounds[1] = pfx_f32_as_u32(fminf(fmaxf(floorf(b.min_y), 0.0f), ch));
    g.bounds[2] = pfx_f32_as_u32(fminf(fmaxf(ceilf(b.max_x), 0.0f), cw));
    g.bounds[3] = pfx_f32_as_u32(fminf(fmaxf(ceilf(b.max_y), 0.0f), ch));
    g.has_bounds = g.bounds[2] > g.bounds[0] && g.bounds[3] > g.bounds[1];
    const bbox r = fold_corners(g.corners, 3.40282347e38f, 3.40282347e38f, -3.40282347e38f, -3.40282347e38f);   // :1061-1070
    g.raster_col = f32_as_i32(floorf(r.min_x));
    g.raster_row = f32_as_i32(floorf(r.min_y));
    const int64_t rw = (int64_t)f32_as_i32(ceilf(r.max_x)) - g.raster_col + 1, rh = (int64_t)f32_as_i32(ceilf(r.max_y)) - g.raster_row + 1;
    g.raster_w = rw <= 0 ? 0u : (rw > 0xffffffffll ? 0xffffffffu : (uint32_t)rw);   // :1076: col_end < col_start is None
    g.raster_h = rh <= 0 ? 0u : (rh > 0xffffffffll ? 0xffffffffu : (uint32_t)rh);
    if (!g.raster_w || !g.raster_h) g.raster_w = g.raster_h = 0u;
    *G = g;
    return PFX_OK;
}

// what the kernels take; the window is the caller's
pfxk_overlay kernel_params(const pfx_overlay* ov, const pfx_overlay_geom& G)
{
    pfxk_overlay P;
    std::memset(&P, 0, sizeof P);
    P.ax = ov->center_x + ov->anchor_x;   // anchor_canvas :1292
    P.ay = ov->center_y + ov->anchor_y;
    P.cos_r = G.cos_r;
    P.sin_r = G.sin_r;
    P.origin_x = ov->center_x - (float)G.scaled_w / 2.0f;   // :2074
    P.origin_y = ov->center_y - (float)G.scaled_h / 2.0f;
    P.ratio_x = (float)ov->source_w / (float)G.scaled_w;    // pfx_resize.cpp:build_axis
    P.ratio_y = (float)ov->source_h / (float)G.scaled_h;
    P.scaled_w = G.scaled_w; P.scaled_h = G.scaled_h;
    P.source_w = ov->source_w; P.source_h = ov->source_h;
    return P;
}

void commit_window(pfxk_overlay& P, const pfx_overlay* ov, const pfx_overlay_geom& G)
{
    // the ends are below the document's size, except that `cw as f32 - 1.0` can round up to cw on a side above 2^24, where the reference's put_pixel would
    // panic: the launch stays inside the document
    const uint32_t col_end = std::min(G.col_end, ov->doc_w - 1u), row_end = std::min(G.row_end, ov->doc_h - 1u);
    const bool any = G.col_start <= col_end && G.row_start <= row_end;
    P.x0 = (int32_t)G.col_start; P.y0 = (int32_t)G.row_start;
    P.box_w = any ? col_end - G.col_start + 1u : 0u;
    P.box_h = any ? row_end - G.row_start + 1u : 0u;
    if (!any) P.x0 = P.y0 = 0;
    P.out_x0 = P.out_y0 = 0;
    P.pitch = ov->doc_w;
}

// the source scaled with the overlay's filter: the source itself at equal size (the resize copies there), else into ctx->overlay_ws
int scaled_source(pfx_ctx* ctx, const pfx_overlay* ov, const pfx_overlay_geom& G, const void* source_dev, const void** scaled)
{
    *scaled = source_dev;
    if (G.scaled_w == ov->source_w && G.scaled_h == ov->source_h) return PFX_OK;
    PFX_TRY(pfx_reserve(ctx, ctx->overlay_ws, pfx_img_bytes(G.scaled_w, G.scaled_h)));
    PFX_TRY(pfx_resize_image_dev(ctx, source_dev, ov->source_w, ov->source_h, ctx->overlay_ws.p, G.scaled_w, G.scaled_h, ov->interpolation));
    *scaled = ctx->overlay_ws.p;
    return PFX_OK;
}

int check_commit(pfx_ctx* ctx, const char* who, bool dev, const pfx_overlay* ov, const void* source, const void* mask, const void* base, const void* out, pfx_overlay_geom* G)
{
    if (!ctx) return PFX_ERR_INVALID;
    PFX_TRY(geometry(ctx, who, ov, G));
    const size_t src_px = (size_t)ov->source_w * ov->source_h, doc = pfx_img_bytes(ov->doc_w, ov->doc_h);
    return pfx_check_args(ctx, who, dev, {{source, src_px * 4, PFX_ARG_DWORD, "source"}, {mask, src_px, PFX_ARG_OPTIONAL, "the overwrite mask"},
                                          {base, doc, PFX_ARG_DWORD, "base"}, {out, doc, PFX_ARG_OUT | PFX_ARG_DWORD, "out"}}, base);
}

} // namespace

extern "C" {

int pfx_overlay_geometry(const pfx_overlay* ov, pfx_overlay_geom* out) { return geometry(nullptr, "pfx_overlay_geometry", ov, out); }

int pfx_overlay_commit_dev(pfx_ctx* ctx, const pfx_overlay* ov, const void* source_dev, const void* overwrite_mask_dev, const void* base_dev, void* out_dev)
{
    const char* who = "pfx_overlay_commit_dev";
    pfx_overlay_geom G;
    PFX_TRY(check_commit(ctx, who, true, ov, source_dev, overwrite_mask_dev, base_dev, out_dev, &G));
    pfxk_overlay P = kernel_params(ov, G);
    commit_window(P, ov, G);
    const void* scaled = source_dev;
    if (P.box_w) PFX_TRY(scaled_source(ctx, ov, G, source_dev, &scaled));   // before out is touched
    if (out_dev != base_dev) PFX_HIP(ctx, hipMemcpyAsync(out_dev, base_dev, pfx_img_bytes(ov->doc_w, ov->doc_h), hipMemcpyDeviceToDevice, ctx->stream));
    if (!P.box_w) return PFX_OK;
    const int overwrite = !ov->overwrite_transparent ? 0 : (overwrite_mask_dev ? 2 : 1);
    pfx_timer t(ctx, "overlay_commit");
    PFX_HIP(ctx, pfxk_overlay_commit(ctx->stream, (const uint8_t*)scaled, (const uint8_t*)overwrite_mask_dev, (uint8_t*)out_dev, &P, ov->anti_aliasing != 0, overwrite));
    return PFX_OK;
}

int pfx_overlay_commit(pfx_ctx* ctx, const pfx_overlay* ov, const uint8_t* source, const uint8_t* overwrite_mask, const uint8_t* base, uint8_t* out)
{
    pfx_overlay_geom G;
    PFX_TRY(check_commit(ctx, "pfx_overlay_commit", false, ov, source, overwrite_mask, base, out, &G));
    const size_t src_px = (size_t)ov->source_w * ov->source_h, doc = pfx_img_bytes(ov->doc_w, ov->doc_h);
    void *d_src, *d_img;
    const void* d_mask;
    PFX_TRY(pfx_stage(ctx, ctx->st_in, source, src_px * 4, &d_src));
    PFX_TRY(pfx_stage_opt(ctx, ctx->st_mask, overwrite_mask, src_px, &d_mask));
    PFX_TRY(pfx_stage(ctx, ctx->st_out, base, doc, &d_img));
    PFX_TRY(pfx_overlay_commit_dev(ctx, ov, d_src, d_mask, d_img, d_img));   // in place
    return pfx_unstage(ctx, out, ctx->st_out, doc);
}

int pfx_overlay_preview_dev(pfx_ctx* ctx, const pfx_overlay* ov, const void* source_dev, void* preview_dev)
{
    const char* who = "pfx_overlay_preview_dev";
    if (!ctx) return PFX_ERR_INVALID;
    pfx_overlay_geom G;
    PFX_TRY(geometry(ctx, who, ov, &G));   // the whole descriptor is checked, although the scale here is always NEAREST :2184
    PFX_TRY(pfx_check_args(ctx, who, true, {{source_dev, pfx_img_bytes(ov->source_w, ov->source_h), PFX_ARG_DWORD, "source_dev"},
                                            {preview_dev, pfx_img_bytes(ov->doc_w, ov->doc_h), PFX_ARG_OUT | PFX_ARG_DWORD, "preview_dev"}}));
    pfxk_overlay P = kernel_params(ov, G);
    const bool translate = fabsf(ov->rotation) < 0.0001f && fabsf(ov->anchor_x) < 0.001f && fabsf(ov->anchor_y) < 0.001f;   // :2197
    if (translate) {
        const int32_t ox = f32_as_i32(rs_round(P.origin_x)), oy = f32_as_i32(rs_round(P.origin_y));   // :2202
        // [max(origin, 0), min(origin + scaled, doc)); the reference wraps a negative origin + scaled to a huge u32 and panics on its first read: nothing here
        const int64_t x0 = ox > 0 ? ox : 0, y0 = oy > 0 ? oy : 0;
        const int64_t x1 = std::min<int64_t>((int64_t)ox + G.scaled_w, ov->doc_w), y1 = std::min<int64_t>((int64_t)oy + G.scaled_h, ov->doc_h);
        const bool any = x1 > x0 && y1 > y0;
        P.x0 = any ? (int32_t)x0 : 0; P.y0 = any ? (int32_t)y0 : 0;
        P.box_w = any ? (uint32_t)(x1 - x0) : 0u; P.box_h = any ? (uint32_t)(y1 - y0) : 0u;
        P.out_x0 = ox; P.out_y0 = oy;
        P.pitch = ov->doc_w;
    } else {
        commit_window(P, ov, G);   // :2245-2248 is commit's box
    }
    pfx_timer t(ctx, "overlay_preview");
    PFX_HIP(ctx, pfxk_overlay_preview(ctx->stream, (const uint8_t*)source_dev, (uint8_t*)preview_dev, ov->doc_w, ov->doc_h, &P, translate));
    return PFX_OK;
}

int pfx_overlay_rasterize_dev(pfx_ctx* ctx, const pfx_overlay* ov, const void* source_dev, void* out_dev, int* has_pixels)
{
    const char* who = "pfx_overlay_rasterize_dev";
    if (!ctx) return PFX_ERR_INVALID;
    pfx_overlay_geom G;
    PFX_TRY(geometry(ctx, who, ov, &G));
    if (G.raster_w && !pfx_dims_ok(G.raster_w, G.raster_h)) return pfx_fail(ctx, PFX_ERR_INVALID, "%s: bad raster window %ux%u", who, G.raster_w, G.raster_h);
    PFX_TRY(pfx_check_args(ctx, who, true, {{source_dev, pfx_img_bytes(ov->source_w, ov->source_h), PFX_ARG_DWORD, "source_dev"},
                                            {out_dev, pfx_img_bytes(G.raster_w, G.raster_h), PFX_ARG_OUT | PFX_ARG_DWORD, "out_dev"}, {has_pixels, 0, PFX_ARG_IN, "has_pixels"}}));
    if (!G.raster_w) { *has_pixels = 0; return PFX_OK; }
    pfxk_overlay P = kernel_params(ov, G);
    P.x0 = P.out_x0 = G.raster_col; P.y0 = P.out_y0 = G.raster_row;
    P.box_w = P.pitch = G.raster_w; P.box_h = G.raster_h;
    const void* scaled;
    PFX_TRY(scaled_source(ctx, ov, G, source_dev, &scaled));
    PFX_TRY(pfx_reserve(ctx, ctx->d_misc, 4096));
    uint32_t any = 0;
    {
        pfx_timer t(ctx, "overlay_rasterize");
        PFX_HIP(ctx, hipMemsetAsync(ctx->d_misc.p, 0, sizeof any, ctx->stream));
        PFX_HIP(ctx, hipMemsetAsync(out_dev, 0, pfx_img_bytes(G.raster_w, G.raster_h), ctx->stream));
        PFX_HIP(ctx, pfxk_overlay_rasterize(ctx->stream, (const uint8_t*)scaled, (uint8_t*)out_dev, &P, ov->anti_aliasing != 0, (uint32_t*)ctx->d_misc.p));
    }
    PFX_TRY(pfx_d2h(ctx, &any, ctx->d_misc.p, sizeof any));
    PFX_TRY(pfx_sync(ctx));
    *has_pixels = any != 0u;
    return PFX_OK;
}

int pfx_overlay_extract_dev(pfx_ctx* ctx, void* layer_dev, const void* selection_dev, uint32_t doc_w, uint32_t doc_h, void* clip_dev, void* clip_mask_dev, pfx_overlay* out)
{
    const char* who = "pfx_overlay_extract_dev";
    PFX_TRY(pfx_check_dims(ctx, who, doc_w, doc_h));
    const size_t px = (size_t)doc_w * doc_h;
    PFX_TRY(pfx_check_args(ctx, who, true, {{layer_dev, px * 4, PFX_ARG_OUT | PFX_ARG_DWORD, "layer_dev"}, {selection_dev, px, PFX_ARG_OPTIONAL, "selection_dev"},
                                            {clip_dev, px * 4, PFX_ARG_OUT | PFX_ARG_DWORD, "clip_dev"},
                                            {clip_mask_dev, px, PFX_ARG_OUT | (selection_dev ? 0 : PFX_ARG_OPTIONAL), "clip_mask_dev"}, {out, 0, PFX_ARG_IN, "out"}}));
    PFX_TRY(pfx_reserve(ctx, ctx->d_misc, 4096));
    uint32_t got[4] = {0, 0, 0, 0};
    PFX_HIP(ctx, hipMemsetAsync(ctx->d_misc.p, 0, sizeof got, ctx->stream));
    if (selection_dev) PFX_HIP(ctx, pfxk_select_bounds(ctx->stream, (const uint8_t*)selection_dev, doc_w, doc_h, (uint32_t*)ctx->d_misc.p));
    else PFX_HIP(ctx, pfxk_overlay_any_alpha(ctx->stream, (const uint8_t*)layer_dev, px, (uint32_t*)ctx->d_misc.p));   // has_content :796
    PFX_TRY(pfx_d2h(ctx, got, ctx->d_misc.p, sizeof got));
    PFX_TRY(pfx_sync(ctx));
    pfx_overlay o;
    std::memset(&o, 0, sizeof o);
    if (got[0] == 0u) { *out = o; return PFX_OK; }   // :759, :797: None
    o.doc_w = doc_w; o.doc_h = doc_h;
    o.scale_x = o.scale_y = 1.0f;                      // PasteOverlay::new :893
    o.interpolation = PFX_RESIZE_BILINEAR;
    o.anti_aliasing = 1;
    pfx_timer t(ctx, "overlay_extract");
    if (selection_dev) {
        const uint32_t min_x = ~got[0], min_y = ~got[1], bw = got[2] - min_x + 1u, bh = got[3] - min_y + 1u;
        if (got[2] >= doc_w || got[3] >= doc_h || min_x > got[2] || min_y > got[3]) return pfx_fail(ctx, PFX_ERR_HIP, "%s: the selection's box came back outside the document", who);
        PFX_HIP(ctx, pfxk_overlay_lift(ctx->stream, (const uint8_t*)layer_dev, (const uint8_t*)selection_dev, (uint8_t*)clip_dev, (uint8_t*)clip_mask_dev, doc_w, min_x, min_y, bw, bh));
        PFX_HIP(ctx, pfxk_select_fill(ctx->stream, (uint8_t*)layer_dev, (const uint8_t*)selection_dev, doc_w, doc_h, 0u, 1));   // delete_selected_pixels :780
        o.source_w = bw; o.source_h = bh;
        o.center_x = (float)min_x + (float)bw / 2.0f;   // :784
        o.center_y = (float)min_y + (float)bh / 2.0f;
    } else {
        PFX_HIP(ctx, hipMemcpyAsync(clip_dev, layer_dev, px * 4, hipMemcpyDeviceToDevice, ctx->stream));
        PFX_HIP(ctx, hipMemsetAsync(layer_dev, 0, px * 4, ctx->stream));
        o.source_w = doc_w; o.source_h = doc_h;
        o.center_x = (float)doc_w / 2.0f;               // :807
        o.center_y = (float)doc_h / 2.0f;
    }
    *out = o;
    return PFX_OK;
}

} // extern "C"
