// pfx_customshape.cpp — C ABI of the shape tool with a custom path and of the picker's icon (k_customshape.hip).  The path arrives as host polylines in every
// tier; it is flattened to segments (windows(2) of every polyline, in order), checked, and staged into context scratch once per call — nothing is cached
// between calls.  The box is pfx_shape_bounds'.  What is uniform over the image is computed here with the reference's own f32 expressions (no contraction):
// bw, bh, sx, sy (custom_shape_coverage_sample, src/ops/shapes.rs:1097-1101), sx.max(sy) and outline_width.max(1.0) (:1109-1110).
#include <atomic>
#include <cmath>
#include <vector>

#include "pfx_internal.h"

namespace {

std::atomic<int> g_cull{1};

struct custom_call {
    std::vector<float> segs;   // x1 y1 x2 y2 per segment
    pfxk_custom_params P{};
};

// the segments of a path: PFX_OK and *count, or PFX_ERR_INVALID (a null pointer where one is needed, a non-finite point or bound, too many segments).
// out == NULL only counts and checks.
int path_segments(const pfx_custom_path* path, float* out, uint32_t cap, uint32_t* count)
{
    if (!path || !count) return PFX_ERR_INVALID;
    *count = 0;
    for (float b : path->bounds)
        if (!std::isfinite(b)) return PFX_ERR_INVALID;
    if (path->n_polylines != 0 && !path->polyline_points) return PFX_ERR_INVALID;
    uint64_t n = 0, first = 0;
    for (uint32_t p = 0; p < path->n_polylines; ++p) {
        const uint32_t pts = path->polyline_points[p];
        if (pts != 0 && !path->points_xy) return PFX_ERR_INVALID;
        for (uint32_t i = 0; i < pts; ++i) {
            const float* v = path->points_xy + 2 * (first + i);
            if (!std::isfinite(v[0]) || !std::isfinite(v[1])) return PFX_ERR_INVALID;
            if (i == 0) continue;
            if (n >= PFX_CUSTOM_SHAPE_MAX_SEGMENTS) return PFX_ERR_INVALID;
            if (out && n < cap) { out[4 * n] = v[-2]; out[4 * n + 1] = v[-1]; out[4 * n + 2] = v[0]; out[4 * n + 3] = v[1]; }
            ++n;
        }
        first += pts;
    }
    *count = (uint32_t)n;
    return out && n > cap ? PFX_ERR_INVALID : PFX_OK;
}

// the path's share of the parameter block, for half extents (hx, hy) and an outline width
int path_params(pfx_ctx* ctx, const char* who, const pfx_custom_path* path, float hx, float hy, float outline_width, custom_call& c)
{
    uint32_t n = 0;
    if (path_segments(path, nullptr, 0, &n) != PFX_OK)
        return pfx_fail(ctx, PFX_ERR_INVALID, "%s: bad path (a null array, a non-finite point or bound, or more than %u segments)", who, PFX_CUSTOM_SHAPE_MAX_SEGMENTS);
    c.segs.resize((size_t)n * 4);
    if (n) path_segments(path, c.segs.data(), n, &n);
    pfxk_custom_params& P = c.P;
    const float min_x = path->bounds[0], min_y = path->bounds[1], max_x = path->bounds[2], max_y = path->bounds[3];
    const float bw = fmaxf(max_x - min_x, 1.0f), bh = fmaxf(max_y - min_y, 1.0f);
    P.hx = hx; P.hy = hy;
    P.sx = bw / fmaxf(hx * 2.0f, 1.0f);
    P.sy = bh / fmaxf(hy * 2.0f, 1.0f);
    P.min_x = min_x; P.min_y = min_y;
    P.max_scale = fmaxf(P.sx, P.sy);
    P.outline_width = fmaxf(outline_width, 1.0f);
    P.reach = nextafterf((float)((double)P.outline_width * (double)P.max_scale * (1.0 + 1.0 / 1024.0)), INFINITY);
    float seg_abs = 0.0f;
    for (float v : c.segs) seg_abs = fmaxf(seg_abs, fabsf(v));
    P.seg_abs = seg_abs;
    P.n_segments = n;
    P.cull = g_cull.load();
    return PFX_OK;
}

// the segments into context scratch; the vector is pageable host memory that dies with the call, so the copy is waited for
int stage_segments(pfx_ctx* ctx, const custom_call& c, const float** d_segs)
{
    const size_t bytes = c.segs.size() * sizeof(float);
    PFX_TRY(pfx_reserve(ctx, ctx->d_pts, bytes));
    if (bytes) {
        PFX_TRY(pfx_h2d(ctx, ctx->d_pts.p, c.segs.data(), bytes));
        PFX_TRY(pfx_sync(ctx));
    }
    *d_segs = (const float*)ctx->d_pts.p;
    return PFX_OK;
}

// every check of a rasterising call, then the box and the parameter block; *any = false: an empty box
int prepare(pfx_ctx* ctx, const char* who, bool dev, const pfx_shape* shape, const pfx_custom_path* path, uint32_t w, uint32_t h, const void* image,
            const void* selection, custom_call& c, bool* any)
{
    PFX_TRY(pfx_check_dims(ctx, who, w, h));
    PFX_TRY(pfx_check_args(ctx, who, dev, {{image, pfx_img_bytes(w, h), PFX_ARG_OUT | PFX_ARG_DWORD, "the image"},   // at most the canvas: the box is known below
                                           {selection, (size_t)w * h, PFX_ARG_OPTIONAL, "the selection"},
                                           {shape, 0, PFX_ARG_IN, "the shape"},
                                           {path, 0, PFX_ARG_IN, "the path"}}));
    int32_t box[4];
    if (pfx_shape_bounds(shape, w, h, box) != PFX_OK) return pfx_fail(ctx, PFX_ERR_INVALID, "%s: bad shape (kind, fill mode or non-finite geometry)", who);
    if (!std::isfinite(shape->outline_width)) return pfx_fail(ctx, PFX_ERR_INVALID, "%s: non-finite outline width", who);
    PFX_TRY(path_params(ctx, who, path, shape->hw, shape->hh, shape->outline_width, c));
    pfxk_custom_params& P = c.P;
    P.x0 = box[0]; P.y0 = box[1]; P.bw = box[2]; P.bh = box[3];
    const float cos_r = cosf(shape->rotation), sin_r = sinf(shape->rotation);
    P.cx = shape->cx; P.cy = shape->cy;
    P.inv_cos = cos_r; P.inv_sin = -sin_r; // inverse rotation = transpose
    P.primary = pfx_pack_rgba8(shape->primary);
    P.fill_mode = shape->fill_mode;
    *any = box[2] > 0 && box[3] > 0;
    return PFX_OK;
}

int launch(pfx_ctx* ctx, const custom_call& c, int form, uint32_t w, uint32_t h, void* out_dev, const void* sel_dev, uint32_t mode, const char* timer)
{
    const float* d_segs;
    PFX_TRY(stage_segments(ctx, c, &d_segs));
    pfx_timer t(ctx, timer);
    PFX_HIP(ctx, pfxk_custom_shape(ctx->stream, form, &c.P, d_segs, (uint8_t*)out_dev, (const uint8_t*)sel_dev, mode, w, h));
    return PFX_OK;
}

int prepare_icon(pfx_ctx* ctx, const char* who, bool dev, const pfx_custom_path* path, uint32_t size, const void* rgba, custom_call& c)
{
    PFX_TRY(pfx_check_dims(ctx, who, size, size));
    if (size > 1024u) return pfx_fail(ctx, PFX_ERR_INVALID, "%s: icon size %u is above 1024", who, size);
    PFX_TRY(pfx_check_args(ctx, who, dev, {{rgba, pfx_img_bytes(size, size), PFX_ARG_OUT | PFX_ARG_DWORD, "the icon"}, {path, 0, PFX_ARG_IN, "the path"}}));
    return path_params(ctx, who, path, 0.82f, 0.82f, 0.04f, c);
}

} // namespace

extern "C" {

int pfx_int_customshape_info(int which) { return which == 0 ? PFXK_CUSTOM_BATCH : which == 1 ? PFXK_CUSTOM_LIST : which == 2 ? g_cull.load() : -1; }
int pfx_int_customshape_cull(int on) { return g_cull.exchange(on != 0); }

int pfx_custom_shape_segments(const pfx_custom_path* path, float* seg_xyxy, uint32_t cap, uint32_t* n_segments)
{
    if (!seg_xyxy && cap != 0) return PFX_ERR_INVALID;
    return path_segments(path, seg_xyxy, cap, n_segments);
}

int pfx_custom_shape_rasterize_dev(pfx_ctx* ctx, const pfx_shape* shape, const pfx_custom_path* path, uint32_t w, uint32_t h, void* buf_dev)
{
    custom_call c;
    bool any;
    PFX_TRY(prepare(ctx, "pfx_custom_shape_rasterize_dev", true, shape, path, w, h, buf_dev, nullptr, c, &any));
    if (!any) return PFX_OK; // nothing to draw: the buffer stays as it is
    return launch(ctx, c, PFXK_SHAPE_BOX, w, h, buf_dev, nullptr, 0u, "custom_shape_rasterize");
}

int pfx_custom_shape_rasterize(pfx_ctx* ctx, const pfx_shape* shape, const pfx_custom_path* path, uint32_t w, uint32_t h, uint8_t* buf_rgba)
{
    custom_call c;
    bool any;
    PFX_TRY(prepare(ctx, "pfx_custom_shape_rasterize", false, shape, path, w, h, buf_rgba, nullptr, c, &any));
    if (!any) return PFX_OK;
    const size_t bytes = (size_t)c.P.bw * (size_t)c.P.bh * 4;
    void* d_box;
    PFX_TRY(pfx_stage(ctx, ctx->st_out, nullptr, bytes, &d_box));
    PFX_TRY(launch(ctx, c, PFXK_SHAPE_BOX, w, h, d_box, nullptr, 0u, "custom_shape_rasterize"));
    return pfx_unstage(ctx, buf_rgba, ctx->st_out, bytes);
}

int pfx_custom_shape_preview_dev(pfx_ctx* ctx, const pfx_shape* shape, const pfx_custom_path* path, uint32_t w, uint32_t h, void* preview_dev)
{
    custom_call c;
    bool any;
    PFX_TRY(prepare(ctx, "pfx_custom_shape_preview_dev", true, shape, path, w, h, preview_dev, nullptr, c, &any));
    return launch(ctx, c, PFXK_SHAPE_CANVAS, w, h, preview_dev, nullptr, 0u, "custom_shape_preview");
}

int pfx_custom_shape_preview(pfx_ctx* ctx, const pfx_shape* shape, const pfx_custom_path* path, uint32_t w, uint32_t h, uint8_t* preview_rgba)
{
    custom_call c;
    bool any;
    PFX_TRY(prepare(ctx, "pfx_custom_shape_preview", false, shape, path, w, h, preview_rgba, nullptr, c, &any));
    const size_t bytes = pfx_img_bytes(w, h);
    void* d_canvas;
    PFX_TRY(pfx_stage(ctx, ctx->st_out, nullptr, bytes, &d_canvas));
    PFX_TRY(launch(ctx, c, PFXK_SHAPE_CANVAS, w, h, d_canvas, nullptr, 0u, "custom_shape_preview"));
    return pfx_unstage(ctx, preview_rgba, ctx->st_out, bytes);
}

int pfx_custom_shape_draw_dev(pfx_ctx* ctx, void* image_dev, uint32_t w, uint32_t h, const pfx_shape* shape, const pfx_custom_path* path,
                              uint8_t blend_mode, const void* sel_dev)
{
    custom_call c;
    bool any;
    PFX_TRY(prepare(ctx, "pfx_custom_shape_draw_dev", true, shape, path, w, h, image_dev, sel_dev, c, &any));
    if (!any) return PFX_OK; // nothing to draw: the layer stays as it is
    return launch(ctx, c, PFXK_SHAPE_COMMIT, w, h, image_dev, sel_dev, blend_mode > 24 ? 0u : blend_mode, "custom_shape_draw");
}

int pfx_custom_shape_icon_dev(pfx_ctx* ctx, const pfx_custom_path* path, uint32_t size, int dark, void* rgba_dev)
{
    custom_call c;
    PFX_TRY(prepare_icon(ctx, "pfx_custom_shape_icon_dev", true, path, size, rgba_dev, c));
    const float* d_segs;
    PFX_TRY(stage_segments(ctx, c, &d_segs));
    pfx_timer t(ctx, "custom_shape_icon");
    PFX_HIP(ctx, pfxk_custom_icon(ctx->stream, &c.P, d_segs, (uint8_t*)rgba_dev, size, dark ? 235u : 30u));
    return PFX_OK;
}

int pfx_custom_shape_icon(pfx_ctx* ctx, const pfx_custom_path* path, uint32_t size, int dark, uint8_t* rgba)
{
    custom_call c;
    PFX_TRY(prepare_icon(ctx, "pfx_custom_shape_icon", false, path, size, rgba, c));
    const size_t bytes = pfx_img_bytes(size, size);
    void* d_icon;
    PFX_TRY(pfx_stage(ctx, ctx->st_out, nullptr, bytes, &d_icon));
    const float* d_segs;
    PFX_TRY(stage_segments(ctx, c, &d_segs));
    {
        pfx_timer t(ctx, "custom_shape_icon");
        PFX_HIP(ctx, pfxk_custom_icon(ctx->stream, &c.P, d_segs, (uint8_t*)d_icon, size, dark ? 235u : 30u));
    }
    return pfx_unstage(ctx, rgba, ctx->st_out, bytes);
}

} // extern "C"
