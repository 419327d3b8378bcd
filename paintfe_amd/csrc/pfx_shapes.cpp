// pfx_shapes.cpp — C ABI of the shape tool's rasteriser (k_shapes.hip).  The bounding box and every value that is uniform over the image are computed
// here, once per call, with the reference's own f32 expressions (no contraction) and the host libm — glibc's cosf / sinf, what Rust's f32::cos / sin
// call on Linux: rotation cos / sin, the polygons' and stars' angles and edge vectors, the vertex lists, the heart's 96-vertex path.
// Reference: src/ops/shapes.rs — rasterize_shape :1169-1305, shape_local_corners :1055, the sdf_* prologues :412-604.
#include <algorithm>
#include <cmath>

#include "pfx_internal.h"

namespace {

constexpr float TAU = 6.28318530717958647692f, PI = 3.14159265358979323846f;

inline int32_t f32_as_i32(float v) { return v != v ? 0 : (v >= 2147483648.0f ? 2147483647 : (v <= -2147483648.0f ? (-2147483647 - 1) : (int32_t)v)); }
inline float rs_max(float a, float b) { return fmaxf(a, b); } // f32::max / min: the non-NaN operand, like fmaxf / fminf
inline float rs_min(float a, float b) { return fminf(a, b); }

const char* shape_problem(const pfx_shape* s)
{
    if (!s) return "null shape";
    if (s->kind >= PFX_SHAPE_COUNT) return "unknown shape kind";
    if (s->fill_mode > PFX_SHAPE_BOTH) return "unknown shape fill mode";
    // the reference's `as i32` would saturate a non-finite box to the whole canvas and fill it with garbage
    if (!std::isfinite(s->cx) || !std::isfinite(s->cy) || !std::isfinite(s->hw) || !std::isfinite(s->hh) || !std::isfinite(s->rotation))
        return "non-finite shape geometry";
    return nullptr;
}

// :1175-1207; false = empty box
bool shape_box(const pfx_shape* s, uint32_t canvas_w, uint32_t canvas_h, int32_t box[4])
{
    const float cos_r = cosf(s->rotation), sin_r = sinf(s->rotation);
    const float hw = s->hw, hh = s->hh;
    float corners[4][2] = {{-hw, -hh}, {hw, -hh}, {hw, hh}, {-hw, hh}};
    if (s->kind == PFX_SHAPE_PARALLELOGRAM) { // shape_local_corners: the skewed vertices
        const float skew = hw * 0.3f;
        corners[2][0] = hw + skew;
        corners[3][0] = -hw + skew;
    }
    float min_x = 3.40282347e+38f, min_y = 3.40282347e+38f, max_x = -3.40282347e+38f, max_y = -3.40282347e+38f;
    for (const auto& c : corners) {
        const float rx = c[0] * cos_r - c[1] * sin_r + s->cx;
        const float ry = c[0] * sin_r + c[1] * cos_r + s->cy;
        min_x = rs_min(min_x, rx); min_y = rs_min(min_y, ry);
        max_x = rs_max(max_x, rx); max_y = rs_max(max_y, ry);
    }
    const float pad = 2.0f;
    min_x -= pad; min_y -= pad; max_x += pad; max_y += pad;
    const int64_t x0 = std::max(f32_as_i32(floorf(min_x)), 0), y0 = std::max(f32_as_i32(floorf(min_y)), 0);
    const int64_t x1 = std::min<int64_t>(f32_as_i32(ceilf(max_x)), (int64_t)canvas_w), y1 = std::min<int64_t>(f32_as_i32(ceilf(max_y)), (int64_t)canvas_h);
    const int64_t bw = std::max<int64_t>(x1 - x0, 0), bh = std::max<int64_t>(y1 - y0, 0);
    if (bw == 0 || bh == 0) { box[0] = box[1] = box[2] = box[3] = 0; return false; }
    box[0] = (int32_t)x0; box[1] = (int32_t)y0; box[2] = (int32_t)bw; box[3] = (int32_t)bh;
    return true;
}

// the kernel's parameter block and SDF id for a shape; layouts of k[] are documented next to the branches of shape_sdf (k_shapes.hip)
int shape_params(const pfx_shape* s, const int32_t box[4], pfxk_shape_params& P)
{
    P = pfxk_shape_params{};
    P.x0 = box[0]; P.y0 = box[1]; P.bw = box[2]; P.bh = box[3];
    const float cos_r = cosf(s->rotation), sin_r = sinf(s->rotation);
    P.cx = s->cx; P.cy = s->cy;
    P.inv_cos = cos_r; P.inv_sin = -sin_r; // inverse rotation = transpose
    const float hx = s->hw, hy = s->hh;
    P.hx = hx; P.hy = hy;
    P.outline_width = rs_max(s->outline_width, 0.0f);
    P.corner_radius = s->corner_radius;
    P.primary = pfx_pack_rgba8(s->primary); P.secondary = pfx_pack_rgba8(s->secondary);
    P.fill_mode = s->fill_mode; P.anti_alias = s->anti_alias != 0;
    auto vert = [&](int i, float x, float y) { P.verts[i][0] = x; P.verts[i][1] = y; };
    auto polygon = [&](uint32_t n) { // sdf_polygon_stretched :425, sdf_polygon :412
        const float r = rs_max(rs_min(hx, hy), 0.001f);
        const float sx = r / rs_max(hx, 0.001f), sy = r / rs_max(hy, 0.001f);
        const float angle = TAU / (float)n, half = angle * 0.5f;
        P.k[0] = r; P.k[1] = sx; P.k[2] = sy; P.k[3] = rs_max(sx, sy); P.k[4] = angle; P.k[5] = half; P.k[6] = r * cosf(half);
        return PFXK_SDF_POLYGON;
    };
    auto star = [&](float ro, float ri, uint32_t n) { // sdf_star :433
        const float angle = PI / (float)n;
        const float cos_a = cosf(angle), sin_a = sinf(angle);
        const float ax = ro, ay = 0.0f, bx = ri * cos_a, by = ri * sin_a;
        const float ex = bx - ax, ey = by - ay;
        P.k[0] = angle; P.k[1] = 2.0f * angle; P.k[2] = ax; P.k[3] = ex; P.k[4] = ey; P.k[5] = ex * ex + ey * ey;
        return PFXK_SDF_STAR;
    };
    switch (s->kind) {
    case PFX_SHAPE_ELLIPSE: return PFXK_SDF_ELLIPSE;
    case PFX_SHAPE_RECTANGLE: return PFXK_SDF_BOX;
    case PFX_SHAPE_ROUNDED_RECT: { // sdf_rounded_box :369
        const float r = rs_min(rs_min(s->corner_radius, hx), hy);
        P.k[0] = r; P.k[1] = hx - r; P.k[2] = hy - r;
        return PFXK_SDF_ROUNDED;
    }
    case PFX_SHAPE_TRAPEZOID: { // :580
        const float top_hw = hx * 0.55f;
        vert(0, -top_hw, -hy); vert(1, top_hw, -hy); vert(2, hx, hy); vert(3, -hx, hy);
        P.n_verts = 4;
        return PFXK_SDF_CONVEX;
    }
    case PFX_SHAPE_PARALLELOGRAM: { // :588
        const float skew = hx * 0.3f;
        vert(0, -hx, -hy); vert(1, hx, -hy); vert(2, hx + skew, hy); vert(3, -hx + skew, hy);
        P.n_verts = 4;
        return PFXK_SDF_CONVEX;
    }
    case PFX_SHAPE_RIGHT_TRIANGLE: // :596
        vert(0, -hx, hy); vert(1, hx, hy); vert(2, -hx, -hy);
        P.n_verts = 3;
        return PFXK_SDF_CONVEX;
    case PFX_SHAPE_TRIANGLE: return PFXK_SDF_TRIANGLE;
    case PFX_SHAPE_PENTAGON: return polygon(5);
    case PFX_SHAPE_HEXAGON: return polygon(6);
    case PFX_SHAPE_OCTAGON: return polygon(8);
    case PFX_SHAPE_CROSS: return PFXK_SDF_CROSS;
    case PFX_SHAPE_CHECK: // :793
        P.k[0] = rs_min(hx, hy) * 0.2f;
        P.k[1] = -hx * 0.7f; P.k[2] = hy * 0.0f; P.k[3] = -hx * 0.1f; P.k[4] = hy * 0.6f;
        P.k[5] = -hx * 0.1f; P.k[6] = hy * 0.6f; P.k[7] = hx * 0.8f;  P.k[8] = -hy * 0.7f;
        return PFXK_SDF_CHECK;
    case PFX_SHAPE_HEART: { // sdf_heart :545-575
        float raw[96][2], max_abs_x = 0.0f, max_abs_y = 0.0f;
        for (int i = 0; i < 96; ++i) {
            const float t = (float)i * TAU / 96.0f;
            const float sn = sinf(t), c = cosf(t);
            const float xr = 16.0f * sn * sn * sn;
            const float yr = 13.0f * c - 5.0f * cosf(2.0f * t) - 2.0f * cosf(3.0f * t) - cosf(4.0f * t);
            max_abs_x = rs_max(max_abs_x, fabsf(xr));
            max_abs_y = rs_max(max_abs_y, fabsf(yr));
            raw[i][0] = xr; raw[i][1] = yr;
        }
        const float sx = max_abs_x > 0.0f ? hx * 0.98f / max_abs_x : 1.0f;
        const float sy = max_abs_y > 0.0f ? hy * 0.98f / max_abs_y : 1.0f;
        for (int i = 0; i < 96; ++i) vert(i, raw[i][0] * sx, -raw[i][1] * sy);
        P.n_verts = 96;
        P.k[0] = hy * 0.18f;
        return PFXK_SDF_HEART;
    }
    case PFX_SHAPE_DIAMOND: // :467
        P.k[0] = 1.0f / sqrtf(1.0f / (hx * hx) + 1.0f / (hy * hy));
        return PFXK_SDF_DIAMOND;
    case PFX_SHAPE_STAR5: return star(rs_min(hx, hy), rs_min(hx, hy) * 0.4f, 5);
    case PFX_SHAPE_STAR6: return star(rs_min(hx, hy), rs_min(hx, hy) * 0.5f, 6);
    default: { // PFX_SHAPE_ARROW :475
        const float shaft_w = hx * 0.55f, shaft_h = hy * 0.35f, head_x = hx * 0.05f;
        const float tw = hx - head_x;
        const float nx = -hy, ny = tw;
        const float nl = sqrtf(nx * nx + ny * ny);
        P.k[0] = (-hx + shaft_w) * 0.5f; P.k[1] = shaft_w * 0.5f + hx * 0.25f; P.k[2] = shaft_h; P.k[3] = head_x; P.k[4] = tw;
        P.k[5] = -hy / nl; P.k[6] = tw / nl; P.k[7] = nl;
        return PFXK_SDF_ARROW;
    }
    }
}

int check_shape_call(pfx_ctx* ctx, const pfx_shape* shape, uint32_t w, uint32_t h, const void* buf, const char* who)
{
    PFX_TRY(pfx_check_dims(ctx, who, w, h));
    PFX_TRY(pfx_check_args(ctx, who, false, {{buf, pfx_img_bytes(w, h), PFX_ARG_OUT, "the image"}}));   // at most the canvas: the box is known once the shape is checked
    if (const char* why = shape_problem(shape)) return pfx_fail(ctx, PFX_ERR_INVALID, "%s: %s", who, why);
    return PFX_OK;
}

int launch_shape(pfx_ctx* ctx, const pfx_shape* shape, int form, uint32_t w, uint32_t h, void* out_dev, const void* selection_dev, uint32_t mode,
                 const char* timer)
{
    int32_t box[4];
    const bool any = shape_box(shape, w, h, box);
    if (!any && form != PFXK_SHAPE_CANVAS) return PFX_OK; // nothing to draw: the buffer / layer stays as it is
    pfxk_shape_params P;
    const int sdf = shape_params(shape, box, P);
    pfx_timer t(ctx, timer);
    PFX_HIP(ctx, pfxk_shape(ctx->stream, form, sdf, &P, (uint8_t*)out_dev, (const uint8_t*)selection_dev, mode, w, h));
    return PFX_OK;
}

} // namespace

extern "C" {

int pfx_shape_bounds(const pfx_shape* shape, uint32_t canvas_w, uint32_t canvas_h, int32_t box[4])
{
    if (!box || !pfx_dims_ok(canvas_w, canvas_h) || shape_problem(shape)) return PFX_ERR_INVALID;
    shape_box(shape, canvas_w, canvas_h, box);
    return PFX_OK;
}

int pfx_shape_rasterize_dev(pfx_ctx* ctx, const pfx_shape* shape, uint32_t canvas_w, uint32_t canvas_h, void* box_dev)
{
    PFX_TRY(check_shape_call(ctx, shape, canvas_w, canvas_h, box_dev, "pfx_shape_rasterize_dev"));
    return launch_shape(ctx, shape, PFXK_SHAPE_BOX, canvas_w, canvas_h, box_dev, nullptr, 0u, "shape_rasterize");
}

int pfx_shape_rasterize(pfx_ctx* ctx, const pfx_shape* shape, uint32_t canvas_w, uint32_t canvas_h, uint8_t* box_rgba)
{
    PFX_TRY(check_shape_call(ctx, shape, canvas_w, canvas_h, box_rgba, "pfx_shape_rasterize"));
    int32_t box[4];
    if (!shape_box(shape, canvas_w, canvas_h, box)) return PFX_OK;
    const size_t bytes = (size_t)box[2] * (size_t)box[3] * 4;
    void* d_box;
    PFX_TRY(pfx_stage(ctx, ctx->st_out, nullptr, bytes, &d_box));
    PFX_TRY(pfx_shape_rasterize_dev(ctx, shape, canvas_w, canvas_h, d_box));
    return pfx_unstage(ctx, box_rgba, ctx->st_out, bytes);
}

int pfx_shape_preview_dev(pfx_ctx* ctx, const pfx_shape* shape, uint32_t canvas_w, uint32_t canvas_h, void* canvas_dev)
{
    PFX_TRY(check_shape_call(ctx, shape, canvas_w, canvas_h, canvas_dev, "pfx_shape_preview_dev"));
    return launch_shape(ctx, shape, PFXK_SHAPE_CANVAS, canvas_w, canvas_h, canvas_dev, nullptr, 0u, "shape_preview");
}

int pfx_shape_preview(pfx_ctx* ctx, const pfx_shape* shape, uint32_t canvas_w, uint32_t canvas_h, uint8_t* canvas_rgba)
{
    PFX_TRY(check_shape_call(ctx, shape, canvas_w, canvas_h, canvas_rgba, "pfx_shape_preview"));
    const size_t bytes = pfx_img_bytes(canvas_w, canvas_h);
    void* d_canvas;
    PFX_TRY(pfx_stage(ctx, ctx->st_out, nullptr, bytes, &d_canvas));
    PFX_TRY(pfx_shape_preview_dev(ctx, shape, canvas_w, canvas_h, d_canvas));
    return pfx_unstage(ctx, canvas_rgba, ctx->st_out, bytes);
}

int pfx_shape_draw_dev(pfx_ctx* ctx, void* layer_dev, uint32_t canvas_w, uint32_t canvas_h, const pfx_shape* shape, uint8_t blend_mode,
                       const void* selection_dev)
{
    PFX_TRY(check_shape_call(ctx, shape, canvas_w, canvas_h, layer_dev, "pfx_shape_draw_dev"));
    return launch_shape(ctx, shape, PFXK_SHAPE_COMMIT, canvas_w, canvas_h, layer_dev, selection_dev, blend_mode > 24 ? 0u : blend_mode, "shape_draw");
}

} // extern "C"
