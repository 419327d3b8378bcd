// pfx_textfx.cpp — C ABI of the text layer's styles (k_textfx.hip).  Reference: src/ops/text_layer/effects.rs — apply_text_effects :1, composite_over :47,
// render_outline :80, render_outline_inside :118, dilate_mask :167, render_shadow :222, render_inner_shadow :300, render_gradient_fill :410,
// render_texture_fill :469; the region rule: data_impl.rs:132-194; find_tight_bounds_rgba: raster.rs:23-41.
// check_call refuses what include/pfx.h lists, before anything is reserved or launched; plan_job derives what is uniform over the image — the rounded
// offsets, the discs' row spans (the reference's f32 test, once per row), which planes the compose kernel will read and where they live in ctx->textfx_ws —
// and run_job launches it.  The blurs are the project's Gaussian in the effects' mode
// (pfx_effect_exact): the one-channel plane form where it applies (pfx_gauss_plane_applies: dword rows, radius within the fused kernel), else the RGBA image
// the reference builds, through pfx_gauss_blur, which keeps its f32 intermediate in st_tmp.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "pfx_internal.h"

namespace {

static_assert(PFX_TEXT_FX_MAX_RADIUS == PFXK_TEXTFX_MAX_RADIUS, "the header's cap is the disc kernel's largest halo");

inline int32_t f32_as_i32(float v)   // Rust's `v as i32`: truncates, saturates, NaN -> 0
{
    if (v != v) return 0;
    return v <= -2147483648.0f ? INT32_MIN : (v >= 2147483648.0f ? INT32_MAX : (int32_t)v);
}
inline float to_radians(float deg) { return deg * (3.14159265358979323846f / 180.0f); }   // f32::to_radians
inline uint32_t pack_rgb(const uint8_t c[4]) { return (uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16); }

// dilate_mask's disc :176-207 as row spans: int_radius = ceil(radius), r_sq rounded once, a row is in when dy * dy <= r_sq and then reaches the largest dx
// with dx * dx + dy_sq <= r_sq (both squares and their sum are small integers, exact in f32).  -1 = the row is skipped
int span_half(float radius, int int_radius, int dy)
{
    const float r_sq = radius * radius, dyf = (float)dy, dy_sq = dyf * dyf;
    if (dy_sq > r_sq) return -1;
    int half = 0;
    for (int dx = 1; dx <= int_radius; ++dx) {
        const float dxf = (float)dx;
        if (dxf * dxf + dy_sq <= r_sq) half = dx;
    }
    return half;
}
void build_disc(float radius, pfxk_disc* D)   // 0 < ceil(radius) <= PFXK_TEXTFX_MAX_RADIUS
{
    std::memset(D, 0, sizeof *D);
    D->radius = (int32_t)ceilf(radius);
    uint32_t top = 0;
    for (int dy = -D->radius; dy <= D->radius; ++dy) {
        const int half = span_half(radius, D->radius, dy);
        uint32_t& sp = D->span[dy + D->radius];
        if (half < 0) { sp = PFXK_DISC_SKIP; continue; }
        const uint32_t len = 2u * (uint32_t)half + 1u;
        uint32_t lvl = 0;
        while (lvl < 3u && (4u << (2u * lvl)) <= len) ++lvl;   // the largest window of 4^lvl columns that fits the span
        const uint32_t win = 1u << (2u * lvl);
        sp = (uint32_t)half | (lvl << 8) | (((len + win - 1u) / win) << 16);
        top = std::max(top, lvl);
    }
    D->levels = top + 1u;
}

struct job {   // what plan_job derives from a checked descriptor for a w x h image
    uint32_t w, h;
    bool shadow, shadow_spread, shadow_blur, shadow_plane;   // _plane: the blur runs on the alpha plane
    bool outline_out, outline_in;
    bool inner, inner_blur, inner_plane;
    bool texture;
    int32_t sdx, sdy, idx, idy;
    pfxk_disc spread_disc, outline_disc;
    size_t plane, off_sa, off_sb, off_dil, off_ero, off_ia, off_ib, off_x, off_y, off_z, bytes;   // offsets into the workspace; `plane` = a plane's slot
};

// the dilation radius must fit the disc kernel's tile
int radius_ok(pfx_ctx* ctx, const char* who, const char* what, float radius)
{
    if (radius > 0.0f && ceilf(radius) > (float)PFX_TEXT_FX_MAX_RADIUS)
        return pfx_fail(ctx, PFX_ERR_UNSUPPORTED, "%s: %s %g: a dilation radius above %d is not supported", who, what, (double)radius, PFX_TEXT_FX_MAX_RADIUS);
    return PFX_OK;
}
int blur_ok(pfx_ctx* ctx, const char* who, const char* what, float blur)
{
    const int radius = pfx_host_gaussian_radius(blur);
    if (blur > 0.5f && radius > pfxk_gauss_max_radius())
        return pfx_fail(ctx, PFX_ERR_UNSUPPORTED, "%s: %s %g: gaussian radius %d beyond the device tile limit %d", who, what, (double)blur, radius, pfxk_gauss_max_radius());
    return PFX_OK;
}
inline float outline_radius(const pfx_text_fx* fx) { return fx->outline_position == PFX_TEXT_OUTLINE_CENTER ? fx->outline_width * 0.5f : fx->outline_width; }

// the descriptor alone (ctx may be NULL: pfx_text_effects_plan): PFX_ERR_INVALID first, then PFX_ERR_UNSUPPORTED
int check_descriptor(pfx_ctx* ctx, const char* who, const pfx_text_fx* fx)
{
    if (!fx) return pfx_fail(ctx, PFX_ERR_INVALID, "%s: the descriptor is null", who);
    const float f[] = {fx->outline_width, fx->shadow_offset_x, fx->shadow_offset_y, fx->shadow_blur_radius, fx->shadow_spread, fx->inner_offset_x, fx->inner_offset_y,
                       fx->inner_blur_radius, fx->gradient_angle_degrees, fx->gradient_scale, fx->gradient_offset[0], fx->gradient_offset[1], fx->texture_scale,
                       fx->texture_offset[0], fx->texture_offset[1]};
    for (float v : f)
        if (!std::isfinite(v)) return pfx_fail(ctx, PFX_ERR_INVALID, "%s: a float of the descriptor is not finite", who);
    if (fx->outline_position < PFX_TEXT_OUTLINE_INSIDE || fx->outline_position > PFX_TEXT_OUTLINE_CENTER)
        return pfx_fail(ctx, PFX_ERR_INVALID, "%s: unknown outline position %d", who, fx->outline_position);
    if (!pfx_dims_ok(fx->width, fx->height)) return pfx_fail(ctx, PFX_ERR_INVALID, "%s: bad image size %ux%u (sides above 0, at most 256 Mpx)", who, fx->width, fx->height);
    if ((fx->flags & PFX_TEXT_FX_TEXTURE_FILL) && fx->tex_w && fx->tex_h && !pfx_dims_ok(fx->tex_w, fx->tex_h))
        return pfx_fail(ctx, PFX_ERR_INVALID, "%s: bad texture size %ux%u", who, fx->tex_w, fx->tex_h);
    return PFX_OK;
}
int check_supported(pfx_ctx* ctx, const char* who, const pfx_text_fx* fx)
{
    if (fx->flags & PFX_TEXT_FX_OUTLINE) PFX_TRY(radius_ok(ctx, who, "outline radius", outline_radius(fx)));
    if (fx->flags & PFX_TEXT_FX_SHADOW) {
        if (fx->shadow_spread > 0.5f) PFX_TRY(radius_ok(ctx, who, "shadow spread", fx->shadow_spread));
        PFX_TRY(blur_ok(ctx, who, "shadow blur", fx->shadow_blur_radius));
    }
    if (fx->flags & PFX_TEXT_FX_INNER_SHADOW) PFX_TRY(blur_ok(ctx, who, "inner shadow blur", fx->inner_blur_radius));
    return PFX_OK;
}
inline bool texture_used(const pfx_text_fx* fx) { return (fx->flags & PFX_TEXT_FX_TEXTURE_FILL) && fx->tex_w && fx->tex_h; }
inline size_t texture_bytes(const pfx_text_fx* fx) { return texture_used(fx) ? pfx_img_bytes(fx->tex_w, fx->tex_h) : 0; }

// the stages of a checked descriptor on a w x h image and their workspace
void plan_job(const pfx_ctx* ctx, const pfx_text_fx* fx, uint32_t w, uint32_t h, job* J)
{
    std::memset(J, 0, sizeof *J);
    J->w = w; J->h = h;
    const bool exact = pfx_effect_exact(ctx);
    if (fx->flags & PFX_TEXT_FX_SHADOW) {
        J->shadow = true;
        J->sdx = f32_as_i32(roundf(fx->shadow_offset_x));   // :229
        J->sdy = f32_as_i32(roundf(fx->shadow_offset_y));
        J->shadow_spread = fx->shadow_spread > 0.5f;        // :247
        if (J->shadow_spread) build_disc(fx->shadow_spread, &J->spread_disc);
        J->shadow_blur = fx->shadow_blur_radius > 0.5f;     // :252
        J->shadow_plane = J->shadow_blur && pfx_gauss_plane_applies(ctx, exact, w, h, pfx_host_gaussian_radius(fx->shadow_blur_radius));
    }
    if (fx->flags & PFX_TEXT_FX_OUTLINE) {
        const float radius = outline_radius(fx);
        if (radius > 0.0f) {   // :86, :130
            (fx->outline_position == PFX_TEXT_OUTLINE_INSIDE ? J->outline_in : J->outline_out) = true;
            build_disc(radius, &J->outline_disc);
        }
    }
    if (fx->flags & PFX_TEXT_FX_INNER_SHADOW) {
        J->inner = true;
        J->idx = f32_as_i32(roundf(fx->inner_offset_x));   // :313
        J->idy = f32_as_i32(roundf(fx->inner_offset_y));
        J->inner_blur = fx->inner_blur_radius > 0.5f;      // :335
        J->inner_plane = J->inner_blur && pfx_gauss_plane_applies(ctx, exact, w, h, pfx_host_gaussian_radius(fx->inner_blur_radius));
    }
    J->texture = texture_used(fx) && !(fx->flags & PFX_TEXT_FX_GRADIENT_FILL);
    const size_t n = (size_t)w * h;
    J->plane = pfx_align256(n);
    size_t at = 0;
    auto take = [&](bool wanted, size_t bytes) { const size_t o = at; if (wanted) at += bytes; return o; };
    J->off_sa = take(J->shadow, J->plane);
    J->off_sb = take(J->shadow_spread || J->shadow_plane, J->plane);
    J->off_dil = take(J->outline_out, J->plane);
    J->off_ero = take(J->outline_in, J->plane);
    J->off_ia = take(J->inner_blur, J->plane);
    J->off_ib = take(J->inner_plane, J->plane);
    const bool shadow_rgba = J->shadow_blur && !J->shadow_plane, inner_rgba = J->inner_blur && !J->inner_plane;
    J->off_x = take(shadow_rgba || inner_rgba, 4 * J->plane);   // the Gaussian's input, of either shadow in turn
    J->off_y = take(shadow_rgba, 4 * J->plane);                 // the blurred shadow
    J->off_z = take(inner_rgba, 4 * J->plane);                  // the blurred inner shadow
    J->bytes = at;
}

// apply_text_effects of a checked descriptor on J's image; ws: J->bytes of device memory.  text, texture and out are the caller's to check
int run_job(pfx_ctx* ctx, const pfx_text_fx* fx, const job* J, const uint8_t* text, const uint8_t* texture, uint8_t* out, uint8_t* ws)
{
    const uint32_t w = J->w, h = J->h;
    const size_t n = (size_t)w * h;
    const bool exact = pfx_effect_exact(ctx);
    pfxk_textfx P;
    std::memset(&P, 0, sizeof P);
    P.w = w; P.h = h;
    if (J->shadow) {
        uint8_t *a = ws + J->off_sa, *b = ws + J->off_sb, *cur = a;
        {
            pfx_timer t(ctx, "textfx_plane");
            PFX_HIP(ctx, pfxk_textfx_plane(ctx->stream, text, a, w, h, J->sdx, J->sdy, fx->shadow_color[3], 0));
        }
        if (J->shadow_spread) {
            pfx_timer t(ctx, "textfx_disc");
            PFX_HIP(ctx, pfxk_textfx_disc(ctx->stream, cur, 1, 0, b, w, h, &J->spread_disc, 0));
            cur = b;
        }
        P.flags |= PFXK_TFX_SHADOW;
        P.shadow_rgb = pack_rgb(fx->shadow_color);
        if (J->shadow_plane) {
            uint8_t* other = cur == a ? b : a;
            PFX_TRY(pfx_gauss_plane(ctx, cur, other, w, h, fx->shadow_blur_radius));
            cur = other;
        } else if (J->shadow_blur) {
            PFX_HIP(ctx, pfxk_textfx_expand(ctx->stream, cur, ws + J->off_x, n, P.shadow_rgb));
            PFX_TRY(pfx_gauss_blur(ctx, exact, ws + J->off_x, ws + J->off_y, w, h, fx->shadow_blur_radius, nullptr, 0));
            cur = ws + J->off_y;
            P.flags |= PFXK_TFX_SHADOW_RGBA;
        }
        P.shadow = cur;
    }
    if (J->outline_out || J->outline_in) {
        uint8_t* dst = ws + (J->outline_in ? J->off_ero : J->off_dil);
        pfx_timer t(ctx, "textfx_disc");
        PFX_HIP(ctx, pfxk_textfx_disc(ctx->stream, text, 4, 3, dst, w, h, &J->outline_disc, J->outline_in ? 1 : 0));
        (J->outline_in ? P.eroded : P.dilated) = dst;
        P.flags |= J->outline_in ? PFXK_TFX_OUTLINE_IN : PFXK_TFX_OUTLINE_OUT;
        P.outline_rgb = pack_rgb(fx->outline_color);
        P.outline_oa = (float)fx->outline_color[3] / 255.0f;   // :97
    }
    if (J->inner) {
        P.flags |= PFXK_TFX_INNER;
        P.inner_rgb = pack_rgb(fx->inner_color);
        P.inner_ia = (float)fx->inner_color[3];
        P.inner_dx = J->idx; P.inner_dy = J->idy;
        if (J->inner_blur) {
            uint8_t* a = ws + J->off_ia;
            {
                pfx_timer t(ctx, "textfx_plane");
                PFX_HIP(ctx, pfxk_textfx_plane(ctx->stream, text, a, w, h, J->idx, J->idy, fx->inner_color[3], 1));
            }
            P.flags |= PFXK_TFX_INNER_BLURRED;
            if (J->inner_plane) {
                PFX_TRY(pfx_gauss_plane(ctx, a, ws + J->off_ib, w, h, fx->inner_blur_radius));
                P.inner = ws + J->off_ib;
            } else {
                PFX_HIP(ctx, pfxk_textfx_expand(ctx->stream, a, ws + J->off_x, n, P.inner_rgb));
                PFX_TRY(pfx_gauss_blur(ctx, exact, ws + J->off_x, ws + J->off_z, w, h, fx->inner_blur_radius, nullptr, 0));
                P.inner = ws + J->off_z;
                P.flags |= PFXK_TFX_INNER_RGBA;
            }
        }
    }
    if (fx->flags & PFX_TEXT_FX_GRADIENT_FILL) {
        const float angle = to_radians(fx->gradient_angle_degrees);   // :420-425
        P.flags |= PFXK_TFX_GRADIENT | (fx->gradient_repeat ? PFXK_TFX_GRADIENT_REPEAT : 0);
        P.g_dir_x = cosf(angle); P.g_dir_y = sinf(angle);
        P.g_scale = fmaxf(fx->gradient_scale, 1.0f);
        P.g_off_x = fx->gradient_offset[0]; P.g_off_y = fx->gradient_offset[1];
        P.g_start = pfx_pack_rgba8(fx->gradient_start); P.g_end = pfx_pack_rgba8(fx->gradient_end);
    } else if (J->texture) {
        P.flags |= PFXK_TFX_TEXTURE;
        P.tex_w = fx->tex_w; P.tex_h = fx->tex_h;
        P.t_scale = fmaxf(fx->texture_scale, 0.01f);   // :500
        P.t_off_x = fx->texture_offset[0]; P.t_off_y = fx->texture_offset[1];
    }
    pfx_timer t(ctx, "textfx_compose");
    PFX_HIP(ctx, pfxk_textfx_compose(ctx->stream, text, texture, out, &P));
    return PFX_OK;
}

// the region rule on a checked descriptor; bounds inside the canvas
void plan_region(const pfx_text_fx* fx, const uint32_t bounds[4], pfx_text_region* out)
{
    std::memset(out, 0, sizeof *out);
    if (!bounds[2] || !bounds[3]) return;   // :156
    float pad = 0.0f;   // :134-149
    if (fx->flags & PFX_TEXT_FX_SHADOW) pad = fmaxf(pad, fabsf(fx->shadow_offset_x) + fabsf(fx->shadow_offset_y) + fx->shadow_blur_radius * 3.0f + fx->shadow_spread);
    if (fx->flags & PFX_TEXT_FX_OUTLINE) pad = fmaxf(pad, ceilf(fx->outline_width) + 2.0f);
    if (fx->flags & PFX_TEXT_FX_INNER_SHADOW) pad = fmaxf(pad, fabsf(fx->inner_offset_x) + fabsf(fx->inner_offset_y) + fx->inner_blur_radius * 3.0f);
    const uint32_t pad_px = std::max(pfx_f32_as_u32(ceilf(pad)), 4u);   // :150
    const int64_t bx = bounds[0], by = bounds[1], bw = bounds[2], bh = bounds[3], p = pad_px;
    const int64_t rx = std::max<int64_t>(bx - p, 0), ry = std::max<int64_t>(by - p, 0);   // :162-167
    const int64_t rx2 = std::min<int64_t>(bx + bw + p, fx->width), ry2 = std::min<int64_t>(by + bh + p, fx->height);
    out->x = (uint32_t)rx; out->y = (uint32_t)ry; out->w = (uint32_t)(rx2 - rx); out->h = (uint32_t)(ry2 - ry);
    out->pad_px = pad_px;
    out->full_canvas = (uint64_t)out->w * out->h * 2u >= (uint64_t)fx->width * fx->height;   // :170-172
}

int check_call(pfx_ctx* ctx, const char* who, bool dev, const pfx_text_fx* fx, const void* text, const void* texture, const void* out)
{
    if (!ctx) return PFX_ERR_INVALID;
    PFX_TRY(check_descriptor(ctx, who, fx));
    if (texture_used(fx) && !texture) return pfx_fail(ctx, PFX_ERR_INVALID, "%s: the texture flag is set and tex_w * tex_h is not zero, but the texture is null", who);
    const size_t img = pfx_img_bytes(fx->width, fx->height);
    PFX_TRY(pfx_check_args(ctx, who, dev, {{text, img, PFX_ARG_DWORD, dev ? "text_dev" : "text"},
                                           {texture, texture_bytes(fx), PFX_ARG_OPTIONAL | PFX_ARG_DWORD, dev ? "texture_dev" : "texture"},
                                           {out, img, PFX_ARG_OUT | PFX_ARG_DWORD, dev ? "out_dev" : "out"}}));
    return check_supported(ctx, who, fx);
}

} // namespace

extern "C" {

// test seam (not in include/pfx.h): the half-width of row dy of dilate_mask's disc as the kernels' span table holds it; -1 = the row is skipped, |dy| above
// ceil(radius), or a radius the module refuses
int pfx_int_textfx_span(float radius, int32_t dy)
{
    if (!(radius > 0.0f) || !std::isfinite(radius) || ceilf(radius) > (float)PFX_TEXT_FX_MAX_RADIUS) return -1;
    const int int_radius = (int)ceilf(radius);
    if (dy < -int_radius || dy > int_radius) return -1;
    return span_half(radius, int_radius, dy);
}

// test seam (not in include/pfx.h): the disc's maximum (take_min: minimum) of a tight w x h u8 plane into another, as the stages run it: build_disc, then one
// launch.  Refuses before anything is launched: PFX_ERR_INVALID for a radius that is not finite or not above 0, a bad size, a NULL or overlapping plane;
// PFX_ERR_UNSUPPORTED for ceil(radius) above PFX_TEXT_FX_MAX_RADIUS.  Asynchronous
int pfx_int_textfx_disc_dev(pfx_ctx* ctx, const void* src_plane, void* dst_plane, uint32_t w, uint32_t h, float radius, int take_min)
{
    const char* who = "pfx_int_textfx_disc_dev";
    PFX_TRY(pfx_check_dims(ctx, who, w, h));
    if (!std::isfinite(radius) || !(radius > 0.0f)) return pfx_fail(ctx, PFX_ERR_INVALID, "%s: radius %g is not finite and above 0", who, (double)radius);
    const size_t n = (size_t)w * h;
    PFX_TRY(pfx_check_args(ctx, who, true, {{src_plane, n, PFX_ARG_IN, "src_plane"}, {dst_plane, n, PFX_ARG_OUT, "dst_plane"}}));
    PFX_TRY(radius_ok(ctx, who, "radius", radius));
    pfxk_disc D;
    build_disc(radius, &D);
    pfx_timer t(ctx, "textfx_disc");
    PFX_HIP(ctx, pfxk_textfx_disc(ctx->stream, (const uint8_t*)src_plane, 1, 0, (uint8_t*)dst_plane, w, h, &D, take_min ? 1 : 0));
    return PFX_OK;
}

int pfx_text_effects_plan(const pfx_text_fx* fx, const uint32_t bounds[4], pfx_text_region* out)
{
    const char* who = "pfx_text_effects_plan";
    PFX_TRY(check_descriptor(nullptr, who, fx));
    if (!bounds || !out) return pfx_fail(nullptr, PFX_ERR_INVALID, "%s: bounds or out is null", who);
    if (bounds[2] && bounds[3] && !pfx_rect_inside(bounds[0], bounds[1], bounds[2], bounds[3], fx->width, fx->height))
        return pfx_fail(nullptr, PFX_ERR_INVALID, "%s: the bounds lie outside the canvas", who);
    plan_region(fx, bounds, out);
    return PFX_OK;
}

int pfx_text_effects_dev(pfx_ctx* ctx, const pfx_text_fx* fx, const void* text_dev, const void* texture_dev, void* out_dev)
{
    PFX_TRY(check_call(ctx, "pfx_text_effects_dev", true, fx, text_dev, texture_dev, out_dev));
    job J;
    plan_job(ctx, fx, fx->width, fx->height, &J);
    PFX_TRY(pfx_reserve(ctx, ctx->textfx_ws, J.bytes));
    return run_job(ctx, fx, &J, (const uint8_t*)text_dev, (const uint8_t*)texture_dev, (uint8_t*)out_dev, (uint8_t*)ctx->textfx_ws.p);
}

int pfx_text_effects(pfx_ctx* ctx, const pfx_text_fx* fx, const uint8_t* text, const uint8_t* texture, uint8_t* out)
{
    PFX_TRY(check_call(ctx, "pfx_text_effects", false, fx, text, texture, out));
    const size_t img = pfx_img_bytes(fx->width, fx->height);
    void *d_text, *d_out;
    const void* d_tex;
    PFX_TRY(pfx_stage(ctx, ctx->st_in, text, img, &d_text));
    PFX_TRY(pfx_stage_opt(ctx, ctx->st_mask, texture_used(fx) ? texture : nullptr, texture_bytes(fx), &d_tex));
    PFX_TRY(pfx_stage(ctx, ctx->st_out, nullptr, img, &d_out));
    PFX_TRY(pfx_text_effects_dev(ctx, fx, d_text, d_tex, d_out));
    return pfx_unstage(ctx, out, ctx->st_out, img);
}

int pfx_text_layer_effects_dev(pfx_ctx* ctx, const pfx_text_fx* fx, const void* text_dev, const void* texture_dev, void* out_dev, pfx_text_region* region_out)
{
    const char* who = "pfx_text_layer_effects_dev";
    PFX_TRY(check_call(ctx, who, true, fx, text_dev, texture_dev, out_dev));
    const uint32_t cw = fx->width, ch = fx->height;
    PFX_TRY(pfx_reserve(ctx, ctx->d_misc, 4096));
    uint32_t got[5] = {0, 0, 0, 0, 0};
    PFX_HIP(ctx, hipMemsetAsync(ctx->d_misc.p, 0, sizeof got, ctx->stream));
    {
        pfx_timer t(ctx, "textfx_bounds");
        PFX_HIP(ctx, pfxk_textfx_bounds(ctx->stream, (const uint8_t*)text_dev, cw, ch, (uint32_t*)ctx->d_misc.p));
    }
    PFX_TRY(pfx_d2h(ctx, got, ctx->d_misc.p, sizeof got));
    PFX_TRY(pfx_sync(ctx));
    pfx_text_region R;
    std::memset(&R, 0, sizeof R);
    if (got[4]) {
        const uint32_t min_x = ~got[0], min_y = ~got[1];
        if (got[2] >= cw || got[3] >= ch || min_x > got[2] || min_y > got[3]) return pfx_fail(ctx, PFX_ERR_HIP, "%s: the text's box came back outside the canvas", who);
        const uint32_t bounds[4] = {min_x, min_y, got[2] - min_x + 1u, got[3] - min_y + 1u};
        plan_region(fx, bounds, &R);
    }
    const size_t canvas = pfx_img_bytes(cw, ch);
    if (!R.w || !R.h) {   // no visible text :156
        PFX_HIP(ctx, hipMemsetAsync(out_dev, 0, canvas, ctx->stream));
        if (region_out) *region_out = R;
        return PFX_OK;
    }
    job J;
    if (R.full_canvas) {
        plan_job(ctx, fx, cw, ch, &J);
        PFX_TRY(pfx_reserve(ctx, ctx->textfx_ws, J.bytes));
        PFX_TRY(run_job(ctx, fx, &J, (const uint8_t*)text_dev, (const uint8_t*)texture_dev, (uint8_t*)out_dev, (uint8_t*)ctx->textfx_ws.p));
    } else {   // the cropped region in, its result blitted into a zero canvas :177-193
        plan_job(ctx, fx, R.w, R.h, &J);
        const size_t region = pfx_align256(pfx_img_bytes(R.w, R.h)), pitch = (size_t)R.w * 4, cpitch = (size_t)cw * 4;
        PFX_TRY(pfx_reserve(ctx, ctx->textfx_ws, 2 * region + J.bytes));
        uint8_t *r_in = (uint8_t*)ctx->textfx_ws.p, *r_out = r_in + region, *ws = r_out + region;
        const size_t corner = ((size_t)R.y * cw + R.x) * 4;
        {
            pfx_timer t(ctx, "textfx_crop");
            PFX_HIP(ctx, hipMemcpy2DAsync(r_in, pitch, (const uint8_t*)text_dev + corner, cpitch, pitch, R.h, hipMemcpyDeviceToDevice, ctx->stream));
        }
        PFX_TRY(run_job(ctx, fx, &J, r_in, (const uint8_t*)texture_dev, r_out, ws));
        pfx_timer t(ctx, "textfx_blit");
        PFX_HIP(ctx, hipMemsetAsync(out_dev, 0, canvas, ctx->stream));
        PFX_HIP(ctx, hipMemcpy2DAsync((uint8_t*)out_dev + corner, cpitch, r_out, pitch, pitch, R.h, hipMemcpyDeviceToDevice, ctx->stream));
    }
    if (region_out) *region_out = R;
    return PFX_OK;
}

} // extern "C"
