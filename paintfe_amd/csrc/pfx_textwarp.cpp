// pfx_textwarp.cpp — C ABI of the text block's warps, rotation and placement (k_textwarp.hip).  Reference: src/ops/text_layer/warp.rs — blit_rgba_buffer :39,
// apply_arc_warp :97, arc_map_point :182, arc_inverse_map :222, apply_circular_warp :277, apply_path_follow_warp :355, apply_envelope_warp :447, the Bézier
// helpers :546-704, bilinear_sample :707; raster.rs — the block's way into the layer :374-417, rotate_glyph_buffer :561-653; selection.rs —
// maybe_rotate_and_blit :77-106.
// check_desc refuses what include/pfx.h lists; plan_warp / plan_rotate run the reference's bounds loops in f32 as written (glibc sinf / cosf, f32::min / max
// as fminf / fmaxf, saturating casts) and derive what is uniform over the image — the arc's radius and gates, the path's 65 coarse points and 257 arc lengths,
// the envelope's t denominator — through the reference's own expressions; the kernels do the per-pixel part.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "pfx_internal.h"

namespace {

constexpr float PI_F = 3.14159265358979323846f, F32_MAX = 3.4028234663852886e38f;
constexpr uint64_t DOC_LIMIT = 256000000ull;

inline int32_t f32_as_i32(float v)   // Rust's `v as i32`: truncates, saturates, NaN -> 0
{
    if (v != v) return 0;
    return v <= -2147483648.0f ? INT32_MIN : (v >= 2147483648.0f ? INT32_MAX : (int32_t)v);
}
inline bool over_limit(uint32_t w, uint32_t h) { return (uint64_t)w * h > DOC_LIMIT; }

struct box {   // the bounds loops' running minima and maxima
    float min_x = F32_MAX, max_x = -F32_MAX, min_y = F32_MAX, max_y = -F32_MAX;
    void grow(float margin) { min_x -= margin; min_y -= margin; max_x += margin; max_y += margin; }
};

// eval_cubic_bezier :546-559 and its tangent :562-571, one coordinate (k = 0: x, 1: y)
inline float bezier(const float p[4][2], int k, float t)
{
    const float u = 1.0f - t, u2 = u * u, t2 = t * t;
    return u2 * u * p[0][k] + 3.0f * u2 * t * p[1][k] + 3.0f * u * t2 * p[2][k] + t2 * t * p[3][k];
}
inline float bezier_tangent(const float p[4][2], int k, float t)
{
    const float u = 1.0f - t;
    return 3.0f * u * u * (p[1][k] - p[0][k]) + 6.0f * u * t * (p[2][k] - p[1][k]) + 3.0f * t * t * (p[3][k] - p[2][k]);
}

// arc_length_to_t :594-623 on the 257-entry table
float arc_length_to_t(float s, const float* lengths, float total)
{
    if (s <= 0.0f) return 0.0f;
    if (s >= total) return 1.0f;
    const size_t n = 256;
    size_t lo = 0, hi = n;
    while (lo < hi) {
        const size_t mid = (lo + hi) / 2;
        if (lengths[mid] < s) lo = mid + 1; else hi = mid;
    }
    if (lo == 0) return 0.0f;
    const float seg_len = lengths[lo] - lengths[lo - 1];
    const float frac = seg_len > 0.0f ? (s - lengths[lo - 1]) / seg_len : 0.0f;
    return ((float)(lo - 1) + frac) / (float)n;
}

// arc_map_point :182-219
void arc_map_point(float sx, float sy, float w, float h, float radius, float angle, float hdist, float vdist, float* ox, float* oy)
{
    const float cx = w / 2.0f;
    const float t = (sx - cx) / (w / 2.0f);
    const float theta = t * angle / 2.0f;
    const float r_sign = angle > 0.0f ? 1.0f : -1.0f, r_abs = fabsf(radius);
    const float sy_norm = sy / h;
    const float r = r_abs - (1.0f - sy_norm) * h * r_sign;
    float dx = cx + r * sinf(theta);
    float dy = r_abs - r * cosf(theta) * r_sign;
    dx = dx + (dx - cx) * hdist;
    dy = dy + (dy - h / 2.0f) * vdist;
    *ox = dx; *oy = dy;
}

void identity_geom(const pfx_text_warp_desc* W, pfx_text_warp_geom* G)
{
    std::memset(G, 0, sizeof *G);
    G->out_w = W->src_w; G->out_h = W->src_h; G->identity = 1u;
}
void box_geom(const box& b, uint32_t out_w, uint32_t out_h, pfx_text_warp_geom* G)
{
    std::memset(G, 0, sizeof *G);
    G->out_w = out_w; G->out_h = out_h;
    G->off_x = f32_as_i32(floorf(b.min_x)); G->off_y = f32_as_i32(floorf(b.min_y));
    G->min_x = b.min_x; G->min_y = b.min_y; G->max_x = b.max_x; G->max_y = b.max_y;
}

// the plan of a checked descriptor; P and T (the kernels' uniforms) are filled for a plan that is not the identity
void plan_warp(const pfx_text_warp_desc* W, pfx_text_warp_geom* G, pfxk_textwarp* P, pfxk_textwarp_tables* T)
{
    std::memset(P, 0, sizeof *P);
    const float w = (float)W->src_w, h = (float)W->src_h;
    P->src_w = W->src_w; P->src_h = W->src_h; P->w = w; P->h = h;
    P->half_w = w / 2.0f; P->half_h = h / 2.0f;
    identity_geom(W, G);
    if (W->kind == PFX_TEXT_WARP_ARC) {
        if (fabsf(W->arc_bend) < 0.001f) return;                       // :103
        const float angle = W->arc_bend * PI_F;
        const bool curved = fabsf(angle) > 0.01f;
        const float radius = curved ? w / (2.0f * sinf(angle / 2.0f)) : w * 100.0f;
        box b;
        for (int i = 0; i <= 32; ++i) {                                // :125
            const float t = (float)i / 32.0f, sx = t * w;
            for (float sy : {0.0f, h}) {
                float dx, dy;
                arc_map_point(sx, sy, w, h, radius, angle, W->arc_hdist, W->arc_vdist, &dx, &dy);
                b.min_x = fminf(b.min_x, dx); b.max_x = fmaxf(b.max_x, dx);
                b.min_y = fminf(b.min_y, dy); b.max_y = fmaxf(b.max_y, dy);
            }
        }
        b.grow(2.0f);
        const uint32_t out_w = pfx_f32_as_u32(ceilf(b.max_x - b.min_x)), out_h = pfx_f32_as_u32(ceilf(b.max_y - b.min_y));
        if (out_w == 0 || out_h == 0 || out_w > 8192 || out_h > 8192) return;   // :145
        box_geom(b, out_w, out_h, G);
        P->cx = w / 2.0f; P->r_abs = fabsf(radius); P->r_sign = angle > 0.0f ? 1.0f : -1.0f;
        P->half_angle = angle / 2.0f; P->theta_lim = fabsf(angle / 2.0f) + 0.1f;
        P->h_r_sign = h * P->r_sign;
        P->one_hdist = 1.0f + W->arc_hdist; P->one_vdist = 1.0f + W->arc_vdist;
        P->curved = curved; P->undo_h = fabsf(W->arc_hdist) > 0.001f; P->undo_v = fabsf(W->arc_vdist) > 0.001f;
    } else if (W->kind == PFX_TEXT_WARP_CIRCULAR) {
        const float r = fmaxf(W->circ_radius, 10.0f), r_outer = r + h;   // :285
        const uint32_t out_size = pfx_f32_as_u32(ceilf(r_outer * 2.0f + 4.0f));
        const float out_c = (float)out_size / 2.0f;
        std::memset(G, 0, sizeof *G);
        G->out_w = G->out_h = out_size;
        G->off_x = f32_as_i32(roundf(w / 2.0f - out_c)); G->off_y = f32_as_i32(roundf(h / 2.0f - out_c));
        P->r = r; P->r_outer = r_outer; P->out_c = out_c; P->start_angle = W->circ_start_angle; P->dir = W->circ_clockwise ? 1.0f : -1.0f;
    } else if (W->kind == PFX_TEXT_WARP_PATH) {
        if (W->path_points < 4) return;                                // :361
        T->len[0] = 0.0f;                                              // build_arc_length_table :575-591
        float total = 0.0f, prev_x = bezier(W->path, 0, 0.0f), prev_y = bezier(W->path, 1, 0.0f);
        for (int i = 1; i <= 256; ++i) {
            const float t = (float)i / 256.0f, x = bezier(W->path, 0, t), y = bezier(W->path, 1, t);
            const float dx = x - prev_x, dy = y - prev_y;
            total += sqrtf(dx * dx + dy * dy);
            T->len[i] = total;
            prev_x = x; prev_y = y;
        }
        box b;
        for (int i = 0; i <= 64; ++i) {                                // :379
            const float s = ((float)i / 64.0f) * total;
            const float t = arc_length_to_t(s, T->len, total);
            const float px = bezier(W->path, 0, t), py = bezier(W->path, 1, t), ny = bezier_tangent(W->path, 1, t);
            for (float offset : {-h, 0.0f, h}) {
                b.min_x = fminf(b.min_x, px - fabsf(offset)); b.max_x = fmaxf(b.max_x, px + fabsf(offset));
                b.min_y = fminf(b.min_y, py + offset + fabsf(ny) * h); b.max_y = fmaxf(b.max_y, py - offset - fabsf(ny) * h);
            }
        }
        b.grow(h + 10.0f);
        const uint32_t out_w = std::min(pfx_f32_as_u32(ceilf(b.max_x - b.min_x)), 4096u), out_h = std::min(pfx_f32_as_u32(ceilf(b.max_y - b.min_y)), 4096u);
        if (out_w == 0 || out_h == 0) return;
        box_geom(b, out_w, out_h, G);
        for (int i = 0; i <= 64; ++i) { T->cx[i] = bezier(W->path, 0, (float)i / 64.0f); T->cy[i] = bezier(W->path, 1, (float)i / 64.0f); }   // :641-642
        std::memcpy(P->top, W->path, sizeof P->top);
    } else if (W->kind == PFX_TEXT_WARP_ENVELOPE) {
        if (W->top_points < 4 || W->bottom_points < 4) return;         // :453
        box b;
        for (int i = 0; i <= 64; ++i) {                                // :467
            const float t = (float)i / 64.0f;
            const float tx = bezier(W->top, 0, t), ty = bezier(W->top, 1, t), bx = bezier(W->bottom, 0, t), by = bezier(W->bottom, 1, t);
            b.min_x = fminf(fminf(b.min_x, tx), bx); b.max_x = fmaxf(fmaxf(b.max_x, tx), bx);
            b.min_y = fminf(fminf(b.min_y, ty), by); b.max_y = fmaxf(fmaxf(b.max_y, ty), by);
        }
        const float margin = 4.0f;
        b.grow(margin);
        const uint32_t out_w = std::min(pfx_f32_as_u32(ceilf(b.max_x - b.min_x)), 4096u), out_h = std::min(pfx_f32_as_u32(ceilf(b.max_y - b.min_y)), 4096u);
        if (out_w == 0 || out_h == 0) return;
        box_geom(b, out_w, out_h, G);
        std::memcpy(P->top, W->top, sizeof P->top);
        std::memcpy(P->bottom, W->bottom, sizeof P->bottom);
        P->t_den = fmaxf(b.max_x - b.min_x - 2.0f * margin, 1.0f);     // :504
    }
    P->out_w = G->out_w; P->out_h = G->out_h; P->min_x = G->min_x; P->min_y = G->min_y;
}

// rotate_glyph_buffer's bounds :568-600, :649-650.  false: new_w or new_h does not fit 32 bits
bool plan_rotate(uint32_t w, uint32_t h, float angle, const float* pivot, pfx_text_warp_geom* G, pfxk_textrotate* R)
{
    std::memset(G, 0, sizeof *G);
    std::memset(R, 0, sizeof *R);
    G->out_w = w; G->out_h = h;
    if (!(fabsf(angle) > 0.001f)) { G->identity = 1u; return true; }   // selection.rs:89
    const float cos_a = cosf(angle), sin_a = sinf(angle), fw = (float)w, fh = (float)h;
    const float cx = pivot ? pivot[0] : fw * 0.5f, cy = pivot ? pivot[1] : fh * 0.5f;
    const float corners[4][2] = {{0.0f, 0.0f}, {fw, 0.0f}, {0.0f, fh}, {fw, fh}};
    box b;
    for (const auto& c : corners) {
        const float dx = c[0] - cx, dy = c[1] - cy;
        const float rx = dx * cos_a - dy * sin_a + cx, ry = dx * sin_a + dy * cos_a + cy;
        b.min_x = fminf(b.min_x, rx); b.min_y = fminf(b.min_y, ry); b.max_x = fmaxf(b.max_x, rx); b.max_y = fmaxf(b.max_y, ry);
    }
    const uint32_t span_w = pfx_f32_as_u32(ceilf(b.max_x - b.min_x)), span_h = pfx_f32_as_u32(ceilf(b.max_y - b.min_y));
    if (span_w == 0xffffffffu || span_h == 0xffffffffu) return false;
    box_geom(b, span_w + 1u, span_h + 1u, G);
    R->w = w; R->h = h; R->new_w = G->out_w; R->new_h = G->out_h;
    R->cos_a = cos_a; R->sin_a = sin_a; R->cx = cx; R->cy = cy;
    R->new_cx = cx - floorf(b.min_x); R->new_cy = cy - floorf(b.min_y);
    return true;
}

// the descriptor alone (ctx may be NULL: pfx_text_warp_plan): PFX_ERR_INVALID first, then PFX_ERR_UNSUPPORTED
int check_desc(pfx_ctx* ctx, const char* who, const pfx_text_warp_desc* W)
{
    if (!W) return pfx_fail(ctx, PFX_ERR_INVALID, "%s: the descriptor is null", who);
    if (W->kind < PFX_TEXT_WARP_NONE || W->kind > PFX_TEXT_WARP_ENVELOPE) return pfx_fail(ctx, PFX_ERR_INVALID, "%s: unknown warp kind %d", who, W->kind);
    if (!W->src_w || !W->src_h) return pfx_fail(ctx, PFX_ERR_INVALID, "%s: bad source size %ux%u", who, W->src_w, W->src_h);
    bool finite = std::isfinite(W->arc_bend) && std::isfinite(W->arc_hdist) && std::isfinite(W->arc_vdist) && std::isfinite(W->circ_radius) &&
                  std::isfinite(W->circ_start_angle);
    for (int i = 0; i < 4; ++i)
        for (int k = 0; k < 2; ++k) finite = finite && std::isfinite(W->path[i][k]) && std::isfinite(W->top[i][k]) && std::isfinite(W->bottom[i][k]);
    if (!finite) return pfx_fail(ctx, PFX_ERR_INVALID, "%s: a float of the descriptor is not finite", who);
    if (over_limit(W->src_w, W->src_h)) return pfx_fail(ctx, PFX_ERR_UNSUPPORTED, "%s: a %ux%u source is over the 256 Mpx document limit", who, W->src_w, W->src_h);
    if (fabsf(W->circ_start_angle) > 8.0f * PI_F)
        return pfx_fail(ctx, PFX_ERR_UNSUPPORTED, "%s: start angle %g: beyond 8 pi the reference's normalisation loops do not end in reasonable time", who,
                        (double)W->circ_start_angle);
    return PFX_OK;
}
int check_planned(pfx_ctx* ctx, const char* who, const char* what, const pfx_text_warp_geom* G)
{
    if (!G->out_w || !G->out_h || over_limit(G->out_w, G->out_h))
        return pfx_fail(ctx, PFX_ERR_UNSUPPORTED, "%s: the %s output %ux%u is outside the 256 Mpx document limit", who, what, G->out_w, G->out_h);
    return PFX_OK;
}
int check_rotation(pfx_ctx* ctx, const char* who, uint32_t w, uint32_t h, float angle, const float* pivot)
{
    if (!w || !h) return pfx_fail(ctx, PFX_ERR_INVALID, "%s: bad image size %ux%u", who, w, h);
    if (!std::isfinite(angle) || (pivot && (!std::isfinite(pivot[0]) || !std::isfinite(pivot[1])))) return pfx_fail(ctx, PFX_ERR_INVALID, "%s: the angle or the pivot is not finite", who);
    if (over_limit(w, h)) return pfx_fail(ctx, PFX_ERR_UNSUPPORTED, "%s: a %ux%u image is over the 256 Mpx document limit", who, w, h);
    return PFX_OK;
}

// the warp of a planned descriptor that is not the identity
int run_warp(pfx_ctx* ctx, const pfx_text_warp_desc* W, const pfxk_textwarp* P, const pfxk_textwarp_tables* T, const uint8_t* src, uint8_t* out)
{
    switch (W->kind) {
    case PFX_TEXT_WARP_ARC: { pfx_timer t(ctx, "textwarp_arc"); PFX_HIP(ctx, pfxk_textwarp_arc(ctx->stream, src, out, P)); break; }
    case PFX_TEXT_WARP_CIRCULAR: { pfx_timer t(ctx, "textwarp_circular"); PFX_HIP(ctx, pfxk_textwarp_circular(ctx->stream, src, out, P)); break; }
    case PFX_TEXT_WARP_PATH: { pfx_timer t(ctx, "textwarp_path"); PFX_HIP(ctx, pfxk_textwarp_path(ctx->stream, src, out, P, T)); break; }
    default: { pfx_timer t(ctx, "textwarp_envelope"); PFX_HIP(ctx, pfxk_textwarp_envelope(ctx->stream, src, out, P)); break; }
    }
    return PFX_OK;
}

} // namespace

extern "C" {

int pfx_text_warp_plan(const pfx_text_warp_desc* warp, pfx_text_warp_geom* out)
{
    const char* who = "pfx_text_warp_plan";
    PFX_TRY(check_desc(nullptr, who, warp));
    if (!out) return pfx_fail(nullptr, PFX_ERR_INVALID, "%s: out is null", who);
    pfx_text_warp_geom G;
    pfxk_textwarp P;
    pfxk_textwarp_tables T;
    plan_warp(warp, &G, &P, &T);
    PFX_TRY(check_planned(nullptr, who, "planned", &G));
    *out = G;
    return PFX_OK;
}

int pfx_text_warp_dev(pfx_ctx* ctx, const pfx_text_warp_desc* warp, const void* src_dev, void* out_dev)
{
    const char* who = "pfx_text_warp_dev";
    if (!ctx) return PFX_ERR_INVALID;
    PFX_TRY(check_desc(ctx, who, warp));
    pfx_text_warp_geom G;
    pfxk_textwarp P;
    pfxk_textwarp_tables T;
    plan_warp(warp, &G, &P, &T);
    PFX_TRY(check_planned(ctx, who, "planned", &G));
    const size_t in_bytes = pfx_img_bytes(warp->src_w, warp->src_h), out_bytes = pfx_img_bytes(G.out_w, G.out_h);
    PFX_TRY(pfx_check_args(ctx, who, true, {{src_dev, in_bytes, PFX_ARG_DWORD, "src_dev"}, {out_dev, out_bytes, PFX_ARG_OUT | PFX_ARG_DWORD, "out_dev"}}));
    if (G.identity) {
        pfx_timer t(ctx, "textwarp_copy");
        PFX_HIP(ctx, hipMemcpyAsync(out_dev, src_dev, in_bytes, hipMemcpyDeviceToDevice, ctx->stream));
        return PFX_OK;
    }
    return run_warp(ctx, warp, &P, &T, (const uint8_t*)src_dev, (uint8_t*)out_dev);
}

int pfx_text_warp(pfx_ctx* ctx, const pfx_text_warp_desc* warp, const uint8_t* src, uint8_t* out, size_t out_bytes, pfx_text_warp_geom* plan_out)
{
    const char* who = "pfx_text_warp";
    if (!ctx) return PFX_ERR_INVALID;
    PFX_TRY(check_desc(ctx, who, warp));
    pfx_text_warp_geom G;
    pfxk_textwarp P;
    pfxk_textwarp_tables T;
    plan_warp(warp, &G, &P, &T);
    PFX_TRY(check_planned(ctx, who, "planned", &G));
    const size_t in_bytes = pfx_img_bytes(warp->src_w, warp->src_h), need = pfx_img_bytes(G.out_w, G.out_h);
    PFX_TRY(pfx_check_args(ctx, who, false, {{src, in_bytes, PFX_ARG_IN, "src"}, {out, need, PFX_ARG_OUT, "out"}}));
    if (out_bytes < need) return pfx_fail(ctx, PFX_ERR_INVALID, "%s: out_bytes %zu is below the %zu of the planned %ux%u output", who, out_bytes, need, G.out_w, G.out_h);
    void *d_src, *d_out;
    PFX_TRY(pfx_stage(ctx, ctx->st_in, src, in_bytes, &d_src));
    PFX_TRY(pfx_stage(ctx, ctx->st_out, nullptr, need, &d_out));
    PFX_TRY(pfx_text_warp_dev(ctx, warp, d_src, d_out));
    PFX_TRY(pfx_unstage(ctx, out, ctx->st_out, need));
    if (plan_out) *plan_out = G;
    return PFX_OK;
}

int pfx_text_rotate_plan(uint32_t w, uint32_t h, float angle, const float* pivot_xy, pfx_text_warp_geom* out)
{
    const char* who = "pfx_text_rotate_plan";
    PFX_TRY(check_rotation(nullptr, who, w, h, angle, pivot_xy));
    if (!out) return pfx_fail(nullptr, PFX_ERR_INVALID, "%s: out is null", who);
    pfx_text_warp_geom G;
    pfxk_textrotate R;
    if (!plan_rotate(w, h, angle, pivot_xy, &G, &R)) return pfx_fail(nullptr, PFX_ERR_UNSUPPORTED, "%s: the rotated bounds do not fit 32 bits", who);
    PFX_TRY(check_planned(nullptr, who, "rotated", &G));
    *out = G;
    return PFX_OK;
}

int pfx_text_rotate_dev(pfx_ctx* ctx, uint32_t w, uint32_t h, float angle, const float* pivot_xy, const void* src_dev, void* out_dev)
{
    const char* who = "pfx_text_rotate_dev";
    if (!ctx) return PFX_ERR_INVALID;
    PFX_TRY(check_rotation(ctx, who, w, h, angle, pivot_xy));
    pfx_text_warp_geom G;
    pfxk_textrotate R;
    if (!plan_rotate(w, h, angle, pivot_xy, &G, &R)) return pfx_fail(ctx, PFX_ERR_UNSUPPORTED, "%s: the rotated bounds do not fit 32 bits", who);
    PFX_TRY(check_planned(ctx, who, "rotated", &G));
    const size_t in_bytes = pfx_img_bytes(w, h);
    PFX_TRY(pfx_check_args(ctx, who, true, {{src_dev, in_bytes, PFX_ARG_DWORD, "src_dev"}, {out_dev, pfx_img_bytes(G.out_w, G.out_h), PFX_ARG_OUT | PFX_ARG_DWORD, "out_dev"}}));
    if (G.identity) {
        pfx_timer t(ctx, "textwarp_copy");
        PFX_HIP(ctx, hipMemcpyAsync(out_dev, src_dev, in_bytes, hipMemcpyDeviceToDevice, ctx->stream));
        return PFX_OK;
    }
    pfx_timer t(ctx, "textwarp_rotate");
    PFX_HIP(ctx, pfxk_textwarp_rotate(ctx->stream, (const uint8_t*)src_dev, (uint8_t*)out_dev, &R));
    return PFX_OK;
}

int pfx_text_block_place_dev(pfx_ctx* ctx, const pfx_text_block* block, const void* src_dev, void* canvas_dev)
{
    const char* who = "pfx_text_block_place_dev";
    if (!ctx) return PFX_ERR_INVALID;
    if (!block) return pfx_fail(ctx, PFX_ERR_INVALID, "%s: the block is null", who);
    const pfx_text_warp_desc* W = &block->warp;
    if (!W->src_w || !W->src_h || !block->canvas_w || !block->canvas_h)
        return pfx_fail(ctx, PFX_ERR_INVALID, "%s: bad size: raster %ux%u, canvas %ux%u", who, W->src_w, W->src_h, block->canvas_w, block->canvas_h);
    if (!std::isfinite(block->rotation) || !std::isfinite(block->pivot[0]) || !std::isfinite(block->pivot[1]))
        return pfx_fail(ctx, PFX_ERR_INVALID, "%s: the rotation or the pivot is not finite", who);
    PFX_TRY(check_desc(ctx, who, W));
    if (over_limit(block->canvas_w, block->canvas_h))
        return pfx_fail(ctx, PFX_ERR_UNSUPPORTED, "%s: a %ux%u canvas is over the 256 Mpx document limit", who, block->canvas_w, block->canvas_h);
    // everything is planned before the first launch: the warp (raster.rs:389), then the rotation around the pivot seen from the warped buffer (selection.rs:90)
    pfx_text_warp_geom G, RG;
    pfxk_textwarp P;
    pfxk_textwarp_tables T;
    pfxk_textrotate R;
    plan_warp(W, &G, &P, &T);
    PFX_TRY(check_planned(ctx, who, "warped", &G));
    int64_t off_x = (int64_t)block->off_x + G.off_x, off_y = (int64_t)block->off_y + G.off_y;
    const float local_pivot[2] = {block->pivot[0] - (float)off_x, block->pivot[1] - (float)off_y};
    if (!plan_rotate(G.out_w, G.out_h, block->rotation, block->has_pivot ? local_pivot : nullptr, &RG, &R))
        return pfx_fail(ctx, PFX_ERR_UNSUPPORTED, "%s: the rotated bounds do not fit 32 bits", who);
    PFX_TRY(check_planned(ctx, who, "rotated", &RG));
    PFX_TRY(pfx_check_args(ctx, who, true, {{src_dev, pfx_img_bytes(W->src_w, W->src_h), PFX_ARG_DWORD, "src_dev"},
                                            {canvas_dev, pfx_img_bytes(block->canvas_w, block->canvas_h), PFX_ARG_OUT | PFX_ARG_DWORD, "canvas_dev"}}));
    const size_t warped = G.identity ? 0 : pfx_align256(pfx_img_bytes(G.out_w, G.out_h)), rotated = RG.identity ? 0 : pfx_align256(pfx_img_bytes(RG.out_w, RG.out_h));
    if (warped + rotated) PFX_TRY(pfx_reserve(ctx, ctx->textwarp_ws, warped + rotated));
    const uint8_t* cur = (const uint8_t*)src_dev;
    uint32_t cur_w = W->src_w, cur_h = W->src_h;
    if (!G.identity) {
        uint8_t* dst = (uint8_t*)ctx->textwarp_ws.p;
        PFX_TRY(run_warp(ctx, W, &P, &T, cur, dst));
        cur = dst; cur_w = G.out_w; cur_h = G.out_h;
    }
    if (!RG.identity) {
        uint8_t* dst = (uint8_t*)ctx->textwarp_ws.p + warped;
        pfx_timer t(ctx, "textwarp_rotate");
        PFX_HIP(ctx, pfxk_textwarp_rotate(ctx->stream, cur, dst, &R));
        cur = dst; cur_w = RG.out_w; cur_h = RG.out_h;
        off_x += RG.off_x; off_y += RG.off_y;
    }
    pfx_timer t(ctx, "textwarp_blit");
    PFX_HIP(ctx, pfxk_textwarp_blit(ctx->stream, cur, cur_w, cur_h, off_x, off_y, (uint8_t*)canvas_dev, block->canvas_w, block->canvas_h));
    return PFX_OK;
}

} // extern "C"
