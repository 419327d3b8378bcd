// pfx_linetool.cpp — C ABI of the line / curve tool (k_linetool.hip): bounds, the dot list and the arrowheads on the host, the render onto a device-resident
// preview, and the mask-target release.
// Reference: src/ui/panels/tools/behavior/raster/bezier_math.rs — bezier_point :27, get_bezier_bounds :41, rasterize_bezier :76, draw_filled_triangle :289,
// draw_bezier_circle_with_hardness :456; compute_line_alpha, brush_render.rs:85; commit_preview_to_layer_mask, bezier_commit.rs:229; TiledImage::clear_region,
// src/canvas/tiled_image.rs:954.
// The host prologue does what the reference does once per call or once per primitive, with its float operations in its order: the step count, the curve
// samples with their running length, the canvas test, the pattern, the cap rule, every dot's pixel box, the triangles' vertices, boxes, edges and winding, the
// chunks to clear.  It then deals the dots to the 64 x 64 chunks their boxes touch, as pfx_dabtools.cpp does.  The selection lives on the device: the dot's
// selection gate is the kernel's.
// Vec2::length is emath's and its source was not at hand: it is taken to be x.hypot(y) — from recollection, unverified — and restated ONCE, in vec2_length
// below.  It enters the step count and a pattern's on / off phase only, never a pixel's arithmetic.
// Every entry point checks its sizes, then its descriptor and buffers, and only then uploads and launches.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <vector>

#include "pfx_internal.h"

namespace {

constexpr uint64_t MAX_ENTRIES = 8ull << 20;   // chunk-list entries of one launch, pfx_dabtools.cpp's bound; a longer curve goes in consecutive pieces
std::atomic<uint64_t> g_piece_entries{MAX_ENTRIES};   // pfx_int_line_piece_entries
constexpr uint32_t MIN_STEPS = 20u, MAX_STEPS = 5000u;   // :143

inline float vec2_length(float x, float y) { return hypotf(x, y); }   // emath 0.35 Vec2::length, see the header

struct pt { float x, y; };

pt bezier_point(const pt p[4], float t)   // :27-38
{
    const float t2 = t * t, t3 = t2 * t, mt = 1.0f - t, mt2 = mt * mt, mt3 = mt2 * mt;
    return {mt3 * p[0].x + 3.0f * mt2 * t * p[1].x + 3.0f * mt * t2 * p[2].x + t3 * p[3].x,
            mt3 * p[0].y + 3.0f * mt2 * t * p[1].y + 3.0f * mt * t2 * p[2].y + t3 * p[3].y};
}

bool tool_ok(const pfx_line_tool* tool)
{
    if (!tool) return false;
    for (float v : tool->p)
        if (!std::isfinite(v)) return false;
    if (!std::isfinite(tool->size)) return false;   // the clone stamp's range: any finite size
    return tool->pattern >= 0 && tool->pattern <= 2 && tool->cap_style >= 0 && tool->cap_style <= 1 && tool->end_shape >= 0 && tool->end_shape <= 1 &&
           tool->arrow_side >= 0 && tool->arrow_side <= 2;
}

void line_bounds(const pfx_line_tool& T, uint32_t w, uint32_t h, float out[4])   // :41-73
{
    float min_x = T.p[0], max_x = T.p[0], min_y = T.p[1], max_y = T.p[1];
    for (int k = 1; k < 4; ++k) {
        min_x = fminf(min_x, T.p[2 * k]); max_x = fmaxf(max_x, T.p[2 * k]);
        min_y = fminf(min_y, T.p[2 * k + 1]); max_y = fmaxf(max_y, T.p[2 * k + 1]);
    }
    const float arrow_extra = T.end_shape == 1 ? fmaxf(T.size * 3.0f, 8.0f) + fmaxf(T.size * 1.5f, 4.0f) : 0.0f;
    const float padding = T.size / 2.0f + 2.0f + arrow_extra;
    out[0] = fmaxf(min_x - padding, 0.0f); out[1] = fmaxf(min_y - padding, 0.0f);
    out[2] = fminf(max_x + padding, (float)w); out[3] = fminf(max_y + padding, (float)h);
}

// the dots of :131-210 before the selection test, in order: emit(fx, fy)
template <class Emit>
void walk_dots(const pfx_line_tool& T, uint32_t w, uint32_t h, Emit emit)
{
    const pt p[4] = {{T.p[0], T.p[1]}, {T.p[2], T.p[3]}, {T.p[4], T.p[5]}, {T.p[6], T.p[7]}};
    const float spacing = fmaxf(T.size * 0.1f, 0.5f);
    const float chord_len = vec2_length(p[3].x - p[0].x, p[3].y - p[0].y);
    const float control_net_len = vec2_length(p[1].x - p[0].x, p[1].y - p[0].y) + vec2_length(p[2].x - p[1].x, p[2].y - p[1].y) + vec2_length(p[3].x - p[2].x, p[3].y - p[2].y);
    const float total_length = control_net_len + chord_len;
    const float steps_f = ceilf(total_length / spacing);   // `as usize` saturates and sends NaN to 0, then .clamp(20, 5000)
    const uint32_t steps = !(steps_f > (float)MIN_STEPS) ? MIN_STEPS : (steps_f >= (float)MAX_STEPS ? MAX_STEPS : (uint32_t)steps_f);
    const float on_length = T.pattern == 1 ? T.size * 0.5f : (T.pattern == 2 ? T.size * 2.0f : 0.0f);
    const float off_length = T.pattern == 0 ? 0.0f : T.size * 1.5f;
    const float pattern_cycle = on_length + off_length;
    float cumulative_distance = 0.0f;
    pt prev = {0.0f, 0.0f};
    for (uint32_t i = 0; i <= steps; ++i) {
        const float t = (float)i / (float)steps;
        const pt pos = bezier_point(p, t);
        if (i) cumulative_distance += vec2_length(pos.x - prev.x, pos.y - prev.y);   // over ALL samples
        prev = pos;
        if (!(pos.x >= 0.0f && pos.y >= 0.0f && pfx_f32_as_u32(pos.x) < w && pfx_f32_as_u32(pos.y) < h)) continue;
        if (T.pattern != 0 && !(fmodf(cumulative_distance, pattern_cycle) < on_length)) continue;   // Rust's `%` on f32; a NaN compares false
        if (T.cap_style == 1 && (i == 0 || i == steps)) continue;                                   // :204
        emit(pos.x, pos.y);
    }
}

// the arrowheads in draw order, End then Start (:212-284): out = tip, wing1, wing2 per triangle; returns how many
uint32_t arrow_triangles(const pfx_line_tool& T, float out[12])
{
    if (T.end_shape != 1) return 0u;
    const float arrow_length = fmaxf(T.size * 3.0f, 8.0f), arrow_half_width = fmaxf(T.size * 1.5f, 4.0f);
    const float tip_advance = T.size + T.size / 2.0f;
    uint32_t n = 0;
    auto head = [&](float ox, float oy, float fx, float fy, float dir) {   // origin, the other point of the tangent, +1 End / -1 Start
        const float tx = 3.0f * (dir > 0.0f ? ox - fx : fx - ox), ty = 3.0f * (dir > 0.0f ? oy - fy : fy - oy);
        const float len = fmaxf(sqrtf(tx * tx + ty * ty), 0.001f);
        const float dx = tx / len, dy = ty / len;
        float tipx, tipy, bx, by;
        if (dir > 0.0f) { tipx = ox + dx * tip_advance; tipy = oy + dy * tip_advance; bx = tipx - dx * arrow_length; by = tipy - dy * arrow_length; }
        else { tipx = ox - dx * tip_advance; tipy = oy - dy * tip_advance; bx = tipx + dx * arrow_length; by = tipy + dy * arrow_length; }
        const float px = -dy, py = dx;
        float* o = out + 6u * n++;
        o[0] = tipx; o[1] = tipy;
        o[2] = bx + px * arrow_half_width; o[3] = by + py * arrow_half_width;
        o[4] = bx - px * arrow_half_width; o[5] = by - py * arrow_half_width;
    };
    if (T.arrow_side == 0 || T.arrow_side == 2) head(T.p[6], T.p[7], T.p[4], T.p[5], 1.0f);    // B'(1) = 3 (P3 - P2)
    if (T.arrow_side == 1 || T.arrow_side == 2) head(T.p[0], T.p[1], T.p[2], T.p[3], -1.0f);   // B'(0) = 3 (P1 - P0), pointing backward
    return n;
}

// draw_filled_triangle's prologue :304-328
void triangle_setup(const float v[6], uint32_t w, uint32_t h, pfxk_line_tri* R)
{
    for (int k = 0; k < 3; ++k) { R->vx[k] = v[2 * k]; R->vy[k] = v[2 * k + 1]; }
    R->x0 = pfx_f32_as_u32(fmaxf(floorf(fminf(fminf(R->vx[0], R->vx[1]), R->vx[2]) - 1.0f), 0.0f));
    R->x1 = std::min(pfx_f32_as_u32(ceilf(fmaxf(fmaxf(R->vx[0], R->vx[1]), R->vx[2]) + 1.0f)), w - 1u);
    R->y0 = pfx_f32_as_u32(fmaxf(floorf(fminf(fminf(R->vy[0], R->vy[1]), R->vy[2]) - 1.0f), 0.0f));
    R->y1 = std::min(pfx_f32_as_u32(ceilf(fmaxf(fmaxf(R->vy[0], R->vy[1]), R->vy[2]) + 1.0f)), h - 1u);
    if (R->x0 > R->x1 || R->y0 > R->y1) { R->x0 = R->y0 = 1u; R->x1 = R->y1 = 0u; }   // the reference's empty loop ranges
    for (int k = 0; k < 3; ++k) {
        const int n = (k + 1) % 3;
        R->ex[k] = R->vx[n] - R->vx[k]; R->ey[k] = R->vy[n] - R->vy[k];
        R->len[k] = fmaxf(sqrtf(R->ex[k] * R->ex[k] + R->ey[k] * R->ey[k]), 0.001f);
    }
    const float cross = R->ex[0] * (R->vy[2] - R->vy[0]) - R->ey[0] * (R->vx[2] - R->vx[0]);
    R->sign = cross >= 0.0f ? 1.0f : -1.0f;
}

void line_params(const pfx_line_tool& T, uint32_t w, uint32_t h, pfxk_line* L, float* outer_radius)
{
    std::memset(L, 0, sizeof *L);
    const float radius = T.size / 2.0f, soft = 1.0f - 0.95f;   // forced_hardness 0.95 = its own clamp(0.0, 0.99)
    L->radius = radius;
    L->anti_alias = T.anti_alias != 0;
    if (radius < 1.5f) { L->eff_radius = radius + 1.0f; L->fade_width = 1.0f; }                       // brush_render.rs:103-116
    else if (radius < 3.0f) { L->eff_radius = radius + 1.5f; L->fade_width = 1.5f + radius * soft; }
    else { L->eff_radius = radius; L->fade_width = fmaxf(radius * soft, 2.0f); }
    L->solid_radius = L->eff_radius - L->fade_width;
    const float aa_pad = L->anti_alias ? (radius < 1.5f ? 1.5f : fmaxf(radius * soft, 2.0f) + 2.0f) : 1.0f;   // :471-479
    *outer_radius = radius + aa_pad;
    L->src_a = (float)T.color[3] / 255.0f;
    for (int k = 0; k < 3; ++k) L->rgb |= std::min(pfx_f32_as_u32(((float)T.color[k] / 255.0f) * 255.0f), 255u) << (8 * k);   // `as u8`, which need not give c back
    float tri[12];
    L->n_tris = arrow_triangles(T, tri);
    for (uint32_t k = 0; k < L->n_tris; ++k) triangle_setup(tri + 6u * k, w, h, &L->tri[k]);
}

int check_tool(pfx_ctx* ctx, const char* who, const pfx_line_tool* tool, const float last_bounds[4])
{
    if (!tool) return pfx_fail(ctx, PFX_ERR_INVALID, "%s: tool is null", who);
    if (!tool_ok(tool)) return pfx_fail(ctx, PFX_ERR_INVALID, "%s: a control point or the size is not finite, or an enum is out of range", who);
    for (int k = 0; last_bounds && k < 4; ++k)
        if (!std::isfinite(last_bounds[k])) return pfx_fail(ctx, PFX_ERR_INVALID, "%s: last_bounds[%d] is not finite", who, k);
    return PFX_OK;
}

int check_render_bufs(pfx_ctx* ctx, const char* who, bool dev, void* preview, const void* sel, uint32_t w, uint32_t h)
{
    return pfx_check_args(ctx, who, dev, {{preview, pfx_img_bytes(w, h), PFX_ARG_OUT | (dev ? PFX_ARG_DWORD : 0), dev ? "preview_dev" : "preview_inout"},
                                          {sel, (size_t)w * h, PFX_ARG_OPTIONAL, dev ? "sel_dev" : "sel"}});
}

// everything is checked
int line_render_dev(pfx_ctx* ctx, const pfx_line_tool& T, void* preview_dev, const void* sel_dev, uint32_t w, uint32_t h, const float last_bounds[4], float bounds_out[4])
{
    pfxk_line L;
    float outer;
    line_params(T, w, h, &L, &outer);
    if (bounds_out) line_bounds(T, w, h, bounds_out);
    std::vector<pfxk_line_dot> dots;
    const uint32_t wm1 = w - 1u, hm1 = h - 1u;
    walk_dots(T, w, h, [&](float fx, float fy) {   // :482-485
        pfxk_line_dot D;
        D.cx = fx; D.cy = fy; D.cell_x = pfx_f32_as_u32(fx); D.cell_y = pfx_f32_as_u32(fy);
        D.x0 = pfx_f32_as_u32(fmaxf(fx - outer, 0.0f)); D.x1 = std::min(pfx_f32_as_u32(ceilf(fx + outer)), wm1);
        D.y0 = pfx_f32_as_u32(fmaxf(fy - outer, 0.0f)); D.y1 = std::min(pfx_f32_as_u32(ceilf(fy + outer)), hm1);
        if (D.x0 > D.x1 || D.y0 > D.y1) { D.x0 = D.y0 = 1u; D.x1 = D.y1 = 0u; }
        dots.push_back(D);
    });
    const uint32_t ncx = (w + 63u) / 64u, ncy = (h + 63u) / 64u, n_dots = (uint32_t)dots.size();
    // :117-129 and clear_region: chunk granular
    uint32_t ccx0 = 0, ccx1 = 0, ccy0 = 0, ccy1 = 0;
    if (last_bounds) {
        const uint32_t min_x = pfx_f32_as_u32(fmaxf(floorf(last_bounds[0]), 0.0f)), max_x = pfx_f32_as_u32(fminf(ceilf(last_bounds[2]), (float)w));
        const uint32_t min_y = pfx_f32_as_u32(fmaxf(floorf(last_bounds[1]), 0.0f)), max_y = pfx_f32_as_u32(fminf(ceilf(last_bounds[3]), (float)h));
        ccx0 = min_x / 64u; ccx1 = std::min((max_x + 63u) / 64u, ncx);
        ccy0 = min_y / 64u; ccy1 = std::min((max_y + 63u) / 64u, ncy);
    } else {
        PFX_HIP(ctx, hipMemsetAsync(preview_dev, 0, pfx_img_bytes(w, h), ctx->stream));   // preview.clear(): the first frame
    }
    const size_t dot_bytes = dots.size() * sizeof(pfxk_line_dot);
    bool uploaded = false;
    const uint64_t max_entries = g_piece_entries.load(std::memory_order_relaxed);
    std::vector<uint32_t> count((size_t)ncx * ncy), first((size_t)ncx * ncy), chunk_tab, bins;
    std::vector<uint8_t> flags((size_t)ncx * ncy);
    for (uint32_t lo = 0;;) {
        // the piece [lo, hi): as many dots as stay within max_entries chunk-list entries, and at least one; the clear rides with the first piece, the
        // arrowheads with the last (after all dots, as in the reference; the maximum does not care)
        uint64_t entries = 0;
        uint32_t hi = lo;
        std::fill(count.begin(), count.end(), 0u);
        std::fill(flags.begin(), flags.end(), (uint8_t)0);
        for (; hi < n_dots; ++hi) {
            const pfxk_line_dot& D = dots[hi];
            if (D.x0 > D.x1) continue;
            const uint64_t e = (uint64_t)((D.x1 >> 6) - (D.x0 >> 6) + 1u) * ((D.y1 >> 6) - (D.y0 >> 6) + 1u);
            if (entries + e > max_entries && hi > lo) break;
            entries += e;
            for (uint32_t cy = D.y0 >> 6; cy <= D.y1 >> 6; ++cy)
                for (uint32_t cx = D.x0 >> 6; cx <= D.x1 >> 6; ++cx) ++count[(size_t)cy * ncx + cx];
        }
        if (lo == 0)
            for (uint32_t cy = ccy0; cy < ccy1; ++cy)
                for (uint32_t cx = ccx0; cx < ccx1; ++cx) flags[(size_t)cy * ncx + cx] |= PFXK_LINE_CLEAR;
        if (hi == n_dots)
            for (uint32_t k = 0; k < L.n_tris; ++k) {
                const pfxk_line_tri& R = L.tri[k];
                if (R.x0 > R.x1) continue;
                for (uint32_t cy = R.y0 >> 6; cy <= R.y1 >> 6; ++cy)
                    for (uint32_t cx = R.x0 >> 6; cx <= R.x1 >> 6; ++cx) flags[(size_t)cy * ncx + cx] |= (uint8_t)(PFXK_LINE_TRI0 << k);
            }
        chunk_tab.clear();
        uint32_t off = 0;
        for (size_t c = 0; c < count.size(); ++c) {
            first[c] = off;
            if (count[c] || flags[c]) chunk_tab.insert(chunk_tab.end(), {(uint32_t)(c % ncx), (uint32_t)(c / ncx), off, count[c], (uint32_t)flags[c], 0u, 0u, 0u});
            off += count[c];
        }
        if (!chunk_tab.empty()) {
            bins.resize(off);
            for (uint32_t i = lo; i < hi; ++i) {
                const pfxk_line_dot& D = dots[i];
                if (D.x0 > D.x1) continue;
                for (uint32_t cy = D.y0 >> 6; cy <= D.y1 >> 6; ++cy)
                    for (uint32_t cx = D.x0 >> 6; cx <= D.x1 >> 6; ++cx) bins[first[(size_t)cy * ncx + cx]++] = i;
            }
            const size_t tab_off = (dot_bytes + 15u) & ~(size_t)15u, tab_bytes = chunk_tab.size() * 4u, bins_bytes = bins.size() * 4u;
            const size_t need = tab_off + tab_bytes + bins_bytes + 512u;
            if (!uploaded || need > ctx->d_pts.cap) {   // a block that grows moves: the dots go up again
                PFX_TRY(pfx_reserve(ctx, ctx->d_pts, need));
                if (dot_bytes) PFX_TRY(pfx_h2d(ctx, ctx->d_pts.p, dots.data(), dot_bytes));
                uploaded = true;
            }
            uint8_t* base = (uint8_t*)ctx->d_pts.p;
            PFX_TRY(pfx_h2d(ctx, base + tab_off, chunk_tab.data(), tab_bytes));
            if (bins_bytes) PFX_TRY(pfx_h2d(ctx, base + tab_off + tab_bytes, bins.data(), bins_bytes));
            PFX_HIP(ctx, hipStreamSynchronize(ctx->stream));   // the vectors are pageable host memory, rewritten by the next piece
            pfx_timer t(ctx, "line_render");
            PFX_HIP(ctx, pfxk_line_render(ctx->stream, &L, (uint8_t*)preview_dev, (const uint8_t*)sel_dev, w, h, (const pfxk_line_dot*)base, (const uint32_t*)(base + tab_off),
                                          (uint32_t)(chunk_tab.size() / 8u), (const uint32_t*)(base + tab_off + tab_bytes)));
        }
        if (hi == n_dots) break;
        lo = hi;
    }
    return PFX_OK;
}

} // namespace

extern "C" {

uint64_t pfx_int_line_piece_entries(uint64_t entries)
{
    return g_piece_entries.exchange(entries ? entries : MAX_ENTRIES, std::memory_order_relaxed);
}

int pfx_line_bounds(const pfx_line_tool* tool, uint32_t w, uint32_t h, float bounds[4])
{
    if (!bounds || !tool_ok(tool) || !pfx_dims_ok(w, h)) return PFX_ERR_INVALID;
    line_bounds(*tool, w, h, bounds);
    return PFX_OK;
}

int pfx_line_plan(const pfx_line_tool* tool, uint32_t w, uint32_t h, float* dots_xy, uint32_t capacity, uint32_t* n_out, float triangles_xy[12], uint32_t* n_triangles)
{
    if (!n_out || (capacity && !dots_xy) || !tool_ok(tool) || !pfx_dims_ok(w, h)) return PFX_ERR_INVALID;
    uint32_t n = 0;
    walk_dots(*tool, w, h, [&](float fx, float fy) {
        if (n < capacity) { dots_xy[2 * (size_t)n] = fx; dots_xy[2 * (size_t)n + 1] = fy; }
        ++n;
    });
    *n_out = n;   // above `capacity`: the list is cut there and the caller comes back with room for n
    float tri[12];
    const uint32_t nt = arrow_triangles(*tool, tri);
    if (triangles_xy) std::memcpy(triangles_xy, tri, (size_t)nt * 6u * sizeof(float));
    if (n_triangles) *n_triangles = nt;
    return PFX_OK;
}

int pfx_line_render_dev(pfx_ctx* ctx, const pfx_line_tool* tool, void* preview_dev, const void* sel_dev, uint32_t w, uint32_t h, const float last_bounds[4],
                        float bounds_out[4])
{
    const char* who = "pfx_line_render_dev";
    PFX_TRY(pfx_check_dims(ctx, who, w, h));
    PFX_TRY(check_tool(ctx, who, tool, last_bounds));
    PFX_TRY(check_render_bufs(ctx, who, true, preview_dev, sel_dev, w, h));
    return line_render_dev(ctx, *tool, preview_dev, sel_dev, w, h, last_bounds, bounds_out);
}

int pfx_line_render(pfx_ctx* ctx, const pfx_line_tool* tool, uint8_t* preview_inout, const uint8_t* sel, uint32_t w, uint32_t h, const float last_bounds[4],
                    float bounds_out[4])
{
    const char* who = "pfx_line_render";
    PFX_TRY(pfx_check_dims(ctx, who, w, h));
    PFX_TRY(check_tool(ctx, who, tool, last_bounds));
    PFX_TRY(check_render_bufs(ctx, who, false, preview_inout, sel, w, h));
    const size_t bytes = pfx_img_bytes(w, h);
    void* d_preview;
    const void* d_sel;
    PFX_TRY(pfx_stage(ctx, ctx->st_out, last_bounds ? preview_inout : nullptr, bytes, &d_preview));   // a first frame clears everything: nothing to upload
    PFX_TRY(pfx_stage_opt(ctx, ctx->st_mask, sel, (size_t)w * h, &d_sel));
    PFX_TRY(line_render_dev(ctx, *tool, d_preview, d_sel, w, h, last_bounds, bounds_out));
    return pfx_unstage(ctx, preview_inout, ctx->st_out, bytes);
}

int pfx_stroke_commit_mask_dev(pfx_ctx* ctx, void* conceal_dev, const void* preview_dev, const void* sel_dev, uint32_t w, uint32_t h, int reveal)
{
    const char* who = "pfx_stroke_commit_mask_dev";
    PFX_TRY(pfx_check_dims(ctx, who, w, h));
    PFX_TRY(pfx_check_args(ctx, who, true, {{conceal_dev, (size_t)w * h, PFX_ARG_OUT, "conceal_dev"},
                                            {preview_dev, pfx_img_bytes(w, h), PFX_ARG_DWORD, "preview_dev"},
                                            {sel_dev, (size_t)w * h, PFX_ARG_OPTIONAL, "sel_dev"}}));
    pfx_timer t(ctx, "stroke_commit_mask");
    PFX_HIP(ctx, pfxk_line_commit_mask(ctx->stream, (uint8_t*)conceal_dev, (const uint8_t*)preview_dev, (const uint8_t*)sel_dev, w, h, reveal != 0));
    return PFX_OK;
}

int pfx_stroke_commit_mask(pfx_ctx* ctx, uint8_t* conceal_inout, const uint8_t* preview, const uint8_t* sel, uint32_t w, uint32_t h, int reveal)
{
    const char* who = "pfx_stroke_commit_mask";
    PFX_TRY(pfx_check_dims(ctx, who, w, h));
    PFX_TRY(pfx_check_args(ctx, who, false, {{conceal_inout, (size_t)w * h, PFX_ARG_OUT, "conceal_inout"},
                                             {preview, pfx_img_bytes(w, h), PFX_ARG_IN, "preview"},
                                             {sel, (size_t)w * h, PFX_ARG_OPTIONAL, "sel"}}));
    void *d_conceal, *d_preview;
    const void* d_sel;
    PFX_TRY(pfx_stage(ctx, ctx->st_out, conceal_inout, (size_t)w * h, &d_conceal));
    PFX_TRY(pfx_stage(ctx, ctx->st_in, preview, pfx_img_bytes(w, h), &d_preview));
    PFX_TRY(pfx_stage_opt(ctx, ctx->st_mask, sel, (size_t)w * h, &d_sel));
    PFX_TRY(pfx_stroke_commit_mask_dev(ctx, d_conceal, d_preview, d_sel, w, h, reveal));
    return pfx_unstage(ctx, conceal_inout, ctx->st_out, (size_t)w * h);
}

} // extern "C"
