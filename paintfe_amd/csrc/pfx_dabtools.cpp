// pfx_dabtools.cpp — C ABI of the clone stamp, the heal brush's live stroke and the pencil (k_dabtools.hip), and the release of a stroke on device memory.
// Reference: src/ui/panels/tools/behavior/raster/clone_heal.rs — clone_stamp_circle :6, clone_stamp_line :101, heal_circle :141, heal_line :262,
// draw_pixel_and_get_bounds :295, draw_pixel_line_and_get_bounds :370; the release is commit_bezier_to_layer / commit_eraser_to_layer (pfxk_brush_commit).
// The host prologue does what the reference does once per dab — the pixel box and the returned dirty rect, with its float operations — and deals the dabs to
// the 64 x 64 chunks their boxes touch.  pfx_brush_stamps_ex_dev (pfx_api.cpp) bins its stamps the same way inside its own body; the few lines are restated
// here rather than moved.  Every entry point checks its sizes, then its descriptor and buffers, then its points, and only then uploads and launches.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <vector>

#include "k_brush_math.h"
#include "pfx_internal.h"

namespace {

// chunk-list entries of one launch: a longer stroke is sent in consecutive pieces, which the preview carries across exactly as it carries a stroke across calls.
// One dab alone stays below this: a canvas has at most 62 500 chunks
constexpr uint64_t MAX_ENTRIES = 8ull << 20;
std::atomic<uint64_t> g_piece_entries{MAX_ENTRIES};   // pfx_int_dab_piece_entries: the tests lower it to send a small stroke in many pieces
constexpr float MAX_LINE_STEPS = 16777216.0f;   // the line helper's bound on ceil(distance): beyond it `i as f32` stops being exact and no canvas is that long

struct dirty_box {   // Rect::union over the dabs' returned rects: componentwise min / max, Rect::NOTHING = (+inf, -inf)
    bool any = false;
    uint32_t x0 = 0, y0 = 0, x1 = 0, y1 = 0;
    void add(uint32_t ax0, uint32_t ay0, uint32_t ax1, uint32_t ay1)
    {
        if (!any) { x0 = ax0; y0 = ay0; x1 = ax1; y1 = ay1; any = true; return; }
        x0 = std::min(x0, ax0); y0 = std::min(y0, ay0); x1 = std::max(x1, ax1); y1 = std::max(y1, ay1);
    }
    void store(uint32_t out[4]) const
    {
        if (!out) return;
        out[0] = any ? x0 : 0u; out[1] = any ? y0 : 0u; out[2] = any ? x1 : 0u; out[3] = any ? y1 : 0u;
    }
};
inline uint32_t sat_sub1(uint32_t v) { return v ? v - 1u : 0u; }

int check_points(pfx_ctx* ctx, const char* who, const float* points_xy, uint32_t n_points)
{
    if (!points_xy) return pfx_fail(ctx, PFX_ERR_INVALID, "%s: points_xy is null", who);
    for (size_t k = 0; k < 2 * (size_t)n_points; ++k)
        if (!std::isfinite(points_xy[k])) return pfx_fail(ctx, PFX_ERR_INVALID, "%s: point %zu is not finite", who, k / 2);
    return PFX_OK;
}

// the shared device tier of the clone stamp and the heal ring: T is filled and the buffers are checked
int dab_stroke_dev(pfx_ctx* ctx, const char* who, const pfxk_dabtool& T, const void* source_dev, void* preview_dev, const void* sel_dev, uint32_t w, uint32_t h,
                   const float* points_xy, uint32_t n_points, uint32_t dirty[4])
{
    dirty_box box;
    if (n_points == 0) { box.store(dirty); return PFX_OK; }
    PFX_TRY(check_points(ctx, who, points_xy, n_points));
    // :17-20 / :149-152 and the returned rect :88-97 / :249-258
    std::vector<pfxk_dab> dabs(n_points);
    const uint32_t wm1 = w - 1u, hm1 = h - 1u;
    for (uint32_t i = 0; i < n_points; ++i) {
        pfxk_dab& D = dabs[i];
        D.cx = points_xy[2 * (size_t)i]; D.cy = points_xy[2 * (size_t)i + 1]; D.pad[0] = D.pad[1] = 0u;
        D.x0 = pfx_f32_as_u32(fmaxf(D.cx - T.radius, 0.0f)); D.x1 = std::min(pfx_f32_as_u32(D.cx + T.radius), wm1);
        D.y0 = pfx_f32_as_u32(fmaxf(D.cy - T.radius, 0.0f)); D.y1 = std::min(pfx_f32_as_u32(D.cy + T.radius), hm1);
        box.add(sat_sub1(D.x0), sat_sub1(D.y0), std::min(D.x1 + 2u, w), std::min(D.y1 + 2u, h));
        if (D.x0 > D.x1 || D.y0 > D.y1) { D.x0 = 1u; D.x1 = 0u; D.y0 = 1u; D.y1 = 0u; }   // the reference's empty loop ranges
    }
    box.store(dirty);
    const uint32_t ncx = (w + 63u) / 64u, ncy = (h + 63u) / 64u;
    const size_t dab_bytes = dabs.size() * sizeof(pfxk_dab);
    bool uploaded = false;
    const uint64_t max_entries = g_piece_entries.load(std::memory_order_relaxed);
    std::vector<uint32_t> count((size_t)ncx * ncy), first((size_t)ncx * ncy), chunk_tab, bins;
    for (uint32_t lo = 0; lo < n_points;) {
        // the piece [lo, hi): as many dabs as stay within max_entries chunk-list entries, and at least one
        uint64_t entries = 0;
        uint32_t hi = lo;
        std::fill(count.begin(), count.end(), 0u);
        for (; hi < n_points; ++hi) {
            const pfxk_dab& D = dabs[hi];
            if (D.x0 > D.x1) continue;
            const uint64_t e = (uint64_t)((D.x1 >> 6) - (D.x0 >> 6) + 1u) * ((D.y1 >> 6) - (D.y0 >> 6) + 1u);
            if (entries + e > max_entries && hi > lo) break;
            entries += e;
            for (uint32_t cy = D.y0 >> 6; cy <= D.y1 >> 6; ++cy)
                for (uint32_t cx = D.x0 >> 6; cx <= D.x1 >> 6; ++cx) ++count[(size_t)cy * ncx + cx];
        }
        if (entries) {
            chunk_tab.clear();
            uint32_t off = 0;
            for (size_t c = 0; c < count.size(); ++c) {
                first[c] = off;
                if (count[c]) { chunk_tab.push_back((uint32_t)(c % ncx)); chunk_tab.push_back((uint32_t)(c / ncx)); chunk_tab.push_back(off); chunk_tab.push_back(count[c]); }
                off += count[c];
            }
            bins.resize(off);
            for (uint32_t i = lo; i < hi; ++i) {   // dabs in order: every chunk's list comes out in stroke order
                const pfxk_dab& D = dabs[i];
                if (D.x0 > D.x1) continue;
                for (uint32_t cy = D.y0 >> 6; cy <= D.y1 >> 6; ++cy)
                    for (uint32_t cx = D.x0 >> 6; cx <= D.x1 >> 6; ++cx) bins[first[(size_t)cy * ncx + cx]++] = i;
            }
            const size_t tab_off = (dab_bytes + 15u) & ~(size_t)15u, tab_bytes = chunk_tab.size() * 4u, bins_bytes = bins.size() * 4u;
            const size_t need = tab_off + tab_bytes + bins_bytes + 512u;
            if (!uploaded || need > ctx->d_pts.cap) {   // a block that grows moves: the dabs go up again
                PFX_TRY(pfx_reserve(ctx, ctx->d_pts, need));
                PFX_TRY(pfx_h2d(ctx, ctx->d_pts.p, dabs.data(), dab_bytes));
                uploaded = true;
            }
            uint8_t* base = (uint8_t*)ctx->d_pts.p;
            PFX_TRY(pfx_h2d(ctx, base + tab_off, chunk_tab.data(), tab_bytes));
            PFX_TRY(pfx_h2d(ctx, base + tab_off + tab_bytes, bins.data(), bins_bytes));
            PFX_HIP(ctx, hipStreamSynchronize(ctx->stream));   // the vectors are pageable host memory, rewritten by the next piece
            pfx_timer t(ctx, T.tool == PFXK_DAB_HEAL ? "heal_ring" : "clone_stamp");
            PFX_HIP(ctx, pfxk_dab_stroke(ctx->stream, &T, (const uint8_t*)source_dev, (uint8_t*)preview_dev, (const uint8_t*)sel_dev, w, h, (const pfxk_dab*)base,
                                         (const uint32_t*)(base + tab_off), (uint32_t)(chunk_tab.size() / 4u), (const uint32_t*)(base + tab_off + tab_bytes)));
        }
        lo = hi;
    }
    return PFX_OK;
}

int check_stroke_bufs(pfx_ctx* ctx, const char* who, bool dev, const void* source, void* preview, const void* sel, uint32_t w, uint32_t h)
{
    const int dword = dev ? PFX_ARG_DWORD : 0;
    return pfx_check_args(ctx, who, dev, {{source, pfx_img_bytes(w, h), PFX_ARG_IN | dword, dev ? "source_dev" : "source"},
                                          {preview, pfx_img_bytes(w, h), PFX_ARG_OUT | dword, dev ? "preview_dev" : "preview_inout"},
                                          {sel, (size_t)w * h, PFX_ARG_OPTIONAL, dev ? "sel_dev" : "sel"}});
}

int clone_params(pfx_ctx* ctx, const char* who, const pfx_clone_stamp_tool* tool, pfxk_dabtool* T)
{
    if (!tool) return pfx_fail(ctx, PFX_ERR_INVALID, "%s: tool is null", who);
    for (float v : {tool->size, tool->hardness, tool->offset_x, tool->offset_y})
        if (!std::isfinite(v)) return pfx_fail(ctx, PFX_ERR_INVALID, "%s: a tool field is not finite", who);
    std::memset(T, 0, sizeof *T);
    T->tool = PFXK_DAB_CLONE;
    T->radius = tool->size / 2.0f;
    T->hardness = tool->hardness;
    T->anti_aliased = tool->anti_aliased != 0;
    T->offset_x = tool->offset_x; T->offset_y = tool->offset_y;
    return PFX_OK;
}

int heal_params(pfx_ctx* ctx, const char* who, const pfx_heal_ring_tool* tool, pfxk_dabtool* T)
{
    if (!tool) return pfx_fail(ctx, PFX_ERR_INVALID, "%s: tool is null", who);
    for (float v : {tool->size, tool->hardness, tool->sample_radius})
        if (!std::isfinite(v)) return pfx_fail(ctx, PFX_ERR_INVALID, "%s: a tool field is not finite", who);
    std::memset(T, 0, sizeof *T);
    T->tool = PFXK_DAB_HEAL;
    T->radius = tool->size / 2.0f;
    T->hardness = tool->hardness;
    T->hard_t = pfx_clampf(tool->hardness * 0.9f + 0.1f, 0.0f, 1.0f);   // :194
    T->hard_den = 1.0f - T->hard_t + 1e-6f;                             // :198
    T->sample_radius = tool->sample_radius;
    return PFX_OK;
}

// the host-buffer tier of both: source -> st_in, preview -> st_out, sel -> st_mask (the device tier's own scratch is d_pts)
int dab_stroke_host(pfx_ctx* ctx, const char* who, const pfxk_dabtool& T, const uint8_t* source, uint8_t* preview_inout, const uint8_t* sel, uint32_t w, uint32_t h,
                    const float* points_xy, uint32_t n_points, uint32_t dirty[4])
{
    if (n_points == 0) return dab_stroke_dev(ctx, who, T, nullptr, nullptr, nullptr, w, h, points_xy, 0u, dirty);
    PFX_TRY(check_points(ctx, who, points_xy, n_points));
    const size_t bytes = pfx_img_bytes(w, h);
    void *d_source, *d_preview;
    const void* d_sel;
    PFX_TRY(pfx_stage(ctx, ctx->st_in, source, bytes, &d_source));
    PFX_TRY(pfx_stage(ctx, ctx->st_out, preview_inout, bytes, &d_preview));
    PFX_TRY(pfx_stage_opt(ctx, ctx->st_mask, sel, (size_t)w * h, &d_sel));
    PFX_TRY(dab_stroke_dev(ctx, who, T, d_source, d_preview, d_sel, w, h, points_xy, n_points, dirty));
    return pfx_unstage(ctx, preview_inout, ctx->st_out, bytes);
}

int pencil_color(pfx_ctx* ctx, const char* who, const float color[4])
{
    if (!color) return pfx_fail(ctx, PFX_ERR_INVALID, "%s: color is null", who);
    for (int k = 0; k < 4; ++k)
        if (!std::isfinite(color[k])) return pfx_fail(ctx, PFX_ERR_INVALID, "%s: color[%d] is not finite", who, k);
    return PFX_OK;
}

// the rects of the listed cells inside the canvas :313, :363-366.  The selection is not consulted (the device tier's lives on the device): where it masks
// a cell the reference returns Rect::NOTHING for it, so this box contains the reference's
void pencil_dirty(const int32_t* cells_xy, uint32_t n_cells, uint32_t w, uint32_t h, uint32_t dirty[4])
{
    dirty_box box;
    for (uint32_t k = 0; k < n_cells; ++k) {
        const int32_t x = cells_xy[2 * (size_t)k], y = cells_xy[2 * (size_t)k + 1];
        if (x < 0 || y < 0 || (uint32_t)x >= w || (uint32_t)y >= h) continue;
        box.add(sat_sub1((uint32_t)x), sat_sub1((uint32_t)y), std::min((uint32_t)x + 2u, w), std::min((uint32_t)y + 2u, h));
    }
    box.store(dirty);
}

} // namespace

extern "C" {

uint64_t pfx_int_dab_piece_entries(uint64_t entries)
{
    return g_piece_entries.exchange(entries ? entries : MAX_ENTRIES, std::memory_order_relaxed);
}

int pfx_stroke_line_points(float x0, float y0, float x1, float y1, uint32_t w, uint32_t h, float* points_xy, uint32_t capacity, uint32_t* n_out)
{
    if (!n_out || (capacity && !points_xy) || !pfx_dims_ok(w, h)) return PFX_ERR_INVALID;
    for (float v : {x0, y0, x1, y1})
        if (!std::isfinite(v)) return PFX_ERR_INVALID;
    const float dx = x1 - x0, dy = y1 - y0;
    const float distance = sqrtf(dx * dx + dy * dy);
    uint32_t n = 0;
    auto put = [&](float x, float y) {
        if (n < capacity) { points_xy[2 * (size_t)n] = x; points_xy[2 * (size_t)n + 1] = y; }
        ++n;
    };
    if (distance < 0.1f) put(x0, y0);   // :112 — the single circle, with no canvas test
    else {
        const float steps_f = ceilf(distance);
        if (!(steps_f <= MAX_LINE_STEPS)) return PFX_ERR_INVALID;   // also an overflowed (infinite) distance
        const uint32_t steps = (uint32_t)steps_f;
        for (uint32_t i = 0; i <= steps; ++i) {   // :119-130
            const float t = (float)i / (float)steps;
            const float x = x0 + dx * t, y = y0 + dy * t;
            if (x >= 0.0f && pfx_f32_as_u32(x) < w && y >= 0.0f && pfx_f32_as_u32(y) < h) put(x, y);
        }
    }
    *n_out = n;   // above `capacity`: the list is cut there and the caller comes back with room for n
    return PFX_OK;
}

int pfx_pencil_line_cells(float x0, float y0, float x1, float y1, uint32_t w, uint32_t h, int32_t* cells_xy, uint32_t capacity, uint32_t* n_out)
{
    if (!n_out || (capacity && !cells_xy) || !pfx_dims_ok(w, h)) return PFX_ERR_INVALID;
    for (float v : {x0, y0, x1, y1})
        if (!std::isfinite(v) || fabsf(v) > MAX_LINE_STEPS) return PFX_ERR_INVALID;   // bounds the walk; `as i32` is then exact
    int64_t cx = (int64_t)floorf(x0), cy = (int64_t)floorf(y0);   // :389-398
    const int64_t ex = (int64_t)floorf(x1), ey = (int64_t)floorf(y1);
    const int64_t dx = std::llabs(ex - cx), dy = std::llabs(ey - cy);
    const int64_t sx = cx < ex ? 1 : -1, sy = cy < ey ? 1 : -1;
    int64_t err = dx - dy;
    uint32_t n = 0;
    for (;;) {
        if (cx >= 0 && cx < (int64_t)w && cy >= 0 && cy < (int64_t)h) {
            if (n < capacity) { cells_xy[2 * (size_t)n] = (int32_t)cx; cells_xy[2 * (size_t)n + 1] = (int32_t)cy; }
            ++n;
        }
        if (cx == ex && cy == ey) break;
        const int64_t e2 = 2 * err;
        if (e2 > -dy) { err -= dy; cx += sx; }
        if (e2 < dx) { err += dx; cy += sy; }
    }
    *n_out = n;   // above `capacity`: the list is cut there and the caller comes back with room for n
    return PFX_OK;
}

int pfx_clone_stamp_dev(pfx_ctx* ctx, const pfx_clone_stamp_tool* tool, const void* source_dev, void* preview_dev, const void* sel_dev, uint32_t w, uint32_t h,
                        const float* points_xy, uint32_t n_points, uint32_t dirty[4])
{
    const char* who = "pfx_clone_stamp_dev";
    pfxk_dabtool T;
    PFX_TRY(pfx_check_dims(ctx, who, w, h));
    PFX_TRY(clone_params(ctx, who, tool, &T));
    PFX_TRY(check_stroke_bufs(ctx, who, true, source_dev, preview_dev, sel_dev, w, h));
    return dab_stroke_dev(ctx, who, T, source_dev, preview_dev, sel_dev, w, h, points_xy, n_points, dirty);
}

int pfx_heal_ring_dev(pfx_ctx* ctx, const pfx_heal_ring_tool* tool, const void* source_dev, void* preview_dev, const void* sel_dev, uint32_t w, uint32_t h,
                      const float* points_xy, uint32_t n_points, uint32_t dirty[4])
{
    const char* who = "pfx_heal_ring_dev";
    pfxk_dabtool T;
    PFX_TRY(pfx_check_dims(ctx, who, w, h));
    PFX_TRY(heal_params(ctx, who, tool, &T));
    PFX_TRY(check_stroke_bufs(ctx, who, true, source_dev, preview_dev, sel_dev, w, h));
    return dab_stroke_dev(ctx, who, T, source_dev, preview_dev, sel_dev, w, h, points_xy, n_points, dirty);
}

int pfx_clone_stamp(pfx_ctx* ctx, const pfx_clone_stamp_tool* tool, const uint8_t* source, uint8_t* preview_inout, const uint8_t* sel, uint32_t w, uint32_t h,
                    const float* points_xy, uint32_t n_points, uint32_t dirty[4])
{
    const char* who = "pfx_clone_stamp";
    pfxk_dabtool T;
    PFX_TRY(pfx_check_dims(ctx, who, w, h));
    PFX_TRY(clone_params(ctx, who, tool, &T));
    PFX_TRY(check_stroke_bufs(ctx, who, false, source, preview_inout, sel, w, h));
    return dab_stroke_host(ctx, who, T, source, preview_inout, sel, w, h, points_xy, n_points, dirty);
}

int pfx_heal_ring(pfx_ctx* ctx, const pfx_heal_ring_tool* tool, const uint8_t* source, uint8_t* preview_inout, const uint8_t* sel, uint32_t w, uint32_t h,
                  const float* points_xy, uint32_t n_points, uint32_t dirty[4])
{
    const char* who = "pfx_heal_ring";
    pfxk_dabtool T;
    PFX_TRY(pfx_check_dims(ctx, who, w, h));
    PFX_TRY(heal_params(ctx, who, tool, &T));
    PFX_TRY(check_stroke_bufs(ctx, who, false, source, preview_inout, sel, w, h));
    return dab_stroke_host(ctx, who, T, source, preview_inout, sel, w, h, points_xy, n_points, dirty);
}

int pfx_pencil_dev(pfx_ctx* ctx, const float color[4], void* preview_dev, const void* sel_dev, uint32_t w, uint32_t h, const int32_t* cells_xy, uint32_t n_cells,
                   uint32_t dirty[4])
{
    const char* who = "pfx_pencil_dev";
    PFX_TRY(pfx_check_dims(ctx, who, w, h));
    PFX_TRY(pencil_color(ctx, who, color));
    PFX_TRY(pfx_check_args(ctx, who, true, {{preview_dev, pfx_img_bytes(w, h), PFX_ARG_OUT | PFX_ARG_DWORD, "preview_dev"},
                                            {sel_dev, (size_t)w * h, PFX_ARG_OPTIONAL, "sel_dev"}}));
    if (n_cells == 0) { pencil_dirty(nullptr, 0u, w, h, dirty); return PFX_OK; }
    if (!cells_xy) return pfx_fail(ctx, PFX_ERR_INVALID, "%s: cells_xy is null", who);
    pencil_dirty(cells_xy, n_cells, w, h, dirty);
    const size_t bytes = (size_t)n_cells * 8u;
    PFX_TRY(pfx_reserve(ctx, ctx->d_pts, bytes + 512u));
    PFX_TRY(pfx_h2d(ctx, ctx->d_pts.p, cells_xy, bytes));
    PFX_HIP(ctx, hipStreamSynchronize(ctx->stream));   // the caller's list may be pageable memory it reuses at once
    pfx_timer t(ctx, "pencil");
    PFX_HIP(ctx, pfxk_pencil_cells(ctx->stream, (uint8_t*)preview_dev, (const uint8_t*)sel_dev, w, h, (const int32_t*)ctx->d_pts.p, n_cells, color[0], color[1], color[2],
                                   color[3]));
    return PFX_OK;
}

int pfx_pencil(pfx_ctx* ctx, const float color[4], uint8_t* preview_inout, const uint8_t* sel, uint32_t w, uint32_t h, const int32_t* cells_xy, uint32_t n_cells,
               uint32_t dirty[4])
{
    const char* who = "pfx_pencil";
    PFX_TRY(pfx_check_dims(ctx, who, w, h));
    PFX_TRY(pencil_color(ctx, who, color));
    const size_t bytes = pfx_img_bytes(w, h);
    PFX_TRY(pfx_check_args(ctx, who, false, {{preview_inout, bytes, PFX_ARG_OUT, "preview_inout"}, {sel, (size_t)w * h, PFX_ARG_OPTIONAL, "sel"}}));
    if (n_cells == 0) { pencil_dirty(nullptr, 0u, w, h, dirty); return PFX_OK; }
    if (!cells_xy) return pfx_fail(ctx, PFX_ERR_INVALID, "%s: cells_xy is null", who);
    void* d_preview;
    const void* d_sel;
    PFX_TRY(pfx_stage(ctx, ctx->st_out, preview_inout, bytes, &d_preview));
    PFX_TRY(pfx_stage_opt(ctx, ctx->st_mask, sel, (size_t)w * h, &d_sel));
    PFX_TRY(pfx_pencil_dev(ctx, color, d_preview, d_sel, w, h, cells_xy, n_cells, dirty));
    return pfx_unstage(ctx, preview_inout, ctx->st_out, bytes);
}

int pfx_stroke_commit_dev(pfx_ctx* ctx, void* active_layer_dev, const void* preview_dev, const void* sel_dev, uint32_t w, uint32_t h, uint8_t blend_mode, int is_eraser)
{
    const char* who = "pfx_stroke_commit_dev";
    PFX_TRY(pfx_check_dims(ctx, who, w, h));
    PFX_TRY(pfx_check_args(ctx, who, true, {{active_layer_dev, pfx_img_bytes(w, h), PFX_ARG_OUT | PFX_ARG_DWORD, "active_layer_dev"},
                                            {preview_dev, pfx_img_bytes(w, h), PFX_ARG_DWORD, "preview_dev"},
                                            {sel_dev, (size_t)w * h, PFX_ARG_OPTIONAL, "sel_dev"}}));
    pfx_timer t(ctx, "stroke_commit");
    PFX_HIP(ctx, pfxk_brush_commit(ctx->stream, (uint8_t*)active_layer_dev, (const uint8_t*)preview_dev, (const uint8_t*)sel_dev, w, h, blend_mode > 24 ? 0u : blend_mode,
                                   is_eraser));   // an unknown mode commits as Normal, as pfx_brush_commit does
    return PFX_OK;
}

} // extern "C"
