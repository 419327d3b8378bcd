// pfx_flood.cpp — C ABI of the bucket fill and the magic wand (k_flood.hip).  Reference: src/ui/panels/tools/behavior/raster/fill_magic.rs —
// tolerance_threshold_u8 :78, srgb_to_linear :84, compute_flood_distance_map :950, perform_flood_fill :1231; tools/state.rs:693 from_distances.
// The host computes what is uniform over the image with the reference's own f32 expressions (no contraction): the 256-entry srgb_to_linear table (host powf,
// uploaded once per context) and the target's linear terms.  For the contiguous scope it runs the pass loop: one 8-byte read-back per pass (how many tiles
// the next pass visits, whether a byte decreased) ends it, as does the cap of w * h + 2 passes (DESIGN.md "Flood distance maps": an optimal path has at most
// w * h pixels and every pass settles the next one).  The flood runs in working memory: a failed call leaves `dist` untouched.  The pass loop itself
// (pfx_flood_converge) takes a device cost map: the colour remover's core flood (pfx_colorkey.cpp) runs it over its passability map.
#include <algorithm>
#include <cmath>

#include "pfx_internal.h"

namespace {

float srgb_to_linear(float v) { return v <= 0.04045f ? v / 12.92f : powf((v + 0.055f) / 1.055f, 2.4f); }   // :84

int check_flood(pfx_ctx* ctx, const void* src, uint32_t w, uint32_t h, const pfx_flood* f, const void* dist, bool dev, const char* who)
{
    PFX_TRY(pfx_check_dims(ctx, who, w, h));
    const size_t px = (size_t)w * h;
    PFX_TRY(pfx_check_args(ctx, who, dev, {{src, px * 4, PFX_ARG_DWORD, "src"}, {dist, px, PFX_ARG_OUT, "dist"}, {f, 0, PFX_ARG_IN, "flood"}}));
    if (f->connectivity != 4 && f->connectivity != 8) return pfx_fail(ctx, PFX_ERR_INVALID, "%s: connectivity %u (4 or 8)", who, f->connectivity);
    if (f->distance_mode > 1 || f->global > 1) return pfx_fail(ctx, PFX_ERR_INVALID, "%s: unknown distance mode %u or scope %u", who, f->distance_mode, f->global);
    if (f->seed_x >= w || f->seed_y >= h) return pfx_fail(ctx, PFX_ERR_INVALID, "%s: seed (%u, %u) outside the %ux%u image", who, f->seed_x, f->seed_y, w, h);
    return PFX_OK;
}

// the threshold kernels' shared declaration: an output of `out_px` bytes per pixel — the wand's mask (1), which may BE the base mask, or an RGBA8 image (4),
// dword-aligned on the device — against the distance map and `other` (the base mask / the selection, may be NULL); `fill` is the colour, where there is one
int check_threshold_call(pfx_ctx* ctx, const void* dist, const void* other, const void* out, size_t out_px, bool dev, uint32_t w, uint32_t h, const uint8_t* fill,
                         const char* who)
{
    PFX_TRY(pfx_check_dims(ctx, who, w, h));
    const size_t px = (size_t)w * h;
    const bool wand = out_px == 1;
    return pfx_check_args(ctx, who, dev, {{dist, px, PFX_ARG_IN, "dist"}, {other, px, PFX_ARG_OPTIONAL, wand ? "base_mask" : "selection"},
                                          {out, px * out_px, wand ? PFX_ARG_OUT : PFX_ARG_OUT | PFX_ARG_DWORD, wand ? "mask_out" : "the image"},
                                          {fill, 0, wand ? PFX_ARG_OPTIONAL : PFX_ARG_IN, "fill"}}, wand ? other : nullptr);
}

int flood_table(pfx_ctx* ctx)
{
    if (ctx->flood_lut_valid) return PFX_OK;
    float lin[256];
    for (int k = 0; k < 256; ++k) lin[k] = srgb_to_linear((float)k / 255.0f);
    PFX_TRY(pfx_reserve(ctx, ctx->flood_lut, sizeof lin));
    PFX_TRY(pfx_h2d(ctx, ctx->flood_lut.p, lin, sizeof lin));
    PFX_TRY(pfx_sync(ctx));   // `lin` is pageable host memory about to go out of scope
    ctx->flood_lut_valid = true;
    return PFX_OK;
}

pfxk_flood_target make_target(const pfx_flood* f)
{
    pfxk_flood_target G;
    G.rgba = pfx_pack_rgba8(f->target);
    G.ta = (float)f->target[3] / 255.0f;
    for (int k = 0; k < 3; ++k) G.lin[k] = srgb_to_linear((float)f->target[k] / 255.0f) * G.ta;   // :112-114
    return G;
}

} // namespace

// working memory, one block: 256 bytes of state (two {list length, changed} pairs, one per list) | c | d | two tile lists | the tiles' pass stamps
int pfx_flood_work_reserve(pfx_ctx* ctx, uint32_t w, uint32_t h, pfx_flood_work* W)
{
    const uint32_t T = PFXK_FLOOD_TILE;
    const size_t px = (size_t)w * h, tiles = (size_t)((w + T - 1) / T) * ((h + T - 1) / T);
    const size_t off_c = 256, off_d = off_c + pfx_align256(px), off_l0 = off_d + pfx_align256(px), off_l1 = off_l0 + pfx_align256(tiles * 4),
                 off_mark = off_l1 + pfx_align256(tiles * 4), total = off_mark + pfx_align256(tiles * 4);
    PFX_TRY(pfx_reserve(ctx, ctx->flood_ws, total));
    uint8_t* ws = (uint8_t*)ctx->flood_ws.p;
    W->state = (uint32_t*)ws;
    W->c = ws + off_c;
    W->d = ws + off_d;
    W->lists[0] = (uint32_t*)(ws + off_l0);
    W->lists[1] = (uint32_t*)(ws + off_l1);
    W->mark = (uint32_t*)(ws + off_mark);
    W->tiles = tiles;
    return PFX_OK;
}

// The pass loop over the cost map in W->c; the map ends in W->d.  Adds to the context's flood counters (the caller zeroes them).
int pfx_flood_converge(pfx_ctx* ctx, const pfx_flood_work* W, uint32_t w, uint32_t h, uint32_t seed_x, uint32_t seed_y, int connectivity, const char* who)
{
    const size_t px = (size_t)w * h, tiles = W->tiles;
    uint32_t* state = W->state;
    uint8_t *c = W->c, *d = W->d;
    uint32_t* const* lists = W->lists;
    uint32_t* mark = W->mark;
    PFX_HIP(ctx, hipMemsetAsync(d, 0xff, px, ctx->stream));
    PFX_HIP(ctx, hipMemsetAsync(mark, 0, tiles * 4, ctx->stream));
    PFX_HIP(ctx, pfxk_flood_seed(ctx->stream, w, seed_x, seed_y, lists[0]));
    ctx->flood_launches += 1;
    // Every pass but the last lowers a byte, and after pass k the first k pixels of every optimal path hold their final value (the first pass plants the seed):
    // at most w * h + 1 passes change something.  The cap can only be met by a defect.
    const uint64_t max_passes = (uint64_t)px + 2u;
    uint32_t n_cur = 1;
    for (uint64_t pass = 0;; ++pass) {
        if (pass >= max_passes) return pfx_fail(ctx, PFX_ERR_HIP, "%s: internal error: no fixed point after %llu passes", who, (unsigned long long)pass);
        uint32_t* st = state + 2 * ((pass + 1) & 1);
        uint32_t got[2] = {0, 0};
        PFX_HIP(ctx, hipMemsetAsync(st, 0, 8, ctx->stream));
        PFX_HIP(ctx, pfxk_flood_pass(ctx->stream, connectivity, c, d, w, h, lists[pass & 1], n_cur, lists[(pass + 1) & 1], st, mark, (uint32_t)(pass + 1),
                                     pass == 0 ? seed_x : 0xffffffffu, pass == 0 ? seed_y : 0xffffffffu));
        PFX_TRY(pfx_d2h(ctx, got, st, sizeof got));
        PFX_TRY(pfx_sync(ctx));
        ctx->flood_passes += 1;
        ctx->flood_launches += 1;
        ctx->flood_visits += n_cur;
        if ((size_t)got[0] > tiles) return pfx_fail(ctx, PFX_ERR_HIP, "%s: internal error: tile list overruns the tile count", who);   // cannot happen: a tile is listed once per pass
        n_cur = got[0];
        if (n_cur == 0 || got[1] == 0) break;   // nothing scheduled / a pass that wrote nothing
    }
    return PFX_OK;
}

extern "C" {

uint8_t pfx_tolerance_threshold(float tolerance)
{
    float n = tolerance / 100.0f;
    n = n < 0.0f ? 0.0f : (n > 1.0f ? 1.0f : n);   // f32::clamp: a NaN stays a NaN
    const float r = roundf(n * 255.0f);
    return !(r > 0.0f) ? 0 : (r >= 255.0f ? 255 : (uint8_t)r);   // .clamp(0.0, 255.0) as u8: NaN -> 0
}

int pfx_flood_distance_dev(pfx_ctx* ctx, const void* src_dev, uint32_t w, uint32_t h, const pfx_flood* flood, void* dist_dev)
{
    PFX_TRY(check_flood(ctx, src_dev, w, h, flood, dist_dev, true, "pfx_flood_distance_dev"));
    const size_t px = (size_t)w * h;
    ctx->flood_passes = ctx->flood_launches = ctx->flood_visits = 0;
    if (flood->distance_mode == 1) PFX_TRY(flood_table(ctx));
    const pfxk_flood_target G = make_target(flood);
    const float* table = flood->distance_mode == 1 ? (const float*)ctx->flood_lut.p : nullptr;
    if (flood->global) {   // compute_global_distance_map :1024, written straight into dist_dev: past the checks above only the launch itself can fail
        pfx_timer t(ctx, "flood_distance_global");
        PFX_HIP(ctx, pfxk_color_distance(ctx->stream, (const uint8_t*)src_dev, (uint8_t*)dist_dev, px, flood->distance_mode, &G, table));
        ctx->flood_launches = 1;
        return PFX_OK;
    }
    pfx_flood_work W;
    PFX_TRY(pfx_flood_work_reserve(ctx, w, h, &W));   // a failure leaves dist untouched
    pfx_timer t(ctx, "flood_distance");
    PFX_HIP(ctx, pfxk_color_distance(ctx->stream, (const uint8_t*)src_dev, W.c, px, flood->distance_mode, &G, table));
    ctx->flood_launches = 1;
    PFX_TRY(pfx_flood_converge(ctx, &W, w, h, flood->seed_x, flood->seed_y, flood->connectivity, "pfx_flood_distance_dev"));
    PFX_HIP(ctx, hipMemcpyAsync(dist_dev, W.d, px, hipMemcpyDeviceToDevice, ctx->stream));
    return PFX_OK;
}

int pfx_flood_distance(pfx_ctx* ctx, const uint8_t* src, uint32_t w, uint32_t h, const pfx_flood* flood, uint8_t* dist)
{
    PFX_TRY(check_flood(ctx, src, w, h, flood, dist, false, "pfx_flood_distance"));
    const size_t px = (size_t)w * h;
    void *d_src, *d_dist;
    PFX_TRY(pfx_stage(ctx, ctx->st_in, src, px * 4, &d_src));
    PFX_TRY(pfx_stage(ctx, ctx->st_mask, nullptr, px, &d_dist));
    PFX_TRY(pfx_flood_distance_dev(ctx, d_src, w, h, flood, d_dist));
    return pfx_unstage(ctx, dist, ctx->st_mask, px);
}

int pfx_flood_bboxes_dev(pfx_ctx* ctx, const void* dist_dev, uint32_t w, uint32_t h, int32_t boxes[1024])
{
    PFX_TRY(pfx_check_dims(ctx, "pfx_flood_bboxes_dev", w, h));
    PFX_TRY(pfx_check_args(ctx, "pfx_flood_bboxes_dev", true, {{dist_dev, (size_t)w * h, PFX_ARG_IN, "dist_dev"}, {boxes, 0, PFX_ARG_IN, "boxes"}}));
    PFX_TRY(pfx_reserve(ctx, ctx->d_misc, 4096));
    uint32_t per[1024];
    {
        pfx_timer t(ctx, "flood_bboxes");
        PFX_HIP(ctx, hipMemsetAsync(ctx->d_misc.p, 0, 4096, ctx->stream));
        PFX_HIP(ctx, pfxk_flood_bboxes(ctx->stream, (const uint8_t*)dist_dev, w, h, (uint32_t*)ctx->d_misc.p));
    }
    PFX_TRY(pfx_d2h(ctx, per, ctx->d_misc.p, sizeof per));
    PFX_TRY(pfx_sync(ctx));
    bool any = false;   // the prefix over t (state.rs:709-721)
    uint32_t x0 = 0, y0 = 0, x1 = 0, y1 = 0;
    for (int t = 0; t < 256; ++t) {
        if (per[t * 4] != 0u) {
            const uint32_t bx0 = ~per[t * 4], by0 = ~per[t * 4 + 1], bx1 = per[t * 4 + 2], by1 = per[t * 4 + 3];
            if (!any) { x0 = bx0; y0 = by0; x1 = bx1; y1 = by1; any = true; }
            else { x0 = std::min(x0, bx0); y0 = std::min(y0, by0); x1 = std::max(x1, bx1); y1 = std::max(y1, by1); }
        }
        boxes[t * 4] = any ? (int32_t)x0 : -1; boxes[t * 4 + 1] = any ? (int32_t)y0 : -1;
        boxes[t * 4 + 2] = any ? (int32_t)x1 : -1; boxes[t * 4 + 3] = any ? (int32_t)y1 : -1;
    }
    return PFX_OK;
}

int pfx_wand_mask_dev(pfx_ctx* ctx, const void* dist_dev, const void* base_mask_dev, uint32_t w, uint32_t h, uint8_t threshold, uint8_t anti_aliased,
                      uint8_t combine_mode, void* mask_out_dev)
{
    const size_t px = (size_t)w * h;
    PFX_TRY(check_threshold_call(ctx, dist_dev, base_mask_dev, mask_out_dev, 1, true, w, h, nullptr, "pfx_wand_mask_dev"));
    if (combine_mode > 3) return pfx_fail(ctx, PFX_ERR_INVALID, "pfx_wand_mask_dev: unknown combine mode %u", combine_mode);
    pfx_timer t(ctx, "wand_mask");
    PFX_HIP(ctx, pfxk_wand_mask(ctx->stream, (const uint8_t*)dist_dev, (const uint8_t*)base_mask_dev, (uint8_t*)mask_out_dev, px, threshold, anti_aliased != 0, combine_mode));
    return PFX_OK;
}

int pfx_wand_mask(pfx_ctx* ctx, const uint8_t* dist, const uint8_t* base_mask, uint32_t w, uint32_t h, uint8_t threshold, uint8_t anti_aliased, uint8_t combine_mode,
                  uint8_t* mask_out)
{
    const size_t px = (size_t)w * h;
    PFX_TRY(check_threshold_call(ctx, dist, base_mask, mask_out, 1, false, w, h, nullptr, "pfx_wand_mask"));
    if (combine_mode > 3) return pfx_fail(ctx, PFX_ERR_INVALID, "pfx_wand_mask: unknown combine mode %u", combine_mode);
    void *d_dist, *d_mask;
    PFX_TRY(pfx_stage(ctx, ctx->st_tmp, dist, px, &d_dist));
    PFX_TRY(pfx_stage(ctx, ctx->st_mask, base_mask, px, &d_mask));
    PFX_TRY(pfx_wand_mask_dev(ctx, d_dist, base_mask ? d_mask : nullptr, w, h, threshold, anti_aliased, combine_mode, d_mask));   // in place
    return pfx_unstage(ctx, mask_out, ctx->st_mask, px);
}

int pfx_fill_preview_dev(pfx_ctx* ctx, const void* dist_dev, const void* selection_dev, uint32_t w, uint32_t h, uint8_t threshold, const uint8_t fill[4],
                         void* canvas_out_dev)
{
    const size_t px = (size_t)w * h;
    PFX_TRY(check_threshold_call(ctx, dist_dev, selection_dev, canvas_out_dev, 4, true, w, h, fill, "pfx_fill_preview_dev"));
    pfx_timer t(ctx, "fill_preview");
    PFX_HIP(ctx, pfxk_fill_preview(ctx->stream, (const uint8_t*)dist_dev, (const uint8_t*)selection_dev, (uint8_t*)canvas_out_dev, px, threshold, pfx_pack_rgba8(fill)));
    return PFX_OK;
}

int pfx_fill_preview(pfx_ctx* ctx, const uint8_t* dist, const uint8_t* selection, uint32_t w, uint32_t h, uint8_t threshold, const uint8_t fill[4],
                     uint8_t* canvas_out)
{
    const size_t px = (size_t)w * h;
    PFX_TRY(check_threshold_call(ctx, dist, selection, canvas_out, 4, false, w, h, fill, "pfx_fill_preview"));
    void *d_dist, *d_out;
    const void* d_sel;
    PFX_TRY(pfx_stage(ctx, ctx->st_tmp, dist, px, &d_dist));
    PFX_TRY(pfx_stage_opt(ctx, ctx->st_mask, selection, px, &d_sel));
    PFX_TRY(pfx_stage(ctx, ctx->st_out, nullptr, px * 4, &d_out));
    PFX_TRY(pfx_fill_preview_dev(ctx, d_dist, d_sel, w, h, threshold, fill, d_out));
    return pfx_unstage(ctx, canvas_out, ctx->st_out, px * 4);
}

int pfx_fill_commit_dev(pfx_ctx* ctx, void* layer_dev, const void* dist_dev, const void* selection_dev, uint32_t w, uint32_t h, uint8_t threshold,
                        const uint8_t fill[4], uint8_t blend_mode)
{
    const size_t px = (size_t)w * h;
    PFX_TRY(check_threshold_call(ctx, dist_dev, selection_dev, layer_dev, 4, true, w, h, fill, "pfx_fill_commit_dev"));
    if (blend_mode > 24) return pfx_fail(ctx, PFX_ERR_INVALID, "pfx_fill_commit_dev: unknown blend mode %u", blend_mode);
    pfx_timer t(ctx, "fill_commit");
    PFX_HIP(ctx, pfxk_fill_commit(ctx->stream, (uint8_t*)layer_dev, (const uint8_t*)dist_dev, (const uint8_t*)selection_dev, px, threshold, pfx_pack_rgba8(fill), blend_mode));
    return PFX_OK;
}

int pfx_bucket_fill(pfx_ctx* ctx, uint8_t* layer_inout, uint32_t w, uint32_t h, uint32_t seed_x, uint32_t seed_y, float tolerance, const uint8_t fill[4],
                    uint8_t blend_mode, int global_fill, const uint8_t* selection)
{
    PFX_TRY(pfx_check_dims(ctx, "pfx_bucket_fill", w, h));
    const size_t px = (size_t)w * h;
    PFX_TRY(pfx_check_args(ctx, "pfx_bucket_fill", false, {{layer_inout, px * 4, PFX_ARG_OUT, "layer_inout"}, {selection, px, PFX_ARG_OPTIONAL, "selection"},
                                                            {fill, 0, PFX_ARG_IN, "fill"}}));
    if (seed_x >= w || seed_y >= h) return pfx_fail(ctx, PFX_ERR_INVALID, "pfx_bucket_fill: seed (%u, %u) outside the %ux%u image", seed_x, seed_y, w, h);
    if (blend_mode > 24) return pfx_fail(ctx, PFX_ERR_INVALID, "pfx_bucket_fill: unknown blend mode %u", blend_mode);
    pfx_flood f{};
    f.seed_x = seed_x; f.seed_y = seed_y;
    memcpy(f.target, layer_inout + ((size_t)seed_y * w + seed_x) * 4, 4);   // :1252
    f.distance_mode = 0; f.connectivity = 4; f.global = global_fill ? 1 : 0;   // :1272-1273
    void *d_layer, *d_dist;
    const void* d_sel;
    PFX_TRY(pfx_stage(ctx, ctx->st_in, layer_inout, px * 4, &d_layer));
    PFX_TRY(pfx_stage(ctx, ctx->st_tmp, nullptr, px, &d_dist));
    PFX_TRY(pfx_stage_opt(ctx, ctx->st_mask, selection, px, &d_sel));
    PFX_TRY(pfx_flood_distance_dev(ctx, d_layer, w, h, &f, d_dist));
    PFX_TRY(pfx_fill_commit_dev(ctx, d_layer, d_dist, d_sel, w, h, pfx_tolerance_threshold(tolerance), fill, blend_mode));
    return pfx_unstage(ctx, layer_inout, ctx->st_in, px * 4);
}

int pfx_int_flood_last(pfx_ctx* ctx, int which)
{
    if (!ctx) return -1;
    switch (which) {
        case 0: return pfx_sat_int(ctx->flood_passes);
        case 1: return pfx_sat_int(ctx->flood_launches);
        case 2: return PFXK_FLOOD_TILE;
        case 3: return pfx_sat_int(ctx->flood_visits);
        default: return -1;
    }
}

} // extern "C"
