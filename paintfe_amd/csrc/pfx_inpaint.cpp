// pfx_inpaint.cpp — C ABI of content-aware fill (k_inpaint.hip).  Reference: src/ops/inpaint.rs — inpaint_instant_brush :76-192, fill_region_patchmatch :394-520.
// The host computes what is uniform over the image with the reference's own f32 expressions (no contraction): a dab's radius, hardness threshold and pixel loop
// bounds, the 32 ring offsets per distinct sample radius (pfx_inpaint_ring_offsets, glibc cosf / sinf).  For PatchMatch it runs the onion-peeling loop: one
// 4-byte read-back per peel (the boundary count) ends it, as does the reference's cap of (max(w, h) + 1) * 2 peels.
#include <algorithm>
#include <cmath>

#include "pfx_internal.h"

namespace {

inline float clamp01(float v) { return v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v); }

int check_instant(pfx_ctx* ctx, const void* src, const void* mask, const void* out, uint32_t w, uint32_t h, const pfx_inpaint_dab* dabs, uint32_t n_dabs,
                  const char* who)
{
    PFX_TRY(pfx_check_dims(ctx, who, w, h));
    const size_t px = (size_t)w * h;
    PFX_TRY(pfx_check_args(ctx, who, false, {{src, px * 4, PFX_ARG_IN, "src"}, {mask, px, PFX_ARG_IN, "hole_mask"}, {out, px * 4, PFX_ARG_OUT, "out"}}));
    if (n_dabs && !dabs) return pfx_fail(ctx, PFX_ERR_INVALID, "%s: null dab list", who);
    for (uint32_t i = 0; i < n_dabs; ++i) {
        const pfx_inpaint_dab& D = dabs[i];
        if (!std::isfinite(D.cx) || !std::isfinite(D.cy) || !std::isfinite(D.brush_radius) || !std::isfinite(D.sample_radius) || !std::isfinite(D.hardness))
            return pfx_fail(ctx, PFX_ERR_INVALID, "%s: non-finite field in dab %u", who, i);
    }
    return PFX_OK;
}

int check_patchmatch(pfx_ctx* ctx, const void* src, const void* mask, const void* dst, uint32_t w, uint32_t h, uint32_t patch_size, const char* who)
{
    PFX_TRY(pfx_check_dims(ctx, who, w, h));
    const size_t px = (size_t)w * h;
    PFX_TRY(pfx_check_args(ctx, who, false, {{src, px * 4, PFX_ARG_IN, "src"}, {mask, px, PFX_ARG_IN, "hole_mask"}, {dst, px * 4, PFX_ARG_OUT, "dst"}}, src));
    if (patch_size > 11) return pfx_fail(ctx, PFX_ERR_INVALID, "%s: patch size %u (the tool's range is 3..11)", who, patch_size);
    return PFX_OK;
}

} // namespace

extern "C" {

int pfx_inpaint_instant_dev(pfx_ctx* ctx, const void* src_dev, const void* hole_mask_dev, void* out_dev, uint32_t w, uint32_t h, const pfx_inpaint_dab* dabs,
                            uint32_t n_dabs)
{
    PFX_TRY(check_instant(ctx, src_dev, hole_mask_dev, out_dev, w, h, dabs, n_dabs, "pfx_inpaint_instant_dev"));
    if (n_dabs == 0) return PFX_OK;
    std::vector<pfxk_inpaint_dab> k(n_dabs);
    std::vector<float> rings;        // 64 floats per distinct sample radius
    std::vector<uint32_t> ring_key;  // its bit pattern
    uint32_t bx0 = w, by0 = h, bx1 = 0, by1 = 0;
    bool any = false;
    for (uint32_t i = 0; i < n_dabs; ++i) {
        const pfx_inpaint_dab& D = dabs[i];
        pfxk_inpaint_dab& K = k[i];
        K = pfxk_inpaint_dab{};
        K.cx = D.cx; K.cy = D.cy;
        K.r = fmaxf(D.brush_radius, 1.0f);
        K.hard_t = clamp01(D.hardness * 0.9f + 0.1f);
        K.soft_den = 1.0f - K.hard_t + 1e-6f;
        K.x0 = pfx_f32_as_u32(fmaxf(D.cx - K.r, 0.0f)); K.x1 = std::min(pfx_f32_as_u32(ceilf(D.cx + K.r)), w - 1u);   // :93-96
        K.y0 = pfx_f32_as_u32(fmaxf(D.cy - K.r, 0.0f)); K.y1 = std::min(pfx_f32_as_u32(ceilf(D.cy + K.r)), h - 1u);
        uint32_t key;
        memcpy(&key, &D.sample_radius, 4);
        size_t at = std::find(ring_key.begin(), ring_key.end(), key) - ring_key.begin();
        if (at == ring_key.size()) {
            ring_key.push_back(key);
            rings.resize(rings.size() + 64);
            pfx_inpaint_ring_offsets(D.sample_radius, &rings[at * 64]);
        }
        K.ring = (uint32_t)at;
        if (K.x0 <= K.x1 && K.y0 <= K.y1) {
            any = true;
            bx0 = std::min(bx0, K.x0); by0 = std::min(by0, K.y0); bx1 = std::max(bx1, K.x1); by1 = std::max(by1, K.y1);
        }
    }
    if (!any) return PFX_OK;   // every dab's pixel loop is empty
    const size_t dab_bytes = pfx_align256(k.size() * sizeof(pfxk_inpaint_dab));
    PFX_TRY(pfx_reserve(ctx, ctx->d_pts, dab_bytes + rings.size() * 4));
    PFX_TRY(pfx_h2d(ctx, ctx->d_pts.p, k.data(), k.size() * sizeof(pfxk_inpaint_dab)));
    PFX_TRY(pfx_h2d(ctx, (uint8_t*)ctx->d_pts.p + dab_bytes, rings.data(), rings.size() * 4));
    PFX_HIP(ctx, hipStreamSynchronize(ctx->stream));   // `k` / `rings` are pageable host memory about to go out of scope
    pfx_timer t(ctx, "inpaint_instant");
    PFX_HIP(ctx, pfxk_inpaint_instant(ctx->stream, (const uint8_t*)src_dev, (const uint8_t*)hole_mask_dev, (uint8_t*)out_dev, w, h, (const pfxk_inpaint_dab*)ctx->d_pts.p,
                                      n_dabs, (const float*)((const uint8_t*)ctx->d_pts.p + dab_bytes), bx0, by0, bx1, by1));
    return PFX_OK;
}

int pfx_inpaint_instant(pfx_ctx* ctx, const uint8_t* src, const uint8_t* hole_mask, uint8_t* out_inout, uint32_t w, uint32_t h, const pfx_inpaint_dab* dabs,
                        uint32_t n_dabs)
{
    PFX_TRY(check_instant(ctx, src, hole_mask, out_inout, w, h, dabs, n_dabs, "pfx_inpaint_instant"));
    if (n_dabs == 0) return PFX_OK;
    const size_t px = (size_t)w * h;
    void *d_src, *d_mask, *d_out;
    PFX_TRY(pfx_stage(ctx, ctx->st_in, src, px * 4, &d_src));
    PFX_TRY(pfx_stage(ctx, ctx->st_mask, hole_mask, px, &d_mask));
    PFX_TRY(pfx_stage(ctx, ctx->st_out, out_inout, px * 4, &d_out));
    PFX_TRY(pfx_inpaint_instant_dev(ctx, d_src, d_mask, d_out, w, h, dabs, n_dabs));
    return pfx_unstage(ctx, out_inout, ctx->st_out, px * 4);
}

int pfx_inpaint_patchmatch_dev(pfx_ctx* ctx, const void* src_dev, const void* hole_mask_dev, void* dst_dev, uint32_t w, uint32_t h, uint32_t patch_size,
                               uint32_t iterations)
{
    PFX_TRY(check_patchmatch(ctx, src_dev, hole_mask_dev, dst_dev, w, h, patch_size, "pfx_inpaint_patchmatch_dev"));
    const size_t px = (size_t)w * h;
    ctx->inpaint_peels = ctx->inpaint_launches = 0;
    // the hole's bounding box and size
    PFX_TRY(pfx_reserve(ctx, ctx->inpaint_ws, 256));
    uint32_t stats[8];
    {
        pfx_timer t(ctx, "inpaint_patchmatch_stats");
        PFX_HIP(ctx, pfxk_pm_stats(ctx->stream, (const uint8_t*)hole_mask_dev, w, h, (uint32_t*)ctx->inpaint_ws.p));
    }
    PFX_TRY(pfx_d2h(ctx, stats, ctx->inpaint_ws.p, sizeof stats));
    PFX_TRY(pfx_sync(ctx));
    ctx->inpaint_launches += 1;
    const uint32_t holes = stats[4];
    if (holes == 0 || holes == px) {   // nothing to fill / nothing to fill from (:419): a copy of src
        if (dst_dev != src_dev) PFX_HIP(ctx, hipMemcpyAsync(dst_dev, src_dev, px * 4, hipMemcpyDeviceToDevice, ctx->stream));
        return PFX_OK;
    }
    pfxk_pm_geom G;
    G.w = w; G.h = h;
    G.x0 = ~stats[0]; G.y0 = ~stats[1]; G.bw = stats[2] - G.x0 + 1u; G.bh = stats[3] - G.y0 + 1u;
    const uint32_t ps = std::max(patch_size, 3u);
    G.half = ps / 2u;
    G.min_valid = std::max((G.half * 2u + 1u) * (G.half * 2u + 1u), 4u) / 4u;
    G.max_radius = (float)std::max(w, h);
    const int pm_iters = iterations <= 3 ? 2 : 4;
    // working memory, one block: [0] 256 bytes of counters | live mask | source list (w * h indices: the non-hole pixels, then every peel's boundary) |
    // compaction block counts | NNF ox, oy, ssd over the box plus one | diagonal starts, cursors, list
    const size_t nnf = (size_t)(G.bw + 2u) * (G.bh + 2u), n_diag = (size_t)G.bw + G.bh - 1u, blocks = (px + 1023u) / 1024u;
    const size_t off_live = 256, off_list = off_live + pfx_align256(px), off_counts = off_list + pfx_align256(px * 4), off_ox = off_counts + pfx_align256(blocks * 4),
                 off_oy = off_ox + pfx_align256(nnf * 4), off_sd = off_oy + pfx_align256(nnf * 4), off_dstart = off_sd + pfx_align256(nnf * 4),
                 off_cursor = off_dstart + pfx_align256((n_diag + 1) * 4), off_dlist = off_cursor + pfx_align256(n_diag * 4), total = off_dlist + pfx_align256((size_t)holes * 4);
    PFX_TRY(pfx_reserve(ctx, ctx->inpaint_ws, total));   // a failure leaves dst untouched
    uint8_t* ws = (uint8_t*)ctx->inpaint_ws.p;
    uint32_t* d_total = (uint32_t*)ws;
    uint8_t* live = ws + off_live;
    uint32_t* list = (uint32_t*)(ws + off_list);
    uint32_t* counts = (uint32_t*)(ws + off_counts);
    pfx_timer t(ctx, "inpaint_patchmatch");
    if (dst_dev != src_dev) PFX_HIP(ctx, hipMemcpyAsync(dst_dev, src_dev, px * 4, hipMemcpyDeviceToDevice, ctx->stream));
    PFX_HIP(ctx, hipMemcpyAsync(live, hole_mask_dev, px, hipMemcpyDeviceToDevice, ctx->stream));
    PFX_HIP(ctx, pfxk_pm_compact(ctx->stream, 0, live, w, h, 0, 0, w, h, counts, d_total, list, 0));
    PFX_HIP(ctx, pfxk_pm_compact(ctx->stream, 0, live, w, h, 0, 0, w, h, counts, d_total, list, 1));
    PFX_HIP(ctx, pfxk_pm_nnf_reset(ctx->stream, &G, (float*)(ws + off_sd)));
    ctx->inpaint_launches += 4;
    uint32_t src_count = (uint32_t)(px - holes);
    const uint64_t max_peels = ((uint64_t)std::max(w, h) + 1u) * 2u;
    for (uint64_t peel = 0; peel < max_peels; ++peel) {
        uint32_t nb = 0;
        PFX_HIP(ctx, pfxk_pm_compact(ctx->stream, 1, live, w, h, G.x0, G.y0, G.bw, G.bh, counts, d_total, list + src_count, 0));
        PFX_TRY(pfx_d2h(ctx, &nb, d_total, 4));
        PFX_TRY(pfx_sync(ctx));
        ctx->inpaint_launches += 2;
        if (nb == 0) break;
        if ((uint64_t)src_count + nb > px) return pfx_fail(ctx, PFX_ERR_HIP, "pfx_inpaint_patchmatch_dev: boundary list overruns the hole");   // cannot happen: a pixel is boundary once
        PFX_HIP(ctx, pfxk_pm_compact(ctx->stream, 1, live, w, h, G.x0, G.y0, G.bw, G.bh, counts, d_total, list + src_count, 1));
        PFX_HIP(ctx, pfxk_pm_peel(ctx->stream, &G, (uint8_t*)dst_dev, live, list, src_count, nb, pm_iters, (int32_t*)(ws + off_ox), (int32_t*)(ws + off_oy),
                                  (float*)(ws + off_sd), (uint32_t*)(ws + off_dstart), (uint32_t*)(ws + off_cursor), (uint32_t*)(ws + off_dlist)));
        ctx->inpaint_launches += 5 + pm_iters;
        ctx->inpaint_peels += 1;
        src_count += nb;
    }
    return PFX_OK;
}

int pfx_inpaint_patchmatch(pfx_ctx* ctx, const uint8_t* src, const uint8_t* hole_mask, uint8_t* dst, uint32_t w, uint32_t h, uint32_t patch_size,
                           uint32_t iterations)
{
    PFX_TRY(check_patchmatch(ctx, src, hole_mask, dst, w, h, patch_size, "pfx_inpaint_patchmatch"));
    const size_t px = (size_t)w * h;
    void *d_img, *d_mask;
    PFX_TRY(pfx_stage(ctx, ctx->st_in, src, px * 4, &d_img));
    PFX_TRY(pfx_stage(ctx, ctx->st_mask, hole_mask, px, &d_mask));
    PFX_TRY(pfx_inpaint_patchmatch_dev(ctx, d_img, d_mask, d_img, w, h, patch_size, iterations));   // in place in the staging copy
    return pfx_unstage(ctx, dst, ctx->st_in, px * 4);
}

int pfx_int_inpaint_last(pfx_ctx* ctx, int which) { return !ctx ? -1 : (which == 0 ? (int)ctx->inpaint_peels : (int)ctx->inpaint_launches); }

} // extern "C"
