// pfx_colorkey.cpp — C ABI of removal by colour (k_colorkey.hip).  Reference: src/ops/color_removal.rs — color_to_alpha_core :32, compute_color_removal :161,
// apply_color_removal :421; tools/state.rs:1723 ColorRemovalRequest.
// The host computes what is uniform over the image with the reference's own f32 expressions (no contraction): the dialog's prepared settings (:51-58) and the
// tool's tol_sq (:189).  The colour remover reads the clicked pixel (and its selection byte) back once — the reference's two no-ops and the seed colour hang on
// it — then launches: the passability map, the connected flood's passes (contiguous scope only; pfx_flood_converge, one 8-byte read-back per pass), and
// ceil(smoothness / 32) ring launches, the last of which writes dst (smoothness 0: one streaming launch).  All working memory is reserved before the first
// launch, and nothing but the last launch (or the no-op's copy) writes dst: a failed call leaves it untouched.
#include <cmath>

#include "pfx_internal.h"

namespace {

inline float clampf(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }   // f32::clamp for finite arguments

// what the four entry points share: dst == src (in place) is allowed, any other overlap of dst with src or the mask is refused
int check_images(pfx_ctx* ctx, const void* src, const void* dst, const void* mask, const void* params, uint32_t w, uint32_t h, bool dev, const char* who)
{
    PFX_TRY(pfx_check_dims(ctx, who, w, h));
    const size_t px = (size_t)w * h;
    return pfx_check_args(ctx, who, dev, {{src, px * 4, PFX_ARG_DWORD, "src"}, {dst, px * 4, PFX_ARG_OUT | PFX_ARG_DWORD, "dst"},
                                          {mask, px, PFX_ARG_OPTIONAL, "the mask"}, {params, 0, PFX_ARG_IN, "the settings"}}, src);
}

int check_settings(pfx_ctx* ctx, const pfx_color_to_alpha* s, const char* who)
{
    const float f[7] = {s->tolerance, s->softness, s->strength, s->spill_suppression, s->alpha_floor, s->alpha_ceiling, s->protect_luminance};
    for (float v : f)
        if (!std::isfinite(v)) return pfx_fail(ctx, PFX_ERR_INVALID, "%s: a setting is not finite", who);
    return PFX_OK;
}

pfxk_cta prepare_settings(const pfx_color_to_alpha* s)   // :46-58
{
    pfxk_cta S;
    for (int k = 0; k < 3; ++k) S.target[k] = (float)s->target[k];
    S.tolerance = clampf(s->tolerance / 255.0f, 0.0f, 1.0f);
    S.softness = std::fmax(s->softness / 255.0f, 0.001f);
    S.strength = clampf(s->strength, 0.0f, 1.0f);
    S.spill = clampf(s->spill_suppression, 0.0f, 1.0f);
    S.alpha_floor = clampf(s->alpha_floor, 0.0f, 1.0f);
    S.alpha_ceiling = clampf(s->alpha_ceiling, S.alpha_floor, 1.0f);
    S.protect = clampf(s->protect_luminance, 0.0f, 1.0f);
    S.target_luma = S.target[0] * 0.2126f + S.target[1] * 0.7152f + S.target[2] * 0.0722f;   // luma :139
    return S;
}

int check_request(pfx_ctx* ctx, const pfx_color_removal_req* r, uint32_t w, uint32_t h, const char* who)
{
    if (!std::isfinite(r->tolerance)) return pfx_fail(ctx, PFX_ERR_INVALID, "%s: the tolerance is not finite", who);
    if (r->contiguous > 1) return pfx_fail(ctx, PFX_ERR_INVALID, "%s: unknown scope %u", who, r->contiguous);
    if (r->seed_x >= w || r->seed_y >= h) return pfx_fail(ctx, PFX_ERR_INVALID, "%s: seed (%u, %u) outside the %ux%u image", who, r->seed_x, r->seed_y, w, h);
    if (r->smoothness > PFXK_COLORKEY_MAX_SMOOTHNESS)
        return pfx_fail(ctx, PFX_ERR_UNSUPPORTED, "%s: smoothness %u beyond the device path's %d", who, r->smoothness, PFXK_COLORKEY_MAX_SMOOTHNESS);
    return PFX_OK;
}

} // namespace

extern "C" {

int pfx_color_to_alpha_dev(pfx_ctx* ctx, const void* src_dev, void* dst_dev, uint32_t w, uint32_t h, const pfx_color_to_alpha* settings, const void* mask_dev)
{
    PFX_TRY(check_images(ctx, src_dev, dst_dev, mask_dev, settings, w, h, true, "pfx_color_to_alpha_dev"));
    PFX_TRY(check_settings(ctx, settings, "pfx_color_to_alpha_dev"));
    const pfxk_cta S = prepare_settings(settings);
    pfx_timer t(ctx, "color_to_alpha");
    PFX_HIP(ctx, pfxk_color_to_alpha(ctx->stream, (const uint8_t*)src_dev, (uint8_t*)dst_dev, (const uint8_t*)mask_dev, (size_t)w * h, &S));
    return PFX_OK;
}

int pfx_color_to_alpha_core(pfx_ctx* ctx, const uint8_t* src, uint8_t* dst, uint32_t w, uint32_t h, const pfx_color_to_alpha* settings, const uint8_t* mask)
{
    PFX_TRY(check_images(ctx, src, dst, mask, settings, w, h, false, "pfx_color_to_alpha_core"));
    PFX_TRY(check_settings(ctx, settings, "pfx_color_to_alpha_core"));
    const size_t px = (size_t)w * h;
    void* d_img;
    const void* d_mask;
    PFX_TRY(pfx_stage(ctx, ctx->st_in, src, px * 4, &d_img));
    PFX_TRY(pfx_stage_opt(ctx, ctx->st_mask, mask, px, &d_mask));
    PFX_TRY(pfx_color_to_alpha_dev(ctx, d_img, d_img, w, h, settings, d_mask));   // in place
    return pfx_unstage(ctx, dst, ctx->st_in, px * 4);
}

int pfx_color_removal_dev(pfx_ctx* ctx, const void* src_dev, void* dst_dev, uint32_t w, uint32_t h, const pfx_color_removal_req* req, const void* selection_dev)
{
    const char* who = "pfx_color_removal_dev";
    PFX_TRY(check_images(ctx, src_dev, dst_dev, selection_dev, req, w, h, true, who));
    PFX_TRY(check_request(ctx, req, w, h, who));
    const size_t px = (size_t)w * h;
    const uint32_t smooth = req->smoothness, chunk = PFXK_COLORKEY_CHUNK;
    const uint8_t* src = (const uint8_t*)src_dev;
    const uint8_t* sel = (const uint8_t*)selection_dev;
    ctx->colorkey_flood_passes = 0;
    ctx->colorkey_ring_launches = ctx->colorkey_launches = 0;
    // working memory: the flood's block (its c and d are the passability map and the core map) and, beyond one ring chunk, two u16 level maps
    pfx_flood_work W;
    PFX_TRY(pfx_flood_work_reserve(ctx, w, h, &W));
    uint16_t* levels[2] = {nullptr, nullptr};
    if (smooth > chunk) {
        PFX_TRY(pfx_reserve(ctx, ctx->colorkey_ws, 2 * pfx_align256(px * 2)));
        levels[0] = (uint16_t*)ctx->colorkey_ws.p;
        levels[1] = (uint16_t*)((uint8_t*)ctx->colorkey_ws.p + pfx_align256(px * 2));
    }
    // the click: the seed's pixel and its selection byte
    const size_t seed_at = (size_t)req->seed_y * w + req->seed_x;
    uint8_t seed[4] = {0, 0, 0, 0}, seed_sel = 255;
    PFX_TRY(pfx_d2h(ctx, seed, src + seed_at * 4, 4));
    if (sel) PFX_TRY(pfx_d2h(ctx, &seed_sel, sel + seed_at, 1));
    PFX_TRY(pfx_sync(ctx));
    if (seed_sel == 0 || seed[3] == 0) {   // :175-181, :185: the reference returns no changes
        if (dst_dev != src_dev) PFX_HIP(ctx, hipMemcpyAsync(dst_dev, src_dev, px * 4, hipMemcpyDeviceToDevice, ctx->stream));
        return PFX_OK;
    }
    pfxk_ckey P;
    for (int k = 0; k < 3; ++k) P.seed[k] = (float)seed[k];
    P.seed_rgb = (uint32_t)seed[0] | ((uint32_t)seed[1] << 8) | ((uint32_t)seed[2] << 16);
    const float tol = req->tolerance * 2.55f;   // :189
    P.tol_sq = tol * tol;
    P.smoothness = smooth;
    P.fade_den = (float)smooth + 1.0f;   // :376
    P.global = req->contiguous ? 0u : 1u;

    pfx_timer t(ctx, "color_removal");
    PFX_HIP(ctx, pfxk_ckey_passable(ctx->stream, src, sel, W.c, px, &P));
    ctx->colorkey_launches = 1;
    const uint8_t* core = W.c;   // the global scope: the map is the core
    if (req->contiguous) {       // the core is where the minimax distance over the 0 / 255 map is 0; the seed itself always passes (dist_sq 0)
        ctx->flood_passes = ctx->flood_launches = ctx->flood_visits = 0;
        PFX_TRY(pfx_flood_converge(ctx, &W, w, h, req->seed_x, req->seed_y, 4, who));
        ctx->colorkey_flood_passes = ctx->flood_passes;
        ctx->colorkey_launches += (uint32_t)pfx_sat_int(ctx->flood_launches);
        core = W.d;
    }
    if (smooth == 0) {
        PFX_HIP(ctx, pfxk_ckey_apply_core(ctx->stream, src, core, (uint8_t*)dst_dev, px, &P));
        ctx->colorkey_launches += 1;
        return PFX_OK;
    }
    for (uint32_t base = 0, n = 0; base < smooth; base += chunk, ++n) {
        const uint32_t k = smooth - base < chunk ? smooth - base : chunk;
        const bool last = base + k == smooth;
        PFX_HIP(ctx, pfxk_ckey_rings(ctx->stream, core, base ? levels[(n + 1) & 1] : nullptr, sel, last ? nullptr : levels[n & 1], src, (uint8_t*)dst_dev, w, h, base, k, &P));
        ctx->colorkey_ring_launches += 1;
        ctx->colorkey_launches += 1;
    }
    return PFX_OK;
}

int pfx_color_removal(pfx_ctx* ctx, const uint8_t* src, uint8_t* dst, uint32_t w, uint32_t h, const pfx_color_removal_req* req, const uint8_t* selection)
{
    PFX_TRY(check_images(ctx, src, dst, selection, req, w, h, false, "pfx_color_removal"));
    PFX_TRY(check_request(ctx, req, w, h, "pfx_color_removal"));
    const size_t px = (size_t)w * h;
    void* d_img;
    const void* d_sel;
    PFX_TRY(pfx_stage(ctx, ctx->st_in, src, px * 4, &d_img));
    PFX_TRY(pfx_stage_opt(ctx, ctx->st_mask, selection, px, &d_sel));
    PFX_TRY(pfx_color_removal_dev(ctx, d_img, d_img, w, h, req, d_sel));   // in place
    return pfx_unstage(ctx, dst, ctx->st_in, px * 4);
}

int pfx_int_colorkey_last(pfx_ctx* ctx, int which)
{
    if (!ctx) return -1;
    switch (which) {
        case 0: return pfx_sat_int(ctx->colorkey_flood_passes);
        case 1: return (int)ctx->colorkey_ring_launches;
        case 2: return PFXK_COLORKEY_TILE;
        case 3: return PFXK_COLORKEY_CHUNK;
        case 4: return (int)ctx->colorkey_launches;
        default: return -1;
    }
}

} // extern "C"
