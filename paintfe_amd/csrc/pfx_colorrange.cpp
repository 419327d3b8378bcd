// pfx_colorrange.cpp — C ABI of the colour dialogs' last pixel loops (k_colorrange.hip).  Reference: src/ops/adjustments.rs — compute_histogram :883,
// hue_saturation_per_band_from_flat :1635, select_color_range :1684.
// The host computes what is uniform over the image with the reference's own f32 expressions (no contraction): g_sat and g_light (:1644-1645) and each band's
// pixel-independent factors, the colour range's prepared values (:1705-1707) and its exponent.  Every refusal comes before the first launch, so a refused call
// leaves its outputs untouched.
#include <cmath>

#include "pfx_internal.h"

namespace {

inline float clampf(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }   // f32::clamp for finite arguments

int check_histogram(pfx_ctx* ctx, const void* image, const void* sel, const void* hist_out, uint32_t w, uint32_t h, bool dev, const char* who)
{
    PFX_TRY(pfx_check_dims(ctx, who, w, h));
    const size_t px = (size_t)w * h;
    return pfx_check_args(ctx, who, dev, {{image, px * 4, PFX_ARG_DWORD, "the image"}, {sel, px, PFX_ARG_OPTIONAL, "the mask"}, {hist_out, 0, PFX_ARG_IN, "hist_out"}});
}

// dst == src (in place) is allowed, any other overlap of the result with the image or the mask is refused
int check_bands(pfx_ctx* ctx, const void* image, const void* result, const void* sel, uint32_t w, uint32_t h, float global_hue, float global_sat, float global_light,
                const pfx_hue_band* bands, int sparse_mode, bool dev, const char* who)
{
    PFX_TRY(pfx_check_dims(ctx, who, w, h));
    const size_t px = (size_t)w * h;
    PFX_TRY(pfx_check_args(ctx, who, dev, {{image, px * 4, PFX_ARG_DWORD, "the image"}, {result, px * 4, PFX_ARG_OUT | PFX_ARG_DWORD, "the result"},
                                           {sel, px, PFX_ARG_OPTIONAL, "the mask"}, {bands, 0, PFX_ARG_IN, "bands"}}, image));
    if (sparse_mode < PFX_DENSE || sparse_mode > PFX_IN_PLACE) return pfx_fail(ctx, PFX_ERR_INVALID, "%s: unknown sparse mode %d", who, sparse_mode);
    bool finite = std::isfinite(global_hue) && std::isfinite(global_sat) && std::isfinite(global_light);
    for (int i = 0; i < 6; ++i) finite = finite && std::isfinite(bands[i].hue) && std::isfinite(bands[i].saturation) && std::isfinite(bands[i].lightness);
    if (!finite) return pfx_fail(ctx, PFX_ERR_INVALID, "%s: a slider value is not finite", who);
    return PFX_OK;
}

pfxk_hsl_bands prepare_bands(float global_hue, float global_sat, float global_light, const pfx_hue_band* bands)
{
    pfxk_hsl_bands B;
    B.g_hue = global_hue;
    B.g_sat = 1.0f + global_sat / 100.0f;          // :1644
    B.g_light = global_light * 255.0f / 100.0f;    // :1645
    for (int i = 0; i < 6; ++i) {                  // :1658-1660, the factors in front of `* w`
        B.hue[i] = bands[i].hue;
        B.sat[i] = bands[i].saturation / 100.0f;
        B.light[i] = bands[i].lightness * 255.0f / 100.0f;
    }
    return B;
}

// sel_out == base_sel (in place) is allowed, any other overlap of sel_out with the image or the base is refused
int check_range(pfx_ctx* ctx, const void* image, const void* base_sel, const void* sel_out, uint32_t w, uint32_t h, float hue_center_deg, float hue_tolerance_deg,
                float sat_min, float fuzziness, uint8_t combine_mode, bool dev, const char* who)
{
    PFX_TRY(pfx_check_dims(ctx, who, w, h));
    const size_t px = (size_t)w * h;
    PFX_TRY(pfx_check_args(ctx, who, dev, {{image, px * 4, PFX_ARG_DWORD, "the image"}, {base_sel, px, PFX_ARG_OPTIONAL, "the base mask"},
                                           {sel_out, px, PFX_ARG_OUT, "the output mask"}}, base_sel));
    if (combine_mode > 3) return pfx_fail(ctx, PFX_ERR_INVALID, "%s: unknown combine mode %u", who, combine_mode);
    if (!std::isfinite(hue_center_deg) || !std::isfinite(hue_tolerance_deg) || !std::isfinite(sat_min) || !std::isfinite(fuzziness))
        return pfx_fail(ctx, PFX_ERR_INVALID, "%s: a setting is not finite", who);
    if (hue_center_deg < 0.0f || hue_center_deg > 360.0f) return pfx_fail(ctx, PFX_ERR_INVALID, "%s: hue centre %g outside 0 .. 360", who, (double)hue_center_deg);
    return PFX_OK;
}

pfxk_color_range prepare_range(float hue_center_deg, float hue_tolerance_deg, float sat_min, float fuzziness, uint8_t combine_mode)
{
    pfxk_color_range R;
    R.hue_center = hue_center_deg / 360.0f;                      // :1705
    R.hue_tol = std::fmax(hue_tolerance_deg / 360.0f, 0.001f);   // :1706
    const float fuzz = clampf(fuzziness, 0.001f, 1.0f);          // :1707
    R.expo = 1.0f / std::fmax(fuzz, 0.01f);                      // :1734
    R.sat_min = sat_min;
    R.combine = combine_mode;
    return R;
}

} // namespace

extern "C" {

int pfx_histogram_dev(pfx_ctx* ctx, const void* image_dev, uint32_t w, uint32_t h, const void* sel_dev, uint32_t hist_out[1024])
{
    PFX_TRY(check_histogram(ctx, image_dev, sel_dev, hist_out, w, h, true, "pfx_histogram_dev"));
    PFX_TRY(pfx_reserve(ctx, ctx->d_misc, 4096));
    {
        pfx_timer t(ctx, "histogram");
        PFX_HIP(ctx, pfxk_histogram(ctx->stream, (const uint8_t*)image_dev, (const uint8_t*)sel_dev, (size_t)w * h, (uint32_t*)ctx->d_misc.p));
    }
    PFX_TRY(pfx_d2h(ctx, hist_out, ctx->d_misc.p, 1024 * sizeof(uint32_t)));
    return pfx_sync(ctx);
}

int pfx_histogram(pfx_ctx* ctx, const uint8_t* image, uint32_t w, uint32_t h, const uint8_t* sel, uint32_t hist_out[1024])
{
    PFX_TRY(check_histogram(ctx, image, sel, hist_out, w, h, false, "pfx_histogram"));
    const size_t px = (size_t)w * h;
    void* d_img;
    const void* d_sel;
    PFX_TRY(pfx_stage(ctx, ctx->st_in, image, px * 4, &d_img));
    PFX_TRY(pfx_stage_opt(ctx, ctx->st_mask, sel, px, &d_sel));
    return pfx_histogram_dev(ctx, d_img, w, h, d_sel, hist_out);
}

int pfx_hsl_bands_dev(pfx_ctx* ctx, const void* image_dev, void* result_dev, uint32_t w, uint32_t h, float global_hue, float global_sat, float global_light,
                      const pfx_hue_band bands[6], const void* sel_dev, int sparse_mode)
{
    PFX_TRY(check_bands(ctx, image_dev, result_dev, sel_dev, w, h, global_hue, global_sat, global_light, bands, sparse_mode, true, "pfx_hsl_bands_dev"));
    const pfxk_hsl_bands B = prepare_bands(global_hue, global_sat, global_light, bands);
    pfx_timer t(ctx, "hsl_bands");
    PFX_HIP(ctx, pfxk_hsl_bands_apply(ctx->stream, (const uint8_t*)image_dev, (uint8_t*)result_dev, (const uint8_t*)sel_dev, &B, sparse_mode, w, h));
    return PFX_OK;
}

int pfx_hsl_bands(pfx_ctx* ctx, const uint8_t* image, uint8_t* result, uint32_t w, uint32_t h, float global_hue, float global_sat, float global_light,
                  const pfx_hue_band bands[6], const uint8_t* sel, int sparse_mode)
{
    PFX_TRY(check_bands(ctx, image, result, sel, w, h, global_hue, global_sat, global_light, bands, sparse_mode, false, "pfx_hsl_bands"));
    const size_t px = (size_t)w * h;
    void* d_img;
    const void* d_sel;
    PFX_TRY(pfx_stage(ctx, ctx->st_in, image, px * 4, &d_img));
    PFX_TRY(pfx_stage_opt(ctx, ctx->st_mask, sel, px, &d_sel));
    PFX_TRY(pfx_hsl_bands_dev(ctx, d_img, d_img, w, h, global_hue, global_sat, global_light, bands, d_sel, sparse_mode));   // in place
    return pfx_unstage(ctx, result, ctx->st_in, px * 4);
}

int pfx_select_color_range_dev(pfx_ctx* ctx, const void* image_dev, const void* base_sel_dev, uint32_t w, uint32_t h, float hue_center_deg, float hue_tolerance_deg,
                               float sat_min, float fuzziness, uint8_t combine_mode, void* sel_out_dev)
{
    PFX_TRY(check_range(ctx, image_dev, base_sel_dev, sel_out_dev, w, h, hue_center_deg, hue_tolerance_deg, sat_min, fuzziness, combine_mode, true,
                        "pfx_select_color_range_dev"));
    const pfxk_color_range R = prepare_range(hue_center_deg, hue_tolerance_deg, sat_min, fuzziness, combine_mode);
    pfx_timer t(ctx, "color_range");
    PFX_HIP(ctx, pfxk_color_range_select(ctx->stream, (const uint8_t*)image_dev, (const uint8_t*)base_sel_dev, (uint8_t*)sel_out_dev, (size_t)w * h, &R));
    return PFX_OK;
}

int pfx_select_color_range(pfx_ctx* ctx, const uint8_t* image, const uint8_t* base_sel, uint32_t w, uint32_t h, float hue_center_deg, float hue_tolerance_deg,
                           float sat_min, float fuzziness, uint8_t combine_mode, uint8_t* sel_out)
{
    PFX_TRY(check_range(ctx, image, base_sel, sel_out, w, h, hue_center_deg, hue_tolerance_deg, sat_min, fuzziness, combine_mode, false, "pfx_select_color_range"));
    const size_t px = (size_t)w * h;
    void *d_img, *d_out;
    const void* d_base;
    PFX_TRY(pfx_stage(ctx, ctx->st_in, image, px * 4, &d_img));
    PFX_TRY(pfx_stage_opt(ctx, ctx->st_mask, base_sel, px, &d_base));
    PFX_TRY(pfx_stage(ctx, ctx->st_out, nullptr, px, &d_out));
    PFX_TRY(pfx_select_color_range_dev(ctx, d_img, d_base, w, h, hue_center_deg, hue_tolerance_deg, sat_min, fuzziness, combine_mode, d_out));
    return pfx_unstage(ctx, sel_out, ctx->st_out, px);
}

int pfx_int_colorrange_info(int which)
{
    switch (which) {
        case 0: return PFXK_HIST_MAX_BLOCKS;
        case 1: return PFXK_HIST_COPIES;
        default: return -1;
    }
}

} // extern "C"
