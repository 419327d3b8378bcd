// pfx_matte.cpp — C ABI of background removal around the model (k_matte.hip).  Reference: src/ops/ai.rs — preprocess_image :731, is_probability_space :675,
// to_probability :693, mask_confidence_score :706, ModelProfile :621-669, the output selection :1356-1380, postprocess_mask :766, apply_mask_expansion :850,
// morphological_close :904, blur_grayscale :913.  The model runs in the caller's process; these are the pixel loops in front of it and behind it.
// The host computes what is uniform over a call with the reference's own expressions (no contraction): the normalisation table, the sampling step, the
// probability-space verdict from the sampled minimum / maximum, the feather's radius, the resize tables (pfx_resample.h).  Every refusal comes before the first
// launch, so a refused call leaves its outputs untouched.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "pfx_internal.h"
#include "pfx_resample.h"

namespace {

constexpr int32_t MAX_EXPANSION = 64;   // |mask_expansion| and fill_holes; the dialog's sliders stop at 10 and 20 (ui/dialogs/effects/ai.rs)

// IMAGENET_MEAN / IMAGENET_STD :722-723; entry [c][k] = ((k as f32 / 255.0) - MEAN[c]) / STD[c] :747-750
const float* tensor_table()
{
    static float table[768];
    static const bool built = [] {
        const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};
        for (int c = 0; c < 3; ++c)
            for (int k = 0; k < 256; ++k) table[c * 256 + k] = ((float)k / 255.0f - mean[c]) / stdv[c];
        return true;
    }();
    (void)built;
    return table;
}

int check_settings(pfx_ctx* ctx, const char* who, const pfx_matte_settings* S)
{
    if (!std::isfinite(S->threshold) || !std::isfinite(S->edge_feather)) return pfx_fail(ctx, PFX_ERR_INVALID, "%s: a setting is not finite", who);
    return PFX_OK;
}
int check_is_probability(pfx_ctx* ctx, const char* who, int32_t is_probability)
{
    if (is_probability < -1 || is_probability > 1) return pfx_fail(ctx, PFX_ERR_INVALID, "%s: is_probability %d outside -1 .. 1", who, is_probability);
    return PFX_OK;
}
int check_expansion(pfx_ctx* ctx, const char* who, int64_t expansion, const char* name)
{
    if (expansion > MAX_EXPANSION || expansion < -MAX_EXPANSION) return pfx_fail(ctx, PFX_ERR_UNSUPPORTED, "%s: %s %lld beyond %d", who, name, (long long)expansion, MAX_EXPANSION);
    return PFX_OK;
}
// blur_grayscale's radius :915: 0 = no feather (:828); PFX_ERR_UNSUPPORTED beyond the kernels' cap
int feather_radius(pfx_ctx* ctx, const char* who, float edge_feather, uint32_t* r)
{
    *r = 0;
    if (!(edge_feather > 0.5f)) return PFX_OK;
    const float c = ceilf(edge_feather);
    if (c > (float)PFXK_MATTE_MAX_FEATHER) return pfx_fail(ctx, PFX_ERR_UNSUPPORTED, "%s: edge_feather %g beyond %d", who, (double)edge_feather, PFXK_MATTE_MAX_FEATHER);
    *r = std::max<uint32_t>((uint32_t)c, 1u);
    return PFX_OK;
}
// the column pass's band: tall enough that a band's 2 r + 1 start-up reads stay a bounded share of its rows
uint32_t feather_band(uint32_t r) { return std::max<uint32_t>(64u, 4u * r); }

struct score_result { int32_t is_prob; double confidence; };
// the one launch behind pfx_matte_score[_dev] and behind is_probability = -1; waits for its 16 bytes
int run_score(pfx_ctx* ctx, const void* values_dev, size_t n, score_result* out)
{
    out->is_prob = 0;
    out->confidence = 0.0;
    if (n == 0) return PFX_OK;   // :676, :707
    PFX_TRY(pfx_reserve(ctx, ctx->d_misc, 4096));
    const uint32_t step = (uint32_t)std::max<size_t>(n / 10000u, 1u);   // :680
    PFX_HIP(ctx, pfxk_matte_score(ctx->stream, (const float*)values_dev, (uint32_t)n, step, (uint32_t*)ctx->d_misc.p));
    uint32_t r[4];
    PFX_TRY(pfx_d2h(ctx, r, ctx->d_misc.p, sizeof r));
    PFX_TRY(pfx_sync(ctx));
    auto unkey = [](uint32_t k) { const uint32_t b = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k; float f; std::memcpy(&f, &b, 4); return f; };
    const float mn = unkey(r[0]), mx = unkey(r[1]);
    out->is_prob = (mn >= -0.05f && mx <= 1.05f) ? 1 : 0;   // :688, f32 against f32 literals
    out->confidence = (double)(out->is_prob ? r[2] : r[3]) / (double)n;   // :718
    return PFX_OK;
}

int check_score(pfx_ctx* ctx, const char* who, bool dev, const void* values, size_t n, const void* is_probability, const void* confidence)
{
    if (!ctx) return PFX_ERR_INVALID;
    if (n > 256000000ull) return pfx_fail(ctx, PFX_ERR_INVALID, "%s: %zu values (at most 256 M)", who, n);
    return pfx_check_args(ctx, who, dev, {{values, std::max<size_t>(n * 4, 1), PFX_ARG_DWORD, "the values"}, {is_probability, 0, PFX_ARG_IN, "is_probability"},
                                          {confidence, 0, PFX_ARG_IN, "confidence"}});
}

// ---- the stages on plain device pointers: arguments are the caller's to check ----
int run_byte(pfx_ctx* ctx, const void* values, uint32_t pw, uint32_t ph, int32_t is_probability, const pfx_matte_settings* S, void* grey)
{
    const size_t n = (size_t)pw * ph;
    if (is_probability < 0) {   // :1402
        score_result sc;
        PFX_TRY(run_score(ctx, values, n, &sc));
        is_probability = sc.is_prob;
    }
    PFX_HIP(ctx, pfxk_matte_byte(ctx->stream, (const float*)values, (uint8_t*)grey, n, is_probability, S->smooth_edges != 0, S->threshold));
    return PFX_OK;
}

// |expansion| iterations in ceil(|expansion| / K) launches: src -> (tmp0 -> tmp1 -> ..) -> dst; 0 copies
int run_expand(pfx_ctx* ctx, const void* src, void* dst, uint32_t pw, uint32_t ph, int32_t expansion, void* tmp0, void* tmp1)
{
    const size_t n = (size_t)pw * ph;
    if (expansion == 0) {
        if (src != dst) PFX_HIP(ctx, hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToDevice, ctx->stream));
        return PFX_OK;
    }
    uint32_t left = (uint32_t)std::abs(expansion);
    const uint32_t launches = (left + PFXK_MATTE_K - 1u) / PFXK_MATTE_K;
    const void* from = src;
    for (uint32_t i = 0; i < launches; ++i) {
        void* to = i + 1 == launches ? dst : ((i & 1u) ? tmp1 : tmp0);
        const uint32_t iters = std::min<uint32_t>(left, PFXK_MATTE_K);
        PFX_HIP(ctx, pfxk_matte_morph(ctx->stream, (const uint8_t*)from, (uint8_t*)to, pw, ph, iters, expansion > 0));
        left -= iters;
        from = to;
    }
    return PFX_OK;
}

// the one-channel resize in two steps, so that the host's table work stays in front of a timed launch sequence: the tables of a pw x ph -> w x h resize, then
// the launch with its optional epilogue.  Sizes differ (an equal size is the caller's copy).  The tables live in a buffer of their own and are kept for the next
// call of the same four sizes: a dialog re-runs the post-process on every settings change, and building them (sinf per tap) costs the host more than the kernels
// cost the device (profiles/matte.md)
int prepare_resize(pfx_ctx* ctx, const char* who, uint32_t pw, uint32_t ph, uint32_t w, uint32_t h, pfx_matte_axes** plan)
{
    pfx_matte_axes& A = ctx->matte_axes;
    *plan = &A;
    if (A.valid && A.pw == pw && A.ph == ph && A.w == w && A.h == h) return PFX_OK;
    pfx_resample::AxisTable v, hz;
    pfx_resample::build_axis(ph, h, PFX_RESIZE_LANCZOS3, v);
    pfx_resample::build_axis(pw, w, PFX_RESIZE_LANCZOS3, hz);
    const uint32_t span_max = pfx_resample::span_max(hz, w, PFXK_MATTE_RZ_TOX);
    if (span_max > PFXK_MATTE_RZ_MAX_SPAN)
        return pfx_fail(ctx, PFX_ERR_UNSUPPORTED, "%s: a %u-column output tile reaches %u source columns (at most %u)", who, PFXK_MATTE_RZ_TOX, span_max, PFXK_MATTE_RZ_MAX_SPAN);
    if (v.wts.size() >= 0xffffffffull || hz.wts.size() >= 0xffffffffull) return pfx_fail(ctx, PFX_ERR_INVALID, "%s: weight table too large", who);
    std::vector<uint32_t> blob;
    const size_t n_u32 = pfx_resample::pack_axes(v, hz, blob);
    A.valid = false;
    PFX_TRY(pfx_reserve(ctx, A.buf, blob.size() * 4));
    PFX_TRY(pfx_h2d(ctx, A.buf.p, blob.data(), blob.size() * 4));
    PFX_HIP(ctx, hipStreamSynchronize(ctx->stream)); // `blob` is pageable host memory about to go out of scope
    A.pw = pw; A.ph = ph; A.w = w; A.h = h;
    A.n_u32 = n_u32; A.v_wts = v.wts.size(); A.span_max = span_max;
    A.valid = true;
    return PFX_OK;
}
int launch_resize(pfx_ctx* ctx, const pfx_matte_axes* A, const void* grey, void* matte, const void* image, void* result)
{
    const uint32_t* d = (const uint32_t*)A->buf.p;
    const float* wts = (const float*)(d + A->n_u32);
    const size_t w = A->w, h = A->h;
    PFX_HIP(ctx, pfxk_matte_resize(ctx->stream, (const uint8_t*)grey, d, d + h, d + 2 * h, wts, d + 3 * h, d + 3 * h + w, d + 3 * h + 2 * w, wts + A->v_wts, A->pw, A->w, A->h,
                                   A->span_max, (uint8_t*)matte, (const uint8_t*)image, (uint8_t*)result));
    return PFX_OK;
}

// working memory: planes of `bytes` each, 256-byte aligned, carved from ctx->matte_ws
int reserve_planes(pfx_ctx* ctx, std::initializer_list<size_t> bytes, uint8_t** out)
{
    size_t total = 0;
    for (size_t b : bytes) total += pfx_align256(b);
    PFX_TRY(pfx_reserve(ctx, ctx->matte_ws, total));
    size_t at = 0;
    for (size_t b : bytes) { *out++ = (uint8_t*)ctx->matte_ws.p + at; at += pfx_align256(b); }
    return PFX_OK;
}

int check_postprocess(pfx_ctx* ctx, const char* who, bool dev, const void* values, uint32_t pw, uint32_t ph, int32_t is_probability, const void* image, uint32_t w, uint32_t h,
                      const pfx_matte_settings* S, const void* result, const void* matte, uint32_t* r)
{
    PFX_TRY(pfx_check_dims(ctx, who, pw, ph));
    PFX_TRY(pfx_check_dims(ctx, who, w, h));
    const size_t pn = (size_t)pw * ph, n = (size_t)w * h;
    const int out = dev ? PFX_ARG_OUT : PFX_ARG_STAGED_OUT;
    PFX_TRY(pfx_check_args(ctx, who, dev, {{values, pn * 4, PFX_ARG_DWORD, "the values"}, {image, n * 4, PFX_ARG_DWORD, "the image"}, {S, 0, PFX_ARG_IN, "settings"},
                                           {result, n * 4, out | PFX_ARG_DWORD, "the result"}, {matte, n, out | PFX_ARG_OPTIONAL, "the matte"}}, image));
    PFX_TRY(check_is_probability(ctx, who, is_probability));
    PFX_TRY(check_settings(ctx, who, S));
    PFX_TRY(check_expansion(ctx, who, S->mask_expansion, "mask_expansion"));
    PFX_TRY(check_expansion(ctx, who, (int64_t)S->fill_holes, "fill_holes"));
    return feather_radius(ctx, who, S->edge_feather, r);
}

} // namespace

extern "C" {

int pfx_int_matte_info(int which)
{
    switch (which) {
        case 0: return PFXK_MATTE_TILE;
        case 1: return PFXK_MATTE_K;
        case 2: return PFXK_MATTE_RZ_TOX;
        case 3: return PFXK_MATTE_RZ_TOY;
        case 4: return PFXK_MATTE_BOX_CHUNK;
        case 5: return PFXK_MATTE_BOX_COLS;
        case 6: return PFXK_MATTE_RZ_MAX_SPAN;
        case 7: return PFXK_MATTE_RZ_TALL_SPAN;
        case 8: return PFXK_MATTE_RZ_TOY_WIDE;
        default: return -1;
    }
}

int pfx_matte_tensor_dev(pfx_ctx* ctx, const void* image_dev, uint32_t w, uint32_t h, uint32_t tensor_size, void* tensor_dev)
{
    const char* who = "pfx_matte_tensor_dev";
    PFX_TRY(pfx_check_dims(ctx, who, w, h));
    if (!pfx_dims_ok(tensor_size, tensor_size)) return pfx_fail(ctx, PFX_ERR_INVALID, "%s: bad tensor size %u", who, tensor_size);
    const size_t n = (size_t)tensor_size * tensor_size;
    PFX_TRY(pfx_check_args(ctx, who, true, {{image_dev, pfx_img_bytes(w, h), PFX_ARG_DWORD, "the image"}, {tensor_dev, n * 12, PFX_ARG_OUT | PFX_ARG_DWORD, "the tensor"}}));
    if (!ctx->matte_tab_valid) {
        PFX_TRY(pfx_reserve(ctx, ctx->matte_tab, 768 * sizeof(float)));
        PFX_TRY(pfx_h2d(ctx, ctx->matte_tab.p, tensor_table(), 768 * sizeof(float)));   // a static table: it outlives the copy
        ctx->matte_tab_valid = true;
    }
    const void* rgba = image_dev;
    if (w != tensor_size || h != tensor_size) {   // at the model's own size imageops::resize copies, and the table reads the image itself
        uint8_t* scaled;
        PFX_TRY(reserve_planes(ctx, {n * 4}, &scaled));
        PFX_TRY(pfx_resize_image_dev(ctx, image_dev, w, h, scaled, tensor_size, tensor_size, PFX_RESIZE_LANCZOS3));
        rgba = scaled;
    }
    pfx_timer t(ctx, "matte_tensor");
    PFX_HIP(ctx, pfxk_matte_tensor(ctx->stream, (const uint8_t*)rgba, (const float*)ctx->matte_tab.p, (float*)tensor_dev, n));
    return PFX_OK;
}

int pfx_matte_tensor(pfx_ctx* ctx, const uint8_t* image, uint32_t w, uint32_t h, uint32_t tensor_size, float* tensor)
{
    const char* who = "pfx_matte_tensor";
    PFX_TRY(pfx_check_dims(ctx, who, w, h));
    if (!pfx_dims_ok(tensor_size, tensor_size)) return pfx_fail(ctx, PFX_ERR_INVALID, "%s: bad tensor size %u", who, tensor_size);
    const size_t n = (size_t)tensor_size * tensor_size;
    PFX_TRY(pfx_check_args(ctx, who, false, {{image, pfx_img_bytes(w, h), PFX_ARG_IN, "the image"}, {tensor, n * 12, PFX_ARG_STAGED_OUT, "the tensor"}}));
    void *d_img, *d_out;
    PFX_TRY(pfx_stage(ctx, ctx->st_in, image, pfx_img_bytes(w, h), &d_img));
    PFX_TRY(pfx_stage(ctx, ctx->st_out, nullptr, n * 12, &d_out));
    PFX_TRY(pfx_matte_tensor_dev(ctx, d_img, w, h, tensor_size, d_out));
    return pfx_unstage(ctx, tensor, ctx->st_out, n * 12);
}

int pfx_matte_score_dev(pfx_ctx* ctx, const void* values_dev, size_t n_values, int32_t* is_probability, double* confidence)
{
    PFX_TRY(check_score(ctx, "pfx_matte_score_dev", true, values_dev, n_values, is_probability, confidence));
    score_result sc;
    {
        pfx_timer t(ctx, "matte_score");
        PFX_TRY(run_score(ctx, values_dev, n_values, &sc));
    }
    *is_probability = sc.is_prob;
    *confidence = sc.confidence;
    return PFX_OK;
}

int pfx_matte_score(pfx_ctx* ctx, const float* values, size_t n_values, int32_t* is_probability, double* confidence)
{
    PFX_TRY(check_score(ctx, "pfx_matte_score", false, values, n_values, is_probability, confidence));
    void* d_values;
    PFX_TRY(pfx_stage(ctx, ctx->st_aux, values, n_values * 4, &d_values));
    return pfx_matte_score_dev(ctx, d_values, n_values, is_probability, confidence);
}

int pfx_matte_pick_output(uint32_t input_w, uint32_t input_h, const double* confidence, uint32_t n_outputs, uint32_t* picked)
{
    if (!confidence || !picked || n_outputs == 0) return PFX_ERR_INVALID;
    // ModelProfile::detect :634 and preferred_output_index :661: U2-Net (320 x 320), IS-Net and unknown models prefer the first output, BiRefNet (1024 x 1024 with
    // five or more outputs) the last
    const bool birefnet = input_h == 1024 && input_w == 1024 && n_outputs >= 5;
    const uint32_t preferred = birefnet ? n_outputs - 1 : 0;
    auto usable = [&](uint32_t i) { return confidence[i] >= 0.0; };   // a negative (or NaN) confidence: an output the caller could not read
    double best = 0.0;   // fold(0.0, f64::max) :1365
    bool any = false;
    for (uint32_t i = 0; i < n_outputs; ++i)
        if (usable(i)) { any = true; best = std::max(best, confidence[i]); }
    if (!any) return PFX_ERR_INVALID;   // "No valid outputs found" :1358
    const double close = best - 0.01;
    if (usable(preferred) && confidence[preferred] >= close) { *picked = preferred; return PFX_OK; }
    uint32_t at = 0;
    bool have = false;
    for (uint32_t i = 0; i < n_outputs; ++i)   // max_by keeps the last of equal maxima :1377
        if (usable(i) && confidence[i] >= close && (!have || confidence[i] >= confidence[at])) { at = i; have = true; }
    *picked = at;
    return PFX_OK;
}

int pfx_matte_byte_dev(pfx_ctx* ctx, const void* values_dev, uint32_t prob_w, uint32_t prob_h, int32_t is_probability, const pfx_matte_settings* settings, void* grey_dev)
{
    const char* who = "pfx_matte_byte_dev";
    PFX_TRY(pfx_check_dims(ctx, who, prob_w, prob_h));
    const size_t n = (size_t)prob_w * prob_h;
    PFX_TRY(pfx_check_args(ctx, who, true, {{values_dev, n * 4, PFX_ARG_DWORD, "the values"}, {settings, 0, PFX_ARG_IN, "settings"}, {grey_dev, n, PFX_ARG_OUT, "the grey image"}}));
    PFX_TRY(check_is_probability(ctx, who, is_probability));
    PFX_TRY(check_settings(ctx, who, settings));
    pfx_timer t(ctx, "matte_byte");
    return run_byte(ctx, values_dev, prob_w, prob_h, is_probability, settings, grey_dev);
}

int pfx_matte_expand_dev(pfx_ctx* ctx, const void* grey_dev, uint32_t prob_w, uint32_t prob_h, int32_t expansion, void* grey_out_dev)
{
    const char* who = "pfx_matte_expand_dev";
    PFX_TRY(pfx_check_dims(ctx, who, prob_w, prob_h));
    const size_t n = (size_t)prob_w * prob_h;
    PFX_TRY(pfx_check_args(ctx, who, true, {{grey_dev, n, PFX_ARG_IN, "the grey image"}, {grey_out_dev, n, PFX_ARG_OUT, "the grey output"}}));
    PFX_TRY(check_expansion(ctx, who, expansion, "expansion"));
    uint8_t* tmp[2];
    PFX_TRY(reserve_planes(ctx, {n, n}, tmp));
    pfx_timer t(ctx, "matte_expand");
    return run_expand(ctx, grey_dev, grey_out_dev, prob_w, prob_h, expansion, tmp[0], tmp[1]);
}

int pfx_matte_resize_dev(pfx_ctx* ctx, const void* grey_dev, uint32_t prob_w, uint32_t prob_h, void* matte_dev, uint32_t w, uint32_t h)
{
    const char* who = "pfx_matte_resize_dev";
    PFX_TRY(pfx_check_dims(ctx, who, prob_w, prob_h));
    PFX_TRY(pfx_check_dims(ctx, who, w, h));
    PFX_TRY(pfx_check_args(ctx, who, true, {{grey_dev, (size_t)prob_w * prob_h, PFX_ARG_IN, "the grey image"}, {matte_dev, (size_t)w * h, PFX_ARG_OUT, "the matte"}}));
    const bool resize = prob_w != w || prob_h != h;   // :816
    pfx_matte_axes* A = nullptr;
    if (resize) PFX_TRY(prepare_resize(ctx, who, prob_w, prob_h, w, h, &A));
    pfx_timer t(ctx, "matte_resize");
    if (resize) return launch_resize(ctx, A, grey_dev, matte_dev, nullptr, nullptr);
    PFX_HIP(ctx, hipMemcpyAsync(matte_dev, grey_dev, (size_t)w * h, hipMemcpyDeviceToDevice, ctx->stream));
    return PFX_OK;
}

int pfx_matte_feather_dev(pfx_ctx* ctx, const void* grey_dev, uint32_t w, uint32_t h, float edge_feather, void* matte_dev)
{
    const char* who = "pfx_matte_feather_dev";
    PFX_TRY(pfx_check_dims(ctx, who, w, h));
    const size_t n = (size_t)w * h;
    PFX_TRY(pfx_check_args(ctx, who, true, {{grey_dev, n, PFX_ARG_IN, "the grey image"}, {matte_dev, n, PFX_ARG_OUT, "the matte"}}));
    if (!std::isfinite(edge_feather)) return pfx_fail(ctx, PFX_ERR_INVALID, "%s: edge_feather is not finite", who);
    uint32_t r;
    PFX_TRY(feather_radius(ctx, who, edge_feather, &r));
    uint8_t* tmp = nullptr;
    if (r) PFX_TRY(reserve_planes(ctx, {n}, &tmp));
    pfx_timer t(ctx, "matte_feather");
    if (!r) {
        PFX_HIP(ctx, hipMemcpyAsync(matte_dev, grey_dev, n, hipMemcpyDeviceToDevice, ctx->stream));
        return PFX_OK;
    }
    PFX_HIP(ctx, pfxk_matte_box_h(ctx->stream, (const uint8_t*)grey_dev, tmp, w, h, r));
    PFX_HIP(ctx, pfxk_matte_box_v(ctx->stream, tmp, (uint8_t*)matte_dev, w, h, r, feather_band(r)));
    return PFX_OK;
}

int pfx_matte_apply_dev(pfx_ctx* ctx, const void* image_dev, const void* matte_dev, uint32_t w, uint32_t h, void* result_dev)
{
    const char* who = "pfx_matte_apply_dev";
    PFX_TRY(pfx_check_dims(ctx, who, w, h));
    const size_t n = (size_t)w * h;
    PFX_TRY(pfx_check_args(ctx, who, true, {{image_dev, n * 4, PFX_ARG_DWORD, "the image"}, {matte_dev, n, PFX_ARG_IN, "the matte"},
                                            {result_dev, n * 4, PFX_ARG_OUT | PFX_ARG_DWORD, "the result"}}, image_dev));
    pfx_timer t(ctx, "matte_apply");
    PFX_HIP(ctx, pfxk_matte_apply(ctx->stream, (const uint8_t*)image_dev, (const uint8_t*)matte_dev, (uint8_t*)result_dev, n));
    return PFX_OK;
}

// postprocess_mask in one call: the stage calls' own launches in the same order, except that without a feather the resize multiplies into alpha in its store, and
// the full-size matte is then written only when the caller asks for it.  Behind a feather the tail is the composition (profiles/matte.md: the column pass with the
// multiply in its store was no faster than the column pass and the streaming multiply)
int pfx_matte_postprocess_dev(pfx_ctx* ctx, const void* values_dev, uint32_t prob_w, uint32_t prob_h, int32_t is_probability, const void* image_dev, uint32_t w, uint32_t h,
                              const pfx_matte_settings* settings, void* result_dev, void* matte_dev)
{
    const char* who = "pfx_matte_postprocess_dev";
    uint32_t r;
    PFX_TRY(check_postprocess(ctx, who, true, values_dev, prob_w, prob_h, is_probability, image_dev, w, h, settings, result_dev, matte_dev, &r));
    const size_t pn = (size_t)prob_w * prob_h, n = (size_t)w * h;
    const bool resize = prob_w != w || prob_h != h;
    uint8_t* ws[7];   // two morphology planes, two grey planes at the model's size; at the document's: the resized matte, the row pass's, the final one
    PFX_TRY(reserve_planes(ctx, {pn, pn, pn, pn, (resize && r) ? n : 0, r ? n : 0, (r && !matte_dev) ? n : 0}, ws));
    pfx_matte_axes* A = nullptr;
    if (resize) PFX_TRY(prepare_resize(ctx, who, prob_w, prob_h, w, h, &A));   // refusals and the host's table work come before the first launch
    pfx_timer t(ctx, "matte_postprocess");
    uint8_t *grey = ws[2], *other = ws[3];
    PFX_TRY(run_byte(ctx, values_dev, prob_w, prob_h, is_probability, settings, grey));
    const int32_t runs[3] = {settings->mask_expansion, (int32_t)settings->fill_holes, -(int32_t)settings->fill_holes};   // :801, :807, :904-908
    for (int32_t e : runs)
        if (e != 0) {
            PFX_TRY(run_expand(ctx, grey, other, prob_w, prob_h, e, ws[0], ws[1]));
            std::swap(grey, other);
        }
    if (!r) {
        if (resize) return launch_resize(ctx, A, grey, matte_dev, image_dev, result_dev);
        if (matte_dev) PFX_HIP(ctx, hipMemcpyAsync(matte_dev, grey, n, hipMemcpyDeviceToDevice, ctx->stream));
        PFX_HIP(ctx, pfxk_matte_apply(ctx->stream, (const uint8_t*)image_dev, grey, (uint8_t*)result_dev, n));
        return PFX_OK;
    }
    const uint8_t* full = grey;
    if (resize) {
        PFX_TRY(launch_resize(ctx, A, grey, ws[4], nullptr, nullptr));
        full = ws[4];
    }
    uint8_t* soft = matte_dev ? (uint8_t*)matte_dev : ws[6];
    PFX_HIP(ctx, pfxk_matte_box_h(ctx->stream, full, ws[5], w, h, r));
    PFX_HIP(ctx, pfxk_matte_box_v(ctx->stream, ws[5], soft, w, h, r, feather_band(r)));
    PFX_HIP(ctx, pfxk_matte_apply(ctx->stream, (const uint8_t*)image_dev, soft, (uint8_t*)result_dev, n));
    return PFX_OK;
}

int pfx_matte_postprocess(pfx_ctx* ctx, const float* values, uint32_t prob_w, uint32_t prob_h, int32_t is_probability, const uint8_t* image, uint32_t w, uint32_t h,
                          const pfx_matte_settings* settings, uint8_t* result, uint8_t* matte)
{
    const char* who = "pfx_matte_postprocess";
    uint32_t r;
    PFX_TRY(check_postprocess(ctx, who, false, values, prob_w, prob_h, is_probability, image, w, h, settings, result, matte, &r));
    const size_t pn = (size_t)prob_w * prob_h, n = (size_t)w * h;
    void *d_values, *d_img, *d_matte = nullptr;
    PFX_TRY(pfx_stage(ctx, ctx->st_aux, values, pn * 4, &d_values));
    PFX_TRY(pfx_stage(ctx, ctx->st_in, image, n * 4, &d_img));
    if (matte) PFX_TRY(pfx_stage(ctx, ctx->st_mask, nullptr, n, &d_matte));
    PFX_TRY(pfx_matte_postprocess_dev(ctx, d_values, prob_w, prob_h, is_probability, d_img, w, h, settings, d_img, d_matte));   // in place
    if (matte) PFX_TRY(pfx_d2h(ctx, matte, d_matte, n));
    return pfx_unstage(ctx, result, ctx->st_in, n * 4);
}

} // extern "C"
