// pfx_api.cpp — the C ABI (include/pfx.h): argument checking, host<->device staging, kernel sequencing (the compositor's entry points: pfx_flatten.cpp).
// Host-buffer entry points = upload -> the `_dev` entry point -> download -> stream sync; `dst` is written only
// after every step succeeded (the reference's "never poison the document" rule).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "k_brush_math.h"
#include "pfx_internal.h"

void pfx_host_brush_lut(float size, float hardness, bool anti_aliased, uint8_t lut[256]);
void pfx_host_line_points(float x0, float y0, float x1, float y1, uint32_t w, uint32_t h, std::vector<float>& out);
void pfx_host_rhai_levels_lut(float in_black, float in_white, float gamma, uint8_t lut[256]);

static_assert((int)PFX_OP_COUNT == (int)PFXK_OP_COUNT && (int)PFX_OP_DESATURATE == (int)PFXK_OP_DESATURATE, "op ids out of sync");
static_assert((int)PFX_RHAI_COUNT == (int)PFXK_RHAI_COUNT && (int)PFX_RHAI_LEVELS == (int)PFXK_RHAI_LEVELS, "rhai ids out of sync");
static_assert((int)PFX_ADJ_CHANNEL_MIXER == (int)PFXK_ADJ_CHANNEL_MIXER, "layer kinds out of sync");

namespace {

// The filter family's declaration: a w x h src and dst.  In a `_dev` call dst shares no byte with src — a kernel that reads a halo while other workgroups write
// the same memory would race silently — unless the header allows in place (same_ok) and the two are the same pointer; the host tier works on staged copies.
// The mask is not declared: these calls have never looked at where it lies.
int check_img(pfx_ctx* ctx, const char* who, bool dev, const void* src, const void* dst, uint32_t w, uint32_t h, bool same_ok = false)
{
    PFX_TRY(pfx_check_dims(ctx, who, w, h));
    return pfx_check_args(ctx, who, dev, {{src, pfx_img_bytes(w, h), PFX_ARG_IN, "src"}, {dst, pfx_img_bytes(w, h), dev ? PFX_ARG_OUT : PFX_ARG_STAGED_OUT, "dst"}},
                          same_ok ? src : nullptr);
}
// the same for a call that works in one image (the selection is not declared either)
int check_inout(pfx_ctx* ctx, const char* who, const void* pixels, uint32_t w, uint32_t h)
{
    PFX_TRY(pfx_check_dims(ctx, who, w, h));
    return pfx_check_args(ctx, who, false, {{pixels, pfx_img_bytes(w, h), PFX_ARG_OUT, "the image"}});
}

// the filter family's staging: src in st_in, room for dst in st_out, the optional mask in st_mask
int stage_in(pfx_ctx* ctx, const uint8_t* src, const uint8_t* mask, uint32_t w, uint32_t h, const void** d_mask)
{
    void* d;
    PFX_TRY(pfx_stage(ctx, ctx->st_in, src, pfx_img_bytes(w, h), &d));
    PFX_TRY(pfx_stage(ctx, ctx->st_out, nullptr, pfx_img_bytes(w, h), &d));
    return pfx_stage_opt(ctx, ctx->st_mask, mask, (size_t)w * h, d_mask);
}

// host-side parameter preparation for the pointwise bank: everything that is uniform per call is folded here with
// the same f32 expressions the reference evaluates per pixel (so the kernels see identical constants)
int prepare_adjust(pfx_ctx* ctx, int op, const float* p, uint32_t n, pfxk_params& P, bool& needs_lut)
{
    std::memset(&P, 0, sizeof P);
    needs_lut = false;
    auto need = [&](uint32_t k) { return n >= k && p != nullptr; };
    switch (op) {
    case PFX_OP_INVERT: case PFX_OP_INVERT_ALPHA: case PFX_OP_SEPIA: case PFX_OP_DESATURATE: return PFX_OK;
    case PFX_OP_BRIGHTNESS_CONTRAST:
        if (!need(2)) break;
        P.p[0] = p[0]; P.p[1] = pfx_host_bc_factor(p[1]); return PFX_OK;
    case PFX_OP_HSL:
        if (!need(3)) break;
        P.p[0] = p[0] / 360.0f;            // hue_shift / 360.0   (adjustments.rs:310)
        P.p[1] = 1.0f + p[1] / 100.0f;     // sat_factor          (:307)
        P.p[2] = p[2] * 255.0f / 100.0f;   // light_offset        (:308)
        // p[11] != 0: every parameter is finite, so the kernel's results are finite and its cheaper round-and-pack applies (k_pointwise.hip)
        P.p[11] = (std::isfinite(P.p[0]) && std::isfinite(P.p[1]) && std::isfinite(P.p[2])) ? 1.0f : 0.0f;
        return PFX_OK;
    case PFX_OP_EXPOSURE:
        if (!need(1)) break;
        P.p[0] = pfx_host_exposure_gain(p[0]); return PFX_OK;
    case PFX_OP_HIGHLIGHTS_SHADOWS:
        if (!need(2)) break;
        P.p[0] = p[0] / 100.0f; P.p[1] = p[1] / 100.0f; return PFX_OK;
    case PFX_OP_TEMPERATURE_TINT:
        if (!need(2)) break;
        P.p[0] = p[0] * 1.5f; P.p[1] = p[1] * 1.0f; return PFX_OK;
    case PFX_OP_THRESHOLD:
        if (!need(1)) break;
        P.p[0] = p[0]; return PFX_OK;
    case PFX_OP_POSTERIZE:
        if (!need(1)) break;
        P.p[0] = std::max(p[0], 2.0f); return PFX_OK; // levels.max(2) as f32
    case PFX_OP_COLOR_BALANCE:
        if (!need(9)) break;
        for (int i = 0; i < 9; ++i) P.p[i] = p[i];
        return PFX_OK;
    case PFX_OP_BLACK_AND_WHITE:
        if (!need(3)) break;
        P.p[0] = p[0]; P.p[1] = p[1]; P.p[2] = p[2]; return PFX_OK;
    case PFX_OP_VIBRANCE:
        if (!need(1)) break;
        P.p[0] = p[0] / 100.0f;
        P.p[11] = std::isfinite(P.p[0]) ? 1.0f : 0.0f; // as for HSL
        return PFX_OK;
    case PFX_OP_GRADIENT_MAP: case PFX_OP_LUT_RGBA: needs_lut = true; return PFX_OK;
    default: return pfx_fail(ctx, PFX_ERR_INVALID, "pfx_adjust: unknown op %d", op);
    }
    return pfx_fail(ctx, PFX_ERR_INVALID, "pfx_adjust: op %d needs more parameters (got %u)", op, n);
}

int upload_lut(pfx_ctx* ctx, const uint8_t* lut_host, size_t bytes)
{
    uint8_t padded[1024] = {0};
    std::memcpy(padded, lut_host, std::min<size_t>(bytes, 1024));
    PFX_TRY(pfx_reserve(ctx, ctx->d_lut, 1024));
    return pfx_h2d(ctx, ctx->d_lut.p, padded, 1024);
}

// the displacement warp's declaration: an sw x sh source sampled into a w x h output through a w x h field.  The SOURCE's extent counts, it may be larger
// than the output; the field is only required (these calls have never looked at where it lies)
int check_warp(pfx_ctx* ctx, const char* who, bool dev, const void* src, uint32_t sw, uint32_t sh, const void* disp, uint32_t w, uint32_t h, const void* dst)
{
    PFX_TRY(pfx_check_dims(ctx, who, w, h));
    PFX_TRY(pfx_check_dims(ctx, who, sw, sh));
    return pfx_check_args(ctx, who, dev, {{src, pfx_img_bytes(sw, sh), PFX_ARG_IN, "src"}, {disp, 0, PFX_ARG_IN, "the displacement field"},
                                          {dst, pfx_img_bytes(w, h), dev ? PFX_ARG_OUT : PFX_ARG_STAGED_OUT, "dst"}});
}

int brush_prepare(pfx_ctx* ctx, const pfx_brush* b, pfxk_brush& B, bool& skip)
{
    PFX_REQUIRE(ctx, b != nullptr, "null brush");
    std::memset(&B, 0, sizeof B);
    skip = false;
    B.radius = b->size / 2.0f;                 // pressure_size() / 2 (brush_render.rs:196)
    B.radius_sq = B.radius * B.radius;
    if (B.radius_sq < 0.001f) { skip = true; return PFX_OK; }
    B.draw_radius = b->anti_aliased ? B.radius + 0.5f : B.radius;
    B.draw_radius_sq = B.draw_radius * B.draw_radius;
    B.use_direct_alpha = B.draw_radius > B.radius;
    B.inv_radius_sq = 1.0f / B.radius_sq;
    B.hardness = b->hardness;
    B.flow = b->flow;
    B.src_r = b->color[0]; B.src_g = b->color[1]; B.src_b = b->color[2]; B.src_a = b->color[3];
    auto u8 = [](float v) -> uint32_t { return !(v > 0.0f) ? 0u : (v >= 255.0f ? 255u : (uint32_t)(int)v); };
    B.rgb8 = u8(B.src_r * 255.0f) | (u8(B.src_g * 255.0f) << 8) | (u8(B.src_b * 255.0f) << 16); // :223-225 truncating
    B.anti_aliased = b->anti_aliased != 0;
    B.is_eraser = b->is_eraser != 0;
    B.mode = b->mode;
    PFX_REQUIRE(ctx, b->mode >= 0 && b->mode <= 3, "unknown brush mode");
    return PFX_OK;
}

} // namespace

extern "C" {

// ======================================================================= device tier
int pfx_gaussian_blur_dev(pfx_ctx* ctx, const void* src_dev, void* dst_dev, uint32_t w, uint32_t h, float sigma, void* tmp_dev)
{
    return pfx_gaussian_blur_band_dev(ctx, src_dev, dst_dev, w, h, sigma, tmp_dev, 0);
}

int pfx_gaussian_blur_band_dev(pfx_ctx* ctx, const void* src_dev, void* dst_dev, uint32_t w, uint32_t h, float sigma, void* tmp_dev,
                               uint32_t first_row)
{
    PFX_TRY(check_img(ctx, "pfx_gaussian_blur_dev", true, src_dev, dst_dev, w, h, true)); // in place: the two-pass kernels (through tmp)
    PFX_REQUIRE(ctx, (uint64_t)first_row + h <= 0x7fffffffull, "pfx_gaussian_blur_band_dev: band outside any image");   // the kernels carry image rows in 32-bit signed integers
    return pfx_gauss_blur(ctx, ctx->exact, src_dev, dst_dev, w, h, sigma, tmp_dev, first_row);   // which kernels run: pfx_gauss.cpp
}

int pfx_box_blur_dev(pfx_ctx* ctx, const void* src_dev, void* dst_dev, uint32_t w, uint32_t h, float radius,
                     const void* mask_dev, void* tmp_dev)
{
    PFX_TRY(check_img(ctx, "pfx_box_blur_dev", true, src_dev, dst_dev, w, h, true));
    if (radius < 0.5f) { // blur.rs:234: returns flat.clone()
        PFX_HIP(ctx, hipMemcpyAsync(dst_dev, src_dev, pfx_img_bytes(w, h), hipMemcpyDeviceToDevice, ctx->stream));
        return PFX_OK;
    }
    const float rc = ceilf(radius);
    PFX_REQUIRE(ctx, rc < 2040.0f, "box blur radius too large");
    return pfx_stencil_box(ctx, src_dev, dst_dev, w, h, (int)rc, mask_dev, tmp_dev);   // which kernels run: pfx_stencil.cpp
}

int pfx_box_blur_band_dev(pfx_ctx* ctx, const void* src_dev, void* dst_dev, uint32_t w, uint32_t h, float radius, const void* mask_dev,
                          void* tmp_dev, uint32_t first_row)
{
    (void)first_row; // integer window sums: a row's result does not depend on where the band was cut (pfx.h)
    return pfx_box_blur_dev(ctx, src_dev, dst_dev, w, h, radius, mask_dev, tmp_dev);
}

int pfx_median_band_dev(pfx_ctx* ctx, const void* src_dev, void* dst_dev, uint32_t w, uint32_t h, uint32_t radius, const void* mask_dev,
                        uint32_t first_row)
{
    (void)first_row;
    return pfx_median_dev(ctx, src_dev, dst_dev, w, h, radius, mask_dev);
}

int pfx_median_dev(pfx_ctx* ctx, const void* src_dev, void* dst_dev, uint32_t w, uint32_t h, uint32_t radius, const void* mask_dev)
{
    PFX_TRY(check_img(ctx, "pfx_median_dev", true, src_dev, dst_dev, w, h));
    const uint32_t r = std::max(radius, 1u); // noise.rs:364
    if (r > PFX_MEDIAN_MAX_RADIUS) return pfx_fail(ctx, PFX_ERR_UNSUPPORTED, "median radius %u > %d", r, PFX_MEDIAN_MAX_RADIUS);
    return pfx_stencil_median(ctx, src_dev, dst_dev, w, h, (int)r, mask_dev);   // which kernel runs: pfx_stencil.cpp
}

int pfx_pixelate_dev(pfx_ctx* ctx, const void* src_dev, void* dst_dev, uint32_t w, uint32_t h, uint32_t block_size, const void* mask_dev)
{
    PFX_TRY(check_img(ctx, "pfx_pixelate_dev", true, src_dev, dst_dev, w, h));
    pfx_timer t(ctx, "pixelate");
    PFX_HIP(ctx, pfxk_pixelate(ctx->stream, (const uint8_t*)src_dev, (uint8_t*)dst_dev, (const uint8_t*)mask_dev,
                               std::max(block_size, 2u), w, h)); // distort.rs:334
    return PFX_OK;
}

int pfx_adjust_dev(pfx_ctx* ctx, const void* src_dev, void* dst_dev, uint32_t w, uint32_t h, int op, const float* params,
                   uint32_t n_params, const uint8_t* lut_host, const void* mask_dev, int sparse_mode)
{
    PFX_TRY(check_img(ctx, "pfx_adjust_dev", true, src_dev, dst_dev, w, h, true)); // in place is fine (pointwise); a partial overlap races
    PFX_REQUIRE(ctx, sparse_mode >= PFX_DENSE && sparse_mode <= PFX_IN_PLACE, "unknown sparse mode");
    pfxk_params P;
    bool needs_lut = false;
    PFX_TRY(prepare_adjust(ctx, op, params, n_params, P, needs_lut));
    if (needs_lut) {
        PFX_REQUIRE(ctx, lut_host != nullptr, "this op needs a LUT");
        PFX_TRY(upload_lut(ctx, lut_host, 1024));
    }
    pfx_timer t(ctx, "adjust");
    PFX_HIP(ctx, pfxk_adjust(ctx->stream, (const uint8_t*)src_dev, (uint8_t*)dst_dev, (const uint8_t*)mask_dev,
                             (const uint8_t*)ctx->d_lut.p, op, &P, sparse_mode, w, h));
    return PFX_OK;
}

// parameter block of a Rhai-flavour op (scripting.rs:869-1075); `lut` (256 bytes) is filled when the op reads a table
static int prepare_rhai(pfx_ctx* ctx, int op, const float* p, uint32_t n, pfxk_params& P, uint8_t (&lut)[256], bool& needs_lut)
{
    std::memset(&P, 0, sizeof P);
    needs_lut = false;
    auto need = [&](uint32_t k) { return n >= k && p != nullptr; };
    bool ok = true;
    switch (op) {
    case PFX_RHAI_INVERT: case PFX_RHAI_DESATURATE: case PFX_RHAI_SEPIA: break;
    case PFX_RHAI_SEPIA_STRENGTH: // strength.clamp(0,1) as f32; inv = 1 - strength (scripting.rs:923-924)
        if ((ok = need(1))) { P.p[0] = (float)std::min(std::max((double)p[0], 0.0), 1.0); P.p[1] = 1.0f - P.p[0]; }
        break;
    case PFX_RHAI_BRIGHTNESS_CONTRAST:
        if ((ok = need(2))) { P.p[0] = p[0]; P.p[1] = pfx_host_bc_factor(p[1]); }
        break;
    case PFX_RHAI_HSL:
        if ((ok = need(3))) { P.p[0] = p[0] / 360.0f; P.p[1] = 1.0f + p[1] / 100.0f; P.p[2] = p[2] * 255.0f / 100.0f; }
        break;
    case PFX_RHAI_EXPOSURE:
        if ((ok = need(1))) P.p[0] = pfx_host_exposure_gain(p[0]);
        break;
    case PFX_RHAI_LEVELS:
        if ((ok = need(3))) { pfx_host_rhai_levels_lut(p[0], p[1], p[2], lut); needs_lut = true; }
        break;
    default: return pfx_fail(ctx, PFX_ERR_INVALID, "pfx_rhai_adjust: unknown op %d", op);
    }
    if (!ok) return pfx_fail(ctx, PFX_ERR_INVALID, "pfx_rhai_adjust: op %d needs more parameters", op);
    return PFX_OK;
}

int pfx_rhai_adjust_dev(pfx_ctx* ctx, void* pixels_dev, uint32_t w, uint32_t h, int op, const float* p, uint32_t n)
{
    PFX_TRY(check_inout(ctx, "pfx_rhai_adjust_dev", pixels_dev, w, h));
    pfxk_params P;
    uint8_t lut[256];
    bool needs_lut = false;
    PFX_TRY(prepare_rhai(ctx, op, p, n, P, lut, needs_lut));
    if (needs_lut) PFX_TRY(upload_lut(ctx, lut, 256));
    pfx_timer t(ctx, "rhai_adjust");
    PFX_HIP(ctx, pfxk_rhai_adjust(ctx->stream, (uint8_t*)pixels_dev, (const uint8_t*)ctx->d_lut.p, op, &P, w, h));
    return PFX_OK;
}

// ---- chains (round 6): several ops, as few passes over memory as the kernels allow; results equal the single-op entry points applied one after the other ----
// A run of pointwise ops is ONE launch (k_pointwise.hip: pointwise_chain_kernel, each op re-quantises to u8 in registers); a bit-exact Gaussian of radius <= 16
// followed by pointwise ops is ONE launch too (k_gauss_exact.hip, epilogue 3: the blurred image never exists in memory).  Every other stencil op runs as its own
// launch and hands its result to the next stage through at most one scratch image.  References: the ops' own (src/ops/filters.rs:214-316, src/ops/adjustments.rs,
// src/ops/scripting.rs:869-1075); the chain itself is how a script `apply_gaussian_blur(..); apply_hsl(..);` or the batch pipeline strings them together.
namespace {
struct chain_stage { int stencil = -1; uint32_t first = 0, count = 0; };   // stencil: index of the stage's Gaussian / box op or -1; [first, first + count): its pointwise ops
bool chain_pointwise(const pfx_chain_op& o) { return o.kind == PFX_CHAIN_ADJUST || o.kind == PFX_CHAIN_RHAI; }
}

static int chain_prepare(pfx_ctx* ctx, const pfx_chain_op* ops, uint32_t first, uint32_t count, pfxk_chain& C)
{
    std::memset(&C, 0, sizeof C);
    uint8_t luts[PFXK_CHAIN_LUTS][1024];
    for (uint32_t k = 0; k < count; ++k) {
        const pfx_chain_op& o = ops[first + k];
        bool needs_lut = false;
        if (o.kind == PFX_CHAIN_ADJUST) {
            PFX_TRY(prepare_adjust(ctx, o.op, o.params, o.n_params, C.P[k], needs_lut));
            C.op[k] = (uint32_t)o.op;
            if (needs_lut) {
                PFX_REQUIRE(ctx, o.lut != nullptr, "pfx_chain_dev: this op needs a LUT");
                std::memcpy(luts[C.n_luts], o.lut, 1024);
            }
        } else {
            uint8_t l256[256];
            PFX_TRY(prepare_rhai(ctx, o.op, o.params, o.n_params, C.P[k], l256, needs_lut));
            C.op[k] = PFXK_CHAIN_RHAI | (uint32_t)o.op;
            if (needs_lut) { std::memset(luts[C.n_luts], 0, 1024); std::memcpy(luts[C.n_luts], l256, 256); }
        }
        if (needs_lut) C.lut_slot[k] = C.n_luts++;
    }
    C.n = count;
    if (C.n_luts) {
        PFX_TRY(pfx_reserve(ctx, ctx->d_chain_luts, (size_t)PFXK_CHAIN_LUTS * 1024));
        PFX_TRY(pfx_h2d(ctx, ctx->d_chain_luts.p, luts, (size_t)C.n_luts * 1024));
    }
    return PFX_OK;
}

int pfx_chain_dev(pfx_ctx* ctx, const void* src_dev, void* dst_dev, uint32_t w, uint32_t h, const pfx_chain_op* ops, uint32_t n_ops)
{
    PFX_TRY(check_img(ctx, "pfx_chain_dev", true, src_dev, dst_dev, w, h, true));
    PFX_REQUIRE(ctx, ops != nullptr || n_ops == 0, "pfx_chain_dev: null op list");
    const size_t bytes = pfx_img_bytes(w, h);
    // stages: [stencil op +] a run of pointwise ops that one launch can carry (PFXK_CHAIN_MAX ops, PFXK_CHAIN_LUTS tables)
    std::vector<chain_stage> stages;
    uint32_t n_stencil = 0;
    for (uint32_t i = 0; i < n_ops;) {
        chain_stage st;
        if (!chain_pointwise(ops[i])) {
            if (ops[i].kind != PFX_CHAIN_GAUSSIAN && ops[i].kind != PFX_CHAIN_BOX) return pfx_fail(ctx, PFX_ERR_INVALID, "pfx_chain_dev: unknown op kind %d", ops[i].kind);
            PFX_REQUIRE(ctx, ops[i].n_params >= 1, "pfx_chain_dev: a blur needs its sigma / radius in params[0]");
            st.stencil = (int)i++;
            ++n_stencil;
        }
        st.first = i;
        uint32_t luts = 0;
        while (i < n_ops && chain_pointwise(ops[i]) && st.count < PFXK_CHAIN_MAX) {
            const bool lut_op = ops[i].kind == PFX_CHAIN_ADJUST ? (ops[i].op == PFX_OP_GRADIENT_MAP || ops[i].op == PFX_OP_LUT_RGBA) : ops[i].op == PFX_RHAI_LEVELS;
            if (lut_op && luts == PFXK_CHAIN_LUTS) break;
            luts += lut_op ? 1u : 0u;
            ++st.count; ++i;
        }
        stages.push_back(st);
    }
    if (src_dev == dst_dev) PFX_REQUIRE(ctx, n_stencil == 0, "pfx_chain_dev: a chain with a blur cannot run in place");
    if (stages.empty()) {
        if (src_dev != dst_dev) PFX_HIP(ctx, hipMemcpyAsync(dst_dev, src_dev, bytes, hipMemcpyDeviceToDevice, ctx->stream));
        return PFX_OK;
    }
    if (n_stencil > 1 || (n_stencil == 1 && stages.front().stencil < 0)) PFX_TRY(pfx_reserve(ctx, ctx->st_chain, bytes));
    // a stencil stage writes dst or the scratch image, alternating so that the LAST one writes dst (pointwise stages behind a stencil run in place)
    uint32_t seen = 0;
    auto stencil_out = [&](uint32_t j) -> void* { return ((n_stencil - 1u - j) % 2u == 0u) ? dst_dev : ctx->st_chain.p; };
    const void* cur = src_dev;
    for (const chain_stage& st : stages) {
        pfxk_chain C;
        if (st.count) PFX_TRY(chain_prepare(ctx, ops, st.first, st.count, C));
        if (st.stencil < 0) {
            // pointwise only: in place behind a stencil; in front of the first one into the buffer that stencil does not write
            void* out = cur == src_dev ? (n_stencil == 0 ? dst_dev : (stencil_out(0) == dst_dev ? ctx->st_chain.p : dst_dev)) : const_cast<void*>(cur);
            pfx_timer t(ctx, "chain");
            PFX_HIP(ctx, pfxk_pointwise_chain(ctx->stream, (const uint8_t*)cur, (uint8_t*)out, (const uint8_t*)ctx->d_chain_luts.p, &C, w, h));
            cur = out;
            continue;
        }
        const pfx_chain_op& so = ops[st.stencil];
        void* out = stencil_out(seen++);
        // The pointwise run rides in the Gaussian's store only when it is light: a Gaussian kernel is bound by its own arithmetic and dependency chains, not by HBM,
        // so an op of ~140 instructions per pixel (HSL, vibrance) costs there what it costs as a streaming pass of its own and the fused launch saves nothing
        // (8K sigma 16 -> HSL: 0.210 ms fused against 0.206 as two launches; bit-exact sigma 4 -> HSL 0.381 against 0.371: profiles/r06_tuning.md); light ops
        // (invert, exposure, brightness / contrast, tables ...) cost a few instructions and save the 8 B/px round trip.  pfx_tune "chain_fuse_heavy" = 1 fuses anyway
        // (the rule itself: pfx_gauss.cpp).
        bool heavy = false, rode = false;
        for (uint32_t k = 0; k < st.count; ++k) {
            const pfx_chain_op& o = ops[st.first + k];
            heavy = heavy || (o.kind == PFX_CHAIN_ADJUST && (o.op == PFX_OP_HSL || o.op == PFX_OP_VIBRANCE)) || (o.kind == PFX_CHAIN_RHAI && o.op == PFX_RHAI_HSL);
        }
        if (so.kind == PFX_CHAIN_GAUSSIAN) PFX_TRY(pfx_gauss_chain(ctx, ctx->exact, cur, out, w, h, so.params[0], st.count ? &C : nullptr, heavy, &rode));
        else PFX_TRY(pfx_box_blur_dev(ctx, cur, out, w, h, so.params[0], nullptr, nullptr));
        if (st.count && !rode) {
            pfx_timer t(ctx, "chain");
            PFX_HIP(ctx, pfxk_pointwise_chain(ctx->stream, (const uint8_t*)out, (uint8_t*)out, (const uint8_t*)ctx->d_chain_luts.p, &C, w, h));
        }
        cur = out;
    }
    if (cur != dst_dev) PFX_HIP(ctx, hipMemcpyAsync(dst_dev, cur, bytes, hipMemcpyDeviceToDevice, ctx->stream));   // unreachable by construction; kept as a guard
    return PFX_OK;
}

int pfx_warp_displacement_band_dev(pfx_ctx* ctx, const void* src_dev, uint32_t sw, uint32_t sh, const void* disp_band_dev, uint32_t w,
                                   uint32_t band_rows, void* dst_band_dev, uint32_t first_row)
{
    PFX_TRY(check_warp(ctx, "pfx_warp_displacement_dev", true, src_dev, sw, sh, disp_band_dev, w, band_rows, dst_band_dev));
    PFX_REQUIRE(ctx, (uint64_t)first_row + band_rows <= 0x7fffffffull, "pfx_warp_displacement_dev: band outside any image");
    pfx_timer t(ctx, "warp_displacement");
    PFX_HIP(ctx, pfxk_warp_displacement(ctx->stream, (const uint8_t*)src_dev, sw, sh, (const float*)disp_band_dev, w, band_rows, (uint8_t*)dst_band_dev, first_row,
                                        &ctx->last_warp));
    return PFX_OK;
}

int pfx_warp_displacement_dev(pfx_ctx* ctx, const void* src_dev, uint32_t sw, uint32_t sh, const void* disp_dev, uint32_t w,
                              uint32_t h, void* dst_dev)
{
    return pfx_warp_displacement_band_dev(ctx, src_dev, sw, sh, disp_dev, w, h, dst_dev, 0);
}

// DisplacementField::apply_* on a device-resident field: per-dab prologue (radius clamp, sigma, loop bounds) on the host exactly as
// the reference computes it (transform.rs:1056-1069), accumulation in k_warp.hip
int pfx_displacement_brushes_dev(pfx_ctx* ctx, void* disp_dev, uint32_t w, uint32_t h, const pfx_disp_dab* dabs, uint32_t n_dabs)
{
    PFX_TRY(pfx_check_dims(ctx, "pfx_displacement_brushes_dev", w, h));
    PFX_TRY(pfx_check_args(ctx, "pfx_displacement_brushes_dev", true, {{disp_dev, (size_t)w * h * 8, PFX_ARG_OUT, "disp_dev"}}));
    PFX_REQUIRE(ctx, n_dabs == 0 || dabs, "pfx_displacement_brushes_dev: null dab list");
    ctx->last_dab_launch = 0;   // nothing launched, unless the list reaches the canvas
    ctx->last_dab_chunks = 0;
    if (n_dabs == 0) return PFX_OK;
    auto f2i = [](float v) -> int32_t { return v != v ? 0 : (v >= 2147483648.0f ? 2147483647 : (v <= -2147483648.0f ? (-2147483647 - 1) : (int32_t)v)); };
    std::vector<pfxk_disp_dab> k(n_dabs);
    int bx0 = (int)w, by0 = (int)h, bx1 = 0, by1 = 0;
    for (uint32_t i = 0; i < n_dabs; ++i) {
        const pfx_disp_dab& D = dabs[i];
        PFX_REQUIRE(ctx, D.mode >= 0 && D.mode <= 4, "pfx_displacement_brushes_dev: unknown brush mode");
        pfxk_disp_dab& K = k[i];
        K.mode = D.mode;
        K.cx = D.cx; K.cy = D.cy; K.delta_x = D.delta_x; K.delta_y = D.delta_y; K.strength = D.strength;
        K.r = fmaxf(D.radius, 1.0f);
        const float sigma = K.r / 3.0f;
        K.sigma_sq_2 = 2.0f * sigma * sigma;
        K.x0 = std::max(f2i(floorf(D.cx - K.r)), 0);
        K.y0 = std::max(f2i(floorf(D.cy - K.r)), 0);
        K.x1 = std::min(f2i(ceilf(D.cx + K.r)), (int32_t)w);
        K.y1 = std::min(f2i(ceilf(D.cy + K.r)), (int32_t)h);
        if (K.x1 > K.x0 && K.y1 > K.y0) { bx0 = std::min(bx0, K.x0); by0 = std::min(by0, K.y0); bx1 = std::max(bx1, K.x1); by1 = std::max(by1, K.y1); }
    }
    if (bx1 <= bx0 || by1 <= by0) return PFX_OK; // every dab is off-canvas
    // Dabs spread over a large field: launch over the 64 x 64 chunks their boxes touch instead of the common bounding box when that is less than half of it
    std::vector<uint32_t> chunks;
    {
        const uint32_t cx0 = (uint32_t)bx0 >> 6, cy0 = (uint32_t)by0 >> 6, ncx = (((uint32_t)bx1 + 63u) >> 6) - cx0, ncy = (((uint32_t)by1 + 63u) >> 6) - cy0;
        if ((uint64_t)ncx * ncy >= 256u && ncx < 65536u && ncy < 65536u) {
            std::vector<uint8_t> hit((size_t)ncx * ncy, 0);
            for (const pfxk_disp_dab& K : k) {
                if (!(K.x1 > K.x0 && K.y1 > K.y0)) continue;
                for (uint32_t cy = (uint32_t)K.y0 >> 6; cy <= ((uint32_t)K.y1 - 1u) >> 6; ++cy)
                    for (uint32_t cx = (uint32_t)K.x0 >> 6; cx <= ((uint32_t)K.x1 - 1u) >> 6; ++cx) hit[(size_t)(cy - cy0) * ncx + (cx - cx0)] = 1;
            }
            for (uint32_t cy = 0; cy < ncy; ++cy)
                for (uint32_t cx = 0; cx < ncx; ++cx)
                    if (hit[(size_t)cy * ncx + cx]) chunks.push_back((cx0 + cx) | ((cy0 + cy) << 16));
            if (chunks.size() * 2u > (size_t)ncx * ncy) chunks.clear();   // mostly covered: the plain launch
        }
    }
    const size_t dab_bytes = (k.size() * sizeof(pfxk_disp_dab) + 15u) & ~(size_t)15u;
    PFX_TRY(pfx_reserve(ctx, ctx->d_pts, dab_bytes + chunks.size() * 4u + 16u));
    PFX_TRY(pfx_h2d(ctx, ctx->d_pts.p, k.data(), k.size() * sizeof(pfxk_disp_dab)));
    if (!chunks.empty()) PFX_TRY(pfx_h2d(ctx, (uint8_t*)ctx->d_pts.p + dab_bytes, chunks.data(), chunks.size() * 4u));
    PFX_HIP(ctx, hipStreamSynchronize(ctx->stream)); // `k` / `chunks` are pageable host memory about to go out of scope
    pfx_timer t(ctx, "displacement_brush");
    ctx->last_dab_launch = chunks.empty() ? 1 : 2;
    ctx->last_dab_chunks = (int)chunks.size();
    if (!chunks.empty())
        PFX_HIP(ctx, pfxk_disp_brushes_chunked(ctx->stream, (float*)disp_dev, w, h, (const pfxk_disp_dab*)ctx->d_pts.p, n_dabs, bx0, by0, bx1, by1,
                                               (const uint32_t*)((const uint8_t*)ctx->d_pts.p + dab_bytes), (uint32_t)chunks.size()));
    else
        PFX_HIP(ctx, pfxk_disp_brushes(ctx->stream, (float*)disp_dev, w, h, (const pfxk_disp_dab*)ctx->d_pts.p, n_dabs, bx0, by0, bx1, by1));
    return PFX_OK;
}

static int upload_points(pfx_ctx* ctx, const float* orig, const float* def, uint32_t cols, uint32_t rows, const float** d_orig,
                         const float** d_def)
{
    PFX_REQUIRE(ctx, def && cols >= 1 && rows >= 1 && cols <= 4096 && rows <= 4096, "mesh: bad grid");
    const size_t npts = (size_t)(cols + 1) * (rows + 1);
    PFX_TRY(pfx_reserve(ctx, ctx->d_pts, npts * 2 * sizeof(float) * 2));
    float* base = (float*)ctx->d_pts.p;
    PFX_TRY(pfx_h2d(ctx, base, def, npts * 2 * sizeof(float)));
    *d_def = base;
    *d_orig = nullptr;
    if (orig) {
        PFX_TRY(pfx_h2d(ctx, base + npts * 2, orig, npts * 2 * sizeof(float)));
        *d_orig = base + npts * 2;
    }
    return PFX_OK;
}

int pfx_mesh_displacement_dev(pfx_ctx* ctx, const float* orig_pts_xy, const float* deformed_pts_xy, uint32_t cols, uint32_t rows,
                              uint32_t w, uint32_t h, void* disp_dev)
{
    PFX_TRY(pfx_check_dims(ctx, "pfx_mesh_displacement_dev", w, h));
    PFX_TRY(pfx_check_args(ctx, "pfx_mesh_displacement_dev", true, {{disp_dev, (size_t)w * h * 8, PFX_ARG_OUT, "disp_dev"}}));
    const float *d_orig, *d_def;
    PFX_TRY(upload_points(ctx, orig_pts_xy, deformed_pts_xy, cols, rows, &d_orig, &d_def));
    pfx_timer t(ctx, "mesh_displacement");
    PFX_HIP(ctx, pfxk_mesh_displacement(ctx->stream, d_orig, d_def, cols, rows, w, h, (float*)disp_dev, &ctx->last_warp));
    return PFX_OK;
}

int pfx_warp_mesh_catmull_rom_band_dev(pfx_ctx* ctx, const void* src_dev, const float* orig_pts_xy, const float* deformed_pts_xy,
                                       uint32_t cols, uint32_t rows, uint32_t w, uint32_t h, void* dst_band_dev, uint32_t first_row, uint32_t band_rows)
{
    PFX_TRY(pfx_check_dims(ctx, "pfx_warp_mesh_catmull_rom_dev", w, h));
    PFX_TRY(pfx_check_args(ctx, "pfx_warp_mesh_catmull_rom_dev", true, {{src_dev, pfx_img_bytes(w, h), PFX_ARG_IN, "src"}, {dst_band_dev, pfx_img_bytes(w, band_rows), PFX_ARG_OUT, "dst"}}));
    PFX_REQUIRE(ctx, band_rows >= 1 && (uint64_t)first_row + band_rows <= h, "pfx_warp_mesh_catmull_rom_dev: band outside the image");
    const float *d_orig, *d_def;
    PFX_TRY(upload_points(ctx, orig_pts_xy, deformed_pts_xy, cols, rows, &d_orig, &d_def));
    pfx_timer t(ctx, "warp_mesh");
    PFX_HIP(ctx, pfxk_warp_mesh(ctx->stream, (const uint8_t*)src_dev, d_orig, d_def, cols, rows, w, band_rows, (uint8_t*)dst_band_dev, first_row, h, &ctx->last_warp));
    return PFX_OK;
}

int pfx_warp_mesh_catmull_rom_dev(pfx_ctx* ctx, const void* src_dev, const float* orig_pts_xy, const float* deformed_pts_xy,
                                  uint32_t cols, uint32_t rows, uint32_t w, uint32_t h, void* dst_dev)
{
    return pfx_warp_mesh_catmull_rom_band_dev(ctx, src_dev, orig_pts_xy, deformed_pts_xy, cols, rows, w, h, dst_dev, 0, h);
}

// Per-stamp host prologue of draw_circle_no_dirty / draw_image_tip_no_dirty (brush_render.rs:148-256, 552-632): the reference
// computes scatter, colour jitter and tip rotation on the CPU once per stamp; so does this, then the stamp list goes to the kernel.
static uint32_t stamp_hash(float x, float y, uint32_t counter) // :846-857
{
    uint32_t hsh = pfx_f32_as_u32(x * 100.0f) * 374761393u + pfx_f32_as_u32(y * 100.0f) * 668265263u + counter * 1013904223u;
    hsh ^= hsh >> 13;
    hsh *= 1274126177u;
    hsh ^= hsh >> 16;
    return hsh;
}
static void host_rgb_to_hsl(float r, float g, float b, float& hh, float& s, float& l) // adjustments.rs:944-974
{
    const float mx = fmaxf(fmaxf(r, g), b), mn = fminf(fminf(r, g), b);
    l = (mx + mn) / 2.0f;
    if (fabsf(mx - mn) < 1e-6f) { hh = 0.0f; s = 0.0f; return; }
    const float d = mx - mn;
    s = l > 0.5f ? d / (2.0f - mx - mn) : d / (mx + mn);
    if (fabsf(mx - r) < 1e-6f) { float t = (g - b) / d; if (t < 0.0f) t += 6.0f; hh = t / 6.0f; }
    else if (fabsf(mx - g) < 1e-6f) hh = ((b - r) / d + 2.0f) / 6.0f;
    else hh = ((r - g) / d + 4.0f) / 6.0f;
}
static float host_hue_to_rgb(float p, float q, float t) // adjustments.rs:995-1012
{
    if (t < 0.0f) t += 1.0f;
    if (t > 1.0f) t -= 1.0f;
    if (t < 1.0f / 6.0f) return p + (q - p) * 6.0f * t;
    if (t < 1.0f / 2.0f) return q;
    if (t < 2.0f / 3.0f) return p + (q - p) * (2.0f / 3.0f - t) * 6.0f;
    return p;
}
static void host_hsl_to_rgb(float hh, float s, float l, float& r, float& g, float& b) // adjustments.rs:976-993
{
    if (fabsf(s) < 1e-6f) { r = g = b = l; return; }
    const float q = l < 0.5f ? l * (1.0f + s) : l + s - l * s;
    const float p = 2.0f * l - q;
    r = host_hue_to_rgb(p, q, hh + 1.0f / 3.0f);
    g = host_hue_to_rgb(p, q, hh);
    b = host_hue_to_rgb(p, q, hh - 1.0f / 3.0f);
}

int pfx_brush_stamps_ex_dev(pfx_ctx* ctx, void* target_dev, uint32_t w, uint32_t h, const pfx_brush* brush, const pfx_brush_dynamics* dyn,
                            const float* points_xy, uint32_t n_points, const void* selection_dev)
{
    PFX_TRY(check_inout(ctx, "pfx_brush_stamps_dev", target_dev, w, h));
    ctx->last_brush_path = 0;
    if (n_points == 0) return PFX_OK;
    PFX_REQUIRE(ctx, points_xy != nullptr, "null stamp list");
    const bool image_tip = dyn && dyn->tip_mask;
    pfxk_brush B;
    bool skip;
    PFX_TRY(brush_prepare(ctx, brush, B, skip));
    if (image_tip) {
        if (dyn->tip_mask_size == 0) return PFX_OK; // :546-549
        PFX_REQUIRE(ctx, dyn->tip_mask_size <= 8192, "brush tip mask too large");
        B.tip_size = dyn->tip_mask_size;
    } else if (skip) return PFX_OK; // radius_sq < 0.001 (brush_render.rs:198)

    auto u8 = [](float v) -> uint32_t { return !(v > 0.0f) ? 0u : (v >= 255.0f ? 255u : (uint32_t)(int)v); };
    std::vector<pfxk_stamp> st(n_points);
    const float half = image_tip ? (float)dyn->tip_mask_size / 2.0f : 0.0f;
    uint32_t ux0 = 1u, ux1 = 0u, uy0 = 1u, uy1 = 0u;   // union of the stamps' pixel boxes; empty so far
    for (uint32_t i = 0; i < n_points; ++i) {
        const float px = points_xy[2 * i], py = points_xy[2 * i + 1];
        pfxk_stamp& S = st[i];
        S.cx = px; S.cy = py; S.cos_a = 1.0f; S.sin_a = 0.0f; S.rotated = 0;
        if (dyn && dyn->scatter > 0.01f) { // :179-193 / :552-565
            const float diam = brush->size; // pressure_size() without pen pressure
            const float h1 = (float)stamp_hash(px, py, dyn->stamp_counter) / 4294967295.0f;
            const float h2 = (float)stamp_hash(py, px, dyn->stamp_counter + 99991u) / 4294967295.0f;
            S.cx = px + (h1 * 2.0f - 1.0f) * dyn->scatter * diam;
            S.cy = py + (h2 * 2.0f - 1.0f) * dyn->scatter * diam;
        }
        S.rgb8 = B.rgb8;
        if (dyn && (dyn->hue_jitter > 0.01f || dyn->brightness_jitter > 0.01f)) { // :226-256 / :602-632
            float hh, s, l, nr, ng, nb;
            host_rgb_to_hsl(brush->color[0], brush->color[1], brush->color[2], hh, s, l);
            if (dyn->hue_jitter > 0.01f) {
                const float hv = (float)stamp_hash(px + 0.1f, py + 0.2f, dyn->stamp_counter + 777u) / 4294967295.0f;
                const float v = hh + (hv * 2.0f - 1.0f) * dyn->hue_jitter * 0.5f;
                hh = v - truncf(v);
                if (hh < 0.0f) hh += 1.0f;
            }
            if (dyn->brightness_jitter > 0.01f) {
                const float bv = (float)stamp_hash(px + 0.3f, py + 0.4f, dyn->stamp_counter + 555u) / 4294967295.0f;
                l = pfx_clampf(l + (bv * 2.0f - 1.0f) * dyn->brightness_jitter * 0.5f, 0.0f, 1.0f);
            }
            host_hsl_to_rgb(hh, s, l, nr, ng, nb);
            S.rgb8 = u8(nr * 255.0f) | (u8(ng * 255.0f) << 8) | (u8(nb * 255.0f) << 16);
        }
        if (image_tip) { // :148-163, :570-581
            float rotation_deg = dyn->tip_rotation;
            if (dyn->tip_random_rotation) {
                const float lo = dyn->tip_rotation_lo, range = dyn->tip_rotation_hi - lo;
                rotation_deg = fabsf(range) < 0.01f ? lo : lo + (float)(stamp_hash(px, py, dyn->stamp_counter) % 10000u) / 10000.0f * range;
            }
            if (fabsf(rotation_deg) > 0.01f) {
                const float rad = -(rotation_deg * (3.14159265358979323846f / 180.0f)); // negative: inverse rotation for sampling
                S.cos_a = cosf(rad); S.sin_a = sinf(rad); S.rotated = 1;
            }
        }
        // the stamp's pixel box, with the reference's float operations (:209-215 round tip, :584-587 image tip; `as u32` saturates, NaN -> 0): the kernel tests
        // pixels against it and the binning below deals the stamp to the chunks it touches
        {
            const uint32_t wm1 = w - 1u, hm1 = h - 1u;
            if (image_tip) {
                const float eh = S.rotated ? half * 1.41421356237309504880f : half;
                S.x0 = pfx_f32_as_u32(fmaxf(S.cx - eh, 0.0f)); S.y0 = pfx_f32_as_u32(fmaxf(S.cy - eh, 0.0f));
                S.x1 = std::min(pfx_f32_as_u32(S.cx + eh), wm1); S.y1 = std::min(pfx_f32_as_u32(S.cy + eh), hm1);
            } else {
                S.x0 = pfx_f32_as_u32(fmaxf(floorf(S.cx - B.draw_radius), 0.0f)); S.x1 = std::min(pfx_f32_as_u32(ceilf(S.cx + B.draw_radius)), wm1);
                S.y0 = pfx_f32_as_u32(fmaxf(floorf(S.cy - B.draw_radius), 0.0f)); S.y1 = std::min(pfx_f32_as_u32(ceilf(S.cy + B.draw_radius)), hm1);
            }
            if (S.x0 > S.x1 || S.y0 > S.y1) { S.x0 = 1u; S.x1 = 0u; S.y0 = 1u; S.y1 = 0u; }   // touches no pixel
            else if (ux0 > ux1) { ux0 = S.x0; ux1 = S.x1; uy0 = S.y0; uy1 = S.y1; }
            else { ux0 = std::min(ux0, S.x0); ux1 = std::max(ux1, S.x1); uy0 = std::min(uy0, S.y0); uy1 = std::max(uy1, S.y1); }
            S.pad[0] = S.pad[1] = 0u;
        }
    }
    // The launch box of the bounding-box kernel is the union of the per-stamp pixel boxes above, every one of them inside the canvas.  A non-finite centre has
    // the box the reference's casts give it (brush_render.rs:208-215, 584-587: NaN -> column / row 0, +inf -> past the edge and empty, -inf -> column / row 0) and
    // is walked like any other stamp, wherever it stands in the stroke and whichever kernel runs.
    if (ux0 > ux1) return PFX_OK;   // no stamp touches a pixel
    const int bx0 = (int)ux0, by0 = (int)uy0, bx1 = (int)ux1, by1 = (int)uy1;
    const size_t stamp_bytes = st.size() * sizeof(pfxk_stamp), tip_bytes = image_tip ? (size_t)dyn->tip_mask_size * dyn->tip_mask_size : 0;
    // Strokes of more than one cull group: deal the stamps to the 64 x 64 chunks (TiledImage's grid) their boxes touch, so that the kernel's work follows the painted
    // area instead of the stroke's bounding box times its length.  A chunk's list holds every stamp whose pixel box (above) touches it, in stroke order.
    std::vector<uint32_t> chunk_tab, bins;
    if (n_points > 64u && ctx->brush_binning) {
        const uint32_t ncx = (w + 63u) / 64u, ncy = (h + 63u) / 64u;
        std::vector<uint32_t> box(4 * (size_t)n_points), count((size_t)ncx * ncy, 0u);
        uint64_t entries = 0;
        for (uint32_t i = 0; i < n_points && entries <= (8ull << 20); ++i) {
            const pfxk_stamp& S = st[i];
            uint32_t* b = &box[4 * (size_t)i];
            if (S.x0 > S.x1) { b[0] = 1; b[1] = 0; b[2] = 1; b[3] = 0; continue; }
            b[0] = S.x0 >> 6; b[1] = S.x1 >> 6; b[2] = S.y0 >> 6; b[3] = S.y1 >> 6;
            entries += (uint64_t)(b[1] - b[0] + 1u) * (b[3] - b[2] + 1u);
        }
        if (entries > 0 && entries <= (8ull << 20)) {   // beyond 8 M entries (huge tips on long strokes) the unbinned kernel runs
            for (uint32_t i = 0; i < n_points; ++i) {
                const uint32_t* b = &box[4 * (size_t)i];
                for (uint32_t cy = b[2]; cy <= b[3] && b[0] <= b[1]; ++cy)
                    for (uint32_t cx = b[0]; cx <= b[1]; ++cx) ++count[(size_t)cy * ncx + cx];
            }
            std::vector<uint32_t> first(count.size());
            uint32_t off = 0;
            for (size_t c = 0; c < count.size(); ++c) {
                first[c] = off;
                if (count[c]) { chunk_tab.push_back((uint32_t)(c % ncx)); chunk_tab.push_back((uint32_t)(c / ncx)); chunk_tab.push_back(off); chunk_tab.push_back(count[c]); }
                off += count[c];
            }
            bins.resize(off);
            for (uint32_t i = 0; i < n_points; ++i) {   // stamps in order: every chunk's list comes out in stroke order
                const uint32_t* b = &box[4 * (size_t)i];
                for (uint32_t cy = b[2]; cy <= b[3] && b[0] <= b[1]; ++cy)
                    for (uint32_t cx = b[0]; cx <= b[1]; ++cx) bins[first[(size_t)cy * ncx + cx]++] = i;
            }
        }
    }
    const size_t tab_off = (stamp_bytes + tip_bytes + 15u) & ~(size_t)15u, tab_bytes = chunk_tab.size() * 4u, bins_bytes = bins.size() * 4u;
    PFX_TRY(pfx_reserve(ctx, ctx->d_pts, tab_off + tab_bytes + bins_bytes + 512));
    PFX_TRY(pfx_h2d(ctx, ctx->d_pts.p, st.data(), stamp_bytes));
    const uint8_t* d_tip = nullptr;
    if (image_tip) {
        PFX_TRY(pfx_h2d(ctx, (uint8_t*)ctx->d_pts.p + stamp_bytes, dyn->tip_mask, tip_bytes));
        d_tip = (const uint8_t*)ctx->d_pts.p + stamp_bytes;
    }
    if (!chunk_tab.empty()) {
        PFX_TRY(pfx_h2d(ctx, (uint8_t*)ctx->d_pts.p + tab_off, chunk_tab.data(), tab_bytes));
        PFX_TRY(pfx_h2d(ctx, (uint8_t*)ctx->d_pts.p + tab_off + tab_bytes, bins.data(), bins_bytes));
    }
    PFX_HIP(ctx, hipStreamSynchronize(ctx->stream)); // `st` is pageable host memory about to go out of scope
    const uint8_t* d_lut = nullptr;
    if (!image_tip && !B.use_direct_alpha) { // LUT path only when AA is off (brush_render.rs:329-337)
        uint8_t lut[256];
        pfx_host_brush_lut(brush->size, brush->hardness, brush->anti_aliased != 0, lut);
        PFX_TRY(upload_lut(ctx, lut, 256));
        d_lut = (const uint8_t*)ctx->d_lut.p;
    }
    pfx_timer t(ctx, "brush_stamps");
    ctx->last_brush_path = chunk_tab.empty() ? 1 : 2;
    if (!chunk_tab.empty())
        PFX_HIP(ctx, pfxk_brush_stamps_binned(ctx->stream, (uint8_t*)target_dev, w, h, &B, (const pfxk_stamp*)ctx->d_pts.p, n_points, d_lut, d_tip,
                                              (const uint8_t*)selection_dev, (const uint32_t*)((const uint8_t*)ctx->d_pts.p + tab_off), (uint32_t)(chunk_tab.size() / 4u),
                                              (const uint32_t*)((const uint8_t*)ctx->d_pts.p + tab_off + tab_bytes)));
    else
        PFX_HIP(ctx, pfxk_brush_stamps(ctx->stream, (uint8_t*)target_dev, w, h, &B, (const pfxk_stamp*)ctx->d_pts.p, n_points, d_lut, d_tip,
                                       (const uint8_t*)selection_dev, bx0, by0, bx1, by1));
    return PFX_OK;
}

int pfx_int_brush_last(pfx_ctx* ctx) { return !ctx ? -1 : ctx->last_brush_path; }

int pfx_brush_stamps_dev(pfx_ctx* ctx, void* target_dev, uint32_t w, uint32_t h, const pfx_brush* brush, const float* points_xy,
                         uint32_t n_points, const void* selection_dev)
{
    return pfx_brush_stamps_ex_dev(ctx, target_dev, w, h, brush, nullptr, points_xy, n_points, selection_dev);
}

int pfx_tiled_roundtrip_dev(pfx_ctx* ctx, const void* src_dev, void* dst_dev, uint32_t w, uint32_t h)
{
    PFX_TRY(check_img(ctx, "pfx_tiled_roundtrip_dev", true, src_dev, dst_dev, w, h, true));
    pfx_timer t(ctx, "tiled_roundtrip");
    PFX_HIP(ctx, pfxk_tiled_roundtrip(ctx->stream, (const uint8_t*)src_dev, (uint8_t*)dst_dev, w, h));
    return PFX_OK;
}

// ======================================================================= host-buffer tier
int pfx_gaussian_blur_core(pfx_ctx* ctx, const uint8_t* src, uint8_t* dst, uint32_t w, uint32_t h, float sigma, const uint8_t* mask)
{
    PFX_TRY(check_img(ctx, "pfx_gaussian_blur_core", false, src, dst, w, h));
    const void* d_mask;
    PFX_TRY(stage_in(ctx, src, mask, w, h, &d_mask));
    PFX_TRY(pfx_int_blur_with_selection_dev(ctx, ctx->st_in.p, ctx->st_out.p, w, h, sigma, mask, d_mask));
    return pfx_unstage(ctx, dst, ctx->st_out, pfx_img_bytes(w, h));
}

} // extern "C"

// blur_with_selection (ref: src/ops/filters.rs:141-207) on device-resident images.  The reference blurs the
// selection's bounding box padded by the kernel radius *as its own image* (clamp-to-edge happens at the crop border)
// and copies back where mask > 0; the crop is reproduced exactly.  `mask_host` is scanned for the bounding box on the
// host (like the reference), `d_mask` is the same mask on the device.
int pfx_int_blur_with_selection_dev(pfx_ctx* ctx, const void* d_src, void* d_dst, uint32_t w, uint32_t h, float sigma,
                                    const uint8_t* mask, const void* d_mask)
{
    if (!mask) return pfx_gaussian_blur_dev(ctx, d_src, d_dst, w, h, sigma, nullptr);
    struct { void* p; } in{const_cast<void*>(d_src)}, out{d_dst};
    {
        // bounding box of mask > 0 (filters.rs:150-163).  Per row: the first and the last non-zero byte, found 8 bytes at a time — the
        // byte-by-byte scan with four min / max per selected pixel took tens of milliseconds on an 8K mask, more than the blur
        uint32_t min_x = w, min_y = h, max_x = 0, max_y = 0;
        for (uint32_t y = 0; y < h; ++y) {
            const uint8_t* row = mask + (size_t)y * w;
            uint32_t a = 0;
            while (a + 8 <= w) { uint64_t v; std::memcpy(&v, row + a, 8); if (v) break; a += 8; }
            while (a < w && row[a] == 0) ++a;
            if (a == w) continue; // nothing selected in this row
            uint32_t b = w;
            while (b >= a + 8) { uint64_t v; std::memcpy(&v, row + b - 8, 8); if (v) break; b -= 8; }
            while (b > a && row[b - 1] == 0) --b;
            min_x = std::min(min_x, a); max_x = std::max(max_x, b - 1);
            min_y = std::min(min_y, y); max_y = std::max(max_y, y);
        }
        if (min_x > max_x || min_y > max_y) { // nothing selected: flat.clone()
            PFX_HIP(ctx, hipMemcpyAsync(out.p, in.p, pfx_img_bytes(w, h), hipMemcpyDeviceToDevice, ctx->stream));
        } else {
            const float padf = ceilf(sigma * 3.0f);
            const uint32_t pad = pfx_f32_as_u32(padf);
            const uint32_t cx0 = min_x > pad ? min_x - pad : 0, cy0 = min_y > pad ? min_y - pad : 0;
            const uint32_t cx1 = (uint32_t)std::min<uint64_t>((uint64_t)max_x + 1 + pad, w);
            const uint32_t cy1 = (uint32_t)std::min<uint64_t>((uint64_t)max_y + 1 + pad, h);
            const uint32_t cw = cx1 - cx0, ch = cy1 - cy0;
            PFX_TRY(pfx_reserve(ctx, ctx->st_aux, pfx_img_bytes(cw, ch)));
            PFX_TRY(pfx_reserve(ctx, ctx->st_aux2, pfx_img_bytes(w, h)));
            PFX_HIP(ctx, hipMemcpy2DAsync(ctx->st_aux.p, (size_t)cw * 4, (const uint8_t*)in.p + ((size_t)cy0 * w + cx0) * 4,
                                          (size_t)w * 4, (size_t)cw * 4, ch, hipMemcpyDeviceToDevice, ctx->stream));
            // blurred crop -> st_aux2 (the H pass reads its source while the V pass writes the destination)
            PFX_TRY(pfx_gaussian_blur_dev(ctx, ctx->st_aux.p, ctx->st_aux2.p, cw, ch, sigma, nullptr));
            // paste the blurred crop over a copy of the source, then select by mask
            PFX_HIP(ctx, hipMemcpyAsync(out.p, in.p, pfx_img_bytes(w, h), hipMemcpyDeviceToDevice, ctx->stream));
            PFX_HIP(ctx, hipMemcpy2DAsync((uint8_t*)out.p + ((size_t)cy0 * w + cx0) * 4, (size_t)w * 4, ctx->st_aux2.p,
                                          (size_t)cw * 4, (size_t)cw * 4, ch, hipMemcpyDeviceToDevice, ctx->stream));
            PFX_HIP(ctx, pfxk_select_by_mask(ctx->stream, (const uint8_t*)in.p, (const uint8_t*)out.p,
                                             (const uint8_t*)d_mask, (uint8_t*)out.p, w, h));
        }
    }
    return PFX_OK;
}

extern "C" {

int pfx_blur_rgba(pfx_ctx* ctx, const uint8_t* src, uint8_t* dst, uint32_t w, uint32_t h, float sigma)
{
    return pfx_gaussian_blur_core(ctx, src, dst, w, h, sigma, nullptr);
}

int pfx_box_blur_core(pfx_ctx* ctx, const uint8_t* src, uint8_t* dst, uint32_t w, uint32_t h, float radius, const uint8_t* mask)
{
    PFX_TRY(check_img(ctx, "pfx_box_blur_core", false, src, dst, w, h));
    const void* d_mask;
    PFX_TRY(stage_in(ctx, src, mask, w, h, &d_mask));
    PFX_TRY(pfx_box_blur_dev(ctx, ctx->st_in.p, ctx->st_out.p, w, h, radius, d_mask, nullptr));
    return pfx_unstage(ctx, dst, ctx->st_out, pfx_img_bytes(w, h));
}

int pfx_median_core(pfx_ctx* ctx, const uint8_t* src, uint8_t* dst, uint32_t w, uint32_t h, uint32_t radius, const uint8_t* mask)
{
    PFX_TRY(check_img(ctx, "pfx_median_core", false, src, dst, w, h));
    const void* d_mask;
    PFX_TRY(stage_in(ctx, src, mask, w, h, &d_mask));
    PFX_TRY(pfx_median_dev(ctx, ctx->st_in.p, ctx->st_out.p, w, h, radius, d_mask));
    return pfx_unstage(ctx, dst, ctx->st_out, pfx_img_bytes(w, h));
}

int pfx_median_rgba(pfx_ctx* ctx, const uint8_t* src, uint8_t* dst, uint32_t w, uint32_t h, uint32_t radius)
{
    return pfx_median_core(ctx, src, dst, w, h, radius, nullptr);
}

int pfx_pixelate_core(pfx_ctx* ctx, const uint8_t* src, uint8_t* dst, uint32_t w, uint32_t h, uint32_t block_size, const uint8_t* mask)
{
    PFX_TRY(check_img(ctx, "pfx_pixelate_core", false, src, dst, w, h));
    const void* d_mask;
    PFX_TRY(stage_in(ctx, src, mask, w, h, &d_mask));
    PFX_TRY(pfx_pixelate_dev(ctx, ctx->st_in.p, ctx->st_out.p, w, h, block_size, d_mask));
    return pfx_unstage(ctx, dst, ctx->st_out, pfx_img_bytes(w, h));
}

int pfx_adjust(pfx_ctx* ctx, const uint8_t* src, uint8_t* dst, uint32_t w, uint32_t h, int op, const float* params,
               uint32_t n_params, const uint8_t* lut, const uint8_t* mask, int sparse_mode)
{
    PFX_TRY(check_img(ctx, "pfx_adjust", false, src, dst, w, h));
    const void* d_mask;
    PFX_TRY(stage_in(ctx, src, mask, w, h, &d_mask));
    PFX_TRY(pfx_adjust_dev(ctx, ctx->st_in.p, ctx->st_out.p, w, h, op, params, n_params, lut, d_mask, sparse_mode));
    return pfx_unstage(ctx, dst, ctx->st_out, pfx_img_bytes(w, h));
}

int pfx_brightness_contrast_rgba(pfx_ctx* ctx, const uint8_t* src, uint8_t* dst, uint32_t w, uint32_t h, float brightness, float contrast)
{
    const float p[2] = {brightness, contrast};
    return pfx_adjust(ctx, src, dst, w, h, PFX_OP_BRIGHTNESS_CONTRAST, p, 2, nullptr, nullptr, PFX_DENSE);
}

int pfx_hsl_rgba(pfx_ctx* ctx, const uint8_t* src, uint8_t* dst, uint32_t w, uint32_t h, float hue, float sat, float light)
{
    const float p[3] = {hue, sat, light};
    return pfx_adjust(ctx, src, dst, w, h, PFX_OP_HSL, p, 3, nullptr, nullptr, PFX_DENSE);
}

int pfx_invert_rgba(pfx_ctx* ctx, const uint8_t* src, uint8_t* dst, uint32_t w, uint32_t h)
{
    return pfx_adjust(ctx, src, dst, w, h, PFX_OP_INVERT, nullptr, 0, nullptr, nullptr, PFX_DENSE);
}

int pfx_rhai_adjust(pfx_ctx* ctx, uint8_t* pixels_inout, uint32_t w, uint32_t h, int op, const float* params, uint32_t n_params)
{
    PFX_TRY(check_inout(ctx, "pfx_rhai_adjust", pixels_inout, w, h));
    void* d_pixels;
    PFX_TRY(pfx_stage(ctx, ctx->st_in, pixels_inout, pfx_img_bytes(w, h), &d_pixels));
    PFX_TRY(pfx_rhai_adjust_dev(ctx, d_pixels, w, h, op, params, n_params));
    return pfx_unstage(ctx, pixels_inout, ctx->st_in, pfx_img_bytes(w, h));
}

int pfx_auto_levels(pfx_ctx* ctx, const uint8_t* src, uint8_t* dst, uint32_t w, uint32_t h, const uint8_t* mask)
{
    PFX_TRY(check_img(ctx, "pfx_auto_levels", false, src, dst, w, h));
    const void* d_mask;
    PFX_TRY(stage_in(ctx, src, mask, w, h, &d_mask));
    PFX_TRY(pfx_reserve(ctx, ctx->d_misc, 64));
    {
        pfx_timer t(ctx, "minmax");
        PFX_HIP(ctx, pfxk_minmax_rgb(ctx->stream, (const uint8_t*)ctx->st_in.p, (const uint8_t*)d_mask, w, h, (uint32_t*)ctx->d_misc.p));
    }
    uint32_t mm[6];
    PFX_TRY(pfx_d2h(ctx, mm, ctx->d_misc.p, sizeof mm));
    PFX_TRY(pfx_sync(ctx));
    uint8_t luts[1024];
    for (int c = 0; c < 3; ++c) pfx_build_stretch_lut((uint8_t)mm[c * 2], (uint8_t)mm[c * 2 + 1], luts + c * 256);
    for (int i = 0; i < 256; ++i) luts[768 + i] = (uint8_t)i;
    // auto_levels writes through from_rgba_image (adjustments.rs:230-232) => FROM_FLAT
    PFX_TRY(pfx_adjust_dev(ctx, ctx->st_in.p, ctx->st_out.p, w, h, PFX_OP_LUT_RGBA, nullptr, 0, luts, d_mask, PFX_FROM_FLAT));
    return pfx_unstage(ctx, dst, ctx->st_out, pfx_img_bytes(w, h));
}

int pfx_blend_pixels(pfx_ctx* ctx, const uint8_t* base, const uint8_t* top, uint8_t* dst, size_t n_pixels, uint8_t blend_mode, float opacity)
{
    const size_t bytes = n_pixels * 4;
    PFX_TRY(pfx_check_args(ctx, "pfx_blend_pixels", false, {{base, bytes, PFX_ARG_IN, "base"}, {top, bytes, PFX_ARG_IN, "top"}, {dst, bytes, PFX_ARG_STAGED_OUT, "dst"}}));
    PFX_REQUIRE(ctx, n_pixels, "pfx_blend_pixels: no pixels");
    void *d_base, *d_top, *d_dst;
    PFX_TRY(pfx_stage(ctx, ctx->st_in, base, bytes, &d_base));
    PFX_TRY(pfx_stage(ctx, ctx->st_aux, top, bytes, &d_top));
    PFX_TRY(pfx_stage(ctx, ctx->st_out, nullptr, bytes, &d_dst));
    PFX_HIP(ctx, pfxk_blend_arrays(ctx->stream, (const uint8_t*)d_base, (const uint8_t*)d_top, (uint8_t*)d_dst, n_pixels, blend_mode > 24 ? 0u : blend_mode, opacity,
                                   opacity_allows_fast_div(opacity) ? 1 : 0));
    return pfx_unstage(ctx, dst, ctx->st_out, bytes);
}

int pfx_warp_displacement(pfx_ctx* ctx, const uint8_t* src, uint32_t sw, uint32_t sh, const float* disp_xy, uint32_t w, uint32_t h, uint8_t* dst)
{
    PFX_TRY(check_warp(ctx, "pfx_warp_displacement", false, src, sw, sh, disp_xy, w, h, dst));
    void *d_src, *d_disp, *d_dst;
    PFX_TRY(pfx_stage(ctx, ctx->st_in, src, pfx_img_bytes(sw, sh), &d_src));
    PFX_TRY(pfx_stage(ctx, ctx->st_out, nullptr, pfx_img_bytes(w, h), &d_dst));
    PFX_TRY(pfx_stage(ctx, ctx->st_tmp, disp_xy, (size_t)w * h * 8, &d_disp));
    PFX_TRY(pfx_warp_displacement_dev(ctx, d_src, sw, sh, d_disp, w, h, d_dst));
    return pfx_unstage(ctx, dst, ctx->st_out, pfx_img_bytes(w, h));
}

// GpuLiquifyPipeline keeps the source texture across warp_into calls until invalidate_source (ref: src/gpu/compute/liquify.rs:166-176):
// an interactive Liquify session re-sends only the displacement field
int pfx_warp_set_source(pfx_ctx* ctx, const uint8_t* src, uint32_t sw, uint32_t sh)
{
    PFX_TRY(pfx_check_dims(ctx, "pfx_warp_set_source", sw, sh));
    PFX_TRY(pfx_check_args(ctx, "pfx_warp_set_source", false, {{src, pfx_img_bytes(sw, sh), PFX_ARG_IN, "src"}}));
    ctx->warp_src_w = ctx->warp_src_h = 0;
    PFX_TRY(pfx_reserve(ctx, ctx->warp_src, pfx_img_bytes(sw, sh)));
    PFX_TRY(pfx_h2d(ctx, ctx->warp_src.p, src, pfx_img_bytes(sw, sh)));
    PFX_TRY(pfx_sync(ctx)); // the host buffer may be released after the call
    ctx->warp_src_w = sw; ctx->warp_src_h = sh;
    return PFX_OK;
}

int pfx_warp_invalidate_source(pfx_ctx* ctx)
{
    if (!ctx) return PFX_ERR_INVALID;
    ctx->warp_src_w = ctx->warp_src_h = 0;
    return PFX_OK;
}

int pfx_warp_displacement_cached(pfx_ctx* ctx, const float* disp_xy, uint32_t w, uint32_t h, uint8_t* dst)
{
    PFX_TRY(pfx_check_dims(ctx, "pfx_warp_displacement_cached", w, h));
    PFX_TRY(pfx_check_args(ctx, "pfx_warp_displacement_cached", false, {{disp_xy, 0, PFX_ARG_IN, "disp_xy"}, {dst, pfx_img_bytes(w, h), PFX_ARG_STAGED_OUT, "dst"}}));
    PFX_REQUIRE(ctx, ctx->warp_src_w != 0, "pfx_warp_displacement_cached: no source (pfx_warp_set_source, or it was invalidated)");
    void *d_disp, *d_dst;
    PFX_TRY(pfx_stage(ctx, ctx->st_out, nullptr, pfx_img_bytes(w, h), &d_dst));
    PFX_TRY(pfx_stage(ctx, ctx->st_tmp, disp_xy, (size_t)w * h * 8, &d_disp));
    PFX_TRY(pfx_warp_displacement_dev(ctx, ctx->warp_src.p, ctx->warp_src_w, ctx->warp_src_h, d_disp, w, h, d_dst));
    return pfx_unstage(ctx, dst, ctx->st_out, pfx_img_bytes(w, h));
}

int pfx_mesh_displacement(pfx_ctx* ctx, const float* orig_pts_xy, const float* deformed_pts_xy, uint32_t cols, uint32_t rows,
                          uint32_t w, uint32_t h, float* disp_xy_out)
{
    PFX_TRY(pfx_check_dims(ctx, "pfx_mesh_displacement", w, h));
    PFX_TRY(pfx_check_args(ctx, "pfx_mesh_displacement", false, {{disp_xy_out, (size_t)w * h * 8, PFX_ARG_STAGED_OUT, "disp_xy_out"}}));
    void* d_disp;
    PFX_TRY(pfx_stage(ctx, ctx->st_tmp, nullptr, (size_t)w * h * 8, &d_disp));
    PFX_TRY(pfx_mesh_displacement_dev(ctx, orig_pts_xy, deformed_pts_xy, cols, rows, w, h, d_disp));
    return pfx_unstage(ctx, disp_xy_out, ctx->st_tmp, (size_t)w * h * 8);
}

int pfx_warp_mesh_catmull_rom(pfx_ctx* ctx, const uint8_t* src, const float* orig_pts_xy, const float* deformed_pts_xy,
                              uint32_t cols, uint32_t rows, uint32_t w, uint32_t h, uint8_t* dst)
{
    PFX_TRY(check_img(ctx, "pfx_warp_mesh_catmull_rom", false, src, dst, w, h));
    PFX_REQUIRE(ctx, orig_pts_xy != nullptr, "warp_mesh_catmull_rom needs the original grid (transform.rs:1743)");
    const void* d_mask;
    PFX_TRY(stage_in(ctx, src, nullptr, w, h, &d_mask));
    PFX_TRY(pfx_warp_mesh_catmull_rom_dev(ctx, ctx->st_in.p, orig_pts_xy, deformed_pts_xy, cols, rows, w, h, ctx->st_out.p));
    return pfx_unstage(ctx, dst, ctx->st_out, pfx_img_bytes(w, h));
}

int pfx_brush_stamps_ex(pfx_ctx* ctx, uint8_t* target_inout, uint32_t w, uint32_t h, const pfx_brush* brush, const pfx_brush_dynamics* dyn,
                        const float* points_xy, uint32_t n_points, const uint8_t* selection)
{
    PFX_TRY(check_inout(ctx, "pfx_brush_stamps", target_inout, w, h));
    const void* d_sel;
    PFX_TRY(stage_in(ctx, target_inout, selection, w, h, &d_sel));
    PFX_TRY(pfx_brush_stamps_ex_dev(ctx, ctx->st_in.p, w, h, brush, dyn, points_xy, n_points, d_sel));
    return pfx_unstage(ctx, target_inout, ctx->st_in, pfx_img_bytes(w, h));
}

int pfx_brush_stamps(pfx_ctx* ctx, uint8_t* target_inout, uint32_t w, uint32_t h, const pfx_brush* brush, const float* points_xy,
                     uint32_t n_points, const uint8_t* selection)
{
    return pfx_brush_stamps_ex(ctx, target_inout, w, h, brush, nullptr, points_xy, n_points, selection);
}

int pfx_brush_line_ex(pfx_ctx* ctx, uint8_t* target_inout, uint32_t w, uint32_t h, const pfx_brush* brush, const pfx_brush_dynamics* dyn, float x0,
                      float y0, float x1, float y1, const uint8_t* selection)
{
    PFX_TRY(check_inout(ctx, "pfx_brush_line", target_inout, w, h));   // before the "no stamps" early return: bad arguments are bad whatever the line
    PFX_REQUIRE(ctx, brush != nullptr, "pfx_brush_line: null brush");
    std::vector<float> pts;
    pfx_host_line_points(x0, y0, x1, y1, w, h, pts);
    if (pts.empty()) return PFX_OK;
    return pfx_brush_stamps_ex(ctx, target_inout, w, h, brush, dyn, pts.data(), (uint32_t)(pts.size() / 2), selection);
}

int pfx_brush_line(pfx_ctx* ctx, uint8_t* target_inout, uint32_t w, uint32_t h, const pfx_brush* brush, float x0, float y0,
                   float x1, float y1, const uint8_t* selection)
{
    return pfx_brush_line_ex(ctx, target_inout, w, h, brush, nullptr, x0, y0, x1, y1, selection);
}

// rebuild_tip_mask (brush_render.rs:404-528), host side like the reference
uint32_t pfx_brush_tip_rescale(const uint8_t* src, uint32_t src_size, float brush_size, float hardness, uint8_t* out)
{
    if (!src || !out || src_size == 0) return 0;
    auto u8 = [](float v) -> uint8_t { return !(v > 0.0f) ? 0 : (v >= 255.0f ? 255 : (uint8_t)(int)v); };
    const uint32_t dst = std::max(pfx_f32_as_u32(ceilf(brush_size)), 1u);
    const float scale = (float)src_size / (float)dst;
    for (uint32_t dy = 0; dy < dst; ++dy)
        for (uint32_t dx = 0; dx < dst; ++dx) {
            const float sx = (float)dx * scale, sy = (float)dy * scale;
            const uint32_t sx0 = pfx_f32_as_u32(floorf(sx)), sy0 = pfx_f32_as_u32(floorf(sy));
            const uint32_t sx1 = std::min(sx0 + 1, src_size - 1), sy1 = std::min(sy0 + 1, src_size - 1);
            const float fx = sx - (float)sx0, fy = sy - (float)sy0;
            const float v00 = src[sy0 * src_size + sx0], v10 = src[sy0 * src_size + sx1], v01 = src[sy1 * src_size + sx0], v11 = src[sy1 * src_size + sx1];
            const float top = v00 * (1.0f - fx) + v10 * fx, bot = v01 * (1.0f - fx) + v11 * fx;
            out[dy * dst + dx] = u8(fminf(roundf(top * (1.0f - fy) + bot * fy), 255.0f));
        }
    if (hardness < 0.99f) { // hardness as a contrast modifier
        const float threshold = (1.0f - hardness) * 0.6f, range = 1.0f - threshold;
        for (uint32_t i = 0; i < dst * dst; ++i)
            out[i] = u8(roundf(pfx_clampf(((float)out[i] / 255.0f - threshold) / range, 0.0f, 1.0f) * 255.0f));
    }
    if (dst < src_size && dst >= 3) { // anti-alias box passes when downscaling
        const float ratio = (float)src_size / (float)dst;
        const int passes = ratio > 4.0f ? 2 : (ratio > 1.5f ? 1 : 0);
        std::vector<uint8_t> tmp((size_t)dst * dst);
        for (int p = 0; p < passes; ++p) {
            for (uint32_t y = 0; y < dst; ++y)
                for (uint32_t x = 0; x < dst; ++x) {
                    uint32_t sum = out[y * dst + x], count = 1;
                    if (x > 0) { sum += out[y * dst + x - 1]; ++count; }
                    if (x + 1 < dst) { sum += out[y * dst + x + 1]; ++count; }
                    tmp[y * dst + x] = (uint8_t)(sum / count);
                }
            for (uint32_t y = 0; y < dst; ++y)
                for (uint32_t x = 0; x < dst; ++x) {
                    uint32_t sum = tmp[y * dst + x], count = 1;
                    if (y > 0) { sum += tmp[(y - 1) * dst + x]; ++count; }
                    if (y + 1 < dst) { sum += tmp[(y + 1) * dst + x]; ++count; }
                    out[y * dst + x] = (uint8_t)(sum / count);
                }
        }
    }
    return dst;
}

int pfx_brush_commit(pfx_ctx* ctx, uint8_t* layer_inout, const uint8_t* preview, uint32_t w, uint32_t h, uint8_t blend_mode,
                     int is_eraser, const uint8_t* selection)
{
    PFX_TRY(pfx_check_dims(ctx, "pfx_brush_commit", w, h));
    PFX_TRY(pfx_check_args(ctx, "pfx_brush_commit", false, {{layer_inout, pfx_img_bytes(w, h), PFX_ARG_STAGED_OUT, "layer_inout"}, {preview, pfx_img_bytes(w, h), PFX_ARG_IN, "preview"}}));
    const void* d_sel;
    PFX_TRY(stage_in(ctx, layer_inout, selection, w, h, &d_sel));
    PFX_TRY(pfx_h2d(ctx, ctx->st_out.p, preview, pfx_img_bytes(w, h)));
    PFX_HIP(ctx, pfxk_brush_commit(ctx->stream, (uint8_t*)ctx->st_in.p, (const uint8_t*)ctx->st_out.p, (const uint8_t*)d_sel, w, h,
                                   blend_mode > 24 ? 0u : blend_mode, is_eraser));
    return pfx_unstage(ctx, layer_inout, ctx->st_in, pfx_img_bytes(w, h));
}

int pfx_tiled_roundtrip(pfx_ctx* ctx, const uint8_t* src, uint8_t* dst, uint32_t w, uint32_t h)
{
    PFX_TRY(check_img(ctx, "pfx_tiled_roundtrip", false, src, dst, w, h));
    const void* d_mask;
    PFX_TRY(stage_in(ctx, src, nullptr, w, h, &d_mask));
    PFX_TRY(pfx_tiled_roundtrip_dev(ctx, ctx->st_in.p, ctx->st_out.p, w, h));
    return pfx_unstage(ctx, dst, ctx->st_out, pfx_img_bytes(w, h));
}

int pfx_chunk_populated(pfx_ctx* ctx, const uint8_t* src, uint32_t w, uint32_t h, uint8_t* populated)
{
    PFX_TRY(pfx_check_dims(ctx, "pfx_chunk_populated", w, h));
    const size_t nchunks = (size_t)((w + 63) / 64) * ((h + 63) / 64);
    PFX_TRY(pfx_check_args(ctx, "pfx_chunk_populated", false, {{src, pfx_img_bytes(w, h), PFX_ARG_IN, "src"}, {populated, nchunks, PFX_ARG_STAGED_OUT, "populated"}}));
    void *d_src, *d_chunks;
    PFX_TRY(pfx_stage(ctx, ctx->st_in, src, pfx_img_bytes(w, h), &d_src));
    PFX_TRY(pfx_stage(ctx, ctx->d_chunks, nullptr, nchunks, &d_chunks));
    PFX_HIP(ctx, pfxk_chunk_populated(ctx->stream, (const uint8_t*)d_src, w, h, (uint8_t*)d_chunks));
    return pfx_unstage(ctx, populated, ctx->d_chunks, nchunks);
}

int pfx_int_warp_last(pfx_ctx* ctx, int which)
{
    if (!ctx) return -1;
    switch (which) {
        case 0: return ctx->last_warp.flags;
        case 1: return ctx->last_warp.flags < 0 ? -1 : (int)ctx->last_warp.gx;
        case 2: return ctx->last_warp.flags < 0 ? -1 : (int)ctx->last_warp.gy;
        case 3: return ctx->last_dab_launch;
        case 4: return ctx->last_dab_chunks;
        default: return -1;
    }
}

int pfx_int_warp_info(int which) { return pfxk_warp_info(which); }

int pfx_tune(pfx_ctx* ctx, const char* key, int value)
{
    if (!ctx || !key) return PFX_ERR_INVALID;
    if (std::strcmp(key, "gauss_v_cfg") == 0) { pfxk_gauss_set_v_config(value); return PFX_OK; }
    if (std::strcmp(key, "gauss_mfma_segments") == 0) { pfxk_gauss_set_mfma_segments(value); return PFX_OK; }
    if (std::strcmp(key, "gauss_parts") == 0) { pfxk_gauss_set_mfma_parts(value / 10, value % 10); return PFX_OK; } // f16 pieces per weight, per horizontal result: 22, 12, 11
    if (std::strcmp(key, "flatten_variant") == 0 || std::strncmp(key, "dle_", 4) == 0 || std::strcmp(key, "chunk_start") == 0) return pfx_flatten_tune(ctx, key, value);   // the knobs live in pfx_flatten.cpp
    if (std::strncmp(key, "median_", 7) == 0 || std::strncmp(key, "box_", 4) == 0) return pfx_stencil_tune(ctx, key, value);   // the knobs live in pfx_stencil.cpp
    if (std::strcmp(key, "outline_bits") == 0) { ctx->outline_bits = value != 0; return PFX_OK; }
    if (std::strcmp(key, "brush_binning") == 0) { ctx->brush_binning = value != 0; return PFX_OK; }   // 0: long strokes on the bounding-box kernel too
    if (std::strcmp(key, "gauss_fused_exact") == 0) { pfxk_gauss_set_fused_exact(value); return PFX_OK; }  // 0 = the bit-exact Gaussian always through the two kernels
    if (std::strcmp(key, "mesh_xcd") == 0) { pfxk_warp_set_mesh_xcd(value); return PFX_OK; }            // 0 = the fused mesh warp's plain 2-D tile order
    if (std::strcmp(key, "warp_buf32") == 0) { pfxk_warp_set_buf32(value); return PFX_OK; }            // 0 = both warps' 64-bit-address forms whatever the source's size (the tests' way into them)
    if (std::strcmp(key, "shadow_plane") == 0) { ctx->shadow_plane_blur = value != 0; return PFX_OK; } // drop shadow: blur the alpha plane (1) or the RGBA expansion (0); identical results
    if (std::strcmp(key, "gauss_cols64") == 0) { pfxk_gauss_set_mfma_cols64(value); return PFX_OK; } // matrix-core Gaussian at 8 K blocks: 64-column (1) / 32-column (0) strips, same bits
    if (std::strcmp(key, "chain_fuse_heavy") == 0) { ctx->chain_fuse_heavy = value != 0; return PFX_OK; } // pfx_chain_dev: HSL / vibrance in a Gaussian's store too (measured: no gain)
    if (std::strcmp(key, "chain_mfma") == 0) { ctx->chain_mfma_epilogue = value != 0; return PFX_OK; } // pfx_chain_dev: the chain in the matrix-core Gaussian's store (1) or as its own launch (0)
    if (std::strcmp(key, "gauss_fast_effects") == 0) { ctx->gauss_fast_effects = value != 0; return PFX_OK; } // sharpen / glow / shadow on the default-mode Gaussian (+-amount LSB)
    if (std::strcmp(key, "resize_two_pass") == 0) { ctx->resize_two_pass = value != 0; return PFX_OK; } // A/B and the parity test of the fused kernel
    return pfx_fail(ctx, PFX_ERR_INVALID, "pfx_tune: unknown key %s", key);
}

int pfx_selftest_division(pfx_ctx* ctx, uint64_t seed, uint32_t n_millions, uint64_t* mismatches)
{
    if (!ctx || !mismatches) return PFX_ERR_INVALID;
    PFX_TRY(pfx_use(ctx));
    PFX_TRY(pfx_reserve(ctx, ctx->d_misc, 64));
    PFX_HIP(ctx, hipMemsetAsync(ctx->d_misc.p, 0, 8, ctx->stream));
    const uint32_t blocks = 1024, iters = (uint32_t)(((uint64_t)n_millions * 1000000ull + blocks * 256ull - 1) / (blocks * 256ull));
    PFX_HIP(ctx, pfxk_rdiv_check(ctx->stream, seed, blocks, iters, (unsigned long long*)ctx->d_misc.p));
    unsigned long long bad = 0;
    PFX_TRY(pfx_d2h(ctx, &bad, ctx->d_misc.p, 8));
    PFX_TRY(pfx_sync(ctx));
    *mismatches = bad;
    return PFX_OK;
}

int pfx_selftest_division_range(pfx_ctx* ctx, uint64_t seed, uint32_t n_millions, int32_t num_exp_lo, int32_t num_exp_hi, int32_t den_exp_lo,
                                int32_t den_exp_hi, uint64_t* mismatches)
{
    if (!ctx || !mismatches) return PFX_ERR_INVALID;
    PFX_TRY(pfx_use(ctx));
    // normal f32 exponents only, and a pair count that one launch finishes in seconds
    PFX_REQUIRE(ctx, num_exp_lo >= -126 && num_exp_hi <= 127 && num_exp_lo <= num_exp_hi && den_exp_lo >= -126 && den_exp_hi <= 127 && den_exp_lo <= den_exp_hi,
                "pfx_selftest_division_range: exponents must lie in -126 .. 127, lo <= hi");
    PFX_REQUIRE(ctx, n_millions >= 1 && n_millions <= 4096, "pfx_selftest_division_range: 1 .. 4096 million pairs");
    PFX_TRY(pfx_reserve(ctx, ctx->d_misc, 64));
    PFX_HIP(ctx, hipMemsetAsync(ctx->d_misc.p, 0, 8, ctx->stream));
    const uint32_t blocks = 1024, iters = (uint32_t)(((uint64_t)n_millions * 1000000ull + blocks * 256ull - 1) / (blocks * 256ull));
    PFX_HIP(ctx, pfxk_rdiv_check_range(ctx->stream, seed, blocks, iters, (uint32_t)(num_exp_lo + 127), (uint32_t)(num_exp_hi + 127), (uint32_t)(den_exp_lo + 127),
                                       (uint32_t)(den_exp_hi + 127), (unsigned long long*)ctx->d_misc.p));
    unsigned long long bad = 0;
    PFX_TRY(pfx_d2h(ctx, &bad, ctx->d_misc.p, 8));
    PFX_TRY(pfx_sync(ctx));
    *mismatches = bad;
    return PFX_OK;
}

int pfx_selftest_unorm_store(pfx_ctx* ctx, uint64_t* mismatches)
{
    if (!ctx || !mismatches) return PFX_ERR_INVALID;
    PFX_TRY(pfx_use(ctx));
    PFX_TRY(pfx_reserve(ctx, ctx->d_misc, 2048));
    PFX_HIP(ctx, hipMemsetAsync(ctx->d_misc.p, 0, 2048, ctx->stream));
    PFX_HIP(ctx, pfxk_unorm_store_check(ctx->stream, (uint8_t*)ctx->d_misc.p, (unsigned long long*)((uint8_t*)ctx->d_misc.p + 1024)));
    unsigned long long bad = 0;
    PFX_TRY(pfx_d2h(ctx, &bad, (uint8_t*)ctx->d_misc.p + 1024, sizeof bad));
    PFX_TRY(pfx_sync(ctx));
    *mismatches = bad;
    return PFX_OK;
}

int pfx_selftest_round_pack(pfx_ctx* ctx, uint64_t* mismatches, uint64_t* signalling_nan_mismatches)
{
    if (!ctx || !mismatches) return PFX_ERR_INVALID;
    PFX_TRY(pfx_use(ctx));
    PFX_TRY(pfx_reserve(ctx, ctx->d_misc, 64));
    PFX_HIP(ctx, hipMemsetAsync(ctx->d_misc.p, 0, 16, ctx->stream));
    PFX_HIP(ctx, pfxk_round_pack_check(ctx->stream, (unsigned long long*)ctx->d_misc.p));
    unsigned long long bad[2] = {0, 0};
    PFX_TRY(pfx_d2h(ctx, bad, ctx->d_misc.p, 16));
    PFX_TRY(pfx_sync(ctx));
    *mismatches = bad[0];
    if (signalling_nan_mismatches) *signalling_nan_mismatches = bad[1];
    return PFX_OK;
}

} // extern "C"
