// pfx_resize.cpp — C ABI of resize_image: `imageops::resize(&flat, new_w, new_h, filter)` (ref: src/ops/transform.rs:347-359,
// resize_image script function src/ops/scripting.rs:749-770, filter mapping :29-37,60-67).
//
// The sampling algorithm is the `image` crate's (0.25.9 per Cargo.lock; not part of the reference tree): per output sample a
// window of source samples around (o + 0.5) * ratio, kernel weights normalised by their f32 sum, vertical pass into f32 then
// horizontal pass with clamp and round-to-nearest.  The per-axis weight tables are built on the host (pfx_resample.h, shared
// with the matte's one-channel resize) and the two passes run in k_resize.hip.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "pfx_internal.h"
#include "pfx_resample.h"

namespace {

using pfx_resample::AxisTable;
using pfx_resample::build_axis;

// what the resamplers declare: a w x h source and a dw x dh destination.  On the device the two never share a byte; the host tier works on staged copies
int check_resample(pfx_ctx* ctx, const char* who, bool dev, const void* src, uint32_t w, uint32_t h, const void* dst, uint32_t dw, uint32_t dh)
{
    const size_t src_bytes = std::max<size_t>(pfx_img_bytes(w, h), 1);   // pfx_affine_transform_dev's empty source is still a pointer that dst may not contain
    return pfx_check_args(ctx, who, dev, {{src, src_bytes, PFX_ARG_IN, "src"}, {dst, pfx_img_bytes(dw, dh), dev ? PFX_ARG_OUT : PFX_ARG_STAGED_OUT, "dst"}});
}

// the host tier: src staged in st_in, the `_dev` twin into st_out, dst written last
template <class F>
int staged(pfx_ctx* ctx, const uint8_t* src, size_t src_bytes, uint8_t* dst, size_t dst_bytes, F&& dev_call)
{
    void *d_src, *d_dst;
    PFX_TRY(pfx_stage(ctx, ctx->st_in, src, src_bytes, &d_src));
    PFX_TRY(pfx_stage(ctx, ctx->st_out, nullptr, dst_bytes, &d_dst));
    PFX_TRY(dev_call(d_src, d_dst));
    return pfx_unstage(ctx, dst, ctx->st_out, dst_bytes);
}

} // namespace

extern "C" {

int pfx_int_resize_last(pfx_ctx* ctx, int which) { return !ctx ? -1 : (which == 0 ? ctx->last_resize_path : ctx->last_resize_span); }

int pfx_resize_image_dev(pfx_ctx* ctx, const void* src_dev, uint32_t w, uint32_t h, void* dst_dev, uint32_t new_w, uint32_t new_h, int filter)
{
    PFX_TRY(pfx_check_dims(ctx, "pfx_resize_image_dev", w, h));
    PFX_TRY(pfx_check_dims(ctx, "pfx_resize_image_dev", new_w, new_h));
    PFX_TRY(check_resample(ctx, "pfx_resize_image_dev", true, src_dev, w, h, dst_dev, new_w, new_h));
    PFX_REQUIRE(ctx, filter >= PFX_RESIZE_NEAREST && filter <= PFX_RESIZE_LANCZOS3, "pfx_resize_image_dev: unknown filter");
    if (new_w == w && new_h == h) { // the crate copies instead of resampling
        PFX_HIP(ctx, hipMemcpyAsync(dst_dev, src_dev, (size_t)w * h * 4, hipMemcpyDeviceToDevice, ctx->stream));
        ctx->last_resize_path = 0; ctx->last_resize_span = 0;
        return PFX_OK;
    }
    AxisTable v, hz;
    build_axis(h, new_h, filter, v);
    build_axis(w, new_w, filter, hz);
    PFX_REQUIRE(ctx, v.wts.size() < 0xffffffffull && hz.wts.size() < 0xffffffffull, "pfx_resize_image_dev: weight table too large");
    std::vector<uint32_t> blob;
    const size_t n_u32 = pfx_resample::pack_axes(v, hz, blob);   // [v.left | v.count | v.off | h.left | h.count | h.off | v.wts | h.wts]
    PFX_TRY(pfx_reserve(ctx, ctx->fx_a, blob.size() * 4));
    PFX_TRY(pfx_h2d(ctx, ctx->fx_a.p, blob.data(), blob.size() * 4));
    PFX_HIP(ctx, hipStreamSynchronize(ctx->stream)); // `blob` is pageable host memory about to go out of scope
    // the widest source-column range one output tile's horizontal taps reach: decides between the fused kernel (vertical results in
    // LDS) and the two-pass path with its f32 intermediate in HBM (strong downscales)
    const uint32_t span_max = pfx_resample::span_max(hz, new_w, (uint32_t)pfxk_resize_tile_cols());
    const bool fused = (size_t)span_max * 8 * 16 <= 64u * 1024u && !ctx->resize_two_pass;
    if (!fused) PFX_TRY(pfx_reserve(ctx, ctx->st_tmp, (size_t)w * new_h * 16));
    ctx->last_resize_path = fused ? 1 : 2; ctx->last_resize_span = (int)span_max;
    const uint32_t* d = (const uint32_t*)ctx->fx_a.p;
    const float* dw = (const float*)(d + n_u32);
    pfx_timer t(ctx, "resize");
    PFX_HIP(ctx, pfxk_resize(ctx->stream, (const uint8_t*)src_dev, fused ? nullptr : (float*)ctx->st_tmp.p, (uint8_t*)dst_dev, d, d + new_h, d + 2 * (size_t)new_h,
                             dw, d + 3 * (size_t)new_h, d + 3 * (size_t)new_h + new_w, d + 3 * (size_t)new_h + 2 * (size_t)new_w, dw + v.wts.size(), w, h,
                             new_w, new_h, fused ? span_max : 0u));
    return PFX_OK;
}

// apply_affine (ref: src/ops/transform.rs:826-946): the homography is built and inverted on the host exactly as the reference does
int pfx_affine_transform_dev(pfx_ctx* ctx, const void* src_dev, uint32_t src_w, uint32_t src_h, void* dst_dev, uint32_t canvas_w, uint32_t canvas_h,
                             float rotation_z, float rotation_x, float rotation_y, float scale, float offset_x, float offset_y, int interpolation)
{
    PFX_TRY(pfx_check_dims(ctx, "pfx_affine_transform_dev", canvas_w, canvas_h));
    if (src_w && src_h) PFX_TRY(pfx_check_dims(ctx, "pfx_affine_transform_dev", src_w, src_h));   // an empty source has never been refused here (the host tier does)
    PFX_TRY(check_resample(ctx, "pfx_affine_transform_dev", true, src_dev, src_w, src_h, dst_dev, canvas_w, canvas_h));
    PFX_REQUIRE(ctx, interpolation == PFX_RESIZE_NEAREST || interpolation == PFX_RESIZE_BILINEAR, "pfx_affine_transform_dev: nearest or bilinear only");
    pfxk_affine_params P{};
    P.cx = (float)canvas_w * 0.5f;
    P.cy = (float)canvas_h * 0.5f;
    P.off_x = offset_x;
    P.off_y = offset_y;
    P.inv_scale = fabsf(scale) > 1e-6f ? 1.0f / scale : 1.0f;
    P.nearest = interpolation == PFX_RESIZE_NEAREST;
    const float focal = (float)std::max(canvas_w, canvas_h) * 1.5f;
    const float rad = 3.14159265358979323846f / 180.0f; // f32::to_radians
    const float az = rotation_z * rad, ax = rotation_x * rad, ay = rotation_y * rad;
    const float sz = sinf(az), cz = cosf(az), sxr = sinf(ax), cxr = cosf(ax), syr = sinf(ay), cyr = cosf(ay);
    const float r00 = cz * cyr, r01 = cz * syr * sxr - sz * cxr, r10 = sz * cyr, r11 = sz * syr * sxr + cz * cxr, r20 = -syr, r21 = cyr * sxr;
    const float a = focal * r00, b = focal * r01, c = 0.0f, d = focal * r10, e = focal * r11, f = 0.0f, g = r20, h = r21, i = focal;
    const float det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g); // invert_3x3, transform.rs:949-976
    if (fabsf(det) < 1e-12f) {
        const float id[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        std::memcpy(P.hi, id, sizeof id);
    } else {
        const float inv = 1.0f / det;
        P.hi[0] = (e * i - f * h) * inv; P.hi[1] = (c * h - b * i) * inv; P.hi[2] = (b * f - c * e) * inv;
        P.hi[3] = (f * g - d * i) * inv; P.hi[4] = (a * i - c * g) * inv; P.hi[5] = (c * d - a * f) * inv;
        P.hi[6] = (d * h - e * g) * inv; P.hi[7] = (b * g - a * h) * inv; P.hi[8] = (a * e - b * d) * inv;
    }
    pfx_timer t(ctx, "affine");
    PFX_HIP(ctx, pfxk_affine(ctx->stream, (const uint8_t*)src_dev, src_w, src_h, (uint8_t*)dst_dev, canvas_w, canvas_h, &P));
    return PFX_OK;
}

int pfx_affine_transform(pfx_ctx* ctx, const uint8_t* src, uint32_t src_w, uint32_t src_h, uint8_t* dst, uint32_t canvas_w, uint32_t canvas_h,
                         float rotation_z, float rotation_x, float rotation_y, float scale, float offset_x, float offset_y, int interpolation)
{
    PFX_TRY(pfx_check_dims(ctx, "pfx_affine_transform", src_w, src_h));
    PFX_TRY(pfx_check_dims(ctx, "pfx_affine_transform", canvas_w, canvas_h));
    PFX_TRY(check_resample(ctx, "pfx_affine_transform", false, src, src_w, src_h, dst, canvas_w, canvas_h));
    return staged(ctx, src, pfx_img_bytes(src_w, src_h), dst, pfx_img_bytes(canvas_w, canvas_h), [&](const void* s, void* d) {
        return pfx_affine_transform_dev(ctx, s, src_w, src_h, d, canvas_w, canvas_h, rotation_z, rotation_x, rotation_y, scale, offset_x, offset_y, interpolation);
    });
}

// flip / rotate one layer image (ref: src/ops/transform.rs flip_canvas_* / rotate_canvas_* = imageops::flip_* / rotate*)
int pfx_flip_rotate_dev(pfx_ctx* ctx, const void* src_dev, uint32_t w, uint32_t h, void* dst_dev, int op)
{
    PFX_TRY(pfx_check_dims(ctx, "pfx_flip_rotate_dev", w, h));
    PFX_TRY(check_resample(ctx, "pfx_flip_rotate_dev", true, src_dev, w, h, dst_dev, w, h));
    PFX_REQUIRE(ctx, op >= PFX_CANVAS_FLIP_HORIZONTAL && op <= PFX_CANVAS_ROTATE_180, "pfx_flip_rotate_dev: unknown operation");
    static const int mode_of[5] = {0, 1, 3, 4, 2}; // FLIP_H, FLIP_V, ROTATE_90CW, ROTATE_90CCW, ROTATE_180 -> k_script.hip permutation modes
    pfx_timer t(ctx, "permute");
    PFX_HIP(ctx, pfxk_permute(ctx->stream, (const uint8_t*)src_dev, (uint8_t*)dst_dev, mode_of[op], w, h));
    return PFX_OK;
}

int pfx_flip_rotate(pfx_ctx* ctx, const uint8_t* src, uint32_t w, uint32_t h, uint8_t* dst, int op)
{
    PFX_TRY(pfx_check_dims(ctx, "pfx_flip_rotate", w, h));
    PFX_TRY(check_resample(ctx, "pfx_flip_rotate", false, src, w, h, dst, w, h));
    return staged(ctx, src, pfx_img_bytes(w, h), dst, pfx_img_bytes(w, h), [&](const void* s, void* d) { return pfx_flip_rotate_dev(ctx, s, w, h, d, op); });
}

// resize_canvas(state, new_w, new_h, anchor, fill) for one layer image (ref: src/ops/transform.rs:382-424)
int pfx_resize_canvas_dev(pfx_ctx* ctx, const void* src_dev, uint32_t w, uint32_t h, void* dst_dev, uint32_t new_w, uint32_t new_h, uint32_t anchor_x,
                          uint32_t anchor_y, const uint8_t fill[4])
{
    PFX_TRY(pfx_check_dims(ctx, "pfx_resize_canvas_dev", new_w, new_h));
    PFX_REQUIRE(ctx, w && h, "pfx_resize_canvas_dev: bad image size");   // w * h has never been bounded here (the host tier does)
    PFX_TRY(check_resample(ctx, "pfx_resize_canvas_dev", true, src_dev, w, h, dst_dev, new_w, new_h));
    const int32_t off_x = anchor_x == 0 ? 0 : (anchor_x == 1 ? ((int32_t)new_w - (int32_t)w) / 2 : (int32_t)new_w - (int32_t)w);
    const int32_t off_y = anchor_y == 0 ? 0 : (anchor_y == 1 ? ((int32_t)new_h - (int32_t)h) / 2 : (int32_t)new_h - (int32_t)h);
    const uint32_t rgba = fill ? pfx_pack_rgba8(fill) : 0u;
    pfx_timer t(ctx, "resize_canvas");
    PFX_HIP(ctx, pfxk_recanvas(ctx->stream, (const uint8_t*)src_dev, (uint8_t*)dst_dev, w, h, new_w, new_h, off_x, off_y, rgba));
    return PFX_OK;
}

int pfx_resize_canvas(pfx_ctx* ctx, const uint8_t* src, uint32_t w, uint32_t h, uint8_t* dst, uint32_t new_w, uint32_t new_h, uint32_t anchor_x,
                      uint32_t anchor_y, const uint8_t fill[4])
{
    PFX_TRY(pfx_check_dims(ctx, "pfx_resize_canvas", w, h));
    PFX_TRY(pfx_check_dims(ctx, "pfx_resize_canvas", new_w, new_h));
    PFX_TRY(check_resample(ctx, "pfx_resize_canvas", false, src, w, h, dst, new_w, new_h));
    return staged(ctx, src, pfx_img_bytes(w, h), dst, pfx_img_bytes(new_w, new_h),
                  [&](const void* s, void* d) { return pfx_resize_canvas_dev(ctx, s, w, h, d, new_w, new_h, anchor_x, anchor_y, fill); });
}

int pfx_resize_image(pfx_ctx* ctx, const uint8_t* src, uint32_t w, uint32_t h, uint8_t* dst, uint32_t new_w, uint32_t new_h, int filter)
{
    PFX_TRY(pfx_check_dims(ctx, "pfx_resize_image", w, h));
    PFX_TRY(pfx_check_dims(ctx, "pfx_resize_image", new_w, new_h));
    PFX_TRY(check_resample(ctx, "pfx_resize_image", false, src, w, h, dst, new_w, new_h));
    return staged(ctx, src, pfx_img_bytes(w, h), dst, pfx_img_bytes(new_w, new_h),
                  [&](const void* s, void* d) { return pfx_resize_image_dev(ctx, s, w, h, d, new_w, new_h, filter); });
}

} // extern "C"
