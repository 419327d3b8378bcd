// k_overlay.hip — the floating selection (ref: src/ops/clipboard.rs), bit for bit: every f32 expression as the reference writes it, one rounding per operation (no
// contraction), IEEE division, round() half away from zero, `as u32` / `as i32` saturating and truncating.
//
//   sampler     what commit :2089-2125, apply_transformed_pixels_to_image :1212-1247, rasterize_for_clipboard :1091-1125 and render_preview's general path
//               :2257-2279 share: the pixel centre rotated back about the anchor, local = that - origin, the +-0.5 window (anti-aliasing) or the tight one, then
//               sample_bilinear :2326 (clamp to edge, four taps read as one dword each, the four-term sum left to right) or the truncating nearest pick.
//   commit      one thread per pixel of the commit box, blocks of 64 x 4: a wave is 64 consecutive columns of one row, so the read of the document pixel and
//               its write coalesce; the four taps are a gather.  overwrite_mask_allows :1150 reads the one-byte mask through the resize's NEAREST rule (weight 1:
//               an index lookup), alpha_blend :2368 with its three early returns.  Rejected pixels store nothing.  The anti-aliasing and overwrite switches are
//               template parameters.
//   rasterize   the same sampler into the clipboard window, no blending; one atomic per wave that stored a pixel sets the `has pixels` word.
//   preview     render_preview :2168 over every pixel of the document (the output is written whole): NEAREST-scaled pixels straight from the source.
//   lift        extract_to_overlay :769-777 over the selection's box; any_alpha is its `has_content` :796.
// No LDS anywhere.  Pixels are indexed in 32 bits: every image here is within pfx_dims_ok (256 Mpx).
#include "k_tools.h"
#include "pfx_kernels.h"

using namespace pfxk;

namespace {

constexpr uint32_t BX = 64, BY = 4;

// `v as u32` for v that is NaN or non-negative: NaN -> 0, saturating
PFX_DEV uint32_t as_u32(float v) { return v == v ? (uint32_t)__builtin_fminf(v, 4294967040.0f) : 0u; }
// the NEAREST rule of the resize's per-axis tables (pfx_resize.cpp:build_axis at support 0): output o reads source index floor((o + 0.5) * ratio), clamped
PFX_DEV uint32_t nearest_index(uint32_t o, float ratio, uint32_t n_in) { return min(as_u32(__builtin_floorf(((float)o + 0.5f) * ratio)), n_in - 1u); }

// pixel (ix, iy) of the scaled image: SRC = read it from the un-scaled source through the NEAREST rule
template <bool SRC>
PFX_DEV uint32_t texel(const uint32_t* __restrict__ img, const pfxk_overlay& P, uint32_t ix, uint32_t iy)
{
    if constexpr (SRC) return img[nearest_index(iy, P.ratio_y, P.source_h) * P.source_w + nearest_index(ix, P.ratio_x, P.source_w)];
    else return img[iy * P.scaled_w + ix];
}

// sample_bilinear :2326.  x, y are in [-1, scaled) or NaN (the caller's window test lets nothing else through); `NaN as i32` is 0
PFX_DEV uint32_t sample_bilinear(const uint32_t* __restrict__ img, const pfxk_overlay& P, float x, float y)
{
    const int x0 = x == x ? (int)__builtin_floorf(x) : 0, y0 = y == y ? (int)__builtin_floorf(y) : 0;
    const float fx = x - (float)x0, fy = y - (float)y0;
    const int wm = (int)P.scaled_w - 1, hm = (int)P.scaled_h - 1;
    const uint32_t cx0 = (uint32_t)min(max(x0, 0), wm), cx1 = (uint32_t)min(max(x0 + 1, 0), wm);
    const uint32_t cy0 = (uint32_t)min(max(y0, 0), hm), cy1 = (uint32_t)min(max(y0 + 1, 0), hm);
    const uint32_t p00 = img[cy0 * P.scaled_w + cx0], p10 = img[cy0 * P.scaled_w + cx1], p01 = img[cy1 * P.scaled_w + cx0], p11 = img[cy1 * P.scaled_w + cx1];
    const float inv_fx = 1.0f - fx, inv_fy = 1.0f - fy;
    const float w00 = inv_fx * inv_fy, w10 = fx * inv_fy, w01 = inv_fx * fy, w11 = fx * fy;
    return pack_round_rgba(ubyte0(p00) * w00 + ubyte0(p10) * w10 + ubyte0(p01) * w01 + ubyte0(p11) * w11,
                           ubyte1(p00) * w00 + ubyte1(p10) * w10 + ubyte1(p01) * w01 + ubyte1(p11) * w11,
                           ubyte2(p00) * w00 + ubyte2(p10) * w10 + ubyte2(p01) * w01 + ubyte2(p11) * w11,
                           ubyte3(p00) * w00 + ubyte3(p10) * w10 + ubyte3(p01) * w01 + ubyte3(p11) * w11);
}

// the sample of the pixel whose centre is (px, py): false = outside the window.  lx, ly: the local coordinates, for overwrite_mask_allows
template <bool AA, bool SRC>
PFX_DEV bool sample(const uint32_t* __restrict__ img, const pfxk_overlay& P, float px, float py, uint32_t& out, float& lx, float& ly)
{
    const float rx = px - P.ax, ry = py - P.ay;
    const float ur_x = rx * P.cos_r + ry * P.sin_r + P.ax;
    const float ur_y = -rx * P.sin_r + ry * P.cos_r + P.ay;
    lx = ur_x - P.origin_x;
    ly = ur_y - P.origin_y;
    const float sw = (float)P.scaled_w, sh = (float)P.scaled_h;
    if constexpr (AA) {
        if (lx < -0.5f || ly < -0.5f || lx >= sw + 0.5f || ly >= sh + 0.5f) return false;
        static_assert(!SRC, "the bilinear taps read the scaled image");
        out = sample_bilinear(img, P, lx - 0.5f, ly - 0.5f);
    } else {
        if (lx < 0.0f || ly < 0.0f || lx >= sw || ly >= sh) return false;   // the tight window lies inside the +-0.5 one
        out = texel<SRC>(img, P, min(as_u32(lx), P.scaled_w - 1u), min(as_u32(ly), P.scaled_h - 1u));
    }
    return true;
}

// alpha_blend :2368, src over dst
PFX_DEV uint32_t alpha_blend(uint32_t dst, uint32_t src)
{
    const uint32_t sai = src >> 24, dai = dst >> 24;
    if (sai == 0u) return dst;
    if (sai == 255u || dai == 0u) return src;
    const float sa = div255((float)sai), da = div255((float)dai);
    const float rest = 1.0f - sa;
    const float out_a = sa + da * rest;
    if (out_a < 0.001f) return 0u;
    const float inv = 1.0f / out_a;
    return pack_round_rgba_finite((ubyte0(src) * sa + ubyte0(dst) * da * rest) * inv, (ubyte1(src) * sa + ubyte1(dst) * da * rest) * inv,
                                  (ubyte2(src) * sa + ubyte2(dst) * da * rest) * inv, out_a * 255.0f);
}

// overwrite_mask_allows :1150 on the mask scaled with the NEAREST rule
PFX_DEV bool mask_allows(const uint8_t* __restrict__ mask, const pfxk_overlay& P, float lx, float ly)
{
    if (lx < 0.0f || ly < 0.0f) return false;
    const uint32_t ix = min(as_u32(lx), P.scaled_w - 1u), iy = min(as_u32(ly), P.scaled_h - 1u);
    return mask[nearest_index(iy, P.ratio_y, P.source_h) * P.source_w + nearest_index(ix, P.ratio_x, P.source_w)] != 0u;
}

// OVR: 0 blend only, 1 every sample overwrites, 2 where the mask allows
template <bool AA, int OVR>
__global__ __launch_bounds__(256) void commit_kernel(const uint32_t* __restrict__ scaled, const uint8_t* __restrict__ mask, uint32_t* img, uint32_t tiles_x, pfxk_overlay P)
{
    const auto [bx, by] = tile_xy<BX, BY>(tiles_x, threadIdx.x, threadIdx.y);
    if (bx >= P.box_w || by >= P.box_h) return;
    const uint32_t dx = (uint32_t)P.x0 + bx, dy = (uint32_t)P.y0 + by;
    uint32_t src;
    float lx, ly;
    if (!sample<AA, false>(scaled, P, (float)dx + 0.5f, (float)dy + 0.5f, src, lx, ly)) return;
    const uint32_t at = dy * P.pitch + dx;
    bool over = OVR == 1;
    if constexpr (OVR == 2) over = mask_allows(mask, P, lx, ly);
    if (over) img[at] = src;
    else if ((src >> 24) != 0u) img[at] = alpha_blend(img[at], src);
}

template <bool AA>
__global__ __launch_bounds__(256) void rasterize_kernel(const uint32_t* __restrict__ scaled, uint32_t* __restrict__ out, uint32_t tiles_x, pfxk_overlay P, uint32_t* any)
{
    const auto [bx, by] = tile_xy<BX, BY>(tiles_x, threadIdx.x, threadIdx.y);
    bool stored = false;
    if (bx < P.box_w && by < P.box_h) {
        uint32_t src;
        float lx, ly;
        // px = col_start as f32 + out_x as f32 + 0.5 :1095: two additions
        if (sample<AA, false>(scaled, P, (float)P.x0 + (float)bx + 0.5f, (float)P.y0 + (float)by + 0.5f, src, lx, ly) && (src >> 24) != 0u) {
            out[by * P.pitch + bx] = src;
            stored = true;
        }
    }
    if (__any(stored) && (threadIdx.x & 63u) == 0u) atomicOr(any, 1u);   // a wave is one row of the block
}

template <bool TRANSLATE>
__global__ __launch_bounds__(256) void preview_kernel(const uint32_t* __restrict__ source, uint32_t* __restrict__ out, uint32_t doc_w, uint32_t doc_h, uint32_t tiles_x, pfxk_overlay P)
{
    const auto [x, y] = tile_xy<BX, BY>(tiles_x, threadIdx.x, threadIdx.y);
    if (x >= doc_w || y >= doc_h) return;
    uint32_t px = 0u;
    // the box in unsigned arithmetic: x - x0 wraps to a large value left of it (x0 >= 0 here)
    if (x - (uint32_t)P.x0 < P.box_w && y - (uint32_t)P.y0 < P.box_h) {
        if constexpr (TRANSLATE) {
            px = texel<true>(source, P, (uint32_t)((int32_t)x - P.out_x0), (uint32_t)((int32_t)y - P.out_y0));   // :2211-2218; inside the scaled image by the host's box
        } else {
            float lx, ly;
            if (!sample<false, true>(source, P, (float)x + 0.5f, (float)y + 0.5f, px, lx, ly)) px = 0u;
        }
        if ((px >> 24) == 0u) px = 0u;
    }
    out[y * doc_w + x] = px;
}

__global__ __launch_bounds__(256) void lift_kernel(const uint32_t* __restrict__ layer, const uint8_t* __restrict__ sel, uint32_t* __restrict__ clip, uint8_t* __restrict__ clip_mask,
                                                   uint32_t w, uint32_t x0, uint32_t y0, uint32_t bw, uint32_t bh, uint32_t tiles_x)
{
    const auto [bx, by] = tile_xy<BX, BY>(tiles_x, threadIdx.x, threadIdx.y);
    if (bx >= bw || by >= bh) return;
    const uint32_t at = (y0 + by) * w + x0 + bx;
    const bool on = sel[at] != 0u;
    clip[by * bw + bx] = on ? layer[at] : 0u;
    clip_mask[by * bw + bx] = on ? 255u : 0u;
}

__global__ __launch_bounds__(256) void any_alpha_kernel(const uint32_t* __restrict__ img, size_t n, uint32_t* any)
{
    bool found = false;
    for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (size_t)gridDim.x * 256u) found |= (img[i] >> 24) != 0u;
    if (__any(found) && (threadIdx.x & 63u) == 0u) atomicOr(any, 1u);
}

inline bool box_ok(const pfxk_overlay* P) { return P && P->scaled_w && P->scaled_h && P->source_w && P->source_h && (uint64_t)P->box_w * P->box_h <= 256000000ull; }

} // namespace

extern "C" hipError_t pfxk_overlay_commit(hipStream_t s, const uint8_t* d_scaled, const uint8_t* d_mask, uint8_t* d_img, const pfxk_overlay* P, int aa, int overwrite)
{
    if (!box_ok(P) || overwrite < 0 || overwrite > 2 || (overwrite == 2 && !d_mask) || P->x0 < 0 || P->y0 < 0) return hipErrorInvalidValue;
    uint32_t tiles_x;
    const uint32_t blocks = tile_grid<BX, BY>(P->box_w, P->box_h, &tiles_x);
    if (!blocks) return P->box_w && P->box_h ? hipErrorInvalidValue : hipSuccess;
    const dim3 block(BX, BY);
    const uint32_t* sc = (const uint32_t*)d_scaled;
    uint32_t* img = (uint32_t*)d_img;
    if (aa) {
        if (overwrite == 0) commit_kernel<true, 0><<<blocks, block, 0, s>>>(sc, d_mask, img, tiles_x, *P);
        else if (overwrite == 1) commit_kernel<true, 1><<<blocks, block, 0, s>>>(sc, d_mask, img, tiles_x, *P);
        else commit_kernel<true, 2><<<blocks, block, 0, s>>>(sc, d_mask, img, tiles_x, *P);
    } else {
        if (overwrite == 0) commit_kernel<false, 0><<<blocks, block, 0, s>>>(sc, d_mask, img, tiles_x, *P);
        else if (overwrite == 1) commit_kernel<false, 1><<<blocks, block, 0, s>>>(sc, d_mask, img, tiles_x, *P);
        else commit_kernel<false, 2><<<blocks, block, 0, s>>>(sc, d_mask, img, tiles_x, *P);
    }
    return hipGetLastError();
}

extern "C" hipError_t pfxk_overlay_rasterize(hipStream_t s, const uint8_t* d_scaled, uint8_t* d_out, const pfxk_overlay* P, int aa, uint32_t* d_any)
{
    if (!box_ok(P) || !d_any) return hipErrorInvalidValue;
    uint32_t tiles_x;
    const uint32_t blocks = tile_grid<BX, BY>(P->box_w, P->box_h, &tiles_x);
    if (!blocks) return P->box_w && P->box_h ? hipErrorInvalidValue : hipSuccess;
    if (aa) rasterize_kernel<true><<<blocks, dim3(BX, BY), 0, s>>>((const uint32_t*)d_scaled, (uint32_t*)d_out, tiles_x, *P, d_any);
    else rasterize_kernel<false><<<blocks, dim3(BX, BY), 0, s>>>((const uint32_t*)d_scaled, (uint32_t*)d_out, tiles_x, *P, d_any);
    return hipGetLastError();
}

extern "C" hipError_t pfxk_overlay_preview(hipStream_t s, const uint8_t* d_source, uint8_t* d_out, uint32_t doc_w, uint32_t doc_h, const pfxk_overlay* P, int translate)
{
    if (!box_ok(P) || !dims_ok(doc_w, doc_h)) return hipErrorInvalidValue;
    if (P->box_w && P->box_h && (P->x0 < 0 || P->y0 < 0 || (uint64_t)P->x0 + P->box_w > doc_w || (uint64_t)P->y0 + P->box_h > doc_h)) return hipErrorInvalidValue;
    uint32_t tiles_x;
    const uint32_t blocks = tile_grid<BX, BY>(doc_w, doc_h, &tiles_x);
    if (!blocks) return hipErrorInvalidValue;
    if (translate) preview_kernel<true><<<blocks, dim3(BX, BY), 0, s>>>((const uint32_t*)d_source, (uint32_t*)d_out, doc_w, doc_h, tiles_x, *P);
    else preview_kernel<false><<<blocks, dim3(BX, BY), 0, s>>>((const uint32_t*)d_source, (uint32_t*)d_out, doc_w, doc_h, tiles_x, *P);
    return hipGetLastError();
}

extern "C" hipError_t pfxk_overlay_lift(hipStream_t s, const uint8_t* d_layer, const uint8_t* d_sel, uint8_t* d_clip, uint8_t* d_clip_mask, uint32_t w, uint32_t x0,
                                        uint32_t y0, uint32_t bw, uint32_t bh)
{
    if (!bw || !bh || (uint64_t)x0 + bw > w) return hipErrorInvalidValue;
    uint32_t tiles_x;
    const uint32_t blocks = tile_grid<BX, BY>(bw, bh, &tiles_x);
    if (!blocks) return hipErrorInvalidValue;
    lift_kernel<<<blocks, dim3(BX, BY), 0, s>>>((const uint32_t*)d_layer, d_sel, (uint32_t*)d_clip, d_clip_mask, w, x0, y0, bw, bh, tiles_x);
    return hipGetLastError();
}

extern "C" hipError_t pfxk_overlay_any_alpha(hipStream_t s, const uint8_t* d_img, size_t n, uint32_t* d_any)
{
    if (n == 0) return hipSuccess;
    any_alpha_kernel<<<stream_blocks(n), 256, 0, s>>>((const uint32_t*)d_img, n, d_any);
    return hipGetLastError();
}
