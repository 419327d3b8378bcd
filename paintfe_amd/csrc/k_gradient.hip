// k_gradient.hip — the gradient tool and the perspective crop (ref: src/ui/panels/tools/behavior/raster/perspective_gradient.rs), bit for bit: every f32
// expression as the reference writes it, one rounding per operation (no contraction), IEEE division and square root, round() half away from zero.
//
//   render   render_gradient_to_preview's CPU path :386-523 (not its WGSL branch: that one divides start and end by the preview scale), one thread per
//            generated pixel, the output written whole.  A streaming kernel that only writes: four pixels per lane and one 16-byte store where a quad cannot
//            straddle a row (gen_w % 4 == 0, 16-byte aligned outputs), else pixel by pixel.  The LUT index diverges per lane, so the 256 packed entries are
//            staged in LDS once per workgroup (256 lanes, one entry each).  Shape and repeat are template parameters; selection and the premultiplied copy
//            are wave-uniform pointer tests.  The "upscale" branch :527-544 is dead code in the reference (its `scale` IS preview_scale, so `scale > 1 &&
//            preview_scale == 1` never holds) and is not here.
//   commit   commit_gradient (gradient_text/gradient_controls.rs:63-122) over the layer in place.  pfx_brush_commit's Normal arm (k_blend.h:blend_px) is NOT
//            this arithmetic — it blends colours normalised to [0, 1] and truncates, its eraser truncates where this one rounds — so nothing is shared.
//   apply    render at scale 1 and commit in one pass: 4 B/px read and 4 written, no preview buffer.  The same two device functions, so the same bits.
//   crop     apply_perspective_crop's loop :150-165 with bilinear_sample :186-233, one thread per output pixel, blocks of 64 x 4; the map is computed once
//            per pixel and every layer is sampled through it in the same launch.  The sampler is this file's own: fx comes from the UNCLAMPED coordinate and
//            the horizontal lerps are rounded to u8 before the vertical one (k_tools.h says why the samplers are not folded).
// Pixels are indexed in 32 bits: every image here is within pfx_dims_ok (256 Mpx).
#include <type_traits>

#include "k_tools.h"
#include "pfx_kernels.h"

using namespace pfxk;

namespace {

// f32::rem_euclid(M) for M = 1 and M = 2: r = x % M; r < 0 ? r + M : r (the sum may round up to M itself).  x % M is exact in IEEE arithmetic and so is the
// form used here: x - M * trunc(x / M) — x / M is x itself or an exact halving (a subnormal x may lose its last bit, but then trunc gives 0 either way),
// M * trunc(..) is an integer of x's magnitude at most, and the difference of two floats that close is representable.  +-inf gives inf - inf = NaN, as
// fmodf does.  The one difference is the sign of a zero result (fmodf keeps x's sign): `r < 0` is false for both zeros and the caller's index is 0 for both.
template <int M>
PFX_DEV float rem_euclid(float x)
{
    static_assert(M == 1 || M == 2, "");
    const float r = M == 1 ? x - __builtin_truncf(x) : x - 2.0f * __builtin_truncf(x * 0.5f);
    return r < 0.0f ? r + (float)M : r;
}

// the four `t` formulas :461-498.  The reference hoists the row terms (ry * dy, ry * ry, ry * uy, ry * ux): they are pure functions of y, the same bits here
template <int SHAPE, bool REPEAT>
PFX_DEV float gradient_t(float rx, float ry, const pfxk_gradient& P)
{
    if constexpr (SHAPE == 0) {
        const float raw = (rx * P.dx + ry * P.dy) * P.inv_len_sq;
        return REPEAT ? rem_euclid<1>(raw) : rs_clamp(raw, 0.0f, 1.0f);
    } else if constexpr (SHAPE == 1) {
        const float raw = (rx * P.dx + ry * P.dy) * P.inv_len_sq;
        if constexpr (REPEAT) {
            const float t_mod = rem_euclid<2>(raw);
            return t_mod > 1.0f ? 2.0f - t_mod : t_mod;
        } else {
            return 1.0f - __builtin_fabsf(2.0f * rs_clamp(raw, 0.0f, 1.0f) - 1.0f);
        }
    } else if constexpr (SHAPE == 2) {
        const float dist = __builtin_sqrtf(rx * rx + ry * ry) * P.inv_len;
        return REPEAT ? rem_euclid<1>(dist) : rs_clamp(dist, 0.0f, 1.0f);
    } else {
        const float proj = __builtin_fabsf(rx * P.ux + ry * P.uy) * P.inv_len;
        const float perp = __builtin_fabsf(rx * (-P.uy) + ry * P.ux) * P.inv_len;
        const float dist = proj + perp;
        return REPEAT ? rem_euclid<1>(dist) : rs_clamp(dist, 0.0f, 1.0f);
    }
}

// the preview pixel of generated pixel (x, y); sv = its selection byte (255 without a selection).  lut: the workgroup's LDS copy
template <int SHAPE, bool REPEAT>
PFX_DEV uint32_t preview_px(const uint32_t* lut, const pfxk_gradient& P, uint32_t x, uint32_t y, uint32_t sv)
{
    if (sv == 0u) return 0u;                                            // :451-458 `continue`: the row buffer starts as zeros
    const float px = (float)x * P.scale_f + P.scale_f * 0.5f, py = (float)y * P.scale_f + P.scale_f * 0.5f;
    const float t = gradient_t<SHAPE, REPEAT>(px - P.ax, py - P.ay, P);
    // `(t * 255.0) as usize` truncates; NaN (a clamp or remainder of inf - inf, inf * 0) -> 0.  t is never negative and never above 1 for any input: clamp
    // ends in [0, 1]; rem_euclid(1) is r in [0, 1) or r + 1 with r in (-1, 0), at most 1.0 after rounding; the reflected forms map [0, 2] and [0, 1] into
    // [0, 1].  So t * 255 <= 255 and the index cannot pass 255, where the reference would panic; the umin decides nothing and keeps the LDS read in the table
    const uint32_t idx = t == t ? umin((uint32_t)(t * 255.0f), 255u) : 0u;
    const uint32_t c = lut[idx];
    uint32_t a = c >> 24;
    if (sv < 255u) a = a * sv / 255u;                                   // :510-512, u16 arithmetic: 255 * 254 fits
    return a == 0u ? 0u : (c & 0x00ffffffu) | (a << 24);               // :515: a == 0 leaves the zeros
}

// preview_flat_buffer :559-572: (c * a + 128) / 255 in integers, alpha copied
PFX_DEV uint32_t premultiply(uint32_t p)
{
    const uint32_t a = p >> 24;
    return ((p & 0xffu) * a + 128u) / 255u | (((p >> 8) & 0xffu) * a + 128u) / 255u << 8 | (((p >> 16) & 0xffu) * a + 128u) / 255u << 16 | a << 24;
}

// commit_gradient's pixel :85-119: pv the preview's, lp the layer's; the result is the layer's new pixel
PFX_DEV uint32_t commit_px(uint32_t lp, uint32_t pv, bool eraser)
{
    if ((pv >> 24) == 0u) return lp;                                    // :86
    const float sa = div255(ubyte3(pv)), da = div255(ubyte3(lp));       // `as f32 / 255.0`: div255 is that quotient, correctly rounded
    const float rest = 1.0f - sa;
    if (eraser) {
        const float new_a = __builtin_fmaxf(da * rest, 0.0f);
        return (lp & 0x00ffffffu) | ((uint32_t)round_u8f(new_a * 255.0f) << 24);
    }
    const float out_a = sa + da * rest;                                 // sa >= 1 / 255 here, so out_a > 0 :102 always holds
    // the three quotients share their denominator: rdiv (k_common.h) is `/` bit for bit for numerators 0 or in [2^-100, 2^20] and denominators in [2^-48, 2^20];
    // here a numerator is 0 or at least 255^-2 (s * sa >= 1 / 255; d * da * rest >= 1 * (1 / 255) * (1 / 255) unless rest is 0) and at most 510, and out_a
    // is in [1 / 255, 2]
    const rdiv k = rdiv_prepare(out_a);
    return pack_round_rgba_finite(rdiv_apply(k, ubyte0(pv) * sa + ubyte0(lp) * da * rest), rdiv_apply(k, ubyte1(pv) * sa + ubyte1(lp) * da * rest),
                                  rdiv_apply(k, ubyte2(pv) * sa + ubyte2(lp) * da * rest), out_a * 255.0f);
}

// the selection bytes of the quad's four pixels packed low to high; dword: scale 1 and a 4-byte aligned mask, one load (w == gen_w is a multiple of 4)
PFX_DEV uint32_t quad_selection(const uint8_t* __restrict__ sel, uint32_t dword, const pfxk_gradient& P, uint32_t g, uint32_t x, uint32_t y)
{
    if (!sel) return 0xffffffffu;
    if (dword) return reinterpret_cast<const uint32_t*>(sel)[g];
    const uint8_t* row = sel + y * P.scale * P.w;
    return row[x * P.scale] | (uint32_t)row[(x + 1u) * P.scale] << 8 | (uint32_t)row[(x + 2u) * P.scale] << 16 | (uint32_t)row[(x + 3u) * P.scale] << 24;
}

PFX_DEV void stage_lut(uint32_t* lut, const uint32_t* __restrict__ d_lut)
{
    lut[threadIdx.x] = d_lut[threadIdx.x];                              // 256 lanes, 256 entries
    __syncthreads();
}

// VEC: gen_w % 4 == 0 (a quad stays in its row, n % 4 == 0) and 16-byte aligned outputs
template <int SHAPE, bool REPEAT, bool VEC>
__global__ __launch_bounds__(256) void render_kernel(const uint32_t* __restrict__ d_lut, const uint8_t* __restrict__ sel, uint32_t* __restrict__ preview,
                                                     uint32_t* __restrict__ premul, uint32_t sel_dword, pfxk_gradient P)
{
    __shared__ uint32_t lut[256];
    stage_lut(lut, d_lut);
    stream_walk<VEC, uint32_t>(P.gen_w * P.gen_h, [&](uint32_t g) {
        const uint32_t y = g * 4u / P.gen_w, x = g * 4u - y * P.gen_w;
        const uint32_t m = quad_selection(sel, sel_dword, P, g, x, y);
        uint4 o;
        o.x = preview_px<SHAPE, REPEAT>(lut, P, x, y, m & 0xffu);
        o.y = preview_px<SHAPE, REPEAT>(lut, P, x + 1u, y, (m >> 8) & 0xffu);
        o.z = preview_px<SHAPE, REPEAT>(lut, P, x + 2u, y, (m >> 16) & 0xffu);
        o.w = preview_px<SHAPE, REPEAT>(lut, P, x + 3u, y, m >> 24);
        reinterpret_cast<uint4*>(preview)[g] = o;
        if (premul) reinterpret_cast<uint4*>(premul)[g] = make_uint4(premultiply(o.x), premultiply(o.y), premultiply(o.z), premultiply(o.w));
    }, [&](uint32_t i) {
        const uint32_t y = i / P.gen_w, x = i - y * P.gen_w;
        const uint32_t p = preview_px<SHAPE, REPEAT>(lut, P, x, y, sel ? sel[y * P.scale * P.w + x * P.scale] : 255u);
        preview[i] = p;
        if (premul) premul[i] = premultiply(p);
    });
}

// VEC: w % 4 == 0 and a 16-byte aligned layer.  P.scale == 1: generated pixel (x, y) is the layer's, the selection's index is the pixel's
template <int SHAPE, bool REPEAT, bool VEC>
__global__ __launch_bounds__(256) void apply_kernel(const uint32_t* __restrict__ d_lut, const uint8_t* __restrict__ sel, uint32_t* __restrict__ layer, uint32_t sel_dword,
                                                    pfxk_gradient P)
{
    __shared__ uint32_t lut[256];
    stage_lut(lut, d_lut);
    const bool eraser = P.eraser != 0;
    stream_walk<VEC, uint32_t>(P.gen_w * P.gen_h, [&](uint32_t g) {
        const uint32_t y = g * 4u / P.gen_w, x = g * 4u - y * P.gen_w;
        const uint32_t m = quad_selection(sel, sel_dword, P, g, x, y);
        uint4 v = reinterpret_cast<const uint4*>(layer)[g];
        v.x = commit_px(v.x, preview_px<SHAPE, REPEAT>(lut, P, x, y, m & 0xffu), eraser);
        v.y = commit_px(v.y, preview_px<SHAPE, REPEAT>(lut, P, x + 1u, y, (m >> 8) & 0xffu), eraser);
        v.z = commit_px(v.z, preview_px<SHAPE, REPEAT>(lut, P, x + 2u, y, (m >> 16) & 0xffu), eraser);
        v.w = commit_px(v.w, preview_px<SHAPE, REPEAT>(lut, P, x + 3u, y, m >> 24), eraser);
        reinterpret_cast<uint4*>(layer)[g] = v;
    }, [&](uint32_t i) {
        const uint32_t y = i / P.gen_w, x = i - y * P.gen_w;
        const uint32_t p = preview_px<SHAPE, REPEAT>(lut, P, x, y, sel ? sel[i] : 255u);
        if ((p >> 24) != 0u) layer[i] = commit_px(layer[i], p, eraser);
    });
}

// VEC: both images 16-byte aligned
template <bool VEC, bool ERASER>
__global__ __launch_bounds__(256) void commit_kernel(uint32_t* __restrict__ layer, const uint32_t* __restrict__ preview, size_t n)
{
    stream_walk<VEC, size_t>(n, [&](size_t g) {
        const uint4 p = reinterpret_cast<const uint4*>(preview)[g];
        if (((p.x | p.y | p.z | p.w) >> 24) == 0u) return;             // nothing to commit in this quad: the layer is not read
        uint4 v = reinterpret_cast<const uint4*>(layer)[g];
        v.x = commit_px(v.x, p.x, ERASER); v.y = commit_px(v.y, p.y, ERASER); v.z = commit_px(v.z, p.z, ERASER); v.w = commit_px(v.w, p.w, ERASER);
        reinterpret_cast<uint4*>(layer)[g] = v;
    }, [&](size_t i) {
        const uint32_t p = preview[i];
        if ((p >> 24) != 0u) layer[i] = commit_px(layer[i], p, ERASER);
    });
}

// `v as u32` for v that is NaN or any finite or infinite value: NaN and negatives -> 0, saturating
PFX_DEV uint32_t as_u32(float v) { return (uint32_t)__builtin_fminf(__builtin_fmaxf(v, 0.0f), 4294967040.0f); }   // fmaxf(NaN, 0) = 0

constexpr uint32_t BX = 64, BY = 4;

// the lerp of bilinear_sample :205-209 on four channels at once: (a * (1 - t) + b * t).round().clamp(0, 255) as u8; NaN (t from inf - inf) -> 0
PFX_DEV uint32_t lerp_rgba(uint32_t a, uint32_t b, float t)
{
    const float inv = 1.0f - t;
    return pack_round_rgba(ubyte0(a) * inv + ubyte0(b) * t, ubyte1(a) * inv + ubyte1(b) * t, ubyte2(a) * inv + ubyte2(b) * t, ubyte3(a) * inv + ubyte3(b) * t);
}

__global__ __launch_bounds__(256) void crop_kernel(const uint32_t* const* __restrict__ layers, uint32_t* const* __restrict__ outs, uint32_t tiles_x, pfxk_crop P)
{
    const auto [ox, oy] = tile_xy<BX, BY>(tiles_x, threadIdx.x, threadIdx.y);
    if (ox >= P.out_w || oy >= P.out_h) return;
    const float u = ((float)ox + 0.5f) / (float)P.out_w, v = ((float)oy + 0.5f) / (float)P.out_h;
    const float iu = 1.0f - u, iv = 1.0f - v;
    const float sx = iu * iv * P.cx[0] + u * iv * P.cx[1] + u * v * P.cx[2] + iu * v * P.cx[3];   // :155-162, products and sums left to right
    const float sy = iu * iv * P.cy[0] + u * iv * P.cy[1] + u * v * P.cy[2] + iu * v * P.cy[3];
    // bilinear_sample: `floor as i32` then max(0) then min(w - 1) is as_u32 then min(w - 1); x1 from the clamped x0, fx from the unclamped coordinate
    const float flx = __builtin_floorf(sx), fly = __builtin_floorf(sy);
    const uint32_t x0 = umin(as_u32(flx), P.w - 1u), y0 = umin(as_u32(fly), P.h - 1u);
    const uint32_t x1 = umin(x0 + 1u, P.w - 1u), y1 = umin(y0 + 1u, P.h - 1u);
    const float fx = sx - flx, fy = sy - fly;
    const uint32_t i00 = y0 * P.w + x0, i10 = y0 * P.w + x1, i01 = y1 * P.w + x0, i11 = y1 * P.w + x1, at = oy * P.out_w + ox;
    for (uint32_t l = 0; l < P.n_layers; ++l) {
        const uint32_t* __restrict__ img = layers[l];
        outs[l][at] = lerp_rgba(lerp_rgba(img[i00], img[i10], fx), lerp_rgba(img[i01], img[i11], fx), fy);
    }
}

// the instantiation for a shape and a repeat flag: f(shape constant, repeat constant)
template <class F>
hipError_t by_shape(int shape, bool repeat, F f)
{
    switch (shape * 2 + (repeat ? 1 : 0)) {
    case 0: return f(std::integral_constant<int, 0>{}, std::false_type{});
    case 1: return f(std::integral_constant<int, 0>{}, std::true_type{});
    case 2: return f(std::integral_constant<int, 1>{}, std::false_type{});
    case 3: return f(std::integral_constant<int, 1>{}, std::true_type{});
    case 4: return f(std::integral_constant<int, 2>{}, std::false_type{});
    case 5: return f(std::integral_constant<int, 2>{}, std::true_type{});
    case 6: return f(std::integral_constant<int, 3>{}, std::false_type{});
    case 7: return f(std::integral_constant<int, 3>{}, std::true_type{});
    default: return hipErrorInvalidValue;
    }
}

inline bool params_ok(const pfxk_gradient* P)
{
    return P && P->scale >= 1u && dims_ok(P->gen_w, P->gen_h) && P->w != 0u && (uint64_t)(P->gen_w - 1u) * P->scale < P->w && P->shape >= 0 && P->shape <= 3;
}

} // namespace

extern "C" hipError_t pfxk_gradient_render(hipStream_t s, const uint32_t* d_lut, const uint8_t* d_sel, uint8_t* d_preview, uint8_t* d_premul, const pfxk_gradient* P)
{
    if (!params_ok(P) || !d_lut || !d_preview) return hipErrorInvalidValue;
    const size_t n = (size_t)P->gen_w * P->gen_h;
    const bool vec = P->gen_w % 4u == 0u && aligned_to(d_preview, 16) && aligned_to(d_premul, 16);
    const uint32_t sel_dword = d_sel && P->scale == 1u && aligned_to(d_sel, 4);
    return by_shape(P->shape, P->repeat != 0, [&](auto shape, auto repeat) {
        return launch_stream(vec, n, s, render_kernel<shape.value, repeat.value, true>, render_kernel<shape.value, repeat.value, false>, d_lut, d_sel,
                             (uint32_t*)d_preview, (uint32_t*)d_premul, sel_dword, *P);
    });
}

extern "C" hipError_t pfxk_gradient_apply(hipStream_t s, const uint32_t* d_lut, const uint8_t* d_sel, uint8_t* d_layer, const pfxk_gradient* P)
{
    if (!params_ok(P) || P->scale != 1u || P->w != P->gen_w || !d_lut || !d_layer) return hipErrorInvalidValue;
    const size_t n = (size_t)P->gen_w * P->gen_h;
    const bool vec = P->gen_w % 4u == 0u && aligned_to(d_layer, 16);
    const uint32_t sel_dword = d_sel && aligned_to(d_sel, 4);
    return by_shape(P->shape, P->repeat != 0, [&](auto shape, auto repeat) {
        return launch_stream(vec, n, s, apply_kernel<shape.value, repeat.value, true>, apply_kernel<shape.value, repeat.value, false>, d_lut, d_sel, (uint32_t*)d_layer,
                             sel_dword, *P);
    });
}

extern "C" hipError_t pfxk_gradient_commit(hipStream_t s, uint8_t* d_layer, const uint8_t* d_preview, size_t n, int is_eraser)
{
    if (n == 0) return hipSuccess;
    if (!d_layer || !d_preview || n > 256000000ull) return hipErrorInvalidValue;
    const bool vec = aligned_to(d_layer, 16) && aligned_to(d_preview, 16);
    if (is_eraser) return launch_stream(vec, n, s, commit_kernel<true, true>, commit_kernel<false, true>, (uint32_t*)d_layer, (const uint32_t*)d_preview, n);
    return launch_stream(vec, n, s, commit_kernel<true, false>, commit_kernel<false, false>, (uint32_t*)d_layer, (const uint32_t*)d_preview, n);
}

extern "C" hipError_t pfxk_perspective_crop(hipStream_t s, const uint8_t* const* d_layers, uint8_t* const* d_outs, const pfxk_crop* P)
{
    if (!P || !d_layers || !d_outs || !P->n_layers || !dims_ok(P->w, P->h) || !dims_ok(P->out_w, P->out_h)) return hipErrorInvalidValue;
    uint32_t tiles_x;
    const uint32_t blocks = tile_grid<BX, BY>(P->out_w, P->out_h, &tiles_x);
    if (!blocks) return hipErrorInvalidValue;
    crop_kernel<<<blocks, dim3(BX, BY), 0, s>>>((const uint32_t* const*)d_layers, (uint32_t* const*)d_outs, tiles_x, *P);
    return hipGetLastError();
}
