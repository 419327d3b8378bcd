// k_colorrange.hip — the colour dialogs' last three pixel loops (ref: src/ops/adjustments.rs), bit for bit: u8 -> f32, one rounding per written operation
// (no contraction), IEEE division, round() half away from zero, `as u8` saturating.
//
//   histogram     compute_histogram :883-937, the Levels dialog's four 256-bin histograms.  A grid-stride walk, 16-byte loads where the pointers allow it.  A
//                 workgroup counts into PFXK_HIST_COPIES private copies of the 1024 counters in LDS (32 KiB); a lane's copy is lane % COPIES and the copies of
//                 one bin are neighbouring dwords, so on a flat image — every lane on the same bin — a wave's 64 increments fall on 8 addresses in 8 banks
//                 and not on one.  After the walk a lane sums the copies of four bins and adds the non-zero sums to the global counters with atomicAdd.
//                 Integer sums do not depend on the order of arrival: the result is exact.  The counters are u32: 2^32 pixels would wrap one, the document
//                 limit of 256 000 000 pixels (pfx_check_dims) stays below it.
//   per-band      hue_saturation_per_band_from_flat :1616-1673.  The pixel function below inside the pointwise bank's chunk walk (k_pointwise.h:
//                 chunk_walk), which owns the selection mask and the three sparse modes: no second copy of either here.
//   colour range  select_color_range :1705-1787, a streaming RGBA8 -> mask kernel with the function's own combine rule.  Its powf puts it in the LIBM class: the
//                 device takes the f64 pow rounded once to f32, as k_tools.h does for cos / sin (tests/colorrange_model.py marks the pixels where one f32
//                 ulp of the power moves the byte).
//
// rgb_to_hsl / hsl_to_rgb<false> are k_pointwise.h's.  Their preconditions hold at every call below: rgb_to_hsl only ever sees div255 of a byte (k / 255,
// correctly rounded), and hsl_to_rgb's h is the result of `% 1.0` of a value in (-1, 1) plus 1 (see band_px), so it lies in [0, 1) — unless a slider sum
// overflowed to a NaN, for which both the reference's if-chain and hue_seg's selects fall through to `p`.
#include "k_tools.h"
#include "pfx_kernels.h"
#include "k_pointwise.h"

using namespace pfxk;

namespace {

// ---------------------------------------------------------------------------------------------------------------- histogram
constexpr uint32_t HC = PFXK_HIST_COPIES;

// r, g, b bins and min(round(0.2126 r + 0.7152 g + 0.0722 b), 255) (:928-932); round_u8f is round() half away from zero, then the clamp
PFX_DEV void count_px(uint32_t* sH, uint32_t copy, uint32_t p)
{
    if ((p >> 24) == 0u) return;   // :925
    const uint32_t l = (uint32_t)round_u8f(pw::lum709(ubyte0(p), ubyte1(p), ubyte2(p)));
    atomicAdd(&sH[(p & 0xffu) * HC + copy], 1u);
    atomicAdd(&sH[(256u + ((p >> 8) & 0xffu)) * HC + copy], 1u);
    atomicAdd(&sH[(512u + ((p >> 16) & 0xffu)) * HC + copy], 1u);
    atomicAdd(&sH[(768u + l) * HC + copy], 1u);
}

__global__ __launch_bounds__(256) void hist_zero_kernel(uint32_t* hist) { hist[blockIdx.x * 256u + threadIdx.x] = 0u; }   // 4 workgroups

// VEC: src 16-byte, mask 4-byte aligned
template <bool VEC>
__global__ __launch_bounds__(256) void hist_kernel(const uint32_t* __restrict__ src, const uint8_t* __restrict__ mask, size_t n, uint32_t* hist)
{
    __shared__ uint32_t sH[1024 * HC];
    for (uint32_t i = threadIdx.x; i < 1024u * HC; i += 256u) sH[i] = 0u;
    __syncthreads();
    const uint32_t copy = threadIdx.x & (HC - 1u);
    stream_walk<VEC, size_t>(n, [&](size_t g) {
        const uint4 v = reinterpret_cast<const uint4*>(src)[g];
        const uint32_t m = mask ? reinterpret_cast<const uint32_t*>(mask)[g] : 0xffffffffu;
        if (m & 0xffu) count_px(sH, copy, v.x);
        if (m & 0xff00u) count_px(sH, copy, v.y);
        if (m & 0xff0000u) count_px(sH, copy, v.z);
        if (m >> 24) count_px(sH, copy, v.w);
    }, [&](size_t i) {
        if (!mask || mask[i] != 0u) count_px(sH, copy, src[i]);
    });
    __syncthreads();
    for (uint32_t bin = threadIdx.x; bin < 1024u; bin += 256u) {
        uint32_t sum = 0u;
#pragma unroll
        for (uint32_t c = 0; c < HC; ++c) sum += sH[bin * HC + c];
        if (sum != 0u) atomicAdd(&hist[bin], sum);
    }
}

// ---------------------------------------------------------------------------------------------------------------- per-band Hue/Saturation
// band_weight :1620-1632.  h_deg = h * 360 with h in [0, 1) and the centre in [0, 300]: the distance is at most 360, so `% 360.0` (exact in f32) is one select
PFX_DEV float band_weight(float h_deg, float centre)
{
    float dist = __builtin_fabsf(h_deg - centre);
    dist = dist >= 360.0f ? dist - 360.0f : dist;
    if (dist > 180.0f) dist = 360.0f - dist;
    const float fall = 1.0f - (dist - 30.0f) / 15.0f;
    return dist <= 30.0f ? 1.0f : (dist < 45.0f ? fall : 0.0f);
}

PFX_DEV float fmod1(float x) { return x - __builtin_truncf(x); }   // Rust's `x % 1.0`: fmod, exact, the sign of x

PFX_DEV uint32_t band_px(const pfxk_hsl_bands& B, uint32_t px)
{
    const pw::hsl3 c = pw::rgb_to_hsl(div255(ubyte0(px)), div255(ubyte1(px)), div255(ubyte2(px)));   // bytes: div255 == / 255.0
    const float h_deg = c.h * 360.0f;
    float extra_hue = B.g_hue, factor = B.g_sat, extra_light = B.g_light;
#pragma unroll
    for (int i = 0; i < 6; ++i) {   // in index order; a band of weight 0 adds nothing (:1657)
        const float wgt = band_weight(h_deg, 60.0f * (float)i);
        if (wgt > 0.0f) {
            extra_hue = extra_hue + B.hue[i] * wgt;
            factor = factor + B.sat[i] * wgt;
            extra_light = extra_light + B.light[i] * wgt;
        }
    }
    const float nh = fmod1(fmod1(c.h + extra_hue / 360.0f) + 1.0f);   // :1664: (-1, 1) + 1 in [0, 2], then `% 1.0`: [0, 1)
    const float ns = rs_clamp(c.s * factor, 0.0f, 1.0f);
    const pw::rgb3 o = pw::hsl_to_rgb<false>(nh, ns, c.l);
    // `.round().clamp(0, 255) as u8` of three channels, the alpha byte kept (k_common.h: round_tie_prep; the med3 stays: a slider sum may have overflowed)
    uint32_t q = __builtin_amdgcn_cvt_pk_u8_f32(round_tie_prep(o.r * 255.0f + extra_light), 0, px);
    q = __builtin_amdgcn_cvt_pk_u8_f32(round_tie_prep(o.g * 255.0f + extra_light), 1, q);
    return __builtin_amdgcn_cvt_pk_u8_f32(round_tie_prep(o.b * 255.0f + extra_light), 2, q);
}

__global__ __launch_bounds__(256) void hsl_bands_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, const uint8_t* __restrict__ mask, pfxk_hsl_bands B,
                                                        int sparse_mode, uint32_t w, uint32_t h)
{
    pw::chunk_walk(xcd_swizzle(blockIdx.x, gridDim.x), src, dst, mask, sparse_mode, w, h, [&](uint32_t px) __attribute__((always_inline)) { return band_px(B, px); });
}

// ---------------------------------------------------------------------------------------------------------------- colour range
// glibc's powf evaluated through f64 and rounded once (k_tools.h: libm_cos)
PFX_DEV float libm_pow(float x, float y) { return (float)pow((double)x, (double)y); }

// the new mask's byte (:1713-1736); a skipped pixel keeps GrayImage::new's 0
PFX_DEV uint32_t range_px(uint32_t p, const pfxk_color_range& R)
{
    if ((p >> 24) == 0u) return 0u;   // :1713
    const pw::hsl3 c = pw::rgb_to_hsl(div255(ubyte0(p)), div255(ubyte1(p)), div255(ubyte2(p)));
    if (c.s < R.sat_min) return 0u;   // :1721
    float diff = __builtin_fabsf(c.h - R.hue_center);   // both in [0, 1]: at most 1, so the fold stays at or above 0
    if (diff > 0.5f) diff = 1.0f - diff;
    if (diff > R.hue_tol) return 0u;   // :1730
    const float weight = 1.0f - libm_pow(diff / R.hue_tol, R.expo);
    return (uint32_t)rs_clamp(weight * 255.0f, 0.0f, 255.0f);   // `as u8` of a value in [0, 255]: truncation
}

// :1742-1787, this function's own rule: a = the new byte, b = the base's
PFX_DEV uint32_t range_combine(uint32_t a, uint32_t b, uint32_t mode)
{
    switch (mode) {
        case 1: return umax(a, b);
        case 2: return b - umin(a, b);   // saturating_sub
        case 3: return a * b / 255u;
        default: return a;
    }
}

// VEC: src 16-byte, base and out 4-byte aligned.  out may be base: a lane reads the bytes it writes before it writes them, and no other lane touches them
template <bool VEC>
__global__ __launch_bounds__(256) void color_range_kernel(const uint32_t* __restrict__ src, const uint8_t* base, uint8_t* out, size_t n, pfxk_color_range R)
{
    stream_walk<VEC, size_t>(n, [&](size_t g) {
        const uint4 v = reinterpret_cast<const uint4*>(src)[g];
        const uint32_t b = base ? reinterpret_cast<const uint32_t*>(base)[g] : 0u;
        reinterpret_cast<uint32_t*>(out)[g] = range_combine(range_px(v.x, R), b & 0xffu, R.combine) | (range_combine(range_px(v.y, R), (b >> 8) & 0xffu, R.combine) << 8) |
                                              (range_combine(range_px(v.z, R), (b >> 16) & 0xffu, R.combine) << 16) | (range_combine(range_px(v.w, R), b >> 24, R.combine) << 24);
    }, [&](size_t i) { out[i] = (uint8_t)range_combine(range_px(src[i], R), base ? base[i] : 0u, R.combine); });
}

} // namespace

extern "C" hipError_t pfxk_histogram(hipStream_t s, const uint8_t* d_src, const uint8_t* d_mask, size_t n, uint32_t* d_hist)
{
    hist_zero_kernel<<<4, 256, 0, s>>>(d_hist);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || n == 0) return e;
    const bool vec = aligned_to(d_src, 16) && aligned_to(d_mask, 4);
    const uint32_t blocks = std::min<uint32_t>(stream_blocks(vec ? (n + 3u) / 4u : n), PFXK_HIST_MAX_BLOCKS);
    if (vec) hist_kernel<true><<<blocks, 256, 0, s>>>((const uint32_t*)d_src, d_mask, n, d_hist);
    else hist_kernel<false><<<blocks, 256, 0, s>>>((const uint32_t*)d_src, d_mask, n, d_hist);
    return hipGetLastError();
}

extern "C" hipError_t pfxk_hsl_bands_apply(hipStream_t s, const uint8_t* d_src, uint8_t* d_dst, const uint8_t* d_mask, const pfxk_hsl_bands* B, int sparse_mode, uint32_t w,
                                           uint32_t h)
{
    if (w == 0 || h == 0) return hipSuccess;
    const uint32_t nchunks = ((w + 63u) / 64u) * ((h + 63u) / 64u);
    hsl_bands_kernel<<<nchunks, 256, 0, s>>>(d_src, d_dst, d_mask, *B, sparse_mode, w, h);
    return hipGetLastError();
}

extern "C" hipError_t pfxk_color_range_select(hipStream_t s, const uint8_t* d_src, const uint8_t* d_base, uint8_t* d_out, size_t n, const pfxk_color_range* R)
{
    if (n == 0) return hipSuccess;
    return launch_stream(aligned_to(d_src, 16) && aligned_to(d_base, 4) && aligned_to(d_out, 4), n, s, color_range_kernel<true>, color_range_kernel<false>,
                         (const uint32_t*)d_src, d_base, d_out, n, *R);
}
