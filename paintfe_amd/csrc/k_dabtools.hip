// k_dabtools.hip — the dab-list tools that write into the preview layer besides the brush: clone stamp, the heal brush's live stroke, pencil.
//
// Reference: src/ui/panels/tools/behavior/raster/clone_heal.rs — clone_stamp_circle :6-98, heal_circle :141-259, draw_pixel_and_get_bounds :295-367; the line
// stepping (:101-132, :262-292, :370-431) is host code (pfx_dabtools.cpp) and callers hand over dab centres / cells.
//
// The reference stamps serially, dab after dab, each dab looping over its box.  A dab reads and writes only the preview pixel it stands on, so the loop nest is
// interchanged as in k_brush.hip: one lane per pixel walks the dab list of its 64 x 64 chunk IN ORDER (brush_kernel<BINNED>'s layout: the host deals the dabs to
// the chunks their boxes touch, a workgroup takes four rows of an active chunk, dab centres are wave-uniform).
//
// Why the colour leaves the dab loop, exactly.  Of everything a dab computes at pixel (x, y) only the geometric alpha depends on the dab:
//   clone   the source pixel is layer(round(x + offset_x), round(y + offset_y)), the skip "source outside the canvas" tests those coordinates, and the written
//           rgb is a function of that pixel.  Its alpha byte sa scales the dab's alpha, so the one gather happens BEFORE the walk (once per pixel, not per dab);
//   heal    the ring's 48 sample coordinates depend on (x, y, sample_radius) alone, hence so do the sums, `count`, the skip `count < 1` and the written rgb.
// A dab's decision to write compares its alpha with the preview's CURRENT alpha byte (`>=` against the quantised byte: order matters, a maximum would not do),
// and what it writes is (the pixel's colour, its own alpha byte).  So the walk carries one alpha byte and one "written" flag; whichever dab wrote last, the rgb
// it wrote is the pixel's colour.  A pixel the reference skips for its source (off-canvas source, empty ring) is skipped by EVERY dab: it keeps its initial
// value, and whatever the walk tracked for it is dropped.  The ring is evaluated after the walk and only where some dab wrote.
// tests/test_dabtools_model_host.py holds this to a scalar transcription of the reference's loops.
//
// Arithmetic: single correctly rounded f32 operations in the reference's order (-ffp-contract=off); cos / sin are k_tools.h's libm_cos / libm_sin, the f64
// routine rounded once (+-1 ulp against the reference's cosf / sinf: tests/dabtools_model.py marks the pixels where that can move a sample).
// Every gather address is tested against the canvas before the load — the reference's `continue`; nothing is clamped.
#include "k_brush_math.h"
#include "k_tools.h"
#include "pfx_kernels.h"

using namespace pfxk;

namespace {

// Rust's `v as i32`: truncates, saturates, NaN -> 0
PFX_DEV int32_t as_i32(float v)
{
    if (v != v) return 0;
    if (v >= 2147483648.0f) return 2147483647;
    if (v <= -2147483648.0f) return (-2147483647 - 1);
    return (int32_t)v;
}
// `(x as f32 + d).round() as i32` inside [0, dim)?  *out = the coordinate
PFX_DEV bool sample_at(float xf, float d, uint32_t dim, uint32_t* out)
{
    const int32_t s = as_i32(__builtin_roundf(xf + d));
    *out = (uint32_t)s;
    return s >= 0 && (uint32_t)s < dim;   // dim <= 2^28
}

constexpr float TAU = 6.28318530717958647692f;

// heal_circle :205-234 — the 24 x 2 ring around (gx, gy); false = no sample inside the canvas (`count < 1`)
PFX_DEV bool heal_ring(const uint32_t* __restrict__ source, uint32_t w, uint32_t h, uint32_t gx, uint32_t gy, float sample_radius, uint32_t* rgb)
{
    const uint32_t seed = gx * 1619u + gy * 3929u;
    const float angle_offset = (float)seed / 4294967296.0f * TAU;   // u32::MAX as f32 is 2^32
    const float xf = (float)gx, yf = (float)gy;
    const float rr[2] = {sample_radius * 0.75f, sample_radius};
    float sum_r = 0.0f, sum_g = 0.0f, sum_b = 0.0f, count = 0.0f;
#pragma nounroll
    for (int i = 0; i < 24; ++i) {
        const float angle = angle_offset + ((float)i / 24.0f) * TAU;
        const float c = libm_cos(angle), s = libm_sin(angle);
        for (int k = 0; k < 2; ++k) {
            uint32_t sx, sy;
            const bool in_x = sample_at(xf, c * rr[k], w, &sx), in_y = sample_at(yf, s * rr[k], h, &sy);
            if (!in_x || !in_y) continue;
            const uint32_t sp = source[(size_t)sy * w + sx];
            sum_r += ubyte0(sp); sum_g += ubyte1(sp); sum_b += ubyte2(sp);
            count += 1.0f;
        }
    }
    if (count < 1.0f) return false;
    *rgb = pack_rgba(trunc_u8f(sum_r / count), trunc_u8f(sum_g / count), trunc_u8f(sum_b / count), 0.0f);
    return true;
}

template <int TOOL, bool AA>
__global__ __launch_bounds__(256) void dab_kernel(pfxk_dabtool T, const uint32_t* __restrict__ source, uint32_t* __restrict__ preview,
                                                  const uint8_t* __restrict__ sel, uint32_t w, uint32_t h, const pfxk_dab* __restrict__ dabs,
                                                  const uint4* __restrict__ chunks, const uint32_t* __restrict__ bins)
{
    // a wave covers one 64-pixel row segment of the chunk: gy and the segment's x range are wave-uniform
    const uint32_t lane = threadIdx.x & 63u;
    const uint4 ch = chunks[blockIdx.x];
    const uint32_t bx0 = ch.x * 64u, by0 = ch.y * 64u, bx1 = umin(bx0 + 63u, w - 1u), by1 = umin(by0 + 63u, h - 1u);
    const uint32_t n_dabs = ch.w;
    bins += ch.z;
    const uint32_t gx = bx0 + lane, gy = by0 + blockIdx.y * 4u + (threadIdx.x >> 6);
    if (gy > by1) return;   // whole wave
    const size_t i = (size_t)gy * w + umin(gx, bx1);
    bool active = gx <= bx1;
    if (active && sel && sel[i] == 0) active = false;   // :37-46
    uint32_t src_px = 0u;
    if constexpr (TOOL == PFXK_DAB_CLONE) {   // :61-67, once per pixel
        uint32_t sx, sy;
        const bool in_x = sample_at((float)gx, T.offset_x, w, &sx), in_y = sample_at((float)gy, T.offset_y, h, &sy);
        if (!in_x || !in_y) active = false;
        if (active) src_px = source[(size_t)sy * w + sx];
    }
    const uint32_t px_in = active ? preview[i] : 0u;
    const float sa = div255(ubyte3(src_px));
    uint32_t a8 = px_in >> 24;
    bool written = false;
    auto dab_px = [&](const pfxk_dab& D) {   // D is wave-uniform
        if (gx < D.x0 || gx > D.x1 || gy < D.y0 || gy > D.y1) return;   // the dab's box (host prologue)
        const float dx = (float)gx - D.cx, dy = (float)gy - D.cy;
        const float dist = __builtin_sqrtf(dx * dx + dy * dy);
        if (dist > T.radius) return;
        float alpha;
        if constexpr (TOOL == PFXK_DAB_CLONE) {   // :55-73
            const float geom = pfx_brush_alpha(dist, T.radius, T.hardness, AA);
            if (geom < 0.01f) return;
            alpha = geom * sa;
        } else {                                  // :193-203
            const float t = rs_clamp(dist / T.radius, 0.0f, 1.0f);
            if (t < T.hard_t) alpha = 1.0f;
            else {
                const float s = (t - T.hard_t) / T.hard_den;
                alpha = 1.0f - s * s * (3.0f - 2.0f * s);
            }
            if (alpha < 0.01f) return;
        }
        if (alpha >= div255((float)a8)) {         // :76 / :237 — ties overwrite
            a8 = (uint32_t)trunc_u8f(alpha * 255.0f);
            written = true;
        }
    };
    // Dab culling, 64 dabs at a time, as brush_kernel does it: lane j tests dab k0 + j's box against the wave's row segment; the dabs some lane can see are
    // walked in order, each fetched through a wave-uniform index (scalar loads).
    const uint32_t seg_lo = bx0, seg_hi = bx1;
    for (uint32_t k0 = 0; k0 < n_dabs; k0 += 64u) {
        const uint32_t kk = k0 + lane;
        uint32_t didx = 0u;
        bool seen = false;
        if (kk < n_dabs) {
            didx = bins[kk];
            const uint4 bx = reinterpret_cast<const uint4*>(&dabs[didx])[1];
            seen = !(seg_hi < bx.x || seg_lo > bx.y || gy < bx.z || gy > bx.w);
        }
        unsigned long long m = __ballot(seen);
        while (m) {
            const int j = (int)__builtin_ctzll(m);
            m &= m - 1ull;
            const uint32_t d = (uint32_t)__builtin_amdgcn_readlane((int)didx, j);
            if (active) dab_px(dabs[d]);
        }
    }
    if (!written) return;   // no cross-lane operation follows
    uint32_t out;
    if constexpr (TOOL == PFXK_DAB_CLONE) {   // :68-82: the colour's round trip through / 255 * 255
        out = pack_rgba(trunc_u8f(div255(ubyte0(src_px)) * 255.0f), trunc_u8f(div255(ubyte1(src_px)) * 255.0f), trunc_u8f(div255(ubyte2(src_px)) * 255.0f), 0.0f);
    } else {
        if (!heal_ring(source, w, h, gx, gy, T.sample_radius, &out)) return;   // :232: every dab skipped this pixel
    }
    out |= a8 << 24;
    if (out != px_in) preview[i] = out;
}

// :295-367, one lane per listed cell.  Two lanes on the same cell store the same dword: the write is idempotent
__global__ __launch_bounds__(256) void pencil_kernel(uint32_t* __restrict__ preview, const uint8_t* __restrict__ sel, uint32_t w, uint32_t h,
                                                     const int32_t* __restrict__ cells, uint32_t n, float r, float g, float b, float a)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= n) return;
    const int32_t x = cells[2 * (size_t)k], y = cells[2 * (size_t)k + 1];
    if (x < 0 || y < 0 || (uint32_t)x >= w || (uint32_t)y >= h) return;
    const size_t i = (size_t)(uint32_t)y * w + (uint32_t)x;
    if (sel && sel[i] == 0) return;
    if (a >= div255(ubyte3(preview[i]))) preview[i] = pack_rgba(trunc_u8f(r * 255.0f), trunc_u8f(g * 255.0f), trunc_u8f(b * 255.0f), trunc_u8f(a * 255.0f));
}

} // namespace

extern "C" hipError_t pfxk_dab_stroke(hipStream_t s, const pfxk_dabtool* T, const uint8_t* d_source, uint8_t* d_preview, const uint8_t* d_sel, uint32_t w, uint32_t h,
                                      const pfxk_dab* d_dabs, const uint32_t* d_chunks, uint32_t n_chunks, const uint32_t* d_bins)
{
    if (n_chunks == 0 || !dims_ok(w, h)) return hipSuccess;
    const dim3 g(n_chunks, 16);
#define PFX_DAB_GO(TOOL, AA) dab_kernel<TOOL, AA><<<g, 256, 0, s>>>(*T, (const uint32_t*)d_source, (uint32_t*)d_preview, d_sel, w, h, d_dabs, (const uint4*)d_chunks, d_bins)
    if (T->tool == PFXK_DAB_HEAL) PFX_DAB_GO(PFXK_DAB_HEAL, false);
    else if (T->anti_aliased) PFX_DAB_GO(PFXK_DAB_CLONE, true);
    else PFX_DAB_GO(PFXK_DAB_CLONE, false);
#undef PFX_DAB_GO
    return hipGetLastError();
}

extern "C" hipError_t pfxk_pencil_cells(hipStream_t s, uint8_t* d_preview, const uint8_t* d_sel, uint32_t w, uint32_t h, const int32_t* d_cells, uint32_t n, float r,
                                        float g, float b, float a)
{
    if (n == 0 || !dims_ok(w, h)) return hipSuccess;
    pencil_kernel<<<(n + 255u) / 256u, 256, 0, s>>>((uint32_t*)d_preview, d_sel, w, h, d_cells, n, r, g, b, a);
    return hipGetLastError();
}
