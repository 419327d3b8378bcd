// k_linetool.hip — the line / curve tool: the Bezier's dots and arrowheads into the preview layer, and the mask-target release.
//
// Reference: src/ui/panels/tools/behavior/raster/bezier_math.rs — rasterize_bezier :76-286 (the clear :117-129, the dot list :131-195, the arrowheads
// :212-284), draw_filled_triangle :289-373, draw_bezier_circle_with_hardness :456-526; compute_line_alpha, brush_render.rs:85-133; commit_preview_to_layer_mask,
// bezier_commit.rs:229-295.  The dot list, the triangles' vertices and every quantity that is uniform over a call are host code (pfx_linetool.cpp).
//
// The reference draws serially: 20 to 5000 overlapping circles, then up to two triangles, each looping over its own box and writing a pixel iff its
// pixel_alpha is strictly above the pixel's CURRENT alpha byte / 255.  Every primitive of a call writes the same rgb, and the byte a write leaves,
// (pixel_alpha * 255.0) as u8, is never below the byte it beat (enumerated for all 256 bytes in tests/test_linetool_model_host.py: truncation is monotone).
// So the serial walk equals: A = the maximum pixel_alpha over the primitives that cover the pixel; if A > old_a / 255.0 write (rgb, (A * 255.0) as u8), else
// leave the pixel alone.  The maximum is over pixel_alpha, never over distances: the f32 smoothstep need not be monotone to the last ulp.  The primitives are
// exactly the reference's, box tests included.  The same test file holds the maximum form to a loop-for-loop transcription on every case.
//
// Layout: brush_kernel<BINNED>'s (k_brush.hip, k_dabtools.hip).  The host deals the dots to the 64 x 64 chunks their boxes touch; a workgroup takes four rows of
// a chunk of the launch, a wave one 64-pixel row segment, a lane one pixel; dot data is wave-uniform (fetched through a readlane'd index: scalar loads), the two
// triangles sit in the kernel's parameter struct (scalar registers).  The launch's chunks are the union of the chunks to clear (TiledImage::clear_region, chunk
// granular) and the chunks that are drawn into: a pixel of a cleared chunk starts from 0 and is never read, any other starts from the preview, so a focused frame
// is one pass with at most one read and one write per pixel.
//
// The dot's selection gate (:189, the byte at the dot's OWN cell) happens here, in the cull step: the lane that tests dot k's box against the wave's row segment
// also loads that dot's selection byte.  A per-dot keep flag from a pre-kernel was the alternative; it costs a launch and a dependent pass per frame (a drag
// frame is a handful of microseconds of work), while this load rides in a step that already gathers 32 bytes per dot, only for dots whose box meets the segment.
//
// Arithmetic: single correctly rounded f32 operations in the reference's order (-ffp-contract=off, correctly rounded sqrt and divide); no libm call per pixel.
// Every address is tested against the canvas before it is used; nothing is clamped.
#include "k_tools.h"
#include "pfx_kernels.h"

using namespace pfxk;

namespace {

// compute_line_alpha * src_a for one dot at (gx, gy); 0 = the dot skips the pixel (`alpha <= 0.0`)
template <bool AA>
PFX_DEV float dot_alpha(const pfxk_line& L, const pfxk_line_dot& D, uint32_t gx, uint32_t gy)
{
    const float dx = (float)gx - D.cx, dy = (float)gy - D.cy;   // :496-498, no half-pixel offset
    const float dist = __builtin_sqrtf(dx * dx + dy * dy);
    float alpha;
    if constexpr (!AA) {
        if (!(dist < L.radius)) return 0.0f;                    // brush_render.rs:94
        alpha = 1.0f;
    } else {
        if (dist <= L.solid_radius) alpha = 1.0f;               // :120-124
        else if (dist >= L.eff_radius) return 0.0f;
        else {
            const float t = (dist - L.solid_radius) / L.fade_width;
            const float x = 1.0f - rs_clamp(t, 0.0f, 1.0f);
            alpha = x * x * (3.0f - 2.0f * x);
            if (alpha <= 0.0f) return 0.0f;                     // :503
        }
    }
    return alpha * L.src_a;
}

// draw_filled_triangle :335-359 at pixel (gx, gy): the alpha it offers, 0 (or NaN, which loses every comparison as in the reference) = none
PFX_DEV float tri_alpha(const pfxk_line_tri& T, float src_a, uint32_t gx, uint32_t gy)
{
    const float px = (float)gx + 0.5f, py = (float)gy + 0.5f;
    float d[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) d[k] = ((T.ex[k] * (py - T.vy[k]) - T.ey[k] * (px - T.vx[k])) / T.len[k]) * T.sign;   // edge_dist :315-320
    const float min_dist = __builtin_fminf(__builtin_fminf(d[0], d[1]), d[2]);   // f32::min: a NaN operand yields the other
    if (min_dist < -1.0f) return 0.0f;
    if (min_dist >= 1.0f) return src_a;
    const float t = rs_clamp((min_dist + 1.0f) / 2.0f, 0.0f, 1.0f);
    const float smooth = t * t * (3.0f - 2.0f * t);
    return smooth * src_a;
}

template <bool AA>
__global__ __launch_bounds__(256) void line_kernel(pfxk_line L, uint32_t* __restrict__ preview, const uint8_t* __restrict__ sel, uint32_t w, uint32_t h,
                                                   const pfxk_line_dot* __restrict__ dots, const uint4* __restrict__ chunks, const uint32_t* __restrict__ bins)
{
    // a wave covers one 64-pixel row segment of the chunk: gy and the segment's x range are wave-uniform
    const uint32_t lane = threadIdx.x & 63u;
    const uint4 ch = chunks[2u * blockIdx.x], ch2 = chunks[2u * blockIdx.x + 1u];
    if (ch.x > (w - 1u) / 64u || ch.y > (h - 1u) / 64u) return;   // a chunk outside the canvas: not from this host, and nothing of it is addressed
    const uint32_t bx0 = ch.x * 64u, by0 = ch.y * 64u, bx1 = umin(bx0 + 63u, w - 1u), by1 = umin(by0 + 63u, h - 1u);
    const uint32_t n_dots = ch.w, flags = ch2.x;
    bins += ch.z;
    const uint32_t gx = bx0 + lane, gy = by0 + blockIdx.y * 4u + (threadIdx.x >> 6);
    if (gy > by1) return;   // whole wave
    const bool inside = gx <= bx1, cleared = (flags & PFXK_LINE_CLEAR) != 0u;
    const size_t i = (size_t)gy * w + umin(gx, bx1);
    const bool paints = inside && !(sel && sel[i] == 0);   // :492 / :332 — the pixel's own selection byte
    const uint32_t px_in = (inside && !cleared) ? preview[i] : 0u;
    float best = 0.0f;   // the maximum pixel_alpha; a NaN never replaces it
    // Dot culling, 64 dots at a time, as brush_kernel does it: lane j tests dot k0 + j's box against the wave's row segment and reads the dot's selection
    // byte; the dots some lane can see are walked, each fetched through a wave-uniform index
    for (uint32_t k0 = 0; k0 < n_dots; k0 += 64u) {
        const uint32_t kk = k0 + lane;
        uint32_t didx = 0u;
        bool seen = false;
        if (kk < n_dots) {
            didx = bins[kk];
            const uint4 bx = reinterpret_cast<const uint4*>(&dots[didx])[1];
            seen = !(bx1 < bx.x || bx0 > bx.y || gy < bx.z || gy > bx.w);
            if (seen && sel) {   // :189
                const uint4 hd = reinterpret_cast<const uint4*>(&dots[didx])[0];
                seen = hd.z < w && hd.w < h && sel[(size_t)hd.w * w + hd.z] != 0;
            }
        }
        unsigned long long m = __ballot(seen);
        while (m) {
            const int j = (int)__builtin_ctzll(m);
            m &= m - 1ull;
            const uint32_t d = (uint32_t)__builtin_amdgcn_readlane((int)didx, j);
            const pfxk_line_dot& D = dots[d];
            if (paints && gx >= D.x0 && gx <= D.x1 && gy >= D.y0 && gy <= D.y1) {
                const float pa = dot_alpha<AA>(L, D, gx, gy);
                if (pa > best) best = pa;
            }
        }
    }
#pragma unroll
    for (uint32_t k = 0; k < 2u; ++k) {
        if (k >= L.n_tris || !(flags & (PFXK_LINE_TRI0 << k))) continue;   // uniform
        const pfxk_line_tri& T = L.tri[k];
        if (paints && gx >= T.x0 && gx <= T.x1 && gy >= T.y0 && gy <= T.y1) {
            const float pa = tri_alpha(T, L.src_a, gx, gy);
            if (pa > best) best = pa;
        }
    }
    if (!inside) return;   // no cross-lane operation follows
    uint32_t out = px_in;
    if (best > div255(ubyte3(px_in))) out = L.rgb | ((uint32_t)trunc_u8f(best * 255.0f) << 24);   // :516-522 / :363-369, the strict `>`
    if (cleared || out != px_in) preview[i] = out;
}

// bezier_commit.rs:262-291, one lane per pixel
__global__ __launch_bounds__(256) void commit_mask_kernel(uint8_t* __restrict__ conceal, const uint32_t* __restrict__ preview, const uint8_t* __restrict__ sel, uint32_t n,
                                                          int reveal)
{
    stream_walk<false, uint32_t>(n, [](uint32_t) {}, [&](uint32_t i) {
        if (sel && sel[i] == 0) return;
        const uint32_t s = preview[i] >> 24;
        if (s == 0u) return;
        const uint32_t old = conceal[i];
        conceal[i] = (uint8_t)(reveal ? (old * (255u - s)) / 255u : old + ((255u - old) * s) / 255u);
    });
}

} // namespace

extern "C" hipError_t pfxk_line_render(hipStream_t s, const pfxk_line* L, uint8_t* d_preview, const uint8_t* d_sel, uint32_t w, uint32_t h, const pfxk_line_dot* d_dots,
                                       const uint32_t* d_chunks, uint32_t n_chunks, const uint32_t* d_bins)
{
    if (n_chunks == 0 || !dims_ok(w, h)) return hipSuccess;
    const dim3 g(n_chunks, 16);
    if (L->anti_alias) line_kernel<true><<<g, 256, 0, s>>>(*L, (uint32_t*)d_preview, d_sel, w, h, d_dots, (const uint4*)d_chunks, d_bins);
    else line_kernel<false><<<g, 256, 0, s>>>(*L, (uint32_t*)d_preview, d_sel, w, h, d_dots, (const uint4*)d_chunks, d_bins);
    return hipGetLastError();
}

extern "C" hipError_t pfxk_line_commit_mask(hipStream_t s, uint8_t* d_conceal, const uint8_t* d_preview, const uint8_t* d_sel, uint32_t w, uint32_t h, int reveal)
{
    if (!dims_ok(w, h)) return hipSuccess;
    const size_t n = (size_t)w * h;
    commit_mask_kernel<<<stream_blocks(n), 256, 0, s>>>(d_conceal, (const uint32_t*)d_preview, d_sel, (uint32_t)n, reveal);
    return hipGetLastError();
}
