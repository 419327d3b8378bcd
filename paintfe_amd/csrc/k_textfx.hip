// k_textfx.hip — the text layer's styles (ref: src/ops/text_layer/effects.rs), bit for bit: every f32 expression as the reference writes it, one rounding per
// operation (no contraction), IEEE division, round() half away from zero, composite_over :47-71 in u32.
//
//   disc      dilate_mask :167-214 without its O(r^2) loop.  coverage = a / 255.0f is strictly monotone in a, so the disc's maximum of the coverage is the
//             coverage of the disc's maximum of the u8 alpha, and the erosion 1 - dilate(1 - coverage) reads the disc's minimum.  The host cuts the disc into its
//             2 ceil(r) + 1 row spans with the reference's own f32 test (pfx_textfx.cpp).  A workgroup owns 64 x 64 outputs (64 x 32 at small radii, see DISC_SMALL_R) and keeps the tile with its halo in
//             LDS as bytes, and beside it up to three more tables of that size: the maxima of every window of 4, 16 and 64 columns, each built from the one
//             below (four reads, one write per entry).  A span of L columns is then covered by at most four overlapping windows of the largest 4^k <= L:
//             at most 4 (2 ceil(r) + 1) LDS reads per output instead of the disc's area, 7 845 taps at r = 50.  The halo is ceil(r) <= 64, so the largest
//             tile is 192 x 192 x 4 tables = 144 KB of the CU's 160; the small radii of the default styles take 6 KB.  A wave reads 64 consecutive bytes of
//             one row (16 banks, four lanes to a dword: no conflict).  The minimum runs on 255 - a, which turns it into the same maximum with the same zero
//             outside the image.
//   plane     the shadows' shifted alpha, scaled by the colour's alpha: round() commutes with the disc's maximum (it is monotone), so the spread runs on
//             the scaled plane.
//   compose   one thread per pixel runs shadow, outline, fill, inside outline, inner shadow in that order on a pixel in registers and stores it once.
//   bounds    find_tight_bounds_rgba: workgroups walk whole rows, reduce in LDS and issue an atomic maximum only where it would move the box.
// Pixels are indexed in 32 bits: every image here is within pfx_dims_ok (256 Mpx).
#include "k_tools.h"
#include "pfx_kernels.h"

using namespace pfxk;

namespace {

constexpr uint32_t BX = 64, BY = 4;
constexpr uint32_t DISC_TW = 64;   // a disc workgroup's outputs are 64 columns (lane = column, wave = row) by DISC_TH rows: 32 rows and 4 waves up to a halo of
// DISC_SMALL_R (eight rows per thread; the tile is small and many workgroups share a CU), 64 rows and 16 waves above it (four rows per thread; the tables leave room
// for one workgroup per CU, so it brings its own 16 waves to cover the LDS latency: 6.8 -> 2.0 ms at r = 50, 8K; at r = 5 the small shape is 0.14 against 0.19 ms)
constexpr uint32_t DISC_SMALL_R = 8;

PFX_DEV float cov_of(uint32_t a) { return div255((float)a); }   // alpha as f32 / 255.0
// f32::round for v >= 0 (or NaN: 0), as u32; the values here are at most a little above 255
PFX_DEV uint32_t round_u32(float v)
{
    float t = __builtin_truncf(v);
    if (v - t >= 0.5f) t += 1.0f;
    return t == t ? (uint32_t)__builtin_fmaxf(t, 0.0f) : 0u;
}

// composite_over :47-71 of one pixel whose alpha sa is above 0: the stages' own loops are this formula too (at sa == 255 it gives the source)
PFX_DEV uint32_t over(uint32_t dst, uint32_t rgb, uint32_t sa)
{
    const uint32_t da = dst >> 24, inv_sa = 255u - min(sa, 255u);
    const uint32_t out_a = sa + (da * inv_sa) / 255u;
    if (out_a == 0u) return dst;
    uint32_t out = min(out_a, 255u) << 24;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const uint32_t sc = (rgb >> (8 * c)) & 0xffu, dc = (dst >> (8 * c)) & 0xffu;
        out |= min((sc * sa + dc * da * inv_sa / 255u) / out_a, 255u) << (8 * c);
    }
    return out;
}

template <bool MIN, uint32_t DISC_TH, uint32_t DISC_THREADS>
__global__ __launch_bounds__(DISC_THREADS) void disc_kernel(const uint8_t* __restrict__ src, uint32_t stride, uint32_t offset, uint8_t* __restrict__ dst, uint32_t w, uint32_t h,
                                                            uint32_t tiles_x, const pfxk_disc D)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t disc_lds[];   // [levels][ch][ls]
    const uint32_t R = (uint32_t)D.radius, cw = DISC_TW + 2u * R, ch = DISC_TH + 2u * R, ls = (cw + 3u) & ~3u, plane = ls * ch;
    const auto [x0, y0] = tile_xy<DISC_TW, DISC_TH>(tiles_x);
    constexpr uint32_t DISC_WAVES = DISC_THREADS / 64u;
    const uint32_t lx = threadIdx.x & 63u, ly = threadIdx.x >> 6;   // lane and wave: a wave takes whole tile rows, so no index is ever divided
    for (uint32_t ty = ly; ty < ch; ty += DISC_WAVES) {
        const int64_t gy = (int64_t)y0 + ty - R;
        const bool row_in = gy >= 0 && gy < (int64_t)h;
        for (uint32_t tx = lx; tx < ls; tx += 64u) {
            const int64_t gx = (int64_t)x0 + tx - R;
            uint32_t v = 0u;
            if (row_in && tx < cw && gx >= 0 && gx < (int64_t)w) {
                v = src[((size_t)gy * w + (size_t)gx) * stride + offset];
                if (MIN) v = 255u - v;
            }
            disc_lds[ty * ls + tx] = (uint8_t)v;
        }
    }
    for (uint32_t l = 1u; l < D.levels; ++l) {   // windows of 4^l columns from four of 4^(l - 1); past the row's end: nothing (no span reaches there)
        __syncthreads();
        const uint8_t* lo = disc_lds + (l - 1u) * plane;
        uint8_t* hi = disc_lds + l * plane;
        const uint32_t step = 1u << (2u * (l - 1u));
        for (uint32_t ty = ly; ty < ch; ty += DISC_WAVES)
            for (uint32_t tx = lx; tx < ls; tx += 64u) {
                const uint32_t i = ty * ls + tx;
                uint32_t m = lo[i];
#pragma unroll
                for (uint32_t k = 1u; k < 4u; ++k)
                    if (tx + k * step < ls) m = max(m, (uint32_t)lo[i + k * step]);
                hi[i] = (uint8_t)m;
            }
    }
    __syncthreads();
    // lane = column, a wave = one row; a thread keeps its rows' maxima in registers and walks the disc's rows once for all of them: the span word is
    // fetched once per disc row and the rows' reads are independent, so they are in flight together
    constexpr uint32_t ROWS = DISC_TH / DISC_WAVES;
    uint32_t acc[ROWS];
#pragma unroll
    for (uint32_t j = 0u; j < ROWS; ++j) acc[j] = 0u;
    for (uint32_t d = 0u; d <= 2u * R; ++d) {
        const uint32_t sp = D.span[d];
        if (sp == PFXK_DISC_SKIP) continue;
        const uint32_t half = sp & 0xffu, lvl = (sp >> 8) & 0xffu, reads = sp >> 16, win = 1u << (2u * lvl);
        const uint8_t* row = disc_lds + lvl * plane + (ly + d) * ls;
        const uint32_t first = lx + R - half, last = lx + R + half + 1u - win;
        for (uint32_t k = 0u; k < reads; ++k) {
            const uint32_t at = min(first + k * win, last);
#pragma unroll
            for (uint32_t j = 0u; j < ROWS; ++j) acc[j] = max(acc[j], (uint32_t)row[at + DISC_WAVES * j * ls]);
        }
    }
    const uint32_t gx = x0 + lx;
    if (gx >= w) return;
#pragma unroll
    for (uint32_t j = 0u; j < ROWS; ++j) {
        const uint32_t gy = y0 + ly + DISC_WAVES * j;
        if (gy < h) dst[(size_t)gy * w + gx] = (uint8_t)(MIN ? 255u - acc[j] : acc[j]);
    }
}

__global__ __launch_bounds__(256) void plane_kernel(const uint32_t* __restrict__ text, uint8_t* __restrict__ out, uint32_t w, uint32_t h, uint32_t tiles_x, int32_t dx,
                                                    int32_t dy, uint32_t alpha, int inner)
{
    const auto [x, y] = tile_xy<BX, BY>(tiles_x, threadIdx.x, threadIdx.y);
    if (x >= w || y >= h) return;
    const int64_t sx = (int64_t)x - dx, sy = (int64_t)y - dy;
    const bool inside = sx >= 0 && sy >= 0 && sx < (int64_t)w && sy < (int64_t)h;
    float m = inner ? 1.0f : 0.0f;
    if (inside) {
        const float cov = cov_of(text[(size_t)sy * w + (size_t)sx] >> 24);
        m = inner ? 1.0f - cov : cov;
    }
    out[(size_t)y * w + x] = (uint8_t)round_u8f(m * (float)alpha);
}

__global__ __launch_bounds__(256) void expand_kernel(const uint8_t* __restrict__ plane, uint32_t* __restrict__ rgba, size_t n, uint32_t rgb)
{
    for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (size_t)gridDim.x * 256u) rgba[i] = rgb | ((uint32_t)plane[i] << 24);
}

// `v as usize` for the texture's column / row: NaN -> 0, never negative here, and below 2^32 for a texture within the document limit
PFX_DEV uint32_t as_index(float v) { return v == v ? (uint32_t)__builtin_fminf(__builtin_fmaxf(v, 0.0f), 4294967040.0f) : 0u; }

// the outlines' alpha from the two coverages of `a - b`: 0 = skipped
PFX_DEV uint32_t outline_alpha(float a, float b, float oa)
{
    const float alpha = rs_clamp(a - b, 0.0f, 1.0f) * oa;
    if (alpha < 1.0f / 255.0f) return 0u;
    return round_u32(alpha * 255.0f);
}

__global__ __launch_bounds__(256) void compose_kernel(const uint32_t* __restrict__ text, const uint32_t* __restrict__ texture, uint32_t* __restrict__ out, uint32_t tiles_x,
                                                      const pfxk_textfx P)
{
    const auto [x, y] = tile_xy<BX, BY>(tiles_x, threadIdx.x, threadIdx.y);
    if (x >= P.w || y >= P.h) return;
    const size_t at = (size_t)y * P.w + x;
    const uint32_t t = text[at], ta = t >> 24;
    const float cov = cov_of(ta);
    const bool covered = !(cov < 1.0f / 255.0f);
    uint32_t px = 0u;
    if (P.flags & PFXK_TFX_SHADOW) {
        uint32_t rgb = P.shadow_rgb, sa;
        if (P.flags & PFXK_TFX_SHADOW_RGBA) { const uint32_t s = ((const uint32_t*)P.shadow)[at]; rgb = s & 0xffffffu; sa = s >> 24; }
        else sa = P.shadow[at];
        if (sa) px = over(px, rgb, sa);
    }
    if (P.flags & PFXK_TFX_OUTLINE_OUT) {
        const uint32_t sa = outline_alpha(cov_of(P.dilated[at]), cov, P.outline_oa);
        if (sa) px = over(px, P.outline_rgb, sa);
    }
    if (P.flags & PFXK_TFX_GRADIENT) {
        if (covered) {
            const float proj = (((float)x - P.g_off_x) * P.g_dir_x + ((float)y - P.g_off_y) * P.g_dir_y) / P.g_scale;
            float g;
            if (P.flags & PFXK_TFX_GRADIENT_REPEAT) { g = fmodf(proj, 1.0f); if (g < 0.0f) g = g + 1.0f; }   // rem_euclid(1.0)
            else g = rs_clamp(proj, 0.0f, 1.0f);
            const float inv_g = 1.0f - g;
            const uint32_t s = P.g_start, e = P.g_end;
            const uint32_t rgb = (uint32_t)round_u8f(ubyte0(s) * inv_g + ubyte0(e) * g) | ((uint32_t)round_u8f(ubyte1(s) * inv_g + ubyte1(e) * g) << 8) |
                                 ((uint32_t)round_u8f(ubyte2(s) * inv_g + ubyte2(e) * g) << 16);
            const uint32_t sa = (uint32_t)round_u8f((ubyte3(s) * inv_g + ubyte3(e) * g) * cov);
            if (sa) px = over(px, rgb, sa);
        }
    } else if (P.flags & PFXK_TFX_TEXTURE) {
        if (covered) {
            const float tw = (float)P.tex_w, th = (float)P.tex_h;
            const float tx_f = fmodf(((float)x - P.t_off_x) / P.t_scale, tw), ty_f = fmodf(((float)y - P.t_off_y) / P.t_scale, th);
            const uint32_t tx = as_index(tx_f + tw) % P.tex_w, ty = as_index(ty_f + th) % P.tex_h;
            const uint32_t tp = texture[(size_t)ty * P.tex_w + tx];
            const uint32_t sa = min((uint32_t)round_u8f(cov * 255.0f), tp >> 24);
            if (sa) px = over(px, tp & 0xffffffu, sa);
        }
    } else if (ta) {
        px = over(px, t & 0xffffffu, ta);
    }
    if (P.flags & PFXK_TFX_OUTLINE_IN) {
        const float eroded = __builtin_fmaxf(1.0f - (1.0f - cov_of(P.eroded[at])), 0.0f);
        const uint32_t sa = outline_alpha(cov, eroded, P.outline_oa);
        if (sa) px = over(px, P.outline_rgb, sa);
    }
    if ((P.flags & PFXK_TFX_INNER) && covered) {
        uint32_t rgb = P.inner_rgb, sa;
        if (P.flags & PFXK_TFX_INNER_BLURRED) {
            uint32_t ba;
            if (P.flags & PFXK_TFX_INNER_RGBA) { const uint32_t s = ((const uint32_t*)P.inner)[at]; rgb = s & 0xffffffu; ba = s >> 24; }
            else ba = P.inner[at];
            sa = round_u32((float)ba * cov);
        } else {
            const int64_t sx = (int64_t)x - P.inner_dx, sy = (int64_t)y - P.inner_dy;
            float inv = 1.0f;
            if (sx >= 0 && sy >= 0 && sx < (int64_t)P.w && sy < (int64_t)P.h) inv = 1.0f - cov_of(text[(size_t)sy * P.w + (size_t)sx] >> 24);
            sa = (uint32_t)round_u8f(inv * P.inner_ia * cov);
        }
        if (sa) px = over(px, rgb, sa);
    }
    out[at] = px;
}

// a workgroup walks whole rows, so x and y need no division; its four waves meet in LDS, and it touches the five words only where it would move them (the
// plain reads may be stale: the atomic then decides)
__global__ __launch_bounds__(256) void bounds_kernel(const uint32_t* __restrict__ img, uint32_t w, uint32_t h, uint32_t* got)
{
    __shared__ uint32_t part[4][4];
    uint32_t nx = 0u, ny = 0u, mx = 0u, my = 0u;   // maxima of ~x, ~y, x, y
    bool found = false;
    for (uint32_t y = blockIdx.x; y < h; y += gridDim.x) {
        const uint32_t* row = img + (size_t)y * w;
        bool in_row = false;
        for (uint32_t x = threadIdx.x; x < w; x += 256u)
            if ((row[x] >> 24) != 0u) { nx = max(nx, ~x); mx = max(mx, x); in_row = true; }
        if (in_row) { ny = max(ny, ~y); my = max(my, y); found = true; }
    }
    for (int off = 32; off >= 1; off >>= 1) {
        nx = max(nx, (uint32_t)__shfl_xor((int)nx, off)); ny = max(ny, (uint32_t)__shfl_xor((int)ny, off));
        mx = max(mx, (uint32_t)__shfl_xor((int)mx, off)); my = max(my, (uint32_t)__shfl_xor((int)my, off));
    }
    const bool any = __syncthreads_or(found);
    if ((threadIdx.x & 63u) == 0u) { uint32_t* p = part[threadIdx.x >> 6]; p[0] = nx; p[1] = ny; p[2] = mx; p[3] = my; }
    __syncthreads();
    if (!any || threadIdx.x >= 4u) return;
    const uint32_t k = threadIdx.x, v = max(max(part[0][k], part[1][k]), max(part[2][k], part[3][k]));
    // a workgroup that saw no pixel in some direction holds 0 there, which moves nothing
    if (v > got[k]) atomicMax(got + k, v);
    if (k == 0u && got[4] == 0u) atomicOr(got + 4, 1u);
}

} // namespace

extern "C" hipError_t pfxk_textfx_disc(hipStream_t s, const uint8_t* d_src, uint32_t src_stride, uint32_t src_offset, uint8_t* d_dst, uint32_t w, uint32_t h,
                                       const pfxk_disc* D, int take_min)
{
    if (!D || !dims_ok(w, h) || D->radius < 1 || D->radius > PFXK_TEXTFX_MAX_RADIUS || D->levels < 1u || D->levels > 4u || !src_stride || src_offset >= src_stride)
        return hipErrorInvalidValue;
    const uint32_t R = (uint32_t)D->radius;
    for (uint32_t d = 0; d <= 2u * R; ++d) {   // a span the tile cannot serve would read LDS out of bounds: refuse it here
        const uint32_t sp = D->span[d];
        if (sp == PFXK_DISC_SKIP) continue;
        const uint32_t half = sp & 0xffu, lvl = (sp >> 8) & 0xffu, reads = sp >> 16, win = 1u << (2u * lvl);
        if (half > R || lvl >= D->levels || win > 2u * half + 1u || reads < 1u || (uint64_t)reads * win < 2u * half + 1u) return hipErrorInvalidValue;
    }
    const bool small = R <= DISC_SMALL_R;
    const uint32_t th = small ? 32u : 64u, threads = small ? 256u : 1024u;
    const uint32_t ls = (DISC_TW + 2u * R + 3u) & ~3u, lds = D->levels * ls * (th + 2u * R);
    const uint32_t tiles_x = (w + DISC_TW - 1u) / DISC_TW, blocks = tiles_x * ((h + th - 1u) / th);
    auto launch = [&](auto kernel, lds_grant& g) -> hipError_t {
        if (hipError_t e = grant_lds(g, (const void*)kernel, lds)) return e;
        kernel<<<blocks, threads, lds, s>>>(d_src, src_stride, src_offset, d_dst, w, h, tiles_x, *D);
        return hipGetLastError();
    };
    static lds_grant g_max, g_min, g_max_small, g_min_small;
    if (small) return take_min ? launch(disc_kernel<true, 32, 256>, g_min_small) : launch(disc_kernel<false, 32, 256>, g_max_small);
    return take_min ? launch(disc_kernel<true, 64, 1024>, g_min) : launch(disc_kernel<false, 64, 1024>, g_max);
}

extern "C" hipError_t pfxk_textfx_plane(hipStream_t s, const uint8_t* d_text, uint8_t* d_plane, uint32_t w, uint32_t h, int32_t dx, int32_t dy, uint32_t alpha, int inner)
{
    if (!dims_ok(w, h) || alpha > 255u) return hipErrorInvalidValue;
    uint32_t tiles_x;
    const uint32_t blocks = tile_grid<BX, BY>(w, h, &tiles_x);
    plane_kernel<<<blocks, dim3(BX, BY), 0, s>>>((const uint32_t*)d_text, d_plane, w, h, tiles_x, dx, dy, alpha, inner);
    return hipGetLastError();
}

extern "C" hipError_t pfxk_textfx_expand(hipStream_t s, const uint8_t* d_plane, uint8_t* d_rgba, size_t n, uint32_t rgb)
{
    if (n == 0) return hipSuccess;
    const size_t b = (n + 255u) / 256u;
    expand_kernel<<<(uint32_t)(b > 16384u ? 16384u : b), 256, 0, s>>>(d_plane, (uint32_t*)d_rgba, n, rgb & 0xffffffu);
    return hipGetLastError();
}

extern "C" hipError_t pfxk_textfx_compose(hipStream_t s, const uint8_t* d_text, const uint8_t* d_texture, uint8_t* d_out, const pfxk_textfx* P)
{
    if (!P || !dims_ok(P->w, P->h)) return hipErrorInvalidValue;
    const uint32_t f = P->flags;
    if (((f & PFXK_TFX_SHADOW) && !P->shadow) || ((f & PFXK_TFX_OUTLINE_OUT) && !P->dilated) || ((f & PFXK_TFX_OUTLINE_IN) && !P->eroded) ||
        ((f & PFXK_TFX_INNER_BLURRED) && !P->inner) || ((f & PFXK_TFX_TEXTURE) && (!d_texture || !dims_ok(P->tex_w, P->tex_h))))
        return hipErrorInvalidValue;
    uint32_t tiles_x;
    const uint32_t blocks = tile_grid<BX, BY>(P->w, P->h, &tiles_x);
    compose_kernel<<<blocks, dim3(BX, BY), 0, s>>>((const uint32_t*)d_text, (const uint32_t*)d_texture, (uint32_t*)d_out, tiles_x, *P);
    return hipGetLastError();
}

extern "C" hipError_t pfxk_textfx_bounds(hipStream_t s, const uint8_t* d_img, uint32_t w, uint32_t h, uint32_t* d_got)
{
    if (!dims_ok(w, h)) return hipErrorInvalidValue;
    bounds_kernel<<<h > 2048u ? 2048u : h, 256, 0, s>>>((const uint32_t*)d_img, w, h, d_got);
    return hipGetLastError();
}
