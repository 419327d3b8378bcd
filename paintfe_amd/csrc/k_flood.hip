// k_flood.hip — bucket fill and magic wand (ref: src/ui/panels/tools/behavior/raster/fill_magic.rs, tools/state.rs:574-735), the CPU flavour bit for bit.
//
//   colour distance  pixel_color_distance :1048 / perceptual_distance :93: a streaming RGBA8 -> u8 map, 16-byte loads.  The perceptual mode is the reference's
//                    f32 expression in its written order (no contraction, one correctly rounded sqrt); its only transcendental, powf of k / 255, is a
//                    256-entry table the host fills with the host libm, held in LDS.
//   connected flood  compute_flood_distance_map :950 computes d[p] = min over paths seed -> p of the largest c on the path with a 256-bucket queue.  Here a
//                    workgroup owns a 64 x 64 tile: it loads c, d and a one-pixel halo of d into LDS and relaxes d[p] = min(d[p], max(d[q], c[p])) over the
//                    neighbours q in four directional sweeps until a round changes nothing (or PFXK_FLOOD_TILE_ITERS rounds), then writes the tile back.
//                    Nothing waits on another workgroup: the host launches pass after pass over the list of tiles whose halo may have improved (DESIGN.md
//                    "Flood distance maps" has the fixed-point argument).  4-connected sweeps are independent scans (a thread per row, then per column);
//                    an 8-connected sweep step reads what other threads wrote in the step before, so every step ends in a barrier.
//   pointwise        threshold_alpha :415 + merge_magic_wand_masks :486, build_fill_preview_region :550, and the preview blended into the layer in one
//                    kernel (commit_fill_preview_impl :1414-1446: blend_pixel_static(layer, preview, mode, 1.0) where the preview's alpha is > 0).
//   bounding boxes   ThresholdRegionIndex::from_distances (state.rs:693): per-distance min / max in LDS, merged into a 256 x 4 table with atomics.
#include "k_tools.h"
#include "k_blend.h"
#include "pfx_kernels.h"

using namespace pfxk;

namespace {

constexpr int T = PFXK_FLOOD_TILE;
constexpr int PITCH = 68;   // bytes per LDS row: 17 dwords, so the 64 rows of one column fall on different banks

PFX_DEV uint32_t absdiff_u(uint32_t a, uint32_t b) { return a > b ? a - b : b - a; }

template <int MODE>
PFX_DEV uint32_t color_distance(uint32_t p, const pfxk_flood_target& G, const float* lin)
{
    const uint32_t t = G.rgba;
    if ((t >> 24) == 0u && (p >> 24) == 0u) return 0u;   // both transparent (:1065; the perceptual `ta <= 0.0 && a <= 0.0` :105 is the same test)
    if constexpr (MODE == 0) {
        const uint32_t dr = absdiff_u(p & 0xffu, t & 0xffu), dg = absdiff_u((p >> 8) & 0xffu, (t >> 8) & 0xffu);
        const uint32_t db = absdiff_u((p >> 16) & 0xffu, (t >> 16) & 0xffu), da = absdiff_u(p >> 24, t >> 24);
        return umax(umax(dr, dg), umax(db, da));
    } else {
        const float a = div255(ubyte3(p));
        const float dr = lin[p & 0xffu] * a - G.lin[0];
        const float dg = lin[(p >> 8) & 0xffu] * a - G.lin[1];
        const float db = lin[(p >> 16) & 0xffu] * a - G.lin[2];
        const float dluma = __builtin_fabsf(0.2126f * dr + 0.7152f * dg + 0.0722f * db);
        const float dchroma = __builtin_sqrtf(0.5f * (dr - dg) * (dr - dg) + 0.5f * (dg - db) * (dg - db) + 0.5f * (db - dr) * (db - dr));
        const float color_term = rs_clamp(dluma * 0.7f + dchroma * 0.8f, 0.0f, 1.0f);
        const float alpha_term = __builtin_fabsf(a - G.ta);
        return (uint32_t)round_u8f(__builtin_fmaxf(color_term, alpha_term) * 255.0f);
    }
}

// VEC: src is 16-byte and out 4-byte aligned — four pixels per thread; the n % 4 tail and the other case go pixel by pixel (src is 4-byte aligned: the host checks)
template <int MODE, bool VEC>
__global__ __launch_bounds__(256) void color_distance_kernel(const uint32_t* __restrict__ src, uint8_t* __restrict__ out, size_t n, pfxk_flood_target G,
                                                             const float* __restrict__ table)
{
    __shared__ float lin[256];
    if constexpr (MODE == 1) {
        lin[threadIdx.x] = table[threadIdx.x];
        __syncthreads();
    }
    stream_walk<VEC, size_t>(n, [&](size_t g) {
        const uint4 v = reinterpret_cast<const uint4*>(src)[g];
        reinterpret_cast<uint32_t*>(out)[g] = color_distance<MODE>(v.x, G, lin) | (color_distance<MODE>(v.y, G, lin) << 8) |
                                              (color_distance<MODE>(v.z, G, lin) << 16) | (color_distance<MODE>(v.w, G, lin) << 24);
    }, [&](size_t i) { out[i] = (uint8_t)color_distance<MODE>(src[i], G, lin); });
}

// the first pass's list is the seed's tile.  d[seed] itself stays 255 in memory: the first pass lowers it to c[seed] inside the tile (flood_pass_kernel), so
// the seed counts as a pixel that decreased and its neighbours across a tile border are scheduled like any other's
__global__ void flood_seed_kernel(uint32_t w, uint32_t seed_x, uint32_t seed_y, uint32_t* __restrict__ list)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) list[0] = (seed_y / T) * ((w + T - 1) / T) + seed_x / T;
}

// bits a tile raises when it is written back
enum { FB_SELF = 1, FB_L = 2, FB_R = 4, FB_T = 8, FB_B = 16, FB_TL = 32, FB_TR = 64, FB_BL = 128, FB_BR = 256, FB_CHANGED = 512 };

template <int CONN>
__global__ __launch_bounds__(64) void flood_pass_kernel(const uint8_t* __restrict__ c, uint8_t* d, uint32_t w, uint32_t h, const uint32_t* __restrict__ list,
                                                        uint32_t* next, uint32_t* state, uint32_t* mark, uint32_t stamp, uint32_t tiles_x, uint32_t tiles_y,
                                                        uint32_t seed_x, uint32_t seed_y /* the first pass: the seed; later passes: >= w, h */)
{
    __shared__ uint8_t sD[(T + 2) * PITCH];   // d over rows / columns -1 .. 64
    __shared__ uint8_t sC[T * PITCH];
    __shared__ uint8_t s0[T * T];             // d as loaded: what the write-back compares with
    __shared__ uint32_t s_bits;
#define D(r, x) sD[((r) + 1) * PITCH + (x) + 1]
#define CC(r, x) sC[(r) * PITCH + (x)]
    const int t = (int)threadIdx.x;
    const uint32_t tile = list[blockIdx.x];
    if (tile >= tiles_x * tiles_y) return;   // uniform; the host never lists one
    const int tx = (int)(tile % tiles_x), ty = (int)(tile / tiles_x);
    const int x0 = tx * T, y0 = ty * T;
    if (t == 0) s_bits = 0u;
    // pixels outside the image count as d = c = 255: they never change and never lower a neighbour
    for (int r = -1; r <= T; ++r) {
        const int gy = y0 + r;
        const bool row_in = gy >= 0 && gy < (int)h;
        const int gx = x0 + t;
        uint8_t v = 255, cv = 255;
        if (row_in && gx < (int)w) {
            v = d[(size_t)gy * w + gx];
            if (r >= 0 && r < T) cv = c[(size_t)gy * w + gx];
        }
        D(r, t) = v;
        if (r >= 0 && r < T) {
            CC(r, t) = cv;
            s0[r * T + t] = v;
        }
        if (t < 2) {
            const int hx = t == 0 ? x0 - 1 : x0 + T;
            uint8_t hv = 255;
            if (row_in && hx >= 0 && hx < (int)w) hv = d[(size_t)gy * w + hx];
            D(r, t == 0 ? -1 : T) = hv;
        }
    }
    // the first pass plants the seed: d[seed] = c[seed] (:966-967), as a decrease from the 255 in memory (s0 keeps 255)
    if (seed_x < w && seed_y < h && (int)(seed_x / T) == tx && (int)(seed_y / T) == ty && t == (int)(seed_x % T)) {
        const int sr = (int)(seed_y % T);
        if (CC(sr, t) < D(sr, t)) D(sr, t) = CC(sr, t);
    }
    __syncthreads();

    bool capped = false;
    for (int round = 1;; ++round) {
        int ch = 0;
#define RELAX(r, x, from)                                          \
    {                                                              \
        const uint32_t cur = D(r, x), nv = umax((from), CC(r, x)); \
        if (nv < cur) {                                            \
            D(r, x) = (uint8_t)nv;                                 \
            ch = 1;                                                \
            v = nv;                                                \
        } else v = cur;                                            \
    }
        if constexpr (CONN == 4) {
            uint32_t v = D(t, -1);   // a thread per row: left to right, right to left
#pragma unroll 8
            for (int x = 0; x < T; ++x) RELAX(t, x, v)
            v = D(t, T);
#pragma unroll 8
            for (int x = T - 1; x >= 0; --x) RELAX(t, x, v)
            __syncthreads();
            v = D(-1, t);            // a thread per column: top to bottom, bottom to top
#pragma unroll 8
            for (int y = 0; y < T; ++y) RELAX(y, t, v)
            v = D(T, t);
#pragma unroll 8
            for (int y = T - 1; y >= 0; --y) RELAX(y, t, v)
        } else {
            uint32_t v;   // every step reads the line the step before wrote, other threads' pixels included
            for (int x = 0; x < T; ++x) {
                RELAX(t, x, umin(umin(D(t - 1, x - 1), D(t, x - 1)), D(t + 1, x - 1)))
                __syncthreads();
            }
            for (int x = T - 1; x >= 0; --x) {
                RELAX(t, x, umin(umin(D(t - 1, x + 1), D(t, x + 1)), D(t + 1, x + 1)))
                __syncthreads();
            }
            for (int y = 0; y < T; ++y) {
                RELAX(y, t, umin(umin(D(y - 1, t - 1), D(y - 1, t)), D(y - 1, t + 1)))
                __syncthreads();
            }
            for (int y = T - 1; y >= 0; --y) {
                RELAX(y, t, umin(umin(D(y + 1, t - 1), D(y + 1, t)), D(y + 1, t + 1)))
                __syncthreads();
            }
            (void)v;
        }
#undef RELAX
        if (!__syncthreads_or(ch)) break;   // a barrier as well: the next round's row sweep reads this round's columns
        if (round >= PFXK_FLOOD_TILE_ITERS) {
            capped = true;
            break;
        }
    }

    // write back what decreased.  A neighbour is scheduled when a border pixel that decreased is now below a pixel of that neighbour beside it (as read at the
    // start: memory only decreases, so the test can only err towards scheduling)
    uint32_t bits = capped ? (uint32_t)FB_SELF : 0u;
    for (int r = 0; r < T; ++r) {
        const uint32_t nv = D(r, t), ov = s0[r * T + t];
        if (nv < ov) {   // inside the image: a pixel outside stays 255
            d[(size_t)(y0 + r) * w + (x0 + t)] = (uint8_t)nv;
            bits |= FB_CHANGED;
            if (t == 0 && nv < (CONN == 8 ? umax(umax(D(r - 1, -1), D(r, -1)), D(r + 1, -1)) : (uint32_t)D(r, -1))) bits |= FB_L;
            if (t == T - 1 && nv < (CONN == 8 ? umax(umax(D(r - 1, T), D(r, T)), D(r + 1, T)) : (uint32_t)D(r, T))) bits |= FB_R;
            if (r == 0 && nv < (CONN == 8 ? umax(umax(D(-1, t - 1), D(-1, t)), D(-1, t + 1)) : (uint32_t)D(-1, t))) bits |= FB_T;
            if (r == T - 1 && nv < (CONN == 8 ? umax(umax(D(T, t - 1), D(T, t)), D(T, t + 1)) : (uint32_t)D(T, t))) bits |= FB_B;
            if constexpr (CONN == 8) {
                if (r == 0 && t == 0 && nv < D(-1, -1)) bits |= FB_TL;
                if (r == 0 && t == T - 1 && nv < D(-1, T)) bits |= FB_TR;
                if (r == T - 1 && t == 0 && nv < D(T, -1)) bits |= FB_BL;
                if (r == T - 1 && t == T - 1 && nv < D(T, T)) bits |= FB_BR;
            }
        }
    }
    if (bits) atomicOr(&s_bits, bits);
    __syncthreads();
    if (t == 0 && s_bits != 0u) {
        const uint32_t b = s_bits;
        atomicOr(&state[1], 1u);
        auto push = [&](int dx, int dy) {
            const int nx = tx + dx, ny = ty + dy;
            if (nx < 0 || ny < 0 || nx >= (int)tiles_x || ny >= (int)tiles_y) return;
            const uint32_t nt = (uint32_t)ny * tiles_x + (uint32_t)nx;
            if (atomicExch(&mark[nt], stamp) != stamp) {   // once per pass
                const uint32_t k = atomicAdd(&state[0], 1u);
                if (k < tiles_x * tiles_y) next[k] = nt;
            }
        };
        if (b & FB_SELF) push(0, 0);
        if (b & FB_L) push(-1, 0);
        if (b & FB_R) push(1, 0);
        if (b & FB_T) push(0, -1);
        if (b & FB_B) push(0, 1);
        if (b & FB_TL) push(-1, -1);
        if (b & FB_TR) push(1, -1);
        if (b & FB_BL) push(-1, 1);
        if (b & FB_BR) push(1, 1);
    }
#undef D
#undef CC
}

// a thread walks 16 rows of one column: one set of LDS atomics per run of equal distances
__global__ __launch_bounds__(256) void flood_bbox_kernel(const uint8_t* __restrict__ dist, uint32_t w, uint32_t h, uint32_t* __restrict__ table)
{
    __shared__ uint32_t s[1024];
    for (uint32_t i = threadIdx.x; i < 1024u; i += 256u) s[i] = 0u;
    __syncthreads();
    const uint32_t x = blockIdx.x * 256u + threadIdx.x;
    if (x < w) {
        for (uint32_t ya = blockIdx.y * 16u; ya < h; ya += gridDim.y * 16u) {
            const uint32_t yb = umin(ya + 16u, h);
            uint32_t prev = 256u;
            for (uint32_t y = ya; y < yb; ++y) {
                const uint32_t v = dist[(size_t)y * w + x];
                if (v != prev) {
                    if (prev < 256u) atomicMax(&s[prev * 4u + 3u], y - 1u);
                    atomicMax(&s[v * 4u + 0u], ~x);
                    atomicMax(&s[v * 4u + 1u], ~y);
                    atomicMax(&s[v * 4u + 2u], x);
                    prev = v;
                }
            }
            atomicMax(&s[prev * 4u + 3u], yb - 1u);
        }
    }
    __syncthreads();
    const uint32_t k = threadIdx.x;
    if (s[k * 4u] != 0u) {
        atomicMax(&table[k * 4u + 0u], s[k * 4u + 0u]);
        atomicMax(&table[k * 4u + 1u], s[k * 4u + 1u]);
        atomicMax(&table[k * 4u + 2u], s[k * 4u + 2u]);
        atomicMax(&table[k * 4u + 3u], s[k * 4u + 3u]);
    }
}

// band: the distance that gets 128 (threshold.saturating_add(1)), or a value no byte has
PFX_DEV uint32_t wand_px(uint32_t dv, uint32_t base, uint32_t threshold, uint32_t band, int combine)
{
    const uint32_t raw = dv <= threshold ? 255u : (dv == band ? 128u : 0u);
    switch (combine) {
        case 1: return umax(base, raw);
        case 2: return base > raw ? base - raw : 0u;
        case 3: return base * raw / 255u;
        default: return raw;
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void wand_mask_kernel(const uint8_t* dist, const uint8_t* base, uint8_t* out, size_t n, uint32_t threshold, uint32_t band, int combine)
{
    stream_walk<VEC, size_t>(n, [&](size_t g) {
        const uint32_t dv = reinterpret_cast<const uint32_t*>(dist)[g], bv = base ? reinterpret_cast<const uint32_t*>(base)[g] : 0u;
        uint32_t o = 0u;
#pragma unroll
        for (int k = 0; k < 4; ++k) o |= wand_px((dv >> (8 * k)) & 0xffu, (bv >> (8 * k)) & 0xffu, threshold, band, combine) << (8 * k);
        reinterpret_cast<uint32_t*>(out)[g] = o;
    }, [&](size_t i) { out[i] = (uint8_t)wand_px(dist[i], base ? base[i] : 0u, threshold, band, combine); });
}

// the preview pixel: fill.rgb with alpha (fill.a * coverage + 127) / 255 at coverage 255 (:580)
PFX_DEV uint32_t preview_px(uint32_t fill) { return (fill & 0x00ffffffu) | ((((fill >> 24) * 255u + 127u) / 255u) << 24); }

template <bool VEC>
__global__ __launch_bounds__(256) void fill_preview_kernel(const uint8_t* __restrict__ dist, const uint8_t* __restrict__ sel, uint32_t* __restrict__ out, size_t n,
                                                           uint32_t threshold, uint32_t fill)
{
    const uint32_t px = preview_px(fill);
    stream_walk<VEC, size_t>(n, [&](size_t g) {
        const uint32_t dv = reinterpret_cast<const uint32_t*>(dist)[g], sv = sel ? reinterpret_cast<const uint32_t*>(sel)[g] : 0xffffffffu;
        uint4 o;
        o.x = ((dv & 0xffu) <= threshold && (sv & 0xffu) != 0u) ? px : 0u;
        o.y = (((dv >> 8) & 0xffu) <= threshold && ((sv >> 8) & 0xffu) != 0u) ? px : 0u;
        o.z = (((dv >> 16) & 0xffu) <= threshold && ((sv >> 16) & 0xffu) != 0u) ? px : 0u;
        o.w = ((dv >> 24) <= threshold && (sv >> 24) != 0u) ? px : 0u;
        reinterpret_cast<uint4*>(out)[g] = o;
    }, [&](size_t i) { out[i] = (dist[i] <= threshold && (!sel || sel[i] != 0u)) ? px : 0u; });
}

__global__ __launch_bounds__(256) void fill_commit_kernel(uint32_t* __restrict__ layer, const uint8_t* __restrict__ dist, const uint8_t* __restrict__ sel, size_t n,
                                                          uint32_t threshold, uint32_t fill, uint32_t mode)
{
    const uint32_t px = preview_px(fill);
    if ((px >> 24) == 0u) return;   // the commit skips preview pixels with alpha 0 (:1438)
    for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (size_t)gridDim.x * 256u) {
        if (dist[i] > threshold || (sel && sel[i] == 0u)) continue;
        const uint32_t lp = layer[i];
        float acc[1][4] = {{ubyte0(lp), ubyte1(lp), ubyte2(lp), ubyte3(lp)}};
        const uint32_t top[1] = {px};
        blend4_dispatch<true, 1>(mode, acc, top, 1.0f, 1.0f);
        layer[i] = pack_rgba(acc[0][0], acc[0][1], acc[0][2], acc[0][3]);
    }
}

} // namespace

extern "C" hipError_t pfxk_color_distance(hipStream_t s, const uint8_t* d_src, uint8_t* d_out, size_t n, int mode, const pfxk_flood_target* G, const float* d_table)
{
    if (n == 0) return hipSuccess;
    if ((mode != 0 && mode != 1) || (mode == 1 && !d_table)) return hipErrorInvalidValue;
    const bool vec = aligned_to(d_src, 16) && aligned_to(d_out, 4);
    const uint32_t* src = (const uint32_t*)d_src;
    if (mode == 0) return launch_stream(vec, n, s, color_distance_kernel<0, true>, color_distance_kernel<0, false>, src, d_out, n, *G, d_table);
    return launch_stream(vec, n, s, color_distance_kernel<1, true>, color_distance_kernel<1, false>, src, d_out, n, *G, d_table);
}

extern "C" hipError_t pfxk_flood_seed(hipStream_t s, uint32_t w, uint32_t seed_x, uint32_t seed_y, uint32_t* d_list)
{
    flood_seed_kernel<<<1, 64, 0, s>>>(w, seed_x, seed_y, d_list);
    return hipGetLastError();
}

extern "C" hipError_t pfxk_flood_pass(hipStream_t s, int conn, const uint8_t* d_c, uint8_t* d_d, uint32_t w, uint32_t h, const uint32_t* d_list, uint32_t n,
                                      uint32_t* d_next, uint32_t* d_state, uint32_t* d_mark, uint32_t stamp, uint32_t seed_x, uint32_t seed_y)
{
    if (conn != 4 && conn != 8) return hipErrorInvalidValue;
    if (n == 0 || w == 0 || h == 0) return hipSuccess;
    const uint32_t tiles_x = (w + T - 1) / T, tiles_y = (h + T - 1) / T;
    if ((uint64_t)n > (uint64_t)tiles_x * tiles_y) return hipErrorInvalidValue;
    if (conn == 4) flood_pass_kernel<4><<<n, 64, 0, s>>>(d_c, d_d, w, h, d_list, d_next, d_state, d_mark, stamp, tiles_x, tiles_y, seed_x, seed_y);
    else flood_pass_kernel<8><<<n, 64, 0, s>>>(d_c, d_d, w, h, d_list, d_next, d_state, d_mark, stamp, tiles_x, tiles_y, seed_x, seed_y);
    return hipGetLastError();
}

extern "C" hipError_t pfxk_flood_bboxes(hipStream_t s, const uint8_t* d_dist, uint32_t w, uint32_t h, uint32_t* d_table)
{
    if (w == 0 || h == 0) return hipSuccess;
    const uint32_t bands = (h + 15u) / 16u;
    flood_bbox_kernel<<<dim3((w + 255u) / 256u, bands > 4096u ? 4096u : bands), 256, 0, s>>>(d_dist, w, h, d_table);
    return hipGetLastError();
}

extern "C" hipError_t pfxk_wand_mask(hipStream_t s, const uint8_t* d_dist, const uint8_t* d_base, uint8_t* d_out, size_t n, uint32_t threshold, int aa, int combine)
{
    if (n == 0) return hipSuccess;
    if (combine < 0 || combine > 3 || threshold > 255u) return hipErrorInvalidValue;
    const uint32_t band = aa ? (threshold < 255u ? threshold + 1u : 255u) : 0xffffffffu;
    return launch_stream(aligned_to(d_dist, 4) && aligned_to(d_out, 4) && aligned_to(d_base, 4), n, s, wand_mask_kernel<true>, wand_mask_kernel<false>,
                         d_dist, d_base, d_out, n, threshold, band, combine);
}

extern "C" hipError_t pfxk_fill_preview(hipStream_t s, const uint8_t* d_dist, const uint8_t* d_sel, uint8_t* d_out, size_t n, uint32_t threshold, uint32_t fill_rgba)
{
    if (n == 0) return hipSuccess;
    return launch_stream(aligned_to(d_dist, 4) && aligned_to(d_sel, 4) && aligned_to(d_out, 16), n, s, fill_preview_kernel<true>, fill_preview_kernel<false>,
                         d_dist, d_sel, (uint32_t*)d_out, n, threshold, fill_rgba);
}

extern "C" hipError_t pfxk_fill_commit(hipStream_t s, uint8_t* d_layer, const uint8_t* d_dist, const uint8_t* d_sel, size_t n, uint32_t threshold, uint32_t fill_rgba,
                                       uint32_t mode)
{
    if (n == 0) return hipSuccess;
    fill_commit_kernel<<<stream_blocks(n), 256, 0, s>>>((uint32_t*)d_layer, d_dist, d_sel, n, threshold, fill_rgba, mode);
    return hipGetLastError();
}
