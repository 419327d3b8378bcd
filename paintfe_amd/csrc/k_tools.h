// k_tools.h — what the tool kernels share: k_shapes, k_customshape, k_inpaint, k_flood, k_select, k_colorkey, k_overlay, k_textfx, k_textwarp, k_gradient, k_dabtools, k_linetool and k_colorrange include it, no other file does
// (the effect bank, the Gaussians and the compositor keep compiling from k_common.h alone).  A new tool kernel starts from here.
//
//   launch     stream_blocks / aligned_to / launch_stream for a streaming kernel, tile_grid for one workgroup per tile, dims_ok.
//   walk       stream_walk: four pixels per lane, then the n % 4 tail, else pixel by pixel — the loop of every streaming kernel; tile_xy: a tiled one's origin.
//   helpers    umin / umax, and the device flavour of atan2 / cos / sin: the f64 routine rounded once to f32 (k_colorrange.hip keeps its pow beside its one use).
//
// Deliberately NOT here, so that nobody folds them:
//   the float-to-integer casts (as_u32, cast_u32, as_index, cvt_u32_sat, as_i32, round_u32): each restates a different Rust cast over a different domain — NaN or
//       not, negative or not, saturating where — and cvt_u32_sat is a single instruction on purpose;
//   the bilinear samplers: k_textwarp.hip's header says why its sampler shares nothing with k_overlay.hip's, k_warp.hip's or k_resize.hip's; k_gradient.hip's crop
//       sampler rounds its horizontal lerps to u8 before the vertical one and takes its fraction from the unclamped coordinate;
//   the two block_scan's (k_select.hip, k_inpaint.hip): they differ in direction and operator;
//   the host side's pfx_dims_ok (pfx_internal.h): the entry points' check, which no kernel file includes.
#pragma once
#include "k_common.h"

namespace pfxk {

PFX_DEV uint32_t umin(uint32_t a, uint32_t b) { return a < b ? a : b; }
PFX_DEV uint32_t umax(uint32_t a, uint32_t b) { return a > b ? a : b; }

// glibc's f32 routines evaluated through f64 and rounded once: +-1 LSB class against the reference's f32 routines (k_shapes.hip's header, tests/shape_model.py)
PFX_DEV float libm_atan2(float y, float x) { return (float)atan2((double)y, (double)x); }
PFX_DEV float libm_cos(float x) { return (float)cos((double)x); }
PFX_DEV float libm_sin(float x) { return (float)sin((double)x); }

// ---- streaming kernels: 256 lanes per workgroup, a grid-stride loop over at most 8192 workgroups
inline uint32_t stream_blocks(size_t items)
{
    const size_t b = (items + 255u) / 256u;
    return (uint32_t)(b < 1u ? 1u : (b > 8192u ? 8192u : b));
}
inline bool aligned_to(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1u)) == 0u; }   // NULL is aligned: an optional plane that is absent

// VEC: `quad(g)` handles pixels 4 g .. 4 g + 3 for every g < n / 4, then `one(i)` the n % 4 tail; else `one(i)` handles every pixel.  Index is the kernel's own
// index type (size_t, or uint32_t where the launcher holds n below 2^32).  The callbacks are lambdas of the kernel and inline into the loop: a by-value
// parameter struct they capture by reference stays in scalar registers (profiles/tool_kernels_refactor.md has the resource table).
template <bool VEC, class Index, class Quad, class One>
PFX_DEV void stream_walk(Index n, Quad quad, One one)
{
    const Index first = (Index)blockIdx.x * 256u + threadIdx.x, stride = (Index)gridDim.x * 256u;
    Index done = 0;
    if constexpr (VEC) {
        const Index groups = n / 4u;
        for (Index g = first; g < groups; g += stride) quad(g);
        done = groups * 4u;
    }
    for (Index i = done + first; i < n; i += stride) one(i);
}

// the two arms of a stream_walk kernel over n pixels: `vec` is the launcher's own alignment test
template <class... Params, class... Args>
inline hipError_t launch_stream(bool vec, size_t n, hipStream_t s, void (*quads)(Params...), void (*pixels)(Params...), Args... args)
{
    if (vec) quads<<<stream_blocks((n + 3u) / 4u), 256, 0, s>>>(args...);
    else pixels<<<stream_blocks(n), 256, 0, s>>>(args...);
    return hipGetLastError();
}

// ---- tiled kernels: workgroup blockIdx.x owns tile (blockIdx.x % tiles_x, blockIdx.x / tiles_x) of BX x BY pixels
// the number of workgroups; 0 = nothing to launch, or more than 2^31 - 1 of them (not within dims_ok)
template <uint32_t BX, uint32_t BY>
inline uint32_t tile_grid(uint32_t w, uint32_t h, uint32_t* tiles_x)
{
    *tiles_x = (w + BX - 1u) / BX;
    const uint64_t tiles = (uint64_t)*tiles_x * ((h + BY - 1u) / BY);
    return tiles > 0x7fffffffull ? 0u : (uint32_t)tiles;
}
// the tile's origin plus (dx, dy), the lane's place in the tile
struct tile_at { uint32_t x, y; };
template <uint32_t BX, uint32_t BY>
PFX_DEV tile_at tile_xy(uint32_t tiles_x, uint32_t dx = 0u, uint32_t dy = 0u) { return {(blockIdx.x % tiles_x) * BX + dx, (blockIdx.x / tiles_x) * BY + dy}; }

// The ABI's bound (include/pfx.h: 256 000 000 pixels), restated for launchers that are handed bare sizes.  It decides nothing: every entry point refuses such
// sizes in pfx_check_dims before a launcher is reached (tests/test_gpu_arg_contract.py), so the bound a launcher uses — k_select.hip had 2^28 — cannot show.
inline bool dims_ok(uint32_t w, uint32_t h) { return w != 0 && h != 0 && (uint64_t)w * h <= 256000000ull; }

} // namespace pfxk
