// k_shape_pixel.h — what the two rasterisers of the shape tool share: k_shapes.hip (the built-in SDF shapes) and k_customshape.hip (custom path shapes).
// Both run rasterize_shape's pixel loop (src/ops/shapes.rs:1228-1302) around a different coverage: the lane's pixel (64 x 4 tiles, a wave = 64 consecutive
// pixels of a row), the inverse rotation into the shape's frame (:1231-1239), the `coverage > 0.001` gate with the alpha quantisation (:1293-1300), and the
// commit of one pixel (blend_pixel_static(layer, pixel, mode, 1.0) where a > 0 and the selection allows).  The expressions are the ones k_shapes.hip had
// inline: the built-in shapes' results are unchanged (tests/test_gpu_shapes.py, tests/test_gpu_customshape.py).
#pragma once
#include "k_tools.h"
#include "k_blend.h"

namespace pfxk {

constexpr int SHAPE_TILE_W = 64, SHAPE_TILE_H = 4;   // 256 lanes per workgroup

PFX_DEV int shape_tile_x() { return blockIdx.x * SHAPE_TILE_W + (threadIdx.x & 63); }
PFX_DEV int shape_tile_y() { return blockIdx.y * SHAPE_TILE_H + (threadIdx.x >> 6); }
inline dim3 shape_tile_grid(uint32_t w, uint32_t h) { return dim3((w + SHAPE_TILE_W - 1) / SHAPE_TILE_W, (h + SHAPE_TILE_H - 1) / SHAPE_TILE_H); }

// the centre of box pixel (col, row) in the shape's frame; P has x0, y0, cx, cy, inv_cos, inv_sin
template <class Params>
PFX_DEV void shape_local(int col, int row, const Params& P, float& lx, float& ly)
{
    const float px_canvas = (float)(P.x0 + col) + 0.5f, py_canvas = (float)(P.y0 + row) + 0.5f;
    const float dx = px_canvas - P.cx, dy = py_canvas - P.cy;
    lx = dx * P.inv_cos - dy * P.inv_sin;
    ly = dx * P.inv_sin + dy * P.inv_cos;
}

// the reference's buffer pixel for a colour and a coverage: 0 where coverage <= 0.001
PFX_DEV uint32_t shape_quantise(uint32_t color, float coverage)
{
    if (!(coverage > 0.001f)) return 0u;
    // (a * cov).round().min(255.0) as u8: the product is in [0, 255], where round_u8f's clamp is the reference's min
    return (color & 0x00ffffffu) | ((uint32_t)round_u8f(ubyte3(color) * coverage) << 24);
}

// commit buffer pixel `px` into layer pixel i: nothing where its alpha is 0 or the selection is 0 there
PFX_DEV void shape_commit(uint32_t* __restrict__ layer, size_t i, uint32_t px, const uint8_t* __restrict__ selection, uint32_t mode)
{
    if ((px >> 24) == 0u) return;
    if (selection && selection[i] == 0) return;
    const uint32_t lp = layer[i];
    float acc[1][4] = {{ubyte0(lp), ubyte1(lp), ubyte2(lp), ubyte3(lp)}};
    const uint32_t t[1] = {px};
    blend4_dispatch<true, 1>(mode, acc, t, 1.0f, 1.0f);
    layer[i] = pack_rgba(acc[0][0], acc[0][1], acc[0][2], acc[0][3]);
}

} // namespace pfxk
