// k_customshape.hip — the shape tool with a custom path selected (PlacedShape::custom_shape_data), and the shape picker's icon of such a path.
//
// Reference: the custom branch of rasterize_shape (src/ops/shapes.rs:1241-1248, :1380-1383): custom_shape_coverage :1065 (four sub-samples per pixel),
// custom_shape_coverage_sample :1088, point_in_polylines :1122 (crossing parity over every segment), distance_to_polylines :1140 with distance_to_segment
// :1152 (Outline and Both only); render_custom_shape_icon :122-155 (16 samples per pixel, Filled).  `+ - * /`, sqrt and comparisons only: bit-exact class.
//
// One pixel per lane in k_shapes.hip's 64 x 4 tiles and the same three forms (box buffer, whole-canvas preview, rasterise + commit in place); the pixel
// position, the inverse rotation, the coverage gate, the alpha quantisation and the commit are k_shape_pixel.h's.  Every f32 expression is in the
// reference's association order with no contraction, `/` and sqrtf IEEE-correct.  What is uniform over the image — sx, sy, max(sx, sy), max(outline_width, 1)
// — is computed on the host with the reference's expressions (pfx_customshape.cpp).  A pixel's four samples are (px_i, py_j), i, j in {0, 1}: the sample
// offsets are +-0.25 on each axis, so two px and two py values make the four; the crossing test and the intercept depend on py_j alone and are evaluated
// once per j — common subexpressions, not a reordering.
//
// Where the segments live: a workgroup walks the segment array (x1 y1 x2 y2, pfx_custom_shape_segments' order) in batches of PFXK_CUSTOM_BATCH, one segment
// per lane, and appends the segments its tile needs to two lists in LDS (one for the parity, one for the distance; a wave reserves its slots with one LDS
// atomic).  After every fourth batch, and after the last, the workgroup reads the lists back by broadcast (every lane the same address: one LDS cycle per
// group, no conflict) and applies each entry to its samples.  A list holds PFXK_CUSTOM_LIST = 4 batches, so it cannot overflow whatever the culling keeps.
// The order in which segments reach a list is not the path's; parity is an XOR and the distance a minimum, so the order does not show.
//
// Reorderings against the reference:
//  1. Minimum on squared distances: one sqrt and one division per sample at the end.  sqrtf and division by a positive number are correctly rounded, hence
//     monotone non-decreasing, so sqrt(min d2) / s == min(sqrt(d2) / s) bit for bit and `<=` sees the same value; a NaN distance is skipped by both forms
//     (f32::min / v_min_f32 return the other operand); the reference's f32::MAX start is the final min(F32_MAX, .).
//  2. No early exit is taken (a sample that is inside in Both mode still gets its distance): the lists are short once culled.
//  3. Culling, all of it on the f32 values the predicates themselves compare.  py_min, py_max, px_min, px_max are the minimum and maximum of the ACTUAL px / py
//     values of the workgroup's samples, by a reduction over the lanes (a lane outside the box takes the samples of the nearest box pixel, which lies in the
//     same tile, so it adds nothing).
//     Parity: a segment with |y2 - y1| <= 1e-6f fails the predicate's first clause.  With max(y1, y2) <= py_min every sample has y1 > py and y2 > py both
//     false; with min(y1, y2) > py_max both true: the second clause `(y1 > py) != (y2 > py)` fails for every sample.  Exact, no margin.  There is no culling
//     by x: the rounded intercept can leave [min x, max x] by an ulp.
//     Distance: a segment is dropped when its bounding box is farther than `reach` from the samples' bounding box along x or along y, where
//         reach = R * (1 + 2^-10) + 2^-16 * M,   R = max(outline_width, 1) * max(sx, sy),   M = the largest |coordinate| among the segments and the samples.
//     Why that is safe (u = 2^-24): the computed gap fl(a - b) is at most (1 + u) times the true one, so the true gap g along that axis exceeds
//     reach / (1 + u).  The reference's closest point is (ax + dx t, ay + dy t) with t in [0, 1] (or the start point); as computed, each coordinate is
//     within 6 u M of the segment's bounding box (dx, dx t and the sum round once each, |dx| <= 2 M).  So the computed |p - c| along that axis is at least
//     (g - 6 u M)(1 - u), the computed distance at least (g - 6 u M)(1 - 4 u) (two squares, a sum, a sqrt; the other axis only adds), and after the division
//     by max(sx, sy) at least (g - 6 u M)(1 - 5 u) / max(sx, sy) > max(outline_width, 1) (1 + 2^-11): 2^-16 M pays for 6 u M 170 times over and 2^-10 for
//     5 u and the rounding of R itself.  Such a segment fails `dist / max(sx, sy) <= max(outline_width, 1)` for every sample of the tile and a minimum over
//     the rest gives the same outline bit.  With M above 2^40 (squares near overflow) or any NaN in the bounds nothing is dropped.
#include "k_shape_pixel.h"
#include "pfx_kernels.h"

using namespace pfxk;

namespace {

constexpr float F32_MAX = 3.40282347e+38f;
constexpr int BATCH = PFXK_CUSTOM_BATCH, LIST = PFXK_CUSTOM_LIST, FLUSH_EVERY = LIST / BATCH;
static_assert(BATCH == 256 && FLUSH_EVERY * BATCH == LIST, "one segment per lane and whole batches per list");

struct alignas(16) seg4 { float x1, y1, x2, y2; };

template <bool DIST>
struct path_lds {
    seg4 par[LIST];
    seg4 dist[DIST ? LIST : 1];
    uint32_t cnt[2][2];   // [phase][parity, distance]: the lists' fill; the other phase's pair is zeroed while this one is read
    float red[4][4];      // per wave: px_min, px_max, py_min, py_max
};

// the lanes with `keep` append g to the list; slot order within the list is arbitrary
PFX_DEV void append(bool keep, const seg4& g, seg4* list, uint32_t* cnt)
{
    const unsigned long long m = __ballot(keep);
    if (m == 0ull) return;
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t base = 0u;
    if (lane == 0u) base = atomicAdd(cnt, (uint32_t)__popcll(m));
    base = (uint32_t)__shfl((int)base, 0, 64);
    if (keep) list[base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = g;
}

// N x N samples (px[i], py[j]) per lane, sample (i, j) at bit / slot j * N + i: `inside` gets point_in_polylines, best2 the minimum squared distance (DIST).
// Every lane of the workgroup calls it (barriers inside).
template <int N, bool DIST>
PFX_DEV void path_walk(path_lds<DIST>& L, const seg4* __restrict__ segs, const pfxk_custom_params& P, const float (&px)[N], const float (&py)[N],
                       uint32_t& inside, float (&best2)[N * N])
{
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    float xlo = px[0], xhi = px[0], ylo = py[0], yhi = py[0];
    for (int i = 1; i < N; ++i) {
        xlo = __builtin_fminf(xlo, px[i]); xhi = __builtin_fmaxf(xhi, px[i]);
        ylo = __builtin_fminf(ylo, py[i]); yhi = __builtin_fmaxf(yhi, py[i]);
    }
    for (int off = 32; off >= 1; off >>= 1) {
        xlo = __builtin_fminf(xlo, __shfl_xor(xlo, off, 64)); xhi = __builtin_fmaxf(xhi, __shfl_xor(xhi, off, 64));
        ylo = __builtin_fminf(ylo, __shfl_xor(ylo, off, 64)); yhi = __builtin_fmaxf(yhi, __shfl_xor(yhi, off, 64));
    }
    if (lane == 0u) { L.red[wave][0] = xlo; L.red[wave][1] = xhi; L.red[wave][2] = ylo; L.red[wave][3] = yhi; }
    if (tid == 0u) { L.cnt[0][0] = 0u; L.cnt[0][1] = 0u; }
    __syncthreads();
    xlo = __builtin_fminf(__builtin_fminf(L.red[0][0], L.red[1][0]), __builtin_fminf(L.red[2][0], L.red[3][0]));
    xhi = __builtin_fmaxf(__builtin_fmaxf(L.red[0][1], L.red[1][1]), __builtin_fmaxf(L.red[2][1], L.red[3][1]));
    ylo = __builtin_fminf(__builtin_fminf(L.red[0][2], L.red[1][2]), __builtin_fminf(L.red[2][2], L.red[3][2]));
    yhi = __builtin_fmaxf(__builtin_fmaxf(L.red[0][3], L.red[1][3]), __builtin_fmaxf(L.red[2][3], L.red[3][3]));
    float reach = __builtin_inff();   // header, 3: nothing is dropped unless every bound is a number and M is at most 2^40
    {
        const float m = __builtin_fmaxf(__builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf(xlo), __builtin_fabsf(xhi)),
                                                        __builtin_fmaxf(__builtin_fabsf(ylo), __builtin_fabsf(yhi))), P.seg_abs);
        const bool numbers = xlo == xlo && xhi == xhi && ylo == ylo && yhi == yhi;
        if (numbers && m <= 1099511627776.0f) reach = P.reach + m * 1.52587890625e-05f;
    }
    const bool cull = P.cull != 0;

    inside = 0u;
    for (int b = 0; b < N * N; ++b) best2[b] = __builtin_inff();
    const uint32_t n = P.n_segments;
    uint32_t phase = 0u, it = 0u;
    for (uint32_t base = 0u; base < n; base += BATCH, ++it) {
        const uint32_t s = base + tid;
        seg4 g = {0.0f, 0.0f, 0.0f, 0.0f};
        bool keep_p = false, keep_d = false;
        if (s < n) {
            g = segs[s];
            keep_p = keep_d = true;
            if (cull) {
                keep_p = __builtin_fabsf(g.y2 - g.y1) > 1e-6f && !(__builtin_fmaxf(g.y1, g.y2) <= ylo) && !(__builtin_fminf(g.y1, g.y2) > yhi);
                const float gx = __builtin_fmaxf(__builtin_fminf(g.x1, g.x2) - xhi, xlo - __builtin_fmaxf(g.x1, g.x2));
                const float gy = __builtin_fmaxf(__builtin_fminf(g.y1, g.y2) - yhi, ylo - __builtin_fmaxf(g.y1, g.y2));
                keep_d = !(gx > reach || gy > reach);
            }
        }
        append(keep_p, g, L.par, &L.cnt[phase][0]);
        if constexpr (DIST) append(keep_d, g, L.dist, &L.cnt[phase][1]);
        if ((it % FLUSH_EVERY) != FLUSH_EVERY - 1u && base + BATCH < n) continue;

        __syncthreads();
        const uint32_t cp = L.cnt[phase][0], cd = DIST ? L.cnt[phase][1] : 0u;
        if (tid == 0u) { L.cnt[phase ^ 1u][0] = 0u; L.cnt[phase ^ 1u][1] = 0u; }
        for (uint32_t k = 0u; k < cp; ++k) { // point_in_polylines :1122
            const seg4 e = L.par[k];
            const float denom = e.y2 - e.y1;
            if (!(__builtin_fabsf(denom) > 1e-6f)) continue;
            const float ex = e.x2 - e.x1;
            for (int j = 0; j < N; ++j) {
                const bool crosses = (e.y1 > py[j]) != (e.y2 > py[j]);
                if (!__any(crosses)) continue;   // the quotient is only looked at where the scanline crosses the edge
                const float xi = ex * (py[j] - e.y1) / denom + e.x1;
                for (int i = 0; i < N; ++i)
                    if (crosses && px[i] < xi) inside ^= 1u << (j * N + i);
            }
        }
        if constexpr (DIST) {
            for (uint32_t k = 0u; k < cd; ++k) { // distance_to_segment :1152, squared
                const seg4 e = L.dist[k];
                const float dx = e.x2 - e.x1, dy = e.y2 - e.y1;
                const float len2 = dx * dx + dy * dy;
                if (len2 <= 1e-6f) {
                    for (int j = 0; j < N; ++j)
                        for (int i = 0; i < N; ++i) {
                            const float qx = px[i] - e.x1, qy = py[j] - e.y1;
                            best2[j * N + i] = __builtin_fminf(best2[j * N + i], qx * qx + qy * qy);
                        }
                } else {
                    for (int j = 0; j < N; ++j)
                        for (int i = 0; i < N; ++i) {
                            const float t = rs_clamp(((px[i] - e.x1) * dx + (py[j] - e.y1) * dy) / len2, 0.0f, 1.0f);
                            const float cx = e.x1 + dx * t, cy = e.y1 + dy * t;
                            const float qx = px[i] - cx, qy = py[j] - cy;
                            best2[j * N + i] = __builtin_fminf(best2[j * N + i], qx * qx + qy * qy);
                        }
                }
            }
        }
        __syncthreads();
        phase ^= 1u;
    }
}

// FORM 0: out = the box buffer (bw * bh); 1: out = the canvas (every pixel written); 2: out = the layer, committed in place over the box
template <int FORM, bool DIST>
__global__ __launch_bounds__(256) void custom_shape_kernel(const pfxk_custom_params P, const seg4* __restrict__ segs, uint32_t* __restrict__ out,
                                                           const uint8_t* __restrict__ selection, uint32_t mode, int canvas_w, int canvas_h)
{
    __shared__ path_lds<DIST> L;
    const int tx = shape_tile_x(), ty = shape_tile_y();
    int col = tx, row = ty;
    if constexpr (FORM == 1) {
        const int tx0 = blockIdx.x * SHAPE_TILE_W, ty0 = blockIdx.y * SHAPE_TILE_H;
        if (!(P.bw > 0 && P.bh > 0 && tx0 < P.x0 + P.bw && tx0 + SHAPE_TILE_W > P.x0 && ty0 < P.y0 + P.bh && ty0 + SHAPE_TILE_H > P.y0)) { // the whole tile misses the box
            if (tx < canvas_w && ty < canvas_h) out[(size_t)ty * canvas_w + tx] = 0u;
            return;
        }
        col = tx - P.x0;
        row = ty - P.y0;
    }
    const bool in_box = col >= 0 && col < P.bw && row >= 0 && row < P.bh;
    float lx, ly;
    shape_local(min(max(col, 0), P.bw - 1), min(max(row, 0), P.bh - 1), P, lx, ly);
    // custom_shape_coverage :1065 — samples (-.25, -.25) (.25, -.25) (-.25, .25) (.25, .25); custom_shape_coverage_sample :1102-1103
    const float px[2] = {((lx + -0.25f) + P.hx) * P.sx + P.min_x, ((lx + 0.25f) + P.hx) * P.sx + P.min_x};
    const float py[2] = {((ly + -0.25f) + P.hy) * P.sy + P.min_y, ((ly + 0.25f) + P.hy) * P.sy + P.min_y};
    uint32_t inside;
    float best2[4];
    path_walk<2, DIST>(L, segs, P, px, py, inside, best2);
    float total = 0.0f;
    for (int b = 0; b < 4; ++b) {
        const bool fill = ((inside >> b) & 1u) != 0u;
        bool value = fill;
        if constexpr (DIST) {
            const float edge_dist = __builtin_fminf(F32_MAX, __builtin_sqrtf(best2[b])) / P.max_scale;
            const bool outline = edge_dist <= P.outline_width;
            value = P.fill_mode == 0 ? outline : (fill || outline);
        }
        total += value ? 1.0f : 0.0f;
    }
    const uint32_t pixel = shape_quantise(P.primary, total * 0.25f);
    if constexpr (FORM == 0) {
        if (in_box) out[(size_t)ty * P.bw + tx] = pixel;
    } else if constexpr (FORM == 1) {
        if (tx < canvas_w && ty < canvas_h) out[(size_t)ty * canvas_w + tx] = (in_box && (pixel >> 24) != 0u) ? pixel : 0u;
    } else {
        if (in_box) shape_commit(out, (size_t)(P.y0 + ty) * canvas_w + (P.x0 + tx), pixel, selection, mode);
    }
}

// render_custom_shape_icon :122-155: size x size pixels, 4 x 4 samples each, hx = hy = 0.82 (P.hx, P.hy), Filled
__global__ __launch_bounds__(256) void custom_icon_kernel(const pfxk_custom_params P, const seg4* __restrict__ segs, uint32_t* __restrict__ out, int size, uint32_t fg)
{
    __shared__ path_lds<false> L;
    const int tx = shape_tile_x(), ty = shape_tile_y();
    const float x = (float)min(tx, size - 1), y = (float)min(ty, size - 1), fsize = (float)size;
    float px[4], py[4];
    for (int s = 0; s < 4; ++s) {
        const float off = ((float)s + 0.5f) * 0.25f;
        const float lx = (x + off) / fsize * 2.0f - 1.0f, ly = (y + off) / fsize * 2.0f - 1.0f;
        px[s] = (lx + P.hx) * P.sx + P.min_x;
        py[s] = (ly + P.hy) * P.sy + P.min_y;
    }
    uint32_t inside;
    float best2[16];
    path_walk<4, false>(L, segs, P, px, py, inside, best2);
    if (tx >= size || ty >= size) return;
    const float cov = rs_clamp((float)__popc(inside) / 16.0f, 0.0f, 1.0f);
    uint32_t pixel = 0u;
    if (cov > 0.0f) pixel = fg | (fg << 8) | (fg << 16) | ((uint32_t)round_u8f(255.0f * cov) << 24);
    out[(size_t)ty * size + tx] = pixel;
}

template <bool DIST>
void launch(hipStream_t s, int form, const pfxk_custom_params& P, const seg4* segs, uint32_t* out, const uint8_t* sel, uint32_t mode, uint32_t cw, uint32_t ch)
{
    const dim3 box_grid = shape_tile_grid(P.bw, P.bh), canvas_grid = shape_tile_grid(cw, ch);
    if (form == PFXK_SHAPE_BOX) custom_shape_kernel<0, DIST><<<box_grid, 256, 0, s>>>(P, segs, out, sel, mode, (int)cw, (int)ch);
    else if (form == PFXK_SHAPE_CANVAS) custom_shape_kernel<1, DIST><<<canvas_grid, 256, 0, s>>>(P, segs, out, sel, mode, (int)cw, (int)ch);
    else custom_shape_kernel<2, DIST><<<box_grid, 256, 0, s>>>(P, segs, out, sel, mode, (int)cw, (int)ch);
}

} // namespace

extern "C" hipError_t pfxk_custom_shape(hipStream_t s, int form, const pfxk_custom_params* P, const float* d_segs, uint8_t* d_out, const uint8_t* d_selection,
                                        uint32_t mode, uint32_t canvas_w, uint32_t canvas_h)
{
    if (form != PFXK_SHAPE_BOX && form != PFXK_SHAPE_CANVAS && form != PFXK_SHAPE_COMMIT) return hipErrorInvalidValue;
    if (P->fill_mode < 0 || P->fill_mode > 2 || P->bw < 0 || P->bh < 0) return hipErrorInvalidValue;
    if (canvas_w == 0 || canvas_h == 0) return hipSuccess;
    if (form != PFXK_SHAPE_CANVAS && (P->bw == 0 || P->bh == 0)) return hipSuccess;
    if (P->fill_mode == 1) launch<false>(s, form, *P, (const seg4*)d_segs, (uint32_t*)d_out, d_selection, mode, canvas_w, canvas_h);
    else launch<true>(s, form, *P, (const seg4*)d_segs, (uint32_t*)d_out, d_selection, mode, canvas_w, canvas_h);
    return hipGetLastError();
}

extern "C" hipError_t pfxk_custom_icon(hipStream_t s, const pfxk_custom_params* P, const float* d_segs, uint8_t* d_out, uint32_t size, uint32_t fg)
{
    if (size == 0u || size > 1024u) return hipErrorInvalidValue;
    custom_icon_kernel<<<shape_tile_grid(size, size), 256, 0, s>>>(*P, (const seg4*)d_segs, (uint32_t*)d_out, (int)size, fg & 0xffu);
    return hipGetLastError();
}
