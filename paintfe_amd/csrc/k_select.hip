// k_select.hip — selection masks, the CanvasState / tools flavour (ref: src/canvas/selection.rs:66-116, src/canvas/canvas_state.rs:1632-1887,
// src/ui/panels/tools/behavior/raster/perspective_gradient.rs:2-86, src/ops/adjustments.rs:1448-1591), bit for bit.  Masks are w*h bytes.
//
//   shapes      rectangle / ellipse membership inside the reference's bounding box (computed on the host), fused with the combine rule: one streaming kernel
//               that writes every byte of the output, four bytes per lane when base and output are dword aligned.
//   lasso       one workgroup per row: lanes stride over the edges, crossings go to an LDS list through an LDS counter, a bitonic sort of the next power of
//               two (padded with +inf) orders it — the same sequence whatever the append order — and the row is written once, fused with the combine rule:
//               a pixel finds the last pair whose start is <= x by bisection (starts and ends are both ascending, so that pair's end decides).
//   grow/shrink exact without the disc: pass 1 writes per pixel the distance to the nearest predicate pixel of its row, saturated at r + 1 (u16); pass 2 walks
//               the rows dy in [-r, r] of its column and asks g(x, y + dy) <= span[|dy|], span[k] = floor(sqrt(r^2 - k^2)) (DESIGN.md "Selection masks").
//   feather     per pass a horizontal and a vertical shrinking-window box, `sum / count` truncating, through u8: H takes prefix sums in an LDS ring while it
//               walks its row segment in steps, V slides a running sum down a band of rows.  Neither does work per pixel that grows with the radius: the
//               host scales the segment and the band with r.
//   streaming   translate, bounds (block reduction + four atomics), fill / delete of an RGBA8 layer through a grey mask.
#include "k_tools.h"
#include "pfx_kernels.h"

using namespace pfxk;

namespace {

constexpr uint32_t STEP = PFXK_SELECT_SEG;   // threads of a row-walking workgroup = pixels per step
constexpr uint32_t RING = 2048;              // feather H: prefix sums kept; >= 2 * PFXK_SELECT_FEATHER_MAX + 1 + 2 * STEP - 1

// the one combine rule (apply_selection_shape :1743-1801 and the lasso merge :41-86 agree on it for every byte of base; tests/test_select_model_host.py)
PFX_DEV uint32_t combine_px(uint32_t base, bool raw, int mode)
{
    if (raw) return mode == 2 ? 0u : (mode == 3 ? base : 255u);
    return (mode == 0 || mode == 3) ? 0u : base;
}

PFX_DEV bool shape_px(const pfxk_select_shape& S, uint32_t x, uint32_t y)
{
    if (x < S.x0 || x > S.x1 || y < S.y0 || y > S.y1) return false;
    if (S.kind == 0) return true;
    const float dx = ((float)x - S.cx) / S.rx, dy = ((float)y - S.cy) / S.ry;   // selection.rs:86-88, one rounding each
    return dx * dx + dy * dy <= 1.0f;
}

// VEC: base (when given) and out are 4-byte aligned — a lane owns four consecutive bytes, which may run over a row end; the n % 4 tail goes byte by byte
template <bool VEC>
__global__ __launch_bounds__(256) void shape_combine_kernel(const uint8_t* base, uint8_t* out, uint32_t w, uint32_t n, pfxk_select_shape S, int mode)
{
    stream_walk<VEC, uint32_t>(n, [&](uint32_t g) {
        const uint32_t bv = base ? reinterpret_cast<const uint32_t*>(base)[g] : 0u;
        uint32_t y = (g * 4u) / w, x = g * 4u - y * w, o = 0u;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            o |= combine_px((bv >> (8 * k)) & 0xffu, shape_px(S, x, y), mode) << (8 * k);
            if (++x == w) { x = 0; ++y; }
        }
        reinterpret_cast<uint32_t*>(out)[g] = o;
    }, [&](uint32_t i) {
        const uint32_t y = i / w, x = i - y * w;
        out[i] = (uint8_t)combine_px(base ? base[i] : 0u, shape_px(S, x, y), mode);
    });
}

// Rust's `v as u32` for a finite v >= 0 (the host refuses coordinates beyond 1e9, so nothing here is near 2^32; the clamp keeps the cast defined anyway)
PFX_DEV uint32_t cast_u32(float v) { return (uint32_t)__builtin_fminf(__builtin_fmaxf(v, 0.0f), 4294967040.0f); }

__global__ __launch_bounds__(256) void lasso_kernel(const float2* __restrict__ pts, uint32_t n, const uint8_t* base, uint8_t* out, uint32_t w, uint32_t h, int mode)
{
    __shared__ float nodes[PFXK_SELECT_LASSO_MAX];
    __shared__ uint32_t count;
    const uint32_t tid = threadIdx.x;
    for (uint32_t y = blockIdx.x; y < h; y += gridDim.x) {
        if (tid == 0) count = 0u;
        __syncthreads();
        const float yf = (float)y + 0.5f;
        for (uint32_t i = tid; i < n; i += 256u) {
            const float2 a = pts[i], b = pts[i + 1u == n ? 0u : i + 1u];
            if ((a.y < yf && b.y >= yf) || (b.y < yf && a.y >= yf)) {
                const float t = (yf - a.y) / (b.y - a.y);
                const float node = a.x + t * (b.x - a.x);
                const uint32_t at = atomicAdd(&count, 1u);
                if (at < PFXK_SELECT_LASSO_MAX) nodes[at] = node;   // always: an edge crosses a row at most once and n <= PFXK_SELECT_LASSO_MAX
            }
        }
        __syncthreads();
        const uint32_t m = umin(count, (uint32_t)PFXK_SELECT_LASSO_MAX);
        uint32_t p2 = 1u;
        while (p2 < m) p2 <<= 1;
        for (uint32_t i = m + tid; i < p2; i += 256u) nodes[i] = __builtin_inff();
        __syncthreads();
        for (uint32_t k = 2u; k <= p2; k <<= 1) {
            for (uint32_t j = k >> 1; j > 0u; j >>= 1) {
                for (uint32_t i = tid; i < p2; i += 256u) {
                    const uint32_t l = i ^ j;
                    if (l > i) {
                        const float a = nodes[i], b = nodes[l];
                        if (((i & k) == 0u) ? (a > b) : (a < b)) { nodes[i] = b; nodes[l] = a; }
                    }
                }
                __syncthreads();
            }
        }
        // pair q = nodes (2q, 2q + 1) selects [start_q, end_q); both ascend with q, so x is selected iff end_K > x for the last K with start_K <= x
        const uint32_t pairs = m / 2u;
        const size_t row = (size_t)y * w;
        for (uint32_t x = tid; x < w; x += 256u) {
            uint32_t lo = 0u, hi = pairs;   // the number of pairs with start <= x ends up in lo
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                if (umin(cast_u32(nodes[2u * mid]), w) <= x) lo = mid + 1u; else hi = mid;
            }
            const bool raw = lo > 0u && umin(cast_u32(nodes[2u * lo - 1u] + 1.0f), w) > x;
            out[row + x] = (uint8_t)combine_px(base ? base[row + x] : 0u, raw, mode);
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void translate_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ out, uint32_t w, uint32_t h, uint32_t n, int32_t dx,
                                                        int32_t dy)
{
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        const uint32_t y = i / w, x = i - y * w;
        const int64_t sx = (int64_t)x - dx, sy = (int64_t)y - dy;
        out[i] = (sx >= 0 && sx < (int64_t)w && sy >= 0 && sy < (int64_t)h) ? src[(size_t)sy * w + (size_t)sx] : (uint8_t)0;
    }
}

// box[0 .. 4) = ~min x, ~min y, max x, max y of {mask != 0}, zeroed first (~min x == 0 means none), as k_flood.hip's boxes
__global__ __launch_bounds__(256) void bounds_kernel(const uint8_t* __restrict__ mask, uint32_t w, uint32_t h, uint32_t* __restrict__ box)
{
    __shared__ uint32_t s[4];
    if (threadIdx.x < 4u) s[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t x = blockIdx.x * 256u + threadIdx.x;
    if (x < w) {
        uint32_t ylo = 0xffffffffu, yhi = 0u;
        bool any = false;
        for (uint32_t ya = blockIdx.y * 16u; ya < h; ya += gridDim.y * 16u) {
            const uint32_t yb = umin(ya + 16u, h);
            for (uint32_t y = ya; y < yb; ++y)
                if (mask[(size_t)y * w + x] != 0u) { ylo = umin(ylo, y); yhi = umax(yhi, y); any = true; }
        }
        if (any) {
            atomicMax(&s[0], ~x);
            atomicMax(&s[1], ~ylo);
            atomicMax(&s[2], x);
            atomicMax(&s[3], yhi);
        }
    }
    __syncthreads();
    if (threadIdx.x < 4u && s[0] != 0u) atomicMax(&box[threadIdx.x], s[threadIdx.x]);
}

// fill_selected_pixels :1861-1882 / delete_selected_pixels :1823-1836: f32, unfused, round half away from zero
template <bool FILL>
__global__ __launch_bounds__(256) void fill_delete_kernel(uint32_t* __restrict__ layer, const uint8_t* __restrict__ mask, uint32_t n, uint32_t color)
{
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        const uint32_t sel = mask[i];
        if (sel == 0u) continue;
        if (sel == 255u) { layer[i] = FILL ? color : 0u; continue; }
        const uint32_t p = layer[i];
        const float t = div255((float)sel), u = 1.0f - t;
        if constexpr (FILL) {
            layer[i] = pack_rgba(round_u8f(ubyte0(p) * u + ubyte0(color) * t), round_u8f(ubyte1(p) * u + ubyte1(color) * t),
                                 round_u8f(ubyte2(p) * u + ubyte2(color) * t), round_u8f(ubyte3(p) * u + ubyte3(color) * t));
        } else {
            layer[i] = (p & 0x00ffffffu) | ((uint32_t)round_u8f(ubyte3(p) * u) << 24);
        }
    }
}

// ---- scans over the 256 lanes of a row-walking workgroup: wave shuffles, then the four wave totals through LDS.  Every lane of the workgroup calls them.
struct op_add { PFX_DEV uint32_t operator()(uint32_t a, uint32_t b) const { return a + b; } };
struct op_max { PFX_DEV int32_t operator()(int32_t a, int32_t b) const { return a > b ? a : b; } };
struct op_min { PFX_DEV int32_t operator()(int32_t a, int32_t b) const { return a < b ? a : b; } };

// FWD: inclusive prefix (lane i gets op over lanes 0..i); else inclusive suffix (lanes i..255).  *total = op over all 256.  sh: 4 words of LDS
template <bool FWD, class T, class Op>
PFX_DEV T block_scan(T v, Op op, T* sh, T* total)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
    for (uint32_t d = 1u; d < 64u; d <<= 1) {
        const T t = FWD ? __shfl_up(v, d, 64) : __shfl_down(v, d, 64);
        if (FWD ? lane >= d : lane + d < 64u) v = op(v, t);
    }
    __syncthreads();   // sh is free again
    if (lane == (FWD ? 63u : 0u)) sh[wave] = v;
    __syncthreads();
    const T t0 = sh[0], t1 = sh[1], t2 = sh[2], t3 = sh[3];
    *total = op(op(t0, t1), op(t2, t3));
    if constexpr (FWD) {
        if (wave >= 1u) v = op(v, t0);
        if (wave >= 2u) v = op(v, t1);
        if (wave >= 3u) v = op(v, t2);
    } else {
        if (wave <= 2u) v = op(v, t3);
        if (wave <= 1u) v = op(v, t2);
        if (wave <= 0u) v = op(v, t1);
    }
    return v;
}

// grow / shrink pass 1.  Workgroup (segment, row): outputs [sx, ex) of the row; it walks the 256-aligned chunks from the one holding max(sx - r, 0) up to the
// segment's last, carrying the last predicate position, stores min(distance to the left, r + 1), then walks from the chunk holding min(ex - 1 + r, w - 1) down
// to the segment's first carrying the next predicate position.  Chunks are 256-aligned in x, so the lane that stored a pixel's left distance reads it back.
template <bool EXPAND>
__global__ __launch_bounds__(256) void morph_rowdist_kernel(const uint8_t* __restrict__ mask, uint16_t* __restrict__ g, uint32_t w, uint32_t h, uint32_t r, uint32_t seg)
{
    __shared__ int32_t sh[4];
    const uint32_t tid = threadIdx.x, sx = blockIdx.x * seg, ex = umin(sx + seg, w), sat = r + 1u;
    for (uint32_t y = blockIdx.y; y < h; y += gridDim.y) {
        const uint8_t* row = mask + (size_t)y * w;
        uint16_t* grow = g + (size_t)y * w;
        const uint32_t a = sx > r ? sx - r : 0u, b = umin(ex - 1u + r, w - 1u);
        int32_t carry = -1;
        for (uint32_t c = a / STEP; c * STEP < ex; ++c) {
            const uint32_t i = c * STEP + tid;
            const bool p = i >= a && i < w && (EXPAND ? row[i] > 127u : row[i] == 0u);
            int32_t total;
            int32_t last = block_scan<true>(p ? (int32_t)i : -1, op_max(), sh, &total);
            last = op_max()(last, carry);
            carry = op_max()(carry, total);
            if (i >= sx && i < ex) grow[i] = (uint16_t)(last < 0 ? sat : umin(i - (uint32_t)last, sat));
        }
        carry = 0x7fffffff;
        for (uint32_t c = b / STEP + 1u; c-- > sx / STEP;) {
            const uint32_t i = c * STEP + tid;
            const bool p = i <= b && (EXPAND ? row[i] > 127u : row[i] == 0u);
            int32_t total;
            int32_t next = block_scan<false>(p ? (int32_t)i : 0x7fffffff, op_min(), sh, &total);
            next = op_min()(next, carry);
            carry = op_min()(carry, total);
            if (i >= sx && i < ex && next != 0x7fffffff) grow[i] = (uint16_t)umin(grow[i], umin((uint32_t)next - i, sat));
        }
    }
}

// grow / shrink pass 2: lanes along x, so every step of the column walk is one coalesced row read of g
template <bool EXPAND>
__global__ __launch_bounds__(256) void morph_decide_kernel(const uint8_t* mask, const uint16_t* __restrict__ g, const uint16_t* __restrict__ span, uint8_t* out,
                                                           uint32_t w, uint32_t h, uint32_t r)
{
    const uint32_t x = blockIdx.x * 256u + threadIdx.x;
    if (x >= w) return;
    for (uint32_t y = blockIdx.y; y < h; y += gridDim.y) {
        const size_t at = (size_t)y * w + x;
        const uint32_t v = mask[at];
        if (EXPAND ? v > 127u : v == 0u) { out[at] = (uint8_t)v; continue; }   // the rule skips it
        const uint32_t up = umin(r, y), down = umin(r, h - 1u - y);
        bool found = (uint32_t)g[at] <= r;   // dy = 0: span[0] = r
        for (uint32_t k = 1u; k <= up && !found; ++k) found = (uint32_t)g[at - (size_t)k * w] <= (uint32_t)span[k];
        for (uint32_t k = 1u; k <= down && !found; ++k) found = (uint32_t)g[at + (size_t)k * w] <= (uint32_t)span[k];
        out[at] = (uint8_t)(found ? (EXPAND ? 255u : 0u) : v);
    }
}

// feather H.  Workgroup (segment, row): outputs [sx, ex).  ring[i % RING] = sum of row[a .. i], a = max(sx - r, 0) (mod 2^32: only differences are used).
// Before a step's 256 outputs the prefix is advanced, 256 pixels at a time, past the step's last window end.  Live span: from x - r - 1 of the step's first
// pixel to 255 past its last window end, 2 r + 1 + 511 <= RING entries.
__global__ __launch_bounds__(256) void feather_h_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, uint32_t w, uint32_t h, uint32_t r, uint32_t seg)
{
    __shared__ uint32_t ring[RING];
    __shared__ uint32_t sh[4];
    const uint32_t tid = threadIdx.x, sx = blockIdx.x * seg, ex = umin(sx + seg, w);
    for (uint32_t y = blockIdx.y; y < h; y += gridDim.y) {
        const uint8_t* row = src + (size_t)y * w;
        const uint32_t a = sx > r ? sx - r : 0u;
        uint32_t carry = 0u, done = a;
        for (uint32_t X = sx; X < ex; X += STEP) {
            const uint32_t need = umin(X + STEP - 1u + r, w - 1u);
            while (done <= need) {
                const uint32_t i = done + tid;
                uint32_t total;
                const uint32_t s = block_scan<true>(i < w ? (uint32_t)row[i] : 0u, op_add(), sh, &total);
                ring[i % RING] = carry + s;
                carry += total;
                done += STEP;
            }
            __syncthreads();
            const uint32_t x = X + tid;
            if (x < ex) {
                const uint32_t x0 = x > r ? x - r : 0u, x1 = umin(x + r, w - 1u);
                const uint32_t sum = ring[x1 % RING] - (x0 > a ? ring[(x0 - 1u) % RING] : 0u);
                dst[(size_t)y * w + x] = (uint8_t)(sum / (x1 - x0 + 1u));
            }
            __syncthreads();   // the next step overwrites ring entries this one read
        }
    }
}

// feather V: a lane owns a column of a band of rows; the sum is seeded from the band's first window and slides down
__global__ __launch_bounds__(256) void feather_v_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, uint32_t w, uint32_t h, uint32_t r, uint32_t band)
{
    const uint32_t x = blockIdx.x * 256u + threadIdx.x;
    if (x >= w) return;
    const uint32_t bands = (h + band - 1u) / band;
    for (uint32_t bi = blockIdx.y; bi < bands; bi += gridDim.y) {
        const uint32_t ya = bi * band, yb = umin(ya + band, h);
        uint32_t y0 = ya > r ? ya - r : 0u, y1 = umin(ya + r, h - 1u), sum = 0u;
        for (uint32_t yy = y0; yy <= y1; ++yy) sum += src[(size_t)yy * w + x];
        for (uint32_t y = ya; y < yb; ++y) {
            dst[(size_t)y * w + x] = (uint8_t)(sum / (y1 - y0 + 1u));
            if (y1 + 1u < h) { ++y1; sum += src[(size_t)y1 * w + x]; }   // the window of y + 1 ends at min(y + 1 + r, h - 1)
            if (y + 1u > r) { sum -= src[(size_t)y0 * w + x]; ++y0; }    // and starts at max(y + 1 - r, 0)
        }
    }
}

inline uint32_t capped(uint32_t v, uint32_t cap) { return v < cap ? v : cap; }

} // namespace

extern "C" hipError_t pfxk_select_shape_combine(hipStream_t s, const uint8_t* d_base, uint8_t* d_out, uint32_t w, uint32_t h, const pfxk_select_shape* S, int mode)
{
    if (!dims_ok(w, h) || mode < 0 || mode > 3 || S->kind > 1u) return hipErrorInvalidValue;
    return launch_stream(aligned_to(d_base, 4) && aligned_to(d_out, 4), (size_t)w * h, s, shape_combine_kernel<true>, shape_combine_kernel<false>, d_base, d_out, w,
                         w * h, *S, mode);
}

extern "C" hipError_t pfxk_select_lasso(hipStream_t s, const float* d_points_xy, uint32_t n_points, const uint8_t* d_base, uint8_t* d_out, uint32_t w, uint32_t h, int mode)
{
    if (!dims_ok(w, h) || mode < 0 || mode > 3 || n_points > PFXK_SELECT_LASSO_MAX || (n_points != 0 && !d_points_xy)) return hipErrorInvalidValue;
    lasso_kernel<<<capped(h, 16384u), 256, 0, s>>>((const float2*)d_points_xy, n_points, d_base, d_out, w, h, mode);
    return hipGetLastError();
}

extern "C" hipError_t pfxk_select_translate(hipStream_t s, const uint8_t* d_src, uint8_t* d_out, uint32_t w, uint32_t h, int32_t dx, int32_t dy)
{
    if (!dims_ok(w, h)) return hipErrorInvalidValue;
    translate_kernel<<<stream_blocks((size_t)w * h), 256, 0, s>>>(d_src, d_out, w, h, w * h, dx, dy);
    return hipGetLastError();
}

extern "C" hipError_t pfxk_select_bounds(hipStream_t s, const uint8_t* d_mask, uint32_t w, uint32_t h, uint32_t* d_box)
{
    if (!dims_ok(w, h)) return hipErrorInvalidValue;
    bounds_kernel<<<dim3((w + 255u) / 256u, capped((h + 15u) / 16u, 4096u)), 256, 0, s>>>(d_mask, w, h, d_box);
    return hipGetLastError();
}

extern "C" hipError_t pfxk_select_fill(hipStream_t s, uint8_t* d_layer, const uint8_t* d_mask, uint32_t w, uint32_t h, uint32_t color_rgba, int erase)
{
    if (!dims_ok(w, h) || !aligned_to(d_layer, 4)) return hipErrorInvalidValue;
    const uint32_t n = w * h;
    if (erase) fill_delete_kernel<false><<<stream_blocks(n), 256, 0, s>>>((uint32_t*)d_layer, d_mask, n, 0u);
    else fill_delete_kernel<true><<<stream_blocks(n), 256, 0, s>>>((uint32_t*)d_layer, d_mask, n, color_rgba);
    return hipGetLastError();
}

extern "C" uint32_t pfxk_select_segment(uint32_t r) { return STEP * ((r + 63u) / 64u < 1u ? 1u : (r + 63u) / 64u); }
extern "C" uint32_t pfxk_select_band(uint32_t r) { return PFXK_SELECT_BAND * ((r + 7u) / 8u < 1u ? 1u : (r + 7u) / 8u); }

extern "C" hipError_t pfxk_select_morph(hipStream_t s, int expand, const uint8_t* d_mask, uint16_t* d_rowdist, const uint16_t* d_span, uint8_t* d_out, uint32_t w,
                                        uint32_t h, uint32_t r)
{
    if (!dims_ok(w, h) || r == 0u || r > PFXK_SELECT_MORPH_MAX) return hipErrorInvalidValue;
    const uint32_t seg = pfxk_select_segment(r);
    const dim3 g1((w + seg - 1u) / seg, capped(h, 32768u)), g2((w + 255u) / 256u, capped(h, 32768u));
    if (expand) {
        morph_rowdist_kernel<true><<<g1, 256, 0, s>>>(d_mask, d_rowdist, w, h, r, seg);
        morph_decide_kernel<true><<<g2, 256, 0, s>>>(d_mask, d_rowdist, d_span, d_out, w, h, r);
    } else {
        morph_rowdist_kernel<false><<<g1, 256, 0, s>>>(d_mask, d_rowdist, w, h, r, seg);
        morph_decide_kernel<false><<<g2, 256, 0, s>>>(d_mask, d_rowdist, d_span, d_out, w, h, r);
    }
    return hipGetLastError();
}

extern "C" hipError_t pfxk_select_feather_pass(hipStream_t s, const uint8_t* d_src, uint8_t* d_tmp, uint8_t* d_dst, uint32_t w, uint32_t h, uint32_t r)
{
    if (!dims_ok(w, h) || r == 0u || r > PFXK_SELECT_FEATHER_MAX || d_src == d_tmp || d_tmp == d_dst) return hipErrorInvalidValue;
    const uint32_t seg = pfxk_select_segment(r), band = pfxk_select_band(r);
    feather_h_kernel<<<dim3((w + seg - 1u) / seg, capped(h, 32768u)), 256, 0, s>>>(d_src, d_tmp, w, h, r, seg);
    feather_v_kernel<<<dim3((w + 255u) / 256u, capped((h + band - 1u) / band, 32768u)), 256, 0, s>>>(d_tmp, d_dst, w, h, r, band);
    return hipGetLastError();
}
