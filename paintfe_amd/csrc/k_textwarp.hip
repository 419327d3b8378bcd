// k_textwarp.hip — the text block's warps, rotation and blit (ref: src/ops/text_layer/warp.rs, raster.rs:561-653): every f32 expression as the reference writes it,
// one rounding per operation (no contraction), IEEE division and square root, round() half away from zero.  Only what is uniform over the image is hoisted,
// and only through the reference's own expressions (pfx_textwarp.cpp), so no bit can move.
//
//   shape     but for the envelope, a workgroup of four waves owns 256 columns x 16 rows: a lane takes four adjacent pixels, a wave every fourth row.  The
//             four pixels leave as one 16-byte store where the address allows it; the taps of bilinear_sample :707-740 are dword loads.  Every output
//             pixel is written, zero where the reference skips, so nothing clears the output first.
//   arc       arc_inverse_map :222-274.  sy depends on the radius alone, so it is tested before atan2; the rejections are pure, their order is free.
//   circular  :305-349.  The annulus and the sy test come before atan2: most of the square never reaches it, and a wave wholly outside only stores zeros.
//             The angle is normalised by the reference's two loops of f32 additions; the launcher bounds the start angle, which bounds the loops.
//   path      inverse_path_follow :627-695.  The 65 coarse curve points and the 257 arc lengths come from the host in the kernel's arguments and are kept
//             in LDS (every lane reads the same word: a broadcast); the coarse search is 65 distances, the eight refinement steps stay per pixel.
//   envelope  :495-536.  t, top_y and span depend on the column alone, and so does the x half of bilinear_sample: one output column per lane, the column's
//             part in registers for 32 rows, the taps of four rows in flight together (envelope_kernel).
//   atan2     the project's device flavour: the f64 atan2 rounded once to f32 (k_tools.h's libm_atan2).  It is the register-heavy part, so each warp is a
//             kernel of its own and the path and envelope kernels do not carry its registers.
// This bilinear is neither transform.rs's nor effects.rs's: nothing is shared with k_warp.hip or k_resize.hip.  Pixels are indexed within pfx_dims_ok (256 Mpx).
#include "k_tools.h"
#include "pfx_kernels.h"

using namespace pfxk;

namespace {

constexpr uint32_t TW = 256, TH = 16, PX = 4, WAVES = 4;   // tile; pixels per lane; waves per workgroup
constexpr float TAU = 6.28318530717958647692f;

// bilinear_sample :707-740 for 0 <= x < w, 0 <= y < h (the callers' tests).  x0 and y0 are then inside: w is src_w rounded to f32, and the largest f32
// below it is at most src_w - 1 whichever way that rounded; only the +1 taps can fall past the edge, where they are transparent
PFX_DEV uint32_t sample(const uint32_t* __restrict__ src, uint32_t sw, uint32_t sh, float x, float y)
{
    const float x0f = __builtin_floorf(x), y0f = __builtin_floorf(y);
    const uint32_t x0 = (uint32_t)x0f, y0 = (uint32_t)y0f;
    const float fx = x - x0f, fy = y - y0f;
    const bool in_x1 = x0 + 1u < sw, in_y1 = y0 + 1u < sh;
    const size_t at = (size_t)y0 * sw + x0;
    const uint32_t p00 = src[at], p10 = in_x1 ? src[at + 1u] : 0u;
    const uint32_t p01 = in_y1 ? src[at + sw] : 0u, p11 = in_x1 && in_y1 ? src[at + sw + 1u] : 0u;
    const float ux = 1.0f - fx, uy = 1.0f - fy;
    const float r = ubyte0(p00) * ux * uy + ubyte0(p10) * fx * uy + ubyte0(p01) * ux * fy + ubyte0(p11) * fx * fy;
    const float g = ubyte1(p00) * ux * uy + ubyte1(p10) * fx * uy + ubyte1(p01) * ux * fy + ubyte1(p11) * fx * fy;
    const float b = ubyte2(p00) * ux * uy + ubyte2(p10) * fx * uy + ubyte2(p01) * ux * fy + ubyte2(p11) * fx * fy;
    const float a = ubyte3(p00) * ux * uy + ubyte3(p10) * fx * uy + ubyte3(p01) * ux * fy + ubyte3(p11) * fx * fy;
    return pack_round_rgba_finite(r, g, b, a);   // finite, within [0, 255]
}

// four adjacent pixels of row y from column x (x < out_w): one 16-byte store where all four exist and the address is aligned
PFX_DEV void store_px(uint32_t* __restrict__ out, uint32_t out_w, uint32_t x, uint32_t y, const uint32_t px[PX])
{
    uint32_t* p = out + (size_t)y * out_w + x;
    if (x + PX <= out_w && ((uintptr_t)p & 15u) == 0u) {
        *(uint4*)p = make_uint4(px[0], px[1], px[2], px[3]);
        return;
    }
#pragma unroll
    for (uint32_t k = 0; k < PX; ++k)
        if (x + k < out_w) p[k] = px[k];
}

// the tile walk shared by the kernels: `pixel(ox, oy)` gives one output pixel
template <class F>
PFX_DEV void walk_tile(uint32_t* __restrict__ out, uint32_t out_w, uint32_t out_h, uint32_t tiles_x, F pixel)
{
    const auto [x, y0] = tile_xy<TW, TH>(tiles_x, (threadIdx.x & 63u) * PX, threadIdx.x >> 6);
    if (x >= out_w) return;
    for (uint32_t y = y0; y < out_h && y < y0 + TH; y += WAVES) {
        uint32_t px[PX];
#pragma unroll
        for (uint32_t k = 0; k < PX; ++k) px[k] = x + k < out_w ? pixel(x + k, y) : 0u;
        store_px(out, out_w, x, y, px);
    }
}

__global__ __launch_bounds__(256) void arc_kernel(const uint32_t* __restrict__ src, uint32_t* __restrict__ out, uint32_t tiles_x, const pfxk_textwarp P)
{
    walk_tile(out, P.out_w, P.out_h, tiles_x, [&](uint32_t ox, uint32_t oy) -> uint32_t {
        float dx = (float)ox + P.min_x, dy = (float)oy + P.min_y;
        if (P.undo_h) dx = P.cx + (dx - P.cx) / P.one_hdist;              // :238
        if (P.undo_v) dy = P.half_h + (dy - P.half_h) / P.one_vdist;      // :243
        const float rel_x = dx - P.cx, rel_y = P.r_abs - dy * P.r_sign;   // :250
        const float ry = rel_y * P.r_sign;
        const float r = __builtin_sqrtf(rel_x * rel_x + ry * ry);
        const float sy_norm = 1.0f - (P.r_abs - r) / P.h_r_sign;          // :270
        const float sy = sy_norm * P.h;
        if (!(sy >= 0.0f && sy < P.h)) return 0u;
        float t;
        if (P.curved) {
            const float theta = libm_atan2(rel_x, ry);                    // :254
            if (__builtin_fabsf(theta) > P.theta_lim) return 0u;          // :257
            t = theta / P.half_angle;
        } else {
            t = (dx - P.cx) / P.half_w;
        }
        const float sx = P.cx + t * P.w / 2.0f;                           // :267
        if (!(sx >= 0.0f && sx < P.w)) return 0u;
        return sample(src, P.src_w, P.src_h, sx, sy);
    });
}

__global__ __launch_bounds__(256) void circular_kernel(const uint32_t* __restrict__ src, uint32_t* __restrict__ out, uint32_t tiles_x, const pfxk_textwarp P)
{
    walk_tile(out, P.out_w, P.out_h, tiles_x, [&](uint32_t ox, uint32_t oy) -> uint32_t {
        const float px = (float)ox - P.out_c, py = (float)oy - P.out_c;
        const float dist = __builtin_sqrtf(px * px + py * py);
        if (dist < P.r || dist > P.r_outer) return 0u;                    // :314
        const float sy = P.r_outer - dist;                                // :337
        if (!(sy >= 0.0f && sy < P.h)) return 0u;
        const float pixel_angle = libm_atan2(py, px);
        float rel = (pixel_angle - P.start_angle) * P.dir;                // :321
        while (rel < 0.0f) rel += TAU;                                    // at most five steps each: |start_angle| <= 8 pi (the launcher)
        while (rel >= TAU) rel -= TAU;
        const float sx = rel * P.r;
        if (!(sx >= 0.0f && sx < P.w)) return 0u;
        return sample(src, P.src_w, P.src_h, sx, sy);
    });
}

// eval_cubic_bezier :546-559, one coordinate
PFX_DEV float bezier(float t, float p0, float p1, float p2, float p3)
{
    const float u = 1.0f - t, u2 = u * u, t2 = t * t;
    return u2 * u * p0 + 3.0f * u2 * t * p1 + 3.0f * u * t2 * p2 + t2 * t * p3;
}
// eval_cubic_bezier_tangent :562-571, one coordinate; d10 = p1 - p0, d21 = p2 - p1, d32 = p3 - p2
PFX_DEV float bezier_tangent(float t, float d10, float d21, float d32)
{
    const float u = 1.0f - t;
    return 3.0f * u * u * d10 + 6.0f * u * t * d21 + 3.0f * t * t * d32;
}

// inverse_path_follow :627-695 and the gather for one output pixel
struct path_uniforms { float x0, x1, x2, x3, y0, y1, y2, y3, half_h, w, h; uint32_t src_w, src_h; };
PFX_DEV uint32_t path_pixel(const uint32_t* __restrict__ src, const float* __restrict__ s_cx, const float* __restrict__ s_cy,
                                            const float* __restrict__ s_len, const path_uniforms& U, float px, float py)
{
    uint32_t best_i = 0u;
    float best = 3.4028234663852886e38f;
    // 65 = 5 x 13.  Unrolled in full the loop requests its 130 LDS words up front and holds them: 256 VGPRs, two waves per SIMD
#pragma unroll 13
    for (uint32_t i = 0u; i <= 64u; ++i) {                            // :640; strict <: the first minimum wins
        const float ex = px - s_cx[i], ey = py - s_cy[i];
        const float d = ex * ex + ey * ey;
        if (d < best) { best = d; best_i = i; }
    }
    const float best_t = (float)best_i / 64.0f, step = 1.0f / 64.0f;
    float t_lo = __builtin_fmaxf(best_t - step, 0.0f), t_hi = __builtin_fminf(best_t + step, 1.0f);
#pragma unroll 1
    for (int k = 0; k < 8; ++k) {                                     // :654
        const float t_mid = (t_lo + t_hi) / 2.0f;
        const float t_a = (t_lo + t_mid) / 2.0f, t_b = (t_mid + t_hi) / 2.0f;
        const float ax = px - bezier(t_a, U.x0, U.x1, U.x2, U.x3), ay = py - bezier(t_a, U.y0, U.y1, U.y2, U.y3);
        const float bx = px - bezier(t_b, U.x0, U.x1, U.x2, U.x3), by = py - bezier(t_b, U.y0, U.y1, U.y2, U.y3);
        const float da = ax * ax + ay * ay, db = bx * bx + by * by;
        if (da < db) t_hi = t_mid; else t_lo = t_mid;
    }
    const float t = (t_lo + t_hi) / 2.0f;
    const float cx = bezier(t, U.x0, U.x1, U.x2, U.x3), cy = bezier(t, U.y0, U.y1, U.y2, U.y3);
    const float tx = bezier_tangent(t, U.x1 - U.x0, U.x2 - U.x1, U.x3 - U.x2), ty = bezier_tangent(t, U.y1 - U.y0, U.y2 - U.y1, U.y3 - U.y2);
    const float tangent_len = __builtin_sqrtf(tx * tx + ty * ty);
    if (tangent_len < 0.0001f) return 0u;                             // :674
    const float nx = -ty / tangent_len, ny = tx / tangent_len;
    const float rel_x = px - cx, rel_y = py - cy;
    const float perp = rel_x * nx + rel_y * ny;
    const float idx_f = t * 256.0f;                                   // arc_length_to_t_inverse :698-704; t is within [0, 1]
    const uint32_t idx = min((uint32_t)idx_f, 255u);
    const float frac = idx_f - (float)idx;
    const float sx = s_len[idx] + frac * (s_len[idx + 1u] - s_len[idx]);
    const float sy = U.half_h - perp;
    if (!(sx >= 0.0f && sx < U.w && sy >= 0.0f && sy < U.h)) return 0u;
    return sample(src, U.src_w, U.src_h, sx, sy);
}

__global__ __launch_bounds__(256) void path_kernel(const uint32_t* __restrict__ src, uint32_t* __restrict__ out, uint32_t tiles_x, const pfxk_textwarp P,
                                                   const pfxk_textwarp_tables T)
{
    __shared__ float s_cx[65], s_cy[65], s_len[257];
    for (uint32_t i = threadIdx.x; i < 257u; i += 256u) s_len[i] = T.len[i];
    if (threadIdx.x < 65u) { s_cx[threadIdx.x] = T.cx[threadIdx.x]; s_cy[threadIdx.x] = T.cy[threadIdx.x]; }
    __syncthreads();
    const path_uniforms U = {P.top[0][0], P.top[1][0], P.top[2][0], P.top[3][0], P.top[0][1], P.top[1][1], P.top[2][1], P.top[3][1], P.half_h, P.w, P.h, P.src_w, P.src_h};
    walk_tile(out, P.out_w, P.out_h, tiles_x, [&](uint32_t ox, uint32_t oy) -> uint32_t {
        return path_pixel(src, s_cx, s_cy, s_len, U, (float)ox + P.min_x, (float)oy + P.min_y);
    });
}

// v_cvt_u32_f32 saturates and maps NaN to 0, so a coordinate that failed its range test still gives a row that a min() keeps inside the source
PFX_DEV uint32_t cvt_u32_sat(float v)
{
    uint32_t r;
    asm("v_cvt_u32_f32 %0, %1" : "=v"(r) : "v"(v));
    return r;
}

// apply_envelope_warp :495-536, one output column per lane and ENV_ROWS rows down it: what depends on the column alone (:504-515 t, top_y, span, and of
// bilinear_sample the source column, the x weights and the tap offsets) is computed once into registers, a wave's tap loads and stores are contiguous, and
// the taps of ENV_BATCH rows are requested before any is consumed.  A tap past the right or bottom edge is read from a clamped address with the weight 0
// (p * 0 * w is the reference's 0.0 * fx * w: +0), so no loaded value is tested.  RDIV: the launcher found the source below 2^22 x 2^24 and the curves within
// +-2^18, so row offsets fit v_mad_u32_u24 and every quotient lies where k_common.h's shared-reciprocal division is proved to equal `/`, but for a numerator
// below 2^-90, which takes the plain divide behind a wave-uniform branch
constexpr uint32_t ENV_ROWS = 32, ENV_BATCH = 4;
template <bool RDIV>
__global__ __launch_bounds__(256) void envelope_kernel(const uint32_t* __restrict__ src, uint32_t* __restrict__ out, uint32_t tiles_x, const pfxk_textwarp P)
{
    const uint32_t ox = (blockIdx.x % tiles_x) * 64u + (threadIdx.x & 63u);
    const uint32_t y_first = ((blockIdx.x / tiles_x) * WAVES + (threadIdx.x >> 6)) * ENV_ROWS;
    if (ox >= P.out_w) return;
    const float px = (float)ox + P.min_x;
    const float t = (px - P.min_x) / P.t_den;                             // :504, the margin-shifted min_x as the reference has it
    const float top_y = bezier(t, P.top[0][1], P.top[1][1], P.top[2][1], P.top[3][1]);
    const float bot_y = bezier(t, P.bottom[0][1], P.bottom[1][1], P.bottom[2][1], P.bottom[3][1]);
    const float span_y = bot_y - top_y, sx_t = t * P.w;
    const bool keep = t >= 0.0f && t <= 1.0f && !(__builtin_fabsf(span_y) < 0.001f) && sx_t >= 0.0f && sx_t < P.w;
    const float sx = keep ? sx_t : 0.0f, span = keep ? span_y : 1.0f;
    const float x0f = __builtin_floorf(sx), fx_true = sx - x0f, ux = 1.0f - fx_true;
    const uint32_t x0 = min(cvt_u32_sat(x0f), P.src_w - 1u);              // inside already (sx < w): the min only keeps a load in bounds
    const bool in_x1 = x0 + 1u < P.src_w;
    const float fx = in_x1 ? fx_true : 0.0f;
    const uint32_t o0 = x0 * 4u, step_x = in_x1 ? 4u : 0u, pitch = P.src_w * 4u, last_row = P.src_h - 1u;
    const rdiv D = rdiv_prepare(span);
    const char* __restrict__ base = (const char*)src;
    const uint32_t y_end = min(y_first + ENV_ROWS, P.out_h);
    char* __restrict__ out_base = (char*)out;
    const uint32_t out_pitch = P.out_w * 4u;                             // byte offsets: an image of at most 256 Mpx ends below 2^32
    uint32_t out_at = y_first * out_pitch + ox * 4u;
    for (uint32_t yb = y_first; yb < y_end; yb += ENV_BATCH, out_at += ENV_BATCH * out_pitch) {
        uint32_t p00[ENV_BATCH], p10[ENV_BATCH], p01[ENV_BATCH], p11[ENV_BATCH];
        float uy[ENV_BATCH], fy[ENV_BATCH];
        bool ok[ENV_BATCH];
#pragma unroll
        for (uint32_t j = 0; j < ENV_BATCH; ++j) {
            const float py = (float)(yb + j) + P.min_y;
            const float n = py - top_y;
            float v;
            if constexpr (RDIV) {
                v = rdiv_apply(D, n);                                     // :518
                if (__builtin_amdgcn_ballot_w64(__builtin_fabsf(n) < 0x1p-90f) != 0ull) v = n / span;
            } else {
                v = n / span;
            }
            const float sy = v * P.h;                                     // v >= 0 and h > 0: sy >= 0 holds with it
            ok[j] = keep && v >= 0.0f && v <= 1.0f && sy < P.h;
            const float y0f = __builtin_floorf(sy), f = sy - y0f;
            const uint32_t y0 = min(cvt_u32_sat(y0f), last_row);
            const bool in_y1 = y0 < last_row;
            uy[j] = 1.0f - f;
            fy[j] = in_y1 ? f : 0.0f;
            const uint32_t r0 = (RDIV ? __umul24(y0, pitch) : y0 * pitch) + o0, r1 = r0 + (in_y1 ? pitch : 0u);
            p00[j] = *(const uint32_t*)(base + r0); p10[j] = *(const uint32_t*)(base + (r0 + step_x));
            p01[j] = *(const uint32_t*)(base + r1); p11[j] = *(const uint32_t*)(base + (r1 + step_x));
        }
#pragma unroll
        for (uint32_t j = 0; j < ENV_BATCH; ++j) {
            const float r = ubyte0(p00[j]) * ux * uy[j] + ubyte0(p10[j]) * fx * uy[j] + ubyte0(p01[j]) * ux * fy[j] + ubyte0(p11[j]) * fx * fy[j];
            const float g = ubyte1(p00[j]) * ux * uy[j] + ubyte1(p10[j]) * fx * uy[j] + ubyte1(p01[j]) * ux * fy[j] + ubyte1(p11[j]) * fx * fy[j];
            const float b = ubyte2(p00[j]) * ux * uy[j] + ubyte2(p10[j]) * fx * uy[j] + ubyte2(p01[j]) * ux * fy[j] + ubyte2(p11[j]) * fx * fy[j];
            const float a = ubyte3(p00[j]) * ux * uy[j] + ubyte3(p10[j]) * fx * uy[j] + ubyte3(p01[j]) * ux * fy[j] + ubyte3(p11[j]) * fx * fy[j];
            // a rejected pixel's weights may be anything: its packed value is computed and dropped
            if (yb + j < y_end) *(uint32_t*)(out_base + (out_at + j * out_pitch)) = ok[j] ? pack_round_rgba_finite(r, g, b, a) : 0u;
        }
    }
}

// rotate_glyph_buffer :605-647: the +1 taps are clamped to the last column / row, not transparent
__global__ __launch_bounds__(256) void rotate_kernel(const uint32_t* __restrict__ src, uint32_t* __restrict__ out, uint32_t tiles_x, const pfxk_textrotate R)
{
    const float fw = (float)R.w, fh = (float)R.h;
    walk_tile(out, R.new_w, R.new_h, tiles_x, [&](uint32_t ox, uint32_t oy) -> uint32_t {
        const float dx = (float)ox - R.new_cx, dy = (float)oy - R.new_cy;
        const float sx = dx * R.cos_a + dy * R.sin_a + R.cx;
        const float sy = -dx * R.sin_a + dy * R.cos_a + R.cy;
        if (!(sx >= 0.0f && sx < fw && sy >= 0.0f && sy < fh)) return 0u;
        const float x0f = __builtin_floorf(sx), y0f = __builtin_floorf(sy);
        const uint32_t x0 = min((uint32_t)x0f, R.w - 1u), y0 = min((uint32_t)y0f, R.h - 1u);   // inside already: the min only keeps a load in bounds
        const uint32_t x1 = min(x0 + 1u, R.w - 1u), y1 = min(y0 + 1u, R.h - 1u);
        const float fx = sx - x0f, fy = sy - y0f, ux = 1.0f - fx, uy = 1.0f - fy;
        const uint32_t p00 = src[(size_t)y0 * R.w + x0], p10 = src[(size_t)y0 * R.w + x1], p01 = src[(size_t)y1 * R.w + x0], p11 = src[(size_t)y1 * R.w + x1];
        const float r = ubyte0(p00) * ux * uy + ubyte0(p10) * fx * uy + ubyte0(p01) * ux * fy + ubyte0(p11) * fx * fy;
        const float g = ubyte1(p00) * ux * uy + ubyte1(p10) * fx * uy + ubyte1(p01) * ux * fy + ubyte1(p11) * fx * fy;
        const float b = ubyte2(p00) * ux * uy + ubyte2(p10) * fx * uy + ubyte2(p01) * ux * fy + ubyte2(p11) * fx * fy;
        const float a = ubyte3(p00) * ux * uy + ubyte3(p10) * fx * uy + ubyte3(p01) * ux * fy + ubyte3(p11) * fx * fy;
        return pack_round_rgba_finite(r, g, b, a);
    });
}

// blit_rgba_buffer :39-70 over the part of the buffer that lies on the canvas: [bx0, bx0 + rw) x [by0, by0 + rh) of the buffer lands at (cx0, cy0)
__global__ __launch_bounds__(256) void blit_kernel(const uint32_t* __restrict__ buf, uint32_t bw, uint32_t bx0, uint32_t by0, uint32_t rw, uint32_t rh,
                                                   uint32_t* __restrict__ canvas, uint32_t cw, uint32_t cx0, uint32_t cy0, uint32_t tiles_x)
{
    const auto [x, y] = tile_xy<64, 4>(tiles_x, threadIdx.x, threadIdx.y);
    if (x >= rw || y >= rh) return;
    const uint32_t s = buf[(size_t)(by0 + y) * bw + bx0 + x];
    if (s >> 24) canvas[(size_t)(cy0 + y) * cw + cx0 + x] = s;
}

inline bool warp_ok(const uint8_t* d_src, uint8_t* d_out, const pfxk_textwarp* P)
{
    return d_src && d_out && P && dims_ok(P->src_w, P->src_h) && dims_ok(P->out_w, P->out_h);
}

} // namespace

extern "C" hipError_t pfxk_textwarp_arc(hipStream_t s, const uint8_t* d_src, uint8_t* d_out, const pfxk_textwarp* P)
{
    if (!warp_ok(d_src, d_out, P)) return hipErrorInvalidValue;
    uint32_t tiles_x;
    const uint32_t blocks = tile_grid<TW, TH>(P->out_w, P->out_h, &tiles_x);
    arc_kernel<<<blocks, 256, 0, s>>>((const uint32_t*)d_src, (uint32_t*)d_out, tiles_x, *P);
    return hipGetLastError();
}

extern "C" hipError_t pfxk_textwarp_circular(hipStream_t s, const uint8_t* d_src, uint8_t* d_out, const pfxk_textwarp* P)
{
    if (!warp_ok(d_src, d_out, P)) return hipErrorInvalidValue;
    // |pixel_angle| <= pi and |start_angle| <= 8 pi keep each of the kernel's two loops to five steps; anything else is not launched
    if (!(__builtin_fabsf(P->start_angle) <= 25.2f) || !(P->dir == 1.0f || P->dir == -1.0f)) return hipErrorInvalidValue;
    uint32_t tiles_x;
    const uint32_t blocks = tile_grid<TW, TH>(P->out_w, P->out_h, &tiles_x);
    circular_kernel<<<blocks, 256, 0, s>>>((const uint32_t*)d_src, (uint32_t*)d_out, tiles_x, *P);
    return hipGetLastError();
}

extern "C" hipError_t pfxk_textwarp_path(hipStream_t s, const uint8_t* d_src, uint8_t* d_out, const pfxk_textwarp* P, const pfxk_textwarp_tables* T)
{
    if (!warp_ok(d_src, d_out, P) || !T) return hipErrorInvalidValue;
    uint32_t tiles_x;
    const uint32_t blocks = tile_grid<TW, TH>(P->out_w, P->out_h, &tiles_x);
    path_kernel<<<blocks, 256, 0, s>>>((const uint32_t*)d_src, (uint32_t*)d_out, tiles_x, *P, *T);
    return hipGetLastError();
}

extern "C" hipError_t pfxk_textwarp_envelope(hipStream_t s, const uint8_t* d_src, uint8_t* d_out, const pfxk_textwarp* P)
{
    if (!warp_ok(d_src, d_out, P)) return hipErrorInvalidValue;
    // envelope_kernel<true>'s conditions: 24-bit row offsets, numerators and spans within the shared-reciprocal division's proved range
    bool ordinary = P->src_w < (1u << 22) && P->src_h < (1u << 24) && __builtin_fabsf(P->min_y) <= 524288.0f;
    for (int i = 0; i < 4; ++i) ordinary = ordinary && __builtin_fabsf(P->top[i][1]) <= 262144.0f && __builtin_fabsf(P->bottom[i][1]) <= 262144.0f;
    const uint32_t tiles_x = (P->out_w + 63u) / 64u, blocks = tiles_x * ((P->out_h + WAVES * ENV_ROWS - 1u) / (WAVES * ENV_ROWS));
    if (ordinary) envelope_kernel<true><<<blocks, 256, 0, s>>>((const uint32_t*)d_src, (uint32_t*)d_out, tiles_x, *P);
    else envelope_kernel<false><<<blocks, 256, 0, s>>>((const uint32_t*)d_src, (uint32_t*)d_out, tiles_x, *P);
    return hipGetLastError();
}

extern "C" hipError_t pfxk_textwarp_rotate(hipStream_t s, const uint8_t* d_src, uint8_t* d_out, const pfxk_textrotate* R)
{
    if (!d_src || !d_out || !R || !dims_ok(R->w, R->h) || !dims_ok(R->new_w, R->new_h)) return hipErrorInvalidValue;
    uint32_t tiles_x;
    const uint32_t blocks = tile_grid<TW, TH>(R->new_w, R->new_h, &tiles_x);
    rotate_kernel<<<blocks, 256, 0, s>>>((const uint32_t*)d_src, (uint32_t*)d_out, tiles_x, *R);
    return hipGetLastError();
}

extern "C" hipError_t pfxk_textwarp_blit(hipStream_t s, const uint8_t* d_buf, uint32_t bw, uint32_t bh, int64_t off_x, int64_t off_y, uint8_t* d_canvas, uint32_t cw,
                                         uint32_t ch)
{
    if (!d_buf || !d_canvas || !dims_ok(bw, bh) || !dims_ok(cw, ch)) return hipErrorInvalidValue;
    // the buffer's columns [bx0, bx1) and rows [by0, by1) that land on the canvas
    const int64_t bx0 = std::max<int64_t>(0, -off_x), by0 = std::max<int64_t>(0, -off_y);
    const int64_t bx1 = std::min<int64_t>(bw, (int64_t)cw - off_x), by1 = std::min<int64_t>(bh, (int64_t)ch - off_y);
    if (bx1 <= bx0 || by1 <= by0) return hipSuccess;
    const uint32_t rw = (uint32_t)(bx1 - bx0), rh = (uint32_t)(by1 - by0), tiles_x = (rw + 63u) / 64u;
    blit_kernel<<<tiles_x * ((rh + 3u) / 4u), dim3(64, 4), 0, s>>>((const uint32_t*)d_buf, bw, (uint32_t)bx0, (uint32_t)by0, rw, rh, (uint32_t*)d_canvas, cw,
                                                                    (uint32_t)(bx0 + off_x), (uint32_t)(by0 + off_y), tiles_x);
    return hipGetLastError();
}
