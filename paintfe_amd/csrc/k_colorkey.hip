// k_colorkey.hip — removal by colour (ref: src/ops/color_removal.rs), bit for bit: u8 -> f32, one rounding per written operation (no contraction), IEEE
// division, round() half away from zero, `as u8` saturating.
//
//   colour to alpha   color_to_alpha_core :64-133: a streaming RGBA8 -> RGBA8 kernel, 16-byte loads, all settings prepared on the host (:51-58) in one struct.
//   passability       the colour remover's step 1 as a cost map for the minimax flood of k_flood.hip: 0 where the flood may pass (selected, and alpha 0 or
//                     dist_sq <= tol_sq, :219-235), else 255.  dist_sq is a sum of three integer squares below 2^24: computed in integers, exact as f32.  In the
//                     global scope (:238-256) the same kernel marks the core itself: alpha 0 is not core there.
//   rings             step 2 (:264-333), a geodesic city-block distance capped at `smoothness`: a workgroup owns a 64 x 64 tile and loads one state byte per pixel
//                     of the tile and a halo of k <= 32 pixels into LDS — a level, unreached, or blocked (unselected / outside the image).  k barrier-separated
//                     steps follow: an unreached pixel with a 4-neighbour at level j - 1 becomes j.  Updating in place is safe: step j writes only the value j
//                     into bytes that held `unreached`, and tests only for j - 1.  A lane owns a dword of four state bytes and compares them at once.  Only the
//                     tile's interior is written back: an interior pixel of level <= k has its whole shortest path within L1 radius k of itself, so inside the
//                     window; halo pixels may end up wrong and are never written (DESIGN.md "Colour removal").
//   write-out         step 3 (:344-415) rides in the last ring launch's write-back; at smoothness 0 it is a streaming kernel over the core map.
#include "k_tools.h"
#include "pfx_kernels.h"

using namespace pfxk;

namespace {

constexpr int RT = PFXK_COLORKEY_TILE;
constexpr int RK = PFXK_COLORKEY_CHUNK;
constexpr int RW = (RT + 2 * RK) / 4;   // dwords per LDS row: 32, so a wave's two half-rows fall on the 32 banks once each
constexpr uint32_t ST_UNREACHED = 0xffu, ST_BLOCKED = 0xfeu, ST_DONE = 0xfdu;   // DONE: a level below the chunk's base, inert (its own ring is complete)
constexpr uint32_t LVL_NONE = 0xffffffffu;

PFX_DEV float luma(float r, float g, float b) { return r * 0.2126f + g * 0.7152f + b * 0.0722f; }   // :139, in that order
PFX_DEV float absdiff255(float a, float b) { return div255(__builtin_fabsf(a - b)); }               // |a - b| is an integer in 0 .. 255

PFX_DEV uint32_t cta_px(uint32_t p, const pfxk_cta& S)
{
    const uint32_t ai = p >> 24;
    if (ai == 0u) return p;   // :75
    const float r = ubyte0(p), g = ubyte1(p), b = ubyte2(p);
    const float max_d = __builtin_fmaxf(__builtin_fmaxf(absdiff255(r, S.target[0]), absdiff255(g, S.target[1])), absdiff255(b, S.target[2]));   // :82
    float contribution = 1.0f - rs_clamp((max_d - S.tolerance) / S.softness, 0.0f, 1.0f);
    if (S.protect > 0.0f) {   // :87
        const float luma_delta = rs_clamp(__builtin_fabsf(luma(r, g, b) - S.target_luma) / 255.0f, 0.0f, 1.0f);
        const float protection = rs_clamp(luma_delta * S.protect, 0.0f, 1.0f);
        contribution *= 1.0f - protection;
    }
    const float removal = rs_clamp(contribution * S.strength, 0.0f, 1.0f);
    if (removal <= 0.0f) return p;   // :94
    const float a = div255((float)ai);
    const float new_a_f = rs_clamp(a * (1.0f - removal), S.alpha_floor, S.alpha_ceiling);
    const float kept = rs_clamp(new_a_f / a, 0.0f, 1.0f);
    const float new_a = round_u8f(new_a_f * 255.0f);
    if (new_a == 0.0f || kept < 0.001f) return (uint32_t)new_a << 24;   // :108: rgb 0, the alpha is written all the same
    float nr = rs_clamp((r - S.target[0] * removal) / kept, 0.0f, 255.0f);
    float ng = rs_clamp((g - S.target[1] * removal) / kept, 0.0f, 255.0f);
    float nb = rs_clamp((b - S.target[2] * removal) / kept, 0.0f, 255.0f);
    if (S.spill > 0.0f) {   // :122, :144: only channels the target has
        const float keep = 1.0f - rs_clamp(S.spill * contribution * (1.0f - kept), 0.0f, 1.0f);
        if (S.target[0] > 0.0f) nr = nr * keep;
        if (S.target[1] > 0.0f) ng = ng * keep;
        if (S.target[2] > 0.0f) nb = nb * keep;
    }
    return pack_rgba(round_u8f(nr), round_u8f(ng), round_u8f(nb), new_a);
}

// VEC: src and dst 16-byte, mask 4-byte aligned — four pixels per lane; the n % 4 tail and the other case go pixel by pixel (RGBA8 pointers are 4-byte aligned: the host checks)
template <bool VEC>
__global__ __launch_bounds__(256) void color_to_alpha_kernel(const uint32_t* src, uint32_t* dst, const uint8_t* __restrict__ mask, size_t n, pfxk_cta S)
{
    stream_walk<VEC, size_t>(n, [&](size_t g) {
        const uint4 v = reinterpret_cast<const uint4*>(src)[g];
        const uint32_t m = mask ? reinterpret_cast<const uint32_t*>(mask)[g] : 0xffffffffu;
        uint4 o;
        o.x = (m & 0xffu) ? cta_px(v.x, S) : v.x;
        o.y = (m & 0xff00u) ? cta_px(v.y, S) : v.y;
        o.z = (m & 0xff0000u) ? cta_px(v.z, S) : v.z;
        o.w = (m >> 24) ? cta_px(v.w, S) : v.w;
        reinterpret_cast<uint4*>(dst)[g] = o;
    }, [&](size_t i) {
        const uint32_t p = src[i];
        dst[i] = (!mask || mask[i] != 0u) ? cta_px(p, S) : p;
    });
}

PFX_DEV uint32_t passable_cost(uint32_t p, uint32_t sel, const pfxk_ckey& P)
{
    if (sel == 0u) return 255u;                                  // :219, :243
    if ((p >> 24) == 0u) return P.global ? 255u : 0u;            // :225 the flood runs through transparent pixels; :249 the global core has none
    const int dr = (int)(p & 0xffu) - (int)(P.seed_rgb & 0xffu), dg = (int)((p >> 8) & 0xffu) - (int)((P.seed_rgb >> 8) & 0xffu),
              db = (int)((p >> 16) & 0xffu) - (int)((P.seed_rgb >> 16) & 0xffu);
    return (float)(dr * dr + dg * dg + db * db) <= P.tol_sq ? 0u : 255u;   // color_dist_sq :429, exact
}

template <bool VEC>
__global__ __launch_bounds__(256) void passable_kernel(const uint32_t* __restrict__ src, const uint8_t* __restrict__ sel, uint8_t* __restrict__ out, size_t n, pfxk_ckey P)
{
    stream_walk<VEC, size_t>(n, [&](size_t g) {
        const uint4 v = reinterpret_cast<const uint4*>(src)[g];
        const uint32_t m = sel ? reinterpret_cast<const uint32_t*>(sel)[g] : 0xffffffffu;
        reinterpret_cast<uint32_t*>(out)[g] = passable_cost(v.x, m & 0xffu, P) | (passable_cost(v.y, m & 0xff00u, P) << 8) |
                                              (passable_cost(v.z, m & 0xff0000u, P) << 16) | (passable_cost(v.w, m >> 24, P) << 24);
    }, [&](size_t i) { out[i] = (uint8_t)passable_cost(src[i], sel ? sel[i] : 255u, P); });
}

// step 3 for a pixel of the dilated mask at ring `lvl` (0 = core)
PFX_DEV uint32_t remove_px(uint32_t p, uint32_t lvl, const pfxk_ckey& P)
{
    const uint32_t ai = p >> 24;
    if (ai == 0u) return p;   // :354
    const float r = ubyte0(p), g = ubyte1(p), b = ubyte2(p);
    const float max_d = __builtin_fmaxf(__builtin_fmaxf(absdiff255(r, P.seed[0]), absdiff255(g, P.seed[1])), absdiff255(b, P.seed[2]));   // :364-367
    float removal = 1.0f - max_d;
    if (lvl > 0u && P.smoothness > 0u) removal *= 1.0f - (float)lvl / P.fade_den;   // :375
    removal = rs_clamp(removal, 0.0f, 1.0f);
    if (removal < 0.004f) return p;   // :381
    const float kept = 1.0f - removal;
    const float new_a = round_u8f(div255((float)ai) * kept * 255.0f);   // :386-387
    if (new_a == 0.0f) return 0u;
    if (kept < 0.001f) return (p & 0x00ffffffu) | ((uint32_t)new_a << 24);   // :402, not reachable with new_a != 0; kept for fidelity
    return pack_rgba(round_u8f((r - P.seed[0] * removal) / kept), round_u8f((g - P.seed[1] * removal) / kept), round_u8f((b - P.seed[2] * removal) / kept), new_a);
}

template <bool VEC>
__global__ __launch_bounds__(256) void apply_core_kernel(const uint32_t* src, const uint8_t* __restrict__ core, uint32_t* dst, size_t n, pfxk_ckey P)
{
    stream_walk<VEC, size_t>(n, [&](size_t g) {
        const uint4 v = reinterpret_cast<const uint4*>(src)[g];
        const uint32_t c = reinterpret_cast<const uint32_t*>(core)[g];
        uint4 o;
        o.x = (c & 0xffu) ? v.x : remove_px(v.x, 0u, P);
        o.y = (c & 0xff00u) ? v.y : remove_px(v.y, 0u, P);
        o.z = (c & 0xff0000u) ? v.z : remove_px(v.z, 0u, P);
        o.w = (c >> 24) ? v.w : remove_px(v.w, 0u, P);
        reinterpret_cast<uint4*>(dst)[g] = o;
    }, [&](size_t i) {
        const uint32_t p = src[i];
        dst[i] = core[i] != 0u ? p : remove_px(p, 0u, P);
    });
}

// 0x80 in every byte of x that is zero, 0 elsewhere (exact: no borrow crosses a byte)
PFX_DEV uint32_t zero_bytes(uint32_t x) { return ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu); }

// IN16: the known levels come from a u16 map and `base` > 0 (else from the core map, base 0).  FINAL: the write-back is step 3 into dst (else the u16 map lout).
// A lane's dword is column cw of the rows it walks; the window's left edge is x0 - ka with ka = k rounded up to 4, so a pixel's dword never straddles two lanes.
template <bool IN16, bool FINAL>
__global__ __launch_bounds__(256) void ring_kernel(const uint8_t* __restrict__ core, const uint16_t* __restrict__ lin, const uint8_t* __restrict__ sel, uint16_t* __restrict__ lout,
                                                   const uint32_t* src, uint32_t* dst, uint32_t w, uint32_t h, uint32_t tiles_x, uint32_t base, int k, pfxk_ckey P)
{
    __shared__ uint32_t sS[(RT + 2 * RK) * RW];   // 128 rows of 128 state bytes
    const int t = (int)threadIdx.x, cw = t & (RW - 1), r0 = t >> 5;
    const int ka = (k + 3) & ~3, ww = (RT + 2 * ka) / 4, wr = RT + 2 * k;   // the window: ww dwords by wr rows
    const int x0 = (int)(blockIdx.x % tiles_x) * RT, y0 = (int)(blockIdx.x / tiles_x) * RT;
    const bool lane_on = cw < ww;
    if (lane_on) {
        for (int r = r0; r < wr; r += 8) {
            const int gy = y0 - k + r;
            uint32_t word = 0u;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int gx = x0 - ka + cw * 4 + j;
                uint32_t st = ST_BLOCKED;   // outside the image, or unselected: a ring never passes (:292, :324)
                if (gy >= 0 && gy < (int)h && gx >= 0 && gx < (int)w) {
                    const size_t gi = (size_t)gy * w + (size_t)gx;
                    if (!sel || sel[gi] != 0u) {
                        if constexpr (IN16) {
                            const uint32_t l = lin[gi];
                            st = l == PFXK_COLORKEY_NONE ? ST_UNREACHED : (l == base ? 0u : ST_DONE);
                        } else {
                            st = core[gi] == 0u ? 0u : ST_UNREACHED;
                        }
                    }
                }
                word |= st << (8 * j);
            }
            sS[r * RW + cw] = word;
        }
    }
    const uint32_t blocked = ST_BLOCKED * 0x01010101u;
    __syncthreads();
    for (int j = 1; j <= k; ++j) {   // every step ends in a barrier
        // a pixel that step j must get right lies at least j rows inside the window (its path of j steps does): the rows walked shrink with j
        const uint32_t want = (uint32_t)(j - 1) * 0x01010101u, mine = (uint32_t)j * 0x01010101u;
        int changed = 0;
        if (lane_on) {
            for (int r = j + r0; r < wr - j; r += 8) {
                const uint32_t c = sS[r * RW + cw];
                const uint32_t open = zero_bytes(~c);   // bytes still unreached
                if (open == 0u) continue;
                const uint32_t up = sS[(r - 1) * RW + cw], dn = sS[(r + 1) * RW + cw];   // j >= 1: both rows are inside the window
                const uint32_t lw = cw > 0 ? sS[r * RW + cw - 1] : blocked, rw = cw + 1 < ww ? sS[r * RW + cw + 1] : blocked;
                const uint32_t left = (c << 8) | (lw >> 24), right = (c >> 8) | (rw << 24);
                const uint32_t hit = (zero_bytes(up ^ want) | zero_bytes(dn ^ want) | zero_bytes(left ^ want) | zero_bytes(right ^ want)) & open;
                if (hit != 0u) {
                    const uint32_t full = (hit >> 7) * 0xffu;
                    sS[r * RW + cw] = (c & ~full) | (mine & full);
                    changed = 1;
                }
            }
        }
        if (!__syncthreads_or(changed)) break;   // no pixel at level j: no later level either
    }
    const uint8_t* sB = reinterpret_cast<const uint8_t*>(sS);
    const int col = t & 63, gx = x0 + col;
    if (gx >= (int)w) return;
    for (int rr = t >> 6; rr < RT; rr += 4) {
        const int gy = y0 + rr;
        if (gy >= (int)h) break;
        const size_t gi = (size_t)gy * w + (size_t)gx;
        const uint32_t st = sB[(rr + k) * (RW * 4) + ka + col];
        uint32_t lvl = LVL_NONE;
        if (st <= (uint32_t)k) lvl = base + st;
        else if (st == ST_DONE) {
            if constexpr (IN16) lvl = lin[gi];
        }
        if constexpr (FINAL) {
            const uint32_t p = src[gi];
            dst[gi] = lvl == LVL_NONE ? p : remove_px(p, lvl, P);
        } else {
            lout[gi] = (uint16_t)(lvl == LVL_NONE ? PFXK_COLORKEY_NONE : lvl);
        }
    }
}

} // namespace

extern "C" hipError_t pfxk_color_to_alpha(hipStream_t s, const uint8_t* d_src, uint8_t* d_dst, const uint8_t* d_mask, size_t n, const pfxk_cta* S)
{
    if (n == 0) return hipSuccess;
    return launch_stream(aligned_to(d_src, 16) && aligned_to(d_dst, 16) && aligned_to(d_mask, 4), n, s, color_to_alpha_kernel<true>, color_to_alpha_kernel<false>,
                         (const uint32_t*)d_src, (uint32_t*)d_dst, d_mask, n, *S);
}

extern "C" hipError_t pfxk_ckey_passable(hipStream_t s, const uint8_t* d_src, const uint8_t* d_sel, uint8_t* d_out, size_t n, const pfxk_ckey* P)
{
    if (n == 0) return hipSuccess;
    return launch_stream(aligned_to(d_src, 16) && aligned_to(d_sel, 4) && aligned_to(d_out, 4), n, s, passable_kernel<true>, passable_kernel<false>,
                         (const uint32_t*)d_src, d_sel, d_out, n, *P);
}

extern "C" hipError_t pfxk_ckey_apply_core(hipStream_t s, const uint8_t* d_src, const uint8_t* d_core, uint8_t* d_dst, size_t n, const pfxk_ckey* P)
{
    if (n == 0) return hipSuccess;
    return launch_stream(aligned_to(d_src, 16) && aligned_to(d_dst, 16) && aligned_to(d_core, 4), n, s, apply_core_kernel<true>, apply_core_kernel<false>,
                         (const uint32_t*)d_src, d_core, (uint32_t*)d_dst, n, *P);
}

extern "C" hipError_t pfxk_ckey_rings(hipStream_t s, const uint8_t* d_core, const uint16_t* d_lin, const uint8_t* d_sel, uint16_t* d_lout, const uint8_t* d_src,
                                      uint8_t* d_dst, uint32_t w, uint32_t h, uint32_t base, uint32_t k, const pfxk_ckey* P)
{
    if (w == 0 || h == 0) return hipSuccess;
    if (k < 1u || k > (uint32_t)RK || (d_lin ? base == 0u : base != 0u) || (uint64_t)base + k > PFXK_COLORKEY_MAX_SMOOTHNESS || (d_lout && d_lout == d_lin) ||
        (!d_lin && !d_core) || (!d_lout && (!d_src || !d_dst)))
        return hipErrorInvalidValue;
    const uint32_t tiles_x = (w + RT - 1) / RT, tiles_y = (h + RT - 1) / RT;
    const uint64_t tiles = (uint64_t)tiles_x * tiles_y;
    if (tiles > 0x7fffffffull) return hipErrorInvalidValue;
    const uint32_t* src = (const uint32_t*)d_src;
    uint32_t* dst = (uint32_t*)d_dst;
    if (d_lin) {
        if (d_lout) ring_kernel<true, false><<<(uint32_t)tiles, 256, 0, s>>>(d_core, d_lin, d_sel, d_lout, src, dst, w, h, tiles_x, base, (int)k, *P);
        else ring_kernel<true, true><<<(uint32_t)tiles, 256, 0, s>>>(d_core, d_lin, d_sel, d_lout, src, dst, w, h, tiles_x, base, (int)k, *P);
    } else {
        if (d_lout) ring_kernel<false, false><<<(uint32_t)tiles, 256, 0, s>>>(d_core, d_lin, d_sel, d_lout, src, dst, w, h, tiles_x, base, (int)k, *P);
        else ring_kernel<false, true><<<(uint32_t)tiles, 256, 0, s>>>(d_core, d_lin, d_sel, d_lout, src, dst, w, h, tiles_x, base, (int)k, *P);
    }
    return hipGetLastError();
}
