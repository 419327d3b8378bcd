// k_inpaint.hip — content-aware fill (ref: src/ops/inpaint.rs): the instant heal dabs (inpaint_instant_brush :76-192) and the onion-peeling PatchMatch
// (fill_region_patchmatch :394-520).  Both are in the bit-exact class: every f32 expression is the reference's, in its order, without contraction; the one
// per-pixel transcendental is exp (libm_exp = glibc's expf bit for bit), the ring's cos / sin are uniform and come from the host (pfx_inpaint_ring_offsets).
//
// PatchMatch keeps the reference's serial scan orders — they pick the random seeds and break SSD ties with a strict `<` — in a form without any wait between
// workgroups: a peel's boundary pixels are compacted stably in row-major order (count / scan / scatter: three launches), a pass is ONE workgroup that sweeps
// the anti-diagonals x + y with a block barrier between them (forward passes read the left / up neighbours' NNF, backward passes right / down, so pixels of one
// diagonal never read each other), and every other step is a map over the boundary list.  One wave per boundary pixel: the patch's pixels spread over the lanes.
#include "k_libm.h"
#include "k_tools.h"
#include "pfx_kernels.h"

namespace {
using namespace pfxk;

constexpr float F32_MAX = 3.40282347e+38f;

// f32::round (half away from zero), exact: trunc, then one step where the fraction reaches 0.5
PFX_DEV float rs_round(float v)
{
    float t = __builtin_truncf(v);
    if (__builtin_fabsf(v - t) >= 0.5f) t += __builtin_copysignf(1.0f, v);
    return t;
}
// Rust `as i32`: truncate, saturate, NaN -> 0
PFX_DEV int32_t as_i32(float v)
{
    if (v != v) return 0;
    if (v >= 2147483648.0f) return 2147483647;
    if (v <= -2147483648.0f) return -2147483647 - 1;
    return (int32_t)v;
}

// ================================================================================================ instant dabs
// One thread per pixel of the dabs' union box; a thread walks the dab list in order.  A pixel's result depends on its own `out` value, on src and on the mask
// only, so one launch covers the list without a race: src and mask are read-only, out is touched at the thread's own pixel.
__global__ __launch_bounds__(256) void inpaint_instant_kernel(const uint32_t* __restrict__ src, const uint8_t* __restrict__ mask, uint32_t* out, int w, int h,
                                                              const pfxk_inpaint_dab* __restrict__ dabs, uint32_t n_dabs, const float* __restrict__ rings,
                                                              uint32_t bx0, uint32_t by0, uint32_t bx1, uint32_t by1)
{
    const uint32_t x = bx0 + blockIdx.x * 64u + (threadIdx.x & 63u), y = by0 + blockIdx.y * 4u + (threadIdx.x >> 6);
    if (x > bx1 || y > by1) return;
    const size_t i = (size_t)y * (uint32_t)w + x;
    if (mask[i] == 0) return;                                             // :101-107 only painted-over pixels
    const uint32_t before = out[i], ref = src[i];
    uint32_t o = before;
    const float xf = (float)x, yf = (float)y, ref_r = ubyte0(ref), ref_g = ubyte1(ref), ref_b = ubyte2(ref);
    for (uint32_t d = 0; d < n_dabs; ++d) {
        const pfxk_inpaint_dab D = dabs[d];
        if (x < D.x0 || x > D.x1 || y < D.y0 || y > D.y1) continue;      // :93-99 the dab's own loop bounds
        const float dx = xf - D.cx, dy = yf - D.cy;
        const float dist = sqrtf(dx * dx + dy * dy);
        if (dist > D.r) continue;
        const float t = rs_clamp(dist / D.r, 0.0f, 1.0f);
        float geom_alpha = 1.0f;
        if (!(t < D.hard_t)) {
            const float s = (t - D.hard_t) / D.soft_den;
            geom_alpha = 1.0f - s * s * (3.0f - 2.0f * s);
        }
        if (geom_alpha < 0.01f) continue;
        const float* ring = rings + (size_t)D.ring * 64u;
        float sum_r = 0.0f, sum_g = 0.0f, sum_b = 0.0f, weight_total = 0.0f;   // sum_a feeds nothing (:177 _filled_a)
        for (int c = 0; c < 32; ++c) {
            const int32_t sx = as_i32(rs_round(xf + ring[2 * c])), sy = as_i32(rs_round(yf + ring[2 * c + 1]));
            if (sx < 0 || sx >= w || sy < 0 || sy >= h) continue;
            const size_t si = (size_t)sy * (uint32_t)w + (uint32_t)sx;
            if (mask[si] > 0) continue;
            const uint32_t sp = src[si];
            const float dr = ubyte0(sp) - ref_r, dg = ubyte1(sp) - ref_g, db = ubyte2(sp) - ref_b;
            const float w_color = libm_exp(-(dr * dr + dg * dg + db * db) / 2500.0f);
            sum_r += ubyte0(sp) * w_color;
            sum_g += ubyte1(sp) * w_color;
            sum_b += ubyte2(sp) * w_color;
            weight_total += w_color;
        }
        if (weight_total < 1e-6f) continue;
        const float filled_r = quant255(sum_r / weight_total), filled_g = quant255(sum_g / weight_total), filled_b = quant255(sum_b / weight_total);
        const float ea = ubyte3(o) / 255.0f;
        if (geom_alpha >= ea) {
            const float er = ubyte0(o), eg = ubyte1(o), eb = ubyte2(o);   // lerp_u8 :195
            o = pack_rgba(quant255(er + (filled_r - er) * geom_alpha), quant255(eg + (filled_g - eg) * geom_alpha), quant255(eb + (filled_b - eb) * geom_alpha),
                          trunc_u8f(geom_alpha * 255.0f));
        }
    }
    if (o != before) out[i] = o;
}

// ================================================================================================ PatchMatch
struct pm_geom {
    int w, h;               // canvas
    int x0, y0, bw, bh;     // the hole's bounding box; the NNF arrays cover it plus one pixel on every side
    int half, min_valid;
    float max_radius;
};
PFX_DEV uint32_t nnf_index(const pm_geom& G, int x, int y) { return (uint32_t)(y - G.y0 + 1) * (uint32_t)(G.bw + 2) + (uint32_t)(x - G.x0 + 1); }
// NNF entries written by one wave are read by others of the same workgroup behind a barrier, and by later launches: device-scope relaxed accesses keep them out of
// any per-CU cache question
template <class T> PFX_DEV T dev_load(const T* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
template <class T> PFX_DEV void dev_store(T* p, T v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

PFX_DEV uint32_t wave_sum(uint32_t v)
{
    for (int m = 32; m >= 1; m >>= 1) v += (uint32_t)__shfl_xor((int)v, m, 64);
    return v;
}

// exclusive scan of one value per thread over the block (NT threads); lds holds NT / 64 + 1 words
template <int NT> PFX_DEV uint32_t block_scan(uint32_t v, uint32_t* lds, uint32_t& total)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t inc = v;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = (uint32_t)__shfl_up((int)inc, o, 64);
        if (lane >= (uint32_t)o) inc += t;
    }
    if (lane == 63u) lds[wave] = inc;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t run = 0;
        for (int i = 0; i < NT / 64; ++i) { const uint32_t t = lds[i]; lds[i] = run; run += t; }
        lds[NT / 64] = run;
    }
    __syncthreads();
    const uint32_t res = lds[wave] + inc - v;
    total = lds[NT / 64];
    __syncthreads();
    return res;
}

// hole statistics into zeroed words: stats[0..3] = ~min x, ~min y, max x, max y of mask != 0 (all four by atomic max), stats[4] = hole pixels
__global__ __launch_bounds__(256) void pm_stats_kernel(const uint8_t* __restrict__ mask, uint32_t w, uint32_t h, uint32_t* stats)
{
    const uint32_t n = w * h;
    uint32_t lo_x = ~0u, lo_y = ~0u, hi_x = 0, hi_y = 0, cnt = 0;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        if (mask[i] == 0) continue;
        const uint32_t x = i % w, y = i / w;
        lo_x = min(lo_x, x); lo_y = min(lo_y, y); hi_x = max(hi_x, x); hi_y = max(hi_y, y);
        ++cnt;
    }
    for (int m = 32; m >= 1; m >>= 1) {
        lo_x = min(lo_x, (uint32_t)__shfl_xor((int)lo_x, m, 64)); lo_y = min(lo_y, (uint32_t)__shfl_xor((int)lo_y, m, 64));
        hi_x = max(hi_x, (uint32_t)__shfl_xor((int)hi_x, m, 64)); hi_y = max(hi_y, (uint32_t)__shfl_xor((int)hi_y, m, 64));
    }
    cnt = wave_sum(cnt);
    if ((threadIdx.x & 63u) == 0 && cnt) {
        atomicMax(&stats[0], ~lo_x); atomicMax(&stats[1], ~lo_y); atomicMax(&stats[2], hi_x); atomicMax(&stats[3], hi_y);
        atomicAdd(&stats[4], cnt);
    }
}

// is_boundary_hole :214-232
PFX_DEV bool is_boundary(const uint8_t* mask, int w, int h, int x, int y)
{
    const size_t i = (size_t)y * (uint32_t)w + (uint32_t)x;
    if (mask[i] == 0) return false;
    return (x > 0 && mask[i - 1] == 0) || (x + 1 < w && mask[i + 1] == 0) || (y > 0 && mask[i - (uint32_t)w] == 0) || (y + 1 < h && mask[i + (uint32_t)w] == 0);
}

// Stable compaction in row-major order of a rectangle's pixels that pass a test — KIND 0: mask == 0 (the initial source list), 1: boundary pixel of the live
// mask.  Element e of the rectangle is (rx0 + e % rw, ry0 + e / rw); a block owns 1024 consecutive elements, a thread 4 consecutive ones.
template <int KIND> PFX_DEV uint32_t compact_flags(const uint8_t* mask, int w, int h, int rx0, int ry0, uint32_t rw, uint32_t n, uint32_t e0, uint32_t idx[4])
{
    uint32_t c = 0;
    for (uint32_t k = 0; k < 4; ++k) {
        const uint32_t e = e0 + k;
        if (e >= n) break;
        const int x = rx0 + (int)(e % rw), y = ry0 + (int)(e / rw);
        const uint32_t li = (uint32_t)y * (uint32_t)w + (uint32_t)x;
        const bool keep = KIND == 0 ? mask[li] == 0 : is_boundary(mask, w, h, x, y);
        if (keep) idx[c++] = li;
    }
    return c;
}
template <int KIND>
__global__ __launch_bounds__(256) void pm_count_kernel(const uint8_t* __restrict__ mask, int w, int h, int rx0, int ry0, uint32_t rw, uint32_t n, uint32_t* counts)
{
    __shared__ uint32_t lds[5];
    uint32_t idx[4], total;
    const uint32_t c = compact_flags<KIND>(mask, w, h, rx0, ry0, rw, n, blockIdx.x * 1024u + threadIdx.x * 4u, idx);
    block_scan<256>(c, lds, total);
    if (threadIdx.x == 0) counts[blockIdx.x] = total;
}
// in-place exclusive scan of the per-block counts by one workgroup; *total_out = their sum
__global__ __launch_bounds__(1024) void pm_scan_kernel(uint32_t* counts, uint32_t n_blocks, uint32_t* total_out)
{
    __shared__ uint32_t lds[17];
    uint32_t carry = 0;
    for (uint32_t base = 0; base < n_blocks; base += 1024u) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < n_blocks ? counts[i] : 0u;
        uint32_t total;
        const uint32_t ex = block_scan<1024>(v, lds, total);
        if (i < n_blocks) counts[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) *total_out = carry;
}
template <int KIND>
__global__ __launch_bounds__(256) void pm_scatter_kernel(const uint8_t* __restrict__ mask, int w, int h, int rx0, int ry0, uint32_t rw, uint32_t n,
                                                         const uint32_t* __restrict__ offsets, uint32_t* list)
{
    __shared__ uint32_t lds[5];
    uint32_t idx[4], total;
    const uint32_t c = compact_flags<KIND>(mask, w, h, rx0, ry0, rw, n, blockIdx.x * 1024u + threadIdx.x * 4u, idx);
    const uint32_t at = offsets[blockIdx.x] + block_scan<256>(c, lds, total);
    for (uint32_t k = 0; k < c; ++k) list[at + k] = idx[k];
}

// the boundary list bucketed by anti-diagonal d = (x - x0) + (y - y0): diag_start[0 .. n_diag] and the pixels of diagonal d at diag_list[diag_start[d] ..
// diag_start[d + 1]) in any order (a diagonal's pixels run in parallel).  One workgroup; cursor = n_diag words of scratch.
__global__ __launch_bounds__(1024) void pm_bucket_kernel(const uint32_t* __restrict__ boundary, uint32_t nb, pm_geom G, uint32_t n_diag, uint32_t* diag_start,
                                                         uint32_t* cursor, uint32_t* diag_list)
{
    __shared__ uint32_t lds[17];
    for (uint32_t d = threadIdx.x; d < n_diag; d += 1024u) dev_store(&cursor[d], 0u);
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < nb; i += 1024u) {
        const uint32_t li = boundary[i];
        atomicAdd(&cursor[(li % (uint32_t)G.w - (uint32_t)G.x0) + (li / (uint32_t)G.w - (uint32_t)G.y0)], 1u);
    }
    __syncthreads();
    uint32_t carry = 0;
    for (uint32_t base = 0; base < n_diag; base += 1024u) {
        const uint32_t d = base + threadIdx.x;
        const uint32_t v = d < n_diag ? dev_load(&cursor[d]) : 0u;
        uint32_t total;
        const uint32_t ex = block_scan<1024>(v, lds, total);
        if (d < n_diag) { dev_store(&diag_start[d], carry + ex); dev_store(&cursor[d], carry + ex); }
        carry += total;
    }
    if (threadIdx.x == 0) dev_store(&diag_start[n_diag], carry);
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < nb; i += 1024u) {
        const uint32_t li = boundary[i];
        const uint32_t at = atomicAdd(&cursor[(li % (uint32_t)G.w - (uint32_t)G.x0) + (li / (uint32_t)G.w - (uint32_t)G.y0)], 1u);
        diag_list[at] = li;
    }
}

// The query side of patch_ssd_masked for one boundary pixel, held by the wave: patch slot p = lane + 64 k (k = 0, 1; (2 half + 1)^2 <= 121) is the patch pixel
// (p % side - half, p / side - half); ok = inside the canvas and not in the hole.
struct pm_query { uint32_t px[2]; bool ok[2]; };
PFX_DEV pm_query load_query(const pm_geom& G, const uint32_t* img, const uint8_t* mask, int ax, int ay)
{
    pm_query Q;
    const int side = 2 * G.half + 1, n = side * side, lane = (int)(threadIdx.x & 63u);
    for (int k = 0; k < 2; ++k) {
        const int p = lane + 64 * k, apx = ax + p % side - G.half, apy = ay + p / side - G.half;
        Q.ok[k] = false;
        Q.px[k] = 0u;
        if (p < n && apx >= 0 && apy >= 0 && apx < G.w && apy < G.h) {
            const size_t i = (size_t)apy * (uint32_t)G.w + (uint32_t)apx;
            if (mask[i] == 0) { Q.ok[k] = true; Q.px[k] = img[i]; }
        }
    }
    return Q;
}
PFX_DEV uint32_t sq_diff3(uint32_t a, uint32_t b)
{
    const int d0 = (int)(a & 0xffu) - (int)(b & 0xffu), d1 = (int)((a >> 8) & 0xffu) - (int)((b >> 8) & 0xffu), d2 = (int)((a >> 16) & 0xffu) - (int)((b >> 16) & 0xffu);
    return (uint32_t)(d0 * d0 + d1 * d1 + d2 * d2);
}
// patch_ssd_masked :238-285, the whole wave together (every lane returns the value).  The reference adds d * d sequentially in f32; every addend is an integer and
// the sum only grows, so a total below 2^24 means every partial sum was below it and exact: the f32 sum IS the integer (always so for half <= 4).  Otherwise the
// sum is redone sequentially in f32 in the reference's dy, dx, channel order.
PFX_DEV float patch_ssd(const pm_geom& G, const uint32_t* img, const uint8_t* mask, const pm_query& Q, int ax, int ay, int bx, int by)
{
    const int side = 2 * G.half + 1, lane = (int)(threadIdx.x & 63u);
    uint32_t sum = 0, cnt = 0;
    for (int k = 0; k < 2; ++k) {
        if (!Q.ok[k]) continue;
        const int p = lane + 64 * k, bpx = bx + p % side - G.half, bpy = by + p / side - G.half;
        if (bpx < 0 || bpy < 0 || bpx >= G.w || bpy >= G.h) continue;
        const size_t i = (size_t)bpy * (uint32_t)G.w + (uint32_t)bpx;
        if (mask[i] > 0) continue;
        sum += sq_diff3(Q.px[k], img[i]);
        ++cnt;
    }
    sum = wave_sum(sum);
    cnt = wave_sum(cnt);
    if ((int)cnt < G.min_valid) return F32_MAX;
    if (sum < (1u << 24)) return (float)sum / (float)cnt;
    float ssd = 0.0f;   // the same on every lane
    for (int dy = -G.half; dy <= G.half; ++dy)
        for (int dx = -G.half; dx <= G.half; ++dx) {
            const int apx = ax + dx, apy = ay + dy, bpx = bx + dx, bpy = by + dy;
            if (apx < 0 || apy < 0 || apx >= G.w || apy >= G.h || bpx < 0 || bpy < 0 || bpx >= G.w || bpy >= G.h) continue;
            const size_t ia = (size_t)apy * (uint32_t)G.w + (uint32_t)apx, ib = (size_t)bpy * (uint32_t)G.w + (uint32_t)bpx;
            if (mask[ia] > 0 || mask[ib] > 0) continue;
            const uint32_t pa = img[ia], pb = img[ib];
            float d = ubyte0(pa) - ubyte0(pb);
            ssd += d * d;
            d = ubyte1(pa) - ubyte1(pb);
            ssd += d * d;
            d = ubyte2(pa) - ubyte2(pb);
            ssd += d * d;
        }
    return ssd / (float)cnt;
}

constexpr unsigned long long LCG_MUL = 6364136223846793005ull;

// random init :439-469 — one wave per boundary pixel; `sources` holds src_count linear pixel indices
__global__ __launch_bounds__(256) void pm_init_kernel(pm_geom G, const uint32_t* __restrict__ img, const uint8_t* __restrict__ mask, const uint32_t* __restrict__ boundary,
                                                      uint32_t nb, const uint32_t* __restrict__ sources, uint32_t src_count, int32_t* nnf_ox, int32_t* nnf_oy, float* nnf_ssd)
{
    const uint32_t b = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (b >= nb) return;
    const uint32_t li = __builtin_amdgcn_readfirstlane(boundary[b]);
    const int hx = (int)(li % (uint32_t)G.w), hy = (int)(li / (uint32_t)G.w);
    const pm_query Q = load_query(G, img, mask, hx, hy);
    const uint32_t seed = (uint32_t)(((unsigned long long)hx * 7919ull + (unsigned long long)hy * 6271ull) % src_count);
    uint32_t s = sources[seed];
    int sx = (int)(s % (uint32_t)G.w), sy = (int)(s / (uint32_t)G.w);
    int best_ox = sx - hx, best_oy = sy - hy;
    float best = patch_ssd(G, img, mask, Q, hx, hy, sx, sy);
    unsigned long long rng = (unsigned long long)hx * 1234567891ull + (unsigned long long)hy * 987654321ull;
    for (int k = 0; k < 4; ++k) {
        rng = rng * LCG_MUL + 1ull;
        s = sources[(uint32_t)((rng >> 33) % src_count)];
        sx = (int)(s % (uint32_t)G.w); sy = (int)(s / (uint32_t)G.w);
        const float s2 = patch_ssd(G, img, mask, Q, hx, hy, sx, sy);
        if (s2 < best) { best = s2; best_ox = sx - hx; best_oy = sy - hy; }
    }
    if ((threadIdx.x & 63u) == 0) {
        const uint32_t ni = nnf_index(G, hx, hy);
        dev_store(&nnf_ox[ni], best_ox); dev_store(&nnf_oy[ni], best_oy); dev_store(&nnf_ssd[ni], best);
    }
}

PFX_DEV float lcg_unit(unsigned long long rng) { return (float)(rng >> 33) / 4294967296.0f; }   // u32::MAX as f32 is 2^32

// patchmatch_pass :289-386 for one pixel, by one wave
PFX_DEV void pass_pixel(const pm_geom& G, const uint32_t* img, const uint8_t* mask, int32_t* nnf_ox, int32_t* nnf_oy, float* nnf_ssd, int hx, int hy, int iter)
{
    const bool forward = (iter & 1) == 0;
    const uint32_t ni = nnf_index(G, hx, hy);
    int best_ox = dev_load(&nnf_ox[ni]), best_oy = dev_load(&nnf_oy[ni]);
    float best = dev_load(&nnf_ssd[ni]);
    const pm_query Q = load_query(G, img, mask, hx, hy);
    for (int k = 0; k < 2; ++k) {   // propagation: (-1, 0), (0, -1) forward; (1, 0), (0, 1) backward
        const int step = forward ? -1 : 1, nx = hx + (k == 0 ? step : 0), ny = hy + (k == 0 ? 0 : step);
        if (nx < 0 || ny < 0 || nx >= G.w || ny >= G.h) continue;
        const uint32_t nn = nnf_index(G, nx, ny);   // inside the box plus one: the neighbour of a pixel of the box
        if (dev_load(&nnf_ssd[nn]) == F32_MAX) continue;
        const int cx = hx + dev_load(&nnf_ox[nn]), cy = hy + dev_load(&nnf_oy[nn]);
        if (cx < 0 || cy < 0 || cx >= G.w || cy >= G.h) continue;
        if (mask[(size_t)cy * (uint32_t)G.w + (uint32_t)cx] > 0) continue;
        const float ssd = patch_ssd(G, img, mask, Q, hx, hy, cx, cy);
        if (ssd < best) { best = ssd; best_ox = cx - hx; best_oy = cy - hy; }
    }
    unsigned long long rng = (unsigned long long)hx * LCG_MUL + (unsigned long long)hy * 982451653ull + (unsigned long long)iter * 1234567891ull;
    for (float search_r = G.max_radius; search_r >= 1.0f; search_r *= 0.5f) {   // each candidate is centred on the current best: a dependent chain
        rng = rng * LCG_MUL + 1442695040888963407ull;
        const float ra = lcg_unit(rng);
        rng = rng * LCG_MUL + 1442695040888963407ull;
        const float rb = lcg_unit(rng);
        const int cx = as_i32(rs_round((float)hx + (float)best_ox + (ra * 2.0f - 1.0f) * search_r));
        const int cy = as_i32(rs_round((float)hy + (float)best_oy + (rb * 2.0f - 1.0f) * search_r));
        if (cx >= 0 && cy >= 0 && cx < G.w && cy < G.h && mask[(size_t)cy * (uint32_t)G.w + (uint32_t)cx] == 0) {
            const float ssd = patch_ssd(G, img, mask, Q, hx, hy, cx, cy);
            if (ssd < best) { best = ssd; best_ox = cx - hx; best_oy = cy - hy; }
        }
    }
    if ((threadIdx.x & 63u) == 0) { dev_store(&nnf_ox[ni], best_ox); dev_store(&nnf_oy[ni], best_oy); dev_store(&nnf_ssd[ni], best); }
}

// one pass = one workgroup: the diagonals in ascending (even iter) or descending order, a block barrier between them; img and mask do not change during a pass
__global__ __launch_bounds__(1024) void pm_pass_kernel(pm_geom G, const uint32_t* __restrict__ img, const uint8_t* __restrict__ mask, const uint32_t* __restrict__ diag_start,
                                                       const uint32_t* __restrict__ diag_list, uint32_t n_diag, int iter, int32_t* nnf_ox, int32_t* nnf_oy, float* nnf_ssd)
{
    const uint32_t wave = threadIdx.x >> 6;
    for (uint32_t k = 0; k < n_diag; ++k) {
        const uint32_t d = (iter & 1) == 0 ? k : n_diag - 1u - k;
        const uint32_t lo = diag_start[d], hi = diag_start[d + 1];   // uniform over the block: an empty diagonal is skipped by all
        if (lo == hi) continue;
        for (uint32_t i = lo + wave; i < hi; i += 16u) {
            const uint32_t li = __builtin_amdgcn_readfirstlane(diag_list[i]);
            pass_pixel(G, img, mask, nnf_ox, nnf_oy, nnf_ssd, (int)(li % (uint32_t)G.w), (int)(li / (uint32_t)G.w), iter);
        }
        __syncthreads();
    }
}

// fill :490-511.  A source pixel has live mask 0 and a written pixel has it != 0, so no thread reads a pixel another writes: the reference's "gather, then
// write" order needs no second launch.  The mask is cleared by the next launch (pm_clear_kernel), after every read of it here.
__global__ __launch_bounds__(256) void pm_fill_kernel(pm_geom G, uint32_t* img, const uint8_t* __restrict__ mask, const uint32_t* __restrict__ boundary, uint32_t nb,
                                                      const int32_t* __restrict__ nnf_ox, const int32_t* __restrict__ nnf_oy, const float* __restrict__ nnf_ssd)
{
    const uint32_t b = blockIdx.x * 256u + threadIdx.x;
    if (b >= nb) return;
    const uint32_t li = boundary[b];
    const int hx = (int)(li % (uint32_t)G.w), hy = (int)(li / (uint32_t)G.w);
    const uint32_t ni = nnf_index(G, hx, hy);
    if (dev_load(&nnf_ssd[ni]) == F32_MAX) return;
    const int sx = hx + dev_load(&nnf_ox[ni]), sy = hy + dev_load(&nnf_oy[ni]);
    if (sx < 0 || sy < 0 || sx >= G.w || sy >= G.h) return;
    const size_t si = (size_t)sy * (uint32_t)G.w + (uint32_t)sx;
    if (mask[si] > 0) return;
    img[li] = img[si];
}
__global__ __launch_bounds__(256) void pm_clear_kernel(uint8_t* mask, const uint32_t* __restrict__ boundary, uint32_t nb)
{
    const uint32_t b = blockIdx.x * 256u + threadIdx.x;
    if (b < nb) mask[boundary[b]] = 0;
}
__global__ __launch_bounds__(256) void pm_fill_f32_kernel(float* p, uint32_t n, float v)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) p[i] = v;
}

pm_geom make_geom(const pfxk_pm_geom* g)
{
    pm_geom G;
    G.w = (int)g->w; G.h = (int)g->h; G.x0 = (int)g->x0; G.y0 = (int)g->y0; G.bw = (int)g->bw; G.bh = (int)g->bh;
    G.half = (int)g->half; G.min_valid = (int)g->min_valid; G.max_radius = g->max_radius;
    return G;
}
bool geom_ok(const pfxk_pm_geom* g)
{
    return g && dims_ok(g->w, g->h) && g->bw && g->bh && (uint64_t)g->x0 + g->bw <= g->w && (uint64_t)g->y0 + g->bh <= g->h &&
           g->half >= 1 && g->half <= 5;
}

} // namespace

extern "C" {

hipError_t pfxk_inpaint_instant(hipStream_t s, const uint8_t* d_src, const uint8_t* d_mask, uint8_t* d_out, uint32_t w, uint32_t h, const pfxk_inpaint_dab* d_dabs,
                                uint32_t n_dabs, const float* d_rings, uint32_t bx0, uint32_t by0, uint32_t bx1, uint32_t by1)
{
    if (n_dabs == 0 || bx1 < bx0 || by1 < by0) return hipSuccess;
    if (bx1 >= w || by1 >= h) return hipErrorInvalidValue;
    const dim3 grid((bx1 - bx0 + 64u) / 64u, (by1 - by0 + 4u) / 4u);
    inpaint_instant_kernel<<<grid, 256, 0, s>>>((const uint32_t*)d_src, d_mask, (uint32_t*)d_out, (int)w, (int)h, d_dabs, n_dabs, d_rings, bx0, by0, bx1, by1);
    return hipGetLastError();
}

hipError_t pfxk_pm_stats(hipStream_t s, const uint8_t* d_mask, uint32_t w, uint32_t h, uint32_t* d_stats)
{
    hipError_t e = hipMemsetAsync(d_stats, 0, 8 * sizeof(uint32_t), s);
    if (e) return e;
    const uint64_t n = (uint64_t)w * h;
    pm_stats_kernel<<<(uint32_t)std::min<uint64_t>((n + 2047u) / 2048u, 2048u), 256, 0, s>>>(d_mask, w, h, d_stats);
    return hipGetLastError();
}

hipError_t pfxk_pm_compact(hipStream_t s, int kind, const uint8_t* d_mask, uint32_t w, uint32_t h, uint32_t rx0, uint32_t ry0, uint32_t rw, uint32_t rh,
                           uint32_t* d_counts, uint32_t* d_total, uint32_t* d_list, int phase)
{
    if (!rw || !rh || (uint64_t)rx0 + rw > w || (uint64_t)ry0 + rh > h) return hipErrorInvalidValue;
    const uint32_t n = rw * rh, blocks = (n + 1023u) / 1024u;
    if (phase == 0) {
        if (kind == 0) pm_count_kernel<0><<<blocks, 256, 0, s>>>(d_mask, (int)w, (int)h, (int)rx0, (int)ry0, rw, n, d_counts);
        else pm_count_kernel<1><<<blocks, 256, 0, s>>>(d_mask, (int)w, (int)h, (int)rx0, (int)ry0, rw, n, d_counts);
        pm_scan_kernel<<<1, 1024, 0, s>>>(d_counts, blocks, d_total);
    } else {
        if (kind == 0) pm_scatter_kernel<0><<<blocks, 256, 0, s>>>(d_mask, (int)w, (int)h, (int)rx0, (int)ry0, rw, n, d_counts, d_list);
        else pm_scatter_kernel<1><<<blocks, 256, 0, s>>>(d_mask, (int)w, (int)h, (int)rx0, (int)ry0, rw, n, d_counts, d_list);
    }
    return hipGetLastError();
}

hipError_t pfxk_pm_nnf_reset(hipStream_t s, const pfxk_pm_geom* g, float* d_nnf_ssd)
{
    if (!geom_ok(g)) return hipErrorInvalidValue;
    const uint32_t n = (g->bw + 2u) * (g->bh + 2u);
    pm_fill_f32_kernel<<<(n + 255u) / 256u, 256, 0, s>>>(d_nnf_ssd, n, F32_MAX);
    return hipGetLastError();
}

hipError_t pfxk_pm_peel(hipStream_t s, const pfxk_pm_geom* g, uint8_t* d_img, uint8_t* d_live, const uint32_t* d_sources, uint32_t src_count, uint32_t nb,
                        int pm_iters, int32_t* d_nnf_ox, int32_t* d_nnf_oy, float* d_nnf_ssd, uint32_t* d_diag_start, uint32_t* d_cursor, uint32_t* d_diag_list)
{
    if (!geom_ok(g) || !src_count) return hipErrorInvalidValue;
    if (!nb) return hipSuccess;
    const pm_geom G = make_geom(g);
    const uint32_t* boundary = d_sources + src_count;   // this peel's boundary pixels were appended behind the sources they may copy from
    const uint32_t n_diag = g->bw + g->bh - 1u;
    pm_bucket_kernel<<<1, 1024, 0, s>>>(boundary, nb, G, n_diag, d_diag_start, d_cursor, d_diag_list);
    pm_init_kernel<<<(nb + 3u) / 4u, 256, 0, s>>>(G, (const uint32_t*)d_img, d_live, boundary, nb, d_sources, src_count, d_nnf_ox, d_nnf_oy, d_nnf_ssd);
    for (int iter = 0; iter < pm_iters; ++iter)
        pm_pass_kernel<<<1, 1024, 0, s>>>(G, (const uint32_t*)d_img, d_live, d_diag_start, d_diag_list, n_diag, iter, d_nnf_ox, d_nnf_oy, d_nnf_ssd);
    pm_fill_kernel<<<(nb + 255u) / 256u, 256, 0, s>>>(G, (uint32_t*)d_img, d_live, boundary, nb, d_nnf_ox, d_nnf_oy, d_nnf_ssd);
    pm_clear_kernel<<<(nb + 255u) / 256u, 256, 0, s>>>(d_live, boundary, nb);
    return hipGetLastError();
}

} // extern "C"
