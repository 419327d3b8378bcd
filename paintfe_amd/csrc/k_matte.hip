// k_matte.hip — background removal around the model (ref: src/ops/ai.rs), bit for bit: what runs before the model (preprocess_image :731) and behind it
// (is_probability_space :675, to_probability :693, mask_confidence_score :706, postprocess_mask :766, apply_mask_expansion :850, blur_grayscale :913).  The model
// itself is the caller's.  f32 with one rounding per written operation (no contraction), IEEE division, glibc's expf (k_libm.h), `as u8` truncating.
//
//   tensor    plane c of the [3][S][S] tensor = table[c][byte c]; the 768-entry table is the host's ((k / 255.0) - MEAN[c]) / STD[c], copied to LDS.
//   score     one pass over an output tensor: the sampled minimum / maximum (NaN-ignoring, as order-preserving integer keys) and BOTH decisive counts — the
//             values read as probabilities and as logits — reduced per wave, then integer atomics.  The host picks the count the minimum / maximum select.
//   byte      to_probability + the threshold or the sigmoid edge, four values per lane.
//   morph     apply_mask_expansion: a workgroup owns a PFXK_MATTE_TILE^2 tile, loads it with an apron of PFXK_MATTE_K cells into one of two byte planes in LDS
//             and runs up to K iterations there.  *Why the tile is right*: an iteration reads the 3 x 3 neighbourhood, so a wrong cell spoils its neighbours one
//             ring per iteration; the only wrong cells at the start are those beyond the window (held at the neutral value), so after j iterations the cells at
//             least j inside the window are still right, and the tile lies K inside.  Cells outside the IMAGE hold the neutral value (0 under max, 255 under
//             min) and are never updated, so they never act as neighbours.
//   resize    imageops::resize on one byte per sample: k_resize.hip's fused kernel with a float where that has a float4 — the same tables, the same operations
//             in the same order — so the result is channel 0 of the RGBA resize of the replicated grey; the tile shape is the matte's own (see the kernel).  The epilogue stores the byte, or multiplies it straight
//             into the document's alpha (the full-size matte is then never written unless asked for).
//   feather   blur_grayscale: the row pass takes a row segment's exclusive prefix sums in LDS (one window = one difference), the column pass slides a running
//             sum down a band of rows, lanes along x; sums are integers below 2^24, so (float)sum is exact and `(sum / count) as u8` is the reference's own
//             expression.  The alpha multiply behind a feather is the streaming kernel: riding in the column pass's store it was no faster (profiles/matte.md).
#include "k_tools.h"
#include "pfx_kernels.h"
#include "k_libm.h"

using namespace pfxk;

namespace {

// ((a / 255.0) * (m / 255.0) * 255.0).clamp(0.0, 255.0) as u8 (:839-841), left to right; div255 is the correctly rounded k / 255.0
PFX_DEV uint32_t alpha_times(uint32_t px, uint32_t m)
{
    const float a = quant255(div255((float)(px >> 24)) * div255((float)m) * 255.0f);
    return (px & 0x00ffffffu) | ((uint32_t)a << 24);
}

// ---------------------------------------------------------------------------------------------------------------- tensor
// VEC: src and out 16-byte aligned and n a multiple of 4, so that every plane starts on a 16-byte address
template <bool VEC>
__global__ __launch_bounds__(256) void tensor_kernel(const uint32_t* __restrict__ src, const float* __restrict__ table, float* __restrict__ out, size_t n)
{
    __shared__ float sT[768];
    for (uint32_t i = threadIdx.x; i < 768u; i += 256u) sT[i] = table[i];
    __syncthreads();
    float *o0 = out, *o1 = out + n, *o2 = out + 2u * n;
    stream_walk<VEC, size_t>(n, [&](size_t g) {
        const uint4 v = reinterpret_cast<const uint4*>(src)[g];
        reinterpret_cast<float4*>(o0)[g] = make_float4(sT[v.x & 0xffu], sT[v.y & 0xffu], sT[v.z & 0xffu], sT[v.w & 0xffu]);
        reinterpret_cast<float4*>(o1)[g] = make_float4(sT[256u + ((v.x >> 8) & 0xffu)], sT[256u + ((v.y >> 8) & 0xffu)], sT[256u + ((v.z >> 8) & 0xffu)],
                                                       sT[256u + ((v.w >> 8) & 0xffu)]);
        reinterpret_cast<float4*>(o2)[g] = make_float4(sT[512u + ((v.x >> 16) & 0xffu)], sT[512u + ((v.y >> 16) & 0xffu)], sT[512u + ((v.z >> 16) & 0xffu)],
                                                       sT[512u + ((v.w >> 16) & 0xffu)]);
    }, [&](size_t i) {
        const uint32_t p = src[i];
        o0[i] = sT[p & 0xffu];
        o1[i] = sT[256u + ((p >> 8) & 0xffu)];
        o2[i] = sT[512u + ((p >> 16) & 0xffu)];
    });
}

// ---------------------------------------------------------------------------------------------------------------- probabilities, score, byte
// to_probability :693: clamp keeps a NaN, the sigmoid propagates it
PFX_DEV float to_prob(float v, bool is_prob) { return is_prob ? rs_clamp(v, 0.0f, 1.0f) : 1.0f / (1.0f + libm_exp(-v)); }
// !(0.1..=0.9).contains(&(prob as f64)) :715: the f64 literals; a NaN is decisive
PFX_DEV uint32_t decisive(float prob)
{
    const double q = (double)prob;
    return (q >= 0.1 && q <= 0.9) ? 0u : 1u;
}

#define PFXK_MATTE_KEY_MAX 0xff7fffffu   /* PFXK_MATTE_KEY of FLT_MAX */
#define PFXK_MATTE_KEY_MIN 0x00800000u   /* PFXK_MATTE_KEY of -FLT_MAX */
__global__ void score_init_kernel(uint32_t* out)
{
    if (threadIdx.x == 0) { out[0] = PFXK_MATTE_KEY_MAX; out[1] = PFXK_MATTE_KEY_MIN; out[2] = 0u; out[3] = 0u; }
}

__global__ __launch_bounds__(256) void score_kernel(const float* __restrict__ v, uint32_t n, uint32_t step, uint32_t n_samples, uint32_t* out)
{
    const uint32_t first = blockIdx.x * 256u + threadIdx.x, stride = gridDim.x * 256u;
    uint32_t mn = PFXK_MATTE_KEY_MAX, mx = PFXK_MATTE_KEY_MIN, as_prob = 0u, as_logit = 0u;
    for (uint32_t k = first; k < n_samples; k += stride) {   // f32::min / max ignore a NaN (:684-685)
        const float x = v[(size_t)k * step];
        if (x == x) {
            const uint32_t bits = __builtin_bit_cast(uint32_t, x), key = PFXK_MATTE_KEY(bits);
            mn = umin(mn, key);
            mx = umax(mx, key);
        }
    }
    for (uint32_t i = first; i < n; i += stride) {   // n is at most 256 000 000 and the stride at most 2^21: i does not wrap
        const float x = v[i];
        as_prob += decisive(to_prob(x, true));
        as_logit += decisive(to_prob(x, false));
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        mn = umin(mn, (uint32_t)__shfl_xor((int)mn, off));
        mx = umax(mx, (uint32_t)__shfl_xor((int)mx, off));
        as_prob += (uint32_t)__shfl_xor((int)as_prob, off);
        as_logit += (uint32_t)__shfl_xor((int)as_logit, off);
    }
    if ((threadIdx.x & 63u) == 0u) {   // integer minimum, maximum and sums: the order of arrival does not show
        if (mn != PFXK_MATTE_KEY_MAX) atomicMin(&out[0], mn);
        if (mx != PFXK_MATTE_KEY_MIN) atomicMax(&out[1], mx);
        if (as_prob) atomicAdd(&out[2], as_prob);
        if (as_logit) atomicAdd(&out[3], as_logit);
    }
}

// postprocess_mask's first step :776-794
PFX_DEV uint32_t byte_of(float v, bool is_prob, bool smooth, float threshold)
{
    const float p = to_prob(v, is_prob);
    if (smooth) {
        const float remapped = 1.0f / (1.0f + libm_exp(-(p - threshold) * 12.0f));
        return (uint32_t)quant255(remapped * 255.0f);   // truncates; NaN -> 0
    }
    return p >= threshold ? 255u : 0u;
}

// VEC: values 16-byte, grey 4-byte aligned
template <bool VEC>
__global__ __launch_bounds__(256) void byte_kernel(const float* __restrict__ v, uint8_t* __restrict__ grey, size_t n, int is_prob, int smooth, float threshold)
{
    stream_walk<VEC, size_t>(n, [&](size_t g) {
        const float4 x = reinterpret_cast<const float4*>(v)[g];
        reinterpret_cast<uint32_t*>(grey)[g] = byte_of(x.x, is_prob, smooth, threshold) | (byte_of(x.y, is_prob, smooth, threshold) << 8) |
                                               (byte_of(x.z, is_prob, smooth, threshold) << 16) | (byte_of(x.w, is_prob, smooth, threshold) << 24);
    }, [&](size_t i) { grey[i] = (uint8_t)byte_of(v[i], is_prob, smooth, threshold); });
}

// ---------------------------------------------------------------------------------------------------------------- morphology
constexpr int MT = PFXK_MATTE_TILE, MK = PFXK_MATTE_K, MW = MT + 2 * MK + 2;   // the window: tile + apron + one ring of neutral cells, so no neighbour read leaves it

__global__ __launch_bounds__(256) void morph_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int w, int h, int tiles_x, int iters, int dilate)
{
    __shared__ uint8_t sA[MW * MW], sB[MW * MW];
    const int ox = (int)(blockIdx.x % (uint32_t)tiles_x) * MT - MK - 1, oy = (int)(blockIdx.x / (uint32_t)tiles_x) * MT - MK - 1;   // the image position of cell (0, 0)
    const uint8_t neutral = dilate ? 0u : 255u;
    // a cell that is updated: inside the ring and inside the image.  Every other cell keeps the neutral value in both planes
    auto live = [&](int lx, int ly) { return lx > 0 && lx < MW - 1 && ly > 0 && ly < MW - 1 && ox + lx >= 0 && ox + lx < w && oy + ly >= 0 && oy + ly < h; };
    for (int c = (int)threadIdx.x; c < MW * MW; c += 256) {
        const int ly = c / MW, lx = c - ly * MW;
        const uint8_t v = live(lx, ly) ? src[(size_t)(oy + ly) * w + (ox + lx)] : neutral;
        sA[c] = v;
        sB[c] = v;
    }
    __syncthreads();
    uint8_t *cur = sA, *nxt = sB;
    for (int it = 0; it < iters; ++it) {
        for (int c = (int)threadIdx.x; c < MW * MW; c += 256) {
            const int ly = c / MW, lx = c - ly * MW;
            if (!live(lx, ly)) continue;
            const uint32_t centre = cur[c];
            uint32_t out = centre;
            if (dilate ? centre < 128u : centre > 128u) {   // :862, :878: a centre of 128 never changes, one that has crossed it is frozen
#pragma unroll
                for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                    for (int dx = -1; dx <= 1; ++dx) {
                        const uint32_t q = cur[c + dy * MW + dx];
                        out = dilate ? umax(out, q) : umin(out, q);
                    }
            }
            nxt[c] = (uint8_t)out;
        }
        __syncthreads();
        uint8_t* t = cur; cur = nxt; nxt = t;
    }
    for (int c = (int)threadIdx.x; c < MT * MT; c += 256) {
        const int ly = c / MT + MK + 1, lx = c % MT + MK + 1;
        if (ox + lx < w && oy + ly < h) dst[(size_t)(oy + ly) * w + (ox + lx)] = cur[ly * MW + lx];
    }
}

// ---------------------------------------------------------------------------------------------------------------- one-channel resize
constexpr int MZ_TOX = PFXK_MATTE_RZ_TOX;

// k_resize.hip: resize_fused_kernel on one byte per sample.  A block owns MZ_TOX x TOY output samples: the vertical pass for the source columns its horizontal
// taps reach into an f32 tile in LDS, then the horizontal pass out of it with clamp and round half away from zero.  `t += v * w` in source order, one rounding
// per operation: the same operations in the same order as the RGBA kernel.  Two things differ from its shape, for the matte's usual case — a small model output
// onto a large document, where a 64-column tile reaches some 15 source columns and every output has at most 8 taps:
//   * the vertical pass deals (row, source column) pairs to the lanes, so a narrow span still fills the waves (bounds and weights are then per lane);
//   * the tile is TOY = 32 rows tall where its span fits (PFXK_MATTE_RZ_TALL_SPAN), a lane keeps its column across the tile's rows, and a column of at most 8
//     taps holds its weights in registers: they are read once per tile and not once per output.
// APPLY: image and result may be the same buffer (a lane reads the pixel it writes)
template <bool APPLY, int TOY>
__global__ __launch_bounds__(256) void matte_resize_kernel(const uint8_t* __restrict__ src, const uint32_t* __restrict__ v_left, const uint32_t* __restrict__ v_count,
                                                           const uint32_t* __restrict__ v_off, const float* __restrict__ v_wts, const uint32_t* __restrict__ h_left,
                                                           const uint32_t* __restrict__ h_count, const uint32_t* __restrict__ h_off, const float* __restrict__ h_wts,
                                                           int w, int nw, int nh, int span_max, uint8_t* __restrict__ matte, const uint32_t* image, uint32_t* result)
{
    extern __shared__ float mz_tile[]; // [TOY][span_max]
    const int ox0 = blockIdx.x * MZ_TOX, oy0 = blockIdx.y * TOY, ox_last = min(ox0 + MZ_TOX, nw) - 1;
    const int L = (int)h_left[ox0], span = (int)(h_left[ox_last] + h_count[ox_last]) - L, rows = min(TOY, nh - oy0);
    for (int item = (int)threadIdx.x; item < rows * span; item += 256) {
        const int ry = item / span, xs = item - ry * span, oy = oy0 + ry;
        const uint32_t l = v_left[oy], n = v_count[oy];
        const float* wp = v_wts + v_off[oy];
        const uint8_t* p = src + (size_t)l * w + L + xs;
        float t = 0.f;
        for (uint32_t i = 0; i < n; i += 4) {   // taps four at a time from clamped (always valid) indices; the guard is a select per tap
            uint32_t v[4]; float wt[4];
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) { const uint32_t j = min(i + k, n - 1u); v[k] = p[(size_t)j * w]; wt[k] = wp[j]; }
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k)
                if (i + k < n) t += (float)v[k] * wt[k];
        }
        mz_tile[ry * span_max + xs] = t;
    }
    __syncthreads();
    const int ox = ox0 + (int)(threadIdx.x & 63u), wv = (int)(threadIdx.x >> 6);
    if (ox >= nw) return;
    const uint32_t n = h_count[ox];
    const float* wp = h_wts + h_off[ox];
    const int first = (int)h_left[ox] - L;
    float wr[8];
#pragma unroll
    for (uint32_t q = 0; q < 8; ++q) wr[q] = wp[min(q, n - 1u)];
    for (int ry = wv; ry < rows; ry += 4) {
        const float* p = mz_tile + ry * span_max + first;
        float t = 0.f;
        if (n <= 8u) {
            float v[8];
#pragma unroll
            for (uint32_t q = 0; q < 8; ++q) v[q] = p[min(q, n - 1u)];
#pragma unroll
            for (uint32_t q = 0; q < 8; ++q)
                if (q < n) t += v[q] * wr[q];
        } else {
            for (uint32_t i = 0; i < n; i += 4) {
                float v[4], wt[4];
#pragma unroll
                for (uint32_t q = 0; q < 4; ++q) { const uint32_t j = min(i + q, n - 1u); v[q] = p[j]; wt[q] = wp[j]; }
#pragma unroll
                for (uint32_t q = 0; q < 4; ++q)
                    if (i + q < n) t += v[q] * wt[q];
            }
        }
        const uint32_t m = (uint32_t)round_u8f(t);   // NumCast::from(FloatNearest(clamp(t, 0, 255))): round half away from zero
        const size_t at = (size_t)(oy0 + ry) * nw + ox;
        if (matte) matte[at] = (uint8_t)m;
        if constexpr (APPLY) result[at] = alpha_times(image[at], m);
    }
}

// ---------------------------------------------------------------------------------------------------------------- feather
constexpr int BOXC = PFXK_MATTE_BOX_CHUNK, BOXR = PFXK_MATTE_MAX_FEATHER, BOXN = BOXC + 2 * BOXR;

// the row pass: a workgroup owns up to BOXC outputs of one row.  s[i] = the row's sample at clamp(x0 - r + i), i < N = cols + 2 r; P = its exclusive prefix sums
// (N + 1 entries); output j = (P[j + 2 r + 1] - P[j]) / (2 r + 1).  A lane sums a segment of E consecutive samples, the 256 segment totals are scanned in LDS
__global__ __launch_bounds__(256) void box_h_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int w, int r, int chunks_x)
{
    __shared__ uint32_t sP[BOXN + 1];
    __shared__ uint32_t sPart[256];
    const int y = (int)(blockIdx.x / (uint32_t)chunks_x), x0 = (int)(blockIdx.x % (uint32_t)chunks_x) * BOXC, cols = min(BOXC, w - x0), N = cols + 2 * r;
    const uint8_t* row = src + (size_t)y * w;
    const int E = (N + 255) / 256, b = min((int)threadIdx.x * E, N), e = min(b + E, N);
    uint32_t sum = 0u;
    for (int i = b; i < e; ++i) {
        sum += row[min(max(x0 - r + i, 0), w - 1)];
        sP[i + 1] = sum;
    }
    sPart[threadIdx.x] = sum;
    __syncthreads();
    for (uint32_t off = 1u; off < 256u; off <<= 1) {
        const uint32_t add = threadIdx.x >= off ? sPart[threadIdx.x - off] : 0u;
        __syncthreads();
        sPart[threadIdx.x] += add;
        __syncthreads();
    }
    const uint32_t base = threadIdx.x ? sPart[threadIdx.x - 1u] : 0u;
    for (int i = b; i < e; ++i) sP[i + 1] += base;
    if (threadIdx.x == 0u) sP[0] = 0u;
    __syncthreads();
    const rdiv count = rdiv_prepare((float)(2 * r + 1));   // the correctly rounded quotient of two exact f32 values, then `as u8`: the reference's expression
    for (int j = (int)threadIdx.x; j < cols; j += 256) dst[(size_t)y * w + x0 + j] = (uint8_t)(uint32_t)rdiv_apply(count, (float)(sP[j + 2 * r + 1] - sP[j]));
}

// the column pass: a lane owns a column of a band of rows and slides the window's integer sum down it
__global__ __launch_bounds__(PFXK_MATTE_BOX_COLS) void box_v_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int w, int h, int r, int band, int strips_x)
{
    const int x = (int)(blockIdx.x % (uint32_t)strips_x) * PFXK_MATTE_BOX_COLS + (int)threadIdx.x, y0 = (int)(blockIdx.x / (uint32_t)strips_x) * band;
    const int y1 = min(y0 + band, h);
    if (x >= w) return;
    const uint8_t* col = src + x;
    auto at = [&](int y) { return (uint32_t)col[(size_t)min(max(y, 0), h - 1) * w]; };
    uint32_t sum = 0u;
    for (int dy = -r; dy <= r; ++dy) sum += at(y0 + dy);
    const rdiv count = rdiv_prepare((float)(2 * r + 1));
    for (int y = y0;;) {
        dst[(size_t)y * w + x] = (uint8_t)(uint32_t)rdiv_apply(count, (float)sum);
        if (++y >= y1) break;
        sum += at(y + r);
        sum -= at(y - 1 - r);
    }
}

// ---------------------------------------------------------------------------------------------------------------- apply
// VEC: image and result 16-byte, matte 4-byte aligned.  result may be image: a lane reads the pixels it writes before it writes them
template <bool VEC>
__global__ __launch_bounds__(256) void apply_kernel(const uint32_t* image, const uint8_t* __restrict__ matte, uint32_t* result, size_t n)
{
    stream_walk<VEC, size_t>(n, [&](size_t g) {
        const uint4 v = reinterpret_cast<const uint4*>(image)[g];
        const uint32_t m = reinterpret_cast<const uint32_t*>(matte)[g];
        reinterpret_cast<uint4*>(result)[g] = make_uint4(alpha_times(v.x, m & 0xffu), alpha_times(v.y, (m >> 8) & 0xffu), alpha_times(v.z, (m >> 16) & 0xffu),
                                                         alpha_times(v.w, m >> 24));
    }, [&](size_t i) { result[i] = alpha_times(image[i], matte[i]); });
}

} // namespace

extern "C" hipError_t pfxk_matte_tensor(hipStream_t s, const uint8_t* d_rgba, const float* d_table, float* d_tensor, size_t n)
{
    if (n == 0) return hipSuccess;
    return launch_stream(aligned_to(d_rgba, 16) && aligned_to(d_tensor, 16) && n % 4u == 0u, n, s, tensor_kernel<true>, tensor_kernel<false>, (const uint32_t*)d_rgba,
                         d_table, d_tensor, n);
}

extern "C" hipError_t pfxk_matte_score(hipStream_t s, const float* d_values, uint32_t n, uint32_t step, uint32_t* d_out)
{
    score_init_kernel<<<1, 64, 0, s>>>(d_out);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || n == 0 || step == 0) return e;
    const uint32_t n_samples = (n + step - 1u) / step;
    score_kernel<<<std::min<uint32_t>(stream_blocks(n), 2048u), 256, 0, s>>>(d_values, n, step, n_samples, d_out);
    return hipGetLastError();
}

extern "C" hipError_t pfxk_matte_byte(hipStream_t s, const float* d_values, uint8_t* d_grey, size_t n, int is_prob, int smooth, float threshold)
{
    if (n == 0) return hipSuccess;
    return launch_stream(aligned_to(d_values, 16) && aligned_to(d_grey, 4), n, s, byte_kernel<true>, byte_kernel<false>, d_values, d_grey, n, is_prob, smooth, threshold);
}

extern "C" hipError_t pfxk_matte_morph(hipStream_t s, const uint8_t* d_src, uint8_t* d_dst, uint32_t w, uint32_t h, uint32_t iters, int dilate)
{
    if (!dims_ok(w, h) || iters == 0 || iters > (uint32_t)MK) return hipErrorInvalidValue;
    uint32_t tiles_x;
    const uint32_t tiles = tile_grid<MT, MT>(w, h, &tiles_x);
    if (tiles == 0) return hipErrorInvalidValue;
    morph_kernel<<<tiles, 256, 0, s>>>(d_src, d_dst, (int)w, (int)h, (int)tiles_x, (int)iters, dilate);
    return hipGetLastError();
}

template <bool APPLY, int TOY>
hipError_t launch_matte_resize(hipStream_t s, const uint8_t* d_grey, const uint32_t* v_left, const uint32_t* v_count, const uint32_t* v_off, const float* v_wts,
                               const uint32_t* h_left, const uint32_t* h_count, const uint32_t* h_off, const float* h_wts, uint32_t w, uint32_t nw, uint32_t nh,
                               uint32_t span_max, uint8_t* d_matte, const uint8_t* d_image, uint8_t* d_result)
{
    const size_t lds = (size_t)span_max * TOY * sizeof(float);
    hipError_t e = grant_lds_for((const void*)matte_resize_kernel<APPLY, TOY>, lds);
    if (e) return e;
    matte_resize_kernel<APPLY, TOY><<<dim3((nw + MZ_TOX - 1) / MZ_TOX, (nh + TOY - 1) / TOY), 256, lds, s>>>(
        d_grey, v_left, v_count, v_off, v_wts, h_left, h_count, h_off, h_wts, (int)w, (int)nw, (int)nh, (int)span_max, d_matte, (const uint32_t*)d_image, (uint32_t*)d_result);
    return hipGetLastError();
}

extern "C" hipError_t pfxk_matte_resize(hipStream_t s, const uint8_t* d_grey, const uint32_t* v_left, const uint32_t* v_count, const uint32_t* v_off, const float* v_wts,
                                        const uint32_t* h_left, const uint32_t* h_count, const uint32_t* h_off, const float* h_wts, uint32_t w, uint32_t nw, uint32_t nh,
                                        uint32_t span_max, uint8_t* d_matte, const uint8_t* d_image, uint8_t* d_result)
{
    if (w == 0 || !dims_ok(nw, nh) || span_max == 0 || span_max > PFXK_MATTE_RZ_MAX_SPAN) return hipErrorInvalidValue;
    const bool tall = span_max <= PFXK_MATTE_RZ_TALL_SPAN;   // both tile heights: at most 64 KiB of LDS
#define PFXK_MATTE_RZ_GO(APPLY, TOY) \
    launch_matte_resize<APPLY, TOY>(s, d_grey, v_left, v_count, v_off, v_wts, h_left, h_count, h_off, h_wts, w, nw, nh, span_max, d_matte, d_image, d_result)
    if (d_image) return tall ? PFXK_MATTE_RZ_GO(true, PFXK_MATTE_RZ_TOY) : PFXK_MATTE_RZ_GO(true, PFXK_MATTE_RZ_TOY_WIDE);
    return tall ? PFXK_MATTE_RZ_GO(false, PFXK_MATTE_RZ_TOY) : PFXK_MATTE_RZ_GO(false, PFXK_MATTE_RZ_TOY_WIDE);
#undef PFXK_MATTE_RZ_GO
}

extern "C" hipError_t pfxk_matte_box_h(hipStream_t s, const uint8_t* d_src, uint8_t* d_dst, uint32_t w, uint32_t h, uint32_t r)
{
    if (!dims_ok(w, h) || r == 0 || r > (uint32_t)BOXR) return hipErrorInvalidValue;
    const uint32_t chunks_x = (w + BOXC - 1u) / BOXC;
    const uint64_t blocks = (uint64_t)chunks_x * h;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    box_h_kernel<<<(uint32_t)blocks, 256, 0, s>>>(d_src, d_dst, (int)w, (int)r, (int)chunks_x);
    return hipGetLastError();
}

extern "C" hipError_t pfxk_matte_box_v(hipStream_t s, const uint8_t* d_src, uint8_t* d_dst, uint32_t w, uint32_t h, uint32_t r, uint32_t band)
{
    if (!dims_ok(w, h) || r == 0 || r > (uint32_t)BOXR || band == 0) return hipErrorInvalidValue;
    const uint32_t strips_x = (w + PFXK_MATTE_BOX_COLS - 1u) / PFXK_MATTE_BOX_COLS;
    const uint64_t blocks = (uint64_t)strips_x * ((h + band - 1u) / band);
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    box_v_kernel<<<(uint32_t)blocks, PFXK_MATTE_BOX_COLS, 0, s>>>(d_src, d_dst, (int)w, (int)h, (int)r, (int)band, (int)strips_x);
    return hipGetLastError();
}

extern "C" hipError_t pfxk_matte_apply(hipStream_t s, const uint8_t* d_image, const uint8_t* d_matte, uint8_t* d_result, size_t n)
{
    if (n == 0) return hipSuccess;
    return launch_stream(aligned_to(d_image, 16) && aligned_to(d_result, 16) && aligned_to(d_matte, 4), n, s, apply_kernel<true>, apply_kernel<false>,
                         (const uint32_t*)d_image, d_matte, (uint32_t*)d_result, n);
}
