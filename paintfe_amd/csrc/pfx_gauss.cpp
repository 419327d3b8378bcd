// pfx_gauss.cpp — everything the host knows about the Gaussian: the two tap-table caches, the ONE decision which kernel runs for a call and
// what rides in its store (pfx_int_gauss_path), and the launches with their timers.  The entry points (pfx_api.cpp, pfx_effects.cpp) check
// arguments, own their buffers and call in here; a new Gaussian kernel is a change to this file and its .hip file.
#include <algorithm>
#include <vector>

#include "pfx_internal.h"

// Which path a call takes: a pure function of the case (no HIP call, no context).  `exact` is the effective mode, an argument: plain blurs pass
// ctx->exact, the composite effects ctx->exact || !ctx->gauss_fast_effects (pfx_internal.h).
int pfx_int_gauss_path(const pfx_gauss_case* cp)
{
    const pfx_gauss_case& c = *cp;
    if (c.radius > pfxk_gauss_max_radius()) return PFX_GAUSS_UNSUPPORTED;
    const bool mfma_r = c.radius >= 1 && c.radius <= pfxk_gauss_mfma_max_radius();
    const bool fused_r = c.fused_enabled && c.radius >= 1 && c.radius <= pfxk_gauss_fused_exact_max_radius();
    switch (c.ride) {
    case PFX_GAUSS_SHARPEN: case PFX_GAUSS_GLOW:   // the combine reads src beside the blurred value: only on buffers that share no byte
        if (c.exact && fused_r && !c.overlap) return PFX_GAUSS_FUSED_RIDE;
        break;
    case PFX_GAUSS_CHAIN:   // pfx_chain_dev refuses a blur in place, so src != dst here; `heavy`: see there
        if (c.heavy && !c.fuse_heavy) break;
        if (c.exact && fused_r) return PFX_GAUSS_FUSED_RIDE;
        if (!c.exact && mfma_r && c.n_luts == 0 && c.chain_mfma) return PFX_GAUSS_MFMA_RIDE;   // table-free ops only
        break;
    case PFX_GAUSS_PLANE:
        // Keyed on the gauss_fast_effects knob, not on `exact` like sharpen / glow: with gauss_fast_effects = 1 on an exact context the shadow blurs its RGBA
        // image (bit-exact all the same) where sharpen / glow still fuse.  Kept as it was; radius 0 = no blur, the plane layout alone.
        if ((c.w & 3u) == 0 && c.shadow_plane && !c.fast_effects && (c.radius == 0 || fused_r)) return PFX_GAUSS_PLANE_FUSED;
        break;
    }
    // the blur alone; a rider that stayed behind gets a launch of its own.  Sharpen / glow / shadow then blur into scratch of the context: never in place
    const bool in_place = c.same && (c.ride == PFX_GAUSS_PLAIN || c.ride == PFX_GAUSS_CHAIN);
    if (!c.exact && mfma_r && !in_place) return PFX_GAUSS_MFMA;    // fused H+V on the matrix cores, no intermediate in HBM, no scratch (k_gauss.hip:gauss_strip_kernel)
    if (c.exact && fused_r && !in_place) return PFX_GAUSS_FUSED;   // both passes in one kernel, no f32 intermediate in HBM (k_gauss_exact.hip)
    return PFX_GAUSS_TWO_PASS;                                     // in place, radius 0, large radii: gauss_h / gauss_v through w * h * 16 bytes
}

namespace {

pfx_gauss_case case_of(const pfx_ctx* ctx, bool exact, int radius, const void* src, const void* dst, uint32_t w, uint32_t h, int ride)
{
    const size_t bytes = (size_t)w * h * 4;
    pfx_gauss_case c{};
    c.exact = exact; c.radius = radius; c.same = src == dst; c.overlap = pfx_ranges_overlap(src, bytes, dst, bytes); c.ride = ride;
    c.chain_mfma = ctx->chain_mfma_epilogue; c.fuse_heavy = ctx->chain_fuse_heavy; c.w = w; c.shadow_plane = ctx->shadow_plane_blur; c.fast_effects = ctx->gauss_fast_effects;
    c.fused_enabled = pfxk_gauss_fused_exact_enabled();
    return c;
}

int unsupported(pfx_ctx* ctx, int radius) { return pfx_fail(ctx, PFX_ERR_UNSUPPORTED, "gaussian radius %d beyond the device tile limit %d", radius, pfxk_gauss_max_radius()); }

inline uint32_t bits_of(float v) { uint32_t b; std::memcpy(&b, &v, 4); return b; }
inline int cus_of(const pfx_ctx* ctx) { return ctx->n_cus > 0 ? ctx->n_cus : 256; }

// the f32 taps of sigma on the device (cached per context): *wts points at tap 0, pfxk_gauss_weight_pad() zero taps on both sides (the kernels' register
// blocking reads past the ends)
int f32_taps(pfx_ctx* ctx, float sigma, const float** wts)
{
    const int pad = pfxk_gauss_weight_pad();
    if (!ctx->wts_valid || ctx->wts_sigma_bits != bits_of(sigma)) {
        std::vector<float> k; pfx_host_gaussian_kernel(sigma, k);
        std::vector<float> padded(k.size() + 2 * (size_t)pad, 0.0f);
        std::copy(k.begin(), k.end(), padded.begin() + pad);
        PFX_TRY(pfx_reserve(ctx, ctx->d_wts, padded.size() * sizeof(float)));
        PFX_TRY(pfx_h2d(ctx, ctx->d_wts.p, padded.data(), padded.size() * sizeof(float)));
        ctx->wts_sigma_bits = bits_of(sigma); ctx->wts_valid = true;
    }
    *wts = (const float*)ctx->d_wts.p + pad;
    return PFX_OK;
}

// the matrix-core Gaussian's f16 tap tables for sigma on the device (cached per context)
int f16_tables(pfx_ctx* ctx, float sigma)
{
    if (!ctx->wsplit_valid || ctx->wsplit_sigma_bits != bits_of(sigma)) {
        std::vector<float> k; pfx_host_gaussian_kernel(sigma, k);
        std::vector<uint16_t> ws;
        ctx->wsplit_inv_scale = pfx_host_gaussian_split_f16(k, pfxk_gauss_mfma_wlen(), pfxk_gauss_mfma_woff(), ws, &ctx->wsplit_bias, &ctx->wsplit_bias_single);
        PFX_TRY(pfx_reserve(ctx, ctx->d_wsplit, ws.size() * sizeof(uint16_t)));
        PFX_TRY(pfx_h2d(ctx, ctx->d_wsplit.p, ws.data(), ws.size() * sizeof(uint16_t)));
        ctx->wsplit_sigma_bits = bits_of(sigma); ctx->wsplit_valid = true;
    }
    return PFX_OK;
}

// the blur alone on `path` (PFX_GAUSS_MFMA, _FUSED or _TWO_PASS); tmp_dev == NULL: the two passes go through st_tmp
int run_blur(pfx_ctx* ctx, int path, bool exact, const void* src_dev, void* dst_dev, uint32_t w, uint32_t h, float sigma, int radius, void* tmp_dev, uint32_t first_row)
{
    if (path == PFX_GAUSS_MFMA) {
        PFX_TRY(f16_tables(ctx, sigma));
        pfx_timer t(ctx, "gauss_mfma");
        PFX_HIP(ctx, pfxk_gauss_mfma(ctx->stream, (const uint8_t*)src_dev, (uint8_t*)dst_dev, (const uint16_t*)ctx->d_wsplit.p, radius, ctx->wsplit_inv_scale, ctx->wsplit_bias, ctx->wsplit_bias_single, w, h, first_row, cus_of(ctx)));
        return PFX_OK;
    }
    const float* wts = nullptr; PFX_TRY(f32_taps(ctx, sigma, &wts));
    if (path == PFX_GAUSS_FUSED) {
        pfx_timer t(ctx, "gauss_fused");
        PFX_HIP(ctx, pfxk_gauss_fused_exact(ctx->stream, (const uint8_t*)src_dev, (uint8_t*)dst_dev, wts, radius, w, h, 0, 0.0f, nullptr));
        return PFX_OK;
    }
    if (!tmp_dev) { PFX_TRY(pfx_reserve(ctx, ctx->st_tmp, (size_t)w * h * 16)); tmp_dev = ctx->st_tmp.p; }
    { pfx_timer t(ctx, "gauss_h"); PFX_HIP(ctx, pfxk_gauss_h(ctx->stream, (const uint8_t*)src_dev, (float*)tmp_dev, wts, radius, w, h, exact ? 1 : 0)); }
    { pfx_timer t(ctx, "gauss_v"); PFX_HIP(ctx, pfxk_gauss_v(ctx->stream, (const float*)tmp_dev, (uint8_t*)dst_dev, wts, radius, w, h, exact ? 1 : 0)); }
    return PFX_OK;
}

} // namespace

int pfx_gauss_blur(pfx_ctx* ctx, bool exact, const void* src_dev, void* dst_dev, uint32_t w, uint32_t h, float sigma, void* tmp_dev, uint32_t first_row)
{
    // radius first: a huge sigma must be refused before a tap array of that size is built (the C ABI must not throw)
    const int radius = pfx_host_gaussian_radius(sigma);
    const pfx_gauss_case c = case_of(ctx, exact, radius, src_dev, dst_dev, w, h, PFX_GAUSS_PLAIN);
    const int path = pfx_int_gauss_path(&c);
    if (path == PFX_GAUSS_UNSUPPORTED) return unsupported(ctx, radius);
    return run_blur(ctx, path, exact, src_dev, dst_dev, w, h, sigma, radius, tmp_dev, first_row);
}

// sharpen / glow (stylize.rs: `blurred = parallel_gaussian_blur_pub(flat, radius)`, then the two-input pass): the Gaussian and the combine in one kernel where
// the bit-exact fused Gaussian applies — the blurred image never exists in memory — else the Gaussian into st_aux2 and pfxk_combine
int pfx_gauss_combine(pfx_ctx* ctx, bool exact, const void* src_dev, void* dst_dev, uint32_t w, uint32_t h, float sigma, int ride, float p0, const void* mask_dev, const char* timer)
{
    const int radius = pfx_host_gaussian_radius(sigma);
    const pfx_gauss_case c = case_of(ctx, exact, radius, src_dev, dst_dev, w, h, ride);
    const int path = pfx_int_gauss_path(&c);
    if (path == PFX_GAUSS_UNSUPPORTED) return unsupported(ctx, radius);
    if (path == PFX_GAUSS_FUSED_RIDE) {   // PFX_GAUSS_SHARPEN / _GLOW are the kernel's epilogue ids
        pfx_timer t(ctx, timer);
        const float* wts = nullptr; PFX_TRY(f32_taps(ctx, sigma, &wts));
        PFX_HIP(ctx, pfxk_gauss_fused_exact(ctx->stream, (const uint8_t*)src_dev, (uint8_t*)dst_dev, wts, radius, w, h, ride, p0, (const uint8_t*)mask_dev));
        return PFX_OK;
    }
    PFX_TRY(pfx_reserve(ctx, ctx->st_aux2, (size_t)w * h * 4));
    PFX_TRY(run_blur(ctx, path, exact, src_dev, ctx->st_aux2.p, w, h, sigma, radius, nullptr, 0));
    pfx_timer t(ctx, timer);
    PFX_HIP(ctx, pfxk_combine(ctx->stream, (const uint8_t*)src_dev, (const uint8_t*)ctx->st_aux2.p, (const uint8_t*)mask_dev, (uint8_t*)dst_dev, w, h,
                              ride == PFX_GAUSS_SHARPEN ? PFXK_FX_SHARPEN : PFXK_FX_GLOW, p0));
    return PFX_OK;
}

// a Gaussian in front of the pointwise run C of a chain (C == NULL: no run).  *rode: C went out in the Gaussian's store; otherwise dst holds the blur and the
// caller runs C over it
int pfx_gauss_chain(pfx_ctx* ctx, bool exact, const void* src_dev, void* dst_dev, uint32_t w, uint32_t h, float sigma, const pfxk_chain* C, bool heavy, bool* rode)
{
    *rode = false;
    const int radius = pfx_host_gaussian_radius(sigma);
    pfx_gauss_case c = case_of(ctx, exact, radius, src_dev, dst_dev, w, h, C ? PFX_GAUSS_CHAIN : PFX_GAUSS_PLAIN);
    c.n_luts = C ? C->n_luts : 0; c.heavy = heavy;
    int path = pfx_int_gauss_path(&c);
    if (path == PFX_GAUSS_UNSUPPORTED) return unsupported(ctx, radius);
    if (path == PFX_GAUSS_FUSED_RIDE) {
        const float* wts = nullptr; PFX_TRY(f32_taps(ctx, sigma, &wts));
        pfx_timer t(ctx, "gauss_fused_chain");
        PFX_HIP(ctx, pfxk_gauss_fused_exact_chain(ctx->stream, (const uint8_t*)src_dev, (uint8_t*)dst_dev, wts, radius, w, h, C, (const uint8_t*)ctx->d_chain_luts.p));
        *rode = true;
        return PFX_OK;
    }
    if (path == PFX_GAUSS_MFMA_RIDE) {   // aligned buffers only: the kernel file says hipErrorNotSupported otherwise, and the two launches run
        PFX_TRY(f16_tables(ctx, sigma));
        pfx_timer t(ctx, "gauss_mfma_chain");
        const hipError_t e = pfxk_gauss_mfma_chain(ctx->stream, (const uint8_t*)src_dev, (uint8_t*)dst_dev, (const uint16_t*)ctx->d_wsplit.p, radius, ctx->wsplit_inv_scale,
                                                   ctx->wsplit_bias, ctx->wsplit_bias_single, w, h, 0u, cus_of(ctx), C);
        if (e == hipSuccess) { *rode = true; return PFX_OK; }
        if (e != hipErrorNotSupported) PFX_HIP(ctx, e);
        (void)hipGetLastError();   // the refusal must not stay behind as the runtime's sticky error
        c.ride = PFX_GAUSS_PLAIN; path = pfx_int_gauss_path(&c);
    }
    return run_blur(ctx, path, exact, src_dev, dst_dev, w, h, sigma, radius, nullptr, 0);
}

// the drop shadow's alpha: may it stay a one-channel plane (radius 0: it is not blurred at all), and the blur of that plane
bool pfx_gauss_plane_applies(const pfx_ctx* ctx, bool exact, uint32_t w, uint32_t h, int radius)
{
    const pfx_gauss_case c = case_of(ctx, exact, radius, nullptr, nullptr, w, h, PFX_GAUSS_PLANE);
    return pfx_int_gauss_path(&c) == PFX_GAUSS_PLANE_FUSED;
}
int pfx_gauss_plane(pfx_ctx* ctx, const void* src_plane, void* dst_plane, uint32_t w, uint32_t h, float sigma)
{
    const float* wts = nullptr; PFX_TRY(f32_taps(ctx, sigma, &wts));
    pfx_timer t(ctx, "gauss_plane");
    PFX_HIP(ctx, pfxk_gauss_plane_exact(ctx->stream, (const uint8_t*)src_plane, (uint8_t*)dst_plane, wts, pfx_host_gaussian_radius(sigma), w, h));
    return PFX_OK;
}
