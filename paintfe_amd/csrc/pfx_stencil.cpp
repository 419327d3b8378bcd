// pfx_stencil.cpp — everything the host knows about the median and the box blur: pfx_tune's knobs, the ONE decision which kernel runs for a call
// (pfx_int_median_path, pfx_int_box_plan) and the launches with their timers.  The entry points (pfx_api.cpp) check arguments and call in here; the launchers
// (k_stencil.hip, k_median_bits.hip) launch what they are told; a new median or box kernel is a change to this file and its .hip file.
#include <algorithm>
#include <atomic>
#include <climits>

#include "pfx_internal.h"

namespace {
// The process-wide knobs, under their pfx_tune names (median_bits_min is per context: pfx_internal.h).  Relaxed: a launch on another thread sees the old value or the new one.
struct {
    std::atomic<int> median_xlane{1};     // bits 0-1: radius 2 on the cross-lane network, one (1) or two (2) rows per lane, or on the per-lane shared-column network (0, round 3's kernel); bit 2: radius 3 on it too
    std::atomic<int> median_single{0};    // radii 2, 3: one window per lane (the pre-sharing selection networks); radius 4: the value search
    std::atomic<int> median_search1{0};   // the value search with one pixel per lane instead of four (the pre-sharing kernel)
    std::atomic<int> median_pair{1};      // 0: the single-column bit-plane kernel for every radius
    // 2 = the fused strip walk for every radius it takes (8K r = 1 .. 4: 0.085-0.098 ms against the 64 x 64 tile kernel's 0.095-0.102), 1 = the tile kernel for small radii
    // and the strip walk above, 0 = tile kernel / two passes; chip fill in % of one round of workgroups; forced segment count (0 = auto)
    std::atomic<int> box_strip{2}, box_strip_fill{100}, box_strip_nseg{0};
    std::atomic<int> box_two_pass{0};     // keep the u8 intermediate in HBM (the pre-fusion path; A/B and parity tests)
    // radii from which the horizontal pass uses prefix sums (0 = never).  8K, tools/lab/box_prefix_ab.py: the prefix pass costs ~0.115 ms whatever the radius (three barriers,
    // a 6-step scan), the sliding window 0.06 ms at r = 9 and 0.15 at r = 100: r = 48 0.201 / 0.221 ms, r = 100 0.276 / 0.237, r = 300 0.570 / 0.339
    std::atomic<int> box_prefix_from{72};
    std::atomic<int> box_px{0}, box_py{0};   // development sweep: columns / rows per lane of the two passes, 0 = by radius
    // radii from which a lane takes 16 columns instead of 8 / 64 rows instead of 16 (128 rows from twice that radius on).  Round-4 sweep of 3 x 4 shapes per radius
    // (tools/lab/box_sweep.py, profiles/r04_box_sweep.txt): 8K r = 5 / 9 / 16 / 24 0.132 / 0.145 / 0.157 / 0.171 -> 0.128 / 0.139 / 0.151 / 0.165 ms; r >= 48 unchanged
    std::atomic<int> box_px_switch{12}, box_py_switch{20};
} K;
inline int ld(const std::atomic<int>& v) { return v.load(std::memory_order_relaxed); }
} // namespace

int pfx_stencil_tune(pfx_ctx* ctx, const char* key, int value)
{
    if (std::strcmp(key, "median_bits_min") == 0) { ctx->median_bits_min = value; return PFX_OK; }
    const struct { const char* key; std::atomic<int>& v; int min; } keys[] = {   // a value below min leaves the knob as it is
        {"median_xlane", K.median_xlane, INT_MIN}, {"median_single", K.median_single, INT_MIN}, {"median_search1", K.median_search1, INT_MIN}, {"median_pair", K.median_pair, INT_MIN},
        {"box_strip", K.box_strip, 0}, {"box_strip_fill", K.box_strip_fill, 1}, {"box_strip_nseg", K.box_strip_nseg, 0}, {"box_two_pass", K.box_two_pass, INT_MIN},
        {"box_prefix_from", K.box_prefix_from, INT_MIN}, {"box_px", K.box_px, 0}, {"box_py", K.box_py, 0}, {"box_px_switch", K.box_px_switch, 0}, {"box_py_switch", K.box_py_switch, 0}};
    for (const auto& k : keys)
        if (std::strcmp(key, k.key) == 0) { if (value >= k.min) k.v.store(value, std::memory_order_relaxed); return PFX_OK; }
    return pfx_fail(ctx, PFX_ERR_INVALID, "pfx_tune: unknown key %s", key);
}

// Which median kernel: a pure function of the case, the first rule that matches.  bits_min (pfx_tune "median_bits_min", default 3): radii from it to 8 take the bit-plane
// radix select (r = 2: 0.35 ms against the networks' 0.22; 9: never); the select has no radius-1 build, so a smaller value means 2.
int pfx_int_median_path(const pfx_median_case* cp)
{
    const pfx_median_case& c = *cp; const int r = c.radius;
    const bool xlane7 = r == 3 && (c.xlane & 4);   // 7x7 on the cross-lane network
    if (r > PFX_MEDIAN_MAX_RADIUS) return PFX_MEDIAN_UNSUPPORTED;
    if (r >= std::max(c.bits_min, 2) && r <= 8 && !xlane7) return c.pair && r <= 7 ? PFX_MEDIAN_BITS_PAIR : PFX_MEDIAN_BITS;
    if (r <= 1) return PFX_MEDIAN_NET3;
    if (xlane7 && !c.single) return PFX_MEDIAN_XLANE7;
    if (r == 2 && (c.xlane & 3) && !c.single) return (c.xlane & 3) == 2 ? PFX_MEDIAN_XLANE_ROWS2 : PFX_MEDIAN_XLANE;
    if (r <= 4 && !c.single) return PFX_MEDIAN_SHARED;
    if (r <= 3) return PFX_MEDIAN_SINGLE_NET;
    if (r > PFXK_MEDIAN_TILE_MAX_RADIUS) return PFX_MEDIAN_HIST;
    return c.search1 ? PFX_MEDIAN_SEARCH1 : PFX_MEDIAN_SEARCH4;
}

// Which box kernels.  In place only the two passes work (H into tmp, V reads tmp and its own pixel of src): a fused kernel stages a halo from src while neighbouring
// workgroups write dst.  px / py: outputs per lane of the two passes, filled whatever the kind.
int pfx_int_box_plan(const pfx_box_case* cp, pfx_box_plan* p)
{
    const pfx_box_case& c = *cp; const bool fused_ok = !c.in_place && !c.two_pass;
    const int r = c.radius, tile_max = pfxk_box_tile_max_radius();
    p->h_kind = PFX_BOX_SLIDING;
    p->px = c.px_force ? (c.px_force == 4 || c.px_force == 8 ? c.px_force : 16) : (r < c.px_switch ? 8 : 16);
    p->py = c.py_force ? (c.py_force == 16 || c.py_force == 32 || c.py_force == 64 ? c.py_force : 128) : (r < c.py_switch ? 16 : (r < 2 * c.py_switch ? 64 : 128));
    if (fused_ok && r <= tile_max && c.strip != 2) return p->kind = PFX_BOX_TILE;
    if (fused_ok && c.strip != 0 && r >= 1 && r <= pfxk_box_strip_max_radius() && (r > tile_max || c.strip == 2) && (uint64_t)c.w * c.h < (1ull << 29)) return p->kind = PFX_BOX_STRIP;
    if (c.prefix_from > 0 && r >= c.prefix_from && c.px_force == 0 && r <= pfxk_box_prefix_max_radius()) p->h_kind = PFX_BOX_PREFIX;
    return p->kind = PFX_BOX_TWO_PASS;
}

int pfx_int_stencil_last_path(pfx_ctx* ctx, int which) { return !ctx ? -1 : (which == 0 ? ctx->last_median_path : ctx->last_box_plan); }

int pfx_stencil_median(pfx_ctx* ctx, const void* src_dev, void* dst_dev, uint32_t w, uint32_t h, int radius, const void* mask_dev)
{
    const pfx_median_case c{radius, ctx->median_bits_min, ld(K.median_xlane), ld(K.median_single), ld(K.median_search1), ld(K.median_pair)};
    const int path = pfx_int_median_path(&c);
    if (path == PFX_MEDIAN_UNSUPPORTED) return pfx_fail(ctx, PFX_ERR_UNSUPPORTED, "median radius %d > %d", radius, PFX_MEDIAN_MAX_RADIUS);
    const bool bits = path == PFX_MEDIAN_BITS_PAIR || path == PFX_MEDIAN_BITS;
    if (bits) PFX_TRY(pfx_reserve(ctx, ctx->st_tmp, pfxk_median_bits_scratch(radius, w, h)));   // the bit planes: scratch ~ the image size
    pfx_timer t(ctx, "median");
    if (bits) PFX_HIP(ctx, pfxk_median_bits(ctx->stream, (const uint8_t*)src_dev, (uint8_t*)dst_dev, (const uint8_t*)mask_dev, (uint32_t*)ctx->st_tmp.p, radius, w, h, path == PFX_MEDIAN_BITS_PAIR));
    else PFX_HIP(ctx, pfxk_median(ctx->stream, (const uint8_t*)src_dev, (uint8_t*)dst_dev, (const uint8_t*)mask_dev, path, radius, w, h));
    ctx->last_median_path = path;
    return PFX_OK;
}

int pfx_stencil_box(pfx_ctx* ctx, const void* src_dev, void* dst_dev, uint32_t w, uint32_t h, int radius, const void* mask_dev, void* tmp_dev)
{
    const pfx_box_case c{radius, src_dev == dst_dev, w, h, ld(K.box_strip), ld(K.box_two_pass), ld(K.box_prefix_from), ld(K.box_px), ld(K.box_py), ld(K.box_px_switch), ld(K.box_py_switch)};
    pfx_box_plan plan; pfx_int_box_plan(&c, &plan);
    if (!tmp_dev) { PFX_TRY(pfx_reserve(ctx, ctx->st_tmp, (size_t)w * h * 4)); tmp_dev = ctx->st_tmp.p; }
    pfx_timer t(ctx, "box_blur");
    PFX_HIP(ctx, pfxk_box_blur(ctx->stream, (const uint8_t*)src_dev, (uint8_t*)tmp_dev, (uint8_t*)dst_dev, (const uint8_t*)mask_dev, radius, w, h, &plan, ld(K.box_strip_fill), ld(K.box_strip_nseg)));
    ctx->last_box_plan = plan.kind | plan.h_kind << 4 | plan.px << 8 | plan.py << 16;
    return PFX_OK;
}
