// pfx_flatten.cpp — everything the host knows about the compositor: pfx_tune's knobs, the layer stack's descriptors and reset-layer candidates
// (pfx_int_flatten_cands), the probe's verdict (pfx_int_flatten_verdict), the ONE decision which kernel runs and in what shape (pfx_int_flatten_plan) and the
// entry points that end in it.  The launcher (k_flatten.hip: pfxk_flatten) launches what the plan says; a new compositor kernel or shape is a change to
// this file and to k_flatten.hip.
#include <algorithm>
#include <atomic>
#include <climits>
#include <vector>

#include "pfx_internal.h"

namespace {
// The knobs, under their pfx_tune names less "dle_" (variant: "flatten_variant").  PROCESS-WIDE on purpose — they select among bit-identical kernel shapes for
// A/B runs and tests, not per-document behaviour; atomics because batch workers and device groups run one context per thread, relaxed: a launch on another
// thread sees the old value or the new one.  dle_min_layers, dle_adaptive and chunk_start are per context (pfx_internal.h).
struct {
    // 0 = shipped (2 px x 2 sets, grid stride up to 16 layers; 4 px by mode class), 1-5 = PX / register-set variants, 6 = 3 px x 3 sets (the round-2 shape),
    // +10 = grid-stride launch, 8 = no elimination kernel, 9 = the general kernel
    std::atomic<int> variant{0};
    std::atomic<int> units{0};                // units per wave (0 = default)
    // 0 = 3 pixels per lane, 2 register sets (6 waves per SIMD; measured best), 1 = 2 pixels per lane, 2 = 3 pixels per lane, 3 sets (old kernel only)
    std::atomic<int> cfg{0};
    std::atomic<int> sched{1}, fracA{75}, fracB{20};   // 0 = equal streams of `units`, 1 = streams that shrink: fracA % of the units in long streams, fracB % in quarter-length ones
    std::atomic<int> kernel{0};               // 0 = class sorting inside a unit (flatten_srt_kernel), 1 = round 3's flatten_dle_kernel
    std::atomic<int> s1{-1}, s2{-1};          // re-deal plan: first attempt this many layers above the topmost candidate (-1: 1; 0: never), then every s2 layers (-1: 3; 0: only the first)
    std::atomic<int> stats_on{0};             // pfxk_dle_cands.stats: bit 0 the work counters, bits 1 and 2 the diagnostic builds
} K;
inline int ld(const std::atomic<int>& v) { return v.load(std::memory_order_relaxed); }

// raster-only, whole frame, no preview, pixel indices below 2^30: what every kernel but the template needs besides fast division
inline bool whole_frame_raster(const pfx_flatten_case& c) { return !c.general && !c.has_preview && !(c.rw && c.rh) && (uint64_t)c.w * c.h < (1ull << 30); }
} // namespace

int pfx_flatten_tune(pfx_ctx* ctx, const char* key, int value)
{
    if (std::strcmp(key, "chunk_start") == 0) { ctx->use_chunk_start = value != 0; return PFX_OK; }
    if (std::strcmp(key, "dle_min_layers") == 0) { ctx->dle_min_layers = value; return PFX_OK; }
    if (std::strcmp(key, "dle_adaptive") == 0) { ctx->dle_adaptive = value != 0; ctx->dle_probe_state = 0; return PFX_OK; }   // 0 = shallow stacks never take the elimination kernel
    if (std::strcmp(key, "dle_ring") == 0) return PFX_OK;   // round 3's ring size is a template argument now: accepted, does nothing
    const struct { const char* key; std::atomic<int>& v; int min, max; } keys[] = {   // a value outside [min, max] leaves the knob as it is
        {"flatten_variant", K.variant, INT_MIN, INT_MAX}, {"dle_units", K.units, 0, INT_MAX}, {"dle_cfg", K.cfg, 0, INT_MAX}, {"dle_sched", K.sched, 0, INT_MAX},
        {"dle_frac_a", K.fracA, 0, 100}, {"dle_frac_b", K.fracB, 0, 100 - ld(K.fracA)}, {"dle_kernel", K.kernel, 0, INT_MAX}, {"dle_s1", K.s1, -1, INT_MAX},
        {"dle_s2", K.s2, -1, INT_MAX}, {"dle_stats", K.stats_on, 0, INT_MAX}};
    for (const auto& k : keys)
        if (std::strcmp(key, k.key) == 0) { if (value >= k.min && value <= k.max) k.v.store(value, std::memory_order_relaxed); return PFX_OK; }
    return pfx_fail(ctx, PFX_ERR_INVALID, "pfx_tune: unknown key %s", key);
}

// Which kernel composites a call and in what shape: a pure function of the case, knobs included.  Returns the plan's kernel.
int pfx_int_flatten_plan(const pfx_flatten_case* cp, pfxk_flatten_plan* p)
{
    const pfx_flatten_case& c = *cp;
    *p = pfxk_flatten_plan{};
    const bool region = c.rw && c.rh;
    const uint64_t n_px = (uint64_t)c.w * c.h;
    const uint32_t cap = 256u * 8u * 4u; // 256 CUs x 8 blocks, x4 waves of grid-stride work granularity
    p->general = c.general || c.has_preview || region;   // a preview or a rectangle only exists in flatten_kernel<true, F>
    p->fast_div = c.fast_div != 0;
    if (!(whole_frame_raster(c) && c.fast_div && c.n_desc > 0 && c.variant != 9)) {
        const uint64_t n_quads = region ? (uint64_t)((c.rw + 3u) / 4u) * c.rh : (n_px + 3) / 4;
        p->grid = (uint32_t)std::min<uint64_t>((n_quads + 255) / 256, cap);
        p->path = PFXK_FLATTEN_TEMPLATE | (p->general ? PFXK_FLATTEN_GENERAL : 0) | (p->fast_div ? PFXK_FLATTEN_FAST_DIV : 0) | (region ? PFXK_FLATTEN_REGION : 0) |
                  (c.has_preview ? PFXK_FLATTEN_PREVIEW : 0);
        return p->kernel = PFXK_FLATTEN_TEMPLATE;
    }
    // dead-layer elimination when the stack holds a reset layer above the bottom one (variant 8 switches it off)
    if (c.n_cands > 0 && c.variant != 8) {
        // dle_sched 0 = equal streams of dle_units
        const bool srt_kernel = c.kernel == 0 && c.unorm_ok;
        const uint32_t px = c.cfg == 1 ? 2u : 3u;
        const uint32_t upx = 64u * px;
        const uint32_t units = (uint32_t)((n_px + upx - 1) / upx);
        const uint32_t umax = 65535u / upx; // queue entries are 16-bit pixel offsets
        pfxk_dle_sched& SC = p->sched;
        if (c.sched == 0) {
            SC.UA = SC.UB = SC.UC = std::min(c.units > 0 ? (uint32_t)c.units : 8u, umax);
            SC.wavesA = (units + SC.UA - 1) / SC.UA;
        } else {
            // the long streams fill the chip about once (256 CUs x 24 waves): measured best (profiles/r03_tuning.md).  No floor: a floor of 4 units left small
            // launches (a 64-row dirty rectangle, a thin band of a sharded document) with a quarter of the waves the chip holds — 8K x 64 rows 0.091 -> 0.037 ms,
            // 8K x 256 rows 0.115 -> 0.081 (tools/lab/band_units_sweep.py, profiles/r04_band_units_sweep.txt)
            // No ceiling above 8 either since the class-sorting kernel (no queue across units: a stream's length only sets how the launch drains): at 8K
            // 22 units per wave left the long streams at 0.82 of a chip-full, 8 runs 1.1 % faster (18 — a hair over one chip-full — 3 % slower),
            // 8K x 2176 rows 11 -> 8: -1.4 % (tools/lab/units_ab.py, randomised order, profiles/r04_units_ab.txt)
            // (round 3's queue kernel keeps its rule: its compacted rounds need long streams)
            const uint32_t ua_fill = ((uint32_t)((uint64_t)units * (uint32_t)c.fracA / 100u) + 6143u) / 6144u;
            const uint32_t ua_auto = srt_kernel ? std::min(std::max(ua_fill, 1u), 8u) : std::max(ua_fill, 4u);
            SC.UA = std::min(c.units > 0 ? (uint32_t)c.units : ua_auto, umax);
            SC.UB = std::max(SC.UA / 4u, 1u);
            SC.UC = 1u;
            SC.wavesA = (uint32_t)((uint64_t)units * (uint32_t)c.fracA / 100u) / SC.UA;
            SC.wavesB = (uint32_t)((uint64_t)units * (uint32_t)c.fracB / 100u) / SC.UB;
        }
        const uint32_t rest = units - std::min(units, SC.wavesA * SC.UA + SC.wavesB * SC.UB);
        p->waves = SC.wavesA + SC.wavesB + (rest + SC.UC - 1) / SC.UC;
        p->stats = (uint32_t)c.stats;
        if (srt_kernel) {
            // re-deal attempts start right above the topmost candidate (below it the early pixels' rounds and the reset layer itself run) and
            // repeat every `seg` layers
            p->redeal.s1 = (uint32_t)c.cand_top + (c.s1 > 0 ? (uint32_t)c.s1 : 1u);
            p->redeal.seg = c.s2 < 0 ? 3u : (c.s2 == 0 ? 1000u : (uint32_t)c.s2);   // 0: a single attempt
            if (c.s1 == 0) p->redeal.seg = 0u;                                       // no attempts at all: round 3's natural pass + parking in the destination
            p->diag = (c.stats & 4) ? 4 : ((c.stats & 2) ? 2 : 0);
            p->px = p->diag ? 3 : (int)px;   // the diagnostic builds exist with 3 pixels per lane only (under dle_cfg 1 the schedule above still counts 2-pixel units: more waves than units, no harm)
            p->path = PFXK_FLATTEN_SRT | PFXK_FLATTEN_FAST_DIV;
            return p->kernel = PFXK_FLATTEN_SRT;
        }
        p->px = (int)px; p->nb = c.cfg == 1 || c.cfg == 2 ? 3 : 2; p->ring = c.cfg == 1 ? 9 : 10;
        p->path = PFXK_FLATTEN_DLE | PFXK_FLATTEN_FAST_DIV;
        return p->kernel = PFXK_FLATTEN_DLE;
    }
    // one 64*PX-pixel tile per wave while that stays below the cap (the dispatcher balances the tail), grid-stride beyond
    // Shipped shape (variant 0), from tools/ab_shallow.py at 8K on stacks of 2 .. 32 layers, with and without an opaque background: 2 pixels
    // per lane and 2 register sets everywhere (against 3 x 3: -2 % at 32 layers, -8 % at 9, -20 % at 4); up to 16 layers the waves also
    // walk the image with a grid stride instead of taking one tile each (a 4-layer tile is over before its launch cost is: -5 .. -10 % more)
    int variant = c.variant % 10;
    bool stride = c.variant >= 10;
    if (c.variant == 0 || c.variant == 8) {
        variant = 1; stride = c.n_desc <= 16;
        // Round 4, tools/lab/shallow_modes_ab.py (8K, 9 and 12 layers, every mode, S2 data; profiles/r04_shallow_modes_ab.txt) and tools/ab_shallow.py (2 .. 9 layers):
        // 4 pixels per lane pay where the blend arithmetic is light — Normal, Multiply, Additive, Difference, Lighten / Darken, Overwrite, Subtract, Linear Burn:
        // one tile per wave -5 .. -7 % from 7 layers up (Normal at 9 layers 0.312 -> 0.290 ms), grid-stride -2 .. -3 % at 5 - 6 layers and for the medium modes
        // (Screen, Overlay, Negation, Hard Light, Exclusion, Linear Light, Hard Mix); the heavy modes (Reflect .. Color Dodge, Xor, Soft Light, Divide, Vivid
        // Light, Pin Light) keep 2 pixels per lane (Vivid Light +9 % with 4), and so do stacks of up to 4 layers
        if (c.n_desc >= 5 && c.mode_class == 2) { variant = 3; stride = c.n_desc < 7; }
        else if (c.n_desc >= 5 && c.mode_class == 1) { variant = 3; stride = true; }
    }
    static const int shape[7][2] = {{3, 3}, {2, 2}, {2, 3}, {4, 2}, {4, 3}, {1, 3}, {3, 3}};   // variant -> PX, NB; any other: 3 x 3
    p->px = shape[variant >= 1 && variant <= 6 ? variant : 0][0];
    p->nb = shape[variant >= 1 && variant <= 6 ? variant : 0][1];
    const uint64_t tiles = (n_px + 64u * p->px - 1) / (64u * p->px);
    p->grid = (uint32_t)std::min<uint64_t>((tiles + 3) / 4, stride ? cap : 1u << 20);
    p->path = PFXK_FLATTEN_STREAM | PFXK_FLATTEN_FAST_DIV | (c.chunk_start ? PFXK_FLATTEN_CHUNK_START : 0);
    return p->kernel = PFXK_FLATTEN_STREAM;
}

// The reset-layer candidates of a stack of n descriptors, bottom -> top (modes[p] < 0: not a raster layer): the topmost min(PFXK_DLE_MAX, max(1, n / 6)) layers
// above the bottom one that are unmasked and Overwrite (canvas_state.rs:1275) or Normal at opacity >= 1 (:1258); only used by the raster-only streaming path
int pfx_int_flatten_cands(const int* modes, const float* opacities, const uint8_t* masked, uint32_t n, int min_layers, int adaptive, pfxk_dle_cands* cands, int* shallow)
{
    std::memset(cands, 0, sizeof *cands);
    *shallow = 0;
    std::vector<std::pair<uint32_t, uint32_t>> found;
    for (uint32_t p = 1; p < n; ++p) {
        if (modes[p] < 0 || masked[p]) continue;
        if (modes[p] == 14) found.emplace_back(p, 0u);
        else if (modes[p] == 0 && opacities[p] >= 1.0f) found.emplace_back(p, 1u);
    }
    // Every candidate the kernel inspects costs a layer's worth of reads for the units it examines, and the elimination kernel's load
    // stream is less efficient than the plain streaming kernel's (4.7 against 5+ TB/s with the arithmetic taken out): it pays where the
    // blend arithmetic dominates — deep stacks — and loses up to 30 % on shallow, memory-bound ones (tools/ab_docs_dle.py: nine Normal
    // layers with S2's alpha 0.43 against 0.33 ms).  Stacks below 16 layers keep the plain kernel (pfx_tune "dle_min_layers").
    // ... unless the caller can decide per stack (flatten_common: a probe of the candidate's alpha, `shallow` tells it the threshold applied)
    if (n < (size_t)min_layers) { if (adaptive) *shallow = 1; else found.clear(); }
    const size_t kmax = std::min<size_t>(PFXK_DLE_MAX, std::max<size_t>(1, n / 6));
    const size_t first = found.size() > kmax ? found.size() - kmax : 0;
    for (size_t k = first; k < found.size(); ++k) {
        cands->layer[cands->n] = found[k].first;
        cands->kind[cands->n] = found[k].second;
        cands->n++;
    }
    return (int)cands->n;
}

// A shallow stack's candidates against the probe of its topmost one (state: pfx_ctx::dle_probe_state; same: the probe was of this stack; usable: whole_frame_raster):
// bit 0 = the stack keeps its candidates (the probe found elimination pays), bit 1 = it is probed behind this composite
int pfx_int_flatten_verdict(int usable, int same, int state) { return !usable ? 0 : (same ? (state == 2 ? 1 : 0) : 2); }

namespace {

// layer stack -> device descriptors
// preview layer of a composite call (device pointers; see pfx_preview in include/pfx.h)
struct preview_arg {
    const void* d_pixels = nullptr;
    const void* d_chunk_present = nullptr; // NULL: derive with the from_rgba_image rule
    pfx_preview info{};
};

int build_stack(pfx_ctx* ctx, const void* const* layer_ptrs, const void* const* mask_ptrs, const pfx_layer_info* layers,
                uint32_t n, uint32_t w, uint32_t h, bool from_store, uint32_t* n_desc, bool* general, bool* has_adj,
                uint32_t track_info = 0xFFFFFFFFu, uint32_t* track_pos = nullptr, const uint8_t** track_pixels = nullptr,
                pfxk_dle_cands* cands = nullptr, std::vector<uint8_t>* chunk_meta = nullptr, bool* shallow = nullptr)
{
    std::vector<const uint8_t*> flag_ptrs; // per descriptor: the stored layer's chunk alpha summary (NULL: none)
    std::vector<pfxk_layer_desc> desc;
    std::vector<float> adj;
    desc.reserve(n);
    *general = false;
    *has_adj = false;
    if (track_pos) *track_pos = 0xFFFFFFFFu;
    for (uint32_t i = 0; i < n; ++i) {
        const pfx_layer_info& L = layers[i];
        if (!L.visible) continue; // layer_effectively_visible == false: skipped entirely (canvas_state.rs:576)
        pfxk_layer_desc d{};
        d.opacity = L.opacity;
        d.mode = L.blend_mode > 24 ? 0u : (uint32_t)L.blend_mode; // BlendMode::from_u8 fallback
        d.kind = L.kind;
        if (L.kind != PFX_LAYER_RASTER) {
            if (L.kind > PFX_ADJ_CHANNEL_MIXER) return pfx_fail(ctx, PFX_ERR_INVALID, "layer %u: unknown kind %u", i, L.kind);
            d.adj_off = (uint32_t)adj.size();
            float a[16];
            std::memcpy(a, L.adj, sizeof a);
            if (L.kind == PFX_ADJ_EXPOSURE) a[0] = pfx_host_exposure_gain(L.adj[0]);
            if (L.kind == PFX_ADJ_BRIGHTNESS_CONTRAST) a[1] = pfx_host_bc_factor(L.adj[1]);
            adj.insert(adj.end(), a, a + 16);
            *general = true;
            *has_adj = true;
        } else if (from_store) {
            auto it = ctx->layers.find(L.layer_idx);
            if (it == ctx->layers.end()) continue; // not uploaded: skipped like the reference (renderer.rs:556)
            if (it->second.w != w || it->second.h != h)
                return pfx_fail(ctx, PFX_ERR_INVALID, "layer %u is %ux%u, canvas is %ux%u", L.layer_idx, it->second.w, it->second.h, w, h);
            d.pixels = (const uint8_t*)it->second.pixels.p;
            if (it->second.has_mask) { d.mask = (const uint8_t*)it->second.mask.p; *general = true; }
            flag_ptrs.resize(desc.size() + 1, nullptr);
            flag_ptrs[desc.size()] = it->second.has_mask ? nullptr : (const uint8_t*)it->second.chunk_flags.p;
        } else {
            d.pixels = (const uint8_t*)layer_ptrs[i];
            if (!d.pixels) return pfx_fail(ctx, PFX_ERR_INVALID, "layer %u: null device pointer", i);
            if (mask_ptrs && mask_ptrs[i]) { d.mask = (const uint8_t*)mask_ptrs[i]; *general = true; }
        }
        if (d.kind == PFX_LAYER_RASTER) { // Rust f32::clamp(0.0, 1.0); NaN stays NaN (such a stack never takes the streaming kernels)
            const float c = d.opacity < 0.0f ? 0.0f : (d.opacity > 1.0f ? 1.0f : d.opacity);
            std::memcpy(&d.adj_off, &c, 4);
        }
        if (i == track_info && track_pos && d.kind == PFX_LAYER_RASTER) { *track_pos = (uint32_t)desc.size(); *track_pixels = d.pixels; }
        desc.push_back(d);
    }
    *n_desc = (uint32_t)desc.size();
    if (chunk_meta) {
        // [n_desc summary pointers | n_desc wanted bits]: Normal at opacity >= 1 resets a chunk whose alpha is all 255 (canvas_state.rs:1258),
        // Overwrite one without a zero alpha (:1275); layer 0 has nothing below it
        chunk_meta->clear();
        flag_ptrs.resize(desc.size(), nullptr);
        std::vector<uint8_t> want(desc.size(), 0);
        bool any = false;
        for (size_t p = 1; p < desc.size(); ++p) {
            if (desc[p].kind != PFX_LAYER_RASTER || desc[p].mask || !flag_ptrs[p]) continue;
            if (desc[p].mode == 14u) want[p] = 2;
            else if (desc[p].mode == 0u && desc[p].opacity >= 1.0f) want[p] = 1;
            any = any || want[p] != 0;
        }
        if (any) {
            chunk_meta->resize(desc.size() * sizeof(void*) + desc.size());
            std::memcpy(chunk_meta->data(), flag_ptrs.data(), desc.size() * sizeof(void*));
            std::memcpy(chunk_meta->data() + desc.size() * sizeof(void*), want.data(), desc.size());
        }
    }
    {   // arithmetic weight of the stack's blend modes (k_blend.h instruction counts, profiles/r03_blend_isa.md): the streaming compositor's register shape follows it
        static const uint8_t cls_of_mode[25] = {2, 2, 1, 2, 0, 0, 0, 0, 1, 2, 1, 2, 2, 0, 2, 1, 0, 1, 2, 0, 2, 0, 1, 0, 1};
        int cls = 2;
        for (const pfxk_layer_desc& d : desc) cls = std::min(cls, d.kind == PFX_LAYER_RASTER && d.mode < 25u ? (int)cls_of_mode[d.mode] : 0);
        ctx->stack_mode_class = desc.empty() ? 0 : cls;
    }
    if (cands) {   // reset layers (k_flatten.hip: dead-layer elimination)
        std::vector<int> modes; std::vector<float> opac; std::vector<uint8_t> masked;
        for (const pfxk_layer_desc& d : desc) { modes.push_back(d.kind == PFX_LAYER_RASTER ? (int)d.mode : -1); opac.push_back(d.opacity); masked.push_back(d.mask != nullptr); }
        int below = 0;
        pfx_int_flatten_cands(modes.data(), opac.data(), masked.data(), (uint32_t)desc.size(), ctx->dle_min_layers, shallow && ctx->dle_adaptive, cands, &below);
        if (shallow) *shallow = below != 0;
    }
    // PFXK_DESC_PAD copies of the last descriptor behind the stack: the class-sorting compositor requests descriptors ahead of the layer it blends without
    // clamping the index (k_flatten.hip: srt_layers: every fetch() loads the next descriptor, and the loop runs its fetches in pairs, so a pass over an
    // odd number of layers that ends at the top of the stack has read descriptor n + 2; srt_early<NB> runs NB - 1 layers ahead in groups of NB; what is
    // fetched through the copies is never blended)
    if (!desc.empty()) { const pfxk_layer_desc last = desc.back(); desc.insert(desc.end(), PFXK_DESC_PAD, last); }
    // the tables only travel when they differ from what the device already holds (a render loop re-composites the same stack: the
    // small pageable-memory copy in front of every launch was a ~10 us bubble on the stream)
    const size_t desc_bytes = desc.size() * sizeof(pfxk_layer_desc), adj_bytes = adj.size() * sizeof(float);
    const bool same_desc = ctx->d_desc.p && ctx->desc_cache.size() == desc_bytes && (desc_bytes == 0 || std::memcmp(ctx->desc_cache.data(), desc.data(), desc_bytes) == 0);
    if (!same_desc) {
        ctx->desc_cache.clear();
        PFX_TRY(pfx_reserve(ctx, ctx->d_desc, std::max<size_t>(desc.size(), 1) * sizeof(pfxk_layer_desc)));
        PFX_TRY(pfx_h2d(ctx, ctx->d_desc.p, desc.data(), desc_bytes));
        ctx->desc_cache.assign((const uint8_t*)desc.data(), (const uint8_t*)desc.data() + desc_bytes);
    }
    if (!adj.empty()) {
        const bool same_adj = ctx->d_adj.p && ctx->adj_cache.size() == adj_bytes && std::memcmp(ctx->adj_cache.data(), adj.data(), adj_bytes) == 0;
        if (!same_adj) {
            ctx->adj_cache.clear();
            PFX_TRY(pfx_reserve(ctx, ctx->d_adj, adj_bytes));
            PFX_TRY(pfx_h2d(ctx, ctx->d_adj.p, adj.data(), adj_bytes));
            ctx->adj_cache.assign((const uint8_t*)adj.data(), (const uint8_t*)adj.data() + adj_bytes);
        }
    }
    return PFX_OK;
}

int flatten_common(pfx_ctx* ctx, const void* const* layer_ptrs, const void* const* mask_ptrs, const pfx_layer_info* layers,
                   uint32_t n_layers, uint32_t w, uint32_t h, bool from_store, void* dst_dev, const preview_arg* pv = nullptr,
                   const pfxk_region* region = nullptr, const uint8_t* chunk_keys_host = nullptr)
{
    PFX_REQUIRE(ctx, n_layers <= PFX_MAX_LAYERS, "too many layers");
    PFX_REQUIRE(ctx, n_layers == 0 || layers, "null layer list");
    // in place is allowed — dst may BE one of the layers (every kernel reads a pixel of every layer before it writes that pixel) — a partial overlap is not:
    // a workgroup would read pixels another one has already replaced
    if (!from_store && layer_ptrs && dst_dev)
        for (uint32_t l = 0; l < n_layers; ++l)
            if (layer_ptrs[l] && layer_ptrs[l] != dst_dev && pfx_ranges_overlap(layer_ptrs[l], pfx_img_bytes(w, h), dst_dev, pfx_img_bytes(w, h)))
                return pfx_fail(ctx, PFX_ERR_INVALID, "pfx_flatten_dev: dst partially overlaps layer %u (it may be a layer, or disjoint from all)", l);
    uint32_t n_desc = 0, active_pos = 0xFFFFFFFFu;
    const uint8_t* active_pixels = nullptr;
    bool general = false, has_adj = false;
    pfxk_dle_cands cands{};
    std::vector<uint8_t> chunk_meta;
    bool shallow = false;
    PFX_TRY(build_stack(ctx, layer_ptrs, mask_ptrs, layers, n_layers, w, h, from_store, &n_desc, &general, &has_adj,
                        pv ? pv->info.active_layer : 0xFFFFFFFFu, &active_pos, &active_pixels, &cands, from_store ? &chunk_meta : nullptr,
                        from_store ? nullptr : &shallow));
    bool fast_div = true; // k_flatten.hip:rdiv is bit-identical to '/' unless an opacity is a positive value < 2^-40
    for (uint32_t i = 0; i < n_layers; ++i) fast_div = fast_div && opacity_allows_fast_div(layers[i].opacity);
    pfx_flatten_case c{};   // what the plan reads: the call here, the candidates, the flags and the knobs as they settle below
    c.n_desc = (int)n_desc; c.w = w; c.h = h; c.general = general; c.has_preview = pv && pv->d_pixels; c.fast_div = fast_div; c.mode_class = ctx->stack_mode_class;
    if (region) { c.rw = region->rw; c.rh = region->rh; }
    const bool fast_ok = whole_frame_raster(c) && fast_div;   // anything else runs flatten_kernel
    bool probe_now = false;
    uint32_t probe_layer = 0, probe_kind = 0;
    if (shallow && cands.n > 0) {
        // Below the depth threshold the elimination kernel runs only where a probe of THIS stack found its topmost reset layer coherent (an opaque photo layer,
        // a filled background above old layers: most units start there and read nothing below; per-pixel-random alpha splits every unit and loses 30 %).  The
        // probe runs once per stack, behind the composite that found none, and reports through pinned memory: later composites of the same stack use it.
        std::vector<uint8_t> key(ctx->desc_cache);
        key.insert(key.end(), (const uint8_t*)&w, (const uint8_t*)&w + 4); key.insert(key.end(), (const uint8_t*)&h, (const uint8_t*)&h + 4);
        const bool same = ctx->dle_probe_state != 0 && key == ctx->dle_probe_key;
        if (same && ctx->dle_probe_state == 1 && hipEventQuery(ctx->ev_dle_probe) == hipSuccess)
            ctx->dle_probe_state = *ctx->h_dle_verdict == (ctx->dle_probe_tag | 0x80000000u) ? 2 : 3;
        const int verdict = pfx_int_flatten_verdict(whole_frame_raster(c), same, ctx->dle_probe_state);
        if (verdict & 2) { probe_now = true; ctx->dle_probe_key.swap(key); ctx->dle_probe_state = 0; }
        probe_layer = cands.layer[cands.n - 1u]; probe_kind = cands.kind[cands.n - 1u];
        if (!(verdict & 1)) cands.n = 0;   // the plain streaming kernel
    }
    const size_t nchunks = (size_t)((w + 63) / 64) * ((h + 63) / 64);
    uint8_t* d_chunks = nullptr;
    bool chunks_ready = false;
    if (has_adj) { // adjustment layers only run on chunks populated in some visible layer (canvas_state.rs:529-550)
        PFX_TRY(pfx_reserve(ctx, ctx->d_chunks, nchunks));
        d_chunks = (uint8_t*)ctx->d_chunks.p;
        // a caller that still has the layers' TiledImage chunk keys (a loaded document) passes their union: a chunk that is present
        // but fully transparent counts, exactly as in the reference; flat layers can only offer "some alpha != 0" (the kernel's pre-pass)
        if (chunk_keys_host && !(pv && pv->d_pixels)) { PFX_TRY(pfx_h2d(ctx, d_chunks, chunk_keys_host, nchunks)); chunks_ready = true; }
    }
    pfxk_preview PV{};
    if (pv && pv->d_pixels) { // chunk flags: [preview present | active layer present] (canvas_state.rs:541-548,587,593-597)
        PFX_TRY(pfx_reserve(ctx, ctx->fx_a, 2 * nchunks));
        uint8_t* flags = (uint8_t*)ctx->fx_a.p;
        if (pv->d_chunk_present) PFX_HIP(ctx, hipMemcpyAsync(flags, pv->d_chunk_present, nchunks, hipMemcpyDeviceToDevice, ctx->stream));
        else PFX_HIP(ctx, pfxk_chunk_populated(ctx->stream, (const uint8_t*)pv->d_pixels, w, h, flags));
        if (active_pixels) PFX_HIP(ctx, pfxk_chunk_populated(ctx->stream, active_pixels, w, h, flags + nchunks));
        PV.pixels = (const uint8_t*)pv->d_pixels;
        PV.chunk_present = flags;
        PV.layer_chunk_present = flags + nchunks;
        PV.active_pos = active_pos; // 0xFFFFFFFF when the active layer is hidden: only its chunk keys count
        PV.mode = pv->info.blend_mode > 24 ? 0u : pv->info.blend_mode;
        PV.is_eraser = pv->info.is_eraser != 0;
        PV.replaces = pv->info.replaces_layer != 0;
    }
    // stored layers: the per-chunk start table (which layer is the first that can show in a 64 x 64 chunk) from their alpha summaries —
    // only the plain streaming kernel takes it (whole-frame, raster-only stacks)
    const uint8_t* d_chunk_start = nullptr;
    if (ctx->use_chunk_start && !chunk_meta.empty() && fast_ok && cands.n == 0 && n_desc < 255) {
        if (!ctx->h_chunk_useful) {
            PFX_HIP(ctx, hipHostMalloc((void**)&ctx->h_chunk_useful, sizeof(uint32_t), hipHostMallocDefault));
            *ctx->h_chunk_useful = 0;
            PFX_HIP(ctx, hipEventCreateWithFlags(&ctx->ev_chunk_useful, hipEventDisableTiming));
        }
        const bool same = ctx->chunk_state != 0 && ctx->chunk_epoch == ctx->store_epoch && ctx->chunk_meta_cache == chunk_meta &&
                          ctx->d_chunk_start.cap >= nchunks;
        if (same && ctx->chunk_state == 1 && hipEventQuery(ctx->ev_chunk_useful) == hipSuccess)
            ctx->chunk_state = (*ctx->h_chunk_useful == ctx->chunk_tag) ? 2 : 3; // the table kernel of an earlier call has finished: its verdict is in
        if (!same) {
            ctx->chunk_meta_cache.clear();
            PFX_TRY(pfx_reserve(ctx, ctx->d_chunk_meta, chunk_meta.size()));
            PFX_TRY(pfx_h2d(ctx, ctx->d_chunk_meta.p, chunk_meta.data(), chunk_meta.size()));
            ctx->chunk_meta_cache = chunk_meta;
            PFX_TRY(pfx_reserve(ctx, ctx->d_chunk_start, nchunks));
            ctx->chunk_tag += 1u;
            PFX_HIP(ctx, pfxk_chunk_start(ctx->stream, (const uint8_t* const*)ctx->d_chunk_meta.p, (const uint8_t*)ctx->d_chunk_meta.p + (size_t)n_desc * sizeof(void*),
                                          n_desc, (uint32_t)nchunks, (uint8_t*)ctx->d_chunk_start.p, ctx->h_chunk_useful, ctx->chunk_tag));
            PFX_HIP(ctx, hipEventRecord(ctx->ev_chunk_useful, ctx->stream));
            ctx->chunk_state = 1;
            ctx->chunk_epoch = ctx->store_epoch;
        }
        if (ctx->chunk_state != 3) d_chunk_start = (const uint8_t*)ctx->d_chunk_start.p; // pending or useful: the table of THIS stack is in the buffer
    }
    // The class-sorting compositor (k_flatten.hip: flatten_srt_kernel) reads every layer through typed UNORM8 buffer loads and keeps its accumulators as
    // RN(k / 255); its result leaves as v_cvt_pk_u8_f32 + dword stores (the typed format store measured 1 % slower).  The device's UNORM8 <-> float
    // conversions must be exact for all 256 byte values, which is checked once per context on the device itself.  Otherwise round 3's kernel runs.
    if (cands.n > 0 && fast_ok) {
        if (ctx->unorm_store_ok < 0) {
            PFX_TRY(pfx_reserve(ctx, ctx->d_misc, 2048));
            PFX_HIP(ctx, hipMemsetAsync(ctx->d_misc.p, 0, 2048, ctx->stream));
            PFX_HIP(ctx, pfxk_unorm_store_check(ctx->stream, (uint8_t*)ctx->d_misc.p, (unsigned long long*)((uint8_t*)ctx->d_misc.p + 1024)));
            unsigned long long bad = 1;
            PFX_TRY(pfx_d2h(ctx, &bad, (uint8_t*)ctx->d_misc.p + 1024, sizeof bad));
            PFX_TRY(pfx_sync(ctx)); // once per context
            ctx->unorm_store_ok = bad == 0 ? 1 : 0;
        }
        c.unorm_ok = ctx->unorm_store_ok == 1;
    }
    if (cands.n > 0) { c.n_cands = (int)cands.n; c.cand_top = (int)cands.layer[cands.n - 1u]; }
    c.chunk_start = d_chunk_start != nullptr;
    c.variant = ld(K.variant); c.units = ld(K.units); c.cfg = ld(K.cfg); c.sched = ld(K.sched); c.fracA = ld(K.fracA); c.fracB = ld(K.fracB);
    c.kernel = ld(K.kernel); c.s1 = ld(K.s1); c.s2 = ld(K.s2); c.stats = ld(K.stats_on);
    pfx_int_flatten_plan(&c, &ctx->last_flatten_plan);
    {
        pfx_timer t(ctx, "flatten");
        PFX_HIP(ctx, pfxk_flatten(ctx->stream, &ctx->last_flatten_plan, (const pfxk_layer_desc*)ctx->d_desc.p, n_desc, (const float*)ctx->d_adj.p, d_chunks, chunks_ready ? 1 : 0,
                                  w, h, (uint8_t*)dst_dev, PV.pixels ? &PV : nullptr, region, &cands, d_chunk_start));
    }
    if (probe_now) {   // behind the composite (it may have been in place: the probe reads layers, and a layer that was the destination now holds the result — a hint all the same)
        if (!ctx->h_dle_verdict) {
            PFX_HIP(ctx, hipHostMalloc((void**)&ctx->h_dle_verdict, sizeof(uint32_t), hipHostMallocDefault));
            *ctx->h_dle_verdict = 0;
        }
        if (!ctx->ev_dle_probe) PFX_HIP(ctx, hipEventCreateWithFlags(&ctx->ev_dle_probe, hipEventDisableTiming));
        ctx->dle_probe_tag = (ctx->dle_probe_tag + 1u) & 0x7fffffffu;
        PFX_HIP(ctx, pfxk_dle_probe(ctx->stream, (const pfxk_layer_desc*)ctx->d_desc.p, probe_layer, probe_kind, (uint32_t)((size_t)w * h), ctx->h_dle_verdict, ctx->dle_probe_tag));
        PFX_HIP(ctx, hipEventRecord(ctx->ev_dle_probe, ctx->stream));
        ctx->dle_probe_state = 1;
    }
    return PFX_OK;
}

} // namespace

extern "C" {

int pfx_flatten_dev(pfx_ctx* ctx, const void* const* layer_ptrs_dev, const void* const* mask_ptrs_dev,
                    const pfx_layer_info* layers, uint32_t n_layers, uint32_t w, uint32_t h, void* dst_dev)
{
    if (!ctx) return PFX_ERR_INVALID;
    PFX_REQUIRE(ctx, dst_dev && pfx_dims_ok(w, h) && (n_layers == 0 || layer_ptrs_dev), "pfx_flatten_dev: bad arguments");
    PFX_TRY(pfx_use(ctx));
    return flatten_common(ctx, layer_ptrs_dev, mask_ptrs_dev, layers, n_layers, w, h, false, dst_dev);
}

// pfx_flatten_dev for a document whose layers are TiledImages: chunk_keys_host[c] != 0 where some visible raster layer HOLDS chunk c
// (canvas_state.rs:528-550 `chunk_keys()`), whatever its pixels are
int pfx_int_flatten_with_chunk_keys_dev(pfx_ctx* ctx, const void* const* layer_ptrs_dev, const pfx_layer_info* layers, uint32_t n_layers,
                                        uint32_t w, uint32_t h, void* dst_dev, const uint8_t* chunk_keys_host)
{
    if (!ctx) return PFX_ERR_INVALID;
    PFX_REQUIRE(ctx, dst_dev && w && h && (n_layers == 0 || layer_ptrs_dev), "pfx_int_flatten_with_chunk_keys_dev: bad arguments");
    PFX_TRY(pfx_use(ctx));
    return flatten_common(ctx, layer_ptrs_dev, nullptr, layers, n_layers, w, h, false, dst_dev, nullptr, nullptr, chunk_keys_host);
}

int pfx_int_flatten_last_path(pfx_ctx* ctx) { return !ctx ? -1 : ctx->last_flatten_plan.path; }
int pfx_int_flatten_last_plan(pfx_ctx* ctx, pfxk_flatten_plan* plan) { if (!ctx || !plan) return -1; *plan = ctx->last_flatten_plan; return plan->path; }

int pfx_composite_region(pfx_ctx* ctx, uint32_t w, uint32_t h, const pfx_layer_info* layers, uint32_t n_layers, uint32_t x,
                         uint32_t y, uint32_t rw, uint32_t rh, uint8_t* dst_region)
{
    if (!ctx) return PFX_ERR_INVALID;
    PFX_REQUIRE(ctx, dst_region && pfx_dims_ok(w, h) && pfx_rect_inside(x, y, rw, rh, w, h), "pfx_composite: bad arguments");
    PFX_TRY(pfx_use(ctx));
    PFX_TRY(pfx_reserve(ctx, ctx->st_out, pfx_img_bytes(w, h)));
    if (rw == w && rh == h) {
        PFX_TRY(flatten_common(ctx, nullptr, nullptr, layers, n_layers, w, h, true, ctx->st_out.p));
        return pfx_unstage(ctx, dst_region, ctx->st_out, pfx_img_bytes(w, h));
    }
    // dirty rectangle (composite_dirty_readback, renderer.rs:588): only its pixels are composited, into a compact rw x rh image
    const pfxk_region rg{x, y, rw, rh};
    PFX_TRY(flatten_common(ctx, nullptr, nullptr, layers, n_layers, w, h, true, ctx->st_out.p, nullptr, &rg));
    PFX_TRY(pfx_d2h(ctx, dst_region, ctx->st_out.p, (size_t)rw * rh * 4));
    return pfx_sync(ctx);
}

int pfx_composite(pfx_ctx* ctx, uint32_t w, uint32_t h, const pfx_layer_info* layers, uint32_t n_layers, uint8_t* dst)
{
    return pfx_composite_region(ctx, w, h, layers, n_layers, 0, 0, w, h, dst);
}

// composite with the tool preview layer folded into the active layer (canvas_state.rs:541-548,593-658)
int pfx_composite_preview(pfx_ctx* ctx, uint32_t w, uint32_t h, const pfx_layer_info* layers, uint32_t n_layers, const uint8_t* preview_pixels,
                          const uint8_t* preview_chunk_present, const pfx_preview* preview, uint8_t* dst)
{
    if (!ctx) return PFX_ERR_INVALID;
    PFX_REQUIRE(ctx, dst && pfx_dims_ok(w, h), "pfx_composite_preview: bad arguments");
    if (!preview_pixels) return pfx_composite(ctx, w, h, layers, n_layers, dst);
    PFX_REQUIRE(ctx, preview != nullptr, "pfx_composite_preview: null preview description");
    PFX_TRY(pfx_use(ctx));
    const size_t nchunks = (size_t)((w + 63) / 64) * ((h + 63) / 64);
    PFX_TRY(pfx_reserve(ctx, ctx->st_out, pfx_img_bytes(w, h)));
    PFX_TRY(pfx_reserve(ctx, ctx->fx_b, pfx_img_bytes(w, h) + nchunks));
    PFX_TRY(pfx_h2d(ctx, ctx->fx_b.p, preview_pixels, pfx_img_bytes(w, h)));
    preview_arg pv;
    pv.d_pixels = ctx->fx_b.p;
    if (preview_chunk_present) {
        PFX_TRY(pfx_h2d(ctx, (uint8_t*)ctx->fx_b.p + pfx_img_bytes(w, h), preview_chunk_present, nchunks));
        pv.d_chunk_present = (const uint8_t*)ctx->fx_b.p + pfx_img_bytes(w, h);
    }
    pv.info = *preview;
    PFX_TRY(flatten_common(ctx, nullptr, nullptr, layers, n_layers, w, h, true, ctx->st_out.p, &pv));
    return pfx_unstage(ctx, dst, ctx->st_out, pfx_img_bytes(w, h));
}

int pfx_flatten_preview_dev(pfx_ctx* ctx, const void* const* layer_ptrs_dev, const void* const* mask_ptrs_dev, const pfx_layer_info* layers,
                            uint32_t n_layers, uint32_t w, uint32_t h, const void* preview_dev, const void* preview_chunk_present_dev,
                            const pfx_preview* preview, void* dst_dev)
{
    if (!ctx) return PFX_ERR_INVALID;
    PFX_REQUIRE(ctx, dst_dev && pfx_dims_ok(w, h) && (n_layers == 0 || layer_ptrs_dev) && (!preview_dev || preview), "pfx_flatten_preview_dev: bad arguments");
    PFX_TRY(pfx_use(ctx));
    preview_arg pv;
    pv.d_pixels = preview_dev;
    pv.d_chunk_present = preview_chunk_present_dev;
    if (preview) pv.info = *preview;
    return flatten_common(ctx, layer_ptrs_dev, mask_ptrs_dev, layers, n_layers, w, h, false, dst_dev, preview_dev ? &pv : nullptr);
}

int pfx_flatten_stats(pfx_ctx* ctx, uint64_t out[8], int reset)
{
    if (!ctx) return PFX_ERR_INVALID;
    PFX_REQUIRE(ctx, out != nullptr, "pfx_flatten_stats: null output");
    PFX_TRY(pfx_sync(ctx));
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "counter width");
    unsigned long long all[16];
    PFX_HIP(ctx, pfxk_flatten_dle_stats(all, reset));
    for (int i = 0; i < 8; ++i) out[i] = all[i];
    return PFX_OK;
}

int pfx_flatten_trace(pfx_ctx* ctx, uint64_t out[16], int reset)
{
    if (!ctx) return PFX_ERR_INVALID;
    PFX_REQUIRE(ctx, out != nullptr, "pfx_flatten_trace: null output");
    PFX_TRY(pfx_sync(ctx));
    PFX_HIP(ctx, pfxk_flatten_dle_stats((unsigned long long*)out, reset));
    return PFX_OK;
}

} // extern "C"
