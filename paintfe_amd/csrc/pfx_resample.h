// pfx_resample.h — the `image` crate's per-axis weight tables (0.25.9, imageops::resize), built on the host: shared by pfx_resize.cpp (RGBA8) and pfx_matte.cpp (the
// one-channel matte), so that both resamplers take their windows and weights from one function.  Per output sample: a window of source samples around
// (o + 0.5) * ratio, the kernel's weights normalised by their f32 sum (sinf for Lanczos3 from glibc, as the crate's f32::sin resolves to on Linux).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/pfx.h"

namespace pfx_resample {

inline float k_box(float) { return 1.0f; }
inline float k_triangle(float x) { const float a = fabsf(x); return a < 1.0f ? 1.0f - a : 0.0f; }
inline float sinc(float t)
{
    const float a = t * 3.14159265358979323846f;
    return t == 0.0f ? 1.0f : sinf(a) / a;
}
inline float k_lanczos3(float x) { return fabsf(x) < 3.0f ? sinc(x) * sinc(x / 3.0f) : 0.0f; }
inline float k_catmullrom(float x) // bc_cubic_spline(x, 0.0, 0.5)
{
    const float b = 0.0f, c = 0.5f, a = fabsf(x);
    float k;
    if (a < 1.0f) k = (12.0f - 9.0f * b - 6.0f * c) * (a * a * a) + (-18.0f + 12.0f * b + 6.0f * c) * (a * a) + (6.0f - 2.0f * b);
    else if (a < 2.0f) k = (-b - 6.0f * c) * (a * a * a) + (6.0f * b + 30.0f * c) * (a * a) + (-12.0f * b - 48.0f * c) * a + (8.0f * b + 24.0f * c);
    else k = 0.0f;
    return k / 6.0f;
}

struct AxisTable {
    std::vector<uint32_t> left, count, off;
    std::vector<float> wts;
};

inline void build_axis(uint32_t n_in, uint32_t n_out, int filter, AxisTable& t)
{
    float (*kernel)(float) = k_triangle;
    float support = 1.0f;
    switch (filter) {
    case PFX_RESIZE_NEAREST: kernel = k_box; support = 0.0f; break;
    case PFX_RESIZE_BICUBIC: kernel = k_catmullrom; support = 2.0f; break;
    case PFX_RESIZE_LANCZOS3: kernel = k_lanczos3; support = 3.0f; break;
    default: break;
    }
    const float ratio = (float)n_in / (float)n_out;
    const float sratio = ratio < 1.0f ? 1.0f : ratio;
    const float src_support = support * sratio;
    t.left.resize(n_out);
    t.count.resize(n_out);
    t.off.resize(n_out);
    t.wts.clear();
    for (uint32_t o = 0; o < n_out; ++o) {
        float input = ((float)o + 0.5f) * ratio;
        int64_t l = (int64_t)floorf(input - src_support);
        l = std::min<int64_t>(std::max<int64_t>(l, 0), (int64_t)n_in - 1);
        int64_t r = (int64_t)ceilf(input + src_support);
        r = std::min<int64_t>(std::max<int64_t>(r, l + 1), (int64_t)n_in);
        input = input - 0.5f;
        t.left[o] = (uint32_t)l;
        t.count[o] = (uint32_t)(r - l);
        t.off[o] = (uint32_t)t.wts.size();
        float sum = 0.0f;
        const size_t base = t.wts.size();
        for (int64_t i = l; i < r; ++i) {
            const float w = kernel(((float)i - input) / sratio);
            t.wts.push_back(w);
            sum += w;
        }
        for (size_t k = base; k < t.wts.size(); ++k) t.wts[k] /= sum;
    }
}

// one parameter blob for the device: [v.left | v.count | v.off | h.left | h.count | h.off | v.wts | h.wts], v indexed by output row, h by output column; returns
// the number of u32 entries in front of the weights
inline size_t pack_axes(const AxisTable& v, const AxisTable& hz, std::vector<uint32_t>& blob)
{
    const size_t n_u32 = 3 * v.left.size() + 3 * hz.left.size();
    blob.resize(n_u32 + v.wts.size() + hz.wts.size());
    uint32_t* p = blob.data();
    auto put = [&](const std::vector<uint32_t>& a) { std::copy(a.begin(), a.end(), p); p += a.size(); };
    put(v.left); put(v.count); put(v.off); put(hz.left); put(hz.count); put(hz.off);
    std::memcpy(p, v.wts.data(), v.wts.size() * 4);
    std::memcpy(p + v.wts.size(), hz.wts.data(), hz.wts.size() * 4);
    return n_u32;
}

// the widest source-column range the horizontal taps of one output tile of `tile` columns reach (left and left + count are both monotone in the output column)
inline uint32_t span_max(const AxisTable& hz, uint32_t new_w, uint32_t tile)
{
    uint32_t span = 0;
    for (uint32_t ox0 = 0; ox0 < new_w; ox0 += tile) {
        const uint32_t last = std::min(ox0 + tile, new_w) - 1;
        span = std::max(span, hz.left[last] + hz.count[last] - hz.left[ox0]);
    }
    return span;
}

} // namespace pfx_resample
