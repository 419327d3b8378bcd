// k_shapes.hip — the shape tool's rasteriser: the 17 built-in SDF shapes of src/ops/shapes.rs (custom path shapes: k_customshape.hip; what the two share:
// k_shape_pixel.h).
//
// Reference: rasterize_shape (src/ops/shapes.rs:1169-1305) — per pixel centre of the shape's bounding box: inverse-rotate into the shape's frame,
// shape_sdf (:827, the sdf_* functions :357-824), coverage_from_sdf / smoothstep (:850, :1441), the fill / outline / both colour mix (:1251-1290) and
// the alpha quantisation (:1293-1300).  shape_outline_coverage (:1020) is not called by the rasteriser and is not here.
//
// Like k_effects2.hip: one pixel per lane, 64x4 pixel tiles (a wave = 64 consecutive pixels of a row), the SDF a template argument and the fill mode a
// wave-uniform branch, every f32 expression in the reference's association order with no contraction, `/` and sqrtf IEEE-correct (k_common.h).
// Everything the reference evaluates per pixel but that is uniform over the image — rotation cos / sin, polygon and star angles and edge vectors,
// vertex lists, the heart's 96-vertex path — is computed once on the host with the reference's own f32 expressions and the host libm
// (pfx_shapes.cpp) and arrives in the parameter block (kernel arguments: uniform indices become scalar loads).
//
// One reordering: min over segment distances is taken on the SQUARED distances with one sqrt at the end (heart path).  sqrtf is correctly rounded,
// hence monotone non-decreasing, so sqrt(min d2) == min sqrt(d2) bit for bit; NaN distances are skipped by both forms (f32::min / v_min_f32 return
// the other operand).
//
// Parity classes: the regular polygons and the stars evaluate atan2 / cos / sin per pixel (:412-463) the way twist does (k_effects2.hip): the f64
// routine rounded once to f32 — +-1 LSB class against the reference's glibc f32 routines; `%` is fmodf, exact by definition.  The other twelve
// kinds are bit-exact.  tests/shape_model.py restates all of it in numpy with both libm flavours.
//
// Three forms of one kernel: the box buffer (`buf` of the reference), the whole-canvas preview (tests/visual_shapes.rs:18-41: box pixels with a > 0 on
// a zeroed canvas), and rasterise + commit in place (blend_pixel_static(layer, pixel, mode, 1.0) where a > 0 and the selection allows: what
// pfx_brush_commit does with the preview) without an intermediate buffer.
#include "k_shape_pixel.h"
#include "pfx_kernels.h"

using namespace pfxk;

namespace {

constexpr float F32_MAX = 3.40282347e+38f;
constexpr float FRAC_PI_2 = 1.57079632679489661923f;

PFX_DEV float sdf_box(float px, float py, float hx, float hy) // :359
{
    const float dx = __builtin_fabsf(px) - hx, dy = __builtin_fabsf(py) - hy;
    const float mx = __builtin_fmaxf(dx, 0.0f), my = __builtin_fmaxf(dy, 0.0f);
    const float outside = __builtin_sqrtf(mx * mx + my * my);
    const float inside = __builtin_fminf(__builtin_fmaxf(dx, dy), 0.0f);
    return outside + inside;
}

PFX_DEV float sdf_line_segment(float px, float py, float ax, float ay, float bx, float by) // :816
{
    const float dx = bx - ax, dy = by - ay;
    const float t = rs_clamp(((px - ax) * dx + (py - ay) * dy) / (dx * dx + dy * dy), 0.0f, 1.0f);
    const float cx = ax + t * dx, cy = ay + t * dy;
    return __builtin_sqrtf((px - cx) * (px - cx) + (py - cy) * (py - cy));
}

template <int SDF>
PFX_DEV float shape_sdf(float px, float py, const pfxk_shape_params& P)
{
    const float hx = P.hx, hy = P.hy;
    if constexpr (SDF == PFXK_SDF_BOX) return sdf_box(px, py, hx, hy);
    else if constexpr (SDF == PFXK_SDF_ELLIPSE) { // :376
        const float nx = px / hx, ny = py / hy;
        const float len = __builtin_sqrtf(nx * nx + ny * ny);
        if (len < 1e-8f) return -__builtin_fminf(hx, hy);
        const float scale = __builtin_sqrtf(hx * hx * ny * ny + hy * hy * nx * nx) / (hx * hy * len);
        return (len - 1.0f) / scale;
    } else if constexpr (SDF == PFXK_SDF_ROUNDED) { // :369; k: r hx-r hy-r
        return sdf_box(px, py, P.k[1], P.k[2]) - P.k[0];
    } else if constexpr (SDF == PFXK_SDF_CONVEX) { // :607; trapezoid / parallelogram / right triangle: verts[0 .. n_verts)
        const int n = P.n_verts;
        float d = (px - P.verts[0][0]) * (px - P.verts[0][0]) + (py - P.verts[0][1]) * (py - P.verts[0][1]);
        float s = 1.0f;
        for (int i = 0, j = n - 1; i < n; j = i, ++i) {
            const float vix = P.verts[i][0], viy = P.verts[i][1], vjy = P.verts[j][1];
            const float ex = P.verts[j][0] - vix, ey = vjy - viy;
            const float wx = px - vix, wy = py - viy;
            const float t = rs_clamp((wx * ex + wy * ey) / (ex * ex + ey * ey), 0.0f, 1.0f);
            const float bx = wx - ex * t, by = wy - ey * t;
            d = __builtin_fminf(d, bx * bx + by * by);
            const bool c1 = py >= viy, c2 = py < vjy, c3 = ex * wy > ey * wx;
            if ((c1 && c2 && c3) || (!c1 && !c2 && !c3)) s = -s;
        }
        return s * __builtin_sqrtf(d);
    } else if constexpr (SDF == PFXK_SDF_TRIANGLE) { // :390
        const float ax = 0.0f, ay = -hy, bx = hx, by = hy, cx = -hx, cy = hy;
        const float d1 = sdf_line_segment(px, py, ax, ay, bx, by);
        const float d2 = sdf_line_segment(px, py, bx, by, cx, cy);
        const float d3 = sdf_line_segment(px, py, cx, cy, ax, ay);
        const float edge = __builtin_fminf(d1, __builtin_fminf(d2, d3));
        const float c1 = (bx - ax) * (py - ay) - (by - ay) * (px - ax);
        const float c2 = (cx - bx) * (py - by) - (cy - by) * (px - bx);
        const float c3 = (ax - cx) * (py - cy) - (ay - cy) * (px - cx);
        const bool inside = (c1 >= 0.0f && c2 >= 0.0f && c3 >= 0.0f) || (c1 <= 0.0f && c2 <= 0.0f && c3 <= 0.0f);
        return inside ? -edge : edge;
    } else if constexpr (SDF == PFXK_SDF_POLYGON) { // :412-430; k: r sx sy max(sx, sy) angle half r*cos(half)
        const float qx = px * P.k[1], qy = py * P.k[2];
        const float angle = P.k[4];
        float theta = libm_atan2(qy, qx) + FRAC_PI_2;
        theta = fmodf(fmodf(theta, angle) + angle, angle) - P.k[5];
        const float len = __builtin_sqrtf(qx * qx + qy * qy);
        return (len * libm_cos(theta) - P.k[6]) / P.k[3];
    } else if constexpr (SDF == PFXK_SDF_CROSS) { // :784
        return __builtin_fminf(sdf_box(px, py, hx * 0.34f, hy), sdf_box(px, py, hx, hy * 0.34f));
    } else if constexpr (SDF == PFXK_SDF_CHECK) { // :793; k: thickness, then the two strokes' end points
        const float d1 = sdf_line_segment(px, py, P.k[1], P.k[2], P.k[3], P.k[4]) - P.k[0];
        const float d2 = sdf_line_segment(px, py, P.k[5], P.k[6], P.k[7], P.k[8]) - P.k[0];
        return __builtin_fminf(d1, d2);
    } else if constexpr (SDF == PFXK_SDF_HEART) { // :519-575; verts: the 96-vertex path, k0 = hy * 0.18
        const float qy = py + P.k[0];
        float min_d2 = __builtin_inff();
        bool inside = false;
        float ax = P.verts[95][0], ay = P.verts[95][1];
        for (int i = 0; i < 96; ++i) {
            const float bx = P.verts[i][0], by = P.verts[i][1];
            const float dx = bx - ax, dy = by - ay;
            const float t = rs_clamp(((px - ax) * dx + (qy - ay) * dy) / (dx * dx + dy * dy), 0.0f, 1.0f);
            const float cx = ax + t * dx, cy = ay + t * dy;
            min_d2 = __builtin_fminf(min_d2, (px - cx) * (px - cx) + (qy - cy) * (qy - cy));
            const float edge_dy = ay - by;
            const bool crosses = (by > qy) != (ay > qy);
            if (__builtin_fabsf(edge_dy) > 1.1920929e-07f && __any(crosses)) { // the quotient is only looked at where the scanline crosses the edge
                const float edge_x = (ax - bx) * (qy - by) / edge_dy + bx;
                if (crosses && px < edge_x) inside = !inside;
            }
            ax = bx;
            ay = by;
        }
        const float dist = __builtin_fminf(F32_MAX, __builtin_sqrtf(min_d2));
        return inside ? -dist : dist;
    } else if constexpr (SDF == PFXK_SDF_DIAMOND) { // :467; k0 = scale
        return (__builtin_fabsf(px) / hx + __builtin_fabsf(py) / hy - 1.0f) * P.k[0];
    } else if constexpr (SDF == PFXK_SDF_STAR) { // :433; k: angle 2*angle ax(ro) ex ey ex*ex+ey*ey
        const float angle = P.k[0], two = P.k[1], ax = P.k[2], ex = P.k[3], ey = P.k[4];
        float theta = libm_atan2(py, px) + FRAC_PI_2;
        theta = fmodf(fmodf(theta, two) + two, two);
        const float len = __builtin_sqrtf(px * px + py * py);
        const float qx = len * libm_cos(theta - angle), qy = len * libm_sin(theta - angle);
        const float fx = qx - ax, fy = qy - 0.0f;
        const float t = rs_clamp((fx * ex + fy * ey) / P.k[5], 0.0f, 1.0f);
        const float cx = ax + ex * t - qx, cy = 0.0f + ey * t - qy;
        const float dist = __builtin_sqrtf(cx * cx + cy * cy);
        return (ex * fy - ey * fx < 0.0f) ? -dist : dist;
    } else { // PFXK_SDF_ARROW :475; k: shaft centre x, shaft half width, shaft_h, head_x, tw, -hy/nl, tw/nl, nl
        static_assert(SDF == PFXK_SDF_ARROW, "unknown SDF");
        const float head_x = P.k[3], tw = P.k[4];
        if (px < head_x) return sdf_box(px - P.k[0], py, P.k[1], P.k[2]);
        const float tx = px - head_x;
        const float max_y = hy * (1.0f - tx / tw);
        const float apy = __builtin_fabsf(py);
        const float dy = apy - max_y;
        if (dy > 0.0f) {
            const float dpx = px - hx, dpy = apy - 0.0f;
            const float to_edge = __builtin_fmaxf(dpx * P.k[5] + dpy * P.k[6], 0.0f);
            const float to_tip = __builtin_sqrtf(dpx * dpx + dpy * dpy);
            return __builtin_fminf(to_edge, to_tip);
        }
        if (tx > tw) return __builtin_sqrtf((px - hx) * (px - hx) + py * py);
        return -__builtin_fmaxf(__builtin_fminf(max_y - apy, (tw - tx) * hy / P.k[7]), 0.0f);
    }
}

PFX_DEV float coverage_from_sdf(float d, int aa) // :850; smoothstep(0.5, -0.5, d) :1441 — edge1 - edge0 is -1.0 exactly
{
    if (!aa) return d < 0.0f ? 1.0f : 0.0f;
    const float t = rs_clamp((d - 0.5f) / -1.0f, 0.0f, 1.0f);
    return t * t * (3.0f - 2.0f * t);
}

// the reference's buffer pixel at box position (col, row): 0 where coverage <= 0.001
template <int SDF>
PFX_DEV uint32_t shape_pixel(int col, int row, const pfxk_shape_params& P)
{
    float lx, ly;
    shape_local(col, row, P, lx, ly);
    const float d = shape_sdf<SDF>(lx, ly, P);
    const int aa = P.anti_alias;
    uint32_t color = P.primary;
    float coverage;
    if (P.fill_mode == 1) coverage = coverage_from_sdf(d, aa);
    else if (P.fill_mode == 0) coverage = rs_clamp(coverage_from_sdf(d, aa) - coverage_from_sdf(d + P.outline_width, aa), 0.0f, 1.0f);
    else { // :1262-1289: interior in the secondary colour, the outline on top in the primary
        const float fill_cov = coverage_from_sdf(d, aa);
        const float oa = rs_clamp(fill_cov - coverage_from_sdf(d + P.outline_width, aa), 0.0f, 1.0f);
        color = P.secondary;
        coverage = fill_cov;
        if (oa > 0.001f) {
            const float fa = fill_cov * (1.0f - oa);
            const float total_a = oa + fa;
            color = 0u;
            coverage = 0.0f;
            if (total_a > 0.0f) {
                const uint32_t p = P.primary, s = P.secondary;
                color = pack_rgba(trunc_u8f((ubyte0(p) * oa + ubyte0(s) * fa) / total_a), trunc_u8f((ubyte1(p) * oa + ubyte1(s) * fa) / total_a),
                                  trunc_u8f((ubyte2(p) * oa + ubyte2(s) * fa) / total_a), trunc_u8f((ubyte3(p) * oa + ubyte3(s) * fa) / total_a));
                coverage = total_a;
            }
        }
    }
    return shape_quantise(color, coverage);
}

// FORM 0: out = the box buffer (bw * bh); 1: out = the canvas (every pixel written); 2: out = the layer, committed in place over the box
template <int SDF, int FORM>
__global__ __launch_bounds__(256) void shape_kernel(const pfxk_shape_params P, uint32_t* __restrict__ out, const uint8_t* __restrict__ selection,
                                                    uint32_t mode, int canvas_w, int canvas_h)
{
    const int tx = shape_tile_x(), ty = shape_tile_y();
    if constexpr (FORM == 1) {
        if (tx >= canvas_w || ty >= canvas_h) return;
        const int col = tx - P.x0, row = ty - P.y0;
        uint32_t px = 0u;
        if (col >= 0 && col < P.bw && row >= 0 && row < P.bh) px = shape_pixel<SDF>(col, row, P);
        out[(size_t)ty * canvas_w + tx] = (px >> 24) != 0u ? px : 0u;
    } else {
        if (tx >= P.bw || ty >= P.bh) return;
        const uint32_t px = shape_pixel<SDF>(tx, ty, P);
        if constexpr (FORM == 0) out[(size_t)ty * P.bw + tx] = px;
        else shape_commit(out, (size_t)(P.y0 + ty) * canvas_w + (P.x0 + tx), px, selection, mode);
    }
}

template <int SDF>
void launch(hipStream_t s, int form, const pfxk_shape_params& P, uint32_t* out, const uint8_t* sel, uint32_t mode, uint32_t cw, uint32_t ch)
{
    const dim3 box_grid = shape_tile_grid(P.bw, P.bh), canvas_grid = shape_tile_grid(cw, ch);
    if (form == PFXK_SHAPE_BOX) shape_kernel<SDF, 0><<<box_grid, 256, 0, s>>>(P, out, sel, mode, (int)cw, (int)ch);
    else if (form == PFXK_SHAPE_CANVAS) shape_kernel<SDF, 1><<<canvas_grid, 256, 0, s>>>(P, out, sel, mode, (int)cw, (int)ch);
    else shape_kernel<SDF, 2><<<box_grid, 256, 0, s>>>(P, out, sel, mode, (int)cw, (int)ch);
}

} // namespace

#define SHAPE_CASE(ID) \
    case ID: launch<ID>(s, form, *P, (uint32_t*)d_out, d_selection, mode, canvas_w, canvas_h); break;

extern "C" hipError_t pfxk_shape(hipStream_t s, int form, int sdf, const pfxk_shape_params* P, uint8_t* d_out, const uint8_t* d_selection, uint32_t mode,
                                 uint32_t canvas_w, uint32_t canvas_h)
{
    if (form != PFXK_SHAPE_BOX && form != PFXK_SHAPE_CANVAS && form != PFXK_SHAPE_COMMIT) return hipErrorInvalidValue;
    if (canvas_w == 0 || canvas_h == 0) return hipSuccess;
    if (form != PFXK_SHAPE_CANVAS && (P->bw <= 0 || P->bh <= 0)) return hipSuccess;
    switch (sdf) {
        SHAPE_CASE(PFXK_SDF_ELLIPSE) SHAPE_CASE(PFXK_SDF_BOX) SHAPE_CASE(PFXK_SDF_ROUNDED) SHAPE_CASE(PFXK_SDF_CONVEX) SHAPE_CASE(PFXK_SDF_TRIANGLE)
        SHAPE_CASE(PFXK_SDF_POLYGON) SHAPE_CASE(PFXK_SDF_CROSS) SHAPE_CASE(PFXK_SDF_CHECK) SHAPE_CASE(PFXK_SDF_HEART) SHAPE_CASE(PFXK_SDF_DIAMOND)
        SHAPE_CASE(PFXK_SDF_STAR) SHAPE_CASE(PFXK_SDF_ARROW)
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
