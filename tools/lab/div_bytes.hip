// tools/lab/div_bytes.hip — are the dividing blend-mode functions of k_blend.h the same bits on an UNREFINED v_rcp_f32 (rdiv_prepare_raw) as with IEEE `/`,
// for every (base byte, top byte) pair?  The Newton step of rdiv_prepare is there for 47045 of 7e13 general significand pairs (profiles/r02_div_exhaust.json);
// a mode function only ever divides operands derived from two bytes.  One lane per pair, six modes, compared on the uint32 view.
// Build: hipcc -O3 -std=c++17 -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt -fno-fast-math -fno-gpu-flush-denormals-to-zero --offload-arch=gfx950
//        -I paintfe_amd/csrc -I include tools/lab/div_bytes.hip -o tools/lab/_bin/div_bytes
#include "k_blend.h"
#include <cstdio>
using namespace pfxk;

template <uint32_t M, bool F, bool R> __device__ float mode_fn(float b, float t)
{
    if constexpr (M == M_REFLECT) return reflect_channel<F, R>(b, t);
    else if constexpr (M == M_GLOW) return reflect_channel<F, R>(t, b);
    else if constexpr (M == M_COLOR_BURN) return color_burn_channel<F, R>(b, t);
    else if constexpr (M == M_COLOR_DODGE) return color_dodge_channel<F, R>(b, t);
    else if constexpr (M == M_DIVIDE) return divide_channel<F, R>(b, t);
    else return vivid_light_channel<F, R>(b, t);
}
// out[3 * slot]: pairs where the raw reciprocal differs from `/`; [3 * slot + 1]: where the refined one does (0 expected); [3 * slot + 2]: one differing pair
template <uint32_t M> __device__ void check(uint32_t slot, float b, float t, uint32_t pair, uint32_t* out)
{
    const uint32_t want = __builtin_bit_cast(uint32_t, mode_fn<M, false, false>(b, t));
    if (__builtin_bit_cast(uint32_t, mode_fn<M, true, true>(b, t)) != want) { atomicAdd(&out[3 * slot], 1u); out[3 * slot + 2] = pair; }
    if (__builtin_bit_cast(uint32_t, mode_fn<M, true, false>(b, t)) != want) atomicAdd(&out[3 * slot + 1], 1u);
}
__global__ __launch_bounds__(256) void k(uint32_t* out)
{
    const uint32_t kb = blockIdx.x & 255u, kt = threadIdx.x & 255u;
    const float b = (float)kb / 255.0f, t = (float)kt / 255.0f;
    const uint32_t pair = kb * 256u + kt;
    check<M_REFLECT>(0, b, t, pair, out); check<M_GLOW>(1, b, t, pair, out); check<M_COLOR_BURN>(2, b, t, pair, out);
    check<M_COLOR_DODGE>(3, b, t, pair, out); check<M_DIVIDE>(4, b, t, pair, out); check<M_VIVID_LIGHT>(5, b, t, pair, out);
}

int main()
{
    static const char* names[6] = {"reflect", "glow", "color_burn", "color_dodge", "divide", "vivid_light"};
    uint32_t h[18] = {0}, *d = nullptr;
    if (hipMalloc(&d, sizeof h) != hipSuccess || hipMemcpy(d, h, sizeof h, hipMemcpyHostToDevice) != hipSuccess) { printf("no device\n"); return 2; }
    k<<<256, 256>>>(d);
    if (hipDeviceSynchronize() != hipSuccess) { printf("kernel failed\n"); return 2; }
    hipMemcpy(h, d, sizeof h, hipMemcpyDeviceToHost);
    uint32_t bad = 0;
    printf("{\"pairs\": 65536");
    for (int m = 0; m < 6; ++m) {
        printf(", \"%s\": {\"raw_rcp_mismatches\": %u, \"refined_mismatches\": %u", names[m], h[3 * m], h[3 * m + 1]);
        if (h[3 * m]) printf(", \"one_pair\": [%u, %u]", h[3 * m + 2] >> 8, h[3 * m + 2] & 255u);
        printf("}");
        bad += h[3 * m] + h[3 * m + 1];
    }
    printf("}\n");
    return bad ? 1 : 0;
}
