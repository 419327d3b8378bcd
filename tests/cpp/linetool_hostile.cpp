// linetool_hostile.cpp — pfx_line_bounds and pfx_line_plan (host only, no context) under hostile floats, as a stand-alone program for AddressSanitizer +
// UndefinedBehaviorSanitizer.  The two functions are compiled INTO this program from paintfe_amd/csrc/pfx_linetool.cpp with the sanitizers on; the rest of
// that file resolves from libpfx.so and is not called.  No GPU is touched.  From tests/cpp:
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fno-omit-frame-pointer -fsanitize=address,undefined,float-cast-overflow
//       -fno-sanitize-recover=undefined,float-cast-overflow -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -o linetool_hostile linetool_hostile.cpp
//       ../../paintfe_amd/csrc/pfx_linetool.cpp -L../../paintfe_amd -lpfx -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,/opt/rocm/lib -Wl,-rpath,'$ORIGIN/../../paintfe_amd'
//   ./linetool_hostile
// It prints the number of calls and exits 0; a sanitizer report ends it with a non-zero status.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../include/pfx.h"

int main()
{
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN(), big = std::numeric_limits<float>::max(),
                tiny = std::numeric_limits<float>::denorm_min();
    const float values[] = {0.0f, -0.0f, 1.0f, -1.0f, 0.5f, 63.999996f, 64.0f, 199.5f, 200.0f, 4294967296.0f, -4294967296.0f, 1e10f, -1e10f, 1e30f, -1e30f,
                            big, -big, tiny, -tiny, 2147483648.0f, 16777216.0f, inf, -inf, nan};
    const float sizes[] = {0.0f, -0.0f, 1.0f, 2.9f, 4.0f, 12.0f, -5.0f, 1e-30f, 1e30f, big, -big, tiny, inf, nan};
    const uint32_t dims[][2] = {{200, 136}, {1, 1}, {256000000, 1}, {1, 256000000}, {16000, 16000}, {0, 5}, {20000, 20000}};
    const size_t nv = sizeof values / sizeof *values;
    std::vector<float> dots(2 * 5001 + 2, -7.0f);   // the two floats behind the list are a canary
    unsigned long calls = 0, ok = 0, refused = 0;
    uint32_t seed = 12345u;
    auto next = [&] { seed = seed * 1664525u + 1013904223u; return seed >> 8; };
    for (int round = 0; round < 20000; ++round) {
        pfx_line_tool t;
        std::memset(&t, 0, sizeof t);
        for (float& v : t.p) v = (round % 3 == 0) ? (float)(next() % 400u) - 100.0f : values[next() % nv];
        t.size = sizes[next() % (sizeof sizes / sizeof *sizes)];
        for (uint8_t& c : t.color) c = (uint8_t)next();
        t.pattern = (int32_t)(next() % 5u) - 1; t.cap_style = (int32_t)(next() % 4u) - 1; t.end_shape = (int32_t)(next() % 4u) - 1; t.arrow_side = (int32_t)(next() % 5u) - 1;
        if (round % 2) { t.pattern = (int32_t)(next() % 3u); t.cap_style = (int32_t)(next() % 2u); t.end_shape = (int32_t)(next() % 2u); t.arrow_side = (int32_t)(next() % 3u); }
        t.anti_alias = (int32_t)(next() % 2u);
        const uint32_t* d = dims[next() % (sizeof dims / sizeof *dims)];
        float bounds[4] = {-7.0f, -7.0f, -7.0f, -7.0f}, tris[12];
        uint32_t n = 0xdeadbeefu, nt = 0xdeadbeefu;
        const uint32_t capacity = (uint32_t)(next() % 3u == 0 ? 0u : (next() % 2u ? 5001u : next() % 100u));
        const int sb = pfx_line_bounds(&t, d[0], d[1], bounds);
        const int sp = pfx_line_plan(&t, d[0], d[1], capacity ? dots.data() : nullptr, capacity, &n, next() % 2u ? tris : nullptr, next() % 2u ? &nt : nullptr);
        calls += 2;
        if (sb != sp) { std::printf("round %d: bounds %d, plan %d disagree about the same tool\n", round, sb, sp); return 1; }
        if (sp == PFX_OK) {
            ++ok;
            if (n > 5001u || dots[2 * 5001] != -7.0f || dots[2 * 5001 + 1] != -7.0f) { std::printf("round %d: %u dots or a write past the list\n", round, n); return 1; }
            for (uint32_t k = 0; k < (n < capacity ? n : capacity); ++k)
                if (!(dots[2 * k] >= 0.0f && dots[2 * k + 1] >= 0.0f && dots[2 * k] < (float)d[0] + 1.0f && dots[2 * k + 1] < (float)d[1] + 1.0f)) {
                    std::printf("round %d: dot %u (%g, %g) outside %u x %u\n", round, k, dots[2 * k], dots[2 * k + 1], d[0], d[1]);
                    return 1;
                }
        } else {
            ++refused;
            if (n != 0xdeadbeefu || bounds[0] != -7.0f) { std::printf("round %d: a refused call wrote its outputs\n", round); return 1; }
        }
    }
    // NULL everything, as the header sweep calls them
    calls += 4;
    pfx_line_tool t;
    std::memset(&t, 0, sizeof t);
    uint32_t n = 0;
    if (pfx_line_bounds(nullptr, 0, 0, nullptr) == PFX_OK || pfx_line_plan(nullptr, 0, 0, nullptr, 0, nullptr, nullptr, nullptr) == PFX_OK ||
        pfx_line_bounds(&t, 8, 8, nullptr) == PFX_OK || pfx_line_plan(&t, 8, 8, nullptr, 3, &n, nullptr, nullptr) == PFX_OK) {
        std::printf("a NULL argument was accepted\n");
        return 1;
    }
    std::printf("linetool_hostile: %lu calls, %lu planned, %lu refused, clean\n", calls, ok, refused);
    return 0;
}
