/* matte_expf_check.c — the oracle's device-flavour expf (the restatement of paintfe_amd/csrc/k_libm.h: libm_exp, held to that header as text by
 * tests/test_libm_model_host.py) against the host's glibc expf on EVERY f32 from +0 to +inf, bit for bit, and on a few NaNs.  The oracle's own exhaustive checker
 * covers arguments <= 0 only; background removal (k_matte.hip) calls the routine with positive ones.  Compiled and run by tests/test_matte_model_host.py:
 *     matte_expf_check <path of libpfx_oracle.so>
 * prints "<arguments> <differences> <first differing argument as hex bits>" and exits 0 when it could run. */
#include <dlfcn.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

static inline uint32_t bits_of(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }
static inline float f32_of(uint32_t b) { float f; memcpy(&f, &b, 4); return f; }

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    void* lib = dlopen(argv[1], RTLD_NOW);
    if (!lib) { fprintf(stderr, "%s\n", dlerror()); return 2; }
    void (*set_libm)(int) = (void (*)(int))dlsym(lib, "pfxo_set_libm");
    float (*eval)(int, float) = (float (*)(int, float))dlsym(lib, "pfxo_libm_eval");
    if (!set_libm || !eval) return 2;
    set_libm(1);   /* O_LIBM_DEVICE */
    const int64_t last = 0x7f800000;   /* +inf */
    long long bad = 0;
    int64_t first = -1;
#pragma omp parallel for schedule(static) reduction(+ : bad)
    for (int64_t b = 0; b <= last; ++b) {
        const float x = f32_of((uint32_t)b);
        if (bits_of(eval(3, x)) != bits_of(expf(x))) {
            ++bad;
#pragma omp critical
            if (first < 0 || b < first) first = b;
        }
    }
    const uint32_t nans[4] = {0x7fc00000u, 0xffc00000u, 0x7fc12345u, 0x7f800001u};
    for (int i = 0; i < 4; ++i)
        if (!isnan(eval(3, f32_of(nans[i])))) { ++bad; if (first < 0) first = nans[i]; }
    printf("%lld %lld %08llx\n", (long long)(last + 1 + 4), bad, (unsigned long long)(first < 0 ? 0 : first));
    return 0;
}
