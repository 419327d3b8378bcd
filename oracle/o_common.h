/* o_common.h — shared helpers for the oracle (TEST INFRASTRUCTURE ONLY, see pfx_oracle.h). */
#ifndef PFX_O_COMMON_H
#define PFX_O_COMMON_H
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#ifdef _OPENMP
#include <omp.h>
#endif
#include "pfx_oracle.h"

/* Rust `f32 as u8`: truncate toward zero, saturate, NaN -> 0. */
static inline uint8_t rs_f32_as_u8(float v)
{
    if (!(v > 0.0f)) return 0; /* also NaN, -0.0, negatives */
    if (v >= 255.0f) return 255;
    return (uint8_t)(int)v;
}
/* Rust `f32 as u32` / `as usize` / `as i32` (saturating truncation) */
static inline uint32_t rs_f32_as_u32(float v)
{
    if (!(v > 0.0f)) return 0;
    if (v >= 4294967296.0f) return 0xFFFFFFFFu;
    return (uint32_t)v;
}
static inline int32_t rs_f32_as_i32(float v)
{
    if (v != v) return 0;
    if (v >= 2147483648.0f) return 2147483647;
    if (v <= -2147483648.0f) return (-2147483647 - 1);
    return (int32_t)v;
}
/* Rust f32::clamp (core::f32): NaN propagates */
static inline float rs_clampf(float x, float lo, float hi)
{
    if (x < lo) x = lo;
    if (x > hi) x = hi;
    return x;
}
static inline void o_set_threads(int threads)
{
#ifdef _OPENMP
    if (threads <= 0) { /* all usable cores: the affinity mask, capped by the cgroup CPU quota (a quota-limited box
                           with a wide affinity mask would otherwise be oversubscribed and throttled) */
        threads = omp_get_num_procs();
        FILE* f = fopen("/sys/fs/cgroup/cpu.max", "r");
        if (f) {
            long long quota = 0, period = 0;
            if (fscanf(f, "%lld %lld", &quota, &period) == 2 && quota > 0 && period > 0) {
                int q = (int)((quota + period - 1) / period);
                if (q >= 1 && q < threads) threads = q;
            }
            fclose(f);
        }
    }
    omp_set_num_threads(threads);
#else
    (void)threads;
#endif
}
static inline int o_chunk_index(uint32_t x, uint32_t y, uint32_t w)
{
    uint32_t cxn = (w + PFXO_CHUNK - 1) / PFXO_CHUNK;
    return (int)((y / PFXO_CHUNK) * cxn + (x / PFXO_CHUNK));
}

/* ---- libm call sites (pfxo_set_libm, o_effects2.c) ----
 * Every transcendental of twist, gaussian noise, reduce_noise, vignette and the displacement brush goes through one of
 * the helpers below.  Flavour GLIBC (the default) is the reference: glibc's f32 routines.  Flavour DEVICE evaluates
 * each call the way the HIP kernel does (k_effects2.hip, k_warp.hip, k_libm.h): the f64 routine rounded once to f32
 * for sin/cos/log, the exact f64 product for powf(q, 2), and glibc's expf algorithm restated in f64 (o_libm_exp) for
 * exp.  The remaining flavours are the device one with one deliberate defect each, for the tests to reject. */
enum {
    O_LIBM_GLIBC = 0, O_LIBM_DEVICE = 1,
    O_LIBM_NUDGED = 2,         /* device, results moved by 1 f32 ulp on ~1 % of arguments */
    O_LIBM_EXP_NOFMA = 3,      /* device, o_libm_exp without any fma (remainder and polynomial) */
    O_LIBM_EXP_UNFUSED_R = 4,  /* device, o_libm_exp's remainder as r = z - kd (the form glibc's FMA build does not use) */
    O_LIBM_BRUSH_F64 = 5,      /* device, but the displacement brush's exp as (float)exp((double)x) */
};
extern int o_libm_flavour;
extern long long o_libm_ambiguous;
float o_libm_exp(float x, int variant); /* variant: 0 as the device, 1 no fma at all, 2 only r = z - kd unfused */

/* one f64 result rounded to f32 the way the device rounds its f64 routine's result.  The call is "ambiguous" when an
 * f32 rounding boundary lies within 4 f64 ulps of y: only there can another f64 routine (the device's) round to a
 * different f32. */
static inline float o_round_dev(double y)
{
    double lo = y, hi = y;
    for (int i = 0; i < 4; ++i) { lo = nextafter(lo, -INFINITY); hi = nextafter(hi, INFINITY); }
    if ((float)lo != (float)hi) __atomic_fetch_add(&o_libm_ambiguous, 1, __ATOMIC_RELAXED);
    return (float)y;
}
static inline float o_libm_nudge(float x, float v)
{
    if (o_libm_flavour != O_LIBM_NUDGED) return v;
    uint32_t b;
    memcpy(&b, &x, 4);
    b *= 0x9E3779B9u; b ^= b >> 15; b *= 0x85EBCA6Bu; b ^= b >> 13;
    return (b % 100u == 0u) ? nextafterf(v, INFINITY) : v;
}
static inline float o_cosf(float x) { return o_libm_flavour == O_LIBM_GLIBC ? cosf(x) : o_libm_nudge(x, o_round_dev(cos((double)x))); }
static inline float o_sinf(float x) { return o_libm_flavour == O_LIBM_GLIBC ? sinf(x) : o_libm_nudge(x, o_round_dev(sin((double)x))); }
static inline float o_logf(float x) { return o_libm_flavour == O_LIBM_GLIBC ? logf(x) : o_libm_nudge(x, o_round_dev(log((double)x))); }
static inline float o_expf(float x)
{
    switch (o_libm_flavour) {
    case O_LIBM_GLIBC: return expf(x);
    case O_LIBM_EXP_NOFMA: return o_libm_exp(x, 1);
    case O_LIBM_EXP_UNFUSED_R: return o_libm_exp(x, 2);
    default: return o_libm_nudge(x, o_libm_exp(x, 0));
    }
}
/* powf(q, 2.0f): the device squares in f64 (exact) and rounds once */
static inline float o_sqf(float q) { return o_libm_flavour == O_LIBM_GLIBC ? powf(q, 2.0f) : o_libm_nudge(q, (float)((double)q * (double)q)); }
/* the displacement brush's exp; BRUSH_F64 is the device form before it shared o_libm_exp's */
static inline float o_brush_expf(float x) { return o_libm_flavour == O_LIBM_BRUSH_F64 ? o_round_dev(exp((double)x)) : o_expf(x); }
#endif
