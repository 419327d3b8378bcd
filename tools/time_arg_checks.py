"""Host time per call of three launch-bound `_dev` entry points at 64 x 64: what an entry point's argument check costs shows here and nowhere else.
    python tools/time_arg_checks.py [--calls 4000] [--repeats 5]          (PFX_LIB_PATH=<another build's libpfx.so> for an A/B in one visit)
Per entry point: `repeats` timings of `calls` back-to-back calls on one stream (wall time from the first call until the stream has drained), printed as
microseconds per call: every repeat, the median and the spread (max - min)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: F401  -- before libpfx.so is loaded

from paintfe_amd import _lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=4000)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    lib = _lib.load()
    ctx = C.c_void_p(None)
    assert lib.pfx_ctx_create(C.c_int(0), C.byref(ctx)) == 0
    w = h = 64
    bufs = []
    for _ in range(3):
        p = C.c_void_p(None)
        assert lib.pfx_dev_alloc(ctx, C.c_size_t(w * h * 4), C.byref(p)) == 0 and lib.pfx_dev_memset(ctx, p, C.c_int(77), C.c_size_t(w * h * 4)) == 0
        bufs.append(p)
    src, dst, mask = bufs
    W, H, null = C.c_uint32(w), C.c_uint32(h), C.c_void_p(None)
    settings = _lib.ColorToAlpha((C.c_uint8 * 3)(255, 255, 255), 0, 10.0, 10.0, 1.0, 0.0, 0.0, 1.0, 0.0)
    calls = {
        "pfx_adjust_dev invert": lambda: lib.pfx_adjust_dev(ctx, src, dst, W, H, C.c_int(0), null, C.c_uint32(0), null, null, C.c_int(0)),
        "pfx_color_to_alpha_dev": lambda: lib.pfx_color_to_alpha_dev(ctx, src, dst, W, H, C.byref(settings), null),
        "pfx_select_rect_dev": lambda: lib.pfx_select_rect_dev(ctx, null, W, H, C.c_uint32(3), C.c_uint32(4), C.c_uint32(40), C.c_uint32(50), C.c_uint8(0), mask),
    }
    out = {"lib": _lib.LIB_PATH, "calls": a.calls}
    for name, call in calls.items():
        for _ in range(200):
            assert call() == 0
        lib.pfx_ctx_synchronize(ctx)
        us = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            for _ in range(a.calls):
                call()
            lib.pfx_ctx_synchronize(ctx)
            us.append((time.perf_counter() - t0) / a.calls * 1e6)
        out[name] = {"us_per_call": [round(v, 3) for v in us], "median": round(statistics.median(us), 3), "spread": round(max(us) - min(us), 3)}
    print(json.dumps(out))
    for p in bufs:
        lib.pfx_dev_free(ctx, p)
    lib.pfx_ctx_destroy(ctx)


if __name__ == "__main__":
    main()
