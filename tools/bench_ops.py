#!/usr/bin/env python3
"""tools/bench_ops.py — per-kernel timings of the rest of the path at BASELINE.json's config sizes (device-resident
data, HIP events on the launch stream via pfx_timing).  Not the headline bench (that is bench.py); this is the
evidence table in DESIGN.md §4 / profiles/rNN_ops.json.

    python tools/bench_ops.py [--out profiles/r01_ops.json]
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8000.0


def custom_shape_kept(shape, path, side):
    """host restatement of the kernel's culling (k_customshape.hip, header 3): the average number of segments on a 64 x 4 tile's parity list and on its
    distance list, over the tiles of the side x side box, from the same f32 values the kernel compares"""
    from tests import customshape_model as CM
    from tests import shape_model as M
    F = np.float32
    box = M.bounds(shape, side, side)
    assert box == (0, 0, side, side)
    lx, ly = CM.local_frame(shape, box)
    sx, sy = CM.scales(path, shape["hw"], shape["hh"])
    tw, th = -(-side // 64), -(-side // 4)

    def tile_range(v):   # min and max of a tile's sample coordinates: both offsets, every pixel of the tile (lanes outside the box repeat an edge pixel)
        lo = np.full((th * 4, tw * 64), np.inf, F)
        hi = np.full((th * 4, tw * 64), -np.inf, F)
        a, b = v[0].reshape(side, side), v[1].reshape(side, side)
        lo[:side, :side], hi[:side, :side] = np.minimum(a, b), np.maximum(a, b)
        return lo.reshape(th, 4, tw, 64).min((1, 3)).ravel(), hi.reshape(th, 4, tw, 64).max((1, 3)).ravel()
    px = [((lx + o) + shape["hw"]) * sx + path["bounds"][0] for o in (F(-0.25), F(0.25))]
    py = [((ly + o) + shape["hh"]) * sy + path["bounds"][1] for o in (F(-0.25), F(0.25))]
    (xlo, xhi), (ylo, yhi) = tile_range(px), tile_range(py)
    segs = CM.segments(path)
    ms, ow = max(sx, sy), max(F(shape["outline_width"]), F(1))
    m = np.maximum(np.maximum(np.abs(xlo), np.abs(xhi)), np.maximum(np.abs(ylo), np.abs(yhi)))
    m = np.maximum(m, np.abs(segs).max()).astype(F)
    reach = (np.nextafter(F(float(ow) * float(ms) * (1 + 1 / 1024)), F(np.inf)) + m * F(2.0 ** -16)).astype(F)[:, None]
    kept_p = kept_d = 0
    for k in range(0, len(segs), 512):
        x1, y1, x2, y2 = (segs[k:k + 512, c][None, :] for c in range(4))
        slo, shi = np.minimum(y1, y2), np.maximum(y1, y2)
        kept_p += int(((np.abs(y2 - y1) > F(1e-6)) & ~(shi <= ylo[:, None]) & ~(slo > yhi[:, None])).sum())
        gx = np.maximum(np.minimum(x1, x2) - xhi[:, None], xlo[:, None] - np.maximum(x1, x2))
        gy = np.maximum(slo - yhi[:, None], ylo[:, None] - shi)
        kept_d += int((~((gx > reach) | (gy > reach))).sum())
    return kept_p / len(xlo), kept_d / len(xlo)


def custom_shape_rows(r, timed, torch):
    from paintfe_amd import CustomPath
    from tests import customshape_cases as CC
    from tests import customshape_model as CM
    from tests import shape_cases as SC
    side = 1500
    box = torch.empty((side, side, 4), dtype=torch.uint8, device="cuda")
    for n in (200, 2000, 20000):
        th = np.arange(n) * (2 * math.pi / n)   # a smooth closed curve flattened into n chords: five lobes and a ripple
        rad = 380.0 * (1 + 0.22 * np.sin(5 * th) + 0.08 * np.sin(13 * th + 1.0))
        pts = np.stack([500 + rad * np.cos(th), 500 + rad * np.sin(th)], 1).astype(np.float32)
        path = CM.path([np.concatenate([pts, pts[:1]])], (0, 0, 1000, 1000))
        cp = CustomPath(path["polylines"], path["bounds"])
        for rot in (0.0, 0.4):
            kp, kd = custom_shape_kept(CC.shape("both", cx=750.0, cy=750.0, hw=748.0, hh=748.0, rotation=rot, outline_width=3.0), path, side)
            for fill in ("filled", "outline", "both"):
                shape = CC.shape(fill, cx=750.0, cy=750.0, hw=748.0, hh=748.0, rotation=rot, outline_width=3.0)
                api = SC.to_api(shape)
                assert r.shape_bounds(api, side, side) == (0, 0, side, side)
                tested = f"{kp:.1f} parity" + ("" if fill == "filled" else f" + {kd:.1f} distance")
                for cull in (True, False):
                    was = r.customshape_cull(cull)
                    try:
                        timed(f"custom shape {fill}, {n} segments, rotation {rot}, culling {'on' if cull else 'off'}", ["custom_shape_rasterize"],
                              lambda: r.rasterize_custom_shape_dev(api, cp, side, side, box.data_ptr()), side * side, 4,
                              f"segments tested per sample: {tested if cull else str(n) + ' on every list'}", reps=3 if not cull and n >= 2000 else None,
                              warm=cull or n < 2000)
                    finally:
                        r.customshape_cull(was)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", default="", help="run only the rows whose name contains this text")
    args = ap.parse_args()
    import torch

    from paintfe_amd import GpuRenderer
    from tests import inputs as I

    dev = torch.device("cuda", 0)
    r = GpuRenderer(0)
    r.set_stream(torch.cuda.current_stream().cuda_stream)
    g = torch.Generator(device=dev)
    g.manual_seed(0x5EED0001)
    rows = []

    def timed(name, timer_names, fn, px, alg_bytes_per_px, note="", reps=None, warm=True):
        if args.only and args.only not in name:
            return
        import time
        reps = reps or args.reps
        t_warm = time.perf_counter()  # clocks ramp over the first ~30 ms of load (bench.py's PREWARM standard)
        while warm:
            for _ in range(5):
                fn()
            torch.cuda.synchronize()
            if time.perf_counter() - t_warm >= 0.04:
                break
        r.timing_reset()
        r.timing_enable(True)
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        r.timing_enable(False)
        ms = sum(r.timing_read(t)[0] for t in timer_names) / reps
        gbs = alg_bytes_per_px * px / (ms * 1e-3) / 1e9
        rows.append({"op": name, "ms": round(ms, 4), "Mpx_s": round(px / ms / 1e3, 1), "alg_bytes_px": alg_bytes_per_px,
                     "achieved_GBs": round(gbs, 1), "hbm_frac": round(gbs / HBM_PEAK, 4), "note": note})
        print(rows[-1], flush=True)

    # ---------------- 8K (config 2: Gaussian sigma=16 + HSL; plus the rest of the bank)
    w, h = 7680, 4320
    px = w * h
    src = torch.randint(0, 256, (h, w, 4), dtype=torch.uint8, device=dev, generator=g)
    dst = torch.empty_like(src)
    tmp = torch.empty((h, w, 4), dtype=torch.float32, device=dev)
    mask = (torch.rand((h, w), device=dev, generator=g) < 0.7).to(torch.uint8) * 255
    s, d, t, m = src.data_ptr(), dst.data_ptr(), tmp.data_ptr(), mask.data_ptr()

    for _ in range(40):  # bring the GPU to its steady clocks before the first measured row
        r.gaussian_blur_dev(s, d, w, h, 16.0, t)
    torch.cuda.synchronize()
    timed("gaussian sigma=16 (matrix cores)", ["gauss_mfma"], lambda: r.gaussian_blur_dev(s, d, w, h, 16.0, t), px, 8, "fused H+V strip walk on v_mfma_f32_32x32x16_f16")
    r.set_exact(True)
    timed("gaussian sigma=16 (exact, no FMA)", ["gauss_h", "gauss_v"], lambda: r.gaussian_blur_dev(s, d, w, h, 16.0, t), px, 8, "bit-exact mode")
    timed("gaussian sigma=1 (exact: fused)", ["gauss_fused"], lambda: r.gaussian_blur_dev(s, d, w, h, 1.0, t), px, 8, "bit-exact mode, both passes in one kernel (radii 1 .. 16): what sharpen / glow / drop shadow run")
    timed("gaussian sigma=4 (exact: fused)", ["gauss_fused"], lambda: r.gaussian_blur_dev(s, d, w, h, 4.0, t), px, 8, "bit-exact mode, radius 12 (fused up to 16)")
    r.set_exact(False)
    timed("gaussian sigma=4", ["gauss_mfma"], lambda: r.gaussian_blur_dev(s, d, w, h, 4.0, t), px, 8)
    timed("hsl(30,-20,10)", ["adjust"], lambda: r.adjust_dev(s, d, w, h, "hsl", [30.0, -20.0, 10.0]), px, 8)
    timed("hsl masked + FROM_FLAT", ["adjust"], lambda: r.adjust_dev(s, d, w, h, "hsl", [30.0, -20.0, 10.0], mask_ptr=m, sparse=1), px, 9)
    timed("TiledImage round trip (from_rgba_image -> to_rgba_image)", ["tiled_roundtrip"], lambda: r.tiled_roundtrip_dev(s, d, w, h), px, 8,
          "A0: chunks of 64 x 64 whose alpha is all zero are dropped; one pass")
    # chains (round 6, pfx_chain_dev): several ops, one pass where the kernels allow; every row's result equals the single-op calls one after the other
    three = [("rhai", "exposure", (0.5,)), ("rhai", "sepia"), ("rhai", "invert")]
    timed("chain: exposure -> sepia -> invert (a script's three calls, ONE pass)", ["chain"], lambda: r.chain_dev(s, d, w, h, three), px, 8,
          "pfx_chain_dev; as three launches the same ops cost 3 x a streaming pass")

    def three_launches():
        r.chain_dev(s, d, w, h, three[:1]); r.chain_dev(d, d, w, h, three[1:2]); r.chain_dev(d, d, w, h, three[2:])
    timed("the same three ops as three launches", ["chain"], three_launches, px, 24, "8 B/px each")
    g_hsl = [("gaussian", 16.0), ("adjust", "hsl", (30.0, -20.0, 10.0))]
    timed("chain: gaussian sigma=16 -> hsl (config 2)", ["gauss_mfma_chain", "gauss_mfma", "chain"], lambda: r.chain_dev(s, d, w, h, g_hsl), px, 16,
          "pfx_chain_dev: the Gaussian, then HSL in place (HSL is heavy: not fused by default)")
    r.tune("chain_fuse_heavy", 1)
    timed("gaussian sigma=16 -> hsl with HSL in the matrix-core Gaussian's store (chain_fuse_heavy, not the default)", ["gauss_mfma_chain", "gauss_mfma", "chain"], lambda: r.chain_dev(s, d, w, h, g_hsl), px, 16,
          "the default runs this pair as two launches: HSL is 143 instructions per pixel and costs in the store what it costs as its own pass")
    r.tune("chain_fuse_heavy", 0)
    g_light = [("gaussian", 16.0), ("adjust", "brightness_contrast", (20.0, 10.0)), ("adjust", "invert")]
    timed("chain: gaussian sigma=16 -> brightness/contrast -> invert (ONE launch)", ["gauss_mfma_chain", "gauss_mfma", "chain"], lambda: r.chain_dev(s, d, w, h, g_light), px, 24,
          "light ops in the Gaussian's store; 24 B/px = the three-launch form's algorithmic bytes")
    r.tune("chain_mfma", 0)
    timed("the same, gaussian sigma=16 then brightness/contrast -> invert, as two launches", ["gauss_mfma_chain", "gauss_mfma", "chain"], lambda: r.chain_dev(s, d, w, h, g_light), px, 24)
    timed("the same, gaussian sigma=16 then hsl, as two launches", ["gauss_mfma_chain", "gauss_mfma", "chain"], lambda: r.chain_dev(s, d, w, h, g_hsl), px, 16)
    r.tune("chain_mfma", 1)
    g4_hsl = [("gaussian", 4.0), ("adjust", "hsl", (30.0, -20.0, 10.0))]
    r.set_exact(True)
    timed("chain: exact gaussian sigma=4 -> hsl (config 5's first two ops)", ["gauss_fused_chain", "gauss_fused", "chain"], lambda: r.chain_dev(s, d, w, h, g4_hsl), px, 16,
          "bit-exact fused Gaussian, then HSL in place")
    g4_light = [("gaussian", 4.0), ("adjust", "exposure", (0.5,)), ("adjust", "invert")]
    timed("chain: exact gaussian sigma=4 -> exposure -> invert (ONE launch)", ["gauss_fused_chain", "gauss_fused", "chain"], lambda: r.chain_dev(s, d, w, h, g4_light), px, 24,
          "light ops in the bit-exact fused Gaussian's store")
    r.set_exact(False)
    timed("invert", ["adjust"], lambda: r.adjust_dev(s, d, w, h, "invert"), px, 8)
    timed("brightness_contrast", ["adjust"], lambda: r.adjust_dev(s, d, w, h, "brightness_contrast", [30.0, 20.0]), px, 8)
    lut = np.tile(np.arange(255, -1, -1, dtype=np.uint8), (4, 1))
    timed("levels/curves LUT apply", ["adjust"], lambda: r.adjust_dev(s, d, w, h, "lut_rgba", lut=lut), px, 8)
    timed("vibrance", ["adjust"], lambda: r.adjust_dev(s, d, w, h, "vibrance", [50.0]), px, 8)
    timed("box blur r=3", ["box_blur"], lambda: r.box_blur_dev(s, d, w, h, 3.0), px, 8, "fused column-strip walk (radii 1 .. 60)")
    timed("box blur r=9", ["box_blur"], lambda: r.box_blur_dev(s, d, w, h, 9.0), px, 8, "fused column-strip walk, u8 intermediate in an LDS ring")
    timed("box blur r=48", ["box_blur"], lambda: r.box_blur_dev(s, d, w, h, 48.0), px, 8, "fused column-strip walk")
    timed("median r=1", ["median"], lambda: r.median_dev(s, d, w, h, 1), px, 8)
    timed("median r=2", ["median"], lambda: r.median_dev(s, d, w, h, 2), px, 8, "5x5 network, sorted columns shared across lanes (wave shifts)")
    timed("median r=3", ["median"], lambda: r.median_dev(s, d, w, h, 3), px, 8, "bit-plane radix select (k_median_bits.hip), incl. the planes pre-pass")
    timed("median r=4", ["median"], lambda: r.median_dev(s, d, w, h, 4), px, 8, "bit-plane radix select")
    timed("median r=5", ["median"], lambda: r.median_dev(s, d, w, h, 5), px, 8, "bit-plane radix select")
    timed("median r=7", ["median"], lambda: r.median_dev(s, d, w, h, 7), px, 8, "225-element windows, bit-plane radix select")
    # ---------------- custom shape (k_customshape.hip): a 1500 x 1500 box, a smooth closed path of 200 / 2 000 / 20 000 segments, the three fill modes, rotation 0
    # and 0.4 rad, each with the culling on and off.  The note carries the host-computed average number of segments a sample is tested against (parity list,
    # distance list) with the culling; without it, it is the segment count for both.  The timer starts after the path's flattening and upload.
    if not args.only or "custom shape" in args.only or args.only in "custom shape":
        custom_shape_rows(r, timed, torch)

    # ---------------- the rest of the effect bank (k_effects2.hip), script VM, resamplers
    timed("pixelate block=8", ["pixelate"], lambda: r.pixelate_dev(s, d, w, h, 8), px, 8, "A6: nearest sample at the block centre (reads 1 / 64 of the pixels)")
    timed("vignette", ["vignette"], lambda: r.vignette_dev(s, d, w, h, 0.8, 0.5), px, 8)
    timed("add_noise gaussian mono", ["add_noise"], lambda: r.add_noise_dev(s, d, w, h, 30.0, "gaussian", True, 42, 1.0, 1), px, 8, "f64 ln + cos per pixel")
    timed("add_noise perlin 3 octaves", ["add_noise"], lambda: r.add_noise_dev(s, d, w, h, 50.0, "perlin", False, 42, 5.0, 3), px, 8)
    timed("reduce_noise r=2", ["reduce_noise"], lambda: r.reduce_noise_dev(s, d, w, h, 10.0, 2), px, 8, "25 exp per pixel (glibc expf algorithm in f64)")
    timed("halftone", ["halftone"], lambda: r.halftone_dev(s, d, w, h, 4.0, 45.0, "circle"), px, 8)
    timed("ink (sobel)", ["ink"], lambda: r.ink_dev(s, d, w, h, 1.0, 0.5), px, 8)
    timed("oil_painting r=3 levels=20", ["oil_painting"], lambda: r.oil_painting_dev(s, d, w, h, 3, 20), px, 8, "per-lane LDS histogram sliding down a column")
    timed("crystallize cell=16", ["crystallize"], lambda: r.crystallize_dev(s, d, w, h, 16.0, 42), px, 8, "wave-scanned cell sums -> LDS table -> u64 atomics, + assign")
    timed("bulge", ["bulge"], lambda: r.bulge_dev(s, d, w, h, 0.5), px, 8)
    timed("twist 45", ["twist"], lambda: r.twist_dev(s, d, w, h, 45.0), px, 8, "f64 sin + cos per pixel")
    timed("zoom_blur 16 samples", ["zoom_blur"], lambda: r.zoom_blur_dev(s, d, w, h, 0.5, 0.5, 0.3, 16), px, 8)
    timed("outline width=2", ["outline"], lambda: r.outline_dev(s, d, w, h, 2, (0, 0, 255, 255)), px, 8, "7x7 window search on a bit plane of alpha != 0")
    timed("sharpen amount=1 radius=1", ["sharpen", "gauss_h", "gauss_v"], lambda: r.sharpen_dev(s, d, w, h, 1.0, 1.0), px, 8, "bit-exact Gaussian + combine in one kernel (k_gauss_exact.hip)")
    timed("glow radius=3 intensity=0.5", ["glow", "gauss_h", "gauss_v"], lambda: r.glow_dev(s, d, w, h, 3.0, 0.5), px, 8, "bit-exact Gaussian + combine in one kernel")
    timed("drop shadow blur=3", ["shadow_alpha", "gauss_plane", "gauss_mfma", "gauss_fused", "gauss_h", "gauss_v", "shadow_composite"], lambda: r.shadow_dev(s, d, w, h, 5, 5, 3.0, False, (0, 0, 0, 255), 0.8), px, 8)
    half = torch.empty((h // 2, w // 2, 4), dtype=torch.uint8, device=dev)
    timed("resize 8K -> 4K bilinear", ["resize"], lambda: r.resize_image_dev(s, w, h, half.data_ptr(), w // 2, h // 2, "bilinear"), px, 5, "4 B read + 1 B/px (quarter-size) written")
    timed("resize 8K -> 4K lanczos3", ["resize"], lambda: r.resize_image_dev(s, w, h, half.data_ptr(), w // 2, h // 2, "lanczos3"), px, 5)
    del half
    # ---------------- bucket fill / magic wand (k_flood.hip): the 5 B/px global-scope distance next to the 5 B/px resizes above, then the connected flood
    dist = torch.empty((h, w), dtype=torch.uint8, device=dev)
    dp = dist.data_ptr()
    grey = (120, 120, 120, 255)
    timed("flood: colour distance, global scope, legacy", ["flood_distance_global"], lambda: r.flood_distance_dev(s, w, h, (0, 0), grey, dp, "legacy", 4, True), px, 5,
          "4 B read + 1 B written per pixel, 16-byte loads")
    timed("flood: colour distance, global scope, perceptual", ["flood_distance_global"], lambda: r.flood_distance_dev(s, w, h, (0, 0), grey, dp, "perceptual", 4, True), px, 5,
          "f32 luma / chroma terms, one sqrt, the sRGB table in LDS")
    fl = torch.empty((h, w, 4), dtype=torch.uint8, device=dev)

    def flood_row(name, build):
        if args.only and args.only not in name:
            return
        build()
        torch.cuda.synchronize()
        target = tuple(int(v) for v in fl[0, 0].tolist())
        run = lambda: r.flood_distance_dev(fl.data_ptr(), w, h, (0, 0), target, dp, "legacy", 4, False)
        run()   # the counters, and the one warm-up call: a connected flood is thousands of launches and read-backs on the serpentine, so 3 timed calls
        p, v, tile = r.flood_last(0), r.flood_last(3), r.flood_last(2)
        timed(name, ["flood_distance"], run, px, 5, reps=3, warm=False, note=
              f"contiguous, legacy, 4-connected, seed (0, 0): {p} passes, {v} tile visits of {((w + tile - 1) // tile) * ((h + tile - 1) // tile)} tiles; per pass "
              f"{v / p:.1f} tiles x ({tile * tile} B of c + {(tile + 2) ** 2} B of d read, <= {tile * tile} B written), one 8-byte read-back; mean of 3 calls")

    def build_uniform():
        fl[...] = torch.tensor(grey, dtype=torch.uint8, device=dev)

    def build_noise():   # steps of a few units around a base colour: every threshold cuts the canvas into ragged regions
        fl[..., :3] = (120 + torch.randint(-8, 9, (h, w, 3), device=dev, generator=g)).to(torch.uint8)
        fl[..., 3] = 255

    def build_serpentine():   # tests/flood_cases.py's snake with 32-pixel bands: corridor bands joined at alternating ends through the wall bands
        band = torch.arange(h, device=dev) // 32
        wall = (band % 2 == 1)[:, None].expand(h, w).clone()
        xs = torch.arange(w, device=dev)[None, :]
        right = ((band // 2) % 2 == 0)[:, None]
        wall &= ~torch.where(right, xs >= w - 32, xs < 32)
        fl[...] = torch.tensor(grey, dtype=torch.uint8, device=dev)
        fl[..., 0] = torch.where(wall, 255, 120).to(torch.uint8)
    flood_row("flood: connected, uniform image", build_uniform)
    flood_row("flood: connected, noise at threshold-scale contrast", build_noise)
    flood_row("flood: connected, serpentine of 32-px bands", build_serpentine)
    bmask = torch.empty((h, w), dtype=torch.uint8, device=dev)
    timed("wand mask: threshold + AA band + add to a base", ["wand_mask"], lambda: r.wand_mask_dev(dp, w, h, 40, bmask.data_ptr(), True, "add", m), px, 3)
    timed("fill preview (whole canvas)", ["fill_preview"], lambda: r.fill_preview_dev(dp, w, h, 40, (200, 30, 60, 255), d, m), px, 6)
    timed("fill commit (preview + blend in one kernel, multiply)", ["fill_commit"], lambda: r.fill_commit_dev(d, dp, w, h, 40, (200, 30, 60, 255), 1, m), px, 10,
          "1 + 1 B read, layer 4 B read + written where the fill lands")
    del fl, dist, bmask
    # ---------------- selection masks (k_select.hip): an 8K mask; the disc the feather / expand / contract rows work on is a quarter of the canvas
    yy, xx = torch.meshgrid(torch.arange(h, device=dev), torch.arange(w, device=dev), indexing="ij")
    sel = (((xx - w // 2) ** 2 + (yy - h // 2) ** 2) <= (h // 3) ** 2).to(torch.uint8) * 255
    del yy, xx
    sel_out = torch.empty_like(sel)
    sp, so = sel.data_ptr(), sel_out.data_ptr()
    ang = np.arange(2000) * (2 * np.pi / 2000)
    rad = np.where(np.arange(2000) % 2 == 0, 0.45, 0.25) * h
    lasso = np.stack([w / 2 + rad * np.cos(ang), h / 2 + rad * np.sin(ang)], axis=1).astype(np.float32)
    timed("select: rectangle, add to a base", ["select_rect"], lambda: r.select_rect_dev(w, h, w // 4, h // 4, 3 * w // 4, 3 * h // 4, so, "add", m), px, 2, "1 B read + 1 B written per pixel")
    timed("select: ellipse, intersect with a base", ["select_ellipse"], lambda: r.select_ellipse_dev(w, h, w / 2, h / 2, w / 3, h / 3, so, "intersect", m), px, 2,
          "two IEEE divides per pixel inside the box")
    timed("select: lasso, 2 000-point star, replace", ["select_lasso"], lambda: r.select_lasso_dev(w, h, lasso, so), px, 1,
          "a workgroup per row: 2 000 edges, an LDS bitonic sort of the crossings, 1 B written per pixel; the timer starts after the points' upload")
    timed("selection: translate by (64, -3)", ["selection_translate"], lambda: r.selection_translate_dev(sp, w, h, 64, -3, so), px, 2)
    timed("selection: feather 10 (5 passes)", ["selection_feather"], lambda: r.selection_feather_dev(sp, w, h, 10.0, so), px, 22,
          "5 x (H + V), 1 B read + 1 B written each, + the copy out")
    timed("selection: expand 20", ["selection_expand"], lambda: r.selection_expand_dev(sp, w, h, 20, so), px, 6,
          "row distances: 1 B read, 2 B written and read back; the column walk reads up to 41 u16 per pixel the rule does not skip (from cache), 1 B written")
    timed("selection: contract 20", ["selection_contract"], lambda: r.selection_contract_dev(sp, w, h, 20, so), px, 6)
    timed("selection: bounds", ["selection_bounds"], lambda: r.selection_bounds_dev(sp, w, h), px, 1, "the call waits for the device: 16 bytes read back")
    timed("selection: fill through a grey mask", ["selection_fill"], lambda: r.selection_fill_dev(d, sp, w, h, (200, 30, 60, 255)), px, 9, "an upper bound: 1 B read everywhere, 4 B read + written only inside the disc (0.29 of the canvas)")
    timed("selection: delete through a grey mask", ["selection_delete"], lambda: r.selection_delete_dev(d, sp, w, h), px, 9)
    # ---------------- histogram, per-band Hue/Saturation, colour range (k_colorrange.hip).  The histogram is a reduction over the image like auto-levels' min / max
    # pass (the "minmax" timer inside pfx_auto_levels, host-buffer entry point: the staging is outside that timer), which is timed beside it on the same bytes
    six_bands = [(30.0, -40.0, 10.0), (-60.0, 80.0, -15.0), (90.0, 25.0, 30.0), (-120.0, -75.0, -5.0), (150.0, 60.0, 20.0), (-170.0, -20.0, -35.0)]
    flat_img = torch.empty_like(src)
    flat_img[...] = torch.tensor([200, 100, 50, 255], dtype=torch.uint8, device=dev)
    timed("colorrange: histogram, noise", ["histogram"], lambda: r.histogram_dev(s, w, h), px, 4, "4 B read per pixel, four LDS atomics per counted pixel; the call waits for 4 KiB read back")
    timed("colorrange: histogram, noise, 70 % selection", ["histogram"], lambda: r.histogram_dev(s, w, h, mask_ptr=m), px, 5)
    timed("colorrange: histogram, flat image", ["histogram"], lambda: r.histogram_dev(flat_img.data_ptr(), w, h), px, 4, "every lane on the same four bins: 8 private copies per workgroup")
    if not args.only or args.only in "colorrange: auto-levels min/max pass":
        src_host = src.cpu().numpy()
        timed("colorrange: auto-levels min/max pass", ["minmax"], lambda: r.auto_levels(src_host), px, 4, "the histogram's yardstick: the same bytes, also a reduction", reps=3, warm=False)
        del src_host
    timed("colorrange: per-band hue/saturation, six bands + global", ["hsl_bands"], lambda: r.hsl_bands_dev(s, d, w, h, -15.0, 20.0, 5.0, six_bands), px, 8, "PFX_FROM_FLAT, no selection")
    timed("colorrange: per-band hue/saturation, 70 % selection", ["hsl_bands"], lambda: r.hsl_bands_dev(s, d, w, h, -15.0, 20.0, 5.0, six_bands, mask_ptr=m), px, 9)
    timed("colorrange: select, hue 30 +- 20, fuzziness 0.5", ["color_range"], lambda: r.select_color_range_dev(s, w, h, 30.0, 20.0, 0.1, 0.5, so), px, 5, "an f64 pow per pixel inside the tolerance")
    timed("colorrange: select, hue 60 +- 180, fuzziness 0.3, add to a base", ["color_range"], lambda: r.select_color_range_dev(s, w, h, 60.0, 180.0, 0.0, 0.3, so, "add", m), px, 6,
          "every opaque pixel takes the pow")
    del sel, sel_out, flat_img
    # ---------------- background removal around the model (k_matte.hip): an 8K layer and a 1024 x 1024 model (BiRefNet's size).  The yardstick is the pointwise bank's
    # invert on the same buffers in the same run: 8 B/px, which is the document traffic of the unfeathered post-process.  Every post-process row comes twice: the one
    # call, and the stage calls composed (byte, expand, close, resize, feather, apply), whose full-size matte makes a round trip through memory
    if not args.only or "matte" in args.only:
        from paintfe_amd import matte_settings
        S = 1024
        spx = S * S
        yy, xx = torch.meshgrid(torch.arange(S, device=dev, dtype=torch.float32), torch.arange(S, device=dev, dtype=torch.float32), indexing="ij")
        blob = (1.0 - torch.hypot((xx - S * 0.45) / (S * 0.3), (yy - S * 0.55) / (S * 0.35))) * 9.0 + torch.randn((S, S), device=dev, generator=g) * 1.2
        logit = blob.contiguous()
        tensor_out = torch.empty((3, S, S), dtype=torch.float32, device=dev)
        grey_a, grey_b = torch.empty((S, S), dtype=torch.uint8, device=dev), torch.empty((S, S), dtype=torch.uint8, device=dev)
        full_a, full_b = torch.empty((h, w), dtype=torch.uint8, device=dev), torch.empty((h, w), dtype=torch.uint8, device=dev)
        lp, tp, ga, gb, fa, fb = logit.data_ptr(), tensor_out.data_ptr(), grey_a.data_ptr(), grey_b.data_ptr(), full_a.data_ptr(), full_b.data_ptr()
        post_bytes = 8 + 4 * spx / px   # the layer read and written, the model's output read

        def composed(ms):
            a, b = ga, gb
            r.matte_byte_dev(lp, S, S, ms, a, is_probability=0)
            for e in (ms.mask_expansion, ms.fill_holes, -ms.fill_holes):
                if e:
                    r.matte_expand_dev(a, S, S, e, b)
                    a, b = b, a
            r.matte_resize_dev(a, S, S, fa, w, h)
            r.matte_feather_dev(fa, w, h, ms.edge_feather, fb)
            r.matte_apply_dev(s, fb, w, h, d)

        stage_timers = ["matte_byte", "matte_expand", "matte_resize", "matte_feather", "matte_apply"]
        timed("matte yardstick: invert", ["adjust"], lambda: r.adjust_dev(s, d, w, h, "invert"), px, 8, "8 B/px on the same buffers, the same run")
        timed("matte: tensor, 8K -> 3 x 1024 x 1024 f32", ["resize", "matte_tensor"], lambda: r.matte_tensor_dev(s, w, h, S, tp), px, 4 + 12 * spx / px,
              "the RGBA Lanczos3 resize (a 7.5 x reduction: two passes through an f32 intermediate) and the table pass")
        timed("matte: score of one 1024 x 1024 output", ["matte_score"], lambda: r.matte_score_dev(lp, spx), spx, 4, "an f64 expf per value; the call waits for 16 bytes")
        timed("matte: score of five outputs", ["matte_score"], lambda: [r.matte_score_dev(lp, spx) for _ in range(5)], 5 * spx, 4)
        for label, ms in (("defaults", matte_settings()), ("Portrait (feather 1, expansion 1, close 8)", matte_settings(0.5, 1.0, 1, True, 8)),
                          ("feather 20", matte_settings(0.5, 20.0, 0, True, 0))):
            timed(f"matte: postprocess, {label}", ["matte_postprocess"], lambda ms=ms: r.matte_postprocess_dev(lp, S, S, s, w, h, ms, d, is_probability=0), px, post_bytes)
            timed(f"matte: stage calls composed, {label}", stage_timers, lambda ms=ms: composed(ms), px, post_bytes, "the matte written and read once more (feather: twice)")
        del logit, blob, tensor_out, grey_a, grey_b, full_a, full_b, yy, xx
    # ---------------- removal by colour (k_colorkey.hip): colour to alpha is a streaming pass like HSL; the colour remover is the passability map, the connected
    # flood's passes (contiguous scope) and ceil(smoothness / 32) ring launches, the last one writing the image.  The HSL row and the bucket tool's flood of the
    # same image are repeated under this section's name so that one `--only colorkey` run holds them side by side
    timed("colorkey: colour to alpha, defaults", ["color_to_alpha"], lambda: r.color_to_alpha_dev(s, d, w, h, (128, 128, 128)), px, 8, "up to five IEEE divisions per changed pixel")
    timed("colorkey: colour to alpha, masked", ["color_to_alpha"], lambda: r.color_to_alpha_dev(s, d, w, h, (128, 128, 128), mask_ptr=m), px, 9)
    timed("colorkey orientation: hsl(30,-20,10)", ["adjust"], lambda: r.adjust_dev(s, d, w, h, "hsl", [30.0, -20.0, 10.0]), px, 8, "the same 8 B/px")
    ck = torch.empty((h, w, 4), dtype=torch.uint8, device=dev)
    ckd = torch.empty((h, w), dtype=torch.uint8, device=dev)

    def build_ck_photo():   # smooth ramps of a few units per hundred pixels under +-4 noise: a tolerance cuts ragged regions, the rings have an edge to follow
        yy, xx = torch.meshgrid(torch.arange(h, device=dev), torch.arange(w, device=dev), indexing="ij")
        base = torch.stack([120 + 40 * torch.sin(xx / 900.0) * torch.cos(yy / 700.0), 110 + 50 * torch.cos(xx / 1300.0 + yy / 500.0), 90 + 30 * torch.sin((xx + yy) / 1100.0)], dim=2)
        ck[..., :3] = (base + torch.randint(-4, 5, (h, w, 3), device=dev, generator=g)).clamp(0, 255).to(torch.uint8)
        ck[..., 3] = 255

    def build_ck_uniform():
        ck[...] = torch.tensor(grey, dtype=torch.uint8, device=dev)

    for image, build in (("photo-like", build_ck_photo), ("uniform", build_ck_uniform)):
        if args.only and "colorkey" not in args.only:   # the images cost more than a skipped row
            break
        build()
        torch.cuda.synchronize()
        seed_px = tuple(int(v) for v in ck[h // 2, w // 2].tolist())
        flood = lambda: r.flood_distance_dev(ck.data_ptr(), w, h, (w // 2, h // 2), seed_px, ckd.data_ptr(), "legacy", 4, False)
        flood()
        timed(f"colorkey orientation: bucket tool's connected flood, {image}", ["flood_distance"], flood, px, 5, reps=3, warm=False,
              note=f"the flood of profiles/flood.md on this image from its centre: {r.flood_last(0)} passes, {r.flood_last(3)} tile visits (it floods on a 0..255 distance, the remover on passable / not)")
        for contiguous in (True, False):
            for smooth in (0, 3, 20, 64):
                run = lambda: r.color_removal_dev(ck.data_ptr(), d, w, h, (w // 2, h // 2), 8.0, smooth, contiguous)
                run()
                timed(f"colorkey: remover, {image}, {'contiguous' if contiguous else 'global'}, smoothness {smooth}", ["color_removal"], run, px, 14, reps=3, warm=False,
                      note=f"seed at the centre, tolerance 8: {r.colorkey_last(0)} flood passes, {r.colorkey_last(1)} ring launches, {r.colorkey_last(4)} launches; 14 B/px = the map (4 + 1) "
                           f"and the last launch (1 + 4 + 4), the flood's and the earlier ring launches' traffic not counted; the timer starts after the seed's read-back; mean of 3 calls")
    del ck, ckd
    # ---------------- the floating selection (k_overlay.hip): commit is a gather of four taps plus the document pixel read and written in place; the affine
    # transform (bilinear) is the existing kernel nearest to it — a four-tap gather and one write — and runs beside it at the same size and angle
    from paintfe_amd import overlay
    full = dict(source_size=(w, h), doc_size=(w, h), center=(w / 2.0, h / 2.0))
    ov_rot = overlay(rotation=0.3, **full)
    timed("overlay: commit, full-canvas source, rotation 0.3, anti-aliased, blend", ["overlay_commit"], lambda: r.overlay_commit_dev(ov_rot, s, d, d), px, 12,
          "in place; 12 B/px = 4 gathered (four taps, mostly cached) + 4 read + 4 written, over the whole canvas although the rotated box's corners hold no sample; random alpha: nearly every pixel takes the general blend with its division")
    timed("overlay orientation: affine transform, bilinear, rotation_z 0.3 rad, same size", ["affine"],
          lambda: r.affine_transform_dev(s, w, h, d, w, h, rotation_z=math.degrees(0.3)), px, 8, "4 gathered + 4 written")
    ov_flat = overlay(rotation=0.3, anti_aliasing=False, overwrite_transparent=True, **full)
    timed("overlay: commit, rotation 0.3, no anti-aliasing, overwrite", ["overlay_commit"], lambda: r.overlay_commit_dev(ov_flat, s, d, d), px, 8, "one tap, no blend: 4 gathered + 4 written")
    timed("overlay: preview, rotation 0.3 (the general path)", ["overlay_preview"], lambda: r.overlay_preview_dev(ov_rot, s, d), px, 8, "every drag frame: one nearest tap, the whole canvas written")
    ov_move = overlay(source_size=(w, h), doc_size=(w, h), center=(w / 2.0 + 301.0, h / 2.0 - 77.0))
    timed("overlay: preview, translation only", ["overlay_preview"], lambda: r.overlay_preview_dev(ov_move, s, d), px, 8)
    ov_clip, ov_cmask = torch.empty_like(src), torch.empty_like(mask)
    timed("overlay: extract through a 70 % selection", ["overlay_extract"], lambda: r.overlay_extract_dev(d, m, w, h, ov_clip.data_ptr(), ov_cmask.data_ptr()), px, 19,
          "lift (1 + 4 read, 4 + 1 written) + the grey-aware delete (1 + 4 read, 4 written where selected); the bounds launch and its read-back come before the timer")
    del ov_clip, ov_cmask
    # ---------------- the text layer's styles (k_textfx.hip).  The disc maximum alone (an outline whose other stages are one compose pass, timed apart) at two
    # radii: the discs hold 81 and 7 845 taps, the span walk reads at most 4 (2 r + 1) bytes of LDS per pixel.  Then the default style on the whole canvas
    # beside the three existing calls nearest to its stages, and on a 1 500 x 400 block of text inside the same canvas (the region rule)
    from paintfe_amd import text_effects
    for radius in (5.0, 50.0):
        fx_o = text_effects((w, h), outline=dict(width=radius))
        timed(f"text styles: disc maximum, r = {radius:g}", ["textfx_disc"], lambda: r.text_effects_dev(fx_o, s, d), px, 2,
              "1 read (the alpha of an RGBA8 pixel: 4 B fetched) + 1 written; the compose pass behind it is not in this row")
    tfx_timers = ["textfx_bounds", "textfx_crop", "textfx_plane", "textfx_disc", "gauss_plane", "gauss_fused", "gauss_mfma", "gauss_h", "gauss_v", "textfx_compose", "textfx_blit"]
    fx_d = text_effects((w, h), outline={}, shadow={}, inner_shadow={})
    timed("text styles: defaults (shadow 4, 4, 5, 0; outline 2 outside; inner shadow 2, 2, 3), whole canvas", tfx_timers, lambda: r.text_layer_effects_dev(fx_d, s, d), px, 8,
          "random alpha everywhere: the tight bounds are the canvas; the bounds launch's read-back is a wait on the host and not in the timers")
    if rows and rows[-1]["op"].startswith("text styles: defaults"):
        for name in tfx_timers:
            print("   ", name, round(r.timing_read(name)[0] / args.reps, 4), "ms", flush=True)
    r.set_exact(True)
    timed("text styles' nearest existing calls: drop shadow blur=5 + outline width=2 + gaussian sigma=3 (exact)",
          ["shadow_alpha", "gauss_plane", "gauss_mfma", "gauss_fused", "gauss_h", "gauss_v", "shadow_composite", "outline"],
          lambda: (r.shadow_dev(s, d, w, h, 4, 4, 5.0, False, (0, 0, 0, 180), 1.0), r.outline_dev(s, d, w, h, 2, (0, 0, 0, 255)), r.gaussian_blur_dev(s, d, w, h, 3.0, t)), px, 24)
    r.set_exact(False)
    block = torch.zeros_like(src)
    block[2000:2400, 3000:4500] = src[2000:2400, 3000:4500]
    timed("text styles: defaults, a 1 500 x 400 text block on the 8K canvas (the region path)", tfx_timers, lambda: r.text_layer_effects_dev(fx_d, block.data_ptr(), d), px, 8,
          "the bounds pass reads the canvas, the effects run on 1 546 x 446, the canvas is zeroed and the region blitted; Mpx_s and GB/s are per canvas pixel")
    del block
    # ---------------- the text block's warps and placement (k_textwarp.hip): each warp at its largest ordinary frame (path and envelope clamp at 4096 x 4096, the
    # arc's sides stay below 8192, the circle's square is 2 (r + h) + 4), the rotation and the placement on the 8K canvas; px = output pixels.  The
    # displacement warp runs at the envelope's pixel count beside it: the envelope reads no field, so it must not be the slower one (profiles/text_warp.md)
    from paintfe_amd import text_block, text_rotate_plan, text_warp, text_warp_plan

    def warp_row(label, size, timer, note, **fields):
        wd = text_warp(size, **fields)
        gm = text_warp_plan(wd)
        raster = torch.randint(0, 256, (size[1], size[0], 4), dtype=torch.uint8, device=dev, generator=g)
        timed(f"text warp: {label}, {size[0]} x {size[1]} -> {gm.out_w} x {gm.out_h}", [timer], lambda: r.text_warp_dev(wd, raster.data_ptr(), d), gm.out_w * gm.out_h, 8, note)
        return gm

    gm_env = warp_row("envelope", (4088, 4088), "textwarp_envelope", "4 gathered + 4 written; t, top_y and span once per column and workgroup", kind="envelope",
                      top_curve=[(0.0, 60.0), (1363.0, -20.0), (2725.0, -20.0), (4088.0, 60.0)], bottom_curve=[(0.0, 4028.0), (1363.0, 4108.0), (2725.0, 4108.0), (4088.0, 4028.0)])
    ew, eh = gm_env.out_w, gm_env.out_h
    e_disp = torch.empty((eh, ew, 2), dtype=torch.float32, device=dev)
    e_yy = torch.arange(eh, device=dev, dtype=torch.float32)[:, None]
    e_xx = torch.arange(ew, device=dev, dtype=torch.float32)[None, :]
    e_disp[..., 0] = 40.0 * torch.sin(e_yy / 300.0) * torch.cos(e_xx / 500.0)
    e_disp[..., 1] = 40.0 * torch.cos(e_yy / 400.0) * torch.sin(e_xx / 350.0)
    del e_yy, e_xx
    timed(f"text warp's yardstick: liquify displacement warp, {ew} x {eh}", ["warp_displacement"], lambda: r.warp_displacement_dev(s, ew, eh, e_disp.data_ptr(), ew, eh, d),
          ew * eh, 16, "4 + 8 (field) + 4 B/px at the envelope row's pixel count")
    del e_disp
    warp_row("path follow", (3900, 64), "textwarp_path", "65 distances + 17 Bézier evaluations per pixel; most of the frame is far from the text", kind="path",
             control_points=[(0.0, 0.0), (2000.0, 0.0), (2000.0, 3900.0), (4000.0, 3900.0)])
    warp_row("arc, bend 0.5", (6500, 1000), "textwarp_arc", "f64 atan2 per pixel whose sy is inside the text", kind="arc", bend=0.5)
    warp_row("circular, r = 1800", (8000, 200), "textwarp_circular", "f64 atan2 inside the annulus only", kind="circular", radius=1800.0)
    gm_rot = text_rotate_plan(w, h, 0.3)
    rot_out = torch.empty((gm_rot.out_h, gm_rot.out_w, 4), dtype=torch.uint8, device=dev)
    timed(f"text rotate: the 8K canvas by 0.3 -> {gm_rot.out_w} x {gm_rot.out_h}", ["textwarp_rotate"], lambda: r.text_rotate_dev(w, h, 0.3, s, rot_out.data_ptr()),
          gm_rot.out_w * gm_rot.out_h, 8)
    del rot_out
    place_timers = ["textwarp_arc", "textwarp_rotate", "textwarp_blit"]
    blk_small = text_block(text_warp((1500, 400), kind="arc", bend=0.5), (3000, 2000), (w, h), rotation=0.3)
    timed("text place: a 1 500 x 400 block, arc 0.5, rotated 0.3, into the 8K canvas", place_timers, lambda: r.text_block_place_dev(blk_small, s, d), 1500 * 400, 8,
          "three launches on the block's own pixels; Mpx_s per source pixel")
    blk_full = text_block(text_warp((w, h), kind="none"), (0, 0), (w, h), rotation=0.3)
    canvas2 = torch.zeros_like(src)
    timed("text place: an 8K raster rotated 0.3 into the 8K canvas", place_timers, lambda: r.text_block_place_dev(blk_full, s, canvas2.data_ptr()), px, 12,
          "rotate (4 + 4 B per rotated pixel) and blit (4 read, 4 written where alpha > 0); Mpx_s per canvas pixel")
    del canvas2
    # ---------------- the gradient tool and the perspective crop (k_gradient.hip), 8K, device-resident.  The render only writes (4 B/px; 5 with a selection), so a
    # memset of one frame runs beside it; commit and the fused apply read and write the layer (12 and 8 B/px) beside invert (8 B/px); the crop is a four-tap
    # gather and one write per layer beside the bilinear affine transform.  No time here is an acceptance criterion (profiles/gradient.md)
    if not args.only or "gradient" in args.only:
        import ctypes as C

        from paintfe_amd import gradient, gradient_drag_scale, gradient_lut, perspective_crop_plan
        g_lut = gradient_lut([(0.0, (255, 0, 0, 255)), (0.3, (0, 255, 0, 0)), (0.35, (0, 0, 255, 0)), (0.7, (10, 20, 200, 128)), (1.0, (255, 255, 255, 255))])
        g_ends = ((w * 0.31 + 0.3, h * 0.24 + 0.2), (w * 0.52 + 0.7, h * 0.71 + 0.4))
        pm = torch.empty_like(src)
        for shape in ("linear", "linear_reflected", "radial", "diamond"):
            gd = gradient(*g_ends, shape=shape, repeat=True)
            timed(f"gradient: render, {shape}, repeat, full resolution", ["gradient_render"], lambda: r.gradient_render_dev(gd, g_lut, w, h, d), px, 4, "write only: one 16-byte store per lane")
        gd = gradient(*g_ends, shape="linear", repeat=True)
        timed("gradient: render, linear, with a 70 % selection", ["gradient_render"], lambda: r.gradient_render_dev(gd, g_lut, w, h, d, selection_ptr=m), px, 5)
        timed("gradient: render, linear, with the premultiplied copy", ["gradient_render"], lambda: r.gradient_render_dev(gd, g_lut, w, h, d, premul_ptr=pm.data_ptr()), px, 8,
              "the fast path's preview_flat_buffer: a second 16-byte store")
        drag = gradient_drag_scale(w, h)
        gdrag = gradient(*g_ends, shape="linear", repeat=True, preview_scale=drag)
        gen_px = -(-w // drag) * -(-h // drag)
        timed(f"gradient: render at the drag scale {drag} ({-(-w // drag)} x {-(-h // drag)})", ["gradient_render"], lambda: r.gradient_render_dev(gdrag, g_lut, w, h, d), gen_px, 4,
              "what a drag frame costs; Mpx_s per generated pixel")
        r.gradient_render_dev(gd, g_lut, w, h, pm.data_ptr())
        timed("gradient: commit, colour mode", ["gradient_commit"], lambda: r.gradient_commit_dev(d, pm.data_ptr(), w, h, False), px, 12,
              "4 preview + 4 layer read, 4 written; the layer converges over the repetitions (it is committed onto again)")
        timed("gradient: commit, transparency mode", ["gradient_commit"], lambda: r.gradient_commit_dev(d, pm.data_ptr(), w, h, True), px, 12)
        timed("gradient: fused apply (render + commit), colour mode", ["gradient_apply"], lambda: r.gradient_apply_dev(gd, g_lut, d, w, h), px, 8, "4 read + 4 written, no preview buffer")
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        memset = lambda: r._lib.pfx_dev_memset(r.handle, C.c_void_p(d), C.c_int(0), C.c_size_t(px * 4))
        for _ in range(20):
            memset()
        ev0.record()
        for _ in range(args.reps):
            memset()
        ev1.record()
        torch.cuda.synchronize()
        ms = ev0.elapsed_time(ev1) / args.reps
        rows.append({"op": "gradient orientation: pfx_dev_memset of one 8K frame", "ms": round(ms, 4), "Mpx_s": round(px / ms / 1e3, 1), "alg_bytes_px": 4,
                     "achieved_GBs": round(4 * px / (ms * 1e-3) / 1e9, 1), "hbm_frac": round(4 * px / (ms * 1e-3) / 1e9 / HBM_PEAK, 4),
                     "note": "the write-only yardstick; stream events around the calls (the memset has no pfx_timing scope)"})
        print(rows[-1], flush=True)
        timed("gradient orientation: invert", ["adjust"], lambda: r.adjust_dev(s, d, w, h, "invert", []), px, 8, "the 8 B/px yardstick for commit and apply")
        quad = [(w * 0.08 + 0.3, h * 0.08), (w * 0.9 + 0.2, h * 0.18), (w * 0.87 + 0.1, h * 0.92), (w * 0.11 + 0.7, h * 0.84)]
        cw, ch = perspective_crop_plan(quad, w, h)
        crop_in = [src] + [torch.randint(0, 256, (h, w, 4), dtype=torch.uint8, device=dev, generator=g) for _ in range(3)]
        crop_out = [torch.empty((ch, cw, 4), dtype=torch.uint8, device=dev) for _ in range(4)]
        for n in (1, 4):
            ins, outs = [t_.data_ptr() for t_ in crop_in[:n]], [t_.data_ptr() for t_ in crop_out[:n]]
            timed(f"gradient: perspective crop of {n} layer{'s' if n > 1 else ''}, 8K -> {cw} x {ch}", ["perspective_crop"], lambda: r.perspective_crop_dev(quad, ins, outs, w, h),
                  cw * ch * n, 8, "4 gathered + 4 written per layer and output pixel; Mpx_s counts every layer's pixels")
        timed("gradient orientation: affine transform, bilinear, rotation_z 0.3 rad, 8K", ["affine"],
              lambda: r.affine_transform_dev(s, w, h, d, w, h, rotation_z=math.degrees(0.3)), px, 8, "the four-tap yardstick for the crop")
        del pm, crop_in, crop_out
    src_h = src.cpu().numpy()
    import time
    r.execute_script_sync("map_channels(|r, g, b, a| [255 - r, g / 2, (b * 3 + a) / 4, a]);", src_h)   # warm: a process's first launch of k_script's code object loads it (~1 ms)
    r.timing_reset()
    r.timing_enable(True)
    t0 = time.perf_counter()
    r.execute_script_sync("map_channels(|r, g, b, a| [255 - r, g / 2, (b * 3 + a) / 4, a]);", src_h)
    wall = (time.perf_counter() - t0) * 1e3
    r.timing_enable(False)
    vm_ms = r.timing_read("script_vm")[0]
    rows.append({"op": "script: map_channels closure at 8K (bytecode VM kernel)", "ms": round(vm_ms, 4), "Mpx_s": round(px / vm_ms / 1e3, 1), "alg_bytes_px": 8,
                 "achieved_GBs": round(8 * px / (vm_ms * 1e-3) / 1e9, 1), "hbm_frac": round(8 * px / (vm_ms * 1e-3) / 1e9 / HBM_PEAK, 4),
                 "note": f"pfx_script_execute wall clock incl. H2D/D2H of 133 MB each way and closure compile: {wall:.0f} ms"})
    print(rows[-1], flush=True)
    del src_h
    del tmp, mask
    # ---------------- compositor, one blend mode at a time: 8 layers of the same mode over an opaque background (8K)
    from paintfe_amd import BLEND_MODES
    nl = 9
    layers = [src] + [torch.randint(0, 256, (h, w, 4), dtype=torch.uint8, device=dev, generator=g) for _ in range(nl - 1)]
    layers[0][..., 3] = 255
    ptrs = [t_.data_ptr() for t_ in layers]
    for m, name in enumerate(BLEND_MODES):
        info = [(0, 1.0, True, 0)] + [(k, 0.8, True, m) for k in range(1, nl)]
        timed(f"flatten 9 layers, mode {m} {name}", ["flatten"], lambda: r.flatten_dev(ptrs, info, w, h, d), px, 4 * nl + 4,
              f"{(nl - 1)} blends/px")
    del layers, src, dst

    # ---------------- 4K per-image pipeline of config 5 / S4: Gaussian sigma=4 -> HSL -> 4-layer flatten (image + 3 overlays)
    w, h = 3840, 2160
    px = w * h
    img = torch.randint(0, 256, (h, w, 4), dtype=torch.uint8, device=dev, generator=g)
    overlays = [torch.randint(0, 256, (h, w, 4), dtype=torch.uint8, device=dev, generator=g) for _ in range(3)]
    a = torch.empty_like(img)
    b = torch.empty_like(img)
    tmp4 = torch.empty((h, w, 4), dtype=torch.float32, device=dev)
    info4 = [(0, 1.0, True, 0), (1, 0.8, True, 1), (2, 0.8, True, 2), (3, 0.8, True, 8)]  # Normal, Multiply, Screen, Overlay

    def pipeline():
        r.gaussian_blur_dev(img.data_ptr(), a.data_ptr(), w, h, 4.0, tmp4.data_ptr())
        r.adjust_dev(a.data_ptr(), b.data_ptr(), w, h, "hsl", [30.0, -20.0, 10.0])
        r.flatten_dev([b.data_ptr()] + [o.data_ptr() for o in overlays], info4, w, h, a.data_ptr())
    timed("config-5 per-image pipeline at 4K (blur s=4 + HSL + 4-layer flatten)", ["gauss_mfma", "adjust", "flatten"], pipeline, px, 36,
          "8 + 8 + 20 algorithmic B/px; images/s = 1000 / ms")
    for name in ("gauss_mfma", "adjust", "flatten"):
        print("   ", name, round(r.timing_read(name)[0] / args.reps, 4), "ms", flush=True)
    del img, overlays, a, b, tmp4

    # ---------------- brush stamp loop on a device-resident 8K preview layer (A13): px = stamped pixel visits (stamps x pi r^2)
    w, h = 7680, 4320
    tgt = torch.zeros((h, w, 4), dtype=torch.uint8, device=dev)

    def line(p0, p1):   # draw_line_no_dirty's dense 1-px stepping (brush_render.rs:762-835)
        n = int(max(abs(p1[0] - p0[0]), abs(p1[1] - p0[1]))) + 1
        t = np.linspace(0.0, 1.0, n, dtype=np.float32)
        return np.stack([p0[0] + (p1[0] - p0[0]) * t, p0[1] + (p1[1] - p0[1]) * t], axis=1)
    tt = np.linspace(0, 40 * np.pi, 4000, dtype=np.float32)
    scribble = np.stack([3800 + 1200 * np.cos(tt * 0.37) * np.sin(tt * 0.11 + 1.0), 2100 + 1200 * np.sin(tt * 0.53) * np.cos(tt * 0.07)], axis=1).astype(np.float32)
    for name, b, pts in (("brush: mouse segment, 60 stamps, size 50", r.make_brush(50.0, 0.75, True, (0.8, 0.2, 0.1, 1.0)), line((3000, 2000), (3059, 2010))),
                         ("brush: diagonal stroke, 6501 stamps, size 100", r.make_brush(100.0, 0.75, True, (0.1, 0.2, 0.9, 1.0)), line((500, 500), (7000, 3800))),
                         ("brush: scribble, 4000 stamps, size 120", r.make_brush(120.0, 0.5, True, (0.1, 0.7, 0.2, 0.8)), scribble),
                         ("brush: dodge, diagonal stroke, size 100", r.make_brush(100.0, 0.75, True, (1, 1, 1, 1.0), mode=1), line((500, 500), (7000, 3800)))):
        timed(name, ["brush_stamps"], lambda: r.brush_stamps_dev(tgt.data_ptr(), w, h, b, pts), int(len(pts) * np.pi * (b.size / 2) ** 2), 0,
              "kernel only (the call adds the host prologue and the stamp upload, ~0.03-0.06 ms); Mpx_s = stamped pixel visits (a pixel stays in its lane's register across the stamps: no HBM figure); strokes of > 64 stamps are dealt to 64 x 64 chunks")
    # ---------------- clone stamp, heal ring, release (k_dabtools.hip) on the same 8K preview, beside the brush's binned walk over the SAME dab list: the yardstick
    # is the walk without a source gather.  px = stamped pixel visits as above.  The heal stroke at two steppings shows that the ring is evaluated per pixel, not
    # per dab: halving the step doubles the walk and leaves the ring alone.  No time here is an acceptance criterion (profiles/dab_tools.md)
    if not args.only or "dabtools" in args.only:
        from paintfe_amd import clone_stamp_tool, heal_ring_tool
        lay = torch.randint(0, 256, (h, w, 4), dtype=torch.uint8, device=dev, generator=g)
        p0, p1 = (500.3, 700.2), (2499.3, 1100.7)
        steps = {1.0: np.linspace(0.0, 1.0, 2000, dtype=np.float32), 0.5: np.linspace(0.0, 1.0, 3999, dtype=np.float32)}
        strokes = {k: np.stack([p0[0] + (p1[0] - p0[0]) * t_, p0[1] + (p1[1] - p0[1]) * t_], axis=1) for k, t_ in steps.items()}
        frame = strokes[1.0][1000:1016]
        clone, heal = clone_stamp_tool(100.0, 0.75, True, (300.5, -200.5)), heal_ring_tool(100.0, 0.75, 30.0)
        brush = r.make_brush(100.0, 0.75, True, (0.1, 0.2, 0.9, 1.0))
        visits = lambda pts: int(len(pts) * np.pi * 50.0 ** 2)
        note = "kernel only; the preview keeps the previous repetition's stroke, so every dab ties with what is there and writes again"
        for label, pts in (("2000-dab stroke, stepping 1 px", strokes[1.0]), ("3999-dab stroke, stepping 0.5 px", strokes[0.5]), ("drag frame of 16 dabs", frame)):
            timed(f"dabtools: clone stamp, size 100, {label}", ["clone_stamp"], lambda: r.clone_stamp_dev(clone, lay.data_ptr(), tgt.data_ptr(), w, h, pts), visits(pts), 0, note)
            timed(f"dabtools: heal ring, size 100, sample_radius 30, {label}", ["heal_ring"], lambda: r.heal_ring_dev(heal, lay.data_ptr(), tgt.data_ptr(), w, h, pts), visits(pts), 0,
                  note + "; 24 f64 cos + sin and 48 gathers per written pixel, once")
            timed(f"dabtools yardstick: brush, size 100, {label}", ["brush_stamps"], lambda: r.brush_stamps_dev(tgt.data_ptr(), w, h, brush, pts), visits(pts), 0,
                  "the same dab list through pfx_brush_stamps_ex_dev (binned above 64 stamps): the walk without a source")
        timed("dabtools: stroke commit (release), Normal, 8K", ["stroke_commit"], lambda: r.stroke_commit_dev(lay.data_ptr(), tgt.data_ptr(), w, h), w * h, 4,
              "pfxk_brush_commit on device memory: the preview is read everywhere (4 B/px, and one 8K frame stays in the Infinity Cache between repetitions); "
              "the layer is read and written only under the stroke")
        del lay
    del tgt

    # ---------------- line / curve tool (k_linetool.hip): one drag frame of a 4K canvas diagonal — the focused clear with the frame's own bounds, the dots, the
    # arrowheads — beside the brush's binned walk over the SAME number of stamps at the dots' places.  px = dot pixel visits (dots x the dot's box).  The note
    # carries the dot count, the chunk-list entries and the call's wall-clock time, host prologue and uploads included.  No time is an acceptance criterion
    # (profiles/line_tool.md)
    if not args.only or "linetool" in args.only:
        import time

        from paintfe_amd import line_bounds, line_plan, line_tool
        from tests import linetool_model as LM
        lw, lh = 3840, 2160
        pv = torch.zeros((lh, lw, 4), dtype=torch.uint8, device=dev)
        p = [(40.5, 30.25), (1300.0, 700.0), (2500.0, 1500.0), (3800.5, 2130.75)]
        for size in (1.0, 12.0, 60.0):
            for label, opts in (("solid, arrows both", dict(end_shape="arrow", arrow_side="both")), ("dashed", dict(pattern="dashed"))):
                tool = line_tool(p, size, (30, 90, 220, 255), **opts)
                dots, tris = line_plan(tool, lw, lh)
                boxes = [LM.dot_box(x, y, np.float32(size) / np.float32(2), True, lw, lh) for x, y in dots]
                entries = sum((b[1] // 64 - b[0] // 64 + 1) * (b[3] // 64 - b[2] // 64 + 1) for b in boxes if b)
                visits = sum((b[1] - b[0] + 1) * (b[3] - b[2] + 1) for b in boxes if b)
                last = line_bounds(tool, lw, lh)
                frame = lambda: r.line_render_dev(tool, pv.data_ptr(), lw, lh, last)
                for _ in range(5):
                    frame()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(20):
                    frame()
                    torch.cuda.synchronize()
                wall = (time.perf_counter() - t0) / 20 * 1e3
                timed(f"linetool: 4K diagonal drag frame, size {size:g}, {label}", ["line_render"], frame, visits, 0,
                      f"kernel only; {len(dots)} dots, {len(tris)} arrowheads, {entries} chunk-list entries; the whole call, synchronised: {wall:.3f} ms")
                nothing = (0.0, 0.0, 0.0, 0.0)   # bounds that clear no chunk: the dots and arrowheads alone, over the chunks they touch
                timed(f"linetool: the same frame without a clear, size {size:g}, {label}", ["line_render"], lambda: r.line_render_dev(tool, pv.data_ptr(), lw, lh, nothing), visits, 0,
                      "kernel only; the diagonal's bounds cover the canvas, so the frame above clears every chunk of it: the difference is that clear")
                brush = r.make_brush(size, 0.95, True, (0.1, 0.35, 0.86, 1.0))
                timed(f"linetool yardstick: brush, size {size:g}, the {len(dots)} stamps of '{label}'", ["brush_stamps"],
                      lambda: r.brush_stamps_dev(pv.data_ptr(), lw, lh, brush, dots), visits, 0, "pfx_brush_stamps_ex_dev at the dots' places: no clear, no arrowheads")
        conceal = torch.zeros((lh, lw), dtype=torch.uint8, device=dev)
        timed("linetool: mask-target release, 4K", ["stroke_commit_mask"], lambda: r.stroke_commit_mask_dev(conceal.data_ptr(), pv.data_ptr(), lw, lh), lw * lh, 4,
              "the preview's alpha is read everywhere; the conceal bytes are read and written only under the line")
        del pv, conceal

    # ---------------- 16K (config 4: mesh warp 6x6 Catmull-Rom + liquify displacement)
    w, h = 15360, 8640
    px = w * h
    src = torch.randint(0, 256, (h, w, 4), dtype=torch.uint8, device=dev, generator=g)
    dst = torch.empty_like(src)
    orig, deformed = I.jittered_mesh(6, 6, w, h)
    s, d = src.data_ptr(), dst.data_ptr()
    timed("mesh warp 6x6 fused (16K)", ["warp_mesh"], lambda: r.warp_mesh_catmull_rom_dev(s, orig, deformed, 6, 6, w, h, d), px, 8,
          "field never materialised")
    disp = torch.empty((h, w, 2), dtype=torch.float32, device=dev)
    # smooth liquify-like field: sum of a few Gaussian pushes, built with torch (input data, not the product path)
    yy = torch.arange(h, device=dev, dtype=torch.float32)[:, None]
    xx = torch.arange(w, device=dev, dtype=torch.float32)[None, :]
    fx = torch.zeros((h, w), device=dev)
    fy = torch.zeros((h, w), device=dev)
    rng = np.random.default_rng(0x5EED0004)
    for _ in range(16):
        cx, cy = rng.random() * w, rng.random() * h
        ddx, ddy = (rng.random() * 2 - 1) * 60, (rng.random() * 2 - 1) * 60
        wgt = torch.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * (400.0 / 3) ** 2)) * 0.8
        fx += ddx * wgt
        fy += ddy * wgt
    timed("mesh displacement field 6x6 (16K, B3: generate_displacement_from_mesh)", ["mesh_displacement"],
          lambda: r.mesh_displacement_dev(orig, deformed, 6, 6, w, h, disp.data_ptr()), px, 8, "writes the 8 B/px f32 field the fused warp never materialises")
    disp[..., 0] = fx
    disp[..., 1] = fy
    del fx, fy, yy, xx
    rngd = np.random.default_rng(7)
    dabs = [(int(m), float(rngd.uniform(2000, w - 2000)), float(rngd.uniform(1500, h - 1500)), float(rngd.uniform(-20, 20)), float(rngd.uniform(-20, 20)), 400.0, 0.6)
            for m in (0, 1, 2, 3, 4, 0, 0, 0) * 4]
    fld = torch.zeros((h, w, 2), dtype=torch.float32, device=dev)
    timed("liquify dabs into the field: 32 dabs, radius 400 (16K)", ["displacement_brush"], lambda: r.displacement_brushes_dev(fld.data_ptr(), w, h, dabs),
          int(32 * np.pi * 400 * 400), 0, "DisplacementField::apply_* on the device-resident field (N4): Mpx_s = dab pixel visits")
    del fld
    timed("liquify displacement warp (16K)", ["warp_displacement"], lambda: r.warp_displacement_dev(s, w, h, disp.data_ptr(), w, h, d), px, 16,
          "4 + 8 (field) + 4 B/px")

    if args.out:
        json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, open(args.out, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
