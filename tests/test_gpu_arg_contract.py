"""The argument contract of every entry point that takes an image or a mask (include/pfx.h), pinned call by call: which arguments are refused with
PFX_ERR_INVALID, which aliasing is allowed, and that a refused call touches no buffer.

The prototypes are parsed from the header (as tests/test_abi_hostile.py does); TABLE below names the entry points and says, per entry point, what each
pointer is (an RGBA8 image, a one-byte mask, a displacement field; input, output or both; required or optional) and what differs from the defaults.  Every
other pointer gets a small zeroed host block, every other scalar the value 1, every dimension the 67 x 5 image (odd width above 64, w * h no multiple of 4).

Per entry point:
  * the valid call returns PFX_OK (so that every refusal below is a refusal of the one thing that was changed);
  * each required pointer NULL in turn, w = 0, h = 0 and 20000 x 20000 (over the 256 Mpx document limit) are PFX_ERR_INVALID;
  * each output moved to overlap each other buffer by all but 16 bytes is PFX_ERR_INVALID — unless the pair is in the entry point's `accepts`: overlaps that
    the library has never refused (the host-buffer tier of the filter, warp, brush and resize calls works on staged copies; the filter, effect, brush and
    shape `_dev` calls do not look at the mask).  pfx.h promises nothing about those; they are pinned here as they are;
  * the documented in-place pair (output == input) is PFX_OK where pfx.h allows it and PFX_ERR_INVALID where it does not;
  * a device pointer one byte off a dword is PFX_ERR_INVALID for the calls whose pfx.h text says so (the flood, selection fill / delete and colour-removal
    `_dev` calls) — it is never handed to a call that might launch with it;
  * after the refused calls both arenas, the device's and the host's, are byte for byte what they were.

Every buffer is a 4 KiB slot of one arena (one device allocation, one host array) with spare slots behind the last one, so an accepted call with moved
pointers stays inside the allocation."""
import ctypes as C
import re

import numpy as np
import pytest
import torch  # noqa: F401  -- before libpfx.so is loaded (see test_gpu_fullsize.py)

from paintfe_amd import _lib
from .test_abi_hostile import SCALARS, prototypes

pytestmark = pytest.mark.gpu

W, H = 67, 5
SLOT, N_SLOTS = 4096, 12
SIZES = {"rgba": W * H * 4, "mask": W * H, "disp": W * H * 8}
DIMS = {"w": W, "h": H, "sw": W, "sh": H, "new_w": W, "new_h": H, "canvas_w": W, "canvas_h": H, "src_w": W, "src_h": H, "band_rows": H}
OK, INVALID = _lib.OK, _lib.ERR_INVALID


def spec(bufs, args=None, in_place=None, accepts=(), misaligned=(), required=(), keep_dims=()):
    """bufs: 'name:kind:size ...' with kind in / out / inout / opt (an optional input); in_place: (output, input, status); accepts: (output, other) pairs whose
    overlap is not refused; misaligned: device pointers refused off a dword; required: further pointers whose NULL is refused; keep_dims: dimension pairs that
    are not zeroed (see the entry)"""
    parsed = [b.split(":") for b in bufs.split()]
    return dict(bufs={n: (k, s) for n, k, s in parsed}, args=dict(args or {}), in_place=in_place, accepts=set(accepts), misaligned=tuple(misaligned),
                required=tuple(required), keep_dims=tuple(keep_dims))


TABLE = {}
MASK_GAP = {("dst", "mask")}

# ---- filters and pointwise ops (pfx_api.cpp) ----
for name, same in (("gaussian_blur", OK), ("gaussian_blur_band", OK), ("box_blur", OK), ("box_blur_band", OK), ("median", INVALID), ("median_band", INVALID),
                   ("pixelate", INVALID), ("adjust", OK), ("chain", OK), ("tiled_roundtrip", OK)):
    has_mask = name not in ("gaussian_blur", "gaussian_blur_band", "chain", "tiled_roundtrip")
    TABLE[f"pfx_{name}_dev"] = spec("src_dev:in:rgba dst_dev:out:rgba" + (" mask_dev:opt:mask" if has_mask else ""),
                                    args={"tmp_dev": None, "first_row": 0, "op": 0, "sparse_mode": 0, "n_params": 0, "n_ops": 0},
                                    in_place=("dst_dev", "src_dev", same), accepts={("dst_dev", "mask_dev")})
HOST_FILTERS = ("blur_rgba", "brightness_contrast_rgba", "hsl_rgba", "invert_rgba", "median_rgba", "gaussian_blur_core", "box_blur_core", "median_core",
                "pixelate_core", "adjust", "auto_levels", "tiled_roundtrip")
for name in HOST_FILTERS:   # staged: the host tier of these calls has no aliasing rule
    has_mask = name in ("gaussian_blur_core", "box_blur_core", "median_core", "pixelate_core", "adjust", "auto_levels")
    TABLE[f"pfx_{name}"] = spec("src:in:rgba dst:out:rgba" + (" mask:opt:mask" if has_mask else ""), args={"op": 0, "sparse_mode": 0, "n_params": 0},
                                in_place=("dst", "src", OK), accepts={("dst", "src"), ("dst", "mask")})
TABLE["pfx_rhai_adjust_dev"] = spec("pixels_dev:inout:rgba", args={"op": 0, "n": 0})
TABLE["pfx_rhai_adjust"] = spec("pixels_inout:inout:rgba", args={"op": 0, "n_params": 0})
TABLE["pfx_chunk_populated"] = spec("src:in:rgba populated:out:mask", accepts={("populated", "src")})
# ---- warps ----
TABLE["pfx_warp_displacement_dev"] = spec("src_dev:in:rgba disp_dev:in:disp dst_dev:out:rgba", in_place=("dst_dev", "src_dev", INVALID), accepts={("dst_dev", "disp_dev")})
TABLE["pfx_warp_displacement_band_dev"] = spec("src_dev:in:rgba disp_band_dev:in:disp dst_band_dev:out:rgba", args={"first_row": 0},
                                               in_place=("dst_band_dev", "src_dev", INVALID), accepts={("dst_band_dev", "disp_band_dev")})
TABLE["pfx_warp_displacement"] = spec("src:in:rgba disp_xy:in:disp dst:out:rgba", in_place=("dst", "src", OK), accepts={("dst", "src"), ("dst", "disp_xy")})
TABLE["pfx_warp_displacement_cached"] = spec("disp_xy:in:disp dst:out:rgba", accepts={("dst", "disp_xy")})
TABLE["pfx_warp_set_source"] = spec("src:in:rgba")
GRID = {"cols": 1, "rows": 1, "orig_pts_xy": "grid", "deformed_pts_xy": "grid"}
TABLE["pfx_mesh_displacement_dev"] = spec("disp_dev:out:disp", args=GRID)
TABLE["pfx_mesh_displacement"] = spec("disp_xy_out:out:disp", args=GRID)
TABLE["pfx_warp_mesh_catmull_rom_dev"] = spec("src_dev:in:rgba dst_dev:out:rgba", args=GRID, in_place=("dst_dev", "src_dev", INVALID))
TABLE["pfx_warp_mesh_catmull_rom_band_dev"] = spec("src_dev:in:rgba dst_band_dev:out:rgba", args=dict(GRID, first_row=0), in_place=("dst_band_dev", "src_dev", INVALID))
TABLE["pfx_warp_mesh_catmull_rom"] = spec("src:in:rgba dst:out:rgba", args=GRID, in_place=("dst", "src", OK), accepts={("dst", "src")})
TABLE["pfx_displacement_brushes_dev"] = spec("disp_dev:inout:disp", args={"dabs": "disp_dab"})
# ---- brush ----
BRUSH = {"brush": "brush", "dyn": None, "points_xy": "point", "n_points": 1, "x0": 3.0, "y0": 2.0, "x1": 9.0, "y1": 2.0}
for name in ("brush_stamps", "brush_stamps_ex"):
    TABLE[f"pfx_{name}_dev"] = spec("target_dev:inout:rgba selection_dev:opt:mask", args=BRUSH, accepts={("target_dev", "selection_dev")})
for name in ("brush_stamps", "brush_stamps_ex", "brush_line", "brush_line_ex"):
    TABLE[f"pfx_{name}"] = spec("target_inout:inout:rgba selection:opt:mask", args=BRUSH, accepts={("target_inout", "selection")})
TABLE["pfx_brush_commit"] = spec("layer_inout:inout:rgba preview:in:rgba selection:opt:mask", accepts={("layer_inout", "preview"), ("layer_inout", "selection")},
                                 in_place=("layer_inout", "preview", OK))
TABLE["pfx_blend_pixels"] = spec("base:in:rgba top:in:rgba dst:out:rgba", args={"n_pixels": W * H}, accepts={("dst", "base"), ("dst", "top")},
                                 in_place=("dst", "base", OK))
# ---- the effect bank (pfx_effects.cpp): src and dst never share a byte, in either tier ----
EFFECTS = ("sharpen", "glow", "bokeh_blur", "motion_blur", "zoom_blur", "crystallize", "dents", "bulge", "twist", "add_noise", "reduce_noise", "vignette", "halftone",
           "grid", "canvas_border", "shadow", "outline", "pixel_drag", "rgb_displace", "ink", "oil_painting", "color_filter", "contours")
for name in EFFECTS:
    TABLE[f"pfx_{name}_dev"] = spec("src_dev:in:rgba dst_dev:out:rgba mask_dev:opt:mask", in_place=("dst_dev", "src_dev", INVALID), accepts={("dst_dev", "mask_dev")})
    TABLE[f"pfx_{name}_core"] = spec("src:in:rgba dst:out:rgba mask:opt:mask", in_place=("dst", "src", INVALID), accepts={("dst", "mask")})
# ---- resamplers (pfx_resize.cpp) ----
for name in ("resize_image", "affine_transform", "flip_rotate", "resize_canvas"):
    common = {"op": 0, "filter": 1, "interpolation": 1, "anchor_x": 1, "anchor_y": 1}
    # pfx_affine_transform_dev accepts an empty source and pfx_resize_canvas_dev does not bound w * h (gaps, kept): those dimensions are not zeroed here,
    # an accepted call would launch on them
    keep = {"affine_transform": (("src_w", "src_h"),)}.get(name, ())
    TABLE[f"pfx_{name}_dev"] = spec("src_dev:in:rgba dst_dev:out:rgba", args=common, in_place=("dst_dev", "src_dev", INVALID), keep_dims=keep)
    TABLE[f"pfx_{name}"] = spec("src:in:rgba dst:out:rgba", args=common, in_place=("dst", "src", OK), accepts={("dst", "src")})
# ---- shapes ----
for name, buf in (("shape_rasterize_dev", "box_dev"), ("shape_rasterize", "box_rgba"), ("shape_preview_dev", "canvas_dev"), ("shape_preview", "canvas_rgba")):
    TABLE[f"pfx_{name}"] = spec(f"{buf}:inout:rgba", args={"shape": "shape"}, required=("shape",))
TABLE["pfx_shape_draw_dev"] = spec("layer_dev:inout:rgba selection_dev:opt:mask", args={"shape": "shape"}, required=("shape",), accepts={("layer_dev", "selection_dev")})
# ---- content-aware fill ----
for tier, s in (("_dev", "_dev"), ("", "")):
    out = "out_dev" if tier else "out_inout"
    TABLE[f"pfx_inpaint_instant{tier}"] = spec(f"src{s}:in:rgba hole_mask{s}:in:mask {out}:inout:rgba", args={"dabs": "inpaint_dab"}, in_place=(out, f"src{s}", INVALID))
    TABLE[f"pfx_inpaint_patchmatch{tier}"] = spec(f"src{s}:in:rgba hole_mask{s}:in:mask dst{s}:out:rgba", args={"patch_size": 3}, in_place=(f"dst{s}", f"src{s}", OK))
# ---- flood ----
FLOOD = {"flood": "flood", "seed_x": 1, "seed_y": 1, "threshold": 40}
TABLE["pfx_flood_distance_dev"] = spec("src_dev:in:rgba dist_dev:out:mask", args=FLOOD, required=("flood",), misaligned=("src_dev",))
TABLE["pfx_flood_distance"] = spec("src:in:rgba dist:out:mask", args=FLOOD, required=("flood",))
TABLE["pfx_flood_bboxes_dev"] = spec("dist_dev:in:mask", required=("boxes",))
for tier in ("_dev", ""):
    TABLE[f"pfx_wand_mask{tier}"] = spec(f"dist{tier}:in:mask base_mask{tier}:opt:mask mask_out{tier}:out:mask", args=FLOOD, in_place=(f"mask_out{tier}", f"base_mask{tier}", OK))
    TABLE[f"pfx_fill_preview{tier}"] = spec(f"dist{tier}:in:mask selection{tier}:opt:mask canvas_out{tier}:out:rgba", args=FLOOD, required=("fill",),
                                            misaligned=("canvas_out_dev",) if tier else ())
TABLE["pfx_fill_commit_dev"] = spec("layer_dev:inout:rgba dist_dev:in:mask selection_dev:opt:mask", args=FLOOD, required=("fill",), misaligned=("layer_dev",))
TABLE["pfx_bucket_fill"] = spec("layer_inout:inout:rgba selection:opt:mask", args=FLOOD, required=("fill",))
# ---- selection masks ----
for tier in ("_dev", ""):
    for name in ("select_rect", "select_ellipse", "select_lasso"):
        TABLE[f"pfx_{name}{tier}"] = spec(f"base_mask{tier}:opt:mask mask_out{tier}:out:mask", args={"points_xy": "triangle", "n_points": 3, "max_x": 9, "max_y": 3},
                                         in_place=(f"mask_out{tier}", f"base_mask{tier}", OK))
    TABLE[f"pfx_selection_translate{tier}"] = spec(f"mask{tier}:in:mask mask_out{tier}:out:mask", in_place=(f"mask_out{tier}", f"mask{tier}", INVALID))
    for name in ("feather", "expand", "contract"):
        TABLE[f"pfx_selection_{name}{tier}"] = spec(f"mask{tier}:in:mask mask_out{tier}:out:mask", in_place=(f"mask_out{tier}", f"mask{tier}", OK))
TABLE["pfx_selection_bounds_dev"] = spec("mask_dev:in:mask", required=("box",))
TABLE["pfx_selection_fill_dev"] = spec("layer_dev:inout:rgba mask_dev:in:mask", required=("color",), misaligned=("layer_dev",))
TABLE["pfx_selection_delete_dev"] = spec("layer_dev:inout:rgba mask_dev:in:mask", misaligned=("layer_dev",))
# ---- removal by colour ----
for name, tier, sel, params in (("color_to_alpha_dev", "_dev", "mask_dev", "settings"), ("color_to_alpha_core", "", "mask", "settings"),
                                ("color_removal_dev", "_dev", "selection_dev", "req"), ("color_removal", "", "selection", "req")):
    TABLE[f"pfx_{name}"] = spec(f"src{tier}:in:rgba dst{tier}:out:rgba {sel}:opt:mask", args={params: params}, required=(params,),
                                in_place=(f"dst{tier}", f"src{tier}", OK), misaligned=("src_dev", "dst_dev") if tier else ())


def host_blocks():
    """the small host arguments by name; everything is kept alive by the caller"""
    grid = (C.c_float * 8)(0, 0, W, 0, 0, H, W, H)
    brush = _lib.Brush(4.0, 0.5, 1.0, (C.c_float * 4)(1.0, 0.5, 0.25, 1.0), 1, 0, 0)
    flood = _lib.Flood(1, 1, (C.c_uint8 * 4)(9, 9, 9, 255), 0, 4, 0, 0)
    shape = _lib.Shape(30.0, 2.0, 8.0, 1.5, 0.0, 1.0, 0.0, (C.c_uint8 * 4)(255, 0, 0, 255), (C.c_uint8 * 4)(0, 255, 0, 255), 1, 1, 1, 0)
    settings = _lib.ColorToAlpha((C.c_uint8 * 3)(9, 9, 9), 0, 10.0, 10.0, 1.0, 0.0, 0.0, 1.0, 0.0)
    return {"grid": grid, "brush": brush, "flood": flood, "shape": shape, "settings": settings, "req": _lib.ColorRemoval(1, 1, 10.0, 0, 1, (C.c_uint8 * 3)()),
            "point": (C.c_float * 2)(10.0, 2.0), "triangle": (C.c_float * 6)(2.0, 0.5, 40.0, 0.5, 20.0, 4.5),
            "disp_dab": _lib.DispDab(0, 10.0, 2.0, 1.0, 0.0, 3.0, 0.5), "inpaint_dab": _lib.InpaintDab(10.0, 2.0, 2.0, 3.0, 0.5)}


@pytest.fixture(scope="module")
def env():
    lib = _lib.load()
    ctx = C.c_void_p(None)
    assert lib.pfx_ctx_create(C.c_int(0), C.byref(ctx)) == OK
    rng = np.random.default_rng(20)
    pattern = rng.integers(0, 256, SLOT * N_SLOTS, dtype=np.uint8)
    pattern[rng.random(pattern.size) < 0.5] = 0          # masks with holes, images with transparent pixels
    host = pattern.copy()
    dev = C.c_void_p(None)
    assert lib.pfx_dev_alloc(ctx, C.c_size_t(pattern.size), C.byref(dev)) == OK
    assert lib.pfx_warp_set_source(ctx, C.c_void_p(pattern.ctypes.data), C.c_uint32(W), C.c_uint32(H)) == OK   # for pfx_warp_displacement_cached
    yield dict(lib=lib, ctx=ctx, pattern=pattern, host=host, dev=dev.value, blocks=host_blocks(), protos={n: p for _, n, p in prototypes()})
    lib.pfx_dev_free(ctx, dev)
    lib.pfx_ctx_destroy(ctx)


def restore(e):
    e["host"][:] = e["pattern"]
    assert e["lib"].pfx_dev_upload(e["ctx"], C.c_void_p(e["dev"]), C.c_void_p(e["pattern"].ctypes.data), C.c_size_t(e["pattern"].size)) == OK
    assert e["lib"].pfx_ctx_synchronize(e["ctx"]) == OK


def untouched(e):
    got = np.empty_like(e["pattern"])
    assert e["lib"].pfx_ctx_synchronize(e["ctx"]) == OK
    assert e["lib"].pfx_dev_download(e["ctx"], C.c_void_p(got.ctypes.data), C.c_void_p(e["dev"]), C.c_size_t(got.size)) == OK
    assert e["lib"].pfx_ctx_synchronize(e["ctx"]) == OK
    return np.array_equal(got, e["pattern"]) and np.array_equal(e["host"], e["pattern"])


def test_the_table_names_every_entry_point_that_takes_an_image_or_a_mask(env):
    """the converted modules' entry points, from the header: whatever has a pixel / mask pointer and a size is in TABLE (the compositor, the layer store, the
    script front-end and the project / batch calls are other modules)"""
    image_words = ("src", "dst", "mask", "selection", "dist", "layer_dev", "layer_inout", "target", "pixels", "disp", "canvas", "box_dev", "box_rgba", "out_")
    other_modules = ("pfx_layer_", "pfx_composite", "pfx_flatten", "pfx_script_", "pfx_project_", "pfx_tiled_import", "pfx_tiled_export", "pfx_dev_", "pfx_group_",
                     "pfx_batch_", "pfx_png_", "pfx_pfe_")
    missing = []
    for name, plist in env["protos"].items():
        if not plist or not plist[0].replace(" ", "").startswith("pfx_ctx*") or name.startswith(other_modules):
            continue
        pnames = [re.sub(r"\[.*\]", "", p).replace("*", " ").split()[-1] for p in plist[1:]]
        if any(pn.startswith(image_words) for pn in pnames) and len(set(pnames) & (set(DIMS) | {"n_pixels"})) >= 1 and name not in TABLE:
            missing.append(name)
    assert not missing, missing
    assert not [n for n in TABLE if n not in env["protos"]]


@pytest.mark.parametrize("name", sorted(TABLE))
def test_argument_contract(env, name):
    e, S = env, TABLE[name]
    lib, plist = e["lib"], e["protos"][name][1:]
    pnames = [re.sub(r"\[.*\]", "", p).replace("*", " ").split()[-1] for p in plist]
    slots = {b: i for i, b in enumerate(S["bufs"])}
    assert set(S["bufs"]) <= set(pnames), (set(S["bufs"]) - set(pnames))

    def address(b, shift=0):
        base = e["dev"] if b.endswith("_dev") else e["host"].ctypes.data
        return base + slots[b] * SLOT + shift

    def call(ptrs=None, dims=None):
        """ptrs: buffer or pointer name -> address (None = NULL); dims: dimension name -> value"""
        args = [e["ctx"]]
        for p, pn in zip(plist, pnames):
            if ptrs and pn in ptrs:
                args.append(C.c_void_p(ptrs[pn]))
            elif pn in S["bufs"]:
                args.append(C.c_void_p(address(pn)))
            elif "*" in p or "[" in p:
                v = S["args"].get(pn, "zeros")
                args.append(C.c_void_p(None) if v is None else (C.cast(C.pointer(e["blocks"][v]), C.c_void_p) if v != "zeros" else C.c_void_p(zeros.ctypes.data)))
            else:
                ctype = SCALARS[[t for t in p.replace("const", " ").split() if t != "unsigned"][0]] if p.split()[0] != "unsigned" else C.c_uint
                v = (dims or {}).get(pn, DIMS.get(pn, S["args"].get(pn, 1)))
                args.append(ctype(v))
        fn = getattr(lib, name)
        fn.restype = C.c_int
        return fn(*args)

    zeros = np.zeros(8192, np.uint8)
    wrong = []

    def expect(what, status, want):
        if status != want:
            wrong.append(f"{what}: {_lib.STATUS_NAMES.get(status, status)}, expected {_lib.STATUS_NAMES[want]}")

    restore(e)
    expect("the valid call", call(), OK)
    restore(e)
    # ---- refusals ----
    for b, (kind, _) in S["bufs"].items():
        if kind != "opt":
            expect(f"{b} = NULL", call({b: None}), INVALID)
    for pn in S["required"]:
        expect(f"{pn} = NULL", call({pn: None}), INVALID)
    pairs = [(a, b) for a, b in (("w", "h"), ("sw", "sh"), ("new_w", "new_h"), ("canvas_w", "canvas_h"), ("src_w", "src_h"), ("w", "band_rows")) if a in pnames and b in pnames]
    for a, b in pairs:
        if (a, b) not in S["keep_dims"]:
            expect(f"{a} = 0", call(dims={a: 0}), INVALID)
            expect(f"{b} = 0", call(dims={b: 0}), INVALID)
    if pairs:
        expect("20000 x 20000", call(dims={d: 20000 for pair in pairs for d in pair}), INVALID)
    outs = [b for b, (kind, _) in S["bufs"].items() if kind in ("out", "inout")]
    overlaps = [(o, b) for o in outs for b in S["bufs"] if b != o]
    for o, b in overlaps:
        if (o, b) not in S["accepts"]:
            expect(f"{o} overlaps {b}", call({o: address(b, 16)}), INVALID)
            expect(f"{b} overlaps {o}", call({b: address(o, 16)}), INVALID)
    if S["in_place"] and S["in_place"][2] == INVALID:
        expect(f"{S['in_place'][0]} == {S['in_place'][1]}", call({S["in_place"][0]: address(S["in_place"][1])}), INVALID)
    for b in S["misaligned"]:
        for off in (1, 2, 3):
            expect(f"{b} + {off}", call({b: address(b, off)}), INVALID)
    clean = untouched(e)
    # ---- accepted aliasing ----
    for o, b in overlaps:
        if (o, b) in S["accepts"]:
            expect(f"{o} overlaps {b} (not refused: see the module text)", call({o: address(b, 16)}), OK)
            restore(e)
    if S["in_place"] and S["in_place"][2] == OK:
        expect(f"{S['in_place'][0]} == {S['in_place'][1]}", call({S["in_place"][0]: address(S["in_place"][1])}), OK)
        restore(e)
    assert not wrong, "\n".join(wrong)
    assert clean, "a refused call wrote to a buffer"
