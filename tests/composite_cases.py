"""The compositor's document path at its edges: one table for the host test (tests/test_composite_cases_host.py: the table reaches what it claims, the
oracle alone handles every value) and the device test (tests/test_gpu_composite_edges.py: every case against the oracle at tolerance 0).  Pure numpy: no
oracle code and no device code here; `Case.want(compose)` takes the oracle's composite as an argument.

A case is one composite call: a stack in the oracle's form (oracle_lib.composite: dicts bottom -> top; cases of one group share their pixel arrays, so the
device test uploads an image once and changes only descriptors), the route it takes into the library, and optionally a tool preview, a dirty rectangle or
caller-supplied chunk keys.  What is expected of it:
  ORACLE  the device image equals the oracle's (the rectangle: the crop of the oracle's full composite);
  STATUS  the call raises PfxError and leaves the destination as it was (`bound` names the refusing check).

Canvas sizes follow from flatten_kernel's geometry (k_flatten.hip): a lane owns 4 consecutive pixel indices in row-major order over the whole image,
chunks are 64 x 64, and a rectangle's quads run along its rows and take the 16-byte path only when (p0 | o0) & 3 == 0.

Groups: A the conceal lattice, B adjustment layers, C chunk activity, D the tool preview, E dirty rectangles, F raster-only stacks off the fast-division
path, G a seeded editing session (steps and a numpy mirror of the document)."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

f32 = np.float32
INF, NAN = float("inf"), float("nan")
ORACLE, STATUS = "oracle", "status"
STORE, DEV, KEYS = "store", "dev", "keys"   # pfx_layer_* + pfx_composite[_preview | _region]; pfx_flatten[_preview]_dev; pfx_int_flatten_with_chunk_keys_dev
ADJ_EXPOSURE, ADJ_BC, ADJ_INVERT, ADJ_MIXER = 1, 2, 3, 4
NORMAL, MULTIPLY, OVERLAY, XOR, OVERWRITE = 0, 1, 8, 13, 14
CHUNK = 64

CANVASES = [(1, 1), (3, 1), (1, 5), (5, 3), (63, 2), (64, 64), (65, 65), (66, 3), (67, 66), (130, 70), (257, 5)]
LATTICE = (256, 256)

# pfx_int_flatten_last_path (pfx_internal.h)
K_TEMPLATE, K_STREAM, K_DLE, K_SRT = 0, 1, 2, 3
P_GENERAL, P_FAST, P_REGION, P_PREVIEW, P_CHUNK_START = 1 << 4, 1 << 5, 1 << 6, 1 << 7, 1 << 8
FAST_DIV_MIN = float(f32(2.0) ** -40)   # pfx_internal.h: opacity_allows_fast_div


def below(x):
    return float(np.nextafter(f32(x), f32(0.0)))


def rgba(w, h, seed, alpha=None):
    """random colours; alpha random, a constant, or an array"""
    img = np.random.default_rng(seed).integers(0, 256, (h, w, 4), dtype=np.uint8)
    if alpha is not None:
        img[..., 3] = alpha
    return img


def chunk_grid(w, h):
    return (w + CHUNK - 1) // CHUNK, (h + CHUNK - 1) // CHUNK


def chunk_of_pixels(w, h):
    """the chunk index of every pixel, h x w"""
    yy, xx = np.mgrid[0:h, 0:w]
    return (yy // CHUNK) * chunk_grid(w, h)[0] + xx // CHUNK


def populated(img):
    """TiledImage::from_rgba_image's rule (tiled_image.rs:81-95): a chunk exists where some alpha is not 0"""
    h, w = img.shape[:2]
    cxn, cyn = chunk_grid(w, h)
    out = np.zeros(cxn * cyn, np.uint8)
    np.maximum.at(out, chunk_of_pixels(w, h).ravel(), (img[..., 3].ravel() != 0).astype(np.uint8))
    return out


def is_adj(L):
    return L.get("kind", 0) != 0


def fast_div(layers):
    """pfx_flatten.cpp: every layer of the call counts, hidden and adjustment layers too; NaN fails the comparison"""
    return all(f32(L.get("opacity", 1.0)) >= f32(FAST_DIV_MIN) for L in layers)


def is_general(layers):
    return any(L.get("visible", True) and (is_adj(L) or (L.get("pixels") is not None and L.get("mask") is not None)) for L in layers)


@dataclass
class Case:
    name: str
    w: int
    h: int
    layers: list
    route: str = STORE
    preview: dict = None     # oracle form: pixels, active_layer, blend_mode, is_eraser, replaces_layer, chunk_present
    rect: tuple = None       # (x, y, rw, rh)
    keys: np.ndarray = None  # one byte per chunk: the union of the visible layers' TiledImage chunk keys
    expect: str = ORACLE
    bound: str = ""

    def region(self):
        return self.rect is not None and tuple(self.rect) != (0, 0, self.w, self.h)

    def path(self):
        """(value, mask) the launch-path seam must show after this composite, from the rule the host code documents: a preview, a rectangle, a live mask or
        an adjustment layer needs flatten_kernel<true, F>; a raster-only stack with an opacity below 2^-40 (or NaN) flatten_kernel<false, false>; every other
        stack one of the fast kernels (which one depends on depth, candidates and verdicts: only `not the template` is fixed here; the choice among them and their shapes
        are pinned at the plan seam: tests/test_flatten_dispatch_host.py, tests/test_gpu_flatten_plan.py)"""
        fast = P_FAST if fast_div(self.layers) else 0
        special = (P_PREVIEW if self.preview is not None else 0) | (P_REGION if self.region() else 0)
        n_desc = sum(1 for L in self.layers if L.get("visible", True) and (is_adj(L) or L.get("pixels") is not None))
        if special or is_general(self.layers):
            return K_TEMPLATE | P_GENERAL | fast | special, 0xFF
        if not fast or n_desc == 0:
            return K_TEMPLATE | fast, 0xFF
        return P_FAST, 0xF0    # kernel bits free, but see fast_kernel()

    def fast_kernel(self):
        return self.path() == (P_FAST, 0xF0)

    def want(self, compose):
        """compose: oracle_lib.composite.  Caller-supplied chunk keys are handed to the oracle as a preview that draws nothing (every alpha 0: canvas_state.rs:625
        leaves the layer pixel alone) with the keys as its chunk_present: they join the active set exactly as a held chunk's key does (:541-548)"""
        pv = self.preview
        if self.keys is not None:
            active = next(i for i, L in enumerate(self.layers) if L.get("visible", True) and not is_adj(L) and L.get("pixels") is not None)
            pv = dict(pixels=np.zeros((self.h, self.w, 4), np.uint8), active_layer=active, chunk_present=self.keys)
        full = compose(self.layers, self.w, self.h, preview=pv)
        if self.rect is None:
            return full
        x, y, rw, rh = self.rect
        return full[y:y + rh, x:x + rw]


def adj(kind, params=(), opacity=1.0, visible=True):
    return dict(kind=kind, adj=[float(v) for v in params], opacity=opacity, visible=visible)


# ---------------------------------------------------------------------------------------------------------------- A: the conceal lattice
A_DESCRIPTORS = [(NORMAL, 1.0), (NORMAL, 0.5), (OVERWRITE, 1.0), (OVERWRITE, 0.7), (XOR, 1.0), (MULTIPLY, 0.5)]
BASES = {"transparent": 0, "partial": 143, "opaque": 255}


def lattice():
    """256 x 256: layer alpha = row, conceal = column: every (alpha, conceal) pair once"""
    a = np.arange(256, dtype=np.uint8)
    img = rgba(256, 256, 101, alpha=np.repeat(a[:, None], 256, 1))
    mask = np.repeat(a[None, :], 256, 0).copy()
    return img, mask


def group_a():
    w, h = LATTICE
    img, mask = lattice()
    cases = []
    bases = {name: rgba(w, h, 110 + k, alpha=a) for k, (name, a) in enumerate(BASES.items())}
    for bname, base in bases.items():
        for mode, opacity in A_DESCRIPTORS:
            for route in (STORE, DEV):
                cases.append(Case(f"lattice over {bname} mode {mode} opacity {opacity} {route}", w, h,
                                  [dict(pixels=base), dict(pixels=img, mask=mask, mode=mode, opacity=opacity)], route))
    base, top = bases["partial"], rgba(w, h, 120)
    img2, mask2 = np.ascontiguousarray(img.transpose(1, 0, 2)), np.ascontiguousarray(255 - mask)
    everything = np.full((h, w), 255, np.uint8)
    sparse = np.where((chunk_of_pixels(w, h) % 3 == 0)[..., None], img | np.uint8(1), 0).astype(np.uint8)   # content (every alpha != 0) in every third chunk
    for route in (STORE, DEV):
        cases += [
            Case(f"mask on the bottom layer {route}", w, h, [dict(pixels=img, mask=mask), dict(pixels=top, mode=MULTIPLY, opacity=0.5)], route),
            Case(f"masks on two layers {route}", w, h, [dict(pixels=base), dict(pixels=img, mask=mask), dict(pixels=img2, mask=mask2, mode=OVERWRITE, opacity=0.7)], route),
            Case(f"mask on a hidden layer {route}", w, h, [dict(pixels=base), dict(pixels=img, mask=mask, visible=False), dict(pixels=top, opacity=0.5)], route),
            Case(f"all-255 mask: the layer vanishes, its chunks stay populated {route}", w, h,
                 [dict(pixels=np.zeros((h, w, 4), np.uint8)), dict(pixels=sparse, mask=everything), adj(ADJ_INVERT)], route),
        ]
    # the same images with the mask, then without: the device test's store keeps the pixels and clears the mask with NULL
    cases += [Case("mask set", w, h, [dict(pixels=base), dict(pixels=img, mask=mask, opacity=0.5)], STORE),
              Case("mask cleared with NULL", w, h, [dict(pixels=base), dict(pixels=img, opacity=0.5)], STORE)]
    return cases


# ---------------------------------------------------------------------------------------------------------------- B: adjustment layers
@dataclass
class AdjRow:
    name: str
    kind: int
    params: list
    opacity: float = 1.0
    identity: bool = False   # the row leaves every pixel as it was (the host test fixes that; every other row must change the picture)

    def layer(self):
        return adj(self.kind, self.params, self.opacity)


EXPOSURE_EV = [0.0, 0.5, -0.5, 1.0, -1.0, 8.0, -8.0, 127.0, 128.0, -149.0, -150.0, INF, -INF, NAN]
BRIGHTNESS = [0.0, 255.0, -255.0, 1e9, -1e9, INF, NAN]
CONTRAST = [0.0, 100.0, -100.0, 255.0, -255.0, 258.99, 259.0, 260.0, INF, -INF, NAN]
OPACITIES = [1.0, below(1.0), 0.5, 1e-8, 0.0, -1.0, 2.0, INF, NAN]
IDENTITY_OPACITIES = (1e-8, 0.0, -1.0)   # t = clamp(opacity): 0 keeps the pixel; 1e-8: inv = 1 - 1e-8 rounds to 1.0f and 255 * 1e-8 rounds away


def identity_matrix():
    return [1.0 if i % 5 == 0 else 0.0 for i in range(16)]


def matrix(rows):
    return [float(v) for row in rows for v in row]


ALPHA_MIXER = matrix([(1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (1, 0, 0, -1)])   # a' = clamp(r - a): 0 -> r (non-zero after an Invert), 255 -> 0
MIXERS = {
    "identity": identity_matrix(),
    "swap": matrix([(0, 0, 1, 0), (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 0, 1)]),
    "negative": matrix([(1.5, -0.5, 0, 0), (-1, 1, 1, 0), (0.25, -2, 1, 0), (0, 0, 0, 1)]),
    "above 255": matrix([(1, 1, 1, 0), (2, 0, 0.5, 0), (0.7, 0.7, 0.7, 0.7), (0, 0, 0, 1)]),
    "alpha row": ALPHA_MIXER,
    "1e30": matrix([(1e30, 0, 0, 0), (0, -1e30, 1e30, 0), (0, 0, 1, 0), (0, 0, 0, 1)]),
    "inf": matrix([(INF, 0, 0, 0), (0, 1, -INF, 0), (INF, -INF, 1, 0), (0, 0, 0, 1)]),
    "nan": matrix([(NAN, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, NAN), (0, 0, 0, 1)]),
    "-0.0": [1.0 if i % 5 == 0 else -0.0 for i in range(16)],
}
OPACITY_KINDS = {"exposure": (ADJ_EXPOSURE, [1.0]), "brightness_contrast": (ADJ_BC, [30.0, 50.0]), "invert": (ADJ_INVERT, []), "mixer": (ADJ_MIXER, MIXERS["swap"])}


def adj_rows():
    rows = [AdjRow(f"exposure ev {ev}", ADJ_EXPOSURE, [ev], identity=ev == 0.0) for ev in EXPOSURE_EV]
    rows += [AdjRow(f"brightness {b} contrast {c}", ADJ_BC, [b, c], identity=(b == 0.0 and c == 0.0)) for b in BRIGHTNESS for c in CONTRAST]
    rows += [AdjRow(f"mixer {name}", ADJ_MIXER, m, identity=name in ("identity", "-0.0")) for name, m in MIXERS.items()]
    for name, (kind, params) in OPACITY_KINDS.items():
        rows += [AdjRow(f"{name} at opacity {o}", kind, params, o, identity=o in IDENTITY_OPACITIES) for o in OPACITIES]
    return rows


def adj_source(w, h):
    """every byte value on every channel (from 256 pixels up) over accumulators that are transparent, partial (143) and opaque, 256 pixels of each in turn"""
    i = np.arange(w * h)
    img = np.stack([i % 256, (7 * i + 85) % 256, (255 - 3 * i) % 256, np.array([0, 143, 255])[(i // 256) % 3]], -1)
    return img.astype(np.uint8).reshape(h, w, 4)


def lane_alpha(w, h):
    return np.array([0, 1, 127, 254, 255], np.uint8)[np.arange(w * h) % 5].reshape(h, w)


B_MAIN = (130, 70)
ZERO_ADJ = adj(ADJ_EXPOSURE, [0.5], 0.0)    # an adjustment layer at opacity 0: the identity, and it moves the whole stack to flatten_kernel<true, false>
TAIL_ADJ = adj(ADJ_EXPOSURE, [0.5], 0.3)


def b_stack(src, top, middle, zero):
    """[source, the layers under test, a raster layer, an Exposure at opacity 0.3 — or 0 in the twin run]"""
    return [dict(pixels=src)] + list(middle) + [dict(pixels=top, mode=MULTIPLY, opacity=0.8), ZERO_ADJ if zero else TAIL_ADJ]


def b_without(case_layers):
    """the same stack without the layer under test (position 1)"""
    return case_layers[:1] + case_layers[2:]


def compound_stack(w, h, zero=False):
    """all four kinds, a live mask and a hidden layer between them"""
    mask = np.where(np.random.default_rng(5).random((h, w)) < 0.3, 0, rgba(w, h, 6)[..., 0]).astype(np.uint8)
    return [dict(pixels=adj_source(w, h)), adj(ADJ_EXPOSURE, [0.7]), adj(ADJ_BC, [12.0, 30.0], 0.5),
            dict(pixels=rgba(w, h, 7, alpha=lane_alpha(w, h)), mode=OVERLAY, opacity=0.8, mask=mask), dict(pixels=rgba(w, h, 8), visible=False, mode=3),
            adj(ADJ_INVERT, (), 0.0 if zero else 0.6), adj(ADJ_MIXER, MIXERS["negative"], 0.9)]


def group_b_rows():
    """[(row, case, twin case)]: every row in the standard stack on 130 x 70, as is and with the trailing adjustment at opacity 0"""
    w, h = B_MAIN
    src, top = adj_source(w, h), rgba(w, h, 130, alpha=lane_alpha(w, h))
    return [(row, Case(f"{row.name}", w, h, b_stack(src, top, [row.layer()], False)), Case(f"{row.name}, zero-opacity twin", w, h, b_stack(src, top, [row.layer()], True)))
            for row in adj_rows()]


def group_b_positions():
    w, h = B_MAIN
    src, top, top2 = adj_source(w, h), rgba(w, h, 130, alpha=lane_alpha(w, h)), rgba(w, h, 131)
    inv, mix = adj(ADJ_INVERT, (), 0.5), adj(ADJ_MIXER, ALPHA_MIXER)
    R = lambda px, **kw: dict(pixels=px, **kw)   # noqa: E731
    stacks = {
        "bottom of the stack": [adj(ADJ_INVERT), R(src), R(top, mode=MULTIPLY, opacity=0.8)],
        "bottom, then a mixer": [adj(ADJ_INVERT), mix, R(src, opacity=0.7), R(top, mode=XOR)],
        "top": [R(src), R(top, mode=MULTIPLY, opacity=0.8), inv],
        "two in a row": [R(src), inv, mix, R(top, opacity=0.5)],
        "three in a row": [R(src), adj(ADJ_INVERT), mix, adj(ADJ_EXPOSURE, [1.0], 0.5), R(top, mode=OVERLAY, opacity=0.9)],
        "between rasters": [R(src), R(top, opacity=0.5), inv, R(top2, mode=MULTIPLY, opacity=0.4), mix, R(top, mode=XOR, opacity=0.9)],
        "hidden": [R(src), adj(ADJ_INVERT, (), 1.0, visible=False), R(top, opacity=0.5), adj(ADJ_MIXER, ALPHA_MIXER, 1.0, visible=False)],
        "adjustment layers only": [adj(ADJ_INVERT), mix, adj(ADJ_BC, [40.0, 20.0])],
        "every raster hidden": [R(src, visible=False), adj(ADJ_INVERT), R(top, visible=False), mix],
    }
    cases = []
    for name, layers in stacks.items():
        for zero in (False, True):
            cases.append(Case(f"{name}{', zero-opacity twin' if zero else ''}", w, h, layers + ([ZERO_ADJ] if zero else [])))
    return cases


def group_b_modes():
    """above a mixer that rewrote alpha (after an Invert: transparent accumulators become (255, 255, 255, 255), opaque ones lose their alpha), one raster layer
    of each mode: blend_layer_fast's opaque-base choice must follow the new alpha"""
    w, h = B_MAIN
    src, top = adj_source(w, h), rgba(w, h, 132, alpha=lane_alpha(w, h))
    cases = []
    for mode in range(25):
        for opacity in (1.0, 0.6):
            for zero in (False, True):
                layers = [dict(pixels=src), adj(ADJ_INVERT), adj(ADJ_MIXER, ALPHA_MIXER), dict(pixels=top, mode=mode, opacity=opacity)] + ([ZERO_ADJ] if zero else [])
                cases.append(Case(f"mode {mode} at {opacity} above the alpha mixer{', zero-opacity twin' if zero else ''}", w, h, layers))
    return cases


def group_b_canvases():
    cases = []
    for w, h in CANVASES:
        for route in (STORE, DEV):
            for zero in (False, True):
                cases.append(Case(f"compound stack {route}{', zero-opacity twin' if zero else ''}", w, h, compound_stack(w, h, zero), route))
    return cases


# ---------------------------------------------------------------------------------------------------------------- C: chunk activity
C_CANVASES = [(66, 3), (65, 65), (67, 66), (130, 70)]
ROLES = ["visible", "hidden", "concealed", "ghost", "empty"]   # what alone populates a chunk; "ghost": coloured pixels of alpha 0
ACTIVE_ROLES = ("visible", "concealed")                         # a concealed layer's chunk exists (its pixels have alpha); hidden layers do not count
C_ABOVE = [adj(ADJ_INVERT), adj(ADJ_MIXER, MIXERS["swap"], 0.75)]


def roles_of(w, h, variant):
    cxn, cyn = chunk_grid(w, h)
    return [ROLES[(c + variant) % len(ROLES)] for c in range(cxn * cyn)]


def activity_images(w, h, variant):
    """one layer per role: content only in the chunks that role holds"""
    roles = np.array(roles_of(w, h, variant))[chunk_of_pixels(w, h)]
    out = {}
    for k, role in enumerate(ROLES[:4]):
        img = rgba(w, h, 140 + k)
        img[..., 3] = 0 if role == "ghost" else img[..., 3] | 1
        out[role] = np.where((roles == role)[..., None], img, 0).astype(np.uint8)
    return out


def activity_layers(w, h, variant, masks=True):
    im = activity_images(w, h, variant)
    everything = np.full((h, w), 255, np.uint8)
    layers = [dict(pixels=im["visible"], opacity=0.9), dict(pixels=im["hidden"], visible=False)]
    if masks:
        layers.append(dict(pixels=im["concealed"], mask=everything))
    return layers + [dict(pixels=im["ghost"], mode=MULTIPLY)] + C_ABOVE


def pixel_activity(w, h, variant, masks=True):
    """h x w: whether an adjustment layer runs on the pixel"""
    active = np.array([r in ACTIVE_ROLES and (masks or r != "concealed") for r in roles_of(w, h, variant)])
    return active[chunk_of_pixels(w, h)]


def mixed_quads(act):
    """quads (4 consecutive pixel indices over the whole image) that hold an active and an inactive pixel"""
    flat = act.ravel()
    n = len(flat) // 4 * 4
    q = flat[:n].reshape(-1, 4)
    return int((q.any(1) & ~q.all(1)).sum())


def group_c():
    cases = []
    for w, h in C_CANVASES:
        n_chunks = int(np.prod(chunk_grid(w, h)))
        for variant in range(len(ROLES)):
            layers = activity_layers(w, h, variant)
            for route in (STORE, DEV):
                cases.append(Case(f"roles rotated by {variant} {route}", w, h, layers, route))
            # caller-supplied keys (no masks on this route): the layers' own chunks plus the ghost's, which a document can hold although every alpha is 0
            plain = activity_layers(w, h, variant, masks=False)
            ghost_held = populated(plain[0]["pixels"]) | np.array([r == "ghost" for r in roles_of(w, h, variant)], np.uint8)
            cases.append(Case(f"roles rotated by {variant}, keys hold the transparent chunks", w, h, plain, KEYS, keys=ghost_held))
            cases.append(Case(f"roles rotated by {variant}, keys all 1", w, h, plain, KEYS, keys=np.ones(n_chunks, np.uint8)))
        # keys all 0 are what a document holds whose visible layers have no chunk at all: nothing visible has alpha (a hidden layer does), so nothing is active
        ghost = activity_images(w, h, 0)
        nothing = [dict(pixels=ghost["ghost"]), dict(pixels=ghost["visible"], visible=False)] + C_ABOVE
        cases.append(Case("keys all 0 under transparent layers", w, h, nothing, KEYS, keys=np.zeros(n_chunks, np.uint8)))
        cases.append(Case("keys all 1 under transparent layers", w, h, nothing, KEYS, keys=np.ones(n_chunks, np.uint8)))
        # the preview alone populates a chunk: the last one
        pv = np.zeros((h, w, 4), np.uint8)
        sel = chunk_of_pixels(w, h) == n_chunks - 1
        pv[sel] = rgba(w, h, 150, alpha=200)[sel]
        for route in (STORE, DEV):
            cases.append(Case(f"the preview alone populates a chunk {route}", w, h, nothing, route, preview=dict(pixels=pv, active_layer=0, blend_mode=NORMAL)))
    return cases


# ---------------------------------------------------------------------------------------------------------------- D: the tool preview
D_CANVASES = [(5, 3), (66, 3), (130, 70)]
LAYER_ALPHAS, PREVIEW_ALPHAS = [0, 1, 127, 254, 255], [0, 1, 127, 128, 254, 255]
PREVIEW_MODES = list(range(25)) + [25, 255]   # ids past 24 fall back to Normal
CHUNK_PRESENT = ["null", "ones", "zeros", "checker"]
POSITIONS = ["bottom", "middle", "top", "hidden", "masked", "ghost chunk"]


def chunk_local_index(w, h):
    yy, xx = np.mgrid[0:h, 0:w]
    cw = np.minimum(CHUNK, w - xx // CHUNK * CHUNK)
    return (yy % CHUNK) * cw + xx % CHUNK


def preview_pair(w, h):
    """(active layer, preview): inside every chunk, pixel k holds combination 37 k % 90 of layer alpha x preview alpha x colours {0, 255, random}"""
    k = chunk_local_index(w, h) * 37 % 90   # 37 is coprime to 90: a chunk of 15 pixels already meets every colour class and most alphas
    colour = (k // 30) % 3
    out = []
    for seed, alpha in ((160, np.array(LAYER_ALPHAS)[k % 5]), (161, np.array(PREVIEW_ALPHAS)[(k // 5) % 6])):
        img = rgba(w, h, seed, alpha=alpha)
        img[..., :3] = np.where((colour == 0)[..., None], 0, np.where((colour == 1)[..., None], 255, img[..., :3]))
        out.append(img)
    return out[0], out[1]


def present(kind, w, h):
    cxn, cyn = chunk_grid(w, h)
    c = np.arange(cxn * cyn)
    return {"null": None, "ones": np.ones(cxn * cyn, np.uint8), "zeros": np.zeros(cxn * cyn, np.uint8),
            "checker": ((c % cxn + c // cxn) % 2 == 0).astype(np.uint8)}[kind]


class PreviewStacks:
    """the images of one canvas, shared by all its cases"""

    def __init__(self, w, h):
        self.w, self.h = w, h
        self.active, self.preview = preview_pair(w, h)
        self.ghost = self.active.copy()   # the active layer with its last chunk emptied of alpha but not of colour (a missing chunk reads as (0, 0, 0, 0), colour included)
        self.ghost[chunk_of_pixels(w, h) == int(np.prod(chunk_grid(w, h))) - 1, 3] = 0
        self.below, self.above = rgba(w, h, 162, alpha=143), rgba(w, h, 163, alpha=lane_alpha(w, h))
        self.mask = np.where(np.random.default_rng(164).random((h, w)) < 0.4, 0, rgba(w, h, 165)[..., 0]).astype(np.uint8)

    def layers(self, position, with_adj):
        """(stack, index of the active layer)"""
        a = dict(pixels=self.ghost if position == "ghost chunk" else self.active)
        lo, hi = dict(pixels=self.below), dict(pixels=self.above, mode=OVERLAY, opacity=0.7)
        if position == "bottom":
            stack, at = [dict(a, mode=MULTIPLY, opacity=0.6), lo, hi], 0
        elif position == "top":
            stack, at = [lo, hi, dict(a, opacity=0.5)], 2
        else:
            if position == "hidden":
                a["visible"] = False
            if position == "masked":
                a["mask"] = self.mask
            stack, at = [lo, a, hi], 1
        if with_adj:
            stack = stack[:at + 1] + [adj(ADJ_INVERT, (), 0.6)] + stack[at + 1:] + [adj(ADJ_MIXER, MIXERS["negative"], 0.9)]
        return stack, at


PREVIEW_KINDS = {"plain": {}, "eraser": dict(is_eraser=True), "replaces": dict(replaces_layer=True)}
D_FOLDED = [("plain", NORMAL), ("plain", XOR), ("plain", OVERWRITE), ("plain", OVERLAY), ("eraser", NORMAL), ("replaces", NORMAL)]


def group_d(w, h):
    """every preview mode x kind once (130 x 70 only: checkerboard, middle, with an adjustment layer); then chunk_present x position x adjustment layer for six
    (kind, mode) pairs on every canvas.  Both routes each."""
    S = PreviewStacks(w, h)
    cases = []

    def add(kind, mode, cp, position, with_adj):
        stack, at = S.layers(position, with_adj)
        pv = dict(pixels=S.preview, active_layer=at, blend_mode=mode, chunk_present=present(cp, w, h), **PREVIEW_KINDS[kind])
        for route in (STORE, DEV):
            cases.append(Case(f"{kind} mode {mode} chunk_present {cp} active {position} adj {with_adj} {route}", w, h, stack, route, preview=pv))

    if (w, h) == D_CANVASES[-1]:
        for mode in PREVIEW_MODES:
            for kind in PREVIEW_KINDS:
                add(kind, mode, "checker", "middle", True)
    for kind, mode in D_FOLDED:
        for cp in CHUNK_PRESENT:
            for position in POSITIONS:
                for with_adj in (False, True):
                    add(kind, mode, cp, position, with_adj)
    return cases


# ---------------------------------------------------------------------------------------------------------------- E: dirty rectangles
E_CANVASES = [(64, 64), (65, 65), (66, 3), (67, 66), (130, 70)]
E_VARIANT = 2   # roles concealed, ghost, empty, visible on the first four chunks: active, inactive, inactive, active around the corner (64, 64)


def rectangles(w, h):
    """[(name, rect)]: every x0 mod 4 x rw in 1 .. 8 on 2 - 3 rows, once inside the first chunk and once across the chunk corner at (64, 64) where the canvas has
    one; 1 x 1 at the corners; one full row, one full column"""
    out = []
    for a in range(4):
        for rw in range(1, 9):
            rh = min(2 + (a + rw) % 2, h)
            x0 = 4 + a
            if x0 + rw <= min(w, CHUNK):
                out.append((f"x0 % 4 = {a}, rw {rw}, inside a chunk", (x0, (3 * a + 5 * rw) % (min(h, CHUNK) - rh + 1), rw, rh)))
            x0 = 60 + a
            if w > CHUNK and x0 + rw <= w:
                out.append((f"x0 % 4 = {a}, rw {rw}, across x = 64", (x0, CHUNK + 1 - rh if h > CHUNK else 0, rw, rh)))   # its last row is row 64 where there is one
    out += [(f"1 x 1 at ({x}, {y})", (x, y, 1, 1)) for x in sorted({0, w - 1}) for y in sorted({0, h - 1})]
    out += [("one full row", (0, h // 2, w, 1)), ("one full column", (w - 1, 0, 1, h)), ("the first column", (0, 0, 1, h))]
    return out


def refused_rectangles(w, h):
    return [(w, 0, 1, 1), (0, h, 1, 1), (w - 1, 0, 2, 1), (0, h - 1, 1, 2), (0, 0, 0, 1), (0, 0, 1, 0), (0, 0, w + 1, 1), (2 ** 32 - 1, 0, 2, 1), (0, 2 ** 32 - 1, 1, 2)]


def group_e(w, h):
    cases = []
    for sname, layers in (("adjustment stack", compound_stack(w, h)), ("activity stack", activity_layers(w, h, E_VARIANT))):
        cases += [Case(f"{sname}: {name} {rect}", w, h, layers, STORE, rect=rect) for name, rect in rectangles(w, h)]
        cases += [Case(f"{sname}: refused {rect}", w, h, layers, STORE, rect=rect, expect=STATUS, bound="pfx_composite_region: pfx_rect_inside") for rect in refused_rectangles(w, h)]
    return cases


# ---------------------------------------------------------------------------------------------------------------- F: raster-only, off the fast path
F_CANVASES = [(193, 1), (67, 66)]
F_SLOW = [NAN, -0.5, -0.0, 0.0, 1e-44, float(f32(2.0) ** -41), below(FAST_DIV_MIN)]   # flatten_kernel<false, false>
F_FAST = [FAST_DIV_MIN, INF]                                                            # the threshold itself takes the fast side; +inf clamps to 1


def accumulator_alpha(n):
    """tests/test_gpu_blend_writeback.py: base_alpha — 64-pixel groups that are opaque, transparent, mixed lane by lane, partial, mixed, opaque"""
    i = np.arange(n)
    mixed = np.array([255, 0, 77, 255, 200, 0], np.uint8)[i % 6]
    kinds = [np.full(n, 255, np.uint8), np.zeros(n, np.uint8), mixed, np.full(n, 143, np.uint8), mixed, np.full(n, 255, np.uint8)]
    return np.choose((i // 64) % 6, kinds).astype(np.uint8)


def group_f(w, h):
    """[base, mode at 0.6, mode at the opacity under test, mode at 1.0]: one odd opacity takes the whole stack off the fast path"""
    route = DEV if h == 1 else STORE
    imgs = [rgba(w, h, 170, alpha=accumulator_alpha(w * h).reshape(h, w))] + [rgba(w, h, 171 + k, alpha=np.roll(lane_alpha(w, h).ravel(), k).reshape(h, w)) for k in range(3)]
    cases = []
    for mode in list(range(25)) + [25, 255]:
        for opacity in F_SLOW + F_FAST:
            layers = [dict(pixels=imgs[0]), dict(pixels=imgs[1], mode=mode, opacity=0.6), dict(pixels=imgs[2], mode=mode, opacity=opacity), dict(pixels=imgs[3], mode=mode)]
            cases.append(Case(f"mode {mode} opacity {opacity!r}", w, h, layers, route))
    return cases


# ---------------------------------------------------------------------------------------------------------------- G: an editing session
STATE_STEPS = ["upload", "upload_same_generation", "open_hole", "close_hole", "set_mask", "clear_mask", "remove_layer", "name_missing_index", "set_mode",
               "set_opacity", "set_visibility", "insert_adjustment", "remove_adjustment"]
COMPOSITE_STEPS = ["composite_full", "composite_repeat", "composite_rect", "composite_preview"]
SESSION_CANVAS = (130, 70)
SESSION_SEEDS = [11, 12, 13]
SESSION_OPACITIES = [1.0, 1.0, 0.5, 0.25, below(1.0), 0.0]   # 0.0: the slow instantiations come by as well
HOLE = (70, 6, 9, 5)    # x, y, w, h inside chunk 1, which layer 1 starts with as opaque


class Document:
    """the numpy mirror: what the layer store holds and the layer list bottom -> top.  Arrays are replaced, never written, so a step's snapshot stays valid"""

    def __init__(self, w, h):
        self.w, self.h, self.store, self.order = w, h, {}, []

    def layers(self):
        out = []
        for e in self.order:
            if "kind" in e:
                out.append(dict(e))
            else:
                held = self.store.get(e["idx"])
                out.append(dict(pixels=None if held is None else held["pixels"], mask=None if held is None else held["mask"], opacity=e["opacity"], mode=e["mode"], visible=e["visible"]))
        return out

    def info(self):
        """the tuples GpuRenderer._infos takes; adjustment layers carry index 0, which nothing reads"""
        return [(0, e["opacity"], e["visible"], 0, e["kind"], tuple(e["adj"])) if "kind" in e else (e["idx"], e["opacity"], e["visible"], e["mode"]) for e in self.order]


def session_alpha(rng, w, h, kinds=None):
    """per chunk: opaque, holed (alpha 0 on a fifth of the pixels, 255 elsewhere) or empty"""
    n = int(np.prod(chunk_grid(w, h)))
    kinds = rng.integers(0, 3, n) if kinds is None else np.asarray(kinds)
    holes = np.where(rng.random((h, w)) < 0.2, 0, 255)
    return np.choose(kinds[chunk_of_pixels(w, h)], [np.full((h, w), 255), holes, np.zeros((h, w), int)]).astype(np.uint8)


def session(seed, n_layers=6, n_steps=72):
    """(steps, document): steps are dicts with `kind` in STATE_STEPS + COMPOSITE_STEPS; a composite step carries the layer list and info of that moment.  A fixed
    prologue meets every step kind in an order that can leave each host cache stale (mask on / off, hole opened / closed, adjustment in / out, preview on /
    off, each followed by composites, the full one twice so that pending verdicts resolve); seeded random steps follow up to n_steps"""
    w, h = SESSION_CANVAS
    rng = np.random.default_rng(seed)
    doc = Document(w, h)
    steps = []
    generation = [0]

    def composite(kind, **kw):
        steps.append(dict(kind=kind, layers=doc.layers(), info=doc.info(), **kw))

    def full(twice=True):
        composite("composite_full")
        if twice:
            composite("composite_repeat")

    def rect():
        rw, rh = int(rng.integers(1, 40)), int(rng.integers(1, 30))
        composite("composite_rect", rect=(int(rng.integers(0, w - rw + 1)), int(rng.integers(0, h - rh + 1)), rw, rh))

    def preview():
        px = rgba(w, h, int(rng.integers(1 << 30)))
        px[..., 3] = np.where(rng.random((h, w)) < 0.6, 0, px[..., 3])
        px[:, CHUNK:2 * CHUNK] = 0   # a chunk column without preview
        # the active layer is a stored raster layer or an adjustment layer (then only the preview's chunks count), never the index that was not uploaded
        choice = [i for i, e in enumerate(doc.order) if "kind" in e or e["idx"] in doc.store]
        composite("composite_preview", preview=dict(pixels=px, active_layer=int(rng.choice(choice)), blend_mode=int(rng.integers(0, 27)),
                                                    is_eraser=bool(rng.random() < 0.2), replaces_layer=bool(rng.random() < 0.2)))

    def upload(idx, kinds=None, same_generation=False):
        px = rgba(w, h, int(rng.integers(1 << 30)), alpha=session_alpha(rng, w, h, kinds))
        if same_generation:
            steps.append(dict(kind="upload_same_generation", idx=idx, pixels=px, generation=doc.store[idx]["generation"]))   # ignored: the mirror keeps its pixels
            return
        generation[0] += 1
        doc.store[idx] = dict(pixels=px, mask=doc.store.get(idx, {}).get("mask"), generation=generation[0])
        steps.append(dict(kind="upload", idx=idx, pixels=px, generation=generation[0]))

    def patch(idx, alpha, kind):
        x, y, pw, ph = HOLE
        p = rgba(pw, ph, int(rng.integers(1 << 30)), alpha=alpha)
        px = doc.store[idx]["pixels"].copy()
        px[y:y + ph, x:x + pw] = p
        doc.store[idx] = dict(doc.store[idx], pixels=px)
        steps.append(dict(kind=kind, idx=idx, x=x, y=y, pixels=p))

    def mask(idx, on):
        m = np.where(rng.random((h, w)) < 0.3, 0, rng.integers(0, 256, (h, w))).astype(np.uint8) if on else None
        doc.store[idx] = dict(doc.store[idx], mask=m)
        steps.append(dict(kind="set_mask" if on else "clear_mask", idx=idx, mask=m))

    def rasters():
        return [e for e in doc.order if "kind" not in e and e["idx"] in doc.store]

    def insert_adjustment():
        kind = int(rng.integers(1, 5))
        params = {ADJ_EXPOSURE: [float(rng.uniform(-2, 2))], ADJ_BC: [float(rng.uniform(-80, 80)), float(rng.uniform(-90, 90))], ADJ_INVERT: [],
                  ADJ_MIXER: [float(v) for v in rng.uniform(-0.5, 1.2, 16)]}[kind]
        doc.order.insert(int(rng.integers(0, len(doc.order) + 1)), dict(kind=kind, adj=params, opacity=float(rng.choice([1.0, 0.6, 0.0])), visible=True))
        steps.append(dict(kind="insert_adjustment"))

    def remove_adjustment():
        doc.order.remove(next(e for e in doc.order if "kind" in e))
        steps.append(dict(kind="remove_adjustment"))

    def describe(kind, e=None):
        e = e or rasters()[int(rng.integers(0, len(rasters())))]
        if kind == "set_mode":
            e["mode"] = int(rng.integers(0, 27))
        elif kind == "set_opacity":
            e["opacity"] = float(rng.choice(SESSION_OPACITIES))
        else:
            e["visible"] = not e["visible"]
        steps.append(dict(kind=kind))

    # ---- prologue
    for idx in range(n_layers):
        kinds = None if idx > 1 else ([0] * 6 if idx == 0 else [1, 0, 2, 0, 1, 0])   # layer 0 opaque; layer 1: chunk 1 opaque (a start-table entry), others holed or empty
        upload(idx, kinds)
        doc.order.append(dict(idx=idx, opacity=1.0 if idx < 2 else float(rng.choice(SESSION_OPACITIES[:5])), mode=NORMAL if idx < 2 else int(rng.integers(0, 25)), visible=True))
    full()
    upload(2, same_generation=True); full(twice=False)
    patch(1, 0, "open_hole"); full()
    patch(1, 255, "close_hole"); full()
    mask(3, True); rect(); full(twice=False)
    mask(3, False); full()
    insert_adjustment(); preview(); full(twice=False); rect()
    remove_adjustment(); full()
    preview(); full(twice=False)
    steps.append(dict(kind="remove_layer", idx=4)); del doc.store[4]; full()
    doc.order.insert(2, dict(idx=900 + seed, opacity=0.5, mode=MULTIPLY, visible=True)); steps.append(dict(kind="name_missing_index")); full(twice=False)
    for kind in ("set_mode", "set_opacity", "set_visibility"):
        describe(kind); full(twice=False)
    describe("set_visibility", next(e for e in doc.order if not e["visible"]))   # back on
    upload(4); full()
    # ---- seeded random steps
    while len(steps) < n_steps:
        roll = rng.random()
        masked = [i for i, s in doc.store.items() if s["mask"] is not None]
        if roll < 0.12:
            upload(int(rng.choice(list(doc.store))))
        elif roll < 0.18:
            upload(int(rng.choice(list(doc.store))), same_generation=True)
        elif roll < 0.30:
            alpha = int(rng.choice([0, 255]))
            patch(1, alpha, "open_hole" if alpha == 0 else "close_hole")
        elif roll < 0.40:
            mask(masked[0], False) if masked else mask(int(rng.choice(list(doc.store))), True)
        elif roll < 0.52:
            remove_adjustment() if any("kind" in e for e in doc.order) else insert_adjustment()
        else:
            describe(str(rng.choice(["set_mode", "set_opacity", "set_visibility"])))
        roll = rng.random()
        if roll < 0.5:
            full(twice=rng.random() < 0.5)
        elif roll < 0.75:
            rect()
        else:
            preview()
    return steps, doc
