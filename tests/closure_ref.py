"""Host reference for per-pixel closures: the tree-walking interpreter (pfx_rhai.cpp: Interp / Eval) runs the closure on chosen
pixels, and the shape probe reports how the device would compile and launch it.  Both are test seams of libpfx.so that need no
device (pfx_internal.h: pfx_int_script_check_console, pfx_int_script_closure_shape).

Inputs come from integer hash formulas of (x, y, c): numpy builds the device image from them, and a script prelude defines
`fn get_r(x, y)` .. `fn is_selected(x, y)` from the same formulas for the host (script functions win over the host API)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from paintfe_amd import _lib
from paintfe_amd._lib import PfxError, ScriptResult

SHAPE_FIELDS = 9
SHAPE_KEYS = ("n_params", "n_regs", "n_code", "n_pre", "heavy", "lanes", "lcode", "lds_bytes", "bc_count")
# BcOp (pfx_rhai.h) in declaration order
BC_NAMES = ("LOADK MOV IADD ISUB IMUL IDIV IMOD INEG IPOW IAND IOR IXOR ISHL ISHR IABS IMIN IMAX ICLAMP ISIGN IEQ INE ILT ILE IGT IGE "
            "FADD FSUB FMUL FDIV FMOD FNEG FPOW FABS FMIN FMAX FCLAMP FFLOOR FCEIL FROUND FSQRT FSIN FCOS FTAN FATAN2 FEXP FLN FLERP FDIST "
            "FEQ FNE FLT FLE FGT FGE I2F F2I NOT JMP JZ JNZ GETCH ISSEL RET_ARR RET_UNIT ERR").split()


def _fn(name, argtypes):
    f = getattr(_lib.load(), name)
    f.argtypes = argtypes
    f.restype = C.c_int
    return f


def closure_shape(source: str, w: int, h: int) -> dict:
    """compiled form and launch shape of the script's first bulk-iterator closure; raises PfxError(status) if it does not compile"""
    f = _fn("pfx_int_script_closure_shape", [C.c_char_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_int64), C.c_int])
    cap = SHAPE_FIELDS + 128
    buf = (C.c_int64 * cap)()
    st = f(source.encode(), w, h, buf, cap)
    if st != _lib.OK:
        raise PfxError(st, "closure shape probe")
    d = {k: int(buf[i]) for i, k in enumerate(SHAPE_KEYS)}
    assert d["bc_count"] == len(BC_NAMES), "BcOp changed: update BC_NAMES"
    d["ops"] = {BC_NAMES[i]: int(buf[SHAPE_FIELDS + i]) for i in range(d["bc_count"])}
    return d


def check_console(source: str, w: int = 64, h: int = 64):
    """pfx_script_check with the whole console: (lines, None) or (lines so far, (status, line, message))"""
    f = _fn("pfx_int_script_check_console", [C.c_char_p, C.c_uint32, C.c_uint32, C.POINTER(ScriptResult), C.c_char_p, C.c_size_t,
                                              C.POINTER(C.c_size_t)])
    cap = 1 << 20
    while True:
        res, buf, n = ScriptResult(), C.create_string_buffer(cap), C.c_size_t()
        st = f(source.encode(), w, h, C.byref(res), buf, cap, C.byref(n))
        if n.value < cap:
            break
        cap = n.value + 1
    lines = buf.value.decode().split("\n")[:-1]   # every line ends with '\n'; a unit prints as an empty line
    if st != _lib.OK:
        return lines, (st, res.error_line, error_text(res.error.decode(errors="replace")))
    return lines, None


def error_text(friendly: str) -> str:
    """the message of a 'Error on line N[, column C]:\\n  <message>' text"""
    return friendly.split("\n", 1)[1].strip() if "\n" in friendly else friendly.strip()


def same_error(device_msg: str, host_msg: str) -> bool:
    """equal up to the host's operand detail (': 5 / 0', '(1e30)')"""
    return host_msg == device_msg or host_msg.startswith(device_msg + ": ") or host_msg.startswith(device_msg + "(")


# ---------------------------------------------------------------- inputs
def hash_px(x, y, c):
    return ((x * 37 + y * 91 + c * 53) ^ (x * y * 13 + c * 101) ^ (y >> 1)) & 255


def hash_mask(x, y):
    return ((x * 29 + y * 17) & 7) * 36


def image(w: int, h: int):
    y, x = np.mgrid[0:h, 0:w].astype(np.int64)
    img = np.stack([hash_px(x, y, c) for c in range(4)], axis=-1).astype(np.uint8)
    return img, hash_mask(x, y).astype(np.uint8)


def prelude(w: int, h: int) -> str:
    """the host's image API, from the same formulas (0 outside the image, like the device's reads)"""
    out = f"x < 0 || y < 0 || x >= {w} || y >= {h}"
    s = []
    for c, n in enumerate("rgba"):
        s.append(f"fn get_{n}(x, y) {{ if {out} {{ 0 }} else {{ ((x * 37 + y * 91 + {c * 53}) ^ (x * y * 13 + {c * 101}) ^ (y >> 1)) & 255 }} }}")
    s.append("fn get_pixel(x, y) { [get_r(x, y), get_g(x, y), get_b(x, y), get_a(x, y)] }")
    s.append(f"fn is_selected(x, y) {{ if {out} {{ false }} else {{ ((x * 29 + y * 17) & 7) * 36 > 0 }} }}")
    return "\n".join(s)


def parse_result(line: str):
    """a printed closure result -> list of elements (int, or None for anything else) or None for a non-array"""
    if not line.startswith("["):
        return None
    body = line[1:-1].strip()
    if not body:
        return []
    out = []
    for tok in body.split(", "):
        try:
            out.append(int(tok))
        except ValueError:
            out.append(None)
    return out


def write_back(old, res):
    """the bulk iterators' rule: an array of >= 4 elements updates each channel whose element is an integer, clamped to 0..255"""
    if res is None or len(res) < 4:
        return tuple(int(v) for v in old)
    return tuple(int(old[k]) if res[k] is None else min(max(res[k], 0), 255) for k in range(4))


def host_run(prog, pixels, w: int, h: int):
    """run program `prog` (closure_gen.Program) on the host at the (x, y) pixels in order: ([(x, y, result-or-None)], error-or-None)"""
    calls = []
    for (x, y) in pixels:
        args = ", ".join([str(x), str(y)] * (len(prog.params) == 6) + [f"get_{n}({x}, {y})" for n in "rgba"])
        calls.append(f"print(f.call({args}));")
    src = prog.host_closure() + "\n" + "\n".join(calls) + "\n" + prelude(w, h)
    lines, err = check_console(src, w, h)
    return [parse_result(s) for s in lines], err


def host_loop(prog, region, w: int, h: int):
    """like host_run over every pixel of `region` (x0, y0, x1, y1) in row-major order, with a script loop instead of one line per pixel"""
    x0, y0, x1, y1 = region
    args = "x, y, " if len(prog.params) == 6 else ""
    loop = (f"for y in {y0}..{y1} {{ for x in {x0}..{x1} {{ print(f.call({args}get_r(x, y), get_g(x, y), get_b(x, y), get_a(x, y))); }} }}")
    src = prog.host_closure() + "\n" + loop + "\n" + prelude(w, h)
    lines, err = check_console(src, w, h)
    return [parse_result(s) for s in lines], err
