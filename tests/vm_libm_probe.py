"""A probe of the script VM's f64 opcodes through the public script ABI (k_script.hip: vm_kernel, HEAVY instantiation).

One per-pixel closure evaluates one operation per probe: probe i sits in row i // G, pixels 5 * (i % G) .. + 4 — two pixels hold the eight
bytes of argument a (low word first, r = least significant byte), two hold b, the fifth holds the opcode in r.  The closure decodes a and b
with exact integer and power-of-two arithmetic only, applies the opcode, and writes the result's 64 bits back as the bytes of the probe's
first two pixels (low word, high word); the other three pixels keep their value.  NaN comes back as 0x7ff8000000000000 whatever its sign
and payload (a script cannot observe them).

The same closure runs on the host interpreter (pfx_rhai.cpp) through closure_ref's console seam, with a prelude `fn get_pixel` that serves
the probe bytes, so device and host see the same program and the same arguments.  The libm seam (pfx_int_script_libm_hook) traces and
overrides the interpreter's pow / sin / cos / tan / atan2 / exp / ln inside closures: device_table() answers a trace with the device's values."""
from __future__ import annotations

import ctypes as C
import ctypes.util
import struct
from fractions import Fraction

import numpy as np

from paintfe_amd import _lib
from paintfe_amd._lib import PfxError

from . import closure_ref as R

# opcode -> (source of the result, reads b); `a ** n` takes n = to_int(b), so its b must hold an integer
OPS = {
    "pow": "pow(va, vb)", "powop": "va ** vb", "powi": "va ** to_int(vb)", "sin": "sin(va)", "cos": "cos(va)", "tan": "tan(va)",
    "atan2": "atan2(va, vb)", "exp": "exp(va)", "ln": "ln(va)", "sqrt": "sqrt(va)", "fmod": "va % vb", "floor": "floor(va)",
    "ceil": "ceil(va)", "round": "round(va)", "min": "min(va, vb)", "max": "max(va, vb)",
}
OPCODE = {name: k for k, name in enumerate(OPS)}
LIBM = ("pow", "powop", "powi", "sin", "cos", "tan", "atan2", "exp", "ln")
# rhai::LibmOp (pfx_rhai.h) of the seam, and the probe opcode that evaluates it on the device
HOOK_OPS = ("pow", "sin", "cos", "tan", "atan2", "exp", "ln")
# probe opcode -> the function whose accuracy bound applies
FUNCTION = {"pow": "pow", "powop": "pow", "powi": "pow", "sin": "sin", "cos": "cos", "tan": "tan", "atan2": "atan2", "exp": "exp", "ln": "ln"}
G = 64                     # probes per image row
NAN_BITS = 0x7FF8000000000000


def p2(k: int) -> str:
    return repr(2.0 ** k)


def _decode_fn() -> str:
    # v = m * 2^s in binary steps: g runs through 2^512, 2^256, .. 2^1 (or their inverses) by sqrt, which is exact on even powers of two
    return f"""fn probe_dec(x, y) {{
    let lo = 0;
    let hi = 0;
    lo = get_r(x, y) | (get_g(x, y) << 8) | (get_b(x, y) << 16) | (get_a(x, y) << 24);
    hi = get_r(x + 1, y) | (get_g(x + 1, y) << 8) | (get_b(x + 1, y) << 16) | (get_a(x + 1, y) << 24);
    let e = 0;
    e = (hi >> 20) & 2047;
    let m = 0;
    m = ((hi & 1048575) << 32) | lo;
    let v = 0.0;
    if e == 2047 {{
        if m == 0 {{ v = 1.0 / 0.0; }} else {{ v = 0.0 / 0.0; }}
    }} else {{
        if e > 0 {{ m = m | 4503599627370496; }} else {{ e = 1; }}
        v = to_float(m);
        let s = 0;
        s = e - 1075;
        let g = 0.0;
        g = {p2(512)};
        if s < 0 {{
            s = -s;
            g = 1.0 / g;
            if s >= 512 {{ v = v * g; s -= 512; }}
        }}
        let k = 512;
        while k > 0 {{
            if s >= k {{ v = v * g; s -= k; }}
            k = k / 2;
            g = sqrt(g);
        }}
    }}
    if (hi >> 31) == 1 {{ v = -(v); }}
    v
}}"""


def _encode_fn() -> str:
    # |y| = v * 2^(be - 1075) with v normalised into [2^52, 2^53) by the same binary steps; a subnormal scales by 2^1074 into its integer
    return f"""fn probe_enc(y, k) {{
    let hi = 0;
    let lo = 0;
    if y != y {{
        hi = 2146959360;
    }} else if y == 1.0 / 0.0 {{
        hi = 2146435072;
    }} else if y == -1.0 / 0.0 {{
        hi = 4293918720;
    }} else if y == 0.0 {{
        if 1.0 / y < 0.0 {{ hi = 2147483648; }}
    }} else {{
        let v = 0.0;
        v = y;
        let sg = 0;
        if v < 0.0 {{ sg = 2147483648; v = -(v); }}
        let m = 0;
        let be = 1075;
        if v < {p2(-1022)} {{
            m = to_int(v * {p2(1022)} * {p2(52)});
            be = 0;
        }} else {{
            let g = 0.0;
            g = {p2(512)};
            let s = 0;
            s = 512;
            while s > 0 {{
                if v >= 4503599627370496.0 * g {{ v = v / g; be += s; }}
                s = s / 2;
                g = sqrt(g);
            }}
            if v < {p2(53 - 512)} {{ v = v * {p2(512)}; be -= 512; }}
            g = {p2(512)};
            s = 512;
            while s > 0 {{
                if v < 9007199254740992.0 / g {{ v = v * g; be -= s; }}
                s = s / 2;
                g = sqrt(g);
            }}
            m = to_int(v) - 4503599627370496;
        }}
        hi = sg | (be << 20) | (m >> 32);
        lo = m & 4294967295;
    }}
    if k == 0 {{ lo }} else {{ hi }}
}}"""


def closure(n_pad: int = 0) -> str:
    """the probe closure (for_each_pixel parameters); n_pad statements in a branch no probe takes lengthen the program past what the LDS
    stages next to its registers (LCODE = false) without adding steps"""
    chain = " else ".join(f"if op == {OPCODE[n]} {{ res = {src}; }}" for n, src in OPS.items())
    pads = "".join(f"            w = w ^ {j + 3};\n" for j in range(n_pad))
    pad = f"        if k > 4 {{\n{pads}        }}\n" if n_pad else ""
    return f"""|x, y, r, g, b, a| {{
    let k = 0;
    k = x % 5;
    if k < 2 {{
        let x0 = 0;
        x0 = x - k;
        let va = 0.0;
        va = probe_dec(x0, y);
        let vb = 0.0;
        vb = probe_dec(x0 + 2, y);
        let op = 0;
        op = get_r(x0 + 4, y);
        let res = 0.0;
        {chain}
        let w = 0;
        w = probe_enc(res, k);
{pad}        [w & 255, (w >> 8) & 255, (w >> 16) & 255, (w >> 24) & 255]
    }} else {{
        [r, g, b, a]
    }}
}}"""


def functions() -> str:
    return _decode_fn() + "\n" + _encode_fn()


# the register pads of the two LCODE classes (checked through closure_shape by the tests)
PADS = {True: 0, False: 1000}


def device_script(lcode: bool = True) -> str:
    return functions() + "\nfor_each_pixel(" + closure(PADS[lcode]) + ");"


# ---------------------------------------------------------------- bits
def f2b(v: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", v))[0]


def b2f(b: int) -> float:
    return struct.unpack("<d", struct.pack("<Q", int(b) & 0xFFFFFFFFFFFFFFFF))[0]


def canon(b: int) -> int:
    """NaN bits -> the one NaN a probe reports"""
    b = int(b)
    return NAN_BITS if (b >> 52) & 0x7FF == 0x7FF and b & ((1 << 52) - 1) else b


def ordered(b: int) -> int:
    """a monotone integer image of a double's bits: the distance of two finite doubles in ulps is the difference"""
    b = int(b)
    return -(b & 0x7FFFFFFFFFFFFFFF) if b >> 63 else b


UNBOUNDED = 1 << 64


def ulps(x: int, y: int) -> int:
    """the distance in ulps of two finite doubles of the same class; a change of class — NaN against a number, an infinity against anything
    else, +0 against -0 — is UNBOUNDED, so DBL_MAX for inf or +0 for -0 is never '1 ulp'"""
    x, y = canon(x), canon(y)
    if x == y:
        return 0
    special = lambda b: (b >> 52) & 0x7FF == 0x7FF or b & 0x7FFFFFFFFFFFFFFF == 0
    if special(x) and special(y) or (x >> 52) & 0x7FF == 0x7FF or (y >> 52) & 0x7FF == 0x7FF:
        return UNBOUNDED
    return abs(ordered(x) - ordered(y))


# ---------------------------------------------------------------- images
def _args(probe):
    op, a = probe[0], probe[1]
    b = probe[2] if len(probe) > 2 else 0.0
    return OPCODE[op], f2b(float(a)), f2b(float(b))


def image(probes):
    """(H, 5 * G, 4) uint8 holding the probes row by row; unused slots hold floor(0.0)"""
    n = len(probes)
    h = max(1, -(-n // G))
    img = np.zeros((h, 5 * G, 4), np.uint8)
    slots = img.reshape(h, G, 5, 4)
    slots[:, :, 4, 0] = OPCODE["floor"]
    for i, p in enumerate(probes):
        op, a, b = _args(p)
        y, s = divmod(i, G)
        for j, word in enumerate((a & 0xFFFFFFFF, a >> 32, b & 0xFFFFFFFF, b >> 32)):
            slots[y, s, j] = [(word >> (8 * c)) & 255 for c in range(4)]
        slots[y, s, 4, 0] = op
    return img


def results(img, n):
    """the probes' result bits from an output image"""
    h = img.shape[0]
    words = img.reshape(h, G, 5, 4)[:, :, :2].astype(np.uint64)
    w = words[..., 0] | (words[..., 1] << np.uint64(8)) | (words[..., 2] << np.uint64(16)) | (words[..., 3] << np.uint64(24))
    bits = w[..., 0] | (w[..., 1] << np.uint64(32))
    return [int(v) for v in bits.reshape(-1)[:n]]


def device_eval(r, probes, lcode: bool = True):
    img = image(probes)
    out, _ = r.execute_script_sync(device_script(lcode), img, None)
    return results(out, len(probes))


def shape(lcode: bool = True):
    img = image([("floor", 0.0)])
    return R.closure_shape(device_script(lcode), img.shape[1], img.shape[0])


def _prelude(img) -> str:
    rows = []
    for y in range(img.shape[0]):
        rows.append(f"        {y} => [{', '.join(str(int(v)) for v in img[y, :, :].reshape(-1))}]")
    return ("fn px(x, y, c) {\n    let t = switch y {\n" + ",\n".join(rows) + ",\n        _ => []\n    };\n"
            "    t[4 * x + c]\n}\n" + "\n".join(f"fn get_{n}(x, y) {{ px(x, y, {c}) }}" for c, n in enumerate("rgba")))


def host_eval(probes, batch: int = 64):
    """the probes through the host interpreter: the same closure, called per output pixel, reading the probe bytes through the prelude"""
    out = []
    for lo in range(0, len(probes), batch):
        part = probes[lo:lo + batch]
        img = np.zeros((len(part), 5, 4), np.uint8)
        full = image(part)
        for i in range(len(part)):
            y, s = divmod(i, G)
            img[i] = full[y, 5 * s:5 * s + 5]
        calls = []
        for i in range(len(part)):
            for k in range(2):
                calls.append(f"print(f.call({k}, {i}, {', '.join(str(int(v)) for v in img[i, k])}));")
        src = "\n".join([functions(), "let f = " + closure(0) + ";", *calls, _prelude(img)])
        lines, err = R.check_console(src, 5, len(part))
        assert err is None, err
        for i in range(len(part)):
            lo_w, hi_w = (R.parse_result(lines[2 * i + k]) for k in range(2))
            word = [sum(int(v) << (8 * c) for c, v in enumerate(wd)) for wd in (lo_w, hi_w)]
            out.append(word[0] | (word[1] << 32))
    return out


# ---------------------------------------------------------------- glibc and the correctly rounded referee
_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_C1 = {"sin": "sin", "cos": "cos", "tan": "tan", "exp": "exp", "ln": "log", "sqrt": "sqrt", "floor": "floor", "ceil": "ceil", "round": "round"}
_C2 = {"pow": "pow", "powop": "pow", "powi": "pow", "atan2": "atan2", "fmod": "fmod", "min": "fmin", "max": "fmax"}
for _n in set(_C1.values()) | set(_C2.values()):
    getattr(_libm, _n).restype = C.c_double
    getattr(_libm, _n).argtypes = [C.c_double] * (2 if _n in _C2.values() else 1)


def glibc(probe) -> int:
    op, a = probe[0], float(probe[1])
    b = float(probe[2]) if len(probe) > 2 else 0.0
    if op == "powi":
        b = float(int(b))
    v = getattr(_libm, _C2[op])(a, b) if op in _C2 else getattr(_libm, _C1[op])(a)
    return canon(f2b(v))


def referee(probe) -> int:
    """mpmath at 200 bits, rounded once to f64 (finite, non-NaN arguments and results only); sin / cos / tan of a large argument work with
    its binary exponent's worth of extra bits, so the reduction by pi is 200 bits deep too"""
    import math

    import mpmath
    op, a = probe[0], probe[1]
    b = probe[2] if len(probe) > 2 else 0.0
    extra = max(0, math.frexp(a)[1]) if op in ("sin", "cos", "tan") else 0
    # far outside the range (pow(1e300, 1e300)): the magnitude alone decides, without an mpmath number of that size
    t = a if op == "exp" else (b * math.log2(abs(a)) if op in ("pow", "powop", "powi") and a not in (0.0, INF, -INF) and abs(b) != INF else 0.0)
    if abs(t) > 1200:
        if op != "exp" and a < 0 and b != int(b):
            raise ValueError(f"complex referee for {probe}")
        neg = op != "exp" and a < 0 and int(b) % 2 == 1
        return f2b((-1.0 if neg else 1.0) * (INF if t > 0 else 0.0))
    with mpmath.workprec(200 + extra):
        x, y = mpmath.mpf(a), mpmath.mpf(b)
        f = {"pow": lambda: mpmath.power(x, y), "powop": lambda: mpmath.power(x, y), "powi": lambda: mpmath.power(x, y),
             "sin": lambda: mpmath.sin(x), "cos": lambda: mpmath.cos(x), "tan": lambda: mpmath.tan(x), "atan2": lambda: mpmath.atan2(x, y),
             "exp": lambda: mpmath.exp(x), "ln": lambda: mpmath.log(x)}[op]
        try:
            f = f()
        except ZeroDivisionError:
            raise ValueError(f"infinite referee for {probe}") from None   # pow(0, -1.5)
        if isinstance(f, mpmath.mpc):
            raise ValueError(f"complex referee for {probe}")
        sign, man, exp, _ = f._mpf_
    if man == 0:
        if exp != 0:
            raise ValueError(f"infinite or NaN referee for {probe}")   # mpmath's inf / nan: leave such entries to the special table
        # mpmath has no signed zero: an exact zero takes the sign IEEE gives it (odd functions and atan2 follow their first argument;
        # pow(x, n) of a zero base is negative for a negative base and an odd integer n)
        if op in ("sin", "tan", "atan2"):
            return f2b(math.copysign(0.0, a))
        if op in ("pow", "powop", "powi"):
            odd = b == int(b) and int(b) % 2 == 1
            return f2b(math.copysign(0.0, a) if odd else 0.0)
        return f2b(0.0)
    q = (-1) ** sign * Fraction(int(man)) * (Fraction(2) ** int(exp))
    try:
        v = q.numerator / q.denominator    # int / int is correctly rounded, subnormals included
    except OverflowError:
        v = float("inf") if q > 0 else float("-inf")
    return f2b(v)


# ---------------------------------------------------------------- the libm seam
def hook(mode: int, table=None):
    """mode 0 off, 1 trace, 2 override from table {(op, a bits, b bits): result bits}"""
    f = getattr(_lib.load(), "pfx_int_script_libm_hook")
    f.argtypes = [C.c_int, C.POINTER(C.c_uint64), C.c_size_t]
    f.restype = C.c_int
    rows = sorted((table or {}).items())
    buf = (C.c_uint64 * max(1, 4 * len(rows)))()
    for i, ((op, a, b), v) in enumerate(rows):
        buf[4 * i:4 * i + 4] = [op, a, b, v]
    st = f(mode, buf, len(rows))
    if st != _lib.OK:
        raise PfxError(st, "libm hook")


def trace():
    """(distinct [(op, a bits, b bits)] recorded since the last hook(), override misses)"""
    f = getattr(_lib.load(), "pfx_int_script_libm_trace")
    f.argtypes = [C.POINTER(C.c_uint64), C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_uint64)]
    f.restype = C.c_int
    n, miss = C.c_size_t(), C.c_uint64()
    st = f(None, 0, C.byref(n), C.byref(miss))
    assert st == _lib.OK
    buf = (C.c_uint64 * max(1, 3 * n.value))()
    st = f(buf, n.value, C.byref(n), C.byref(miss))
    assert st == _lib.OK
    return [tuple(int(v) for v in buf[3 * i:3 * i + 3]) for i in range(n.value)], int(miss.value)


class traced:
    """with traced() as t: ... — the libm calls of closure bodies evaluated in the block, in t.calls"""
    def __init__(self, table=None):
        self.table = table

    def __enter__(self):
        hook(2 if self.table is not None else 1, self.table)
        self.calls, self.misses = [], 0
        return self

    def __exit__(self, *exc):
        self.calls, self.misses = trace()
        hook(0)
        return False


def call_probe(call):
    op, a, b = call
    name = HOOK_OPS[op]
    return (name, b2f(a), b2f(b)) if name in ("pow", "atan2") else (name, b2f(a))


def device_table(r, calls):
    """the device's result bits for traced calls: {(op, a bits, b bits): bits}"""
    if not calls:
        return {}
    got = device_eval(r, [call_probe(c) for c in calls])
    return {c: v for c, v in zip(calls, got)}


def nudge(table, k: int):
    """every finite result moved by k ulps (away from zero; zeros to the k-th subnormal)"""
    out = {}
    for c, v in table.items():
        if (v >> 52) & 0x7FF == 0x7FF:
            out[c] = v
        else:
            out[c] = ((v & 0x7FFFFFFFFFFFFFFF) + k) | (v & 0x8000000000000000) if (v & 0x7FFFFFFFFFFFFFFF) + k < 0x7FF0000000000000 else v
    return out


# ---------------------------------------------------------------- argument tables
INF, NAN = float("inf"), float("nan")
DBL_MAX, DBL_MIN, SUB_MIN, SUB_MAX = 1.7976931348623157e308, 2.2250738585072014e-308, 5e-324, 2.225073858507201e-308
HALF_DOWN = 0.49999999999999994           # the largest double below 0.5: round() must give 0
SPECIAL = [0.0, -0.0, INF, -INF, NAN, 1.0, -1.0, 0.5, -0.5, 2.0, -2.0, 3.0, -3.0, 2.5, -2.5, 1.5, -1.5, SUB_MIN, -SUB_MIN, SUB_MAX, -SUB_MAX,
           DBL_MIN, -DBL_MIN, DBL_MAX, -DBL_MAX, HALF_DOWN, -HALF_DOWN, 4503599627370495.5, -4503599627370495.5, 4503599627370497.0, 1e-300,
           1e300, -1e300]
# exp's overflow and underflow thresholds (the last finite and the first inf result, the last normal, the last nonzero and the first zero
# result): prescribed entries, held bit for bit
EXP_THRESHOLDS = (709.782712893384, 709.7827128933841, -708.3964185322641, -708.3964185322642, -745.1332191019411, -745.1332191019412,
                  -744.4400719213812)
# ln and trig edges
UNARY_EDGES = [*EXP_THRESHOLDS, 1e-310, -1e-310, 1e22, -1e22, 1e308, 3.141592653589793, 1.5707963267948966, -1.5707963267948966, 6.283185307179586, 0.1, 255.0]
PAIR = [0.0, -0.0, INF, -INF, NAN, 1.0, -1.0, 0.5, -0.5, 2.0, -2.0, 3.0, -3.0, 2.5, -2.5, SUB_MIN, -SUB_MIN, DBL_MAX, -DBL_MAX]
POWI_N = [0, 1, -1, 2, -2, 3, -3, 4, 5, -5, 63, 1023, 1024, -1074, -1075, 9007199254740993]
UNARY = ("sin", "cos", "tan", "exp", "ln", "sqrt", "floor", "ceil", "round")
BINARY = ("pow", "powop", "atan2", "fmod", "min", "max")


def specials():
    """C99 Annex F / IEEE 754 §9.2 special arguments for every opcode: unary ops on SPECIAL + UNARY_EDGES, binary ops on PAIR x PAIR, `a ** n` on
    PAIR x POWI_N"""
    out = [(op, a) for op in UNARY for a in SPECIAL + UNARY_EDGES]
    out += [(op, a, b) for op in BINARY for a in PAIR for b in PAIR]
    out += [("powi", a, float(n)) for a in PAIR for n in POWI_N]
    out += [("round", v) for v in (0.5, -0.5, 2.5, -2.5, 1.5, 3.5, -3.5, HALF_DOWN, -HALF_DOWN, 4503599627370495.5)]
    out += [("fmod", x, y) for x in (5.5, -5.5, 1e300, SUB_MIN) for y in (INF, -INF, 0.0, -0.0, 3.0, SUB_MIN)]
    return out


def prescribed(probe) -> bool:
    """a special-table entry whose result is prescribed, not merely accurate: an exactly rounded control (sqrt, %, floor, ceil, round, min,
    max), a special argument (+-0, +-inf, NaN; a base of +-1 for pow), exp at its overflow and underflow thresholds, a result that overflows to
    +-inf or underflows to +-0, or a result that is exactly a double.  Other entries (sin(2.5), pow(3, 0.5)) are held to the accuracy bound
    instead"""
    op = probe[0]
    if op not in LIBM:
        return True
    args = [float(v) for v in probe[1:]]
    if op == "powi":
        args[1] = float(int(args[1]))
    if any(v != v or v in (0.0, INF, -INF) for v in args) or (op in ("pow", "powop", "powi") and abs(args[0]) == 1.0):
        return True
    if op == "exp" and args[0] in EXP_THRESHOLDS:
        return True
    try:
        ref = referee(probe)
    except ValueError:
        return True        # outside the domain (ln(-1), pow(-3, 2.5)): NaN
    if (ref >> 52) & 0x7FF == 0x7FF or ref & 0x7FFFFFFFFFFFFFFF == 0:
        return True        # overflow to +-inf, underflow to +-0
    return referee_is_exact(probe)


def referee_is_exact(probe) -> bool:
    """pow with an integer exponent whose exact result is a double, and ln(1)"""
    op, a = probe[0], probe[1]
    b = float(int(probe[2])) if op == "powi" else (probe[2] if len(probe) > 2 else 0.0)
    if op in ("pow", "powop", "powi"):
        if b != int(b) or abs(b) > 4096:
            return False
        try:
            q = Fraction(a) ** int(b)
            return Fraction(q.numerator / q.denominator) == q
        except (OverflowError, ZeroDivisionError):
            return False
    if op == "ln" and a == 1.0:
        return True
    return False


def exact_cases():
    """operations whose exact result is a double: they must come back exactly (pow(k, n) < 2^53, pow(2, n) over the whole exponent range, through
    pow(), `**` and `** n`; exp(0), ln(1), sin(+-0), cos(0), atan2 of signed zeros)"""
    out = []
    for k in range(256):
        n = 0
        while n <= 60 and k ** n < 2 ** 53:
            for op in ("pow", "powop", "powi"):
                out.append((op, float(k), float(n)))
            n += 1
            if k < 2:
                break
    for n in range(-1074, 1024):
        for op in ("pow", "powop", "powi"):
            out.append((op, 2.0, float(n)))
    out += [("exp", 0.0), ("exp", -0.0), ("ln", 1.0), ("sin", 0.0), ("sin", -0.0), ("cos", 0.0), ("cos", -0.0), ("tan", 0.0), ("tan", -0.0)]
    for z in (0.0, -0.0):
        for x in (SUB_MIN, 1.0, 3.0, DBL_MAX, -SUB_MIN, -1.0, -DBL_MAX):
            out.append(("atan2", z, x))
        for y in (SUB_MIN, 1.0, DBL_MAX, -SUB_MIN, -1.0, -DBL_MAX):
            out.append(("atan2", y, z))
    return out


def exact_value(probe) -> int:
    """the mathematically exact result of an exact_cases() probe"""
    op, a = probe[0], probe[1]
    if op in ("pow", "powop", "powi"):
        return f2b(float(Fraction(a) ** int(probe[2])))
    return glibc(probe)   # exp(0) = 1, ln(1) = 0, sin / tan(+-0) = +-0, cos(0) = 1, atan2 of zeros: C99 Annex F, which glibc follows


def sweeps(seed: int = 11):
    """{function: [probe]}: the ranges scripts use (byte values, [0, 1], angles) and the hard ones"""
    rng = np.random.default_rng(seed)
    u = lambda lo, hi, n: [float(v) for v in rng.uniform(lo, hi, n)]
    logu = lambda lo, hi, n: [float(v) for v in 10.0 ** rng.uniform(lo, hi, n)]
    byte = [float(v) for v in range(256)]
    out = {}
    halfpi = [float(k * np.pi / 2) for k in range(1, 65)]
    trig_hard = [v for h in halfpi for v in _neigh(h, 2)] + logu(0, 308, 150) + [-v for v in logu(0, 308, 50)]
    for f in ("sin", "cos", "tan"):
        args = byte + u(0, 1, 150) + u(-2 * np.pi, 2 * np.pi, 200) + trig_hard
        out[f] = [(f, a) for a in args]
    out["exp"] = [("exp", a) for a in byte[:120] + [-v for v in byte[1:120]] + u(0, 1, 150) + u(-745.2, 709.79, 300) + u(700, 709.78, 100)
                  + u(-745.13, -708.4, 150)]
    sub = [b2f(int(v)) for v in rng.integers(1, 1 << 52, 150)]
    out["ln"] = [("ln", a) for a in byte[1:] + u(0, 1, 150) + [v for k in range(1, 40) for v in (1 + k * 2.0 ** -52, 1 - k * 2.0 ** -53)]
                 + u(0.999, 1.001, 100) + sub + logu(-300, 308, 150)]
    pw = [("pow", b / 255.0, g) for b, g in zip(rng.integers(0, 256, 300), u(0.2, 4.0, 300))]
    pw += [("pow", b, e) for b, e in zip(byte, u(-3, 3, 256))]
    pw += [("pow", 1.0 + d, y) for d, y in zip(u(-1e-9, 1e-9, 150), logu(6, 11, 150))]
    for x, t in zip(u(0.05, 0.95, 150), u(-1074, -1022, 150)):
        pw.append(("pow", x, float(t * np.log(2) / np.log(x))))     # results in the subnormal range
    out["pow"] = pw
    at = []
    for sy in (1, -1):
        for sx in (1, -1):
            at += [("atan2", sy * y, sx * x) for y, x in zip(logu(-5, 5, 60), logu(-5, 5, 60))]
            at += [("atan2", sy * y, sx * x) for y, x in zip(logu(-300, -250, 15), logu(250, 300, 15))]
            at += [("atan2", sy * y, sx * x) for y, x in zip(logu(250, 300, 15), logu(-300, -250, 15))]
    out["atan2"] = at
    return out


def _neigh(v: float, k: int):
    """v and its k neighbours on either side"""
    out, lo, hi = [v], v, v
    for _ in range(k):
        lo, hi = float(np.nextafter(lo, -INF)), float(np.nextafter(hi, INF))
        out += [lo, hi]
    return out


def substituted(r, run):
    """run() evaluates closures on the host (-> (results, error)).  Trace its libm calls, have the device evaluate them, and run it again with
    the device's results substituted (new calls that the substituted values lead to are evaluated in turn).
    -> (plain run, substituted run or None without libm calls, table)"""
    with traced() as t:
        plain = run()
    calls, table = t.calls, {}
    if not calls:
        return plain, None, table
    for _ in range(4):
        table.update(device_table(r, [c for c in calls if c not in table]))
        with traced(table) as o:
            sub = run()
        if o.misses == 0:
            return plain, sub, table
        calls = o.calls
    raise AssertionError("the substituted run keeps reaching new libm calls")
