"""Seeded generator of per-pixel closures that the script VM compiles (pfx_rhai.cpp: Interp::compile_closure -> k_script.hip: vm_kernel).

A program is a closure for map_channels, for_each_pixel or for_region, plus the header lines in front of it (captured `let`s and
script `fn`s that the compiler inlines).  Types are static: every expression is built as i64, f64 or bool, and every i64 carries
a conservative interval of the values it can take, so that a program fails only where the generator plants a failure.

The same text runs twice: once on the device (`Program.device_script`) and once in the host interpreter, which is the reference
(`Program.host_closure`: the closure bound to `f` on the same lines, so error lines agree).  Per result element the generator
records whether the value depends on a libm routine (pow, sin, cos, tan, atan2, exp, ln): those may differ by one ulp between
the device's and the host's libm, and reach the result only through a clamped to_int, so by at most 1.  Everything else is
expected bit-exact.

The sign of a zero that comes out of min / max is unspecified on both sides: such a value is never used as a divisor or as an
argument of atan2 / pow / `**` (abs() is put around it first)."""
from __future__ import annotations

import random
import re
from dataclasses import dataclass, field

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
INT_EDGES = [0, 1, -1, 2 ** 31 - 1, 2 ** 31, 2 ** 32, I64_MIN, I64_MAX]
LIBM = ("pow", "sin", "cos", "tan", "atan2", "exp", "ln")
KINDS = ("map_channels", "for_each_pixel", "for_region")
# launch classes of the corpus: (lanes, lcode, heavy) — pfxk_vm_shape picks lanes from n_regs (<= 32: 256, 33-42: 192, 43-64: 128, 65-120: 64)
LANE_CLASSES = (256, 192, 128, 64)
# (low, high) register targets per class; a long program (LCODE = false) aims at the top of its class, where the register file leaves the
# least LDS for the staged code (at 32 registers and 256 lanes, or 64 and 128, none at all)
REG_TARGET = {(256, True): (16, 28), (192, True): (33, 37), (128, True): (43, 52), (64, True): (65, 84),
              (256, False): (30, 32), (192, False): (39, 42), (128, False): (60, 64), (64, False): (72, 86)}


def int_src(v: int) -> str:
    if v == I64_MIN:
        return "(-9223372036854775807 - 1)"
    return str(v) if v >= 0 else f"({v})"


def float_src(v: float) -> str:
    if v != v:
        return "(0.0 / 0.0)"
    if v in (float("inf"), float("-inf")):
        return "(1.0 / 0.0)" if v > 0 else "(-1.0 / 0.0)"
    s = repr(v)
    if "e" not in s and "." not in s:
        s += ".0"
    if "e" in s and "." not in s.split("e")[0]:
        m, e = s.split("e")
        s = m + ".0e" + e
    return s if v >= 0 and not s.startswith("-") else f"({s})"


@dataclass
class E:
    src: str
    t: str                  # "i", "f", "b"
    lo: int = I64_MIN
    hi: int = I64_MAX
    libm: bool = False      # value depends on a libm routine
    mm: bool = False        # f64 that may be a zero whose sign min / max decided


_NUM = re.compile(r"(?<![\w.])\d+(\.\d+)?(e[+-]?\d+)?")
_OPS = re.compile(r"\*\*|<<|>>|==|!=|<=|>=|&&|\|\||[-+*/%^&|<>!]")
_CALL = re.compile(r"\b(\w+)\(")
_CALL_REGS = {"get_pixel": 4, "distance": 5, "mixf": 16, "halff": 6}


def reg_cost(src: str) -> int:
    """an upper estimate of the registers the compiler allocates for an expression (one per literal, operator and call; none per variable read)"""
    n = len(_NUM.findall(src)) + len(_OPS.findall(src)) + src.count("if ") + len(re.findall(r"\b(true|false)\b", src))
    n += sum(_CALL_REGS.get(m, 1) for m in _CALL.findall(src))
    return 2 * n + 1


def fits(lo: int, hi: int) -> bool:
    return I64_MIN <= lo and hi <= I64_MAX


def bits_iv(a: E, b: E):
    k = max(abs(a.lo), abs(a.hi), abs(b.lo), abs(b.hi)).bit_length()
    if a.lo >= 0 and b.lo >= 0:
        return 0, (1 << k) - 1
    return max(-(1 << k), I64_MIN), min((1 << k) - 1, I64_MAX)


@dataclass
class Program:
    seed: int
    kind: str
    header: list[str]
    body: list[str]              # the closure's lines; body[0] starts with the parameter list
    fn_name: str | None          # Fn("name") form: the closure is a script fn in the header
    params: tuple
    region: tuple | None         # for_region(x, y, w, h)
    width: int
    height: int
    libm: list[bool]             # per result element: depends on a libm routine
    constructs: dict = field(default_factory=dict)   # construct -> first line it appears on
    errors: list = field(default_factory=list)       # (line, message) of planted failures
    mask: bool = True

    def _closure_text(self) -> str:
        return "\n".join(self.body)

    def device_script(self, region=None) -> str:
        clos = f'Fn("{self.fn_name}")' if self.fn_name else self._closure_text()
        head = "\n".join(self.header)
        if self.kind == "for_region":
            rx, ry, rw, rh = region if region is not None else self.region
            call = f"for_region({rx}, {ry}, {rw}, {rh}, {clos});"
        else:
            call = f"{self.kind}({clos});"
        return head + "\n" + call if head else call

    def host_closure(self) -> str:
        """`let f = <closure>;` with the closure on the lines it has in device_script()"""
        clos = f'Fn("{self.fn_name}")' if self.fn_name else self._closure_text()
        head = "\n".join(self.header)
        s = f"let f = {clos};"
        return head + "\n" + s if head else s


class Gen:
    def __init__(self, seed: int, knobs: dict):
        self.rng = random.Random(seed)
        self.k = knobs
        self.lines: list[str] = []
        self.header: list[str] = []
        self.scopes: list[dict] = [{}]
        self.constructs: dict = {}
        self.errors: list = []
        self.counter = 0
        self.lit_pool: list[int] = []
        self.w = knobs["w"]
        self.h = knobs["h"]
        self.live = 6          # registers the compiler holds at this point (parameters, lets and their initialisers' temporaries)
        self.reg_cap = 110     # no statement may need more
        self.lives: list[int] = []

    def budgeted(self, gen, fallback):
        for _ in range(8):
            e = gen()
            if reg_cost(e.src) + self.live <= self.reg_cap:
                return e
        return fallback

    def push(self):
        self.scopes.append({})
        self.lives.append(self.live)

    def pop(self):
        self.scopes.pop()
        self.live = self.lives.pop()

    # ---------------------------------------------------------------- bookkeeping
    def note(self, what: str):
        self.constructs.setdefault(what, len(self.header) + len(self.lines) + 1)

    def fresh(self, p="v"):
        self.counter += 1
        return f"{p}{self.counter}"

    def vars(self, t, libm_ok=False):
        out = {}
        for s in self.scopes:
            for n, e in s.items():
                out[n] = e
        return [(n, e) for n, e in out.items() if e.t == t and (libm_ok or not e.libm)]

    def bind(self, name, e: E):
        self.scopes[-1][name] = E(name, e.t, e.lo, e.hi, e.libm, e.mm)

    def lit(self) -> int:
        if self.lit_pool and self.rng.random() < 0.6:
            return self.rng.choice(self.lit_pool)
        return self.rng.randint(2, 97)

    # ---------------------------------------------------------------- int expressions
    def int_leaf(self) -> E:
        r = self.rng.random()
        vs = self.vars("i")
        if r < 0.45 and vs:
            n, e = self.rng.choice(vs)
            return E(n, "i", e.lo, e.hi)
        if r < 0.6:
            v = self.rng.choice(INT_EDGES) if self.rng.random() < 0.5 else self.lit()
            self.note("int_edge" if v in INT_EDGES else "int_literal")
            return E(int_src(v), "i", v, v)
        if r < 0.7:
            f = self.rng.choice(["width", "height"])
            self.note(f)
            v = self.w if f == "width" else self.h
            return E(f"{f}()", "i", v, v)
        if r < 0.82 and self.k["xy"]:
            return self.pixel_read()
        n, e = self.rng.choice(self.params_iv())
        return E(n, "i", e[0], e[1])

    def params_iv(self):
        p = [("r", (0, 255)), ("g", (0, 255)), ("b", (0, 255)), ("a", (0, 255))]
        if self.k["xy"]:
            p += [("x", (0, self.w - 1)), ("y", (0, self.h - 1))]
        return p

    def coord(self, axis):
        c = self.rng.choice(["x", "y"]) if self.rng.random() < 0.2 else axis
        off = self.rng.choice([0, 0, 1, -1, -3, 5, 70, -70])
        if off == 0:
            return c
        return f"{c} + {off}" if off > 0 else f"{c} - {-off}"

    def pixel_read(self) -> E:
        f = self.rng.choice(["get_r", "get_g", "get_b", "get_a", "get_pixel"])
        self.note(f)
        if f == "get_pixel":
            k = self.rng.randint(0, 3)
            return E(f"get_pixel({self.coord('x')}, {self.coord('y')})[{k}]", "i", 0, 255)
        return E(f"{f}({self.coord('x')}, {self.coord('y')})", "i", 0, 255)

    def small(self, d) -> E:
        """an int expression known to lie within +-2^40"""
        e = self.int_expr(d)
        if e.lo < -(1 << 40) or e.hi > (1 << 40):
            self.note("&")
            return E(f"({e.src} & 1048575)", "i", 0, 1048575)
        return e

    def divisor(self, d) -> E:
        e = self.small(d)
        c = self.rng.randint(0, 2)
        if c == 0:
            self.note("|")
            return E(f"(({e.src} & 1023) | 1)", "i", 1, 1023) if e.lo < 0 else E(f"({e.src} | 1)", "i", 1, max(1, e.hi | 1))
        if c == 1:
            return E(f"({e.src} % 16 - 17)", "i", -32, -2)          # negative on every pixel
        return E(f"({e.src} % 9 + 10)", "i", 2, 18)

    def int_expr(self, d=0) -> E:
        if d == 0:
            return self.budgeted(lambda: self._int_expr(0), E("r", "i", 0, 255))
        return self._int_expr(d)

    def _int_expr(self, d=0) -> E:
        if d >= self.k["depth"] or self.rng.random() < 0.25:
            return self.int_leaf()
        r = self.rng.random()
        if r < 0.42:
            op = self.rng.choice(["+", "-", "*", "/", "%", "**", "&", "|", "^", "<<", ">>"])
            return self.int_binary(op, d)
        if r < 0.55:
            a = self.int_expr(d + 1)
            f = self.rng.choice(["abs", "sign", "neg", "min", "max", "min_i", "max_i", "clamp", "abs_i"])
            self.note(f)
            if f in ("abs", "abs_i"):
                return E(f"{f}({a.src})", "i", *( (0, max(abs(a.lo), abs(a.hi))) if a.lo > I64_MIN else (I64_MIN, I64_MAX)))
            if f == "sign":
                return E(f"sign({a.src})", "i", -1, 1)
            if f == "neg":
                if a.lo == I64_MIN:
                    return a
                return E(f"-({a.src})", "i", -a.hi, -a.lo)
            if f == "clamp":
                lo = self.rng.randint(-300, 100)
                hi = lo + self.rng.randint(0, 400)
                return E(f"clamp({a.src}, {int_src(lo)}, {int_src(hi)})", "i", lo, hi)
            b = self.int_expr(d + 1)
            if f.startswith("min"):
                return E(f"{f}({a.src}, {b.src})", "i", min(a.lo, b.lo), min(a.hi, b.hi))
            return E(f"{f}({a.src}, {b.src})", "i", max(a.lo, b.lo), max(a.hi, b.hi))
        if r < 0.68:
            self.note("to_int")
            return self.f2i(self.float_expr(d + 1))
        if r < 0.76 and self.k["branches"]:
            c = self.bool_expr(d + 1)
            a, b = self.int_expr(d + 1), self.int_expr(d + 1)
            self.note("if_expr")
            return E(f"(if {c.src} {{ {a.src} }} else {{ {b.src} }})", "i", min(a.lo, b.lo), max(a.hi, b.hi))
        if r < 0.84 and self.k["fns"]:
            a, b = self.int_expr(d + 1), self.int_expr(d + 1)
            self.note("fn_inline")
            return E(f"mixf({a.src}, {b.src})", "i", 0, 250)
        return self.int_leaf()

    def f2i(self, f: E) -> E:
        """NaN-safe, range-safe to_int (min / max of a NaN give the other operand): differs by at most 1 when f's last bit does"""
        self.note("to_int")
        return E(f"to_int(max(min({f.src}, 1000000.0), -1000000.0))", "i", -1000000, 1000000, f.libm)

    def int_binary(self, op, d) -> E:
        self.note(op)
        if op in ("/", "%"):
            a = self.int_expr(d + 1)
            b = self.divisor(d + 1)
            if a.lo == I64_MIN and b.lo <= -1 <= b.hi:
                a = self.small(d + 1)
            m = max(abs(a.lo), abs(a.hi))
            if op == "/":
                return E(f"({a.src} / {b.src})", "i", -m, m)
            bm = max(abs(b.lo), abs(b.hi)) - 1
            return E(f"({a.src} % {b.src})", "i", -min(m, bm) if a.lo < 0 else 0, min(m, bm) if a.hi > 0 else 0)
        if op == "**":
            if self.rng.random() < 0.4:
                base = self.rng.choice([0, 1, -1])
                e = self.rng.randint(0, 64)
                self.note("pow_edge")
                v = base ** e
                return E(f"({int_src(base)} ** {e})", "i", v, v)
            a = self.small(d + 1)
            a = E(f"({a.src} % 11)", "i", -10 if a.lo < 0 else 0, 10 if a.hi > 0 else 0)
            e = self.rng.randint(0, 18)
            m = 10 ** e
            return E(f"({a.src} ** {e})", "i", -m if a.lo < 0 else 0, m)
        if op in ("<<", ">>"):
            a = self.int_expr(d + 1)
            n = self.rng.randint(-70, 70)
            self.note("shift_edge" if abs(n) >= 63 else "shift")
            if op == ">>" and n >= 0:
                return E(f"({a.src} >> {int_src(n)})", "i", a.lo >> min(n, 63), a.hi >> min(n, 63))
            return E(f"({a.src} {op} {int_src(n)})", "i")
        a, b = self.int_expr(d + 1), self.int_expr(d + 1)
        if op in ("&", "|", "^"):
            return E(f"({a.src} {op} {b.src})", "i", *bits_iv(a, b))
        if op == "+":
            lo, hi = a.lo + b.lo, a.hi + b.hi
        elif op == "-":
            lo, hi = a.lo - b.hi, a.hi - b.lo
        else:
            c = [a.lo * b.lo, a.lo * b.hi, a.hi * b.lo, a.hi * b.hi]
            lo, hi = min(c), max(c)
        if not fits(lo, hi):   # would overflow on some pixel: keep the operator, narrow the operands
            a, b = self.small(d + 1), self.small(d + 1)
            a = E(f"({a.src} % 1000)", "i", -999 if a.lo < 0 else 0, 999 if a.hi > 0 else 0)
            b = E(f"({b.src} % 1000)", "i", -999 if b.lo < 0 else 0, 999 if b.hi > 0 else 0)
            return self.combine(op, a, b)
        return E(f"({a.src} {op} {b.src})", "i", lo, hi)

    def combine(self, op, a, b):
        if op == "+":
            return E(f"({a.src} + {b.src})", "i", a.lo + b.lo, a.hi + b.hi)
        if op == "-":
            return E(f"({a.src} - {b.src})", "i", a.lo - b.hi, a.hi - b.lo)
        c = [a.lo * b.lo, a.lo * b.hi, a.hi * b.lo, a.hi * b.hi]
        return E(f"({a.src} * {b.src})", "i", min(c), max(c))

    # ---------------------------------------------------------------- float expressions
    FLOAT_EDGES = [0.0, -0.0, 0.5, -0.5, 2.5, -2.5, 1.5, 1e300, -1e300, float("inf"), float("-inf"), float("nan"),
                   9.223372036854775e18, -9.223372036854775e18, 0.1, 3.0]

    def float_leaf(self, libm_ok) -> E:
        r = self.rng.random()
        vs = self.vars("f", libm_ok)
        if r < 0.35 and vs:
            n, e = self.rng.choice(vs)
            return E(n, "f", libm=e.libm, mm=e.mm)
        if r < 0.6:
            v = self.rng.choice(self.FLOAT_EDGES)
            self.note("float_edge")
            return E(float_src(v), "f")
        if r < 0.7:
            self.note("PI")
            return E("PI()", "f")
        if r < 0.85:
            i = self.int_expr(self.k["depth"] - 1)
            self.note("to_float")
            return E(f"to_float({i.src})", "f")
        i = self.int_expr(self.k["depth"] - 1)
        self.note("mixed_promotion")
        return E(f"({i.src} * {float_src(self.rng.choice([0.5, 0.25, 1.5, -0.75]))})", "f")

    def nz(self, e: E) -> E:
        """e with a zero of defined sign (abs), for divisors and libm arguments"""
        return E(f"abs({e.src})", "f", libm=e.libm) if e.mm else e

    def float_expr(self, d=0, libm_ok=False) -> E:
        if d == 0:
            return self.budgeted(lambda: self._float_expr(0, libm_ok), E("to_float(g)", "f"))
        return self._float_expr(d, libm_ok)

    def _float_expr(self, d=0, libm_ok=False) -> E:
        if d >= self.k["depth"] or self.rng.random() < 0.3:
            return self.float_leaf(libm_ok)
        r = self.rng.random()
        if r < 0.35:
            op = self.rng.choice(["+", "-", "*", "/", "%"])
            self.note("f" + op)
            a, b = self.float_expr(d + 1, libm_ok), self.float_expr(d + 1, libm_ok)
            if op in ("/", "%"):
                b = self.nz(b)
            return E(f"({a.src} {op} {b.src})", "f", libm=a.libm or b.libm, mm=a.mm or b.mm)
        if r < 0.55:
            a = self.float_expr(d + 1, libm_ok)
            f = self.rng.choice(["floor", "ceil", "round", "sqrt", "abs", "neg"])
            self.note(f)
            if f == "neg":
                return E(f"-({a.src})", "f", libm=a.libm, mm=a.mm)
            return E(f"{f}({a.src})", "f", libm=a.libm, mm=a.mm and f != "abs")
        if r < 0.72:
            f = self.rng.choice(["min", "max", "min_f", "max_f", "clamp_f", "lerp", "distance"])
            self.note(f)
            if f == "clamp_f":
                a = self.float_expr(d + 1, libm_ok)
                lo = self.rng.choice([-1.5, 0.0, 0.25, 10.0])
                hi = lo + self.rng.choice([0.0, 0.5, 100.0])
                return E(f"clamp_f({a.src}, {float_src(lo)}, {float_src(hi)})", "f", libm=a.libm, mm=a.mm)
            n = {"lerp": 3, "distance": 4}.get(f, 2)
            args = [self.float_expr(d + 1, libm_ok) for _ in range(n)]
            return E(f"{f}({', '.join(x.src for x in args)})", "f", libm=any(x.libm for x in args),
                     mm=f.startswith(("min", "max")) or any(x.mm for x in args))
        if r < 0.85 and libm_ok and self.k["heavy"]:
            f = self.rng.choice(["sin", "cos", "tan", "exp", "ln", "pow", "atan2", "**"])
            self.note(f)
            if f in ("pow", "atan2"):
                a, b = self.nz(self.float_expr(d + 1, False)), self.nz(self.float_expr(d + 1, False))
                return E(f"{f}({a.src}, {b.src})", "f", libm=True)
            if f == "**":
                a, b = self.nz(self.float_expr(d + 1, False)), self.nz(self.float_expr(d + 1, False))
                return E(f"({a.src} ** {b.src})", "f", libm=True)
            a = self.float_expr(d + 1, False)
            return E(f"{f}({a.src})", "f", libm=True)
        if r < 0.92 and self.k["fns"]:
            a = self.float_expr(d + 1, libm_ok)
            self.note("fn_inline")
            return E(f"halff({a.src})", "f", libm=a.libm, mm=a.mm)
        return self.float_leaf(libm_ok)

    # ---------------------------------------------------------------- bools
    def bool_expr(self, d=0) -> E:
        if d == 0:
            return self.budgeted(lambda: self._bool_expr(0), E("(b < a)", "b"))
        return self._bool_expr(d)

    def _bool_expr(self, d=0) -> E:
        r = self.rng.random()
        if d >= self.k["depth"] or r < 0.45:
            a, b = self.int_expr(d + 1), self.int_expr(d + 1)
            op = self.rng.choice(["==", "!=", "<", "<=", ">", ">="])
            self.note("cmp" + op)
            return E(f"({a.src} {op} {b.src})", "b")
        if r < 0.6:
            a, b = self.float_expr(d + 1), self.float_expr(d + 1)
            op = self.rng.choice(["==", "!=", "<", "<=", ">", ">="])
            self.note("fcmp")
            return E(f"({a.src} {op} {b.src})", "b")
        if r < 0.75:
            a, b = self.bool_expr(d + 1), self.bool_expr(d + 1)
            op = self.rng.choice(["&&", "||", "&", "|", "^", "=="] if self.k["branches"] else ["&", "|", "^", "=="])
            self.note("bool" + op)
            return E(f"({a.src} {op} {b.src})", "b")
        if r < 0.83:
            a = self.bool_expr(d + 1)
            self.note("!")
            return E(f"!{a.src}", "b")
        if r < 0.9 and self.k["xy"]:
            self.note("is_selected")
            return E(f"is_selected({self.coord('x')}, {self.coord('y')})", "b")
        vs = self.vars("b")
        if vs:
            return E(self.rng.choice(vs)[0], "b")
        return E(self.rng.choice(["true", "false"]), "b")

    def any_expr(self, t, libm_ok=False):
        return self.int_expr() if t == "i" else self.float_expr(0, libm_ok) if t == "f" else self.bool_expr()

    # ---------------------------------------------------------------- statements
    def emit(self, s, ind=1):
        self.lines.append("    " * ind + s)

    def acc_update(self, name, ind):
        """name = f(name, small): keeps name within +-16383"""
        e = self.budgeted(lambda: self.small(1), E("g", "i", 0, 255))
        form = self.rng.randint(0, 2)
        if form == 0:
            self.note("+=")
            self.emit(f"{name} += {e.src} % 7;", ind)
            self.emit(f"{name} = {name} % 9973;", ind)
        elif form == 1:
            self.note("^=")
            self.emit(f"{name} ^= {e.src} & 4095;", ind)
        else:
            self.emit(f"{name} = ({name} * 3 + {e.src} % 97) % 9973;", ind)

    def trip(self):
        """a pixel-dependent loop trip count in 0..9"""
        p = self.rng.choice(["r", "g", "b", "a"] + (["x", "y"] if self.k["xy"] else []))
        return f"({p} % {self.rng.randint(3, 10)})"

    def stmt_block(self, n, ind=1):
        for _ in range(n):
            c = self.rng.random()
            if c < 0.3 or ind > 2:
                self.let_stmt(ind)
            elif c < 0.45 and self.k["branches"]:
                self.if_stmt(ind)
            elif c < 0.75 and self.k["branches"] and ind == 1:
                self.loop_stmt(ind)
            else:
                vs = [n for n, e in self.vars("i") if n.startswith("acc")]
                if vs:
                    self.acc_update(self.rng.choice(vs), ind)
                else:
                    self.let_stmt(ind)

    def let_stmt(self, ind):
        t = self.rng.choice(["i", "i", "f", "b"])
        e = self.any_expr(t)
        vs = self.vars(t)
        if vs and self.rng.random() < 0.25:
            name = self.rng.choice(vs)[0]
            self.note("shadowing")
        else:
            name = self.fresh({"i": "n", "f": "u", "b": "q"}[t])
        self.note("let")
        self.emit(f"let {name} = {e.src};", ind)
        self.bind(name, e)
        self.live += reg_cost(e.src) + 1

    def if_stmt(self, ind):
        accs = [n for n, e in self.vars("i") if n.startswith("acc")]
        if not accs:
            name = self.fresh("acc")
            self.emit(f"let {name} = {self.rng.randint(0, 50)};", ind)
            self.live += 2
            self.bind(name, E(name, "i", -16383, 16383))
            accs = [name]
        self.note("if")
        self.emit(f"if {self.bool_expr().src} {{", ind)
        self.acc_update(self.rng.choice(accs), ind + 1)
        if self.rng.random() < 0.5:
            self.note("else_if")
            self.emit(f"}} else if {self.bool_expr().src} {{", ind)
            self.acc_update(self.rng.choice(accs), ind + 1)
        if self.rng.random() < 0.6:
            self.emit("} else {", ind)
            self.acc_update(self.rng.choice(accs), ind + 1)
        self.emit("}", ind)

    def loop_stmt(self, ind):
        acc = self.fresh("acc")
        self.emit(f"let {acc} = {self.rng.randint(0, 9)};", ind)
        self.live += 4
        self.bind(acc, E(acc, "i", -16383, 16383))
        form = self.rng.choice(["while", "loop", "for", "for_incl", "range_neg", "range_pos"])
        self.note(form)
        i = self.fresh("i")
        if form == "while":
            self.emit(f"let {i} = 0;", ind)
            self.emit(f"while {i} < {self.trip()} {{", ind)
            self.emit(f"{i} += 1;", ind + 1)
        elif form == "loop":
            self.emit(f"let {i} = 0;", ind)
            self.emit("loop {", ind)
            self.emit(f"{i} += 1;", ind + 1)
            self.note("break")
            self.emit(f"if {i} > {self.trip()} {{ break; }}", ind + 1)
        elif form == "for":
            self.emit(f"for {i} in 0..{self.trip()} {{", ind)
        elif form == "for_incl":
            self.emit(f"for {i} in {self.rng.randint(-3, 2)}..={self.trip()} {{", ind)
        elif form == "range_neg":
            self.emit(f"for {i} in range({self.trip()}, {self.rng.randint(-4, 0)}, {-self.rng.randint(1, 3)}) {{", ind)
        else:
            self.emit(f"for {i} in range(0, {self.trip()}, {self.rng.randint(1, 3)}) {{", ind)
        self.push()
        self.live += 6
        self.bind(i, E(i, "i", -10, 10))
        if self.rng.random() < 0.4:
            self.note("continue")
            self.emit(f"if ({i} & 1) == 0 {{ continue; }}", ind + 1)
        self.acc_update(acc, ind + 1)
        self.stmt_block(self.rng.randint(0, 1), ind + 1)
        if form not in ("loop",) and self.rng.random() < 0.3:
            self.note("break")
            self.emit(f"if {acc} > {self.rng.randint(100, 5000)} {{ break; }}", ind + 1)
        self.pop()
        self.emit("}", ind)


# The failing operations planted in error mode: (message, statement template).  {p} is a parameter holding 0..255; each fails on the pixels
# where the guarded value hits the bad case, and only there.
FAILURES = [
    ("Division by zero", "let e{n} = 1000 / ({p} % 5 - 2);"),
    ("Modulo division by zero", "let e{n} = 1000 % ({p} % 7 - 3);"),
    ("Addition overflow", "let e{n} = 9223372036854775807 + ({p} & 1);"),
    ("Subtraction overflow", "let e{n} = (-9223372036854775807 - 1) - ({p} & 1);"),
    ("Multiplication overflow", "let e{n} = 4611686018427387904 * (({p} & 1) + 1);"),
    ("Negation overflow", "let e{n} = -((-9223372036854775807 - 1) + ({p} & 1));"),
    ("Exponential overflow", "let e{n} = 2 ** (58 + ({p} & 7));"),
    ("Integer raised to a negative power", "let e{n} = 3 ** (({p} & 3) - 2);"),
    ("Integer overflow: to_int", "let e{n} = to_int(9.223372036854777e18 * to_float({p} & 1));"),
    ("Modulo division overflow", "let e{n} = (-9223372036854775807 - 1) % (({p} & 1) - 2);"),
    ("Division overflow", "let e{n} = (-9223372036854775807 - 1) / (({p} & 1) - 2);"),
    ("clamp: min > max", "let e{n} = clamp(7, {p}, 128);"),
]


def knobs_for(seed: int) -> dict:
    """the shape knobs of corpus program `seed`: seeds walk the 16 launch classes (lanes x lcode x heavy) in turn"""
    rng = random.Random(seed * 7919 + 1)
    cls = seed % 16
    lanes = LANE_CLASSES[cls % 4]
    lcode = (cls // 4) % 2 == 0
    heavy = cls // 8 == 1
    kind = KINDS[(seed // 16) % 3]
    return dict(
        seed=seed, lanes=lanes, lcode=lcode, heavy=heavy, kind=kind,
        w=rng.randint(1, 64), h=rng.randint(1, 48),
        depth=rng.randint(2, 3),
        xy=kind != "map_channels",
        branches=seed % 5 != 4,                           # every fifth program is straight-line: its constants are hoisted
        n_literals=[0, 3, 12, 40, 130][(seed // 5) % 5],   # distinct literals (past the 120-register hoisting cap at the top)
        fns=rng.random() < 0.5 and seed % 5 != 4,
        fn_form=rng.random() < 0.08,
        errors=rng.random() < 0.25,
        result=rng.choice(["ints"] * 6 + ["mixed", "long", "short", "unit"]),
    )


def generate(seed: int, knobs: dict | None = None) -> Program:
    k = dict(knobs_for(seed), **(knobs or {}))
    g = Gen(seed, k)
    rng = g.rng
    params = ("x", "y", "r", "g", "b", "a") if k["xy"] else ("r", "g", "b", "a")
    # header: captured outer lets and inlined script fns
    if k["fns"]:
        g.header.append("fn mixf(p, q) { let s = (p & 1023) * 3 + (q & 1023); if s > 2000 { return s % 251; } s % 250 }")
        g.header.append("fn halff(v) { v * 0.5 + 1.0 }")
    g.lit_pool = [1000 + 7 * j for j in range(k["n_literals"])]
    fn_name = None
    ca0 = 17
    if k["fn_form"]:     # a script fn sees no outer variables
        fn_name = "shade"
        g.lines.append(f"fn shade({', '.join(params)}) {{")
        g.note("Fn_name")
        g.emit("let k0 = 17;")
    else:
        cap_i, cap_f = rng.randint(-50, 300), rng.choice([0.25, -1.5, 2.5])
        ca0 = rng.randint(0, 255)
        g.header.append(f"let ci = {int_src(cap_i)};")
        g.header.append(f"let cf = {float_src(cap_f)};")
        g.header.append("let cb = " + rng.choice(["true", "false"]) + ";")
        g.header.append(f"let ca = [{ca0}, 0.5, true, {int_src(rng.choice(INT_EDGES))}];")
        g.scopes[0].update({"ci": E("ci", "i", cap_i, cap_i), "cf": E("cf", "f"), "cb": E("cb", "b")})
        g.lines.append(f"|{', '.join(params)}| {{")
        g.note("captured")
        g.emit("let k0 = ca[0] + ci;")
        g.emit("let kf = ca[1] + cf;")
        g.bind("kf", E("kf", "f"))
    g.bind("k0", E("k0", "i", -50, 555))
    chans = ("r", "g", "b", "a")
    # registers: live lets pad the register file to the class's target (measured by the probe: the coverage test holds the corpus to it)
    lo_t, hi_t = REG_TARGET[(k["lanes"], k["lcode"])]
    g.live = len(params) + (4 if k["fn_form"] else 12)    # captured values, k0 / kf, and the 4 registers of the result array
    g.reg_cap = min(hi_t - 1, 104)
    n_pad = max(0, (lo_t - g.live) // 3)      # a pad holds 3 registers: the literal, the xor and the variable
    if not k["branches"]:                      # hoisting adds a register per distinct literal
        n_pad = max(0, (lo_t - g.live - min(k["n_literals"], 60)) // 3)
        g.reg_cap = 118 - min(k["n_literals"], 100)
    pads = []
    for j in range(n_pad):
        name = f"p{j}"
        src = f"{chans[j % 4]} ^ {g.lit() if g.lit_pool else j + 3}"
        g.emit(f"let {name} = {src};")
        g.bind(name, E(name, "i", 0, 4095))
        g.live += 3
        pads.append(name)
    compact = k["lanes"] == 256                 # 32 registers at most: little besides the parameters and captured values
    if k["branches"]:
        g.stmt_block({256: 1, 192: 2, 128: 3, 64: 4}[k["lanes"]])
        if not k["lcode"]:   # a long program: the staged code does not fit next to the registers
            g.emit("let accf = 0;")
            g.bind("accf", E("accf", "i", -16383, 16383))
            g.live += 2
            for _ in range(rng.randint(100, 140) * (3 if k["lanes"] == 64 else 1)):
                g.acc_update("accf", 1)
    else:
        for j in range(k["n_literals"]):   # one statement per literal: `sN ^= lit` keeps no register once hoisted
            if j == 0:
                g.emit("let s0 = r;")
                g.bind("s0", E("s0", "i", 0, 4095))
            g.emit(f"s0 ^= {1000 + 7 * j};")
        reps = 0 if k["lcode"] else (220 if k["lanes"] == 256 else 60)
        if reps and not k["n_literals"]:
            g.emit("let s0 = r;")
            g.bind("s0", E("s0", "i", 0, 4095))
        for j in range(reps):
            g.emit(f"s0 ^= {chans[j % 4]} & {1000 + 7 * (j % max(1, k['n_literals']))};")
    if k["errors"] and not compact:
        ps = [p for p in ("r", "g", "b", "a")]
        for kind_ix in rng.sample(range(len(FAILURES)), 2):
            msg, tmpl = FAILURES[kind_ix]
            p = rng.choice(ps)
            g.note("error:" + msg)
            if k["branches"]:
                guard = g.bool_expr(1) if rng.random() < 0.5 else E("true", "b")
                g.emit(f"if {guard.src} {{")
                line = len(g.header) + len(g.lines) + 1
                g.emit(tmpl.format(n=g.counter, p=p), 2)
                g.emit("}")
            else:
                line = len(g.header) + len(g.lines) + 1
                g.emit(tmpl.format(n=g.counter, p=p))
            g.counter += 1
            g.errors.append((line, msg))
    if k["heavy"]:
        # at least one libm routine in the program (its value may or may not reach the result)
        fn = LIBM[(seed // 16) % len(LIBM)]
        arg = "to_float(r)" if compact or k["fn_form"] or g.live + 16 > g.reg_cap else "distance(to_float(g), 0.5, to_float(b), kf)"
        if compact:
            f = E(f"{fn}({arg}, 2.0)" if fn in ("pow", "atan2") else f"{fn}({arg})", "f", libm=True)
        elif rng.random() < 0.5:
            g.note("distance")
            f = E(f"{fn}({arg}, 2.0)" if fn in ("pow", "atan2") else f"{fn}({arg})", "f", libm=True)
        else:
            f = g.float_expr(0, True)
        g.note(fn)
        if not f.libm:
            f = E(f"sin({f.src})", "f", libm=True)
            g.note("sin")
        g.emit(f"let h0 = {f.src};")
        g.bind("h0", f)
        g.live += reg_cost(f.src) + 1
    if rng.random() < 0.3 and k["branches"] and not compact:
        g.note("return")
        cap = g.reg_cap
        g.reg_cap = g.live + (cap - g.live) // 3
        c, e1, e2 = g.bool_expr(), g.int_expr(), g.int_expr()
        g.reg_cap = cap
        g.emit(f"if {c.src} {{ return [{e1.src}, {e2.src}, 17, {'ca[0]' if not k['fn_form'] else ca0}]; }}")
    # the result
    elems, libm, types = [], [], []
    n = {"ints": 4, "mixed": 4, "long": rng.randint(5, 6), "short": rng.randint(0, 3), "unit": 0}[k["result"]]
    cap, live0 = g.reg_cap - 24, g.live   # margin: the estimate of what is live here is the loosest
    g.reg_cap = g.live + max(4, (cap - g.live) // max(n, 1))   # the elements' temporaries are live together
    for j in range(n):
        t = "i"
        if k["result"] in ("mixed", "long") and rng.random() < 0.4:
            t = rng.choice(["f", "b"])
        if t == "i":
            if k["heavy"] and rng.random() < 0.5:
                g.reg_cap -= 8    # what f2i adds around the float
                e = g.f2i(g.float_expr(0, True))
                g.reg_cap += 8
                if rng.random() < 0.5:
                    e = E(f"{e.src} + {chans[j % 4]}", "i", libm=e.libm)
            else:
                e = g.int_expr()
            if j < len(pads) and rng.random() < 0.5 and not e.libm:
                e = E(f"({e.src} ^ {pads[j]})", "i")
        else:
            e = g.any_expr(t, True)
        elems.append(e.src)
        libm.append(e.libm)
        types.append(e.t)
        g.live += reg_cost(e.src)
        g.reg_cap = g.live + max(4, (cap - g.live) // max(n - j - 1, 1))
    g.reg_cap, g.live = cap + 24, live0
    if len(pads) > 4:   # the pads stay live up to here: one statement each (a single expression would need a register per operator)
        g.emit("let pz = 0;")
        for name in pads[4:]:
            g.emit(f"pz ^= {name};")
        if elems and not libm[0] and types[0] == "i":
            elems[0] = f"({elems[0]} ^ pz)"
    if k["result"] == "unit":
        g.note("unit_result")
        g.emit(f"let last = {g.int_expr().src};")
    else:
        g.note("result_" + k["result"])
        g.emit("[" + ", ".join(elems) + "]")
    g.lines.append("}" if k["fn_form"] else "}")
    if k["fn_form"]:
        body_start = len(g.header)
        g.header.extend(g.lines)
        g.lines = []
    region = None
    if k["kind"] == "for_region":
        rr = random.Random(seed + 99)
        c = rr.randint(0, 3)
        if c == 0:
            region = (rr.randint(0, k["w"] - 1), rr.randint(0, k["h"] - 1), rr.randint(1, k["w"]), rr.randint(1, k["h"]))
        elif c == 1:
            region = (rr.randint(-20, -1), rr.randint(-20, -1), rr.randint(10, 100), rr.randint(10, 100))   # clipped on the low side
        elif c == 2:
            region = (rr.randint(0, 5), rr.randint(0, 5), 0 if rr.random() < 0.5 else 1000, 0)              # empty
        else:
            region = (rr.randint(1, k["w"]), rr.randint(1, k["h"]), 1000, 1000)                              # offset, clipped on the high side
    body = g.lines
    return Program(seed=seed, kind=k["kind"], header=g.header, body=body, fn_name=fn_name, params=params, region=region, width=k["w"],
                   height=k["h"], libm=libm if k["result"] not in ("unit", "short") else [], constructs=g.constructs, errors=g.errors)


CORPUS_SEEDS = list(range(320))
