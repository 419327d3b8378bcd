"""Short forms of Vivid Light (k_blend.h: vivid_light_channel), Pin Light and Overlay (exact as well; measured on the device and not adopted)
against the reference's own expressions (canvas_state.rs:1425-1505), in an f32 model on the host, for all 65 536 (base byte, top byte) pairs.

Operands are RN(k / 255), what div255 and the typed load deliver.  Every reference operation is one numpy f32 operation (one rounding, IEEE division).
An FMA of the device is one rounding of the exact a * b + c: the product of two f32 is exact in f64, and the f64 sum is checked to be exact as well
(TwoSum's error term is zero for every operand the forms meet), so that rounding it to f32 is the FMA's single rounding.  Comparisons are on the
uint32 view: -0.0 against +0.0, or a NaN, would show."""
import numpy as np

F = np.float32


def _operands():
    k = np.arange(256, dtype=F) / F(255.0)
    base, top = np.meshgrid(k, k, indexing="ij")
    return base.copy(), top.copy()


def fma(a, b, c):
    a, b, c = (np.asarray(x, F) for x in (a, b, c))
    p = a.astype(np.float64) * b.astype(np.float64)          # exact: 24 + 24 significand bits
    c64 = np.broadcast_to(c.astype(np.float64), p.shape)
    s = p + c64
    fin = np.isfinite(s)
    bb = s - p
    err = (p - (s - bb)) + (c64 - bb)                        # TwoSum
    assert not (err[fin] != 0).any(), "the f64 sum is not exact: this model's FMA would round twice"
    return s.astype(F)


def clamp01(x):
    return np.minimum(np.maximum(x, F(0)), F(1))


def bits(x):
    return np.ascontiguousarray(x, dtype=F).view(np.uint32)


def same(a, b, what, where=None):
    a, b = bits(a), bits(b)
    bad = a != b
    if where is not None:
        bad &= where
    assert not bad.any(), f"{what}: {int(bad.sum())} of 65536 pairs differ, first at (base, top) byte {tuple(int(v) for v in np.argwhere(bad)[0])}"


# ---- the reference, canvas_state.rs:1479-1505 and :1425-1431, with the intermediates of the device's select form ----
def vivid_reference(base, top):
    with np.errstate(all="ignore"):
        lo = top <= F(0.5)
        t2 = np.where(lo, F(2) * top, F(2) * (top - F(0.5)))
        n = np.where(lo, F(1) - base, base)
        d = np.where(lo, t2, F(1) - t2)
        q = n / d
        burn = np.where(t2 <= 0, F(0), np.maximum(F(1) - q, F(0)))
        dodge = np.where(t2 >= 1, F(1), np.minimum(q, F(1)))
        return t2, d, n, np.where(lo, burn, dodge).astype(F)


def vivid_short(base, top, edge=np.less_equal):
    with np.errstate(all="ignore"):
        c = np.where(top <= F(0.5), F(0), F(1)).astype(F)
        s = fma(F(-2), c, F(1))
        ic = F(1) - c
        t2 = fma(F(2), top, -c)
        d = fma(s, t2, c)
        n = fma(-s, base, ic)
        q = n / d
        v = clamp01(fma(-s, q, ic))
        return t2, d, n, np.where(edge(d, F(0)), c, v).astype(F)


def test_vivid_light_short_form_and_its_intermediates():
    base, top = _operands()
    rt2, rd, rn, rres = vivid_reference(base, top)
    t2, d, n, res = vivid_short(base, top)
    same(t2, rt2, "t2")
    same(d, rd, "d")
    same(n, rn, "n")
    same(res, rres, "Vivid Light")
    assert np.isfinite(res).all() and (res >= 0).all() and (res <= 1).all()


def test_vivid_light_edge_select_is_looked_at():
    """the two rare sides (t2 <= 0 on the burn arm, t2 >= 1 on the dodge arm) are d == 0: with `d < 0` in the select the form is wrong there, and only there"""
    base, top = _operands()
    rres = vivid_reference(base, top)[3]
    wrong = vivid_short(base, top, edge=np.less)[3]
    bad = bits(wrong) != bits(rres)
    assert bad.any()
    assert set(np.argwhere(bad)[:, 1].tolist()) <= {0, 255}


def test_pin_light_as_a_median():
    """med3(base, fma(2, top, -1), 2 top).  Exact, but not in the kernel: measured and dropped (profiles/r09_tuning.md); kept so that the form's
    exactness is not worked out twice"""
    base, top = _operands()
    ref = np.where(top <= F(0.5), np.minimum(base, F(2) * top), np.maximum(base, F(2) * (top - F(0.5)))).astype(F)
    a, b, c = base, fma(F(2), top, F(-1)), F(2) * top
    med = np.maximum(np.minimum(a, b), np.minimum(np.maximum(a, b), c))
    same(med, ref, "Pin Light")
    # where two of the three are equal the median is that value whichever operand the instruction hands on: no pair has +0.0 meet -0.0
    assert not (np.signbit(a) | np.signbit(c)).any() and not ((b == 0) & np.signbit(b)).any()


def test_overlay_and_hard_light_sign_form():
    """c = (base < 0.5) ? 0 : 1, s = 1 - 2c, fma(s, 2 fma(s, base, c) fma(s, top, c), c).  Exact, measured and dropped like the median above"""
    base, top = _operands()
    ref = np.where(base < F(0.5), F(2) * base * top, F(1) - F(2) * (F(1) - base) * (F(1) - top)).astype(F)
    c = np.where(base < F(0.5), F(0), F(1)).astype(F)
    s = fma(F(-2), c, F(1))
    B, T = fma(s, base, c), fma(s, top, c)
    same(fma(s, F(2) * B * T, c), ref, "Overlay")   # Hard Light is Overlay with the operands exchanged: the same 65 536 pairs
