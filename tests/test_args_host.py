"""The argument rule every entry point shares (pfx_internal.h: pfx_check_args), through its pure decision function pfx_int_check_args — plain integers in,
the kind and index of the first violation out, nothing dereferenced — against a table written out here from the rule.  No device.

The rule.  An entry point declares its buffers (address, bytes, flags) and at most one `in_place_with` pointer:
  * a buffer that is not OPTIONAL has a non-NULL address;
  * a DWORD buffer's address is a multiple of 4 when the call is a `_dev` call (on a host call the flag is ignored);
  * an OUT buffer shares no byte with any other declared buffer (ranges are half open: end == start is adjacent, not shared) — except that it may start at the
    very address of its in-place partner, the first declared input whose address is `in_place_with`; a NULL buffer and a buffer of 0 bytes (a pointer that is
    only required) share nothing.
Violations are reported NULLs first, then alignment, then overlaps, each in declaration order; an overlap names the OUT buffer and the buffer it overlaps."""
import ctypes as C

import pytest

from paintfe_amd import _lib

IN, OUT, OPTIONAL, DWORD = 0, 1, 2, 4                  # pfx_internal.h: PFX_ARG_*
FINE, IS_NULL, MISALIGNED, OVERLAPS = 0, 1, 2, 3


class ArgCase(C.Structure):   # pfx_internal.h: pfx_arg_case
    _fields_ = [("addr", C.c_uint64), ("bytes", C.c_uint64), ("flags", C.c_int32)]


@pytest.fixture(scope="module")
def check():
    L = _lib.load()
    L.pfx_int_check_args.argtypes = [C.POINTER(ArgCase), C.c_int, C.c_int, C.c_uint64, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.pfx_int_check_args.restype = C.c_int

    def run(bufs, dev=0, in_place_with=0):
        arr = (ArgCase * len(bufs))(*[ArgCase(a, b, f) for a, b, f in bufs])
        which, other = C.c_int(-7), C.c_int(-7)
        kind = L.pfx_int_check_args(arr, len(bufs), dev, in_place_with, C.byref(which), C.byref(other))
        return kind, which.value, other.value
    return run


A, N = 0x10000, 1340          # an address and the bytes of a 67 x 5 RGBA8 image
FINE_ = (FINE, -1, -1)


def test_null_pointers(check):
    assert check([(A, N, IN), (A + 4096, N, OUT)]) == FINE_
    assert check([(0, N, IN), (A, N, OUT)]) == (IS_NULL, 0, -1)                          # a required input
    assert check([(A, N, IN), (0, N, OUT)]) == (IS_NULL, 1, -1)                          # a required output
    assert check([(A, N, IN), (A + 4096, N, OUT), (0, 335, OPTIONAL)]) == FINE_         # an absent mask
    assert check([(A, N, IN), (A + 4096, N, OUT), (0, 0, IN)]) == (IS_NULL, 2, -1)      # a settings pointer that is only required
    assert check([(0, N, IN), (0, N, OUT)]) == (IS_NULL, 0, -1)                          # the first one is named
    assert check([(A + 1, N, DWORD), (0, N, OUT)], dev=1) == (IS_NULL, 1, -1)            # NULLs come before alignment
    assert check([(A, N, IN), (A, N, OUT), (0, N, IN)]) == (IS_NULL, 2, -1)              # ... and before overlaps


# output against input: (name, input start, output start, shares a byte).  Both are N bytes but for "nested", where the output is the inner 100 bytes
LAYOUTS = [("identical", A, A, N, True), ("one byte at the input's end", A, A + N - 1, N, True), ("one byte at the input's start", A, A - N + 1, N, True),
           ("nested", A, A + 200, 100, True), ("adjacent behind", A, A + N, N, False), ("adjacent in front", A, A - N, N, False), ("disjoint", A, A + 3 * N, N, False)]


@pytest.mark.parametrize("name,src,dst,dst_bytes,shared", LAYOUTS, ids=[l[0] for l in LAYOUTS])
@pytest.mark.parametrize("in_place", [False, True])
def test_output_against_input(check, name, src, dst, dst_bytes, shared, in_place):
    allowed = not shared or (in_place and dst == src)        # the same POINTER, nothing else
    want = FINE_ if allowed else (OVERLAPS, 1, 0)
    assert check([(src, N, IN), (dst, dst_bytes, OUT)], in_place_with=src if in_place else 0) == want
    assert check([(dst, dst_bytes, OUT), (src, N, IN)], in_place_with=src if in_place else 0) == (FINE_ if allowed else (OVERLAPS, 0, 1))   # declaration order is free
    # an input that is the outer buffer of a nested pair
    if name == "nested":
        assert check([(dst, dst_bytes, IN), (src, N, OUT)], in_place_with=dst if in_place else 0) == (OVERLAPS, 1, 0)


def test_in_place_is_one_named_pair(check):
    mask = A + 8192
    assert check([(A, N, IN), (A, N, OUT), (mask, 335, OPTIONAL)], in_place_with=A) == FINE_
    assert check([(A, N, IN), (mask, N, OUT), (mask, 335, OPTIONAL)], in_place_with=A) == (OVERLAPS, 1, 2)        # dst == mask is not the in-place pair
    assert check([(A, N, IN), (A, N, OUT), (A, 335, OPTIONAL)], in_place_with=A) == (OVERLAPS, 1, 2)              # one partner: the first input declared there
    assert check([(A, 335, OPTIONAL), (A, N, OUT), (A, N, IN)], in_place_with=A) == (OVERLAPS, 1, 2)
    assert check([(A, N, IN), (A, N, OUT)], in_place_with=A + 4) == (OVERLAPS, 1, 0)                              # some other pointer allows nothing
    assert check([(A, N, IN), (A + 4, N, OUT)], in_place_with=A) == (OVERLAPS, 1, 0)
    assert check([(A, N, IN), (A + 4, N, OUT)], in_place_with=A + 4) == (OVERLAPS, 1, 0)
    assert check([(A, N, IN), (A, N, IN)]) == FINE_                                                               # two inputs may share what they like


def test_output_against_an_optional_input(check):
    src, dst, mask = A, A + 4096, A + 8192
    assert check([(src, N, IN), (dst, N, OUT), (mask, 335, OPTIONAL)]) == FINE_
    assert check([(src, N, IN), (dst, N, OUT), (dst + N - 1, 335, OPTIONAL)]) == (OVERLAPS, 1, 2)
    assert check([(src, N, IN), (dst, N, OUT), (dst - 334, 335, OPTIONAL)]) == (OVERLAPS, 1, 2)
    assert check([(src, N, IN), (dst, N, OUT), (dst + N, 335, OPTIONAL)]) == FINE_
    assert check([(src, N, IN), (dst, N, OUT), (dst, 335, OPTIONAL)], in_place_with=src) == (OVERLAPS, 1, 2)
    assert check([(src, N, IN), (src, N, OUT), (src + 8, 335, OPTIONAL)], in_place_with=src) == (OVERLAPS, 1, 2)   # in place with src, over the mask
    assert check([(dst + 10, 335, OPTIONAL), (dst, N, OUT | DWORD)]) == (OVERLAPS, 1, 0)
    assert check([(dst + 10, 0, IN), (dst, N, OUT)]) == FINE_                                                      # 0 bytes: required, shares nothing
    assert check([(dst, 0, IN), (dst, N, OUT)]) == FINE_


def test_buffers_of_different_sizes(check):
    big, small = 3 * N, N                      # the warps: a 67 x 15 source sampled into a 67 x 5 output
    assert check([(A, big, IN), (A + 2 * N, small, OUT)]) == (OVERLAPS, 1, 0)          # only the source's tail overlaps the output
    assert check([(A, big, IN), (A + big, small, OUT)]) == FINE_                       # behind the source's end
    assert check([(A, big, IN), (A - small, small, OUT)]) == FINE_
    assert check([(A, big, IN), (A - small + 1, small, OUT)]) == (OVERLAPS, 1, 0)
    assert check([(A, small, IN), (A + small, big, OUT)]) == FINE_
    assert check([(A + small, small, IN), (A, big, OUT)]) == (OVERLAPS, 1, 0)          # an output that contains the input


@pytest.mark.parametrize("off", [0, 1, 2, 3])
def test_alignment(check, off):
    bufs = [(A + off, N, DWORD), (A + 4096, N, OUT | DWORD), (A + 8192 + 1, 335, OPTIONAL)]     # the mask is bytes: no flag, any address
    assert check(bufs, dev=0) == FINE_                                                          # a host call ignores the flag
    assert check(bufs, dev=1) == (FINE_ if off == 0 else (MISALIGNED, 0, -1))
    bufs = [(A, N, DWORD), (A + 4096 + off, N, OUT | DWORD)]
    assert check(bufs, dev=0) == FINE_
    assert check(bufs, dev=1) == (FINE_ if off == 0 else (MISALIGNED, 1, -1))
    assert check([(A + off, N, IN), (A + 4096 + off, N, OUT)], dev=1) == FINE_                  # not declared DWORD: not checked
    if off:
        assert check([(A + off, N, DWORD), (A + off, N, OUT | DWORD)], dev=1, in_place_with=A + off) == (MISALIGNED, 0, -1)   # alignment before overlaps
        assert check([(A + off, N, DWORD), (A + off + 4, N, OUT | DWORD)], dev=0) == (OVERLAPS, 1, 0)


def test_no_buffers(check):
    assert check([]) == FINE_
