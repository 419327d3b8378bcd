"""The colour-removal entry points exist in libpfx.so and refuse a NULL context with an error status — checked without a GPU (tests/test_abi_hostile.py sweeps
the same calls from the header; this file names them, so it fails on a library that lacks them)."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["pfx_color_to_alpha_core", "pfx_color_to_alpha_dev", "pfx_color_removal", "pfx_color_removal_dev"]


@pytest.fixture(scope="module")
def lib():
    return C.CDLL(os.environ.get("PFX_LIB_PATH") or os.path.join(ROOT, "paintfe_amd", "libpfx.so"))


@pytest.mark.parametrize("name", ENTRY_POINTS + ["pfx_int_colorkey_last"])
def test_symbol_is_exported(lib, name):
    assert hasattr(lib, name)


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_null_context_is_an_error_status(lib, name):
    from paintfe_amd import _lib
    img = np.zeros((4, 4, 4), np.uint8)
    out = np.zeros_like(img)
    params = _lib.ColorToAlpha() if "alpha" in name else _lib.ColorRemoval()
    fn = getattr(lib, name)
    fn.restype = C.c_int
    st = fn(C.c_void_p(None), img.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), C.c_uint32(4), C.c_uint32(4), C.byref(params), C.c_void_p(None))
    assert st == _lib.ERR_INVALID
    assert not out.any()
    lib.pfx_int_colorkey_last.restype = C.c_int
    assert lib.pfx_int_colorkey_last(C.c_void_p(None), C.c_int(0)) == -1


def test_structs_have_the_header_layout():
    from paintfe_amd import _lib
    assert C.sizeof(_lib.ColorToAlpha) == 32 and _lib.ColorToAlpha.tolerance.offset == 4
    assert C.sizeof(_lib.ColorRemoval) == 20 and _lib.ColorRemoval.contiguous.offset == 16
