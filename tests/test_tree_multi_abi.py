"""The multi-right-hand-side tree solve in the C ABI without a GPU: the symbols are exported and misuse is
rejected before any HIP call."""
import ctypes
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "sip_optimal_control_amd", "lib", "libsip_lqr_amd.so")

SYMBOLS = ("sip_lqr_tree_rhs_len", "sip_lqr_tree_rhs_offset", "sip_lqr_tree_solve_multi_scratch_bytes",
           "sip_lqr_tree_solve_multi", "sip_lqr_tree_multi_kernel_name")


def _lib():
    if not os.path.exists(LIB):
        pytest.skip("library not built")
    try:
        return ctypes.CDLL(LIB)
    except OSError as e:  # the HIP runtime it links against is not loadable here
        pytest.skip(f"cannot load the library: {e}")


def test_symbols_are_exported():
    lib = _lib()
    for name in SYMBOLS:
        assert hasattr(lib, name), name


def test_null_plan_is_rejected_without_hip():
    lib = _lib()
    f = lib.sip_lqr_tree_solve_multi
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_int] + [ctypes.c_void_p] * 3
    assert f(None, None, None, None, None, 3, None, None, None) == -1  # SIP_LQR_ERR_INVALID_ARGUMENT
    lib.sip_lqr_tree_solve_multi_scratch_bytes.restype = ctypes.c_size_t
    lib.sip_lqr_tree_solve_multi_scratch_bytes.argtypes = [ctypes.c_void_p, ctypes.c_int]
    assert lib.sip_lqr_tree_solve_multi_scratch_bytes(None, 3) == 0
    lib.sip_lqr_tree_rhs_offset.restype = ctypes.c_size_t
    lib.sip_lqr_tree_rhs_offset.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    assert lib.sip_lqr_tree_rhs_offset(None, 0, 0) == ctypes.c_size_t(-1).value
    lib.sip_lqr_tree_multi_kernel_name.restype = ctypes.c_char_p
    lib.sip_lqr_tree_multi_kernel_name.argtypes = [ctypes.c_void_p]
    assert lib.sip_lqr_tree_multi_kernel_name(None) == b""
