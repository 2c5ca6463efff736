"""The split factor / solve of trees (sip_lqr_tree_factor_fused, sip_lqr_tree_solve_fused) and the Newton-KKT switch
onto them in the C ABI without a GPU: the symbols are exported and misuse is rejected before any HIP call."""
import ctypes
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "sip_optimal_control_amd", "lib", "libsip_lqr_amd.so")

SYMBOLS = ("sip_lqr_tree_factor_fused", "sip_lqr_tree_solve_fused", "sip_lqr_tree_split_kernel_name",
           "sip_kkt_plan_set_tree_fused")


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


def test_null_plans_and_pointers_are_rejected_without_hip():
    lib = _lib()
    f = lib.sip_lqr_tree_factor_fused
    f.restype, f.argtypes = ctypes.c_int, [ctypes.c_void_p] * 6
    assert f(None, None, None, None, None, None) == -1  # SIP_LQR_ERR_INVALID_ARGUMENT
    dummy = ctypes.c_void_p(16)                          # never dereferenced: the plan is checked first
    assert f(None, dummy, dummy, dummy, dummy, None) == -1
    g = lib.sip_lqr_tree_solve_fused
    g.restype, g.argtypes = ctypes.c_int, [ctypes.c_void_p] * 7
    assert g(None, None, None, None, None, None, None) == -1
    assert g(None, dummy, dummy, dummy, dummy, dummy, None) == -1
    lib.sip_lqr_tree_split_kernel_name.restype = ctypes.c_char_p
    lib.sip_lqr_tree_split_kernel_name.argtypes = [ctypes.c_void_p]
    assert lib.sip_lqr_tree_split_kernel_name(None) == b""
    k = lib.sip_kkt_plan_set_tree_fused
    k.restype, k.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]
    assert k(None, 1) == -1 and k(None, 0) == -1
