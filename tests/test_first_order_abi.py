"""The first-order gather (sip_kkt_first_order_len, sip_kkt_first_order_offset, sip_kkt_gather_first_order) in the C
ABI without a GPU: the symbols are exported with the signatures of include/sip_kkt_amd.h, misuse is rejected before
any HIP call, and the header is still plain C99."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "sip_optimal_control_amd", "lib", "libsip_lqr_amd.so")
HEADER = os.path.join(ROOT, "include", "sip_kkt_amd.h")
INVALID_ARGUMENT = -1  # SIP_LQR_ERR_INVALID_ARGUMENT

# name -> (return type, parameter types) as the header must declare them
DECLARED = {
    "sip_kkt_first_order_len": ("size_t", ["const sip_kkt_plan *"]),
    "sip_kkt_first_order_offset": ("size_t", ["const sip_kkt_plan *", "int", "int"]),
    "sip_kkt_gather_first_order": ("int", ["const sip_kkt_plan *", "const double *", "const double *", "const double *",
                                           "double *", "double *", "double *", "double *", "void *"]),
}
BLOCKS = ("NODE_F", "NODE_DF_DX", "NODE_DF_DTHETA", "NODE_C", "NODE_G", "EDGE_F", "EDGE_DF_DX", "EDGE_DF_DU",
          "EDGE_DF_DTHETA", "EDGE_DYN_RES", "EDGE_C", "EDGE_G", "NUM_BLOCKS")


def _lib():
    if not os.path.exists(LIB):
        pytest.skip("library not built")
    try:
        return ctypes.CDLL(LIB)
    except OSError as e:  # the HIP runtime it links against is not loadable here
        pytest.skip(f"cannot load the library: {e}")


def test_symbols_are_exported():
    lib = _lib()
    for name in DECLARED:
        assert hasattr(lib, name), name


def test_header_declares_the_stated_signatures():
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    for name, (ret, params) in DECLARED.items():
        m = re.search(r"(\w[\w \*]*?)\b" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, name
        assert m.group(1).strip() == ret, (name, m.group(1))
        got = [re.sub(r"\s*\w+$", "", " ".join(a.split())) for a in m.group(2).split(",")]  # drop the parameter names
        assert got == params, (name, got)


def test_binding_mirrors_the_header():
    from sip_optimal_control_amd import _lib as binding
    sig = binding._SIGNATURES
    assert sig["sip_kkt_first_order_len"] == (ctypes.c_size_t, [ctypes.c_void_p])
    assert sig["sip_kkt_first_order_offset"] == (ctypes.c_size_t, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int])
    assert sig["sip_kkt_gather_first_order"] == (ctypes.c_int, [ctypes.c_void_p] * 9)
    from sip_optimal_control_amd import kkt
    assert len(kkt.FIRST_ORDER_NODE_BLOCKS) + len(kkt.FIRST_ORDER_EDGE_BLOCKS) == len(BLOCKS) - 1
    for attr in ("first_order_offset", "gather_first_order"):
        assert callable(getattr(kkt.BatchedNewtonKKT, attr))


def test_null_plans_are_rejected_without_hip():
    lib = _lib()
    length = lib.sip_kkt_first_order_len
    length.restype, length.argtypes = ctypes.c_size_t, [ctypes.c_void_p]
    assert length(None) == 0
    offset = lib.sip_kkt_first_order_offset
    offset.restype, offset.argtypes = ctypes.c_size_t, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    for block, index in ((0, 0), (5, 0), (-1, 0), (12, 0), (0, -1)):
        assert offset(None, block, index) == ctypes.c_size_t(-1).value
    gather = lib.sip_kkt_gather_first_order
    gather.restype, gather.argtypes = ctypes.c_int, [ctypes.c_void_p] * 9
    assert gather(*[None] * 9) == INVALID_ARGUMENT
    dummy = ctypes.c_void_p(16)  # never dereferenced: the plan is checked first
    assert gather(None, dummy, dummy, dummy, dummy, dummy, dummy, dummy, None) == INVALID_ARGUMENT
    assert gather(None, dummy, None, None, dummy, None, None, None, None) == INVALID_ARGUMENT


def test_header_is_plain_c_and_numbers_the_blocks_in_arena_order(tmp_path):
    """C99 next to sip_lqr_amd.h; the enum follows the arena: node blocks 0..4, edge blocks 5..11."""
    checks = "".join("typedef char check_%s[SIP_KKT_FO_%s == %d ? 1 : -1];\n" % (b.lower(), b, k)
                     for k, b in enumerate(BLOCKS))
    src = tmp_path / "first_order.c"
    src.write_text('#include "sip_lqr_amd.h"\n#include "sip_kkt_amd.h"\n' + checks +
                   "int main(void) {\n"
                   "  size_t (*len)(const sip_kkt_plan *) = sip_kkt_first_order_len;\n"
                   "  size_t (*off)(const sip_kkt_plan *, int, int) = sip_kkt_first_order_offset;\n"
                   "  int (*gather)(const sip_kkt_plan *, const double *, const double *, const double *, double *,\n"
                   "                double *, double *, double *, void *) = sip_kkt_gather_first_order;\n"
                   "  return len == 0 || off == 0 || gather == 0;\n}\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only",
                           "-I", os.path.join(ROOT, "include"), str(src)])
