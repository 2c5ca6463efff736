"""sip_lqr_vjp_multi_columns, sip_lqr_vjp_mats_multi and sip_lqr_vjp_multi without a GPU: the symbols, the header and
the argument checks.

The calls are made in a child process that sees no HIP device (HIP_VISIBLE_DEVICES=-1), on a plan that therefore has
none: a misuse returns SIP_LQR_ERR_INVALID_ARGUMENT before any HIP call, and a well-formed call returns
SIP_LQR_ERR_HIP instead of launching on the made-up pointers -- the same on a host with a GPU and on one without.  The
plan is the fp64 (12, 4, 5) one, whose solve_multi needs a column workspace; a second plan with T = 0 needs no gains."""
import ctypes
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sip_lqr_vjp_multi_columns", "sip_lqr_vjp_mats_multi", "sip_lqr_vjp_multi")
OK, INVALID, ERR_HIP = 0, -1, -3

CHILD = r"""
import ctypes, json, os, sys
sys.path.insert(0, sys.argv[1])
from sip_optimal_control_amd._lib import load_library
lib = load_library()
out = {}
h, h0 = ctypes.c_void_p(), ctypes.c_void_p()
assert lib.sip_lqr_plan_create(0, 6, 5, 12, 4, 0, ctypes.byref(h)) == 0
assert lib.sip_lqr_plan_create(0, 6, 0, 12, 4, 0, ctypes.byref(h0)) == 0
P = ctypes.c_void_p(4096)         # never dereferenced: the plans have no device
N = None
ker = lambda **kw: lib.sip_lqr_vjp_mats_multi(*[kw.get(k, d) for k, d in (
    ("plan", h), ("sol", P), ("adj", P), ("num_rhs", 3), ("wide", 0), ("status", P), ("grad", P), ("stream", N))])
vjp = lambda **kw: lib.sip_lqr_vjp_multi(*[kw.get(k, d) for k, d in (
    ("plan", h), ("mats", P), ("sol", P), ("gsol", P), ("num_rhs", 3), ("gains", P), ("ws", P), ("colws", P),
    ("status", P), ("gvecs", P), ("gmats", P), ("stream", N))])
out["columns"] = {"plan": lib.sip_lqr_vjp_multi_columns(h), "null": lib.sip_lqr_vjp_multi_columns(N)}
out["col_ws_bytes"] = lib.sip_lqr_solve_multi_workspace_bytes(h, 3)
out["kernel_misuse"] = {
    "plan": ker(plan=N), "num_rhs=-1": ker(num_rhs=-1), "sol": ker(sol=N), "adj": ker(adj=N), "grad": ker(grad=N),
    "grad, no columns": ker(grad=N, num_rhs=0), "wide=2": ker(wide=2), "wide=-1": ker(wide=-1)}
out["vjp_misuse"] = {
    "plan": vjp(plan=N), "num_rhs=-1": vjp(num_rhs=-1), "sol": vjp(sol=N), "gsol": vjp(gsol=N), "mats": vjp(mats=N),
    "ws": vjp(ws=N), "gvecs": vjp(gvecs=N), "gvecs, no columns": vjp(gvecs=N, num_rhs=0), "gains": vjp(gains=N),
    "colws": vjp(colws=N)}
# the well-formed calls are made only where the HIP runtime itself reports no device to this process
count, hip = ctypes.c_int(0), None
for name in ("libamdhip64.so", os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so")):
    try:
        hip = ctypes.CDLL(name)
        break
    except OSError:
        pass
out["devices_visible"] = None if hip is None else int(hip.hipGetDeviceCount(ctypes.byref(count)) == 0 and count.value > 0)
if out["devices_visible"] == 0:
    out["deviceless"] = {
        "kernel": ker(), "kernel wide, no status": ker(wide=1, status=N),
        "kernel, no columns, NULL arrays": ker(num_rhs=0, sol=N, adj=N),
        "vjp": vjp(), "vjp, no status, no grad_mats": vjp(status=N, gmats=N),
        "vjp T = 0, no gains": vjp(plan=h0, gains=N)}
lib.sip_lqr_plan_destroy(h)
lib.sip_lqr_plan_destroy(h0)
print("RESULT " + json.dumps(out))
"""


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry
    entry.build_hip()
    from sip_optimal_control_amd._lib import load_library
    return load_library()


@pytest.fixture(scope="module")
def child(lib, tmp_path_factory):
    script = tmp_path_factory.mktemp("vjp_multi_abi") / "child.py"
    script.write_text(CHILD)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    run = subprocess.run([sys.executable, str(script), ROOT], env=env, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    line = [l for l in run.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def test_the_symbols_are_exported_and_bound(lib):
    from sip_optimal_control_amd import _lib
    raw = ctypes.CDLL(_lib.library_path())
    for name in NEW:
        assert hasattr(raw, name), name
        assert name in _lib.EXPORTED_SYMBOLS, name
    sig = _lib._SIGNATURES
    assert sig["sip_lqr_vjp_multi_columns"][0] is ctypes.c_int and len(sig["sip_lqr_vjp_multi_columns"][1]) == 1
    assert sig["sip_lqr_vjp_mats_multi"][0] is ctypes.c_int and len(sig["sip_lqr_vjp_mats_multi"][1]) == 8
    assert sig["sip_lqr_vjp_mats_multi"][1][3] is ctypes.c_int and sig["sip_lqr_vjp_mats_multi"][1][4] is ctypes.c_int
    assert sig["sip_lqr_vjp_multi"][0] is ctypes.c_int and len(sig["sip_lqr_vjp_multi"][1]) == 12
    assert sig["sip_lqr_vjp_multi"][1][4] is ctypes.c_int                                  # num_rhs


def test_the_unit_is_part_of_the_build():
    import __graft_entry__ as entry
    units = {os.path.basename(src): dig for _, src, _, dig in entry.hip_units()}
    assert "chain_vjp_cols.hip" in units
    sources = {os.path.basename(p) for p in entry.hip_sources()}
    assert {"chain_vjp_cols.hip", "chain_vjp_cols.hpp", "vjp_cols_launch.hpp", "vjp_cols_shape.hpp"} <= sources
    assert callable(entry.build_vjp_cols_shape_test)


def test_the_package_offers_them():
    import sip_optimal_control_amd as pkg
    assert callable(pkg.chain_lqr_solve_multi) and "chain_lqr_solve_multi" in pkg.__all__
    for name in ("vjp_multi_columns", "vjp_mats_multi", "vjp_multi"):
        assert hasattr(pkg.BatchedChainLQR, name), name


def test_the_header_declares_them_and_is_plain_c(tmp_path):
    text = open(os.path.join(ROOT, "include", "sip_lqr_amd.h")).read()
    for name in NEW:
        assert name + "(" in text, name
    prose = " ".join(text.replace("\n *", " ").split())
    for stated in ("The accumulate rule: the first group never reads d_grad_mats",
                   "does not depend on the grouping (barring underflow)",
                   "every group boundary costs one rounding to float",
                   "num_rhs = 0 writes an all-zero d_grad_mats",
                   "num_rhs = 1 gives the bits of sip_lqr_vjp_mats",
                   "safe under stream capture"):
        assert stated in prose, stated
    src = tmp_path / "hdr.c"
    src.write_text('#include "sip_lqr_amd.h"\n'
                   "int main(void) {\n"
                   "  int (*c)(const sip_lqr_plan *) = sip_lqr_vjp_multi_columns;\n"
                   "  int (*k)(const sip_lqr_plan *, const void *, const void *, int, int, const int32_t *, void *,\n"
                   "           void *) = sip_lqr_vjp_mats_multi;\n"
                   "  int (*v)(const sip_lqr_plan *, const void *, const void *, const void *, int, void *, void *,\n"
                   "           void *, const int32_t *, void *, void *, void *) = sip_lqr_vjp_multi;\n"
                   "  return c == 0 || k == 0 || v == 0;\n}\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only",
                           "-I", os.path.join(ROOT, "include"), str(src)])


def test_columns_of_a_plan_and_of_none(child):
    assert child["columns"] == {"plan": 8, "null": 0}


def test_every_misuse_is_an_invalid_argument(child):
    assert child["col_ws_bytes"] > 0                   # so that the NULL d_col_workspace below is a misuse on this plan
    for entry in ("kernel_misuse", "vjp_misuse"):
        for what, rc in child[entry].items():
            assert rc == INVALID, (entry, what, rc)
    assert len(child["kernel_misuse"]) == 8 and len(child["vjp_misuse"]) == 10


def test_a_plan_without_a_device_computes_nothing(child):
    assert child["devices_visible"] == 0, "the child process was to see no HIP device"
    for what, rc in child["deviceless"].items():
        assert rc == ERR_HIP, (what, rc)
    assert len(child["deviceless"]) == 6
