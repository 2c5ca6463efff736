"""sip_lqr_tree_vjp_kernel_name, sip_lqr_tree_vjp_input, sip_lqr_tree_vjp_scratch_bytes and sip_lqr_tree_vjp without a
GPU: the symbols, the header, the build and the argument checks.

The calls are made in a child process that sees no HIP device (HIP_VISIBLE_DEVICES=-1): a misuse returns
SIP_LQR_ERR_INVALID_ARGUMENT before any HIP call.  A tree plan with a valid topology uploads its tables when it is
created, so it cannot exist in that process (tests/test_tree_refine_abi.py asserts it); a plan with a latched invalid
topology can, and everything is refused on it.  The checks that need a valid plan are in
tests/test_gpu_tree_vjp_solve.py."""
import ctypes
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sip_lqr_tree_vjp_kernel_name", "sip_lqr_tree_vjp_input", "sip_lqr_tree_vjp_scratch_bytes", "sip_lqr_tree_vjp")
OK, INVALID, ERR_HIP = 0, -1, -3

CHILD = r"""
import ctypes, json, os, sys
sys.path.insert(0, sys.argv[1])
from sip_optimal_control_amd._lib import load_library
lib = load_library()
out = {}
ints = lambda v: (ctypes.c_int * len(v))(*v)
P = ctypes.c_void_p(4096)         # never dereferenced: the checks come before any HIP call
N = None
def calls(h):
    ker = lambda **kw: lib.sip_lqr_tree_vjp_input(*[kw.get(k, d) for k, d in (
        ("plan", h), ("output", P), ("adj", P), ("status", P), ("grad", P), ("stream", N))])
    vjp = lambda **kw: lib.sip_lqr_tree_vjp(*[kw.get(k, d) for k, d in (
        ("plan", h), ("input", P), ("work", P), ("output", P), ("gout", P), ("status", P), ("adj", P), ("grad", P),
        ("scratch", P), ("stream", N))])
    return ker, vjp
ker, vjp = calls(None)
out["null_plan"] = {"kernel": ker(), "vjp": vjp(), "bytes": int(lib.sip_lqr_tree_vjp_scratch_bytes(None)),
                    "name": lib.sip_lqr_tree_vjp_kernel_name(None).decode()}
# a cycle: 0 -> 1 -> 0 (latched; the plan exists without a device)
bad = ctypes.c_void_p()
rc = lib.sip_lqr_tree_plan_create(3, 2, 0, ints([0, 1]), ints([1, 0]), ints([2, 2, 2]), ints([1, 1]), 0, ctypes.byref(bad))
out["latched_create"] = [rc, lib.sip_lqr_tree_topology_status(bad)]
ker, vjp = calls(bad)
out["latched"] = {"kernel": ker(), "kernel, no status": ker(status=N), "vjp": vjp(), "vjp, lambda only": vjp(grad=N),
                  "bytes": int(lib.sip_lqr_tree_vjp_scratch_bytes(bad)),
                  "name": lib.sip_lqr_tree_vjp_kernel_name(bad).decode()}
out["misuse_on_latched"] = {
    "kernel output": ker(output=N), "kernel adj": ker(adj=N), "kernel grad": ker(grad=N),
    "vjp input": vjp(input=N), "vjp work": vjp(work=N), "vjp output": vjp(output=N), "vjp gout": vjp(gout=N),
    "vjp status": vjp(status=N), "vjp adj": vjp(adj=N), "vjp scratch": vjp(scratch=N)}
lib.sip_lqr_tree_plan_destroy(bad)
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
    script = tmp_path_factory.mktemp("tree_vjp_abi") / "child.py"
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
    assert sig["sip_lqr_tree_vjp_kernel_name"] == (ctypes.c_char_p, [ctypes.c_void_p])
    assert sig["sip_lqr_tree_vjp_input"][0] is ctypes.c_int and len(sig["sip_lqr_tree_vjp_input"][1]) == 6
    assert sig["sip_lqr_tree_vjp_scratch_bytes"] == (ctypes.c_size_t, [ctypes.c_void_p])
    assert sig["sip_lqr_tree_vjp"][0] is ctypes.c_int and len(sig["sip_lqr_tree_vjp"][1]) == 10


def test_the_python_layers_are_there():
    import sip_optimal_control_amd as pkg
    from sip_optimal_control_amd.tree import BatchedTreeLQR
    assert callable(pkg.tree_lqr_solve) and "tree_lqr_solve" in pkg.__all__
    for name in ("vjp", "vjp_input", "vjp_kernel_name"):
        assert hasattr(BatchedTreeLQR, name), name


def test_the_unit_is_part_of_the_build():
    import __graft_entry__ as entry
    units = {os.path.basename(src): dig for _, src, _, dig in entry.hip_units()}
    assert "tree_vjp.hip" in units
    sources = {os.path.basename(p) for p in entry.hip_sources()}
    assert {"tree_vjp.hip", "tree_vjp.hpp", "tree_vjp_launch.hpp", "tree_vjp_table.hpp"} <= sources
    assert callable(entry.build_tree_vjp_table_test)
    # the unit is rebuilt by each of its headers: its digest is that of the unit, those three and the chain's emit
    csrc = os.path.join(ROOT, "sip_optimal_control_amd", "csrc")
    deps = [os.path.join(csrc, f) for f in ("tree_vjp.hip", "tree_vjp.hpp", "tree_vjp_launch.hpp", "tree_vjp_table.hpp",
                                            "chain_vjp.hpp", "vjp_launch.hpp", "chain_residual.hpp")]
    assert units["tree_vjp.hip"] == entry._digest(deps, entry.HIP_FLAGS)


def test_the_header_declares_them_and_is_plain_c(tmp_path):
    text = open(os.path.join(ROOT, "include", "sip_lqr_amd.h")).read()
    for name in NEW:
        assert name + "(" in text, name
    prose = " ".join(text.replace("\n *", " ").split())
    for stated in ("The gains K | k and the other fields of the work arena are not differentiated",
                   "Gradients through sip_kkt_* are not offered", "No second derivative is offered",
                   "sip_lqr_tree_vjp_scratch_bytes(plan) = sip_lqr_tree_solve_multi_scratch_bytes(plan, 1)",
                   "ly_c[r] x_p[col] + y_c[r] lx_p[col]", "-ly_i[j] y_i[j]"):
        assert stated in prose, stated
    src = tmp_path / "hdr.c"
    src.write_text('#include "sip_lqr_amd.h"\n'
                   "int main(void) {\n"
                   "  const char *(*n)(const sip_lqr_tree_plan *) = sip_lqr_tree_vjp_kernel_name;\n"
                   "  int (*k)(const sip_lqr_tree_plan *, const double *, const double *, const int32_t *, double *,\n"
                   "           void *) = sip_lqr_tree_vjp_input;\n"
                   "  size_t (*b)(const sip_lqr_tree_plan *) = sip_lqr_tree_vjp_scratch_bytes;\n"
                   "  int (*v)(const sip_lqr_tree_plan *, const double *, const double *, const double *, const double *,\n"
                   "           const int32_t *, double *, double *, void *, void *) = sip_lqr_tree_vjp;\n"
                   "  return n == 0 || k == 0 || b == 0 || v == 0;\n}\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only",
                           "-I", os.path.join(ROOT, "include"), str(src)])


def test_a_null_plan_is_refused(child):
    assert child["null_plan"] == {"kernel": INVALID, "vjp": INVALID, "bytes": 0, "name": ""}


def test_a_latched_invalid_topology_is_refused(child):
    assert child["latched_create"] == [OK, 4]                 # the plan exists; SIP_LQR_INVALID_TOPOLOGY is latched
    for what, rc in child["latched"].items():
        assert rc == {"bytes": 0, "name": ""}.get(what, INVALID), (what, rc)
    for what, rc in child["misuse_on_latched"].items():
        assert rc == INVALID, (what, rc)
    assert len(child["misuse_on_latched"]) == 10
