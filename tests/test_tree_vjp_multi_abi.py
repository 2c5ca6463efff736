"""sip_lqr_tree_vjp_multi_columns, sip_lqr_tree_vjp_multi_kernel_name, sip_lqr_tree_vjp_input_multi,
sip_lqr_tree_vjp_multi_scratch_bytes and sip_lqr_tree_vjp_multi without a GPU: the symbols, the header, the build and the
argument checks.

The calls are made in a child process that sees no HIP device (HIP_VISIBLE_DEVICES=-1): a misuse returns
SIP_LQR_ERR_INVALID_ARGUMENT before any HIP call.  A tree plan with a valid topology uploads its tables when it is
created, so it cannot exist in that process; a plan with a latched invalid topology can, and everything is refused on
it.  The checks that need a valid plan are in tests/test_gpu_tree_vjp_multi_solve.py."""
import ctypes
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sip_lqr_tree_vjp_multi_columns", "sip_lqr_tree_vjp_multi_kernel_name", "sip_lqr_tree_vjp_input_multi",
       "sip_lqr_tree_vjp_multi_scratch_bytes", "sip_lqr_tree_vjp_multi")
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
    ker = lambda **kw: lib.sip_lqr_tree_vjp_input_multi(*[kw.get(k, d) for k, d in (
        ("plan", h), ("out", P), ("adj", P), ("num_rhs", 3), ("status", P), ("grad", P), ("stream", N))])
    vjp = lambda **kw: lib.sip_lqr_tree_vjp_multi(*[kw.get(k, d) for k, d in (
        ("plan", h), ("input", P), ("work", P), ("out", P), ("gout", P), ("num_rhs", 3), ("status", P), ("adj", P),
        ("grad", P), ("scratch", P), ("stream", N))])
    return ker, vjp
def facts(h):
    return {"columns": int(lib.sip_lqr_tree_vjp_multi_columns(h)),
            "name": lib.sip_lqr_tree_vjp_multi_kernel_name(h).decode(),
            "bytes": int(lib.sip_lqr_tree_vjp_multi_scratch_bytes(h, 3))}
ker, vjp = calls(None)
out["null_plan"] = dict(facts(None), kernel=ker(), vjp=vjp(), kernel_no_columns=ker(num_rhs=0), vjp_no_columns=vjp(num_rhs=0))
# a cycle: 0 -> 1 -> 0 (latched; the plan exists without a device)
bad = ctypes.c_void_p()
rc = lib.sip_lqr_tree_plan_create(3, 2, 0, ints([0, 1]), ints([1, 0]), ints([2, 2, 2]), ints([1, 1]), 0, ctypes.byref(bad))
out["latched_create"] = [rc, lib.sip_lqr_tree_topology_status(bad)]
ker, vjp = calls(bad)
out["latched"] = dict(facts(bad), kernel=ker(), kernel_no_status=ker(status=N), kernel_no_columns=ker(num_rhs=0),
                      vjp=vjp(), vjp_lambda_only=vjp(grad=N), vjp_no_columns=vjp(num_rhs=0))
out["misuse_on_latched"] = {
    "kernel num_rhs": ker(num_rhs=-1), "kernel out": ker(out=N), "kernel adj": ker(adj=N), "kernel grad": ker(grad=N),
    "kernel grad, no columns": ker(grad=N, num_rhs=0),
    "vjp num_rhs": vjp(num_rhs=-1), "vjp input": vjp(input=N), "vjp work": vjp(work=N), "vjp out": vjp(out=N),
    "vjp gout": vjp(gout=N), "vjp status": vjp(status=N), "vjp adj": vjp(adj=N), "vjp scratch": vjp(scratch=N)}
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
    script = tmp_path_factory.mktemp("tree_vjp_multi_abi") / "child.py"
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
    P, I = ctypes.c_void_p, ctypes.c_int
    assert sig["sip_lqr_tree_vjp_multi_columns"] == (I, [P])
    assert sig["sip_lqr_tree_vjp_multi_kernel_name"] == (ctypes.c_char_p, [P])
    assert sig["sip_lqr_tree_vjp_input_multi"] == (I, [P, P, P, I, P, P, P])
    assert sig["sip_lqr_tree_vjp_multi_scratch_bytes"] == (ctypes.c_size_t, [P, I])
    assert sig["sip_lqr_tree_vjp_multi"] == (I, [P, P, P, P, P, I, P, P, P, P, P])


def test_the_python_layers_are_there():
    import sip_optimal_control_amd as pkg
    from sip_optimal_control_amd.tree import BatchedTreeLQR
    assert callable(pkg.tree_lqr_solve_multi) and "tree_lqr_solve_multi" in pkg.__all__
    for name in ("vjp_multi_columns", "vjp_multi_kernel_name", "vjp_input_multi", "vjp_multi"):
        assert hasattr(BatchedTreeLQR, name), name


def test_the_unit_is_part_of_the_build():
    import __graft_entry__ as entry
    units = {os.path.basename(src): dig for _, src, _, dig in entry.hip_units()}
    assert "tree_vjp_cols.hip" in units
    sources = {os.path.basename(p) for p in entry.hip_sources()}
    assert {"tree_vjp_cols.hip", "tree_vjp_cols.hpp", "tree_vjp_cols_launch.hpp", "tree_vjp_cols_shape.hpp"} <= sources
    assert callable(entry.build_tree_vjp_cols_shape_test)
    # the unit is rebuilt by each of its headers, and by no other: its own three, the one-column launcher's Args, the
    # table's word, and the chain's emit with what that includes
    csrc = os.path.join(ROOT, "sip_optimal_control_amd", "csrc")
    deps = [os.path.join(csrc, f) for f in ("tree_vjp_cols.hip", "tree_vjp_cols.hpp", "tree_vjp_cols_launch.hpp",
                                            "tree_vjp_cols_shape.hpp", "tree_vjp_launch.hpp", "tree_vjp_table.hpp",
                                            "chain_vjp.hpp", "vjp_launch.hpp", "chain_residual.hpp")]
    assert units["tree_vjp_cols.hip"] == entry._digest(deps, entry.HIP_FLAGS)
    # the kernel header is seen by that unit alone: the host code's digest does not move with it
    host = [dig for _, src, _, dig in entry.hip_units() if os.path.basename(src) == "sip_lqr_tree.hip"][0]
    hdrs = [f for f in entry.hip_sources() if f.endswith("tree_vjp_cols.hpp")]
    assert len(hdrs) == 1
    text = open(os.path.join(csrc, "sip_lqr_tree.hip")).read()
    assert '#include "tree_vjp_cols.hpp"' not in text and '#include "tree_vjp_cols_launch.hpp"' in text
    assert host != units["tree_vjp_cols.hip"]
    # tools/lib_objects.py lists what hip_units() lists
    listed = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "lib_objects.py"), "--sources"],
                            capture_output=True, text=True, check=True).stdout.split()
    assert os.path.join("sip_optimal_control_amd", "csrc", "tree_vjp_cols.hip") in listed


def test_the_header_declares_them_and_is_plain_c(tmp_path):
    text = open(os.path.join(ROOT, "include", "sip_lqr_amd.h")).read()
    for name in NEW:
        assert name + "(" in text, name
    prose = " ".join(text.replace("\n *", " ").split())
    for stated in ("THE q, c AND r SLOTS OF d_grad_input ARE WRITTEN +0.0",
                   "dL/db_c is lambda_c itself",
                   "One column therefore gives the bits of sip_lqr_tree_vjp_input on every other entry",
                   "the result does not depend on the grouping (barring underflow in the halving)",
                   "0 writes an all-zero gradient",
                   "SIP_LQR_TREE_VJP_MULTI_COLUMNS=<1..8>",
                   "sip_lqr_tree_solve_multi_scratch_bytes(plan, num_rhs)",
                   "safe under stream capture"):
        assert stated in prose, stated
    src = tmp_path / "hdr.c"
    src.write_text('#include "sip_lqr_amd.h"\n'
                   "int main(void) {\n"
                   "  int (*c)(const sip_lqr_tree_plan *) = sip_lqr_tree_vjp_multi_columns;\n"
                   "  const char *(*n)(const sip_lqr_tree_plan *) = sip_lqr_tree_vjp_multi_kernel_name;\n"
                   "  int (*k)(const sip_lqr_tree_plan *, const double *, const double *, int, const int32_t *, double *,\n"
                   "           void *) = sip_lqr_tree_vjp_input_multi;\n"
                   "  size_t (*b)(const sip_lqr_tree_plan *, int) = sip_lqr_tree_vjp_multi_scratch_bytes;\n"
                   "  int (*v)(const sip_lqr_tree_plan *, const double *, const double *, const double *, const double *,\n"
                   "           int, const int32_t *, double *, double *, void *, void *) = sip_lqr_tree_vjp_multi;\n"
                   "  return c == 0 || n == 0 || k == 0 || b == 0 || v == 0;\n}\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only",
                           "-I", os.path.join(ROOT, "include"), str(src)])


def test_a_null_plan_is_refused(child):
    assert child["null_plan"] == {"columns": 0, "name": "", "bytes": 0, "kernel": INVALID, "vjp": INVALID,
                                  "kernel_no_columns": INVALID, "vjp_no_columns": INVALID}


def test_a_latched_invalid_topology_is_refused(child):
    assert child["latched_create"] == [OK, 4]                 # the plan exists; SIP_LQR_INVALID_TOPOLOGY is latched
    for what, rc in child["latched"].items():
        assert rc == {"columns": 0, "bytes": 0, "name": ""}.get(what, INVALID), (what, rc)
    assert len(child["latched"]) == 9
    for what, rc in child["misuse_on_latched"].items():
        assert rc == INVALID, (what, rc)
    assert len(child["misuse_on_latched"]) == 13
